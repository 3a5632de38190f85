"""tests/feat_edge_model.py, the yardstick of the GPU feature-constraint stage (GlobalMapper::CreateFeatEdge's two-key-frame
bundle adjustment), held to the definitions: its cost, its Jacobians through the vertex updates, its convergence."""
import numpy as np
import pytest

import feat_edge_cases as fc
import feat_edge_model as fm


def _problem(N, seed, mode, **kw):
    c = fc.make_pair(N, seed, **kw)
    return c, fm.Problem(c["kf"], c["mp"], c["z"], c["info"], mode)


@pytest.mark.parametrize("mode", [fm.COVIS, fm.MATCH])
def test_cost_at_the_start_is_the_definitional_cost(synth, mode):
    c, pb = _problem(17, 3, mode, n_outliers=3)
    want, over = 0.0, 0
    for j in range(17):
        for k in range(2):
            T = c["kf"][k]
            e = T[:3, :3].T @ (c["mp"][j] - T[:3, 3]) - c["z"][j, k]
            e2 = e @ c["info"][j, k] @ e
            over += e2 > 5.99 ** 2
            want += e2 if e2 <= 5.99 ** 2 else 2 * np.sqrt(e2) * 5.99 - 5.99 ** 2
    for k in range(2):      # the prior is built from the input pose: both key frames, fixed or not
        Z, W = synth.plane_motion_prior_se3_np(c["kf"][k])
        e = synth.mqt_np(np.linalg.inv(Z) @ c["kf"][k])
        want += e @ W @ e
    assert over > 0, "no edge in the Huber tail: the case does not test the robust cost"
    assert np.isclose(pb.cost(pb.kf0, pb.mp0), want, rtol=1e-12, atol=0)


def _central(f, n, h):
    J = []
    for i in range(n):
        d = np.zeros(n)
        d[i] = h
        J.append((f(d) - f(-d)) / (2 * h))
    return np.stack(J, axis=-1)


def test_edge_and_prior_jacobians_equal_central_differences(synth):
    c, pb = _problem(6, 5, fm.MATCH)
    for j in range(6):
        for k in range(2):
            T, p, z = c["kf"][k], c["mp"][j], c["z"][j, k]
            Jp, Jl = fm.edge_jacobians(T, p)
            Np = _central(lambda d: fm.edge_error(fm.oplus_pose(T, d), p, z), 6, 1e-6)
            Nl = _central(lambda d: fm.edge_error(T, p + d, z), 3, 1e-3)
            assert np.abs(Jp - Np).max() <= 2e-6 * np.abs(Np).max()
            assert np.abs(Jl - Nl).max() <= 2e-6 * np.abs(Nl).max()
    rng = np.random.default_rng(9)
    for k in range(2):
        Z = pb.prior[k][0]
        T = c["kf"][k] @ synth.from_mqt_np(rng.normal(0, 1, 6) * np.array([50, 50, 50, 0.2, 0.2, 0.2]))   # a large error: w_E well below 1
        J = fm.prior_jacobian(Z, T)
        Nj = _central(lambda d: fm.prior_error(Z, fm.oplus_pose(T, d)), 6, 1e-6)
        assert np.abs(J - Nj).max() <= 2e-6 * np.abs(Nj).max()


@pytest.mark.parametrize("mode", [fm.COVIS, fm.MATCH])
def test_b_is_minus_half_the_cost_gradient(mode):
    c, pb = _problem(5, 8, mode, n_outliers=2)
    _, b = pb.system(pb.kf0, pb.mp0)
    free = pb.free()

    def cost(x):
        return np.array([pb.cost(*pb.apply(pb.kf0, pb.mp0, x))])

    n = len(b)
    g = np.zeros(n)
    for i in np.flatnonzero(free):
        d = np.zeros(n)
        d[i] = 1e-6 if i < 12 else 1e-3
        g[i] = (cost(d)[0] - cost(-d)[0]) / (2 * d[i])
    assert np.abs(b[free] + 0.5 * g[free]).max() <= 2e-6 * np.abs(b[free]).max()


@pytest.mark.parametrize("mode,N,seed", [(fm.MATCH, n, s) for n, s in fc.MATCH_SHAPES] + [(fm.COVIS, n, s) for n, s in fc.COVIS_SHAPES])
def test_converges_from_the_perturbed_start(mode, N, seed):
    c, pb = _problem(N, seed, mode)
    r = fm.optimize(pb, 30 if mode == fm.MATCH else 15)
    assert r["chi2_hist"][-1] < 0.1 * r["chi2_init"]
    assert fm.compared_prefix(r["chi2_init"], r["chi2_hist"]) >= 10
    if mode == fm.MATCH:    # the outlier mask is compared exactly on the GPU: nothing at the threshold
        assert np.abs(r["edge_chi2"] - 5.0).min() > 1e-3 * 5.0


@pytest.mark.parametrize("N,seed,planted", fc.OUTLIER_CASES)
def test_planted_outliers_are_rejected(N, seed, planted):
    c, pb = _problem(N, seed, fm.MATCH, n_outliers=planted)
    r = fm.optimize(pb, 30)
    assert c["planted"].sum() == planted and r["chi2_hist"][-1] < r["chi2_init"]
    assert np.all(r["outlier"][c["planted"]])
    assert np.abs(r["edge_chi2"] - 5.0).min() > 1e-3 * 5.0
    assert fm.compared_prefix(r["chi2_init"], r["chi2_hist"]) >= 10


def test_the_turned_start_rejects_trials_while_chi2_still_falls():
    q = fc.REJECTING
    c, pb = _problem(q["N"], q["seed"], fm.COVIS, turn_y=q["turn_y"])
    r = fm.optimize(pb, q["iters"])
    n = fm.compared_prefix(r["chi2_init"], r["chi2_hist"])
    assert n >= 10 and (r["trials_hist"][:n] >= 2).any() and r["chi2_hist"][-1] < r["chi2_init"]
    assert np.array_equal(r["kf"][0], c["kf"][0])       # the fixed key frame is never touched


def test_too_few_iterations_do_not_converge():
    """why the GPU tests run the reference's own 15 / 30 iterations"""
    c, pb = _problem(40, 0, fm.MATCH)
    r8, r30 = fm.optimize(pb, 8), fm.optimize(pb, 30)
    assert r8["chi2_hist"][-1] > 2 * r30["chi2_hist"][-1]
