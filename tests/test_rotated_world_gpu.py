"""The 6-DoF kernels (pose graph: k4_*; SE3-expmap: k3_* and the resident csrc/ba_window3.hip) on problems whose world was moved by
a general rigid motion (tests/world_cases.py): every vertex rotation is a full 3x3 matrix without a zero, the key frames of every
case take all four branches of the matrix-to-quaternion conversion (asserted on the CPU in test_rotated_world.py).  Two kinds of
check, at the bounds of test_pg_gpu.py, test_ba3_gpu.py and test_ba_window_se3_gpu.py:
  - the moved problem against the oracle on the same moved problem: cost, reduced system, 10 iterations;
  - equivariance, which needs no oracle: the device's run on the moved problem, moved back, against its run on the original.
And one pose graph whose headings cross +-pi (world_cases.seam_ring), against the oracle and pg_model."""
import numpy as np
import pytest

import pg_model
import scaled_parity as sp
import world_cases as wc
from ba_cases import REL, env, multi_launch, opt3, pg

pytestmark = pytest.mark.gpu
RTOL = 1e-9          # test_ba_window_se3_gpu.py: the resident path against the multi-launch one

_RUNS = {}


def _pg_poses(o, g):
    from se2lam_amd import optimizer as op
    return np.stack([op.estimateVertexSE3(o, a) for a in range(g.P)])


def _pg_run(name, moved):
    """one 10-iteration device run of a pose-graph case, shared by the tests that look at it: (graph, stats, poses, edge chi2)"""
    from se2lam_amd import optimizer as op
    key = ("pg", name, moved)
    if key not in _RUNS:
        g = wc.pg_case(name)
        g = wc.move_pose_graph(g) if moved else g
        o = pg(g)
        o.optimize(10)
        _RUNS[key] = (g, o.stats, _pg_poses(o, g), op.edgeChi2(o, g.O))
    return _RUNS[key]


def _ba3_run(name, moved):
    """one 10-iteration multi-launch run of an SE3 window: (graph, (stats, (poses12, lms), edge chi2))"""
    key = ("ba3", name, moved)
    if key not in _RUNS:
        g = wc.ba3_case(name)
        g = wc.move_ba3(g) if moved else g
        _RUNS[key] = (g, multi_launch(g, 10, make=opt3))
    return _RUNS[key]


# ---- pose graph ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.PG_CASES)
def test_moved_pose_graph_cost_and_system_match_the_oracle(oracle, name):
    from se2lam_amd import optimizer as op
    g = wc.move_pose_graph(wc.pg_case(name))
    o = pg(g)
    c, ec = oracle.pg_chi2(g)
    assert o.activeRobustChi2() == pytest.approx(c, rel=1e-11)
    assert np.allclose(op.edgeChi2(o, g.O), ec, rtol=1e-9, atol=1e-12)
    tol = sp.bound(oracle.pg_system(g, 0.0)[0])
    for lam in (0.0, 0.7):
        H, b = o.reduced_system(lam)
        Hr, br = oracle.pg_system(g, lam)
        assert np.abs(H - Hr).max() <= 1e-10 * np.abs(Hr).max()
        assert np.abs(b - br).max() <= 1e-10 * np.abs(br).max()
        sp.close(H, b, Hr, br, tol, ("pose graph", g.P, lam))   # in the system's own scale (tests/scaled_parity.py)
    assert o.activeRobustChi2() == pytest.approx(pg_model.cost(g, g.poses)[0], rel=1e-9)


@pytest.mark.parametrize("name", wc.PG_CASES)
def test_moved_pose_graph_run_matches_the_oracle(oracle, name):
    g, s, got, ec_gpu = _pg_run(name, True)
    X, ec, st = oracle.pg_optimize(g, 10)
    print("trials", s["trials_hist"], "oracle", st["trials_hist"])
    assert s["trials_hist"] == st["trials_hist"]
    if name == "rejecting":
        assert max(s["trials_hist"]) > 1
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    upd = np.abs(X - g.poses).max()
    print("poses: max |gpu - oracle| %.3e, largest update %.3e" % (np.abs(got - X).max(), upd))
    assert np.abs(got - X).max() <= REL * upd
    assert np.array_equal(got[0], g.poses[0])
    assert np.allclose(ec_gpu, ec, rtol=1e-4, atol=1e-7)
    assert s["chi2_final"] == pytest.approx(pg_model.cost(g, got)[0], rel=1e-9)


@pytest.mark.parametrize("name", wc.PG_CASES)
def test_pose_graph_run_is_equivariant(name):
    g, s0, X0, _ = _pg_run(name, False)
    _, s1, X1, _ = _pg_run(name, True)
    assert s1["trials_hist"] == s0["trials_hist"]
    assert np.allclose(s1["chi2_hist"], s0["chi2_hist"], rtol=REL, atol=0)
    upd = np.abs(X0 - g.poses).max()
    d = np.abs(wc.pose_graph_back(X1) - X0).max()
    print("moved back: max |difference| %.3e, largest update %.3e" % (d, upd))
    assert d <= REL * upd


def test_seam_ring_matches_the_oracle_and_the_model(oracle):
    from se2lam_amd import optimizer as op
    g, _ = wc.seam_ring()
    o = pg(g)
    c, ec = oracle.pg_chi2(g)
    assert o.activeRobustChi2() == pytest.approx(c, rel=1e-11)
    assert o.activeRobustChi2() == pytest.approx(pg_model.cost(g, g.poses)[0], rel=1e-9)
    assert np.allclose(op.edgeChi2(o, g.O), ec, rtol=1e-9, atol=1e-12)
    tol = sp.bound(oracle.pg_system(g, 0.0)[0])
    for lam in (0.0, 0.7):
        H, b = o.reduced_system(lam)
        Hr, br = oracle.pg_system(g, lam)
        assert np.abs(H - Hr).max() <= 1e-10 * np.abs(Hr).max()
        assert np.abs(b - br).max() <= 1e-10 * np.abs(br).max()
        sp.close(H, b, Hr, br, tol, ("pose graph", g.P, lam))   # in the system's own scale (tests/scaled_parity.py)
    assert o.optimize(10) == 10
    X, ec, st = oracle.pg_optimize(g, 10)
    s, got = o.stats, _pg_poses(o, g)
    assert s["trials_hist"] == st["trials_hist"]
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    assert np.abs(got - X).max() <= REL * np.abs(X - g.poses).max()
    assert s["chi2_final"] == pytest.approx(pg_model.cost(g, got)[0], rel=1e-9)


# ---- SE3-expmap windows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.BA3_CASES)
def test_moved_se3_window_cost_and_system_match_the_oracle(oracle, name):
    from se2lam_amd import optimizer as op
    g = wc.move_ba3(wc.ba3_case(name))
    o = opt3(g)
    c_ref, ec_ref = oracle.ba3_chi2(g)
    assert o.activeRobustChi2() == pytest.approx(c_ref, rel=1e-11)
    assert np.allclose(op.edgeChi2(o, g.E), ec_ref, rtol=1e-10)
    tol = sp.bound(oracle.ba3_reduced_system(g, 0.0)[0])
    for lam in (0.0, 2.5):
        S, bs = o.reduced_system(lam)
        Sr, br = oracle.ba3_reduced_system(g, lam)
        assert np.abs(S - Sr).max() <= 1e-10 * np.abs(Sr).max()
        assert np.abs(bs - br).max() <= 1e-10 * np.abs(br).max()
        sp.close(S, bs, Sr, br, tol, (name, lam))


@pytest.mark.parametrize("name", wc.BA3_CASES)
def test_moved_se3_window_run_matches_the_oracle(oracle, name):
    g, (s, (poses, lms), ec) = _ba3_run(name, True)
    p_ref, l_ref, ec_ref, st = oracle.ba3_optimize(g, 10)
    print("trials", s["trials_hist"], "oracle", st["trials_hist"])
    assert s["trials_hist"] == st["trials_hist"]
    if name == "reject":
        assert max(s["trials_hist"]) > 1
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    assert s["chi2_init"] == pytest.approx(st["chi2_init"], rel=1e-11)
    T = wc.pose44(poses)
    assert np.abs(T - p_ref).max() <= max(REL * np.abs(p_ref - g.poses).max(), 1e-9)
    f = np.asarray(g.fixed, bool)
    assert np.allclose(T[f], g.poses[f], atol=1e-12)
    assert np.abs(lms - l_ref).max() <= REL * np.abs(l_ref - g.lms).max()
    assert np.allclose(ec, ec_ref, rtol=1e-4, atol=1e-6)
    assert ((ec > 25) != (ec_ref > 25)).sum() <= 1e-3 * g.E


@pytest.mark.parametrize("name", wc.BA3_CASES)
def test_se3_window_run_is_equivariant(name):
    g, (s0, (p0, l0), _) = _ba3_run(name, False)
    _, (s1, (p1, l1), _) = _ba3_run(name, True)
    assert s1["trials_hist"] == s0["trials_hist"]
    assert np.allclose(s1["chi2_hist"], s0["chi2_hist"], rtol=REL, atol=0)
    T0 = wc.pose44(p0)
    Tb, lb = wc.ba3_back(wc.pose44(p1), l1)
    dp, dl = np.abs(Tb - T0).max(), np.abs(lb - l0).max()
    up, ul = np.abs(T0 - g.poses).max(), np.abs(l0 - g.lms).max()
    print("moved back: poses %.3e (largest update %.3e), landmarks %.3e (%.3e)" % (dp, up, dl, ul))
    assert dp <= REL * up and dl <= REL * ul


def test_moved_se3_windows_on_the_resident_path(oracle):
    """the three moved windows in one forced-resident batch (csrc/ba_window3.hip): against their multi-launch runs with the
    assertions of test_ba_window_se3_gpu.py::_same, and against the oracle as test_forced_se3_batch_equals_multi_launch_and_the_oracle"""
    from se2lam_amd import capi
    from se2lam_amd import optimizer as op
    runs = [_ba3_run(name, True) for name in wc.BA3_CASES]
    opts = [opt3(g) for g, _ in runs]
    with env(SE2GPU_BA_RESIDENT="1"):
        its = op.optimize_batch(opts, 10)
    assert int(capi.lib().se2gpu_ba_last_batch_path()) == 2
    for (g, (st, est, ec)), o, n in zip(runs, opts, its):
        what = (g.P, g.L)
        assert n == st["iterations"] == o.stats["iterations"] and o.stats["trials"] == st["trials"], what
        assert o.stats["trials_hist"] == st["trials_hist"], (what, o.stats["trials_hist"], st["trials_hist"])
        assert o.stats["terminated"] == st["terminated"] and o.stats["stopped"] == st["stopped"], what
        assert np.isclose(o.stats["chi2_init"], st["chi2_init"], rtol=RTOL), what
        assert np.allclose(o.stats["chi2_hist"][:n], st["chi2_hist"][:n], rtol=RTOL), what
        assert np.allclose(o.stats["lambda_hist"][:n], st["lambda_hist"][:n], rtol=1e-7), what
        p, l = o.estimates()
        assert np.allclose(p, est[0], rtol=1e-9, atol=1e-9) and np.allclose(l, est[1], rtol=1e-9, atol=1e-7), what
        fixed = np.asarray(g.fixed, bool)
        assert np.array_equal(p[fixed], est[0][fixed]), what
        got = op.edgeChi2(o, g.E)
        assert np.allclose(got, ec, rtol=1e-6, atol=1e-9), what
        assert np.array_equal(got > 25, ec > 25), what
        _, _, _, ost = oracle.ba3_optimize(g, 10)
        assert o.stats["trials_hist"] == ost["trials_hist"], what
        assert np.allclose(o.stats["chi2_hist"][:10], ost["chi2_hist"][:10], rtol=1e-7), what
