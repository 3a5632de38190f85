"""CPU tests of the SE3-expmap bundle-adjustment restatement (oracle/ba3_ref.cpp) against things
that are not the restatement: a numpy / scipy model of the cost, numeric derivatives of the edge functions through
exp(update) * estimate, the full (un-reduced) normal equations, and the structure LocalMapper::removeOutlierChi2 relies on."""
import numpy as np
import pytest

from se2lam_amd import synth as _synth            # (the parametrisations below; tests take the `synth` fixture)
from ba_cases import assert_topology3, odo_graph3, odometry_cases3
from independent import BA3ProblemNumpy, ba3_full_normal_equations, se3_log_g2o


@pytest.mark.parametrize("P,L,n_ref", [(8, 60, 0), (21, 800, 0), (21, 800, 4)])
def test_cost_equals_the_numpy_model(oracle, synth, P, L, n_ref):
    g = synth.ba3_graph(P, L, n_ref)
    m = BA3ProblemNumpy(g)
    c0, ec = oracle.ba3_chi2(g)
    # 1e-7, not round-off: SE3Quat::log switches to the first-order form omega = (R - R')^v / 2 below 4.5 mrad (relative
    # error theta^2 / 6 <= 3e-6 of a prior / odometry residual); the numpy model takes the exact logarithm
    assert c0 == pytest.approx(m.cost(g.poses, g.lms), rel=1e-7)
    assert np.allclose(ec, m.edge_chi2, rtol=1e-10)
    p, l, ec2, st = oracle.ba3_optimize(g, 10)
    assert st["chi2_final"] == pytest.approx(m.cost(p, l), rel=1e-7)
    assert np.allclose(ec2, m.edge_chi2, rtol=1e-8)
    assert st["chi2_final"] < 0.5 * st["chi2_init"]
    # fixed vertices (the oldest local key frame, or the reference key frames) do not move
    for a in np.nonzero(g.fixed)[0]:
        assert np.array_equal(p[a], g.poses[a])
    # the plane-motion priors pull the out-of-plane errors of the start back: body height and roll / pitch shrink
    Tbc = np.eye(4); Tbc[:3, :3] = synth.RBC; Tbc[:3, 3] = synth.TBC
    def out_of_plane(T):
        Twb = np.linalg.inv(Tbc @ T)
        return abs(Twb[2, 3]), np.hypot(Twb[2, 0], Twb[2, 1])
    free = np.nonzero(g.fixed == 0)[0]
    z0 = np.mean([out_of_plane(g.poses[a])[0] for a in free]); z1 = np.mean([out_of_plane(p[a])[0] for a in free])
    assert z1 < 0.5 * z0


def test_edge_jacobians_against_numeric_derivatives(oracle, synth):
    """EdgeSE3Expmap: d log(T_j^-1 C exp(d) T_i) / d d = adj(T_j^-1 C) exactly at zero error (checked numerically through
    exp(update) * estimate); away from zero error g2o keeps that first-order form (it drops the inverse left Jacobian),
    so there the Jacobians are checked against their definition adj(T_j^-1 C), -adj(T_i^-1 C^-1) in numpy."""
    g = synth.ba3_graph(8, 60)
    Ti, Tj = g.poses[2], g.poses[3]
    Cm = Tj @ np.linalg.inv(Ti)
    e, Ji, Jj = oracle.ba3_odo_edge(Ti, Tj, Cm)
    assert np.abs(e).max() < 1e-9
    h = 1e-6
    for c in range(6):
        d = np.zeros(6); d[c] = h
        ei = (oracle.ba3_odo_edge(synth.se3_exp_np(d) @ Ti, Tj, Cm)[0] - oracle.ba3_odo_edge(synth.se3_exp_np(-d) @ Ti, Tj, Cm)[0]) / (2 * h)
        ej = (oracle.ba3_odo_edge(Ti, synth.se3_exp_np(d) @ Tj, Cm)[0] - oracle.ba3_odo_edge(Ti, synth.se3_exp_np(-d) @ Tj, Cm)[0]) / (2 * h)
        assert np.allclose(Ji[:, c], ei, atol=1e-5 * max(1.0, np.abs(ei).max()))
        assert np.allclose(Jj[:, c], ej, atol=1e-5 * max(1.0, np.abs(ej).max()))
    Cm = g.o_meas[2]
    e, Ji, Jj = oracle.ba3_odo_edge(Ti, Tj, Cm)
    assert np.allclose(e, synth.se3_log_np(np.linalg.inv(Tj) @ Cm @ Ti), rtol=1e-5, atol=1e-9)
    assert np.allclose(Ji, synth.se3_adj_np(np.linalg.inv(Tj) @ Cm), rtol=1e-9, atol=1e-9)
    assert np.allclose(Jj, -synth.se3_adj_np(np.linalg.inv(Ti) @ np.linalg.inv(Cm)), rtol=1e-9, atol=1e-9)


def test_schur_system_solves_the_full_normal_equations(oracle, synth):
    """The reduced (6P) system's solution is the pose part of the full Gauss-Newton step: checked through the cost
    decrease of one undamped step reproduced with a dense numeric Gauss-Newton on the numpy model (small graph)."""
    g = synth.ba3_graph(8, 60)
    S, bs = oracle.ba3_reduced_system(g, 0.0)
    n = 6 * g.P
    assert np.abs(S - S.T).max() <= 1e-9 * np.abs(S).max()
    free = np.repeat(g.fixed == 0, 6)
    assert np.array_equal(S[~free][:, ~free], np.eye((~free).sum()))
    ev = np.linalg.eigvalsh(S[free][:, free])
    assert ev.min() > 0
    xp = np.linalg.solve(S, bs)
    assert np.abs(xp[~free]).max() == 0
    # the step decreases the independent cost (with the landmarks re-optimised by LM on the oracle side)
    m = BA3ProblemNumpy(g)
    _, _, _, st = oracle.ba3_optimize(g, 1)
    assert st["chi2_hist"][0] < m.cost(g.poses, g.lms)


def test_remove_outlier_chi2_rule(oracle, synth):
    """LocalMapper::removeOutlierChi2 (LocalMapper.cpp:172-230): after optimize(10) the edges with chi2() > 25 are the
    gross outliers the generator planted (and few others)."""
    g = synth.ba3_graph(21, 800)
    p, l, ec, st = oracle.ba3_optimize(g, 10)
    bad = ec > 25
    assert 0 < bad.sum() < 0.06 * g.E
    assert np.median(ec[~bad]) < 3.0


# ---- SE3 windows beyond ba3_graph's chain (synth.odometry_topology3; the cases and their shape checks: tests/ba_cases.py) ----
def _refined_solve(A, b):
    """A x = b by LU with three rounds of refinement on an extended-precision residual: what is left between two such solutions is
    the difference of the two systems, not the rounding of either solve"""
    from scipy.linalg import lu_factor, lu_solve
    lu = lu_factor(A)
    x = lu_solve(lu, b).astype(np.longdouble)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(3):
        x = x + lu_solve(lu, (bl - Al @ x).astype(np.float64))
    return x.astype(np.float64)


def _reduced_system_equals_full_model3(oracle, g, lam):
    """oracle.ba3_reduced_system against the Schur complement of independent.ba3_full_normal_equations (fixed rows and columns
    deleted).  The numpy model restates the small-angle branch of SE3Quat::log (independent.se3_log_g2o) rather than taking the
    exact logarithm, so b and the solution are held to the same 1e-9 as S and no theta^2 / 6 term enters.
    Largest differences seen (x86-64 CPU, every case of test_odometry_topologies3_reduce_like_the_full_model):
    S 7.3e-14 of max|S|, b 4.7e-14 of max|b|, solution 4.7e-12 of max|x| (both solves refined, _refined_solve).  -> the model's (S, b) over the free poses"""
    S, bs = oracle.ba3_reduced_system(g, lam)
    P, L = g.P, g.L
    assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max()
    fp = np.repeat(np.asarray(g.fixed) == 0, 6)
    assert np.array_equal(S[~fp][:, ~fp], np.eye((~fp).sum())) and not S[~fp][:, fp].any() and not S[fp][:, ~fp].any()
    assert not bs[~fp].any()
    H, b = ba3_full_normal_equations(g, lam)
    free = np.r_[fp, np.ones(3 * L, bool)]
    Hf, bf = H[np.ix_(free, free)], b[free]
    nf = int(fp.sum())
    Hll_inv_Hlp = np.linalg.solve(Hf[nf:, nf:], np.c_[Hf[nf:, :nf], bf[nf:]])
    Sm = Hf[:nf, :nf] - Hf[:nf, nf:] @ Hll_inv_Hlp[:, :nf]
    bm = bf[:nf] - Hf[:nf, nf:] @ Hll_inv_Hlp[:, nf]
    dS = np.abs(S[np.ix_(fp, fp)] - Sm).max() / np.abs(Sm).max()
    db = np.abs(bs[fp] - bm).max() / np.abs(bm).max()
    x_full = _refined_solve(Hf, bf)[:nf]                      # the pose part of the full step, not through the Schur complement
    x_red = _refined_solve(S, bs)
    dx = np.abs(x_red[fp] - x_full).max() / np.abs(x_full).max()
    print("full model: P %d O %d lam %g  dS %.2e  db %.2e  dx %.2e" % (P, g.O, lam, dS, db, dx))
    assert dS <= 1e-9 and db <= 1e-9 and dx <= 1e-9, (dS, db, dx)
    assert not x_red[~fp].any()
    return Sm, bm, fp


FULL_MODEL_SIZES = ((8, 60, 0), (21, 800, 0), (21, 800, 4), (30, 600, 0))     # (30, 600): the smallest window `dense` fits


@pytest.mark.parametrize("P,L,n_ref,kind", [(8, 60, 0, "chain"), (21, 800, 4, "chain")]
                         + [c for c in odometry_cases3(_synth, FULL_MODEL_SIZES)
                            if c[0] != 30 or c[3] == "dense"])
def test_odometry_topologies3_reduce_like_the_full_model(oracle, synth, P, L, n_ref, kind):
    """The oracle's reduced system (ba3_ref.cpp) against an independent assembly of the full normal equations, on the chain and
    on every topology the GPU tests use.  A transposed cross block of a reversed edge, a dropped odometry-only block, a prior or
    an odometry term on the wrong side of a fixed pose: all show here with no GPU involved."""
    g = odo_graph3(synth, P, L, n_ref, kind)
    for lam in (0.0, 2.5):
        Sm, bm, fp = _reduced_system_equals_full_model3(oracle, g, lam)
    S, _ = oracle.ba3_reduced_system(g, 0.0)
    # blocks that only an odometry edge fills (the key frames share no landmark) are there, each held to its own size - a dropped
    # or transposed block cannot hide behind the bound on the whole matrix
    cov = synth.covisible(g)
    slot = np.cumsum(np.asarray(g.fixed) == 0) - 1
    lonely = [(int(i), int(j)) for i, j in zip(g.o_i, g.o_j) if not cov[i, j] and not g.fixed[i] and not g.fixed[j]]
    if kind in ("long", "dense"):
        assert len(lonely) >= 1
    for i, j in lonely:
        B = S[6 * i:6 * i + 6, 6 * j:6 * j + 6]
        Bm = Sm[6 * slot[i]:6 * slot[i] + 6, 6 * slot[j]:6 * slot[j] + 6]
        assert np.abs(B).max() > 0 and np.abs(B - Bm).max() <= 1e-9 * np.abs(Bm).max(), (i, j)
        assert np.abs(B - B.T).max() > 1e-3 * np.abs(B).max()          # (not symmetric: its transpose is a different matrix)
        assert np.array_equal(S[6 * j:6 * j + 6, 6 * i:6 * i + 6], B.T)


def test_flipped_odometry_edge_jacobians_against_numeric_derivatives(oracle, synth):
    """test_edge_jacobians_against_numeric_derivatives on an edge stored as (k + 1, k): vertex 0 is the LATER key frame, the
    measurement is inverted to match (true_k true_{k+1}^-1), and at zero error J_i, J_j are the central differences through
    exp(update) * estimate"""
    g = synth.odometry_topology3(synth.ba3_graph(8, 60), "reversed")
    k = int(np.nonzero(g.o_i > g.o_j)[0][0])
    i, j = int(g.o_i[k]), int(g.o_j[k])
    assert i == j + 1
    # the stored measurement takes vertex 0 to vertex 1 (noise only at the true poses): C = T_j T_i^-1, not its inverse
    e_true = synth.se3_log_np(np.linalg.inv(g.poses_true[j]) @ g.o_meas[k] @ g.poses_true[i])
    assert np.abs(e_true[:3]).max() < 0.02 and np.abs(e_true[3:]).max() < 20.0
    Ti, Tj = g.poses[i], g.poses[j]
    Cm = Tj @ np.linalg.inv(Ti)
    e, Ji, Jj = oracle.ba3_odo_edge(Ti, Tj, Cm)
    assert np.abs(e).max() < 1e-9
    h = 1e-6
    for c in range(6):
        d = np.zeros(6); d[c] = h
        ei = (oracle.ba3_odo_edge(synth.se3_exp_np(d) @ Ti, Tj, Cm)[0] - oracle.ba3_odo_edge(synth.se3_exp_np(-d) @ Ti, Tj, Cm)[0]) / (2 * h)
        ej = (oracle.ba3_odo_edge(Ti, synth.se3_exp_np(d) @ Tj, Cm)[0] - oracle.ba3_odo_edge(Ti, synth.se3_exp_np(-d) @ Tj, Cm)[0]) / (2 * h)
        assert np.allclose(Ji[:, c], ei, atol=1e-5 * max(1.0, np.abs(ei).max()))
        assert np.allclose(Jj[:, c], ej, atol=1e-5 * max(1.0, np.abs(ej).max()))
    e, Ji, Jj = oracle.ba3_odo_edge(Ti, Tj, g.o_meas[k])
    assert np.allclose(Ji, synth.se3_adj_np(np.linalg.inv(Tj) @ g.o_meas[k]), rtol=1e-9, atol=1e-9)
    assert np.allclose(Jj, -synth.se3_adj_np(np.linalg.inv(Ti) @ np.linalg.inv(g.o_meas[k])), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("P,L,n_ref,kind", odometry_cases3(_synth,
                                                          ((8, 60, 0), (21, 800, 0), (21, 800, 4))))
def test_cost_equals_the_numpy_model_on_odometry_topologies(oracle, synth, P, L, n_ref, kind):
    """test_cost_equals_the_numpy_model's cost checks on the other odometry and prior layouts (BA3ProblemNumpy takes any o_i, o_j)"""
    g = odo_graph3(synth, P, L, n_ref, kind)
    # with the exact logarithm the two costs differ by up to theta^2 / 3 <= 6.8e-6 of the prior and odometry terms (the file's 1e-7
    # of the whole cost is what the chain gives, and a window without odometry misses it: 1.6e-7).  Here the model restates
    # g2o's first-order branch instead (independent.se3_log_g2o), so only rounding is left: 1e-11 covers sums of ~1e4 terms in
    # doubles; the largest difference seen on an x86-64 CPU is 9.1e-15
    m = BA3ProblemNumpy(g, log=se3_log_g2o)
    c0, ec = oracle.ba3_chi2(g)
    c_np = m.cost(g.poses, g.lms)
    print("cost %s %s: oracle / numpy - 1 = %.2e" % ((P, L, n_ref), kind, c0 / c_np - 1))
    assert c0 == pytest.approx(c_np, rel=1e-11)
    assert np.allclose(ec, m.edge_chi2, rtol=1e-10)
    p, l, ec2, st = oracle.ba3_optimize(g, 10)
    assert st["chi2_final"] == pytest.approx(m.cost(p, l), rel=1e-11)
    assert np.allclose(ec2, m.edge_chi2, rtol=1e-8)
    assert st["chi2_final"] < st["chi2_init"]
    for a in np.nonzero(g.fixed)[0]:
        assert np.array_equal(p[a], g.poses[a])


BA3_GRAPH_SHA256 = {   # of ba3_graph's arrays before odometry_topology3 existed (_digest3 below)
    (8, 60, 0): "c29a9169fe88d7fa0bd2e0b9668e11aa84062a19e0ed4ae8b1c29f476bdae891",
    (21, 800, 4): "bf6df5696de741849b042a7f2b6fc69b2da1f432bc23f30826b3c03056c8aa4b",
    (50, 5000, 10): "904a358ef7887e1ed2319bc2cdc45509407430b61d289647cb75febf87e63338",
}


def _digest3(g):
    import hashlib
    h = hashlib.sha256()
    for f in ("poses", "fixed", "lms", "e_kf", "e_lm", "e_uv", "e_w", "has_prior", "prior_meas", "prior_info", "o_i", "o_j", "o_meas",
              "o_info"):
        a = np.ascontiguousarray(getattr(g, f))
        h.update(f.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    h.update(repr((g.fx, g.cx, g.cy, g.huber)).encode())
    return h.hexdigest()


def test_odometry_topology3_generator_leaves_ba3_graph_alone(synth):
    """ba3_graph's output (the fixtures' and the fuzzers' windows) is what it was before the generator of other layouts was added,
    to the bit, also after that generator ran on the cached instance; every generated edge agrees with the ground truth"""
    for key, want in BA3_GRAPH_SHA256.items():
        g = synth.ba3_graph(*key)
        assert _digest3(g) == want, key
        kinds = [c[3] for c in odometry_cases3(synth, (key,))]
        made = [synth.odometry_topology3(g, kind) for kind in kinds]
        assert _digest3(g) == want and synth.ba3_graph(*key) is g, key
        for kind, h in zip(kinds, made):
            assert_topology3(synth, h, kind, g)
            assert h.poses is g.poses and h.lms is g.lms and h.e_uv is g.e_uv
            for k in range(0, h.O, max(1, h.O // 40)):
                # C = noise true_j true_i^-1: what is left of C true_i true_j^-1 is the noise, six terms of known deviation
                e = synth.se3_log_np(h.o_meas[k] @ h.poses_true[h.o_i[k]] @ np.linalg.inv(h.poses_true[h.o_j[k]]))
                assert np.abs(e / np.array([1e-3, 1e-3, 2e-3, 2.0, 2.0, 2.0])).max() < 6.0, (key, kind, k)
    # the chain through with_odometry3: ba3_graph's pairs, measurements of the same distribution (not the same draws)
    g = synth.ba3_graph(21, 800, 4)
    c = synth.with_odometry3(g, np.c_[g.o_i, g.o_j], seed=5)
    assert np.array_equal(c.o_i, g.o_i) and np.array_equal(c.o_j, g.o_j) and not np.array_equal(c.o_meas, g.o_meas)
    assert np.abs(c.o_meas - g.o_meas)[:, :3, 3].max() < 30.0 and np.abs(c.o_meas - g.o_meas)[:, :3, :3].max() < 0.02
    with pytest.raises(ValueError):
        synth.odometry_topology3(synth.ba3_graph(21, 800, 0), "dense")       # 210 pairs: fewer than DENSE_TERMS - 21
    with pytest.raises(ValueError):
        synth.odometry_topology3(synth.ba3_graph(21, 800, 0), "to_reference")
