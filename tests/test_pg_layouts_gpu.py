"""The pose-graph kernels of csrc/ba.hip (k6_terms / k6_oplus / k6_finalize<PoseGraph>, PoseGraph::slot_terms and prior_terms, the
slot plan and pg_perm) on the graphs of tests/pg_cases.py: layouts the ring of synth.pose_graph never has (fixed key frames other
than 0, slots of three and four edges in both orientations, key frames without a prior, shuffled insertion order) and starts on
which Levenberg-Marquardt rejects trials (the `retry` branch, the estimate swap, trial_decide with rho < 0) - against
oracle/pg_ref.cpp at the tolerances of tests/test_pg_gpu.py, and against the numpy / scipy model of tests/pg_model.py, which
shares no formula with either.

Sizes: the dense solve (k_chol_tiles / k_chol_step) works on block columns of 32; 6 P = 18 lies inside one, 36 straddles the
first boundary, 102 straddles later ones; P = 2 is one free key frame, one slot, a one-block solve.  P = 40 once, for `complete`.

Every bound is an existing one: 1e-11 / (1e-9, 1e-12) / 1e-10 / REL = 1e-5 / (1e-4, 1e-7) from tests/test_pg_gpu.py, 1e-9 on
the cost against the model from tests/test_pg_oracle.py, and the model-to-oracle distances of profiles/pg_layouts.md."""
import dataclasses

import numpy as np
import pytest

import pg_cases
import pg_model
import scaled_parity as sp
from ba_cases import REL, opt, opt3, pg
from pg_cases import recorded, recorded_scaled

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 6, 17)
CASES = [(k, P) for P in SIZES for k in pg_cases.kinds_at(P)] + [("complete", 40)]
REJECTING = pg_cases.REJECTING
_ids = lambda c: "P%d-nbad%d-seed%d" % c


def _poses(o, g):
    from se2lam_amd import optimizer as op
    return np.stack([op.estimateVertexSE3(o, a) for a in range(g.P)])


_ORACLE_RUNS = {}


def _oracle_run(oracle, key, g, iters=10):
    """oracle.pg_optimize of a case, computed once and shared"""
    if key not in _ORACLE_RUNS:
        _ORACLE_RUNS[key] = oracle.pg_optimize(g, iters)
    return _ORACLE_RUNS[key]


def _same_run_as_the_oracle(o, g, ref):
    """the assertions of test_pg_gpu.py::test_global_ba_matches_oracle, with every fixed key frame held to the bit"""
    from se2lam_amd import optimizer as op
    X, ec, st = ref
    s = o.stats
    print("trials", s["trials_hist"], "oracle", st["trials_hist"])
    assert s["trials_hist"] == st["trials_hist"]
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    upd = np.abs(X - g.poses).max()
    got = _poses(o, g)
    print("poses: max |gpu - oracle| %.3e, largest update %.3e" % (np.abs(got - X).max(), upd))
    assert np.abs(got - X).max() <= REL * upd
    for a in np.nonzero(g.fixed)[0]:
        assert np.array_equal(got[a], g.poses[a])
    assert np.allclose(op.edgeChi2(o, g.O), ec, rtol=1e-4, atol=1e-7)
    return got


@pytest.mark.parametrize("kind,P", CASES)
def test_cost_and_system_match_the_oracle_and_the_model(oracle, kind, P):
    from se2lam_amd import optimizer as op
    g = pg_cases.layout(kind, P)
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
        sp.close(H, b, Hr, br, tol, (kind, P, lam))           # in the system's own scale (tests/scaled_parity.py)
    # independent of the oracle: the cost, and the normal equations within (model-to-oracle distance on record) + (the oracle
    # tolerance above) of the model's - the triangle inequality, no other number
    assert o.activeRobustChi2() == pytest.approx(pg_model.cost(g, g.poses)[0], rel=1e-9)
    H, b = o.reduced_system(0.0)
    dH, db = pg_model.distance(g, H, b, *pg_model.system(g, g.poses))
    bH, bb = recorded()[(kind, P)]
    print(f"{kind} P={P}: |H - H_model| / max {dH:.2e} (bound {bH:.0e} + 1e-10), |b - b_model| / max {db:.2e} ({bb:.0e} + 1e-10)")
    assert dH <= bH + 1e-10 and db <= bb + 1e-10
    # the same triangle in the system's own scale: (model-to-oracle scaled distance on record) + (the scaled oracle tolerance)
    sH, sb = pg_model.scaled_distance(g, H, b, *pg_model.system(g, g.poses))
    cH, cb = recorded_scaled()[(kind, P)]
    print(f"{kind} P={P}: scaled {sH:.2e} (bound {cH:.0e} + {tol:.1e}), {sb:.2e} ({cb:.0e} + {tol:.1e})")
    assert sH <= cH + tol and sb <= cb + tol


@pytest.mark.parametrize("kind,P", CASES)
def test_optimize_matches_the_oracle_and_the_model(oracle, kind, P):
    g = pg_cases.layout(kind, P)
    o = pg(g)
    assert o.optimize(10) == 10
    got = _same_run_as_the_oracle(o, g, _oracle_run(oracle, (kind, P), g))
    assert o.stats["chi2_init"] == pytest.approx(pg_model.cost(g, g.poses)[0], rel=1e-9)
    assert o.stats["chi2_final"] == pytest.approx(pg_model.cost(g, got)[0], rel=1e-9)
    assert o.activeRobustChi2() == pytest.approx(pg_model.cost(g, got)[0], rel=1e-9)


@pytest.mark.parametrize("case", REJECTING, ids=_ids)
def test_rejected_trials_match_the_oracle_and_the_model(oracle, case):
    g = pg_cases.rejecting(*case)
    o = pg(g)
    o.optimize(10)
    assert max(o.stats["trials_hist"]) > 1, o.stats["trials_hist"]
    got = _same_run_as_the_oracle(o, g, _oracle_run(oracle, case, g))
    assert o.stats["chi2_init"] == pytest.approx(pg_model.cost(g, g.poses)[0], rel=1e-9)
    assert o.stats["chi2_final"] == pytest.approx(pg_model.cost(g, got)[0], rel=1e-9)


@pytest.mark.parametrize("case", REJECTING, ids=_ids)
def test_rejected_trials_synchronous_controller_and_graph_replay(case):
    """setVerbose(True) - the host decides every trial - gives the asynchronous run's histories to the bit; reset_estimates() +
    optimize(10) four times over gives the same record and estimates each time (from the third call of a shape on the captured
    graph is replayed, and the rejected trials are enqueued after it)."""
    g = pg_cases.rejecting(*case)
    a = pg(g)
    a.optimize(10)
    first, est = a.stats, a.estimates()[0].copy()
    assert max(first["trials_hist"]) > 1, first["trials_hist"]
    v = pg(g)
    v.setVerbose(True)
    v.optimize(10)
    assert v.stats["trials_hist"] == first["trials_hist"]
    assert v.stats["chi2_hist"] == first["chi2_hist"] and v.stats["lambda_hist"] == first["lambda_hist"]
    assert np.array_equal(v.estimates()[0], est)
    for rep in range(4):
        a.reset_estimates()
        a.optimize(10)
        assert a.stats == first, (rep, a.stats, first)
        assert np.array_equal(a.estimates()[0], est), rep


def test_edge_levels_on_multi_edge_slots(oracle):
    """GlobalBA's second pass (tests/test_pg_gpu.py::test_reinitialise_over_the_level_0_edges) where the slot plan has to change:
    one edge of a two-edge slot leaves, a whole slot leaves, and a free key frame with a prior loses every edge."""
    from se2lam_amd import capi, optimizer as op
    P = 17
    g = pg_cases.layout("slots", P)
    key = [(int(min(a, b)), int(max(a, b))) for a, b in zip(g.o_i, g.o_j)]
    assert key.count((1, 2)) == 2 and key.count((3, 4)) == 2
    lone = 10
    assert g.has_prior[lone] and not g.fixed[lone]
    out = [key.index((1, 2))] + [k for k in range(g.O) if key[k] == (3, 4)] + [k for k in range(g.O) if lone in key[k]]
    out = np.unique(out)
    o = pg(g)
    o.optimize(8)
    first = _poses(o, g)
    for k in out:
        capi.check(capi.lib().se2gpu_ba_set_edge_level(o._h, int(k), 1))
    o.initializeOptimization(0)
    o.optimize(8)
    g2, keep = pg_cases.without_edges(g, out)
    g2 = dataclasses.replace(g2, poses=first)
    X, ec2, st = oracle.pg_optimize(g2, 8)
    print("trials", o.stats["trials_hist"], "oracle", st["trials_hist"])
    assert o.stats["trials_hist"] == st["trials_hist"]
    assert np.allclose(o.stats["chi2_hist"], st["chi2_hist"], rtol=REL)
    upd = max(np.abs(X - first).max(), 1e-9)
    err = np.abs(_poses(o, g) - X).max()
    print("poses: max |gpu - oracle| %.3e, largest update %.3e" % (err, upd))
    assert err <= REL * max(upd, 1.0)
    got = op.edgeChi2(o, g.O)
    assert np.all(got[out] == 0.0) and np.allclose(got[keep], ec2, rtol=1e-4, atol=1e-7)
    assert o.stats["chi2_final"] == pytest.approx(pg_model.cost(g2, _poses(o, g))[0], rel=1e-9)


def _one_by_one(make, g):
    o = make(g)
    o.optimize(10)
    return o.stats, [e.copy() for e in o.estimates()]


def test_pose_graphs_inside_optimize_batch(synth):
    """All nine layouts at P = 6 and both rejecting starts in one se2gpu_ba_optimize_batch (a pose graph has no landmarks, so the
    call takes the per-stream path: eleven handles on two enqueue threads), then mixed with an SE(2) and an SE3-expmap window:
    every handle's record and estimates equal its own optimize() to the bit."""
    from se2lam_amd import capi
    from se2lam_amd.optimizer import optimize_batch
    graphs = [(pg, pg_cases.layout(k, 6)) for k in pg_cases.KINDS] + [(pg, pg_cases.rejecting(*c)) for c in REJECTING]
    assert len(graphs) == 11
    refs = [_one_by_one(make, g) for make, g in graphs]
    assert max(refs[-1][0]["trials_hist"]) > 1 and max(refs[-2][0]["trials_hist"]) > 1
    opts = [make(g) for make, g in graphs]
    optimize_batch(opts, 10)
    assert int(capi.lib().se2gpu_ba_last_batch_path()) == 0
    for o, (st, est) in zip(opts, refs):
        assert o.stats == st
        assert all(np.array_equal(x, y) for x, y in zip(o.estimates(), est))
    mixed = graphs[:5] + [(opt, synth.ba_graph(8, 60))] + graphs[5:] + [(opt3, synth.ba3_graph(8, 60, 0))]
    refs = refs[:5] + [_one_by_one(*mixed[5])] + refs[5:] + [_one_by_one(*mixed[-1])]
    opts = [make(g) for make, g in mixed]
    optimize_batch(opts, 10)
    for o, (st, est) in zip(opts, refs):
        assert o.stats == st
        assert all(np.array_equal(x, y) for x, y in zip(o.estimates(), est))
