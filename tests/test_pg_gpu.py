"""GPU parity of the pose-graph optimisation (GlobalMapper::GlobalBA, /root/reference/src/GlobalMapper.cpp:328-535; k4_*
kernels in csrc/ba.hip on the SE3 model's reduce / dataflow solve / device LM controller) against oracle/pg_ref.cpp.
Cost and pose updates within 1e-5 relative (BASELINE north_star's BA tolerance)."""
import numpy as np
import pytest

import scaled_parity as sp
from ba_cases import REL, pg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [12, 60, 200])
def test_system_and_chi2_match_oracle(oracle, synth, P):
    from se2lam_amd import optimizer as op
    g = synth.pose_graph(P)
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
        sp.close(H, b, Hr, br, tol, (P, lam))                 # in the system's own scale (tests/scaled_parity.py)


@pytest.mark.parametrize("P", [12, 60, 200])
def test_global_ba_matches_oracle(oracle, synth, P):
    """optimize(GLOBAL_ITER) on all key frames: LM history, poses, per-edge chi2 (the feature-edge rejection rule)."""
    from se2lam_amd import optimizer as op
    g = synth.pose_graph(P)
    o = pg(g)
    assert o.optimize(10) == 10
    X, ec, st = oracle.pg_optimize(g, 10)
    s = o.stats
    assert s["trials_hist"] == st["trials_hist"]
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    upd = np.abs(X - g.poses).max()
    for a in range(g.P):
        T = op.estimateVertexSE3(o, a)
        assert np.abs(T - X[a]).max() <= REL * upd
    assert np.array_equal(op.estimateVertexSE3(o, 0), g.poses[0])
    ec_gpu = op.edgeChi2(o, g.O)
    assert np.allclose(ec_gpu, ec, rtol=1e-4, atol=1e-7)
    other = np.nonzero((ec_gpu > 30.0) != (ec > 30.0))[0]                   # threshFeatEdgeChi2: at most one edge may fall on the
    assert len(other) <= 1                                                  # other side, and only one that sits on the threshold
    assert all(abs(ec[k] - 30.0) <= 1e-4 * 30.0 for k in other), (other, ec[other], ec_gpu[other])


def test_parallel_edges_and_graph_type_errors(synth):
    from se2lam_amd import capi, optimizer as op
    g = synth.pose_graph(12)
    # both an odometry and a feature edge between consecutive key frames exist in the generated graph
    pairs = [tuple(sorted((int(a), int(b)))) for a, b in zip(g.o_i, g.o_j)]
    assert len(set(pairs)) < len(pairs)
    o = op.SlamOptimizer()
    op.addVertexSE3(o, np.eye(4), 0, True)
    with pytest.raises(capi.Se2GpuError):
        op.addVertexSE3Expmap(o, np.eye(4), 1)               # one pose type per graph
    with pytest.raises(capi.Se2GpuError):
        op.addVertexSBAXYZ(o, [0, 0, 1.0], 5) or op.addVertexSE3(o, np.eye(4), 6)   # no landmarks in a pose graph


def test_reinitialise_over_the_level_0_edges(oracle, synth):
    """GlobalMapper::GlobalBA with PRE_REJECT_FTR_OUTLIER (GlobalMapper.cpp:421-483): feature edges above the chi2 threshold are
    moved to level 1 and the same optimizer is initialised and optimised AGAIN - from the estimates of the first run, over the
    remaining edges.  Against the oracle run on the graph without those edges, started from the first run's poses."""
    import copy
    from se2lam_amd import capi, optimizer as op
    g = copy.copy(synth.pose_graph(60))
    g.o_meas = g.o_meas.copy()
    bad = [7, 40, 111]                                  # three EdgeSE3 that claim another 0.8 m along the optical axis
    for k in bad:
        g.o_meas[k] = g.o_meas[k].copy()
        g.o_meas[k][2, 3] += 800.0
    o = pg(g)
    o.optimize(8)
    ec = op.edgeChi2(o, g.O)
    out = np.nonzero(ec > 30.0)[0]
    assert set(bad) <= set(out.tolist())
    first = np.stack([op.estimateVertexSE3(o, a) for a in range(g.P)])
    for k in out:
        capi.check(capi.lib().se2gpu_ba_set_edge_level(o._h, int(k), 1))
    o.initializeOptimization(0)                          # second initialise: allowed for the pose graph
    o.optimize(8)
    keep = np.setdiff1d(np.arange(g.O), out)
    g2 = copy.copy(g)
    g2.o_i, g2.o_j, g2.o_meas, g2.o_info = g.o_i[keep], g.o_j[keep], g.o_meas[keep], g.o_info[keep]
    g2.poses = first
    X, ec2, st = oracle.pg_optimize(g2, 8)
    assert o.stats["trials_hist"] == st["trials_hist"]
    assert np.allclose(o.stats["chi2_hist"], st["chi2_hist"], rtol=REL)
    upd = max(np.abs(X - first).max(), 1e-9)
    for a in range(g.P):
        assert np.abs(op.estimateVertexSE3(o, a) - X[a]).max() <= REL * max(upd, 1.0)
    got = op.edgeChi2(o, g.O)
    assert np.all(got[out] == 0.0) and np.allclose(got[keep], ec2, rtol=1e-4, atol=1e-7)
    # the landmark models still refuse a second initialise instead of silently optimising over everything
    s = op.SlamOptimizer()
    s.load(synth.ba_graph(8, 60))
    s.initializeOptimization(0)
    with pytest.raises(capi.Se2GpuError):
        s.initializeOptimization(0)
