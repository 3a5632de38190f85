"""The SE(2) bundle adjustment with a camera that is off the body's axes and off the image centre (synth.OFF_AXIS_TBC,
OFF_CENTRE_CAM; tests/off_axis_cases.py).  Under RBC six of the nine entries of Rcb are zero, and every term of se2xyz<JAC>
(csrc/ba_device.h), edge_se2xyz (csrc/ba_window.hip) and k_edge_information that they multiply vanishes from every number the
suite compares; here none does (test_off_axis.py shows the difference on the independent model).  The assertions and bounds are
those of test_ba_gpu.py, test_independent_pin.py and test_ba_window_gpu.py."""
import numpy as np
import pytest

import off_axis_cases as oa
import scaled_parity as sp
from ba_cases import REL, _info_inputs, env, multi_launch, opt, pose_update_close
from independent import BAProblemNumpy

pytestmark = pytest.mark.gpu
RTOL = 1e-9      # test_ba_window_gpu.py

_ORACLE = {}


def _oracle_run(oracle, key, g):
    if key not in _ORACLE:
        _ORACLE[key] = oracle.ba_optimize(g, 10, 0)
    return _ORACLE[key]


@pytest.mark.parametrize("P,L", oa.SIZES)
def test_chi2_matches_oracle_and_the_independent_cost(oracle, P, L):
    """activeRobustChi2 at the start, at the truth and at a rejecting start (large residuals: the Huber branch of most edges).  The
    SE(2) model has no per-edge chi2 call (se2gpu_ba_edge_chi2 takes the 6-DoF models only), so the cost at three states stands
    in for it."""
    import dataclasses
    g = oa.graph(P, L)
    far = oa.kidnapped(*[c for c, _ in oa.REJECT_CASES if c[:2] == (P, L)][0])
    for q in (g, dataclasses.replace(g, poses=g.poses_true.copy(), lms=g.lms_true.copy()), far):
        o = opt(q)
        assert o.activeRobustChi2() == pytest.approx(oracle.ba_chi2(q), rel=1e-12)
        assert o.activeRobustChi2() == pytest.approx(BAProblemNumpy(q).cost(q.poses, q.lms), rel=1e-9)


@pytest.mark.parametrize("P,L", oa.SIZES)
def test_reduced_system_matches_oracle(oracle, P, L):
    g = oa.graph(P, L)
    o = opt(g)
    for lam in (0.0, 3.0):
        S, bs = o.reduced_system(lam)
        ref = oracle.ba_reduced_system(g, lam)
        scale = np.abs(ref["S"]).max()
        assert np.abs(S - ref["S"]).max() <= 1e-11 * scale
        assert np.abs(bs - ref["bs"]).max() <= 1e-11 * np.abs(ref["bs"]).max()
        assert np.abs(S - S.T).max() <= 1e-12 * scale
        sp.close(S, bs, ref["S"], ref["bs"], sp.bound(oracle.ba_reduced_system(g, 0.0)["S"]), (P, L, lam))   # tests/scaled_parity.py


@pytest.mark.parametrize("P,L", oa.SIZES)
def test_lm_10_iterations_match_oracle_and_the_independent_cost(oracle, P, L):
    g = oa.graph(P, L)
    o = opt(g)
    assert o.optimize(10) == 10
    p_ref, l_ref, st = _oracle_run(oracle, (P, L), g)
    s = o.stats
    assert s["trials_hist"] == st["trials_hist"]
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    assert s["chi2_init"] == pytest.approx(st["chi2_init"], rel=1e-12)
    assert s["chi2_final"] == pytest.approx(st["chi2_final"], rel=REL)
    poses, lms = o.estimates()
    pose_update_close(poses, p_ref, g.poses)
    assert np.abs((lms - g.lms) - (l_ref - g.lms)).max() <= REL * np.abs(l_ref - g.lms).max()
    assert o.activeRobustChi2() == pytest.approx(s["chi2_final"], rel=1e-12)
    # the cost from the definitions (projection = the function that generated the measurements), as test_independent_pin.py
    assert s["chi2_final"] == pytest.approx(BAProblemNumpy(g).cost(poses, lms), rel=1e-9)


@pytest.mark.parametrize("case,trials", oa.REJECT_CASES)
def test_rejected_trials_follow_the_oracle(oracle, case, trials):
    g = oa.kidnapped(*case)
    p_ref, l_ref, st = _oracle_run(oracle, case, g)
    assert st["trials_hist"] == trials
    assert np.abs(st["rho_log"]).min() > 0.2
    o = opt(g)
    assert o.optimize(10) == st["iterations"]
    assert o.stats["trials_hist"] == trials
    assert o.stats["trials"] == st["trials"] and bool(o.stats["terminated"]) == st["terminated"]
    assert np.allclose(o.stats["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(o.stats["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    poses, _ = o.estimates()
    pose_update_close(poses, p_ref, g.poses, rel=1e-4)


def test_resident_batch_equals_multi_launch_and_the_oracle(oracle):
    """the off-axis windows and their rejecting starts in one forced-resident batch (csrc/ba_window.hip has its own edge_se2xyz):
    the assertions of test_ba_window_gpu.py"""
    from se2lam_amd import capi
    from se2lam_amd.optimizer import optimize_batch
    keys = list(oa.SIZES) + [c for c, _ in oa.REJECT_CASES]
    graphs = [oa.graph(*k) for k in oa.SIZES] + [oa.kidnapped(*c) for c, _ in oa.REJECT_CASES]
    ref = [multi_launch(g, 10)[:2] for g in graphs]
    opts = [opt(g) for g in graphs]
    with env(SE2GPU_BA_RESIDENT="1"):
        its = optimize_batch(opts, 10)
    assert int(capi.lib().se2gpu_ba_last_batch_path()) == 2
    for key, g, o, (st, est), n in zip(keys, graphs, opts, ref, its):
        what = key
        assert n == st["iterations"] == o.stats["iterations"] and o.stats["trials"] == st["trials"], what
        assert o.stats["trials_hist"] == st["trials_hist"], (what, o.stats["trials_hist"], st["trials_hist"])
        assert o.stats["terminated"] == st["terminated"] and o.stats["stopped"] == st["stopped"], what
        assert np.isclose(o.stats["chi2_init"], st["chi2_init"], rtol=RTOL), what
        assert np.allclose(o.stats["chi2_hist"][:n], st["chi2_hist"][:n], rtol=RTOL), what
        assert np.allclose(o.stats["lambda_hist"][:n], st["lambda_hist"][:n], rtol=1e-7), what
        p, l = o.estimates()
        assert np.allclose(p, est[0], rtol=1e-9, atol=1e-7) and np.allclose(l, est[1], rtol=1e-9, atol=1e-6), what
        poses, lms, ost = _oracle_run(oracle, key, g)
        assert o.stats["trials_hist"] == ost["trials_hist"], what
        assert np.allclose(o.stats["chi2_hist"][:10], ost["chi2_hist"][:10], rtol=1e-7), what
        assert np.allclose(p, poses, rtol=1e-6, atol=1e-6), what
    assert [r[0]["trials_hist"] for r in ref[2:]] == [t for _, t in oa.REJECT_CASES]


def test_edge_information_on_device(oracle, synth):
    """se2gpu_ba_edge_information with the tilted extrinsic: against the oracle at test_ba_gpu.py's bound, and against the
    generator's numpy restatement (synth.edge_information) at the bounds test_ba_oracle.py holds the oracle to"""
    from se2lam_amd import optimizer as op
    for P, L in oa.SIZES:
        inp, g, level = _info_inputs(synth, g=oa.graph(P, L))
        got = op.edge_information(**inp)
        ref = oracle.ba_edge_information(**inp)
        assert got.shape == ref.shape == (g.E, 2, 2)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        gen = synth.edge_information(g.poses, g.lms, g.e_kf, g.e_lm, level, g.Rbc, g.tbc, g.fx)
        assert np.allclose(got[:, 0, 0], gen[:, 0], rtol=1e-9) and np.allclose(got[:, 1, 1], gen[:, 2], rtol=1e-9)
        assert np.allclose(got[:, 0, 1], gen[:, 1], rtol=1e-7, atol=1e-12) and np.array_equal(got[:, 0, 1], got[:, 1, 0])


def test_pose_ba_against_cost_scipy_and_the_restatement(oracle):
    """se2gpu_track_pose_ba on a case of test_track_independent.POSE_CASES seen through the off-axis camera: the checks of
    test_hip_pose_ba_against_cost_and_scipy"""
    from se2lam_amd.localizer import Localizer
    from test_off_axis import _pose_check
    from test_pose_ba import _same_run
    from test_track_independent import DELTA
    args, cam = oa.pose_problem(oracle)
    T0, meas, info, Xw, uv, w, iters = args
    loc = Localizer()
    T = loc.pose_ba(T0, meas, info, Xw, uv, w, *cam, DELTA, iters)
    st = loc.stats
    assert loc.stats_tail_intact
    _pose_check(args, cam, T, st)
    To, so = oracle.pose_only_ba(T0, meas, info, Xw, uv, w, *cam, DELTA, iters)
    _same_run(st, so)
    assert np.isfinite(T).all()
    assert np.allclose(T[:3, :3], To[:3, :3], atol=1e-7) and np.allclose(T[:3, 3], To[:3, 3], rtol=1e-5, atol=1e-3)
    # the prior's host function with the tilted extrinsic, at test_pose_ba.py's bounds
    from se2lam_amd.localizer import addPlaneMotionSE3Expmap
    m, i = addPlaneMotionSE3Expmap(T0, synth_tbc())
    mo, io = oracle.plane_motion_prior(T0, synth_tbc())
    assert np.allclose(m, mo, rtol=0, atol=1e-12) and np.allclose(i, io, rtol=1e-13, atol=0)


def synth_tbc():
    from se2lam_amd import synth
    return synth.OFF_AXIS_TBC
