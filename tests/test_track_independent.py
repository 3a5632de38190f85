"""The four tracking / mapping thread kernels against references that do NOT share the restatement's algorithm:

    k_triangulate (Track::doTriangulate)                 LAPACK's SVD of the same float32 4x4 systems
    k_fm_models / k_fm_score / k_fm_select (RANSAC mask)  numpy 7-point models + an FP64 replay of the registrator's rules
    k_pose_ba (Localizer::DoLocalBA)                     the definitional cost and scipy's trust-region least squares
    k_sparsify (Sparsifier::DoMarginalizeSE3XYZ)         the numpy model, every measurement order, the kernel's edge shapes

Every check is one function of tests/independent.py applied twice: to the CPU restatement's output (no marker - it proves
without a GPU that the reference, the inputs and every cap are sound) and to the HIP path's output (@pytest.mark.gpu), which is
also compared with the restatement wherever the older tests do so.  The `*_has_teeth` tests perturb the restatement's output
and require the checker to fail.

Tolerances come from the number formats or from the restatement's own figures, never from the HIP output:
  * triangulation: 3 * 2^-24 per coordinate plus independent.TRI_C * 2^-52 * s1 / (s3 - s4) mapped to the coordinates;
  * RANSAC: the float band of independent.epipolar_errors; at most 1 % of the points of a case may lie inside it;
  * pose BA: per case, ten times the restatement's own discrepancy / shortfall (the figures in POSE_CASES, measured with
    `python tests/test_track_independent.py`), never below 1e-12 - the round-off of one pass of sums over the edges.
"""
import os
import sys

import numpy as np
import pytest

for _p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import independent as ind  # noqa: E402

# =================================================================================================== 1. triangulation
# (scene, n, seed, has_obs: "some" / "ones" / "zeros" / None, minDegree)
TRI_CASES = [("benign", 600, 7, "some", 2), ("low_parallax", 600, 7, "some", 2), ("far", 600, 7, "some", 2),
             ("behind", 600, 7, "some", 2), ("zero_baseline", 600, 7, "some", 2), ("noisy", 600, 7, "some", 2),
             ("benign", 127, 1, "some", 1), ("benign", 128, 2, "zeros", 2), ("noisy", 129, 3, None, 3),
             ("low_parallax", 255, 4, "some", 4), ("far", 257, 5, "ones", 2), ("benign", 50000, 6, "some", 2),
             ("noisy", 1000, 11, None, 2)]


def _tri_inputs(synth, kind, n, seed, obs, mind):
    k1, k2, match, has_obs, P1, P2, Ocam, _ = synth.triangulation_scene(kind, n, seed)
    ho = {"some": has_obs, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), None: None}[obs]
    lower, upper = (10000.0, 250000.0) if kind == "far" else (500.0, 8000.0)
    return (k1, k2, match, ho, P1, P2, Ocam, lower, upper, mind)


def _tri_special(synth):
    """inputs the generator never produces: no current features at all; two reference features on one current feature"""
    k1, k2, match, ho, P1, P2, Ocam, lower, upper, mind = _tri_inputs(synth, "benign", 200, 9, "some", 2)
    yield (k1, k2[:0], np.full(200, -1, np.int32), ho, P1, P2, Ocam, lower, upper, mind)
    dup = match.copy()
    src = np.flatnonzero(dup >= 0)
    dup[src[1]] = dup[src[0]]; dup[src[7]] = dup[src[0]]
    yield (k1, k2, dup, ho, P1, P2, Ocam, lower, upper, mind)


@pytest.mark.parametrize("kind,n,seed,obs,mind", TRI_CASES)
def test_triangulate_restatement_against_lapack(oracle, synth, kind, n, seed, obs, mind):
    inp = _tri_inputs(synth, kind, n, seed, obs, mind)
    out = oracle.triangulate(*inp)
    fig = ind.check_triangulation(inp, out, degenerate=kind == "zero_baseline")
    print("triangulate %s n %d: %.3f of the tolerance, %.3f %% borderline" % (kind, n, fig["used"], 100 * fig["borderline"]))
    if kind in ("benign", "noisy") and obs != "ones":
        assert out[3] > 0 and (out[2] >= 0).sum() > 0.3 * n          # the scene exercises both gates


def test_triangulate_restatement_special_inputs(oracle, synth):
    for inp in _tri_special(synth):
        ind.check_triangulation(inp, oracle.triangulate(*inp))


def test_triangulation_checker_has_teeth(oracle, synth):
    inp = _tri_inputs(synth, "benign", 600, 7, "some", 2)
    pos, good, m, ng, nold = oracle.triangulate(*inp)
    ind.check_triangulation(inp, (pos, good, m, ng, nold))
    i = int(np.flatnonzero((m >= 0) & (inp[3] == 0))[5])
    bad = pos.copy(); bad[i, 0] *= np.float32(1 + 1e-5)                     # one position, 1e-5 relative
    with pytest.raises(AssertionError):
        ind.check_triangulation(inp, (bad, good, m, ng, nold))
    flip = good.copy(); flip[i] ^= 1                                        # one parallax flag (and the counter with it)
    with pytest.raises(AssertionError):
        ind.check_triangulation(inp, (pos, flip, m, int(flip.sum()), nold))
    with pytest.raises(AssertionError):                                     # a counter that lost an atomic
        ind.check_triangulation(inp, (pos, good, m, ng - 1, nold))
    drop = m.copy(); drop[i] = -1; p2 = pos.copy(); p2[i] = 0; g2 = good.copy(); g2[i] = 0   # a point dropped inside the gate
    with pytest.raises(AssertionError):
        ind.check_triangulation(inp, (p2, g2, drop, int(g2.sum()), nold))


def _same_triangulation(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert tuple(got[3:]) == tuple(ref[3:])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,obs,mind", TRI_CASES)
def test_hip_triangulate_against_lapack(oracle, synth, kind, n, seed, obs, mind):
    from se2lam_amd.matcher import doTriangulate
    from se2lam_amd.track import Track
    inp = _tri_inputs(synth, kind, n, seed, obs, mind)
    ref = oracle.triangulate(*inp)
    for fn in (doTriangulate, Track().doTriangulate):          # se2gpu_triangulate, se2gpu_track_triangulate
        got = fn(*inp)
        ind.check_triangulation(inp, got, degenerate=kind == "zero_baseline")
        _same_triangulation(got, ref)


@pytest.mark.gpu
def test_hip_triangulate_special_inputs_and_workspace_reuse(oracle, synth):
    from se2lam_amd.matcher import doTriangulate
    from se2lam_amd.track import Track
    tr = Track()
    for inp in _tri_special(synth):
        for fn in (doTriangulate, tr.doTriangulate):
            got = fn(*inp)
            ind.check_triangulation(inp, got)
            _same_triangulation(got, oracle.triangulate(*inp))
    # one workspace: a large count, then a small one (nothing of the first call may survive), then large again
    for kind, n, seed in (("benign", 50000, 6), ("noisy", 129, 3), ("behind", 5000, 8)):
        inp = _tri_inputs(synth, kind, n, seed, "some", 2)
        got = tr.doTriangulate(*inp)
        ind.check_triangulation(inp, got)
        _same_triangulation(got, oracle.triangulate(*inp))


# ======================================================================================= 2. fundamental-matrix mask
# (seed, n, outlier share, noise px): the eight cases of tests/test_ransac.py, the first RANSAC count, a few thousand points
# (k_fm_score strides by 64, k_fm_select by 256), pure inliers (the loop stops after a handful of samples), 70 % outliers (all 1000)
FM_CASES = [(0, 700, 0.3, 0.5), (1, 400, 0.5, 0.5), (2, 1000, 0.1, 0.5), (3, 60, 0.2, 0.5), (4, 15, 0.0, 0.5), (5, 16, 0.3, 0.5),
            (6, 250, 0.7, 0.5), (7, 900, 0.0, 0.5), (8, 3001, 0.25, 0.5), (9, 500, 0.0, 0.0), (10, 2047, 0.4, 0.5)]
# (seed, n): every LMedS count, the last one (14) three times.  With n = 14 most seeds put the eighth-smallest error of the winning
# model inside the float band of sigma's floor (0.001 px); seeds 20, 26, 31 do not (the restatement meets the cap on the CPU).
LMEDS_CASES = [(20, 14), (26, 14), (31, 14), (22, 8), (21, 9), (24, 10), (20, 11), (25, 12), (23, 13)]


def _fm_check(oracle, p1, p2, mask, ni, info):
    n = len(p1)
    lmeds = n < 15
    subsets = oracle.ransac_subsets(n, info["iterations"] if lmeds else 1000)
    assert 0 <= info["sample"] < len(subsets), info
    Fs = oracle.seven_point(p1, p2, subsets[info["sample"]])
    assert 0 <= info["model"] < len(Fs), info
    return (ind.check_lmeds_mask if lmeds else ind.check_fundamental_mask)(p1, p2, subsets, mask, ni, info, Fs[info["model"]])


@pytest.mark.parametrize("seed,n,frac,noise", FM_CASES)
def test_fundamental_mask_restatement_against_replay(oracle, synth, seed, n, frac, noise):
    p1, p2, _ = synth.two_view_matches(seed, n, frac, noise)
    mask, info = oracle.fundamental_mask_info(p1, p2)
    fig = _fm_check(oracle, p1, p2, mask, info["inliers"], info)
    print("ransac seed %d n %d: %d inliers, winner (%d, %d), %d iterations, band share %.4f, matrix distance %.1e"
          % (seed, n, info["inliers"], info["sample"], info["model"], info["iterations"], fig["band"], fig["dist"]))
    if frac == 0.0 and noise == 0.0:
        assert info["iterations"] <= 10
    if frac >= 0.7:
        assert info["iterations"] == 1000


@pytest.mark.parametrize("seed,n", LMEDS_CASES)
def test_lmeds_mask_restatement_against_replay(oracle, synth, seed, n):
    p1, p2, _ = synth.two_view_matches(seed, 14, 0.15)
    p1, p2 = p1[:n], p2[:n]
    mask, info = oracle.fundamental_mask_info(p1, p2)
    _fm_check(oracle, p1, p2, mask, info["inliers"], info)


def test_fundamental_mask_checker_has_teeth(oracle, synth):
    p1, p2, _ = synth.two_view_matches(1, 400, 0.5)
    mask, info = oracle.fundamental_mask_info(p1, p2)
    _fm_check(oracle, p1, p2, mask, info["inliers"], info)
    subsets = oracle.ransac_subsets(400, 1000)
    Fw = oracle.seven_point(p1, p2, subsets[info["sample"]])[info["model"]]
    err, dev = ind.epipolar_errors(Fw[None], p1, p2)
    i = int(np.argmax(np.abs(err[0] - 9.0) - dev[0]))                        # a point far outside the band
    bad = mask.copy(); bad[i] ^= 1
    with pytest.raises(AssertionError):                                     # one mask bit, count kept consistent
        _fm_check(oracle, p1, p2, bad, int(bad.sum()), dict(info, inliers=int(bad.sum())))
    with pytest.raises(AssertionError):                                     # the winning sample index by one
        _fm_check(oracle, p1, p2, mask, info["inliers"], dict(info, sample=info["sample"] + 1))
    with pytest.raises(AssertionError):                                     # an iteration count the stop rule does not give
        _fm_check(oracle, p1, p2, mask, info["inliers"], dict(info, iterations=info["iterations"] + 3))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,frac,noise", FM_CASES)
def test_hip_fundamental_mask_against_replay(oracle, synth, seed, n, frac, noise):
    from se2lam_amd.track import Track
    p1, p2, _ = synth.two_view_matches(seed, n, frac, noise)
    tr = Track()
    mask, ni = tr.findFundamentalMat(p1, p2)
    info = tr.last_ransac()
    _fm_check(oracle, p1, p2, mask, ni, info)
    mask_ref, info_ref = oracle.fundamental_mask_info(p1, p2)
    assert np.array_equal(mask, mask_ref) and info == info_ref


@pytest.mark.gpu
def test_hip_lmeds_and_handle_reuse_against_replay(oracle, synth):
    from se2lam_amd.track import Track
    tr = Track()
    for seed, n in LMEDS_CASES:
        p1, p2, _ = synth.two_view_matches(seed, 14, 0.15)
        p1, p2 = p1[:n], p2[:n]
        mask, ni = tr.findFundamentalMat(p1, p2)
        info = tr.last_ransac()
        _fm_check(oracle, p1, p2, mask, ni, info)
        mask_ref, info_ref = oracle.fundamental_mask_info(p1, p2)
        assert np.array_equal(mask, mask_ref) and info == info_ref
    # one handle across different n (the subset cache is keyed on n alone): large, small, large, and the first n again with other data
    for seed, n, frac, noise in (FM_CASES[8], FM_CASES[3], FM_CASES[10], (3, 3001, 0.25, 0.5)):
        p1, p2, _ = synth.two_view_matches(seed, n, frac, noise)
        mask, ni = tr.findFundamentalMat(p1, p2)
        info = tr.last_ransac()
        mask_ref, info_ref = oracle.fundamental_mask_info(p1, p2)
        assert np.array_equal(mask, mask_ref) and info == info_ref
        if seed != 3 or n != 3001:
            _fm_check(oracle, p1, p2, mask, ni, info)


# ================================================================================================ 3. pose-only BA
TBC = np.eye(4)
TBC[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0.0]]
TBC[:3, 3] = [100.0, 0.0, 300.0]
F, CX, CY = 400.0, 320.0, 240.0
DELTA = float(np.sqrt(5.991))
FLOOR = 1e-12

# name: (seed, n, generator arguments, prior from a pose 0.2 rad / 100 mm away, iterations,
#        the restatement's |chi2_final - cost(returned pose)| / cost, its shortfall against scipy (None: LM has not converged
#        within the iterations, no optimum check) - both relative, measured on the CPU by `python tests/test_track_independent.py`)
SLOW = dict(start=(600.0, 0.3))          # a start 600 mm / 0.3 rad off: LM is still moving after 100 iterations
POSE_CASES = {
    "n1": (10, 1, {}, False, 30, 2.8e-07, None),
    "n63": (11, 63, {}, False, 30, 2.0e-10, 1.4e-08),
    "n64": (12, 64, {}, False, 30, 5.3e-10, 4.9e-08),
    "n65": (13, 65, {}, False, 30, 7.2e-11, 1.3e-11),
    "n255": (14, 255, {}, False, 30, 3.3e-16, 5.4e-09),
    "n256": (15, 256, {}, False, 30, 5.3e-16, 7.1e-09),
    "n257": (16, 257, {}, False, 30, 6.8e-16, 4.0e-09),
    "n1023": (17, 1023, {}, False, 30, 3.5e-12, 1.4e-10),
    "prior_far_300": (20, 300, {}, True, 30, 0.0, 1.2e-07),
    "prior_far_64": (21, 64, {}, True, 30, 2.2e-16, 1.1e-06),
    "yaw_plus_pi": (22, 300, dict(yaw=np.pi - 5e-4), False, 30, 4.4e-16, 9.6e-10),
    "yaw_minus_pi": (23, 300, dict(yaw=-np.pi + 5e-4), False, 30, 8.2e-16, 7.7e-12),
    "weights_wide": (24, 300, dict(weights="wide"), False, 30, 2.6e-16, 2.1e-10),
    "behind_4": (25, 300, dict(behind=4), False, 30, 3.2e-16, 2.4e-10),
    "slow_65": (26, 300, SLOW, False, 65, 1.4e-15, None),
    "slow_100": (26, 300, SLOW, False, 100, 5.4e-16, None),
}


def _pose_problem(oracle, synth, name):
    seed, n, kw, far, iters, d_final, short = POSE_CASES[name]
    _, T0, Xw, uv, w, pose = synth.pose_ba_case(seed, n, **kw)
    src = np.linalg.inv(synth.body_pose(pose[0] + 70.0, pose[1] - 70.0, pose[2] + 0.2) @ TBC) if far else T0
    meas, info = oracle.plane_motion_prior(src, TBC)
    return T0, meas, info, Xw, uv, w, iters


def _pose_check(name, args, T, st):
    T0, meas, info, Xw, uv, w, iters = args
    d_final, short = POSE_CASES[name][5:]
    pb = ind.PoseBANumpy(meas, info, Xw, uv, w, F, CX, CY, DELTA)
    if short is None:           # not converged: the two costs only
        c0, c1 = pb.cost(T0), pb.cost(T)
        assert abs(st["chi2_init"] - c0) <= 1e-12 * c0 and abs(st["chi2_final"] - c1) <= max(10 * d_final, FLOOR) * c1
        return dict(d_init=abs(st["chi2_init"] - c0) / c0, d_final=abs(st["chi2_final"] - c1) / c1, shortfall=None)
    h = st["chi2_hist"]
    assert st["terminated"] or abs(h[-1] - h[-2]) <= 1e-9 * h[-1], "the case must converge within its iterations"
    return ind.check_pose_ba(pb, T0, T, st, max(10 * d_final, FLOOR), max(10 * short, FLOOR))


def _pose_restatement(oracle, args):
    T0, meas, info, Xw, uv, w, iters = args
    return oracle.pose_only_ba(T0, meas, info, Xw, uv, w, F, CX, CY, DELTA, iters)


@pytest.mark.parametrize("name", sorted(POSE_CASES))
def test_pose_ba_restatement_against_cost_and_scipy(oracle, synth, name):
    args = _pose_problem(oracle, synth, name)
    T, st = _pose_restatement(oracle, args)
    fig = _pose_check(name, args, T, st)
    print("pose_ba %s: %s" % (name, fig))
    if args[6] > 64:
        assert st["iterations"] > 64 and len(st["chi2_hist"]) == 64


def test_pose_ba_checker_has_teeth(oracle, synth):
    args = _pose_problem(oracle, synth, "n257")
    T, st = _pose_restatement(oracle, args)
    _pose_check("n257", args, T, st)
    with pytest.raises(AssertionError):                                     # chi2_final, 1e-6 relative
        _pose_check("n257", args, T, dict(st, chi2_final=st["chi2_final"] * (1 + 1e-6)))
    with pytest.raises(AssertionError):
        _pose_check("n257", args, T, dict(st, chi2_init=st["chi2_init"] * (1 + 1e-9)))
    T_off = ind.se3_exp_scipy([0, 1e-3, 0, 0, 0, 0]) @ T                     # a pose 1 mrad off the optimum, its own cost reported
    pb = ind.PoseBANumpy(args[1], args[2], args[3], args[4], args[5], F, CX, CY, DELTA)
    with pytest.raises(AssertionError):
        _pose_check("n257", args, T_off, dict(st, chi2_final=pb.cost(T_off)))


def _same_run(st, so):
    """tests/test_pose_ba.py::_same_run: identical trial counts and costs while the steps still change the cost"""
    from test_pose_ba import _same_run as same
    same(st, so)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POSE_CASES))
def test_hip_pose_ba_against_cost_and_scipy(oracle, synth, name):
    from se2lam_amd.localizer import Localizer
    args = _pose_problem(oracle, synth, name)
    T0, meas, info, Xw, uv, w, iters = args
    loc = Localizer()
    T = loc.pose_ba(T0, meas, info, Xw, uv, w, F, CX, CY, DELTA, iters)
    st = loc.stats
    assert loc.stats_tail_intact                     # nothing written past the statistics struct
    _pose_check(name, args, T, st)
    To, so = _pose_restatement(oracle, args)
    _same_run(st, so)
    assert np.isfinite(T).all()
    assert np.allclose(T[:3, :3], To[:3, :3], atol=1e-7) and np.allclose(T[:3, 3], To[:3, 3], rtol=1e-5, atol=1e-3)
    if iters > 64:
        assert st["iterations"] > 64 and len(st["chi2_hist"]) == 64 and st["iterations"] == so["iterations"]


YAWS = [-np.pi, -np.pi + 1e-4, -2.0, -np.pi / 2, -1e-3, 0.0, 1e-9, 0.7, np.pi / 2, 2.9, np.pi - 1e-4, np.pi]


def _check_plane_prior(Tcw, meas, info):
    mn, infn = ind.plane_motion_prior_numpy(Tcw, TBC)
    assert np.allclose(info, infn, rtol=1e-12, atol=0) and np.array_equal(info, info.T)
    Twb = np.linalg.inv(TBC @ meas)                 # the measured body pose: on the plane, upright
    assert abs(Twb[2, 3]) <= 1e-9 and np.allclose(Twb[2, :3], [0, 0, 1], atol=1e-12) and np.allclose(Twb[:3, 2], [0, 0, 1], atol=1e-12)
    assert np.allclose(meas, mn, atol=1e-9)
    assert np.allclose((TBC @ meas)[:2, 3], (TBC @ Tcw)[:2, 3], atol=1e-9)


def _plane_poses(synth):
    for yaw in YAWS:
        for roll, z in ((0.0, 0.0), (0.02, 35.0)):
            Twb = synth.body_pose(300.0, -200.0, yaw)
            cr, sr = np.cos(roll), np.sin(roll)
            Twb[:3, :3] = Twb[:3, :3] @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
            Twb[2, 3] = z
            yield np.linalg.inv(Twb @ TBC)


def test_plane_motion_prior_restatement_against_definition(oracle, synth):
    for Tcw in _plane_poses(synth):
        _check_plane_prior(Tcw, *oracle.plane_motion_prior(Tcw, TBC))
    Tcw = next(_plane_poses(synth))
    meas, info = oracle.plane_motion_prior(Tcw, TBC)
    bad = info.copy(); bad[0, 4] *= 1 + 1e-9; bad[4, 0] = bad[0, 4]
    with pytest.raises(AssertionError):
        _check_plane_prior(Tcw, meas, bad)


@pytest.mark.gpu
def test_hip_plane_motion_prior_against_definition(oracle, synth):
    from se2lam_amd.localizer import addPlaneMotionSE3Expmap
    for Tcw in _plane_poses(synth):
        m, i = addPlaneMotionSE3Expmap(Tcw, TBC)
        _check_plane_prior(Tcw, m, i)
        mo, io = oracle.plane_motion_prior(Tcw, TBC)
        assert np.allclose(m, mo, rtol=0, atol=1e-12) and np.allclose(i, io, rtol=1e-13, atol=0)


# ==================================================================================================== 4. sparsifier
PAIR_SPECS = ((12, 0, 400.0), (80, 1, 250.0), (200, 2, 800.0), (10, 4, 100.0), (150, 5, 600.0), (220, 196366, 484.40666147511246),
              (249, 77, 120.0))          # the pairs of tests/test_sparsify.py::test_hip_batch_matches_oracle
ORDER_SENSITIVE = 5                      # the 220-point pair: H11 summed in another order moves its information by 99 %


def _empty_pair(synth):
    kf = synth.kf_pair(4, 50)[0]
    return kf, np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3, 3))


def _sparsify_shapes(synth):
    """(name, pair, compare the spectrum with the numpy model) - shapes the generator alone never produces"""
    for N in (1, 2, 3):
        yield "N%d" % N, synth.kf_pair(N, 30 + N), False
    for N in (63, 64, 65, 129):                                   # the 64-lane stride of the point loop
        yield "N%d" % N, synth.kf_pair(N, 40 + N), True
    kf, mp, m_kf, m_mp, m_info = synth.kf_pair(40, 60)
    keep = ~((m_mp == 5) | ((m_mp == 9) & (m_kf == 1)))           # point 5 unseen, point 9 seen by key frame 0 only
    yield "unseen_and_single", (kf, mp, m_kf[keep], m_mp[keep], m_info[keep]), True
    third = (kf, mp, np.r_[m_kf[:7], 2, m_kf[7:], 2, 3].astype(np.int32), np.r_[m_mp[:7], 11, m_mp[7:], 0, 39].astype(np.int32),
             np.concatenate([m_info[:7], m_info[:1], m_info[7:], m_info[3:5]]))
    yield "third_key_frame", third, True
    twice = (kf, mp, np.r_[m_kf, 0, 1].astype(np.int32), np.r_[m_mp, 3, 3].astype(np.int32), np.concatenate([m_info, m_info[20:22]]))
    yield "measured_twice", twice, True
    yield "no_points", _empty_pair(synth), False


def _check_shape(oracle, name, pair, spectrum, z, info):
    ind.check_sparsify(pair, z, info, spectrum=spectrum)
    if name == "third_key_frame":                                 # sparsifier.cpp:117-119: as if those measurements were not there
        keep = pair[2] < 2
        zr, ir, _ = oracle.sparsify(pair[0], pair[1], pair[2][keep], pair[3][keep], pair[4][keep])
        ind.check_sparsify_equals(z, info, zr, ir)


def test_sparsify_restatement_shapes_against_numpy_model(oracle, synth):
    for name, pair, spectrum in _sparsify_shapes(synth):
        z, info, _ = oracle.sparsify(*pair)
        _check_shape(oracle, name, pair, spectrum, z, info)


@pytest.mark.parametrize("spec", PAIR_SPECS)
def test_sparsify_restatement_orders(oracle, synth, spec):
    """the restatement follows the reference: the key-frame blocks of H11 are added in the order the measurements come.
    Key-frame-major order (GlobalMapper::CreateVecMeasSE3XYZ) gives the same sums as the generator's point-major order, bit for
    bit; any other order is its own answer, which on the 220-point pair is far from the point-major one."""
    pair = synth.kf_pair(*spec)
    z0, i0, _ = oracle.sparsify(*pair)
    ind.check_sparsify(pair, z0, i0, spectrum=False)
    zk, ik, _ = oracle.sparsify(*synth.kf_pair_reorder(pair, "kf_major"))
    assert np.array_equal(zk, z0) and np.array_equal(ik, i0)
    for order in ("reversed", "permuted"):
        z, info, _ = oracle.sparsify(*synth.kf_pair_reorder(pair, order, seed=1))
        ind.check_sparsify(pair, z, info, spectrum=False)
    if spec == PAIR_SPECS[ORDER_SENSITIVE]:                        # teeth: one measurement order for another
        zr, ir, _ = oracle.sparsify(*synth.kf_pair_reorder(pair, "reversed"))
        with pytest.raises(AssertionError):
            ind.check_sparsify_equals(z0, i0, zr, ir)


def test_sparsify_checker_has_teeth(oracle, synth):
    pair = synth.kf_pair(80, 1)
    z, info, _ = oracle.sparsify(*pair)
    ind.check_sparsify(pair, z, info)
    lam, U = np.linalg.eigh(info)
    for k, f in ((1, 5.0), (5, 0.5), (0, 1e-8 / lam[0])):         # a translation eigenvalue, the clamp above, the clamp below
        l2 = lam.copy(); l2[k] *= f
        bad = (U * l2) @ U.T
        with pytest.raises(AssertionError):
            ind.check_sparsify(pair, z, 0.5 * (bad + bad.T))
    skew = info.copy(); skew[0, 1] += 1e-12
    with pytest.raises(AssertionError):
        ind.check_sparsify(pair, z, skew)
    zb = z.copy(); zb[0, 3] += 1e-6
    with pytest.raises(AssertionError):
        ind.check_sparsify(pair, zb, info)


@pytest.mark.gpu
def test_hip_sparsify_follows_the_measurement_order(oracle, synth):
    """every pair of test_hip_batch_matches_oracle in key-frame-major, reversed and permuted order: the restatement's answer FOR
    THAT ORDER within the suite's 1e-5; key-frame-major bit-equal to point-major.  (The 220-point pair reversed is the case a
    kernel that sums H11 by point index fails: 99 % off.)"""
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ_batch
    pairs = [synth.kf_pair(*sp) for sp in PAIR_SPECS]
    grouped = DoMarginalizeSE3XYZ_batch(pairs)
    for order in synth.KF_PAIR_ORDERS:
        re = [synth.kf_pair_reorder(p, order, seed=1) for p in pairs]
        got = grouped if order == "grouped" else DoMarginalizeSE3XYZ_batch(re)
        for p, (z, info), (z0, i0) in zip(re, got, grouped):
            zr, ir, _ = oracle.sparsify(*p)
            ind.check_sparsify_equals(z, info, zr, ir)
            assert np.abs(info - info.T).max() == 0
            if order == "kf_major":
                assert np.array_equal(z, z0) and np.array_equal(info, i0)


@pytest.mark.gpu
def test_hip_sparsify_against_numpy_model(oracle, synth):
    """the spectrum assertions of tests/test_sparsify.py::test_oracle_against_the_numpy_model on the DEVICE output"""
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ_batch
    pairs = [synth.kf_pair(N, seed) for N, seed in ((12, 0), (80, 1), (200, 2))]
    for pair, (z, info) in zip(pairs, DoMarginalizeSE3XYZ_batch(pairs)):
        ind.check_sparsify(pair, z, info)


@pytest.mark.gpu
def test_hip_sparsify_shapes(oracle, synth):
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ, DoMarginalizeSE3XYZ_batch
    shapes = list(_sparsify_shapes(synth))
    got = DoMarginalizeSE3XYZ_batch([p for _, p, _ in shapes])          # the empty pair sits inside a batch of non-empty ones
    for (name, pair, spectrum), (z, info) in zip(shapes, got):
        _check_shape(oracle, name, pair, spectrum, z, info)
        zr, ir, _ = oracle.sparsify(*pair)
        ind.check_sparsify_equals(z, info, zr, ir)
        za, ia = DoMarginalizeSE3XYZ(*pair)                             # a batch of one: the same bits
        assert np.array_equal(za, z) and np.array_equal(ia, info), name


@pytest.mark.gpu
def test_hip_sparsify_large_batch_equals_single_runs(oracle, synth):
    """600 pairs - more workgroups than compute units - give, pair by pair, the bits of the same pair run alone"""
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ, DoMarginalizeSE3XYZ_batch
    distinct = [synth.kf_pair(N, 70 + N, 150.0 + 10 * N) for N in (5, 17, 33, 48, 64, 65, 70, 90)] + [_empty_pair(synth)]
    alone = [DoMarginalizeSE3XYZ(*p) for p in distinct]
    rng = np.random.default_rng(5)
    pick = rng.integers(0, len(distinct), 600)
    got = DoMarginalizeSE3XYZ_batch([distinct[k] for k in pick])
    for k, (z, info) in zip(pick, got):
        assert np.array_equal(z, alone[k][0]) and np.array_equal(info, alone[k][1])
    for p, (z, info) in zip(distinct, alone):
        zr, ir, _ = oracle.sparsify(*p)
        ind.check_sparsify_equals(z, info, zr, ir)


# ============================================================================================== measured figures
if __name__ == "__main__":
    # the restatement's own figures, for POSE_CASES and profiles/track_independent.md:  python tests/test_track_independent.py
    from oracle import oracle as _o
    from se2lam_amd import synth as _s
    for _name in POSE_CASES:
        _args = _pose_problem(_o, _s, _name)
        _T, _st = _pose_restatement(_o, _args)
        _pb = ind.PoseBANumpy(_args[1], _args[2], _args[3], _args[4], _args[5], F, CX, CY, DELTA)
        _c1 = _pb.cost(_T)
        _short = None
        if POSE_CASES[_name][6] is not None:
            _short = max((_c1 - _pb.minimise(_T)[1]) / _c1, (_c1 - _pb.minimise(_args[0])[1]) / _c1)
        print("%-14s iterations %3d terminated %d  |chi2_final - cost| / cost = %.1e  shortfall = %s"
              % (_name, _st["iterations"], _st["terminated"], abs(_st["chi2_final"] - _c1) / _c1,
                 "-" if _short is None else "%.1e" % _short))
