"""CPU preconditions of the off-axis camera cases (test_off_axis_gpu.py): the new extrinsic has no entry that is zero or one, no
observation comes near a camera plane, the rejecting starts reject with wide margins - and a demonstration of what the old camera
could not see: a projection with one wrong term costs the same under RBC and differs under OFF_AXIS_TBC."""
import numpy as np
import pytest

import off_axis_cases as oa
from independent import BAProblemNumpy
from se2lam_amd import synth


def test_every_entry_of_the_new_rcb_is_general():
    Rcb = synth.OFF_AXIS_TBC[:3, :3].T
    assert np.allclose(Rcb @ Rcb.T, np.eye(3), atol=1e-14) and np.linalg.det(Rcb) > 0
    a = np.abs(Rcb)
    assert a.min() > 0.02 and a.max() < 0.999, a
    old = np.abs(synth.RBC)
    assert ((old == 0) | (old == 1)).all()
    f, cx, cy = synth.OFF_CENTRE_CAM
    assert f != synth.FX and cx != synth.CX and cy != synth.CY and cx != synth.IMG_W / 2 and cy != synth.IMG_H / 2


def test_with_camera_adds_nothing_but_the_camera():
    for P, L in oa.SIZES:
        g, h = synth.ba_graph(P, L), oa.graph(P, L)
        for k in ("poses", "fixed", "lms", "e_kf", "e_lm", "o_i", "o_j", "o_meas", "o_info", "poses_true", "lms_true", "e_level"):
            assert getattr(h, k) is getattr(g, k), k
        assert np.array_equal(g.Rbc, synth.RBC) and g.fx == synth.FX          # the cached graph itself is untouched
        assert np.allclose(h.Rbc, synth.OFF_AXIS_TBC[:3, :3]) and (h.fx, h.cx, h.cy) == synth.OFF_CENTRE_CAM
        # the same noise draws, outliers included: measurement minus projected truth, per camera
        def noise(q):
            Rcb = q.Rbc.T
            u, v, _, _ = synth._project(q.poses_true, q.lms_true, q.e_kf, q.e_lm, Rcb, -Rcb @ q.tbc, q.fx, q.cx, q.cy)
            return q.e_uv - np.stack([u, v], 1)
        assert np.allclose(noise(h), noise(g), rtol=0, atol=1e-9)
        assert np.abs(noise(g)).max() > 10                                      # (an outlier is among them)
        assert np.array_equal(h.e_info, synth.edge_information(g.poses, g.lms, g.e_kf, g.e_lm, g.e_level, h.Rbc, h.tbc, h.fx))
        # with the old camera the function reproduces the generator's own measurements and informations
        same = synth.with_camera(g, synth.tbc44(), (synth.FX, synth.CX, synth.CY))
        assert np.allclose(same.e_uv, g.e_uv, rtol=0, atol=1e-9) and np.array_equal(same.e_info, g.e_info)


def test_no_observation_near_a_camera_plane():
    """Z >= 300 mm in the camera frame for every edge, at the truth and at the start - no edge dropped to get there"""
    for P, L in oa.SIZES:
        g, h = synth.ba_graph(P, L), oa.graph(P, L)
        assert h.E == g.E
        assert synth.camera_depths(h, h.poses_true, h.lms_true).min() >= 300.0
        assert synth.camera_depths(h).min() >= 300.0
    for case, _ in oa.REJECT_CASES:
        assert synth.camera_depths(oa.kidnapped(*case)).min() >= 300.0


def test_reject_cases_have_wide_decision_margins(oracle):
    for case, trials in oa.REJECT_CASES:
        _, _, st = oracle.ba_optimize(oa.kidnapped(*case), 10, 0)
        assert st["trials_hist"] == trials, case
        assert max(trials) > 1 and np.abs(st["rho_log"]).min() > 0.2, case
        assert st["trials"] == sum(trials) and not st["terminated"]


def _wrong_row(problem):
    """the same cost with ONE wrong term in the projection: the landmark-z column of Rcb (what csrc/ba_device.h calls R[2], R[5],
    R[8]) has its x and z rows exchanged.  tcb stays right."""
    R = problem.Rcb.copy()
    R[0, 2], R[2, 2] = problem.Rcb[2, 2], problem.Rcb[0, 2]
    problem.Rcb = R
    return problem


def _cost_and_gradient(problem, x):
    c = problem.fun(x) @ problem.fun(x)
    grad = np.zeros(x.size)
    for k in range(x.size):
        h = 1e-4 * max(1.0, abs(x[k]))
        d = np.zeros(x.size)
        d[k] = h
        fp, fm = problem.fun(x + d), problem.fun(x - d)
        grad[k] = (fp @ fp - fm @ fm) / (2 * h)
    return c, grad


def test_teeth_a_wrong_z_column_is_invisible_under_rbc_and_visible_off_axis():
    g = synth.ba_graph(8, 60)
    x = BAProblemNumpy(g).pack(g.poses, g.lms)
    c0, g0 = _cost_and_gradient(BAProblemNumpy(g), x)
    c1, g1 = _cost_and_gradient(_wrong_row(BAProblemNumpy(g)), x)
    assert c1 == c0 and np.array_equal(g1, g0)             # both exchanged entries are exactly zero: not one bit differs
    h = oa.graph(8, 60)
    c0, g0 = _cost_and_gradient(BAProblemNumpy(h), x)
    c1, g1 = _cost_and_gradient(_wrong_row(BAProblemNumpy(h)), x)
    assert abs(c1 - c0) > 1e-2 * c0, (c0, c1)
    assert np.abs(g1 - g0).max() > 1e-2 * np.abs(g0).max()


def _pose_check(args, cam, T, st):
    """test_track_independent.py::_pose_check for the off-axis case: ten times the restatement's own figures"""
    import independent as ind
    from test_track_independent import DELTA, FLOOR
    T0, meas, info, Xw, uv, w, iters = args
    d_final, short = oa.POSE_FIGURES
    pb = ind.PoseBANumpy(meas, info, Xw, uv, w, *cam, DELTA)
    h = st["chi2_hist"]
    assert st["terminated"] or abs(h[-1] - h[-2]) <= 1e-9 * h[-1], "the case must converge within its iterations"
    return ind.check_pose_ba(pb, T0, T, st, max(10 * d_final, FLOOR), max(10 * short, FLOOR))


def test_pose_ba_restatement_against_cost_and_scipy(oracle):
    from test_track_independent import DELTA
    args, cam = oa.pose_problem(oracle)
    T, st = oracle.pose_only_ba(*args[:6], *cam, DELTA, args[6])
    fig = _pose_check(args, cam, T, st)
    print("pose_ba off axis %s: %s" % (oa.POSE_CASE, fig))
