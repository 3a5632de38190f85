"""SE(2) windows seen through synth.OFF_AXIS_TBC / OFF_CENTRE_CAM (synth.with_camera) instead of the signed permutation RBC and the
centred camera: the graphs and the rejecting starts that test_off_axis.py (CPU preconditions) and test_off_axis_gpu.py share.  No
tests, no fixtures."""
import functools

from se2lam_amd import synth

SIZES = ((8, 60), (21, 600))

# (P, L, dxy [mm], dtheta [rad], displaced key frames, seed) of synth.kidnapped on the off-axis window -> the trials per iteration
# of g2o's policy on that start.  Seeds 0..39 were tried with the oracle on the CPU and these kept because they reject trials,
# every |rho| of the run is above 0.4 (test_off_axis.py asserts 0.2, as test_ba_oracle.py does of ba_cases.LM_REJECT_CASES) and no
# observed point is closer than 2.6 m to its camera plane at the start.
REJECT_CASES = [
    ((8, 60, 3000.0, 0.3, 4, 0), [1, 1, 7, 1, 4, 1, 4, 1, 5, 1]),
    ((21, 600, 3000.0, 0.3, 4, 8), [1, 1, 1, 1, 7, 2, 4, 1, 3, 3]),
]


@functools.lru_cache(maxsize=None)
def graph(P, L):
    return synth.with_camera(synth.ba_graph(P, L))


def kidnapped(P, L, dxy, dth, nbad, seed):
    return synth.kidnapped(graph(P, L), dxy, dth, nbad, seed)


# ---- Localizer::DoLocalBA: a case of test_track_independent.POSE_CASES through the off-axis camera -----------------------------
POSE_CASE = "n257"
# the restatement's own |chi2_final - cost(returned pose)| / cost and its shortfall against scipy on this case (relative; printed
# by test_off_axis.py::test_pose_ba_restatement_against_cost_and_scipy): the bounds are ten times these, as for POSE_CASES
POSE_FIGURES = (6.8e-16, 2.3e-09)


def pose_problem(oracle, name=POSE_CASE):
    """-> ((T0, meas, info, Xw, uv, w, iters), (f, cx, cy)): the case's world points, weights, noise draws and start, with the camera
    at synth.OFF_AXIS_TBC on the same body and the intrinsics OFF_CENTRE_CAM"""
    import numpy as np
    from test_track_independent import CX, CY, F, POSE_CASES, TBC
    seed, n, kw, far, iters = POSE_CASES[name][:5]
    Tt, T0, Xw, uv, w, pose = synth.pose_ba_case(seed, n, **kw)
    Tbc, (f, cx, cy) = synth.OFF_AXIS_TBC, synth.OFF_CENTRE_CAM
    D = np.linalg.inv(Tbc) @ TBC                                   # T_c'_c: the new camera from the old one

    def project(T, f, cx, cy):
        p = Xw @ T[:3, :3].T + T[:3, 3]
        assert (p[:, 2] >= 300.0).all() or kw.get("behind")
        return f * p[:, :2] / p[:, 2:] + [cx, cy]

    uv2 = project(D @ Tt, f, cx, cy) + (uv - project(Tt, F, CX, CY))
    src = np.linalg.inv(synth.body_pose(pose[0] + 70.0, pose[1] - 70.0, pose[2] + 0.2) @ Tbc) if far else D @ T0
    meas, info = oracle.plane_motion_prior(src, Tbc)
    return (D @ T0, meas, info, Xw, uv2, w, iters), (f, cx, cy)
