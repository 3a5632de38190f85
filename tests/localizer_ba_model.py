"""What se2gpu_localizer_ba_batch_device has to compute up to the solve, stated in numpy from the reference's text:
Localizer::MatchLocalMap's renewal (Localizer.cpp:220-227), KeyFrame::addObservation (KeyFrame.cpp:195-203), the gate (:95-98),
the graph of Localizer::DoLocalBA (:245-288), toSE3Quat (converter.cpp:80-90), addPlaneMotionSE3Expmap (optimizer.cpp:236-314)
and the Twb that KeyFrame::setPose derives (:298-299).  Everything is FP64 numpy / Python floats, one operation at a time;
nothing here calls the library.

Tables (a dict): Tcw (nframes, 12) float32, rows 0-2 of Tcw; kps_xy (nframes, cap, 2) float32; kps_octave (nframes, cap) int32;
counts (nframes); ftr_mp (nframes, cap) int32, feature -> point or -1; kf_observed (nframes, cap) uint8; pos (m, 3) float32;
mp_null, good_prl (m) uint8; inv_level_sigma2 float32; Tbc12 (12) float64; xrot_info, yrot_info, z_info."""
import math

import numpy as np

FLAG_ENTRY, FLAG_OCTAVE = 1, 2


# ------------------------------------------------------------------------------------------------ SE3Quat

def quat_of(R):
    """Eigen::Quaterniond(R) as (w, x, y, z), w >= 0, normalised: what SE3Quat(R, t) keeps of a rotation matrix"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        v = [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t]
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        v = [0.0, 0.0, 0.0]
        v[i] = 0.5 * t
        t = 0.5 / t
        w = (R[k, j] - R[j, k]) * t
        v[j] = (R[j, i] + R[i, j]) * t
        v[k] = (R[k, i] + R[i, k]) * t
    q = np.array([w] + v)
    if q[0] < 0:
        q = -q
    return q / math.sqrt(float(q @ q))


def mat_of_quat(q):
    """Eigen::Quaterniond::toRotationMatrix"""
    w, x, y, z = (float(a) for a in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def requat(R):
    return mat_of_quat(quat_of(R))


def se3_mul(a, b):
    """SE3Quat * SE3Quat on (R, t) pairs: the product's rotation is renormalised"""
    return requat(a[0] @ b[0]), a[0] @ b[1] + a[1]


def se3_inv(a):
    return a[0].T, -(a[0].T @ a[1])


def pose12(Rt):
    return np.concatenate([np.asarray(Rt[0]).reshape(-1), np.asarray(Rt[1]).reshape(-1)])


def unpack12(p):
    p = np.asarray(p, np.float64)
    return p[:9].reshape(3, 3).copy(), p[9:12].copy()


def start_pose(row12):
    """toSE3Quat(KeyFrame::getPose()): the float matrix converted to double, its rotation through a unit quaternion"""
    T = np.asarray(row12, np.float32).astype(np.float64).reshape(3, 4)
    return requat(T[:, :3]), T[:, 3].copy()


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def plane_motion_prior(Tcw, Tbc, xrot_info, yrot_info, z_info):
    """addPlaneMotionSE3Expmap (optimizer.cpp:236-314): (measurement (R, t), information 6x6 in the order (rotation, translation))"""
    Rbw, tbw = se3_mul(Tbc, Tcw)
    q = quat_of(Rbw)
    nv = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    yaw = 2 * math.atan2(nv, q[0]) * q[3] / nv if nv > 0 else 0.0       # z of Eigen::AngleAxisd(q).angle() * axis()
    c, s = math.cos(yaw), math.sin(yaw)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    tz = np.array([tbw[0], tbw[1], 0.0])
    meas = se3_mul(se3_inv(Tbc), (Rz, tz))
    A = np.zeros((6, 6))                                               # SE3Quat::adj(): [R 0; skew(t) R  R]
    A[:3, :3] = Tbc[0]
    A[3:, 3:] = Tbc[0]
    A[3:, :3] = skew(Tbc[1]) @ Tbc[0]
    D = [xrot_info, yrot_info, 1e-4, 1e-4, 1e-4, z_info]
    info = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            acc = 0.0
            for k in range(6):
                acc += float(A[k, i]) * D[k] * float(A[k, j])
            info[i, j] = acc
    for i in range(6):                                                 # "make sure the info matrix is symmetric" (:296-298)
        for j in range(i):
            info[i, j] = info[j, i]
    return meas, info


def twb_of(pose_out12, Tbc12):
    """{x, y, theta} of Tcw^-1 * Tbc^-1 in FP64, rounded to float once (KeyFrame::setPose's Twb)"""
    Twc = se3_inv(unpack12(pose_out12))
    Tcb = se3_inv(unpack12(Tbc12))
    R, t = Twc[0] @ Tcb[0], Twc[0] @ Tcb[1] + Twc[1]
    return np.array([t[0], t[1], math.atan2(R[1, 0], R[0, 0])]).astype(np.float32)


def tcw_row_of(pose_out12):
    """toCvMat(SE3Quat) (converter.cpp:92-107) as the table row: rows 0-2 of the 4x4, rounded to float"""
    R, t = unpack12(pose_out12)
    return np.concatenate([R, t[:, None]], axis=1).reshape(12).astype(np.float32)


# ------------------------------------------------------------------------------------------------ one job

def job(T, frame, match_row=None, min_obs=30):
    """One job of the call up to the solve.  -> dict(status (1, 5 or None = the solve runs), info (8 ints), ftr_mp / kf_observed
    (the frame's rows after the renewal; None with status 1), e_ftr, xyz, uv, w, pose0 (12), prior_meas (12), prior_info (6, 6))"""
    nframes, cap = T["ftr_mp"].shape
    m = len(T["pos"])
    if not 0 <= frame < nframes:
        return dict(status=1, info=np.zeros(8, np.int32), ftr_mp=None, kf_observed=None)
    n = max(min(int(T["counts"][frame]), cap), 0)
    dual = T["ftr_mp"][frame].copy()                                   # KeyFrame::mDualObservations
    seen = T["kf_observed"][frame].copy()
    null = lambda p: bool(T["mp_null"][p])                              # noqa: E731
    renewed = 0
    if match_row is not None:                                          # Localizer.cpp:220-227
        for j in range(n):
            q = int(match_row[j])
            if not 0 <= q < m:                                         # -1 (:223), or no index into vpMPLocal at all
                continue
            if null(q):                                                # addObservation: if (pMP->isNull()) return;
                continue
            dual[j] = q
            seen[j] = 1
            renewed += 1
    flags = 0
    observations = {}                                                  # KeyFrame::mObservations: point -> feature
    named = 0
    for j in range(n):                                                 # both passes add in ascending feature order
        p = int(dual[j])
        if p == -1:
            continue
        if not 0 <= p < m:
            flags |= FLAG_ENTRY
            continue
        named += 1
        observations[p] = j                                            # mObservations[pMP] = idx overwrites
    n_obs = len(observations)                                          # getSizeObsMP()
    e_ftr, xyz, uv, w = [], [], [], []
    for p, j in sorted(observations.items(), key=lambda it: it[1]):    # our order: ascending feature index
        if null(p) or not T["good_prl"][p]:                            # :263
            continue
        octave = int(T["kps_octave"][frame, j])                         # the feature's own octave (the two-sided map)
        if not 0 <= octave < len(T["inv_level_sigma2"]):
            flags |= FLAG_OCTAVE
            continue
        e_ftr.append(j)
        xyz.append(T["pos"][p].astype(np.float64))                      # toVector3d(pMP->getPos())
        uv.append(T["kps_xy"][frame, j].astype(np.float64))             # toVector2d(keyPointsUn[ftrIdx].pt)
        w.append(float(np.float32(T["inv_level_sigma2"][octave])))
    p0 = start_pose(T["Tcw"][frame])
    meas, info = plane_motion_prior(p0, unpack12(T["Tbc12"]), T["xrot_info"], T["yrot_info"], T["z_info"])
    words = np.array([n, n_obs, len(e_ftr), renewed, named - n_obs, flags, 0, 0], np.int32)
    return dict(status=5 if n_obs <= min_obs else None, info=words, ftr_mp=dual, kf_observed=seen,
                e_ftr=np.array(e_ftr, np.int32), xyz=np.array(xyz, np.float64).reshape(-1, 3),
                uv=np.array(uv, np.float64).reshape(-1, 2), w=np.array(w, np.float64), pose0=pose12(p0), prior_meas=pose12(meas),
                prior_info=info)
