"""Host-side mirror of Localizer::DoLocalBA (/root/reference/src/Localizer.cpp:233-302): pose-only bundle adjustment of
the current key frame against the fixed map points it observes, computed by libse2gpu (csrc/pose_ba.hip) in one launch, and
do_local_ba_batch_device: the same for a batch of frames on the map's tables in device memory, with the observation renewal,
the gate and the pose write-back around it (csrc/localizer_ba_device.hip).  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import dev_ptr as _ptr


def _pose12(T) -> np.ndarray:
    T = np.asarray(T, np.float64)
    if T.shape == (12,):
        return np.ascontiguousarray(T)
    return np.ascontiguousarray(np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]))


def _matrix(p) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3] = np.asarray(p[:9]).reshape(3, 3)
    T[:3, 3] = p[9:12]
    return T


def addPlaneMotionSE3Expmap(Tcw, bTc, xrot_info=1e6, yrot_info=1e6, z_info=1.0):
    """optimizer.cpp:236-314 -> (measurement 4x4, information 6x6); the defaults are Config::PLANEMOTION_*_INFO"""
    meas = np.zeros(12); info = np.zeros(36)
    a, b = _pose12(Tcw), _pose12(bTc)
    capi.check(capi.lib().se2gpu_plane_motion_prior(a.ctypes.data, b.ctypes.data, float(xrot_info), float(yrot_info),
                                                    float(z_info), meas.ctypes.data, info.ctypes.data))
    return _matrix(meas), info.reshape(6, 6)


class Localizer:
    """Device workspace of the localisation thread."""

    def __init__(self):
        h = C.c_void_p()
        capi.check(capi.lib().se2gpu_track_create(C.byref(h)))
        self._h = h
        self.stats = None

    def DoLocalBA(self, Tcw, bTc, map_points, keypoints_uv, inv_sigma2, fx, cx, cy, th_huber, iterations=30,
                  plane_info=(1e6, 1e6, 1.0)):
        """Tcw: 4x4 pose of mpKFCurr; map_points (n,3) world positions of its good-parallax observations; keypoints_uv
        (n,2) = keyPointsUn[ftrIdx].pt; inv_sigma2 (n,) = mvInvLevelSigma2[octave]; th_huber = Config::TH_HUBER.
        -> optimised Tcw (4x4); self.stats holds the LM history."""
        meas, info = addPlaneMotionSE3Expmap(Tcw, bTc, *plane_info)
        return self.pose_ba(Tcw, meas, info, map_points, keypoints_uv, inv_sigma2, fx, cx, cy, th_huber, iterations)

    def pose_ba(self, Tcw, prior_meas, prior_info, xyz, uv, inv_sigma2, f, cx, cy, delta, iterations=30):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        w = np.ascontiguousarray(inv_sigma2, np.float64).reshape(-1)
        if not (len(xyz) == len(uv) == len(w)):
            raise ValueError("map points, key points and inv_sigma2 differ in length")
        a, m = _pose12(Tcw), _pose12(prior_meas)
        pi = np.ascontiguousarray(prior_info, np.float64).reshape(-1)
        out = np.zeros(12)
        # the statistics struct inside a larger buffer: the bytes behind it must come back untouched
        buf = (C.c_uint8 * (C.sizeof(capi.BaStats) + 64))()
        C.memset(C.byref(buf, C.sizeof(capi.BaStats)), 0xA5, 64)
        st = capi.BaStats.from_buffer(buf)
        capi.check(capi.lib().se2gpu_track_pose_ba(self._h, a.ctypes.data, m.ctypes.data, pi.ctypes.data, len(xyz),
                                                   xyz.ctypes.data, uv.ctypes.data, w.ctypes.data, float(f), float(cx),
                                                   float(cy), float(delta), int(iterations), out.ctypes.data, C.byref(st)))
        self.stats_tail_intact = all(b == 0xA5 for b in buf[C.sizeof(capi.BaStats):])
        n = min(st.iterations, 64)
        self.stats = dict(iterations=st.iterations, trials=st.trials, terminated=bool(st.terminated),
                          chi2_init=st.chi2_init, chi2_final=st.chi2_final, lambda_final=st.lambda_final,
                          chi2_hist=list(st.chi2_hist[:n]), lambda_hist=list(st.lambda_hist[:n]),
                          trials_hist=list(st.trials_hist[:n]))
        return _matrix(out)

    def __del__(self):
        try:
            if self._h:
                capi.lib().se2gpu_track_destroy(self._h)
                self._h = None
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------- the tables in device memory
# se2gpu_localizer_ba_batch_device: renewal, gate, DoLocalBA and setPose for a batch of frames, asynchronous on the matcher's stream

WS_ARRAYS = ("counts", "pose0", "prior_meas", "prior_info", "e_ftr", "xyz", "uv", "w")
STATUS = dict(ok=0, out_of_range=1, too_few_observations=5, non_finite=6)
INFO = ("n_features", "n_obs", "n_edges", "renewed", "duplicates", "flags", "zero0", "zero1")
FLAG_ENTRY, FLAG_OCTAVE = 1, 2


def ws_bytes(njobs, cap) -> int:
    return int(capi.lib().se2gpu_localizer_ba_ws_bytes(int(njobs), int(cap)))


def ws_layout(njobs, cap):
    """name -> (byte offset of job 0's slice, stride from job to job) of the gathered arrays inside d_ws"""
    off, stride = np.zeros(len(WS_ARRAYS), np.int64), np.zeros(len(WS_ARRAYS), np.int64)
    capi.check(capi.lib().se2gpu_localizer_ba_ws_layout(int(njobs), int(cap), capi.vp(off), capi.vp(stride), len(WS_ARRAYS)))
    return {n: (int(o), int(s)) for n, o, s in zip(WS_ARRAYS, off, stride)}


def read_gather(raw, lay, j):
    """the arrays job j left in the work space (raw: its bytes on the host), cut to the job's counts"""
    def arr(name, dtype, count):
        o, s = lay[name]
        return raw[o + s * j:o + s * j + count * np.dtype(dtype).itemsize].view(dtype).copy()
    cnt = arr("counts", np.int32, 8)
    E = int(cnt[2])
    return dict(counts=cnt, pose0=arr("pose0", np.float64, 12), prior_meas=arr("prior_meas", np.float64, 12),
                prior_info=arr("prior_info", np.float64, 36).reshape(6, 6), e_ftr=arr("e_ftr", np.int32, E),
                xyz=arr("xyz", np.float64, 3 * E).reshape(E, 3), uv=arr("uv", np.float64, 2 * E).reshape(E, 2),
                w=arr("w", np.float64, E))


def do_local_ba_batch_device(matcher, d_job_frame, njobs, nframes, d_frame_Tcw, d_frame_Twb, d_kps_un, d_counts, cap, d_ftr_mp,
                             d_kf_observed, d_match_idx_mp, d_pos, m, d_mp_null, d_good_prl, inv_level_sigma2, K, Tbc12, huber,
                             d_ws, d_status, d_pose_out, d_stats, d_info, *, xrot_info=1e6, yrot_info=1e6, z_info=1.0, iters=30,
                             min_obs=30):
    """Localizer::MatchLocalMap's renewal, the numMPCurr > 30 gate, DoLocalBA and setPose for njobs frames on the tables in device
    memory.  Every d_ argument is a capi.DeviceArray, a raw device pointer or None where the C ABI allows NULL; inv_level_sigma2
    (mvInvLevelSigma2), K (3x3) and Tbc12 are host arrays.  Asynchronous: matcher.sync() before an output is read."""
    isig = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    K = np.asarray(K, np.float32)
    tbc = np.ascontiguousarray(Tbc12, np.float64).reshape(12)
    capi.check(capi.lib().se2gpu_localizer_ba_batch_device(
        matcher._h, _ptr(d_job_frame), int(njobs), int(nframes), _ptr(d_frame_Tcw), _ptr(d_frame_Twb), _ptr(d_kps_un),
        _ptr(d_counts), int(cap), _ptr(d_ftr_mp), _ptr(d_kf_observed), _ptr(d_match_idx_mp), _ptr(d_pos), int(m), _ptr(d_mp_null),
        _ptr(d_good_prl), capi.vp(isig), len(isig), float(K[0, 0]), float(K[0, 2]), float(K[1, 2]), capi.vp(tbc), float(huber),
        float(xrot_info), float(yrot_info), float(z_info), int(iters), int(min_obs), _ptr(d_ws), _ptr(d_status), _ptr(d_pose_out),
        _ptr(d_stats), _ptr(d_info)))
