"""Python mirror of the local-BA call over the C ABI (harness view; C++ twin: include/se2lam_amd/LocalBA.h).

Reference: Map::loadLocalGraph (src/Map.cpp:891-1053) and LocalMapper::localBA's optimize.  All compute happens in libse2gpu.so
(se2gpu_local_ba_batch_device, HIP): the lists of localwindow.window_device and the map's tables stay in device memory, the
graphs are gathered and solved there, and the results are read after one matcher.sync().
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import ISENT, SENT, dev_ptr as _ptr, upload as _up
from .covis import _Pending

WS_ARRAYS = ("counts", "fixed", "poses", "o_i", "o_j", "o_meas", "o_info", "lm_ptr", "e_kf", "e_uv", "e_info", "lms")
STATUS = dict(ok=0, out_of_range=1, does_not_fit=2, null_key_frame=3, degree=4, nothing_to_optimise=5, non_finite=6)


def ws_bytes(njobs, max_local, max_ref, max_mp, max_obs) -> int:
    return int(capi.lib().se2gpu_local_ba_ws_bytes(int(njobs), int(max_local), int(max_ref), int(max_mp), int(max_obs)))


def ws_layout(njobs, max_local, max_ref, max_mp, max_obs):
    """name -> (byte offset of job 0's slice, stride from job to job) of the gathered arrays inside d_ws"""
    off, stride = np.zeros(len(WS_ARRAYS), np.int64), np.zeros(len(WS_ARRAYS), np.int64)
    capi.check(capi.lib().se2gpu_local_ba_ws_layout(int(njobs), int(max_local), int(max_ref), int(max_mp), int(max_obs),
                                                    capi.vp(off), capi.vp(stride), len(WS_ARRAYS)))
    return {n: (int(o), int(s)) for n, o, s in zip(WS_ARRAYS, off, stride)}


def flatten_local_graph(T, local, ref, mps):
    """The host route's flattening: the window's lists and the map's host tables (a dict with the keys of DeviceTables' arguments
    plus K, Tbc12, huber, xrot_info, z_info; kps as kps_xy / kps_octave) -> the keyword arguments of optimizer.loadLocalGraph
    (se2gpu_local_graph).  The rules are those of the device call: the entry rule, members of either list, a frame once per
    point, octaves in range."""
    nframes, cap, nlevels = len(T["counts"]), int(T["cap"]), len(T["level_sigma2"])
    null = T.get("frame_null")
    slots = [int(f) for f in local] + [int(f) for f in ref]
    vertex = {f: i for i, f in reversed(list(enumerate(slots)))}
    nl = len(local)
    odo_to, odo_meas, odo_cov = np.full(nl, -1, np.int32), np.zeros((nl, 3)), np.tile(np.eye(3).reshape(-1), (nl, 1))
    if T.get("odo_to") is not None:
        for i, f in enumerate(slots[:nl]):
            t = int(T["odo_to"][f])
            if 0 <= t < nframes and vertex.get(t, nl) < nl and not (null is not None and null[t]):
                odo_to[i], odo_meas[i], odo_cov[i] = vertex[t], T["odo_meas"][f], np.reshape(T["odo_cov"][f], -1)
    obs_mp, obs_kf, obs_uv, obs_lc, obs_s2 = [], [], [], [], []
    nobs = len(T["obs_frame"])
    for l, p in enumerate(mps):
        s, e = (min(max(int(T["mp_ptr"][q]), 0), nobs) for q in (p, p + 1))
        seen = set()
        for i in range(s, e):
            f, k = int(T["obs_frame"][i]), int(T["obs_ftr"][i])
            if not 0 <= f < nframes or (null is not None and null[f]) or not 0 <= k < min(int(T["counts"][f]), cap):
                continue
            if f not in vertex or f in seen:
                continue
            seen.add(f)
            octave = int(T["kps_octave"][f, k])
            if not 0 <= octave < nlevels:
                continue
            obs_mp.append(l); obs_kf.append(vertex[f]); obs_uv.append(T["kps_xy"][f, k]); obs_lc.append(T["view_pos"][f, k])
            obs_s2.append(T["level_sigma2"][octave])
    Tcw = np.asarray(T["Tcw"], np.float32).reshape(nframes, 3, 4)
    tbc = np.asarray(T["Tbc12"], np.float64)
    return dict(kf_id=np.asarray(T["frame_id"])[slots], kf_Twb=np.asarray(T["Twb"])[slots], kf_Rcw=Tcw[slots][:, :, :3].reshape(-1, 9),
                n_local=nl, odo_to=odo_to, odo_meas=odo_meas, odo_cov=odo_cov, mp_pos=np.asarray(T["pos"])[list(mps)].reshape(-1, 3),
                obs_mp=np.array(obs_mp, np.int32), obs_kf=np.array(obs_kf, np.int32), obs_uv=np.array(obs_uv, np.float32).reshape(-1, 2),
                obs_lc=np.array(obs_lc, np.float32).reshape(-1, 3), obs_sigma2=np.array(obs_s2, np.float32), K=T["K"],
                Rbc=tbc[:9].reshape(3, 3), tbc=tbc[9:], huber=T["huber"], xrot_info=T["xrot_info"], z_info=T["z_info"])


def device_tables(T):
    """DeviceTables of a host map dict (kps_xy / kps_octave packed into key points)"""
    kps = np.zeros(T["kps_octave"].shape, capi.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = T["kps_xy"][..., 0], T["kps_xy"][..., 1], T["kps_octave"]
    return DeviceTables(T["frame_id"], T["Twb"], T["Tcw"], kps, T["counts"], T["view_pos"], T["level_sigma2"], T["pos"], T["mp_ptr"],
                        T["obs_frame"], T["obs_ftr"], frame_null=T.get("frame_null"), odo_to=T.get("odo_to"), odo_meas=T.get("odo_meas"),
                        odo_cov=T.get("odo_cov"))


class DeviceTables:
    """The frame, feature and point tables of a map in device memory.  Host arrays in: frame_id (nframes), Twb (nframes, 3),
    Tcw (nframes, 12), frame_null or None, odo_to / odo_meas / odo_cov or None, kps (nframes, cap) of capi.KP_DTYPE, counts,
    view_pos (nframes, cap, 3), level_sigma2 (stays on the host), pos (m, 3), mp_ptr, obs_frame, obs_ftr."""

    def __init__(self, frame_id, Twb, Tcw, kps, counts, view_pos, level_sigma2, pos, mp_ptr, obs_frame, obs_ftr, frame_null=None,
                 odo_to=None, odo_meas=None, odo_cov=None):
        self.nframes, self.cap = int(np.shape(kps)[0]), int(np.shape(kps)[1])
        self.m, self.nobs = int(len(mp_ptr) - 1), int(len(obs_frame))
        self.frame_id, self.Twb, self.Tcw = _up(frame_id, np.int32), _up(Twb, np.float32), _up(Tcw, np.float32)
        self.frame_null = None if frame_null is None else _up(frame_null, np.uint8)
        self.odo_to = None if odo_to is None else _up(odo_to, np.int32)
        self.odo_meas = None if odo_to is None else _up(odo_meas, np.float64)
        self.odo_cov = None if odo_to is None else _up(odo_cov, np.float64)
        self.kps = _up(np.ascontiguousarray(kps, capi.KP_DTYPE))
        self.counts, self.view_pos = _up(counts, np.int32), _up(view_pos, np.float32)
        self.level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
        self.pos = _up(pos, np.float32)
        self.mp_ptr, self.obs_frame, self.obs_ftr = _up(mp_ptr, np.int32), _up(obs_frame, np.int32), _up(obs_ftr, np.int32)


def local_ba_device(matcher, T: DeviceTables, job_kf, win_out, local_list, ref_list, kf_list_cap, mp_list, mp_list_cap, *, K, Tbc12,
                    huber, xrot_info=1e6, z_info=1.0, iters=10, mode=0, max_local, max_ref, max_mp, max_obs, sync=True):
    """se2gpu_local_ba_batch_device.  job_kf, win_out and the three lists are host arrays or the device arrays
    se2gpu_local_window_batch_device wrote.  Returns dict(status (n,), kf_out (n, max_local + max_ref, 3), mp_out (n, max_mp, 3),
    stats [dict], info (n, 8), gather(j) -> the job's gathered arrays read through ws_layout); with sync=False an object whose
    read() gives it after matcher.sync().  Rows the call leaves alone hold capi.SENT / capi.ISENT."""
    dev = lambda a: a if isinstance(a, capi.DeviceArray) else _up(a, np.int32)  # noqa: E731
    n = int(len(job_kf)) if not isinstance(job_kf, capi.DeviceArray) else int(job_kf.nbytes // 4)
    d_job, d_out, d_ll, d_rl, d_ml = dev(job_kf), dev(win_out), dev(local_list), dev(ref_list), dev(mp_list)
    PK = int(max_local) + int(max_ref)
    nbytes = ws_bytes(n, max_local, max_ref, max_mp, max_obs)
    ws = capi.DeviceArray(max(nbytes, 16))
    status = _up(np.full(max(n, 1), ISENT, np.int32))
    kf_out = _up(np.full((max(n, 1), PK, 3), SENT, np.float64))
    mp_out = _up(np.full((max(n, 1), int(max_mp), 3), SENT, np.float64))
    stats = capi.DeviceArray(max(n, 1) * C.sizeof(capi.BaStats))
    info = _up(np.full((max(n, 1), 8), ISENT, np.int32))
    K = np.asarray(K, np.float32)
    tbc = np.ascontiguousarray(Tbc12, np.float64).reshape(12)
    capi.check(capi.lib().se2gpu_local_ba_batch_device(
        matcher._h, _ptr(d_job), n, _ptr(d_out), _ptr(d_ll), _ptr(d_rl), int(kf_list_cap), _ptr(d_ml), int(mp_list_cap),
        T.nframes, _ptr(T.frame_id), _ptr(T.Twb), _ptr(T.Tcw), _ptr(T.frame_null), _ptr(T.odo_to), _ptr(T.odo_meas),
        _ptr(T.odo_cov), _ptr(T.kps), _ptr(T.counts), T.cap, _ptr(T.view_pos), capi.vp(T.level_sigma2), len(T.level_sigma2),
        _ptr(T.pos), T.m, _ptr(T.mp_ptr), _ptr(T.obs_frame), _ptr(T.obs_ftr), T.nobs, float(K[0, 0]), float(K[0, 2]),
        float(K[1, 2]), capi.vp(tbc), float(huber), float(xrot_info), float(z_info), int(iters), int(mode), int(max_local),
        int(max_ref), int(max_mp), int(max_obs), _ptr(ws), _ptr(status), _ptr(kf_out), _ptr(mp_out), _ptr(stats), _ptr(info)))

    def read():
        from .optimizer import _stats_dict
        raw = ws.to_numpy(np.uint8, (max(nbytes, 16),)) if n else np.zeros(16, np.uint8)
        lay = ws_layout(n, max_local, max_ref, max_mp, max_obs) if n else {}
        st_raw = stats.to_numpy(np.uint8, (max(n, 1) * C.sizeof(capi.BaStats),))
        st = [capi.BaStats.from_buffer_copy(st_raw[i * C.sizeof(capi.BaStats):(i + 1) * C.sizeof(capi.BaStats)].tobytes())
              for i in range(n)]

        def gather(j):
            """the arrays the gather wrote for job j, cut to the job's counts"""
            def arr(name, dtype, count):
                o, s = lay[name]
                return raw[o + s * j:o + s * j + count * np.dtype(dtype).itemsize].view(dtype).copy()
            cnt = arr("counts", np.int32, 8)
            P, L, E, O = int(cnt[0]), int(cnt[2]), int(cnt[3]), int(cnt[4])
            return dict(counts=cnt, fixed=arr("fixed", np.uint8, P), poses=arr("poses", np.float64, 3 * P).reshape(P, 3),
                        o_i=arr("o_i", np.int32, O), o_j=arr("o_j", np.int32, O), o_meas=arr("o_meas", np.float64, 3 * O).reshape(O, 3),
                        o_info=arr("o_info", np.float64, 9 * O).reshape(O, 3, 3), lm_ptr=arr("lm_ptr", np.int32, L + 1),
                        e_kf=arr("e_kf", np.int32, E), e_uv=arr("e_uv", np.float64, 2 * E).reshape(E, 2),
                        e_info=arr("e_info", np.float64, 3 * E).reshape(E, 3), lms=arr("lms", np.float64, 3 * L).reshape(L, 3))
        return dict(status=status.to_numpy(np.int32, (max(n, 1),))[:n], kf_out=kf_out.to_numpy(np.float64, (max(n, 1), PK, 3))[:n],
                    mp_out=mp_out.to_numpy(np.float64, (max(n, 1), int(max_mp), 3))[:n], stats=[_stats_dict(s) for s in st],
                    info=info.to_numpy(np.int32, (max(n, 1), 8))[:n], gather=gather)
    if not sync:
        return _Pending((d_job, d_out, d_ll, d_rl, d_ml, T, ws, tbc), read)
    matcher.sync()
    return read()
