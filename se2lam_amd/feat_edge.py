"""Python mirror of GlobalMapper::CreateFeatEdge (/root/reference/src/GlobalMapper.cpp:737-843) over se2gpu_feat_edge_batch -
harness for the tests and tools; the computation is the HIP kernels k_feat_edge and k_sparsify - and over
se2gpu_feat_edge_batch_device, the same computation behind a gather kernel on tables that stay in device memory
(CreateFeatEdgeCovisBatchDevice / CreateFeatEdgeMatchBatchDevice)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, synth

COVIS, MATCH = 0, 1
# the reference's constants: OptKFPair (:911, :747), OptKFPairMatch (:985, :790, :989), addEdgeSE3XYZ's Huber delta (:901)
COVIS_ITERS, COVIS_MIN_POINTS, MATCH_ITERS, MATCH_MIN_POINTS, HUBER_DELTA, OUTLIER_CHI2 = 15, 10, 30, 3, 5.99, 5.0


def pose12(T):
    T = np.asarray(T, np.float64)
    return np.concatenate([T[..., :3, :3].reshape(T.shape[:-2] + (9,)), T[..., :3, 3]], axis=-1)


def pose44(p):
    p = np.asarray(p, np.float64)
    T = np.zeros(p.shape[:-1] + (4, 4))
    T[..., :3, :3] = p[..., :9].reshape(p.shape[:-1] + (3, 3))
    T[..., :3, 3] = p[..., 9:]
    T[..., 3, 3] = 1.0
    return T


def Tbc12(Rbc=synth.RBC, tbc=synth.TBC):
    return np.concatenate([np.asarray(Rbc, np.float64).reshape(9), np.asarray(tbc, np.float64)])


def flatten(pairs):
    """pairs: list of (kf (2,4,4) T_w_c, mp (N,3), z (N,2,3), info (N,2,3,3)) -> the arrays of se2gpu_feat_edge_batch"""
    n = len(pairs)
    kf = np.zeros((n, 2, 12))
    mp_ptr = np.zeros(n + 1, np.int32)
    for p, q in enumerate(pairs):
        kf[p] = pose12(q[0])
        mp_ptr[p + 1] = mp_ptr[p] + len(q[1])
    cat = lambda i, w: np.ascontiguousarray(np.concatenate([np.asarray(q[i], np.float64).reshape(-1, w) for q in pairs])
                                            if n else np.zeros((0, w)))
    return kf, mp_ptr, cat(1, 3), cat(2, 6), cat(3, 18)


def feat_edge_raw(npairs, mode, iters, min_points, kf, mp_ptr, mp, z, info, tbc=None, xrot=synth.PLANEMOTION_XROT_INFO,
                  yrot=synth.PLANEMOTION_XROT_INFO, zinfo=synth.PLANEMOTION_Z_INFO, huber_delta=HUBER_DELTA,
                  outlier_chi2=OUTLIER_CHI2):
    """the call itself on flat arrays -> (rc, dict of the output arrays)"""
    tbc = Tbc12() if tbc is None else np.ascontiguousarray(tbc, np.float64)
    NP = int(mp_ptr[npairs]) if npairs > 0 else 0
    out = dict(kf=np.zeros((max(npairs, 0), 2, 12)), mp=np.zeros((NP, 3)), outlier=np.zeros(NP, np.uint8), edge_chi2=np.zeros((NP, 2)),
               info4=np.zeros((max(npairs, 0), 4), np.int32), stats=(capi.BaStats * max(npairs, 1))(),
               z=np.zeros((max(npairs, 0), 12)), info=np.zeros((max(npairs, 0), 36)))
    rc = capi.lib().se2gpu_feat_edge_batch(npairs, mode, iters, min_points, kf.ctypes.data, tbc.ctypes.data, xrot, yrot, zinfo,
                                           mp_ptr.ctypes.data, mp.ctypes.data, z.ctypes.data, info.ctypes.data, huber_delta, outlier_chi2,
                                           out["kf"].ctypes.data, out["mp"].ctypes.data, out["outlier"].ctypes.data,
                                           out["edge_chi2"].ctypes.data, out["info4"].ctypes.data,
                                           C.cast(out["stats"], C.c_void_p), out["z"].ctypes.data, out["info"].ctypes.data)
    return rc, out


def _pair_dict(status, n_points, n_outliers, n_sparsified, kf12, mp, outlier, edge_chi2, s, z12, info36):
    n = s.iterations
    return dict(status=int(status), n_points=int(n_points), n_outliers=int(n_outliers), n_sparsified=int(n_sparsified),
                kf=pose44(kf12), kf12=kf12.copy(), mp=mp.copy(), outlier=outlier.astype(bool), edge_chi2=edge_chi2.copy(),
                stats=dict(iterations=n, trials=s.trials, terminated=s.terminated, chi2_init=s.chi2_init, chi2_final=s.chi2_final,
                           lambda_final=s.lambda_final, chi2_hist=np.array(s.chi2_hist[:n]), lambda_hist=np.array(s.lambda_hist[:n]),
                           trials_hist=np.array(s.trials_hist[:n])),
                z=pose44(z12) if status == 0 else np.zeros((4, 4)), z12=z12.copy(), info=info36.reshape(6, 6).copy())


# ---- se2gpu_feat_edge_batch_device: the same computation on tables in device memory

WS_ARRAYS = ("count", "kf12", "prior_meas", "prior_info", "xyz", "z", "info")   # se2gpu_feat_edge_ws_layout's order


def ws_layout(npairs, row_cap):
    """-> (bytes of d_ws, {name: byte offset} of the gathered arrays); host only"""
    off = (C.c_longlong * len(WS_ARRAYS))()
    capi.check(capi.lib().se2gpu_feat_edge_ws_layout(npairs, row_cap, C.cast(off, C.c_void_p), len(WS_ARRAYS)))
    return int(capi.lib().se2gpu_feat_edge_ws_bytes(npairs, row_cap)), dict(zip(WS_ARRAYS, (int(v) for v in off)))


def _dev(x, dtype):
    return x if x is None or isinstance(x, (capi.DeviceArray, int, C.c_void_p)) else capi.upload(x, dtype)


def _d2h(dev, offset, dtype, shape):
    out = np.empty(shape, dtype)
    if out.nbytes:
        capi.check(capi.lib().se2gpu_memcpy_d2h(capi.vp(out), C.c_void_p(dev.ptr.value + offset), out.nbytes))
    return out


class FeatEdgeDeviceBuffers:
    """d_ws and the outputs of se2gpu_feat_edge_batch_device for npairs x row_cap, allocated once and reused by every call of
    that shape.  The outputs start from capi's sentinels; with poison the work space starts from 0xA5 bytes (it needs no
    initialisation: the call fills every word it reads)."""

    def __init__(self, npairs, row_cap, points=True, stats=True, poison=True):
        self.npairs, self.row_cap = int(npairs), int(row_cap)
        n, NP = max(self.npairs, 1), max(self.npairs * self.row_cap, 1)
        self.ws_bytes, self.ws_off = ws_layout(self.npairs, self.row_cap)
        self.ws = capi.upload(np.full(self.ws_bytes, 0xA5, np.uint8)) if poison else capi.DeviceArray(self.ws_bytes)
        self.info8 = capi.upload(np.full((n, 8), capi.ISENT, np.int32))
        self.kf = capi.upload(np.full((n, 24), capi.SENT))
        self.z = capi.upload(np.full((n, 12), capi.SENT))
        self.info = capi.upload(np.full((n, 36), capi.SENT))
        self.mp = capi.upload(np.full((NP, 3), capi.SENT)) if points else None
        self.outlier = capi.upload(np.full(NP, capi.SENTINEL_DESC, np.uint8)) if points else None
        self.edge_chi2 = capi.upload(np.full((NP, 2), capi.SENT)) if points else None
        self.stats = capi.DeviceArray(n * C.sizeof(capi.BaStats)) if stats else None

    def read_gather(self):
        """the gathered arrays out of d_ws: count / raw / dropped / cut (n,), kf12 (n, 2, 12), prior_meas (n, 2, 12), prior_info
        (n, 2, 36), xyz (n, row_cap, 3), z (n, row_cap, 6), info (n, row_cap, 18); rows are meaningful below count"""
        n, r, o = self.npairs, self.row_cap, self.ws_off
        meta = _d2h(self.ws, o["count"], np.int32, (4, n))
        g = dict(count=meta[0], raw=meta[1], dropped=meta[2], cut=meta[3])
        for k, w in (("kf12", (n, 2, 12)), ("prior_meas", (n, 2, 12)), ("prior_info", (n, 2, 36)), ("xyz", (n, r, 3)), ("z", (n, r, 6)),
                     ("info", (n, r, 18))):
            g[k] = _d2h(self.ws, o[k], np.float64, w)
        return g

    def read(self):
        """per pair the dict of CreateFeatEdgeBatch (mp, outlier, edge_chi2: the pair's gathered points) with raw, dropped, cut
        and, with points, the whole rows mp_row / outlier_row / edge_chi2_row"""
        n, r = self.npairs, self.row_cap
        info8 = self.info8.to_numpy(np.int32, (max(n, 1), 8))
        kf, z, info = self.kf.to_numpy(np.float64, (max(n, 1), 24)), self.z.to_numpy(np.float64, (max(n, 1), 12)), \
            self.info.to_numpy(np.float64, (max(n, 1), 36))
        if self.mp is not None:
            mp, outl, chi = self.mp.to_numpy(np.float64, (n, r, 3)), self.outlier.to_numpy(np.uint8, (n, r)), \
                self.edge_chi2.to_numpy(np.float64, (n, r, 2))
        stats = (capi.BaStats * max(n, 1))()
        if self.stats is not None:
            raw = self.stats.to_numpy(np.uint8, (max(n, 1) * C.sizeof(capi.BaStats),))
            C.memmove(stats, raw.ctypes.data, C.sizeof(stats))
        res = []
        for p in range(n):
            c = int(info8[p, 1])
            have = self.mp is not None
            d = _pair_dict(info8[p, 0], c, info8[p, 2], info8[p, 3], kf[p].reshape(2, 12),
                           mp[p, :c] if have else np.zeros((0, 3)), outl[p, :c] if have else np.zeros(0, np.uint8),
                           chi[p, :c] if have else np.zeros((0, 2)), stats[p], z[p], info[p])
            d.update(raw=int(info8[p, 4]), dropped=int(info8[p, 5]), cut=int(info8[p, 6]), info8=info8[p].copy())
            if have:
                d.update(mp_row=mp[p].copy(), outlier_row=outl[p].copy(), edge_chi2_row=chi[p].copy())
            res.append(d)
        return res


def feat_edge_batch_device(matcher, buf: FeatEdgeDeviceBuffers, mode, pair_a, pair_b, nframes, Twc, pos, m, covis=None, match=None,
                           iters=None, min_points=None, tbc=None, xrot=synth.PLANEMOTION_XROT_INFO,
                           yrot=synth.PLANEMOTION_XROT_INFO, zinfo=synth.PLANEMOTION_Z_INFO, huber_delta=HUBER_DELTA,
                           outlier_chi2=OUTLIER_CHI2):
    """the call itself on device arrays, asynchronous on `matcher`'s stream -> rc.
    covis = (pair_out, common, list_cap, obs_view, obs_info, nobs); match = (matches, counts, cap, ftr_mp, view_pos, view_info)"""
    iters = (COVIS_ITERS if mode == COVIS else MATCH_ITERS) if iters is None else iters
    min_points = (COVIS_MIN_POINTS if mode == COVIS else MATCH_MIN_POINTS) if min_points is None else min_points
    tbc = Tbc12() if tbc is None else np.ascontiguousarray(tbc, np.float64)
    p = capi.dev_ptr
    cv = (None, None, 1, None, None, 0) if covis is None else covis
    mt = (None, None, 1, None, None, None) if match is None else match
    return capi.lib().se2gpu_feat_edge_batch_device(
        matcher._h, mode, iters, min_points, huber_delta, outlier_chi2, tbc.ctypes.data, xrot, yrot, zinfo,
        p(pair_a), p(pair_b), buf.npairs, nframes, p(Twc), p(pos), m, buf.row_cap,
        p(cv[0]), p(cv[1]), cv[2], p(cv[3]), p(cv[4]), cv[5], p(mt[0]), p(mt[1]), mt[2], p(mt[3]), p(mt[4]), p(mt[5]),
        p(buf.ws), p(buf.info8), p(buf.kf), p(buf.z), p(buf.info), p(buf.mp), p(buf.outlier), p(buf.edge_chi2), p(buf.stats))


def _rows(x, width, given):
    """the number of rows of a host table, or the caller's count for one that already lies in device memory"""
    if given is not None:
        return int(given)
    assert not isinstance(x, capi.DeviceArray), "a device table needs its size (nframes / m / nobs / npairs)"
    return np.size(x) // width


def CreateFeatEdgeCovisBatchDevice(matcher, pair_a, pair_b, Twc, pos, pair_out, common, list_cap, obs_view, obs_info, row_cap,
                                   npairs=None, nframes=None, m=None, nobs=None, buf=None, sync=True, **kw):
    """OptKFPair on the outputs of se2gpu_covis_pairs_device (pair_out (n, 4), common (n, list_cap, 3)) and the tables Twc
    (nframes, 12) float32, pos (m, 3), obs_view (nobs, 3), obs_info (nobs, 9): numpy arrays are uploaded first (harness),
    DeviceArrays are used where they lie (their sizes are then given).  One call and, with sync, one wait -> the
    FeatEdgeDeviceBuffers (read(), read_gather())."""
    n, nframes, m, nobs = _rows(pair_a, 1, npairs), _rows(Twc, 12, nframes), _rows(pos, 3, m), _rows(obs_view, 3, nobs)
    buf = FeatEdgeDeviceBuffers(n, row_cap) if buf is None else buf
    keep = [_dev(pair_a, np.int32), _dev(pair_b, np.int32), _dev(Twc, np.float32), _dev(pos, np.float32), _dev(pair_out, np.int32),
            _dev(common, np.int32), _dev(obs_view, np.float32), _dev(obs_info, np.float32)]
    capi.check(feat_edge_batch_device(matcher, buf, COVIS, keep[0], keep[1], nframes, keep[2], keep[3], m,
                                      covis=(keep[4], keep[5], list_cap, keep[6], keep[7], nobs), **kw))
    buf.keep = keep
    if sync:
        matcher.sync()
    return buf


def CreateFeatEdgeMatchBatchDevice(matcher, pair_a, pair_b, Twc, pos, matches, counts, cap, ftr_mp, view_pos, view_info, row_cap,
                                   npairs=None, nframes=None, m=None, buf=None, sync=True, **kw):
    """OptKFPairMatch on the d_matches_mp rows of se2gpu_track_loop_verify_batch_device (matches (n, cap)) and the tables counts
    (nframes,), ftr_mp (nframes, cap), view_pos (nframes, cap, 3), view_info (nframes, cap, 9), Twc, pos; as the covisibility
    mirror."""
    n, nframes, m = _rows(pair_a, 1, npairs), _rows(counts, 1, nframes), _rows(pos, 3, m)
    buf = FeatEdgeDeviceBuffers(n, row_cap) if buf is None else buf
    keep = [_dev(pair_a, np.int32), _dev(pair_b, np.int32), _dev(Twc, np.float32), _dev(pos, np.float32), _dev(matches, np.int32),
            _dev(counts, np.int32), _dev(ftr_mp, np.int32), _dev(view_pos, np.float32), _dev(view_info, np.float32)]
    capi.check(feat_edge_batch_device(matcher, buf, MATCH, keep[0], keep[1], nframes, keep[2], keep[3], m,
                                      match=(keep[4], keep[5], cap, keep[6], keep[7], keep[8]), **kw))
    buf.keep = keep
    if sync:
        matcher.sync()
    return buf


def CreateFeatEdgeBatch(pairs, mode, iters=None, min_points=None, **kw):
    """-> per pair a dict: status, kf (2,4,4), mp (N,3), outlier (N,) bool, edge_chi2 (N,2), n_outliers, n_sparsified, stats
    (iterations, trials, terminated, chi2_init, chi2_final, lambda_final, chi2_hist, lambda_hist, trials_hist),
    z (4,4) and info (6,6): the SE3Constraint"""
    iters = (COVIS_ITERS if mode == COVIS else MATCH_ITERS) if iters is None else iters
    min_points = (COVIS_MIN_POINTS if mode == COVIS else MATCH_MIN_POINTS) if min_points is None else min_points
    kf, mp_ptr, mp, z, info = flatten(pairs)
    rc, o = feat_edge_raw(len(pairs), mode, iters, min_points, kf, mp_ptr, mp, z, info, **kw)
    capi.check(rc)
    res = []
    for p in range(len(pairs)):
        a, b = int(mp_ptr[p]), int(mp_ptr[p + 1])
        res.append(_pair_dict(*o["info4"][p], o["kf"][p], o["mp"][a:b], o["outlier"][a:b], o["edge_chi2"][a:b], o["stats"][p],
                              o["z"][p], o["info"][p]))
    return res
