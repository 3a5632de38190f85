"""Python mirror of GlobalMapper::CreateFeatEdge (/root/reference/src/GlobalMapper.cpp:737-843) over se2gpu_feat_edge_batch -
harness for the tests and tools; the computation is the HIP kernels k_feat_edge and k_sparsify."""
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
        s = o["stats"][p]
        n = s.iterations
        res.append(dict(status=int(o["info4"][p, 0]), n_points=int(o["info4"][p, 1]), n_outliers=int(o["info4"][p, 2]),
                        n_sparsified=int(o["info4"][p, 3]), kf=pose44(o["kf"][p]), kf12=o["kf"][p].copy(), mp=o["mp"][a:b].copy(),
                        outlier=o["outlier"][a:b].astype(bool), edge_chi2=o["edge_chi2"][a:b].copy(),
                        stats=dict(iterations=n, trials=s.trials, terminated=s.terminated, chi2_init=s.chi2_init, chi2_final=s.chi2_final,
                                   lambda_final=s.lambda_final, chi2_hist=np.array(s.chi2_hist[:n]), lambda_hist=np.array(s.lambda_hist[:n]),
                                   trials_hist=np.array(s.trials_hist[:n])),
                        z=pose44(o["z"][p]) if o["info4"][p, 0] == 0 else np.zeros((4, 4)), z12=o["z"][p].copy(),
                        info=o["info"][p].reshape(6, 6).copy()))
    return res
