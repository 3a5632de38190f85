"""A numpy statement of the two gathers of se2gpu_feat_edge_batch_device, written from the rules of its header comment and
from GlobalMapper::CreateFeatEdge / OptKFPair / OptKFPairMatch (GlobalMapper.cpp:741-750, :790, :956-976) - not from the kernel.
Plain loops, one entry at a time.  Every function returns a dict:
    count, raw, dropped, cut   (npairs,) int32
    kf12                       (npairs, 2, 12) float64: rotation (9, row-major), translation (3)
    xyz, z, info               lists over pairs of (count, 3), (count, 6), (count, 18) float64 arrays, in gathered order
"""
import numpy as np


def kf12_of_slot(Twc, slot, nframes):
    """rows 0-2 of a 3 x 4 float matrix -> rotation, translation in double; a slot out of range gives the identity"""
    if not 0 <= slot < nframes:
        return np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    T = np.asarray(Twc, np.float32).reshape(-1, 3, 4)[slot].astype(np.float64)
    return np.concatenate([T[:, :3].ravel(), T[:, 3]])


def _finish(npairs, rows, meta, kf12):
    cat = lambda k, w: [np.array([r[k] for r in pr], np.float64).reshape(-1, w) for pr in rows]   # noqa: E731
    m = np.array(meta, np.int32).reshape(npairs, 4)
    return dict(count=m[:, 0], raw=m[:, 1], dropped=m[:, 2], cut=m[:, 3], kf12=np.array(kf12, np.float64).reshape(npairs, 2, 12),
                xyz=cat(0, 3), z=cat(1, 6), info=cat(2, 18))


def gather_covis(pair_a, pair_b, nframes, Twc, pos, row_cap, pair_out, common, list_cap, obs_view, obs_info):
    """pair_out (npairs, 4), common (npairs, list_cap, 3) as se2gpu_covis_pairs_device writes them; pos (m, 3), obs_view (nobs, 3),
    obs_info (nobs, 9) float32"""
    pos, obs_view, obs_info = (np.asarray(x, np.float32).reshape(-1, w) for x, w in ((pos, 3), (obs_view, 3), (obs_info, 9)))
    m, nobs = len(pos), len(obs_view)
    common = np.asarray(common, np.int32).reshape(len(pair_a), list_cap, 3)
    rows, meta, kf12 = [], [], []
    for p, (a, b) in enumerate(zip(pair_a, pair_b)):
        kf12.append([kf12_of_slot(Twc, a, nframes), kf12_of_slot(Twc, b, nframes)])
        n_same = int(pair_out[p][0])
        pr = []
        if n_same < 0 or not (0 <= a < nframes and 0 <= b < nframes):     # a pair of no points
            rows.append(pr)
            meta.append((0, n_same, 0, 0))
            continue
        taken = min(n_same, list_cap, row_cap)
        for i in range(taken):
            pt, ea, eb = (int(v) for v in common[p, i])
            if 0 <= pt < m and 0 <= ea < nobs and 0 <= eb < nobs:
                pr.append((pos[pt].astype(np.float64), np.concatenate([obs_view[ea], obs_view[eb]]).astype(np.float64),
                           np.concatenate([obs_info[ea], obs_info[eb]]).astype(np.float64)))
        rows.append(pr)
        meta.append((len(pr), n_same, taken - len(pr), int(n_same > min(list_cap, row_cap))))
    return _finish(len(pair_a), rows, meta, kf12)


def gather_match(pair_a, pair_b, nframes, Twc, pos, row_cap, matches, counts, cap, ftr_mp, view_pos, view_info):
    """matches (npairs, cap) in the layout of the verify call's d_matches_mp; ftr_mp (nframes, cap); view_pos (nframes, cap, 3),
    view_info (nframes, cap, 9) float32"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    m = len(pos)
    matches = np.asarray(matches, np.int32).reshape(len(pair_a), cap)
    ftr_mp = np.asarray(ftr_mp, np.int32).reshape(nframes, cap)
    view_pos = np.asarray(view_pos, np.float32).reshape(nframes, cap, 3)
    view_info = np.asarray(view_info, np.float32).reshape(nframes, cap, 9)
    rows, meta, kf12 = [], [], []
    for p, (a, b) in enumerate(zip(pair_a, pair_b)):
        kf12.append([kf12_of_slot(Twc, a, nframes), kf12_of_slot(Twc, b, nframes)])
        pr, raw, points = [], 0, 0
        if 0 <= a < nframes and 0 <= b < nframes:
            na, nb = (min(max(int(counts[s]), 0), cap) for s in (a, b))
            for i in range(na):                                 # ascending i: the order of std::map<int,int>
                j = int(matches[p, i])
                if not 0 <= j < nb:
                    continue
                raw += 1
                fa, fb = int(ftr_mp[a, i]), int(ftr_mp[b, j])
                if not (0 <= fa < m and fb >= 0):               # :960-965
                    continue
                points += 1
                if points <= row_cap:
                    pr.append((pos[fa].astype(np.float64), np.concatenate([view_pos[a, i], view_pos[b, j]]).astype(np.float64),
                               np.concatenate([view_info[a, i], view_info[b, j]]).astype(np.float64)))
        rows.append(pr)
        meta.append((len(pr), raw, raw - points, int(points > row_cap)))
    return _finish(len(pair_a), rows, meta, kf12)


def host_call_arrays(g):
    """the gathered rows as the arrays of se2gpu_feat_edge_batch: kf (n, 2, 12), mp_ptr, mp (NP, 3), z (NP, 6), info (NP, 18)"""
    n = len(g["count"])
    mp_ptr = np.zeros(n + 1, np.int32)
    mp_ptr[1:] = np.cumsum(g["count"])
    cat = lambda k, w: np.ascontiguousarray(np.concatenate(g[k] + [np.zeros((0, w))]))   # noqa: E731
    return np.ascontiguousarray(g["kf12"]), mp_ptr, cat("xyz", 3), cat("z", 6), cat("info", 18)
