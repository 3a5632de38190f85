"""What se2gpu_track_frames_batch_device has to write for one (reference key frame, current frame) pair, in numpy over the
oracle: oracle.fundamental_mask_info for the mask of Track::removeOutliers (Track.cpp:308-344) and oracle.triangulate for
Track::doTriangulate (Track.cpp:378-419).  Both are held to the single device calls bit for bit and to the compiled reference
in tests/test_ref_compiled.py.

Rules, in the order of include/se2gpu.h:
  1  raw matches: entries i < counts[a] of the row with a value in 0..counts[b]-1 (counts clamped to 0..cap), ascending i
  2  filter: findFundamentalMat's mask over them; fewer than 10 inliers (always so below 10 raw matches) -> the row is -1
  3  triangulation unless flag bit 0: kf_observed[a][i] -> the key frame's map point; else DLT, depth gate, parallax flag
  4  every word of matched12 / local_pos / good_prl is written; info = INFO"""
import numpy as np

INFO = ("n_raw", "n_inliers", "n_tracked_old", "n_good_prl", "n_old_kp", "path", "n_depth_rejected", "status")
RUN, BAD_FRAME, FEW_INLIERS, SKIPPED = 0, 1, 2, 3
MIN_INLIERS = 10


def track_pair(oracle, kps, counts, cap, a, b, row, Trc, P, P_ref, lower, upper, min_degree, kf_observed=None, view_pos=None,
               flag=0):
    """kps (nframes, cap) structured key points, counts (nframes,) as given to the device (clamped here), row (cap,) the
    MatchByWindow row of the pair, Trc / P (12,) of the pair, P_ref (12,), kf_observed (nframes, cap) u8 or None with
    view_pos (nframes, cap, 3) f32, flag the pair's byte
    -> (matched12 (cap,) i32, local_pos (cap, 3) f32, good_prl (cap,) u8, info (8,) i32)"""
    nframes = len(counts)
    matched = np.full(cap, -1, np.int32)
    pos = np.zeros((cap, 3), np.float32)
    good = np.zeros(cap, np.uint8)
    info = np.zeros(8, np.int32)
    if not (0 <= a < nframes and 0 <= b < nframes):
        info[7] = BAD_FRAME
        return matched, pos, good, info
    na, nb = int(np.clip(counts[a], 0, cap)), int(np.clip(counts[b], 0, cap))
    if kf_observed is not None:
        info[4] = int(np.count_nonzero(kf_observed[a, :na]))
    row = np.asarray(row, np.int64)
    src = np.array([i for i in range(na) if 0 <= row[i] < nb], np.int64)    # rule 1
    info[0] = len(src)
    info[7] = FEW_INLIERS
    if len(src) < MIN_INLIERS:                                              # 7 points give 7 inliers, 8 or 9 at most 9
        return matched, pos, good, info
    dst = row[src]
    p1 = np.stack([kps["x"][a, src], kps["y"][a, src]], 1).astype(np.float32)
    p2 = np.stack([kps["x"][b, dst], kps["y"][b, dst]], 1).astype(np.float32)
    mask, r = oracle.fundamental_mask_info(p1, p2)                          # rule 2
    keep = mask.astype(bool)
    info[5] = 1 if len(src) < 15 else 2
    if int(keep.sum()) < MIN_INLIERS:
        return matched, pos, good, info
    info[1] = int(keep.sum())
    matched[src[keep]] = dst[keep]
    if flag & 1:                                                            # rule 3
        info[7] = SKIPPED
        return matched, pos, good, info
    info[7] = RUN
    obs = None if kf_observed is None else (kf_observed[a, :na] != 0).astype(np.uint8)
    Trc = np.asarray(Trc, np.float32).reshape(-1)
    Ocam = Trc[[3, 7, 11]]
    po, go, mo, ng, nold = oracle.triangulate(kps[a, :na], kps[b, :nb], matched[:na], obs, P_ref, P, Ocam, lower, upper, min_degree)
    info[6] = int(np.count_nonzero((matched[:na] >= 0) & (mo < 0)))
    matched[:na] = mo
    pos[:na] = po
    good[:na] = go
    if obs is not None:
        old = (mo >= 0) & (obs != 0)
        pos[:na][old] = view_pos[a, :na][old]
        assert nold == int(old.sum())
    info[2], info[3] = nold, ng
    assert ng == int(good.sum()) and not pos[matched < 0].any()
    return matched, pos, good, info


def track_batch(oracle, kps, counts, cap, pairs, rows, Trc, P, P_ref, lower, upper, min_degree, kf_observed=None, view_pos=None,
                flags=None):
    """-> (matched12 (npairs, cap), local_pos (npairs, cap, 3), good_prl (npairs, cap), info (npairs, 8)); equal pairs are
    computed once"""
    cache, out = {}, []
    for p, ((a, b), row) in enumerate(zip(pairs, rows)):
        f = 0 if flags is None else int(flags[p])
        key = (a, b, np.asarray(row).tobytes(), np.asarray(Trc[p], np.float32).tobytes(), np.asarray(P[p], np.float32).tobytes(), f)
        if key not in cache:
            cache[key] = track_pair(oracle, kps, counts, cap, a, b, row, Trc[p], P[p], P_ref, lower, upper, min_degree,
                                    kf_observed, view_pos, f)
        out.append(cache[key])
    return tuple(np.stack([o[k] for o in out]) for k in range(4))
