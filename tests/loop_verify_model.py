"""What se2gpu_track_loop_verify_batch_device has to write for one pair of key frames, in numpy over the oracle's restatement
of cv::findFundamentalMat (oracle.fundamental_mask_info, the one the single-pair path is held to).  The rules are the
reference's RemoveMatchOutlierRansac (GlobalMapper.cpp:1207-1248, Localizer.cpp:571-612: map order, numMinMatch = 10) and
RemoveKPMatch (GlobalMapper.cpp:1251-1276)."""
import numpy as np

INFO = ("n_raw", "n_good", "n_good_mp", "n_mps_a", "path", "sample", "model", "iterations")
NUM_MIN_MATCH = 10


def verify_pair(oracle, kps, counts, cap, a, b, row, has_mp=None, num_mps=None):
    """kps (nframes, cap) structured key points, counts (nframes,) as given to the device (clamped here), row (cap,) the match
    row of the pair, has_mp (nframes, cap) or None, num_mps (nframes,) or None
    -> (good row (cap,), mp row (cap,) or None, info (8,) int32)"""
    nframes = len(counts)
    good = np.full(cap, -1, np.int32)
    mp = None if has_mp is None else np.full(cap, -1, np.int32)
    info = np.array([0, 0, 0, 0, 0, -1, -1, 0], np.int32)
    if not (0 <= a < nframes and 0 <= b < nframes):
        return good, mp, info
    na, nb = int(np.clip(counts[a], 0, cap)), int(np.clip(counts[b], 0, cap))
    if num_mps is not None:
        info[3] = num_mps[a]
    elif has_mp is not None:
        info[3] = int(np.count_nonzero(has_mp[a, :na]))
    row = np.asarray(row, np.int64)
    src = np.array([i for i in range(na) if 0 <= row[i] < nb], np.int64)    # ascending i: the order of std::map<int,int>
    info[0] = len(src)
    if len(src) < NUM_MIN_MATCH:
        return good, mp, info
    dst = row[src]
    p1 = np.stack([kps["x"][a, src], kps["y"][a, src]], 1).astype(np.float32)
    p2 = np.stack([kps["x"][b, dst], kps["y"][b, dst]], 1).astype(np.float32)
    mask, r = oracle.fundamental_mask_info(p1, p2)
    keep = mask.astype(bool)
    good[src[keep]] = dst[keep]
    info[1] = int(keep.sum())
    info[4] = 1 if len(src) < 15 else 2
    info[5], info[6], info[7] = r["sample"], r["model"], r["iterations"]
    assert r["inliers"] == info[1]
    if has_mp is not None:
        keep_mp = keep & (has_mp[a, src] != 0) & (has_mp[b, dst] != 0)
        mp[src[keep_mp]] = dst[keep_mp]
        info[2] = int(keep_mp.sum())
    return good, mp, info


def verify_batch(oracle, kps, counts, cap, pairs, rows, has_mp=None, num_mps=None):
    """-> (good (npairs, cap), mp (npairs, cap) or None, info (npairs, 8)); equal (a, b, row) are computed once"""
    cache, out = {}, []
    for (a, b), row in zip(pairs, rows):
        key = (a, b, np.asarray(row).tobytes())
        if key not in cache:
            cache[key] = verify_pair(oracle, kps, counts, cap, a, b, row, has_mp, num_mps)
        out.append(cache[key])
    good = np.stack([o[0] for o in out])
    mp = None if has_mp is None else np.stack([o[1] for o in out])
    return good, mp, np.stack([o[2] for o in out])
