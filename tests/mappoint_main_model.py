"""Independent numpy model of MapPoint::updateMainKFandDescriptor (src/MapPoint.cpp:228-292 of the reference) for the tests
of se2gpu_mappoint_main_batch_device and of include/se2lam_amd/MapPointMain.h.  It shares no code with either: distances
from np.unpackbits, np.sort per row, index (N-1)//2, argmin (first wins), distances in float32 from float64."""
import numpy as np


def distance_table(desc):
    """desc (N, 32) uint8 -> (N, N) Hamming distances"""
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8), axis=1).astype(np.int16)
    return (bits[:, None, :] != bits[None, :, :]).sum(axis=2).astype(np.int64)


def main_of(desc):
    """-> (index of the main descriptor among the N given, its median)"""
    D = distance_table(desc)
    N = len(D)
    med = np.sort(D, axis=1)[:, (N - 1) // 2]
    i = int(np.argmin(med))          # the first of equal minima
    return i, int(med[i])


def valid_observations(obs_frame, obs_ftr, counts, cap, nframes, frame_null):
    """places in the list whose observation counts"""
    keep = []
    for i, (f, k) in enumerate(zip(obs_frame, obs_ftr)):
        if not 0 <= f < nframes:
            continue
        if frame_null is not None and frame_null[f]:
            continue
        if not 0 <= k < min(int(counts[f]), cap):
            continue
        keep.append(i)
    return keep


def min_max_dist(view, octave, scale_factors):
    x, y, z = (np.float64(v) for v in view)
    dist = np.float32(np.sqrt(x * x + y * y + z * z))
    mx = np.float32(dist * np.float32(scale_factors[octave]))
    mn = np.float32(mx / np.float32(scale_factors[-1]))
    return mn, mx


def update_main_batch(kps, desc, counts, cap, nframes, frame_null, view_pos, scale_factors, nlevels, mp_ptr, obs_frame,
                      obs_ftr, prev_main_frame, out):
    """kps: structured array with an 'octave' field (nframes * cap), desc (nframes * cap, 32), view_pos (nframes * cap, 3) or
    None; out: dict of info (m, 4) int32, main_desc (m, 32) uint8, main_frame (m,), main_octave (m,) int32, dist (m, 2) float32
    holding the values before the call.  Returns a new dict of the values after it."""
    o = {k: np.array(v, copy=True) for k, v in out.items()}
    m, nobs = len(mp_ptr) - 1, len(obs_frame)
    for p in range(m):
        s, e = (min(max(int(v), 0), nobs) for v in (mp_ptr[p], mp_ptr[p + 1]))   # clamped; a descending segment is empty
        fr, ft = obs_frame[s:max(e, s)], obs_ftr[s:max(e, s)]
        keep = valid_observations(fr, ft, counts, cap, nframes, frame_null)
        if not keep:
            o["info"][p] = (-1, 0, 0, 0)
            continue
        offs = [int(fr[i]) * cap + int(ft[i]) for i in keep]
        j, med = main_of(desc[offs])
        frame, off = int(fr[keep[j]]), offs[j]
        o["main_desc"][p] = desc[off]
        o["main_frame"][p] = frame
        changed = 1 if prev_main_frame is None or int(prev_main_frame[p]) != frame else 0
        if changed:
            octave = int(kps["octave"][off])
            o["main_octave"][p] = octave
            if not 0 <= octave < nlevels:
                changed |= 2
            elif view_pos is not None:
                o["dist"][p] = min_max_dist(view_pos[off], octave, scale_factors)
        o["info"][p] = (keep[j], med, len(keep), changed)
    return o
