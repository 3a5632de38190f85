#!/usr/bin/env python3
"""MapPoint::updateMainKFandDescriptor for batches of points: se2gpu_mappoint_main_batch_device with the data resident in
device memory against include/se2lam_amd/MapPointMain.h's mainObservation on ONE host thread over the same data
(tools/mappoint_main_host.cpp, g++ -O2), and se2gpu_match_projection_device against the host-buffer call at one scene size.

    python tools/mappoint_main_bench.py [--out profiles/mappoint_main.json]

Inputs (seed 7): 120 frames of 1024 features whose descriptors are noisy copies (4 % of the bits) of 2000 landmark descriptors;
256 / 4,096 / 20,000 points; observation counts geometric with mean 6 (at least 1), and 1 % of the points with 60..130
observations, each a random feature of a random frame - the stated stand-in, the drop-in run's own distribution was not dumped.
Device: after two warm-up calls, windows of at least 0.3 s of call + se2gpu_matcher_sync (host clock; what a caller who
needs the result waits for) and, separately, device events around 50 calls queued back to back (the stream's time per call);
medians over 7 windows with the 10th / 90th percentile.  Host: the same windows around passes over the batch.  The device's
info rows are compared with the host's before anything is timed.  No figure is gated."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from se2lam_amd import capi, mappoint as mpt  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

SIZES = [256, 4096, 20000]
NFRAMES, CAP, NLEVELS = 120, 1024, 8


def windows(fn, min_window=0.3, n_windows=7):
    fn(); fn()
    out = []
    for _ in range(n_windows):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= min_window:
                break
        out.append(1e3 * dt / n)
    out.sort()
    return {"median_ms": statistics.median(out), "p10_ms": out[1], "p90_ms": out[-2], "windows": len(out)}


def observation_counts(rng, m):
    n = rng.geometric(1 / 6.0, m)
    big = rng.random(m) < 0.01
    n[big] = rng.integers(60, 131, int(big.sum()))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true",
                    help="20 batch calls of 20,000 points and nothing else: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    rng = np.random.default_rng(7)
    nfeat = NFRAMES * CAP
    kps = np.zeros(nfeat, capi.KP_DTYPE)
    kps["octave"] = rng.integers(0, NLEVELS, nfeat)
    land = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
    desc = land[rng.integers(0, 2000, nfeat)] ^ np.packbits(rng.random((nfeat, 256)) < 0.04, axis=1)
    counts = np.full(NFRAMES, CAP, np.int32)
    view = (rng.standard_normal((nfeat, 3)) * 4).astype(np.float32)
    sf = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)
    frames = mpt.DeviceFrames(kps, desc, counts, CAP, None, view)
    mt = ORBmatcher()
    if a.trace_run:
        nob = observation_counts(rng, SIZES[-1])
        batch = mpt.MainBatch([(rng.integers(0, NFRAMES, n).astype(np.int32), rng.integers(0, CAP, n).astype(np.int32)) for n in nob])
        for _ in range(20):
            batch.run(mt, frames, sf)
        mt.sync()
        return
    tmp = tempfile.mkdtemp(prefix="mappoint_main_")
    exe = os.path.join(tmp, "mappoint_main_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "mappoint_main_host.cpp"), "-o", exe])
    rows = []
    for m in SIZES:
        nob = observation_counts(rng, m)
        lists = [(rng.integers(0, NFRAMES, n).astype(np.int32), rng.integers(0, CAP, n).astype(np.int32)) for n in nob]
        batch = mpt.MainBatch(lists)
        batch.run(mt, frames, sf)
        got = batch.download(mt)
        ptr, fr, ft = mpt.csr(lists)
        d = os.path.join(tmp, str(m))
        os.makedirs(d)
        for name, arr in (("head.i32", np.array([NFRAMES, CAP, NLEVELS, m, len(fr)], np.int32)), ("counts.i32", counts),
                          ("octave.i32", kps["octave"].astype(np.int32)), ("desc.u8", desc), ("view.f32", view), ("sf.f32", sf),
                          ("ptr.i32", ptr), ("frame.i32", fr), ("ftr.i32", ft)):
            np.ascontiguousarray(arr).tofile(os.path.join(d, name))
        host = subprocess.run([exe, d], capture_output=True, text=True, check=True).stdout.split()
        host_info = np.fromfile(os.path.join(d, "host_info.i32"), np.int32).reshape(m, 4)
        assert np.array_equal(host_info, got["info"]), "device and host mirror disagree"

        def call():
            batch.run(mt, frames, sf)
            mt.sync()
        dev = windows(call)
        ev = []
        timer = capi.Timer()
        for _ in range(7):
            timer.start(mt.stream())
            for _ in range(50):
                batch.run(mt, frames, sf)
            timer.stop(mt.stream())
            mt.sync()
            ev.append(timer.elapsed_ms() / 50)
        ev.sort()
        row = {"points": m, "observations": int(len(fr)), "longest": int(nob.max()),
               "pair_distances": int((nob.astype(np.int64) * (nob - 1) // 2).sum()),
               "device_call_and_sync": dev, "device_stream_ms_per_call": {"median_ms": ev[3], "p10_ms": ev[1], "p90_ms": ev[5]},
               "host_one_thread": {"median_ms": float(host[2]), "p10_ms": float(host[3]), "p90_ms": float(host[4]), "windows": int(host[1])}}
        row["host_over_device"] = row["host_one_thread"]["median_ms"] / dev["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)

    # MatchByProjection: device arrays against host buffers, one scene (900 features, 700 map points, tests' scene)
    from test_mappoint_main_gpu import _scene
    mp_pos, mp_desc, mp_octave, mp_skip, Tcw, K4, skps, sdesc, kf_obs = _scene()
    n, m = len(skps), len(mp_octave)
    up = capi.upload
    dv = [up(x) for x in (mp_pos, mp_desc, mp_octave, mp_skip, skps, sdesc, kf_obs)]
    d_idx, d_nm = up(np.zeros(n, np.int32)), up(np.zeros(1, np.int32))

    def host_call():
        mt.MatchByProjection(mp_pos, mp_desc, mp_octave, mp_skip, Tcw, K4, skps, sdesc, kf_obs, 15, 2)

    def dev_call():
        mt.match_projection_device(dv[0].ptr, dv[1].ptr, dv[2].ptr, dv[3].ptr, m, Tcw, K4, dv[4].ptr, dv[5].ptr, dv[6].ptr, n, 15, 2,
                                   d_idx.ptr, d_nm.ptr)
        mt.sync()
    nm_h, idx_h = mt.MatchByProjection(mp_pos, mp_desc, mp_octave, mp_skip, Tcw, K4, skps, sdesc, kf_obs, 15, 2)
    dev_call()
    assert np.array_equal(d_idx.to_numpy(np.int32, (n,)), idx_h) and int(d_nm.to_numpy(np.int32, (1,))[0]) == nm_h
    proj = {"features": n, "map_points": m, "matches": int(nm_h), "host_buffers": windows(host_call), "device_arrays_and_sync": windows(dev_call)}
    print(json.dumps(proj), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"mappoint_main": rows, "match_projection": proj}, f, indent=1)


if __name__ == "__main__":
    main()
