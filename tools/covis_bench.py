#!/usr/bin/env python3
"""Covisibility for batches of key-frame jobs: se2gpu_covis_build_device, _pairs_device and _refset_device with the tables
resident in device memory against the host functions of include/se2lam_amd/Covisibility.h on ONE host thread over the same
tables (tools/covis_host.cpp, g++ -O2).

    python tools/covis_bench.py [--out profiles/covis.json] [--md profiles/covis.md] [--stamp COMMIT]

The map (seed 7): 256 key-frame slots, 20,000 points with 3-8 observations each among the 13 slots around a centre slot (a
point is seen by key frames close in time), 10 % null, 30 % not good parallax; cap 1024.  A job is one new key frame: one
Map::updateCovisibility row (the new key frame against its 50 nearest slots = 50 pairs) plus one redundancy test per local key
frame (each against its 10 nearest slots, k = 2, 0.8 = 50 reference-set jobs).  1, 16 and 256 jobs.
Device: after two warm-up calls, windows of at least 0.3 s of call + se2gpu_matcher_sync (host clock) and device events around
50 calls queued back to back; medians over 7 windows with the 10th / 90th percentile.  The chain is build -> pairs -> refset
queued on one stream with one wait.  The build does not depend on the number of jobs (it is the whole map every time).
Host: CovisHostView::index() (what the build is on the device: the key frames' observation containers from the CSR), then
updateCovisibility and isRedundant per job; median over 5 windows.  The device's flags are compared with the host's before
anything is timed.  No figure is gated.  Not measured: counters, occupancy, kernel times under a profiler."""
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

from se2lam_amd import capi, covis  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

NFRAMES, M, CAP, NLOCAL, NREF = 256, 20000, 1024, 50, 10


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


def stream_ms(mt, fn):
    """device events around 50 calls queued back to back, per call"""
    ev, timer = [], capi.Timer()
    for _ in range(7):
        timer.start(mt.stream())
        for _ in range(50):
            fn()
        timer.stop(mt.stream())
        mt.sync()
        ev.append(timer.elapsed_ms() / 50)
    ev.sort()
    return {"median_ms": ev[3], "p10_ms": ev[1], "p90_ms": ev[5]}


def the_map(rng):
    n = rng.integers(3, 9, M)
    ptr = np.zeros(M + 1, np.int32)
    ptr[1:] = np.cumsum(n)
    centre = rng.integers(0, NFRAMES, M)
    obs_frame = np.concatenate([(c + rng.choice(13, k, replace=False) - 6) % NFRAMES for c, k in zip(centre, n)]).astype(np.int32)
    obs_ftr = np.zeros(len(obs_frame), np.int32)
    nxt = np.zeros(NFRAMES, np.int64)
    for i, f in enumerate(obs_frame):
        obs_ftr[i] = nxt[f]
        nxt[f] += 1
    assert nxt.max() <= CAP
    return dict(counts=np.full(NFRAMES, CAP, np.int32), ptr=ptr, obs_frame=obs_frame, obs_ftr=obs_ftr,
                null=(rng.random(M) < 0.1).astype(np.uint8), good=(rng.random(M) < 0.7).astype(np.uint8))


def nearest(f, k):
    """the k slots nearest to f on the ring, f excluded"""
    return np.array([(f + (1 + i // 2) * (1 if i % 2 == 0 else -1)) % NFRAMES for i in range(k)], np.int32)


def jobs_of(J, rng):
    new = rng.permutation(NFRAMES)[:J].astype(np.int32)
    local = np.stack([nearest(f, NLOCAL) for f in new])
    refs = np.stack([nearest(f, NREF) for f in local.ravel()])
    return new, local, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--stamp", default="unknown")
    ap.add_argument("--sizes", default="1,16,256")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    tmp = tempfile.mkdtemp(prefix="covis_")
    exe = os.path.join(tmp, "covis_host")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "covis_host.cpp"), "-o", exe, "-L", libdir, "-lse2gpu", "-Wl,-rpath," + libdir])
    mt = ORBmatcher()
    mp = the_map(np.random.default_rng(7))
    cv = covis.DeviceCovis(mp["counts"], CAP, mp["ptr"], mp["obs_frame"], mp["obs_ftr"], mp["null"], mp["good"])
    lib, up = capi.lib(), capi.upload
    rows = []
    for J in [int(x) for x in a.sizes.split(",")]:
        new, local, refs = jobs_of(J, np.random.default_rng(11))
        npairs = J * NLOCAL
        d_a, d_b = up(np.repeat(new, NLOCAL), np.int32), up(local, np.int32)
        d_kf, d_rp, d_ri = up(local, np.int32), up(NREF * np.arange(npairs + 1), np.int32), up(refs, np.int32)
        d_pout, d_prat = up(np.zeros((npairs, 4)), np.int32), up(np.zeros((npairs, 2)), np.float32)
        d_jout, d_jrat = up(np.zeros((npairs, 3)), np.int32), up(np.zeros(npairs), np.float64)

        def build():
            cv.build(mt, sync=False)

        def pairs():
            capi.check(lib.se2gpu_covis_pairs_device(mt._h, cv.bits.ptr, NFRAMES, M, d_a.ptr, d_b.ptr, npairs, 0.3, 0.1, d_pout.ptr,
                                                     d_prat.ptr, None, 0, None, 0, None, None, None, 0))

        def refset():
            capi.check(lib.se2gpu_covis_refset_device(mt._h, cv.bits.ptr, NFRAMES, M, d_kf.ptr, d_rp.ptr, d_ri.ptr, npairs * NREF,
                                                      npairs, 2, 0.8, d_jout.ptr, d_jrat.ptr))

        def synced(*fns):
            def f():
                for g in fns:
                    g()
                mt.sync()
            return f
        synced(build, pairs, refset)()
        flags = d_pout.to_numpy(np.int32, (npairs, 4))[:, 3] & 1
        red = d_jout.to_numpy(np.int32, (npairs, 3))[:, 2]
        d = os.path.join(tmp, str(J))
        os.makedirs(d)
        for name, arr in (("head.i32", np.array([NFRAMES, CAP, M, len(mp["obs_frame"]), J, NLOCAL, NREF], np.int32)),
                          ("counts.i32", mp["counts"]), ("ptr.i32", mp["ptr"]), ("obs_frame.i32", mp["obs_frame"]),
                          ("obs_ftr.i32", mp["obs_ftr"]), ("null.u8", mp["null"]), ("good.u8", mp["good"]), ("job_new.i32", new),
                          ("local.i32", local), ("refs.i32", refs)):
            np.ascontiguousarray(arr).tofile(os.path.join(d, name))
        host = subprocess.run([exe, d], capture_output=True, text=True, check=True).stdout.split()
        assert np.array_equal(np.fromfile(os.path.join(d, "host_connect.u8"), np.uint8), flags), "device and host connect other key frames"
        assert np.array_equal(np.fromfile(os.path.join(d, "host_redundant.u8"), np.uint8), red), "device and host disagree on redundancy"
        h = lambda i: {"median_ms": float(host[i]), "p10_ms": float(host[i + 1]), "p90_ms": float(host[i + 2])}  # noqa: E731
        row = {"jobs": J, "pairs": npairs, "refset_jobs": npairs, "connected": int(flags.sum()), "redundant": int(red.sum()),
               "build_call_and_sync": windows(synced(build)), "build_stream_ms_per_call": stream_ms(mt, build),
               "pairs_call_and_sync": windows(synced(pairs)), "pairs_stream_ms_per_call": stream_ms(mt, pairs),
               "refset_call_and_sync": windows(synced(refset)), "refset_stream_ms_per_call": stream_ms(mt, refset),
               "chain_one_wait": windows(synced(build, pairs, refset)),
               "host_index_one_thread": h(1), "host_update_covisibility_one_thread": h(5), "host_is_redundant_one_thread": h(9)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    meta = {"commit": a.stamp, "map": {"key_frame_slots": NFRAMES, "points": M, "observations": int(len(mp["obs_frame"])), "cap": CAP},
            "job": {"local_key_frames": NLOCAL, "references_per_local_key_frame": NREF, "k": 2},
            "not_measured": ["hardware counters", "occupancy", "kernel times under a profiler"]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"_meta": meta, "covis": rows}, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(meta, rows))


def markdown(meta, rows):
    g = lambda r, k: "%.4f (%.4f-%.4f)" % (r[k]["median_ms"], r[k]["p10_ms"], r[k]["p90_ms"])  # noqa: E731
    out = ["# Covisibility: shared map points and redundancy ratio for batches (tools/covis_bench.py)", "",
           "Commit: %s.  MI355X, one process, tables resident in device memory.  Map: %d key-frame slots, %d points, %d observations."
           % (meta["commit"], meta["map"]["key_frame_slots"], meta["map"]["points"], meta["map"]["observations"]),
           "A job = one new key frame: 50 pairs (Map::updateCovisibility) + 50 reference-set jobs of 10 slots (the redundancy test).",
           "Milliseconds, median (10th-90th percentile).  Host = include/se2lam_amd/Covisibility.h on one thread.", "",
           "| jobs | build, call + sync | build, on the stream | pairs, call + sync | pairs, on the stream | refset, call + sync | refset, on the stream | chain, one wait | host index() | host updateCovisibility | host isRedundant |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | " % r["jobs"] + " | ".join(g(r, k) for k in (
            "build_call_and_sync", "build_stream_ms_per_call", "pairs_call_and_sync", "pairs_stream_ms_per_call", "refset_call_and_sync",
            "refset_stream_ms_per_call", "chain_one_wait", "host_index_one_thread", "host_update_covisibility_one_thread",
            "host_is_redundant_one_thread")) + " |")
    out += ["", "Not measured: " + ", ".join(meta["not_measured"]) + ".", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
