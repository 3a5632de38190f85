#!/usr/bin/env python3
"""Map::updateLocalGraph for batches of current key frames: se2gpu_local_window_batch_device on the adjacency and observation
bit matrices resident in device memory against se2gpu_map_update_local_graph (host code of libse2gpu, csrc/map_view.hip) called
once per job on ONE host thread over a CSR view of the same map.

    python tools/local_window_bench.py [--out profiles/local_window.json] [--md profiles/local_window.md] [--stamp COMMIT]

The map is that of tools/covis_bench.py (seed 7): 256 key-frame slots, 20,000 points with 3-8 observations each among the 13
slots around a centre slot, 10 % null.  The covisibility graph is what the chain itself builds: every slot against its 12
nearest slots through se2gpu_covis_pairs_device, connected where Map.cpp:794 says so.  A job is one current key frame with
search_level 3; 1, 16 and 256 jobs (distinct slots), lists at full capacity in index order.
Device: after two warm-up calls, windows of at least 0.3 s of call + se2gpu_matcher_sync (host clock) and device events around
50 calls queued back to back; medians over 7 windows with the 10th / 90th percentile.  The chain is build -> pairs -> connect
-> window queued on one stream with one wait; build and pairs cover the whole map every time and do not depend on the number of
jobs.  Host: the CSR view (covisibility, getAllObsMPs(false) and getObservations() as index lists) is prepared outside the
timing and its preparation is reported on its own; then one call per job from a Python loop over ctypes, median over 7 windows.
The device's three lists and counts are compared with the host's for every job before anything is timed.  No figure is gated.
Not measured: counters, occupancy, kernel times under a profiler."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from covis_bench import CAP, M, NFRAMES, nearest, stream_ms, the_map, windows  # noqa: E402
from se2lam_amd import capi, covis, localwindow as lw  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

NNEAR, LEVEL = 12, 3


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, np.int32) for l in lists] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, np.ascontiguousarray(idx)


def host_view(mp, adj_lists):
    """se2gpu_map_view of the map; returns (view, the arrays it points into, seconds spent preparing it)"""
    t0 = time.perf_counter()
    kf_pts = [[] for _ in range(NFRAMES)]
    mp_kfs = []
    for p in range(M):
        fr = sorted(set(int(f) for f in mp["obs_frame"][mp["ptr"][p]:mp["ptr"][p + 1]]))
        mp_kfs.append(fr)
        if not mp["null"][p]:
            for f in fr:
                kf_pts[f].append(p)
    keep = [np.arange(NFRAMES, dtype=np.int32), *csr(adj_lists), *csr(kf_pts), np.arange(M, dtype=np.int32), *csr(mp_kfs)]
    v = capi.MapView()
    v.n_kf, v.n_mp = NFRAMES, M
    (v.kf_id, v.covis_ptr, v.covis_idx, v.kf_mp_ptr, v.kf_mp_idx, v.mp_id, v.mp_kf_ptr, v.mp_kf_idx) = [a.ctypes.data for a in keep]
    return v, keep, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--stamp", default="unknown")
    ap.add_argument("--sizes", default="1,16,256")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    mt = ORBmatcher()
    lib, up = capi.lib(), capi.upload
    mp = the_map(np.random.default_rng(7))
    cv = covis.DeviceCovis(mp["counts"], CAP, mp["ptr"], mp["obs_frame"], mp["obs_ftr"], mp["null"], mp["good"])
    pa = np.repeat(np.arange(NFRAMES, dtype=np.int32), NNEAR)
    pb = np.concatenate([nearest(f, NNEAR) for f in range(NFRAMES)]).astype(np.int32)
    npairs = len(pa)
    d_a, d_b = up(pa, np.int32), up(pb, np.int32)
    d_pout, d_prat = up(np.zeros((npairs, 4)), np.int32), up(np.zeros((npairs, 2)), np.float32)
    adj = lw.DeviceAdjacency(NFRAMES)
    W, WF = cv.W, adj.WF

    def build():
        cv.build(mt, sync=False)

    def pairs():
        capi.check(lib.se2gpu_covis_pairs_device(mt._h, cv.bits.ptr, NFRAMES, M, d_a.ptr, d_b.ptr, npairs, 0.3, 0.1, d_pout.ptr,
                                                 d_prat.ptr, None, 0, None, 0, None, None, None, 0))

    def connect():
        capi.check(lib.se2gpu_covis_connect_device(mt._h, adj.adj.ptr, NFRAMES, d_a.ptr, d_b.ptr, npairs, d_pout.ptr, 1))

    def synced(*fns):
        def f():
            for g in fns:
                g()
            mt.sync()
        return f
    synced(build, pairs, connect)()
    adj_lists = adj.read_lists()
    view, keep, prep_s = host_view(mp, adj_lists)
    lk, rk, lm = np.zeros(NFRAMES, np.int32), np.zeros(NFRAMES, np.int32), np.zeros(M, np.int32)
    nl, nr, nm = C.c_int(), C.c_int(), C.c_int()

    def host_one(cur):
        capi.check(lib.se2gpu_map_update_local_graph(C.byref(view), int(cur), LEVEL, lk.ctypes.data, C.byref(nl), rk.ctypes.data,
                                                     C.byref(nr), lm.ctypes.data, C.byref(nm)))

    rows = []
    for J in [int(x) for x in a.sizes.split(",")]:
        jobs = np.random.default_rng(11).permutation(NFRAMES)[:J].astype(np.int32)
        d_jobs = up(jobs, np.int32)
        d_wkf, d_wmp = up(np.zeros(J * 2 * WF, np.uint64), np.uint64), up(np.zeros(J * W, np.uint64), np.uint64)
        d_out = up(np.zeros((J, 4)), np.int32)
        d_ll, d_rl, d_ml = up(np.zeros(J * NFRAMES), np.int32), up(np.zeros(J * NFRAMES), np.int32), up(np.zeros(J * M), np.int32)

        def window():
            capi.check(lib.se2gpu_local_window_batch_device(mt._h, cv.bits.ptr, cv.bits.ptr, NFRAMES, M, adj.adj.ptr, None, d_jobs.ptr,
                                                            J, LEVEL, None, None, d_wkf.ptr, d_wmp.ptr, d_out.ptr, d_ll.ptr, d_rl.ptr,
                                                            NFRAMES, d_ml.ptr, M))

        def window_no_lists():
            capi.check(lib.se2gpu_local_window_batch_device(mt._h, cv.bits.ptr, cv.bits.ptr, NFRAMES, M, adj.adj.ptr, None, d_jobs.ptr,
                                                            J, LEVEL, None, None, d_wkf.ptr, d_wmp.ptr, d_out.ptr, None, None, 0, None, 0))

        def host_all():
            for cur in jobs:
                host_one(cur)
        synced(window)()
        out = d_out.to_numpy(np.int32, (J, 4))
        ll, rl = d_ll.to_numpy(np.int32, (J, NFRAMES)), d_rl.to_numpy(np.int32, (J, NFRAMES))
        ml = d_ml.to_numpy(np.int32, (J, M))
        for j, cur in enumerate(jobs):
            host_one(cur)
            assert out[j, :3].tolist() == [nl.value, nr.value, nm.value], "device and host select windows of other sizes"
            assert np.array_equal(ll[j, :nl.value], lk[:nl.value]) and np.array_equal(rl[j, :nr.value], rk[:nr.value]) and \
                np.array_equal(ml[j, :nm.value], lm[:nm.value]), "device and host select other windows"
        row = {"jobs": J, "local_kfs_mean": float(out[:, 0].mean()), "ref_kfs_mean": float(out[:, 1].mean()),
               "points_mean": float(out[:, 2].mean()), "edges_mean": float(out[:, 3].mean()),
               "window_call_and_sync": windows(synced(window)), "window_stream_ms_per_call": stream_ms(mt, window),
               "window_no_lists_call_and_sync": windows(synced(window_no_lists)),
               "window_no_lists_stream_ms_per_call": stream_ms(mt, window_no_lists),
               "chain_one_wait": windows(synced(build, pairs, connect, window)),
               "chain_stream_ms_per_call": stream_ms(mt, lambda: (build(), pairs(), connect(), window())),
               "host_one_thread": windows(host_all)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    meta = {"commit": a.stamp, "map": {"key_frame_slots": NFRAMES, "points": M, "observations": int(len(mp["obs_frame"])),
                                      "covisibility_edges": int(sum(len(l) for l in adj_lists))},
            "search_level": LEVEL, "pairs_in_the_chain": npairs, "host_view_preparation_s": prep_s,
            "not_measured": ["hardware counters", "occupancy", "kernel times under a profiler"]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"_meta": meta, "local_window": rows}, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(meta, rows))


def markdown(meta, rows):
    g = lambda r, k: "%.4f (%.4f-%.4f)" % (r[k]["median_ms"], r[k]["p10_ms"], r[k]["p90_ms"])  # noqa: E731
    cols = ("window_call_and_sync", "window_stream_ms_per_call", "window_no_lists_call_and_sync", "window_no_lists_stream_ms_per_call",
            "chain_one_wait", "chain_stream_ms_per_call", "host_one_thread")
    out = ["# Local window: Map::updateLocalGraph for batches of current key frames (tools/local_window_bench.py)", "",
           "Commit: %s.  MI355X, one process, tables resident in device memory.  Map: %d key-frame slots, %d points, %d observations, "
           "%d directed covisibility edges." % (meta["commit"], meta["map"]["key_frame_slots"], meta["map"]["points"],
                                                meta["map"]["observations"], meta["map"]["covisibility_edges"]),
           "A job = one current key frame, search_level %d; the lists at full capacity in index order.  The chain is build -> pairs "
           "(%d) -> connect -> window with one wait; build and pairs cover the whole map whatever the number of jobs."
           % (meta["search_level"], meta["pairs_in_the_chain"]),
           "Milliseconds per call of the whole batch, median (10th-90th percentile).  Host = se2gpu_map_update_local_graph once per "
           "job on one thread; its CSR view was prepared outside the timing in %.2f s (Python)." % meta["host_view_preparation_s"], "",
           "| jobs | local / ref key frames, points, edges (mean) | window, call + sync | window, on the stream | without lists, call + sync "
           "| without lists, on the stream | chain, one wait | chain, on the stream | host, one thread |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %d | %.1f / %.1f, %.0f, %.0f | " % (r["jobs"], r["local_kfs_mean"], r["ref_kfs_mean"], r["points_mean"],
                                                          r["edges_mean"]) + " | ".join(g(r, k) for k in cols) + " |")
    out += ["", "Not measured: " + ", ".join(meta["not_measured"]) + ".", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
