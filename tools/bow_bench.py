#!/usr/bin/env python3
"""Device vocabulary against the host vocabulary (include/se2lam_amd/ORBVocabulary.h, g++ -O2, 1 and 16 threads) on the same
inputs: a synthetic full k = 10, L = 6 vocabulary (the shape of ORBvoc: 1.1 M nodes, 1 M words), generated with a fixed seed.

    python tools/bow_bench.py [--quick] [--out profiles/bow_device] [--commit ID]

  (a) se2gpu_bow_transform_batch_device over batches of frames of 1,000 descriptors (and the single-frame host-buffer call);
  (b) se2gpu_bowdb_query of one BowVector against data bases of key frames of about 1,000 words.
Device times are HIP events on the context's stream (se2gpu_timer_*) around a window of back-to-back calls, divided by the
number of calls, after warm-up windows; medians over the windows with the 10th and 90th percentile.  Consecutive transform
calls of a window take different frames (a pool of 512), so that no call walks the paths of the call before it.  (b) also
reports the wall time of the synchronous call, which is what a caller waits for.  Writes <out>.md and <out>.json; every device
result is compared with the host's before it is timed (bit for bit)."""
import argparse
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from se2lam_amd import capi, vocabulary as V  # noqa: E402

FEATURES = 1000


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "p10_ms": ms[int(0.1 * (len(ms) - 1))], "p90_ms": ms[int(round(0.9 * (len(ms) - 1)))], "n": len(ms)}


def host_times(out):
    line = [l for l in out.splitlines() if l.startswith("SECONDS")][0]
    return stats([1e3 * float(x) for x in line.split()[1:]])


def machine():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:  # noqa: BLE001
        return "gfx950"


def commit(arg):
    if arg:
        return arg
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="k = 10, L = 4 and small sizes: a functional check of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_device"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--windows", type=int, default=12, help="timed windows per size")
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per window")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per size")
    a = ap.parse_args()
    k, L = (10, 4) if a.quick else (10, 6)
    batches = [1, 4, 16] if a.quick else [1, 2, 4, 8, 16, 64, 256]
    host16_at = {1, 16, 256}
    db_sizes = [100, 500] if a.quick else [500, 5000, 50000]
    host_reps = 3 if a.quick else 5
    tmp = tempfile.mkdtemp(prefix="bow_bench_")
    exe = os.path.join(tmp, "cpp_bow_mirror")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_bow_mirror.cpp"),
                           "-o", exe, "-pthread"])
    t0 = time.time()
    parent, desc, weight, leaf = V.synthetic_vocabulary(2026, k, L, V.TF_IDF, full=True)
    voc_path = os.path.join(tmp, "voc.bin")
    V.write_vocabulary_file(voc_path, k, L, V.L1_NORM, V.TF_IDF, parent, desc, weight, leaf)
    voc = V.Vocabulary(k, L, V.L1_NORM, V.TF_IDF, parent, desc, weight, leaf)
    print("vocabulary: %d nodes, %d words, %.1f s" % (voc.nodes, voc.words, time.time() - t0), flush=True)
    rng = np.random.default_rng(7)
    leaves = np.nonzero(leaf)[0]
    nmax = 2 * max(batches)
    frames = np.concatenate([desc[rng.choice(leaves, (1, FEATURES))] ^ np.packbits(rng.random((1, FEATURES, 256)) < 0.04, axis=2)
                             for _ in range(nmax)])
    counts = np.full(nmax, FEATURES, np.int32)
    ctx = V.BowContext(voc, max_features=FEATURES, max_batch=max(batches))
    timer = capi.Timer()
    D = capi.DeviceArray
    d_pool, d_pool_cnt = D.from_numpy(frames), D.from_numpy(counts)

    def windows(call):
        """-> (per-call ms by events, per-call ms by the host clock) over the timed windows; call(i) is the i-th call of a window"""
        ev, wall = [], []
        for w in range(a.warmup + a.windows):
            t1 = time.perf_counter()
            timer.start(ctx.stream())
            for i in range(a.calls):
                call(i)
            timer.stop(ctx.stream())
            e = timer.elapsed_ms()                                        # synchronises on the stop event
            t2 = time.perf_counter()
            if w >= a.warmup:
                ev.append(e / a.calls); wall.append(1e3 * (t2 - t1) / a.calls)
        return stats(ev), stats(wall)
    result = {"commit": commit(a.commit), "machine": machine(), "vocabulary": {"k": k, "L": L, "nodes": voc.nodes, "words": voc.words},
              "features_per_frame": FEATURES, "timing": "HIP events around windows of %d back-to-back calls, %d warm-up + %d timed windows; host: %d runs" % (a.calls, a.warmup, a.windows, host_reps),
              "transform": [], "query": []}

    # ---- (a) transform
    for B in batches:
        fr, cn = np.ascontiguousarray(frames[:B]), counts[:B]
        bw, bv, bn = D(4 * B * FEATURES), D(8 * B * FEATURES), D(4 * B)
        fn, fp, fi, nn = D(4 * B * FEATURES), D(4 * B * (FEATURES + 1)), D(4 * B * FEATURES), D(4 * B)
        starts = list(range(0, nmax - B + 1, B))

        def call(i):
            f0 = starts[i % len(starts)]
            ctx.transform_batch_device(d_pool.ptr.value + 32 * FEATURES * f0, d_pool_cnt.ptr.value + 4 * f0, FEATURES, B, 4, bw.ptr, bv.ptr,
                                       bn.ptr, fn.ptr, fp.ptr, fi.ptr, nn.ptr)
        dev, _ = windows(call)
        call(0); ctx.sync()                                               # the outputs compared below are those of frames[:B]
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(struct.pack("<ii", B, FEATURES) + cn.tobytes() + fr.tobytes())
        row = {"frames": B, "device": dev}
        for threads in (1, 16):
            if threads == 16 and B not in host16_at:
                continue
            r = subprocess.run([exe, "transform", voc_path, os.path.join(tmp, "in.bin"), "4", os.path.join(tmp, "out.bin"), str(threads), str(host_reps)],
                               capture_output=True, text=True, check=True)
            row["host%d" % threads] = host_times(r.stdout)
        # the device's answer is the host's (first frame of the batch, bit for bit)
        out = open(os.path.join(tmp, "out.bin"), "rb").read()
        nb0 = struct.unpack_from("<i", out)[0]
        h_bn = bn.to_numpy(np.int32, B)
        assert h_bn[0] == nb0 and np.array_equal(bw.to_numpy(np.uint32, (B, FEATURES))[0, :nb0], np.frombuffer(out, "<u4", nb0, 4))
        assert np.array_equal(bv.to_numpy(np.float64, (B, FEATURES))[0, :nb0], np.frombuffer(out, "<f8", nb0, 4 + 4 * nb0))
        row["ratio_host1_over_device"] = row["host1"]["median_ms"] / dev["median_ms"]
        if B == 1:                                                     # the host-buffer call a mapper makes for one key frame
            row["single_frame_call_wall"] = windows(lambda i: ctx.transform(frames[i % nmax], 4))[1]
        result["transform"].append(row)
        print("transform", json.dumps(row), flush=True)

    # ---- (b) query
    nq_words = 1000
    hot = rng.choice(voc.words, min(20000, voc.words // 2), replace=False)

    def bow_vector():
        w = np.unique(np.concatenate([rng.choice(hot, nq_words // 2), rng.integers(0, voc.words, nq_words // 2)])).astype(np.uint32)
        v = rng.random(len(w)) + 0.05
        return w, v / v.sum()
    query = bow_vector()
    nmax_db = max(db_sizes)
    entries = [bow_vector() for _ in range(nmax_db)]
    db = V.BowDatabase(voc)
    filled = 0
    for n in db_sizes:
        for i in range(filled, n):
            db.add(i, *entries[i])
        filled = n
        with open(os.path.join(tmp, "vecs.bin"), "wb") as f:
            f.write(struct.pack("<ii", 1, n))
            for w, v in [query] + entries[:n]:
                f.write(struct.pack("<i", len(w))); f.write(w.tobytes()); f.write(v.tobytes())
        row = {"key_frames": n, "words_per_key_frame": float(np.mean([len(w) for w, _ in entries[:n]]))}
        for threads in (1, 16):
            r = subprocess.run([exe, "score", voc_path, os.path.join(tmp, "vecs.bin"), os.path.join(tmp, "scores.bin"), str(threads), str(host_reps)],
                               capture_output=True, text=True, check=True)
            row["host%d" % threads] = host_times(r.stdout)
        want = np.fromfile(os.path.join(tmp, "scores.bin"), "<f8")
        got, entry, kf, best = db.query(ctx, *query)
        assert np.array_equal(got, want) and entry == int(np.argmax(want)), "device scores differ from the host vocabulary's"
        for label, scores in (("device_with_scores", True), ("device_best_only", False)):
            row[label], row[label + "_wall"] = windows(lambda i: db.query(ctx, *query, want_scores=scores))
        row["ratio_host1_over_device"] = row["host1"]["median_ms"] / row["device_best_only"]["median_ms"]
        result["query"].append(row)
        print("query", json.dumps(row), flush=True)

    def first_faster(rows, key, dev_key):
        for r in rows:
            if dev_key(r) < r["host1"]["median_ms"]:
                return r[key]
        return None
    result["device_overtakes_one_host_thread_at"] = {
        "transform_frames": first_faster(result["transform"], "frames", lambda r: r["device"]["median_ms"]),
        "query_key_frames": first_faster(result["query"], "key_frames", lambda r: r["device_best_only_wall"]["median_ms"])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(result, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write(markdown(result))
    print("wrote", a.out + ".md", a.out + ".json")
    shutil.rmtree(tmp, ignore_errors=True)


def markdown(r):
    def c(s):
        return "%.3f (%.3f-%.3f)" % (s["median_ms"], s["p10_ms"], s["p90_ms"]) if s else "-"
    o = ["# Device vocabulary against the host vocabulary", "",
         "Written by `tools/bow_bench.py`.  Commit %s, %s.  Vocabulary: synthetic, full, k = %d, L = %d, %d nodes, %d words; %d descriptors"
         " per frame; levelsup 4.  %s.  Times in ms: median (10th-90th percentile).  Host: `include/se2lam_amd/ORBVocabulary.h`, g++ -O2,"
         " frames / key frames split over the threads." % (r["commit"], r["machine"], r["vocabulary"]["k"], r["vocabulary"]["L"],
                                                            r["vocabulary"]["nodes"], r["vocabulary"]["words"], r["features_per_frame"], r["timing"]), "",
         "## (a) transform_batch_device", "", "| frames | device | host, 1 thread | host, 16 threads | host 1 / device |", "|---|---|---|---|---|"]
    for t in r["transform"]:
        o.append("| %d | %s | %s | %s | %.2f |" % (t["frames"], c(t["device"]), c(t["host1"]), c(t.get("host16")), t["ratio_host1_over_device"]))
    one = [t for t in r["transform"] if "single_frame_call_wall" in t]
    if one:
        o += ["", "The single-frame call with host buffers (`se2gpu_bow_transform`: upload, two kernels, download), wall time of the call: %s;"
              " the host vocabulary on one thread: %s." % (c(one[0]["single_frame_call_wall"]), c(one[0]["host1"]))]
    o += ["", "## (b) bowdb_query, one query", "",
          "| key frames | device, best only (events) | the call, best only (wall) | device, all scores (events) | the call, all scores (wall) | host, 1 thread | host, 16 threads | host 1 / device |",
          "|---|---|---|---|---|---|---|---|"]
    for q in r["query"]:
        o.append("| %d | %s | %s | %s | %s | %s | %s | %.2f |" % (q["key_frames"], c(q["device_best_only"]), c(q["device_best_only_wall"]), c(q["device_with_scores"]),
                                                                    c(q["device_with_scores_wall"]), c(q["host1"]), c(q["host16"]), q["ratio_host1_over_device"]))
    x = r["device_overtakes_one_host_thread_at"]
    o += ["", "The device overtakes one host thread at: transform - %s frames per batch; query (wall time of the call) - %s key frames"
          " (smallest measured size at which it is faster; `None` = at none of them)." % (x["transform_frames"], x["query_key_frames"]), ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
