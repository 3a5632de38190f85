#!/usr/bin/env python3
"""Loop verification over batches of key-frame pairs: se2gpu_track_loop_verify_batch_device on the match rows where the batched
matcher leaves them, against the only route there was before it: the rows downloaded, then se2gpu_track_remove_outliers pair by
pair (per pair: the samples drawn on the host, one upload, three launches, one blocking download).

    python tools/loop_verify_bench.py [--out profiles/loop_verify_batch] [--commit ID] [--kernel-stats STATS.csv]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o TAG -- python tools/loop_verify_bench.py --trace-run   (a run of its own)

Inputs: 12 frames of 1000 features, cap = 1024; frames 2k and 2k+1 are the two views of synth.two_view_matches(seed k) with
outlier shares 0.1 .. 0.6, each in a random feature order.  A pair is one of the 6 view pairs (drawn with repetition, seed 7)
with a match row of 270 to 330 of its correspondences, number and choice drawn per pair (the samples depend on the number, so
a loop over pairs of one size would draw them once and reuse them).  Both routes start from the rows in device memory and end with
the survivors' counts on the host.  Host clock around whole passes after warm-up: for the batch a pass is one call, the
synchronise and the download of info (8 ints per pair); for the loop it is the download of the rows and one call per pair.
Windows last at least 0.5 s; medians over the timed windows with the 10th and 90th percentile.  Before anything is timed the
batch's rows are compared with the loop's, bit for bit.  From info the report also takes the share of the 1000 samples per
pair that lie beyond the reference's adaptive stop: they are computed, scored and never looked at.
--trace-run makes 20 batch calls of 256 pairs and nothing else, for the kernel trace; --kernel-stats reads the
<TAG>_kernel_stats.csv of such a run into the report."""
import argparse
import csv
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from se2lam_amd import capi, synth  # noqa: E402
from se2lam_amd.track import Track  # noqa: E402

NFRAMES, CAP, FEATURES, RAW = 12, 1024, 1000, (270, 330)
OUTLIERS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
NPAIRS = [1, 16, 256]
TRACE_CALLS, TRACE_PAIRS = 20, 256
KERNELS = ("k_lv_gather", "k_lv_draw", "k_lv_models", "k_lv_score", "k_lv_select")


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "p10_ms": ms[int(0.1 * (len(ms) - 1))], "p90_ms": ms[int(round(0.9 * (len(ms) - 1)))], "n": len(ms)}


def commit(arg):
    if arg:
        return arg
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def machine():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:  # noqa: BLE001
        return "gfx950"


class Scene:
    def __init__(self):
        rng = np.random.default_rng(7)
        self.kps = np.zeros((NFRAMES, CAP), capi.KP_DTYPE)
        self.counts = np.full(NFRAMES, FEATURES, np.int32)
        self.where = []
        for k, frac in enumerate(OUTLIERS):
            p1, p2, _ = synth.two_view_matches(200 + k, FEATURES, frac)
            wa, wb = rng.permutation(FEATURES), rng.permutation(FEATURES)
            for f, w, p in ((2 * k, wa, p1), (2 * k + 1, wb, p2)):
                self.kps["x"][f, w], self.kps["y"][f, w] = p[:, 0], p[:, 1]
            self.where.append((wa, wb))
        self.has_mp = (rng.random((NFRAMES, CAP)) < 0.7).astype(np.uint8)
        self.rng = rng
        D = capi.DeviceArray
        self.d_kps, self.d_cnt, self.d_has = D.from_numpy(self.kps), D.from_numpy(self.counts), D.from_numpy(self.has_mp)

    def batch(self, P):
        """P pairs -> (pairs (P, 2), rows (P, CAP))"""
        ks = self.rng.integers(0, len(OUTLIERS), P)
        rows = np.full((P, CAP), -1, np.int32)
        for p, k in enumerate(ks):
            wa, wb = self.where[k]
            js = self.rng.choice(FEATURES, int(self.rng.integers(RAW[0], RAW[1] + 1)), replace=False)
            rows[p, wa[js]] = wb[js]
        return np.stack([2 * ks, 2 * ks + 1], 1).astype(np.int32), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_verify_batch"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per row")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per row")
    ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--npairs", default=",".join(str(p) for p in NPAIRS), help="batch sizes, comma separated")
    ap.add_argument("--trace-run", action="store_true", help="%d batch calls of %d pairs and nothing else (for rocprofv3)" % (TRACE_CALLS, TRACE_PAIRS))
    ap.add_argument("--kernel-stats", default="", help="<TAG>_kernel_stats.csv of a --trace-run under rocprofv3")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    D = capi.DeviceArray
    scene = Scene()
    tr = Track()
    result = {"commit": commit(a.commit), "machine": machine(), "frames": NFRAMES, "features": FEATURES, "cap": CAP, "raw_matches": "%d-%d" % RAW,
              "outlier_shares": list(OUTLIERS), "timing": "%d warm-up + %d timed windows of at least %.1f s" % (a.warmup, a.windows, a.window_seconds),
              "rows": []}
    for P in [int(p) for p in a.npairs.split(",")]:
        pairs, rows = scene.batch(P)
        d_pa, d_pb = D.from_numpy(np.ascontiguousarray(pairs[:, 0])), D.from_numpy(np.ascontiguousarray(pairs[:, 1]))
        d_rows, d_good, d_mp, d_info = D.from_numpy(rows), D(4 * P * CAP), D(4 * P * CAP), D(4 * P * 8)

        def batch_call():
            tr.loop_verify_batch_device(scene.d_kps.ptr, scene.d_cnt.ptr, CAP, NFRAMES, scene.d_has.ptr, None, d_pa.ptr, d_pb.ptr, P,
                                        d_rows.ptr, d_good.ptr, d_mp.ptr, d_info.ptr)

        def batch_pass():
            batch_call()
            tr.sync()
            return d_info.to_numpy(np.int32, (P, 8))

        def loop_pass():
            h_rows = d_rows.to_numpy(np.int32, (P, CAP))
            out = []
            for p, (x, y) in enumerate(pairs):
                m = h_rows[p, :scene.counts[x]].copy()
                ni = tr.removeOutliers(scene.kps[x, :scene.counts[x]], scene.kps[y, :scene.counts[y]], m)
                out.append((ni, m))
            return out
        if a.trace_run:
            if P == TRACE_PAIRS:
                for _ in range(TRACE_CALLS):
                    batch_call()
                tr.sync()
            continue
        info = batch_pass()
        good = d_good.to_numpy(np.int32, (P, CAP))
        for p, (ni, m) in enumerate(loop_pass()):                          # the batch keeps what the loop keeps
            assert RAW[0] <= info[p, 0] <= RAW[1] and info[p, 4] == 2
            if info[p, 1] >= 10:
                assert ni == info[p, 1] and np.array_equal(good[p, :len(m)], m) and (good[p, len(m):] == -1).all(), (P, p)
            else:
                assert ni == 0

        def window(fn, passes):
            t0 = time.perf_counter()
            for _ in range(passes):
                fn()
            return 1e3 * (time.perf_counter() - t0) / passes

        def timed(fn):
            passes = 1
            while True:                                                     # passes per window: at least window_seconds
                ms = window(fn, passes) * passes
                if ms >= 1e3 * a.window_seconds:
                    break
                passes = int(passes * max(1.2, 1.2e3 * a.window_seconds / max(ms, 1e-3))) + 1
            return passes, stats([window(fn, passes) for w in range(a.warmup + a.windows)][a.warmup:])
        b_passes, b = timed(batch_pass)
        l_passes, lo = timed(loop_pass)
        iters = info[:, 7].astype(np.float64)
        row = {"npairs": P, "inliers_mean": float(info[:, 1].mean()), "inliers_mp_mean": float(info[:, 2].mean()),
               "batch_passes_per_window": b_passes, "loop_passes_per_window": l_passes, "batch_wall": b, "loop_wall": lo,
               "loop_over_batch": lo["median_ms"] / b["median_ms"], "iterations_mean": float(iters.mean()),
               "samples_beyond_stop": float(1.0 - iters.mean() / 1000.0)}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.trace_run:
        print("trace run: %d batch calls of %d pairs" % (TRACE_CALLS, TRACE_PAIRS))
        return
    if a.kernel_stats:
        result["kernel_stats"] = kernel_stats(a.kernel_stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(result, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write(markdown(result))
    print("wrote", a.out + ".md", a.out + ".json")


def kernel_stats(path):
    rows = []
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\(anonymous namespace\)::", "", r["Name"]).split("(")[0].split("::")[-1]
        rows.append({"kernel": name, "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "total_ms": float(r["TotalDurationNs"]) / 1e6})
    lv = [r for r in rows if r["kernel"] in KERNELS]
    total = sum(r["total_ms"] for r in lv)
    for r in lv:
        r["share"] = r["total_ms"] / total if total else 0.0
    return lv


def markdown(r):
    def c(s):
        return "%.3f (%.3f-%.3f)" % (s["median_ms"], s["p10_ms"], s["p90_ms"])
    o = ["# Loop verification: one batch call against one call per pair", "",
         "Written by `tools/loop_verify_bench.py`.  Commit %s, %s.  %d frames of %d features (cap %d): 6 pairs of views from"
         " `synth.two_view_matches` with outlier shares %s; a pair of the batch is one of them (drawn with repetition) with %s raw matches."
         "  %s.  Host clock around whole passes; times in ms per batch of pairs: median (10th-90th percentile)."
         % (r["commit"], r["machine"], r["frames"], r["features"], r["cap"], ", ".join("%.1f" % s for s in r["outlier_shares"]), r["raw_matches"],
            r["timing"]), "",
         "- batch: `se2gpu_track_loop_verify_batch_device` on the rows in device memory (both output rows, map-point flags given), the"
         " synchronise, and the download of `info`.",
         "- loop: the rows downloaded, then `se2gpu_track_remove_outliers` pair by pair (the only route before this entry point existed).", "",
         "| pairs | inliers per pair | batch (wall) | loop (wall) | loop / batch | iterations of the reference's loop, mean | samples beyond the adaptive stop |",
         "|---|---|---|---|---|---|---|"]
    for w in r["rows"]:
        o.append("| %d | %.0f | %s | %s | %.1f | %.0f | %.1f %% |" % (w["npairs"], w["inliers_mean"], c(w["batch_wall"]), c(w["loop_wall"]),
                                                                   w["loop_over_batch"], w["iterations_mean"], 100 * w["samples_beyond_stop"]))
    o += ["", "Samples beyond the adaptive stop: both routes run all 1000 samples of a RANSAC pair and replay the reference's stop rule over"
          " the scores afterwards; the share is 1 - iterations / 1000 from `info`, the work a stop-aware schedule could leave out."]
    if r.get("kernel_stats"):
        o += ["", "## Kernel split", "",
              "`rocprofv3 --kernel-trace --stats` over a run of its own (`--trace-run`: %d batch calls of %d pairs):" % (TRACE_CALLS, TRACE_PAIRS),
              "", "| kernel | calls | average, us | total, ms | share |", "|---|---|---|---|---|"]
        for k in r["kernel_stats"]:
            o.append("| %s | %d | %.2f | %.3f | %.1f %% |" % (k["kernel"], k["calls"], k["avg_us"], k["total_ms"], 100 * k["share"]))
    many = [w for w in r["rows"] if w["npairs"] >= 16]
    if many:
        if all(w["loop_over_batch"] > 1 for w in many):
            o += ["", "From 16 pairs on the batch call is %.0f to %.0f times faster than the loop (1 pair: %s)." % (
                min(w["loop_over_batch"] for w in many), max(w["loop_over_batch"] for w in many),
                ", ".join("%.1f" % w["loop_over_batch"] for w in r["rows"] if w["npairs"] == 1))]
        else:
            o += ["", "The batch call does NOT beat the loop on every row from 16 pairs on (loop / batch: %s); the kernel split shows where its time goes."
                  % ", ".join("%d pairs %.2f" % (w["npairs"], w["loop_over_batch"]) for w in many)]
    behind = [w for w in r["rows"] if w["loop_over_batch"] < 1]
    if behind:
        o += ["", "At %s the loop is the faster route: the five kernels of a slice follow each other whatever the batch holds, and"
              " `k_lv_draw` - one wave per pair, its length does not depend on the number of pairs - is most of that chain, while the"
              " single-pair route draws its samples on the host in less time than that." % ", ".join("%d pair%s" % (w["npairs"], "" if w["npairs"] == 1 else "s") for w in behind)]
    o.append("")
    return "\n".join(o)


if __name__ == "__main__":
    main()
