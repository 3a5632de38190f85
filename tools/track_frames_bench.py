#!/usr/bin/env python3
"""removeOutliers + doTriangulate over batches of frame pairs: se2gpu_track_frames_batch_device on the match rows where the
batched MatchByWindow leaves them, against the route it replaces: wait, download the rows, then se2gpu_track_remove_outliers
and se2gpu_track_triangulate pair by pair (each with its own upload, launches, blocking download).

    python tools/track_frames_bench.py [--out profiles/track_frames_batch] [--commit ID] [--kernel-stats STATS.csv]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o TAG -- python tools/track_frames_bench.py --trace-run   (a run of its own)

Inputs: the scene generator of tests/track_frame_cases.py with 12 frames of 1000 features, cap = 1024: 6 pairs of views with
outlier shares 0.1 .. 0.6 and baselines of 60 .. 300 mm, a third of the features observed by the key frame.  A pair of the
batch is one of the 6 view pairs (drawn with repetition, seed 7) with a match row of 270 to 330 of its correspondences, number
and choice drawn per pair.  Both routes start from the rows in device memory and end with the counts on the host.  Host clock
around whole passes after warm-up: for the batch a pass is one call, the synchronise and the download of info (8 ints per
pair); for the loop it is the download of the rows and two calls per pair.  Windows last at least 0.5 s; medians over the timed
windows with the 10th and 90th percentile (the method of tools/loop_verify_bench.py).  Before anything is timed the batch's
rows, positions and flags are compared with the loop's, bit for bit.
--trace-run makes 20 batch calls of 256 pairs and nothing else, for the kernel trace; --kernel-stats reads the
<TAG>_kernel_stats.csv of such a run into the report."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import track_frame_cases as tc  # noqa: E402
from loop_verify_bench import commit, machine, stats  # noqa: E402
from se2lam_amd import capi  # noqa: E402
from se2lam_amd.track import Track  # noqa: E402

CAP, FEATURES, RAW = 1024, 1000, (270, 330)
OUTLIERS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
BASELINES = (60.0, 100.0, 150.0, 200.0, 250.0, 300.0)
NPAIRS = [1, 16, 256]
TRACE_CALLS, TRACE_PAIRS = 20, 256
KERNELS = ("k_lv_gather", "k_lv_draw", "k_lv_models", "k_lv_score", "k_lv_select", "k_track_frames")


def batch_of(sc, rng, P):
    b = tc.Batch()
    for k in rng.integers(0, len(OUTLIERS), P):
        b.add((2 * int(k), 2 * int(k) + 1), sc.row(int(k), int(rng.integers(RAW[0], RAW[1] + 1))), sc.pose(int(k)))
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_frames_batch"))
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
    sc = tc.Scene(CAP, (FEATURES,) * 6, OUTLIERS, BASELINES, seed=7)
    rng = np.random.default_rng(7)
    d_kps, d_cnt, d_obs, d_view = D.from_numpy(sc.kps), D.from_numpy(sc.counts), D.from_numpy(sc.kf_observed), D.from_numpy(sc.view_pos)
    tr = Track()
    result = {"commit": commit(a.commit), "machine": machine(), "frames": sc.nframes, "features": FEATURES, "cap": CAP, "raw_matches": "%d-%d" % RAW,
              "outlier_shares": list(OUTLIERS), "baselines_mm": list(BASELINES),
              "timing": "%d warm-up + %d timed windows of at least %.1f s" % (a.warmup, a.windows, a.window_seconds), "rows": []}
    for P in [int(p) for p in a.npairs.split(",")]:
        b = batch_of(sc, rng, P)
        pairs = np.array(b.pairs, np.int32)
        Trc, Pm = np.stack(b.Trc).astype(np.float32), np.stack(b.P).astype(np.float32)
        d_pa, d_pb = D.from_numpy(np.ascontiguousarray(pairs[:, 0])), D.from_numpy(np.ascontiguousarray(pairs[:, 1]))
        d_Trc, d_P, d_rows = D.from_numpy(Trc), D.from_numpy(Pm), D.from_numpy(np.stack(b.rows).astype(np.int32))
        d_m, d_pos, d_good, d_info = D(4 * P * CAP), D(12 * P * CAP), D(P * CAP), D(4 * P * 8)

        def batch_call():
            tr.track_frames_batch_device(d_kps.ptr, d_cnt.ptr, CAP, sc.nframes, d_obs.ptr, d_view.ptr, d_pa.ptr, d_pb.ptr, P, d_Trc.ptr,
                                         d_P.ptr, None, tc.P_REF, d_rows.ptr, tc.LOWER, tc.UPPER, tc.MIN_DEGREE, d_m.ptr, d_pos.ptr,
                                         d_good.ptr, d_info.ptr)

        def batch_pass():
            batch_call()
            tr.sync()
            return d_info.to_numpy(np.int32, (P, 8))

        def loop_pass():
            h_rows = d_rows.to_numpy(np.int32, (P, CAP))
            out = []
            for p, (x, y) in enumerate(pairs):
                nx, ny = sc.counts[x], sc.counts[y]
                m = h_rows[p, :nx].copy()
                ni = tr.removeOutliers(sc.kps[x, :nx], sc.kps[y, :ny], m)
                out.append((ni,) + tr.doTriangulate(sc.kps[x, :nx], sc.kps[y, :ny], m, sc.kf_observed[x, :nx], tc.P_REF, Pm[p],
                                                    Trc[p][[3, 7, 11]], tc.LOWER, tc.UPPER, tc.MIN_DEGREE))
            return out
        if a.trace_run:
            if P == TRACE_PAIRS:
                for _ in range(TRACE_CALLS):
                    batch_call()
                tr.sync()
            continue
        info = batch_pass()
        got_m, got_pos, got_good = d_m.to_numpy(np.int32, (P, CAP)), d_pos.to_numpy(np.float32, (P, CAP, 3)), d_good.to_numpy(np.uint8, (P, CAP))
        for p, (ni, pos, good, m, ng, nold) in enumerate(loop_pass()):      # the batch gives what the loop gives
            x = pairs[p, 0]
            n = len(m)
            assert RAW[0] <= info[p, 0] <= RAW[1] and info[p, 5] == 2 and [ni, nold, ng] == info[p, 1:4].tolist(), (P, p)
            old = (m >= 0) & (sc.kf_observed[x, :n] != 0)
            pos = pos.copy(); pos[old] = sc.view_pos[x, :n][old]           # the single call leaves these to the caller
            assert np.array_equal(got_m[p, :n], m) and np.array_equal(got_good[p, :n], good) and got_pos[p, :n].tobytes() == pos.tobytes(), (P, p)

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
        b_passes, bw = timed(batch_pass)
        l_passes, lo = timed(loop_pass)
        row = {"npairs": P, "inliers_mean": float(info[:, 1].mean()), "tracked_old_mean": float(info[:, 2].mean()),
               "good_prl_mean": float(info[:, 3].mean()), "depth_rejected_mean": float(info[:, 6].mean()),
               "batch_passes_per_window": b_passes, "loop_passes_per_window": l_passes, "batch_wall": bw, "loop_wall": lo,
               "loop_over_batch": lo["median_ms"] / bw["median_ms"]}
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
    tf = [r for r in rows if r["kernel"] in KERNELS]
    total = sum(r["total_ms"] for r in tf)
    for r in tf:
        r["share"] = r["total_ms"] / total if total else 0.0
    return tf


def markdown(r):
    def c(s):
        return "%.3f (%.3f-%.3f)" % (s["median_ms"], s["p10_ms"], s["p90_ms"])
    o = ["# Track: removeOutliers + doTriangulate, one batch call against two calls per pair", "",
         "Written by `tools/track_frames_bench.py`.  Commit %s, %s.  %d frames of %d features (cap %d): 6 pairs of views with outlier"
         " shares %s and baselines %s mm, a third of the features observed by the key frame; a pair of the batch is one of them (drawn"
         " with repetition) with %s raw matches.  %s.  Host clock around whole passes; times in ms per batch of pairs: median"
         " (10th-90th percentile)."
         % (r["commit"], r["machine"], r["frames"], r["features"], r["cap"], ", ".join("%.1f" % s for s in r["outlier_shares"]),
            ", ".join("%.0f" % s for s in r["baselines_mm"]), r["raw_matches"], r["timing"]), "",
         "- batch: `se2gpu_track_frames_batch_device` on the rows in device memory, the synchronise, and the download of `info`.",
         "- loop: the rows downloaded, then `se2gpu_track_remove_outliers` and `se2gpu_track_triangulate` pair by pair (the route the"
         " batch call replaces).", "",
         "| pairs | inliers | tracked old | good parallax | depth-rejected | batch (wall) | loop (wall) | loop / batch |",
         "|---|---|---|---|---|---|---|---|"]
    for w in r["rows"]:
        o.append("| %d | %.0f | %.0f | %.0f | %.0f | %s | %s | %.1f |" % (w["npairs"], w["inliers_mean"], w["tracked_old_mean"], w["good_prl_mean"],
                                                                         w["depth_rejected_mean"], c(w["batch_wall"]), c(w["loop_wall"]),
                                                                         w["loop_over_batch"]))
    if r.get("kernel_stats"):
        o += ["", "## Kernel times on the stream", "",
              "`rocprofv3 --kernel-trace --stats` over a run of its own (`--trace-run`: %d batch calls of %d pairs):" % (TRACE_CALLS, TRACE_PAIRS),
              "", "| kernel | calls | average, us | total, ms | share |", "|---|---|---|---|---|"]
        for k in r["kernel_stats"]:
            o.append("| %s | %d | %.2f | %.3f | %.1f %% |" % (k["kernel"], k["calls"], k["avg_us"], k["total_ms"], 100 * k["share"]))
    else:
        o += ["", "Kernel times on the stream were not measured in this run (no `--kernel-stats`)."]
    behind = [w for w in r["rows"] if w["loop_over_batch"] < 1]
    ahead = [w for w in r["rows"] if w["loop_over_batch"] >= 1]
    if ahead:
        o += ["", "The batch call is the faster route at %s." % ", ".join("%d pairs (%.1f x)" % (w["npairs"], w["loop_over_batch"]) for w in ahead)]
    if behind:
        o += ["", "At %s the host route is the faster one, as in the loop verification: the six kernels follow each other whatever the"
              " batch holds, and the sample draw - one wave per pair - is most of that chain." % ", ".join("%d pair%s" % (w["npairs"], "" if w["npairs"] == 1 else "s") for w in behind)]
    o += ["", "Not measured: the chain behind the extractor and the matcher (their own legs are in `bench.py`), and caps other than"
          " %d (at this cap a slice of scratch holds 228 pairs, so the 256-pair row runs as two slices)." % r["cap"], ""]
    return "\n".join(o)


if __name__ == "__main__":
    main()
