#!/usr/bin/env python3
"""SearchByBoW over batches of key-frame pairs: se2gpu_search_by_bow_batch_device on the arrays where the extractor and the
transform left them, against the same pairs through se2gpu_search_by_bow one by one (host buffers, starting from the downloaded
arrays: uploads, a host merge of the node lists, two kernels, a download and a synchronise per pair).

    python tools/search_bow_bench.py [--out profiles/search_bow_batch] [--commit ID] [--kernel-stats STATS.csv]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o TAG -- python tools/search_bow_bench.py --trace-run   (a run of its own)

Inputs: 6 synthetic frames (se2lam_amd.synth) extracted on the device, a vocabulary trained on them on the device (k = 10,
L = 4), FeatureVectors from transform_batch_device at the two values of levelsup whose node counts lie nearest to 100 (the
reference's regime at levelsup = 4 with ORBvoc) and to 500.  Pairs are drawn with repetition from the 6 frames, seed 5.
The batch call is timed with HIP events on the matcher's stream around windows of back-to-back calls, divided by the number
of calls; the loop with the host clock around one pass over the pairs (every call of it ends in a synchronise).  Windows last
at least 0.5 s; medians over the timed windows with the 10th and 90th percentile.  Before anything is timed the batch rows are
compared with the loop's results, bit for bit.  Lane utilisation of k_bow_match_batch is computed from the feature vectors:
the share of the lanes of its distance chunks (64 lanes per chunk of a node of frame b) that hold a feature.
--trace-run makes 20 batch calls of one row (about 100 nodes, 64 pairs) and nothing else, for the kernel trace; --kernel-stats reads the
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

from se2lam_amd import capi, orb, synth, vocabulary as V  # noqa: E402
from se2lam_amd.matcher import ORBmatcher  # noqa: E402

NFRAMES, CAP, K, L = 6, 1024, 10, 4
NPAIRS = [1, 16, 64, 256]
TARGET_NODES = [100, 500]
NNRATIO = 0.6
TRACE_CALLS = 20
TRACE_ROW = (100, 64)   # (target nodes, pairs) of the row the kernel trace is taken at


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
    """the frames and, per levelsup, their feature vectors: on the device and downloaded"""

    def __init__(self):
        D = capi.DeviceArray
        imgs = synth.frames(NFRAMES)
        rows, cols = imgs.shape[1:]
        ex = orb.ORBextractor(max_batch=NFRAMES)
        self.d_kps, self.d_desc, self.d_cnt = D(NFRAMES * CAP * 28), D(NFRAMES * CAP * 32), D(NFRAMES * 4)
        d_img = D.from_numpy(imgs)
        ex.extract_batch_device(d_img.ptr, NFRAMES, rows, cols, self.d_kps.ptr, self.d_desc.ptr, self.d_cnt.ptr, CAP)
        ex.sync()
        self.cnt = self.d_cnt.to_numpy(np.int32, (NFRAMES,))
        self.kps = self.d_kps.to_numpy(capi.KP_DTYPE, (NFRAMES, CAP))
        self.desc = self.d_desc.to_numpy(np.uint8, (NFRAMES, CAP, 32))
        self.voc = V.Vocabulary.train(self.d_desc.ptr, self.d_cnt.ptr, K, L, cap=CAP, nframes=NFRAMES)
        self.ctx = V.BowContext(self.voc, CAP, NFRAMES)
        self.fv = {}
        for levelsup in range(L + 1):
            bw, bv, bn = D(4 * NFRAMES * CAP), D(8 * NFRAMES * CAP), D(4 * NFRAMES)
            fn, fp, fi, nn = D(4 * NFRAMES * CAP), D(4 * NFRAMES * (CAP + 1)), D(4 * NFRAMES * CAP), D(4 * NFRAMES)
            self.ctx.transform_batch_device(self.d_desc.ptr, self.d_cnt.ptr, CAP, NFRAMES, levelsup, bw.ptr, bv.ptr, bn.ptr, fn.ptr, fp.ptr,
                                            fi.ptr, nn.ptr)
            self.ctx.sync()
            h_nn = nn.to_numpy(np.int32, NFRAMES)
            h_fn, h_fp = fn.to_numpy(np.int32, (NFRAMES, CAP)), fp.to_numpy(np.int32, (NFRAMES, CAP + 1))
            h_fi = fi.to_numpy(np.int32, (NFRAMES, CAP))
            host = [(h_fn[f, :h_nn[f]].copy(), h_fp[f, :h_nn[f] + 1].copy(), h_fi[f, :h_fp[f, h_nn[f]]].copy()) for f in range(NFRAMES)]
            self.fv[levelsup] = {"device": (fn, fp, fi, nn), "host": host, "nodes": float(h_nn.mean())}

    def levelsup_near(self, nodes):
        return min(self.fv, key=lambda lv: abs(self.fv[lv]["nodes"] - nodes))


def node_shape(scene, levelsup, pairs):
    """node pairs per key-frame pair, features per node, and the lane utilisation of the distance chunks"""
    host = scene.fv[levelsup]["host"]
    npairs_nodes, used, lanes, sizes = [], 0, 0, []
    for a, b in pairs:
        (na, pa, _), (nb, pb, _) = host[a], host[b]
        common, ia, ib = np.intersect1d(na, nb, return_indices=True)
        npairs_nodes.append(len(common))
        m1, m2 = (pa[ia + 1] - pa[ia]).astype(np.int64), (pb[ib + 1] - pb[ib]).astype(np.int64)
        sizes += list(m2)
        used += int((m1 * m2).sum())
        lanes += int((m1 * ((m2 + 63) // 64) * 64).sum())
    return {"node_pairs_mean": float(np.mean(npairs_nodes)), "node_features_median": float(np.median(sizes)), "node_features_max": int(max(sizes)),
            "lane_utilisation": used / max(lanes, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bow_batch"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per row")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per row")
    ap.add_argument("--window-seconds", type=float, default=0.5)
    ap.add_argument("--trace-run", action="store_true", help="%d batch calls of the row %s and nothing else (for rocprofv3)" % (TRACE_CALLS, TRACE_ROW))
    ap.add_argument("--kernel-stats", default="", help="<TAG>_kernel_stats.csv of a --trace-run under rocprofv3")
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    D = capi.DeviceArray
    scene = Scene()
    mt = ORBmatcher(NNRATIO, max_features=CAP, max_batch=NFRAMES)
    timer = capi.Timer()
    rng = np.random.default_rng(5)
    result = {"commit": commit(a.commit), "machine": machine(), "frames": NFRAMES, "features": [int(c) for c in scene.cnt],
              "vocabulary": {"k": K, "L": L, "nodes": scene.voc.nodes, "words": scene.voc.words},
              "nodes_per_levelsup": {str(lv): scene.fv[lv]["nodes"] for lv in sorted(scene.fv)}, "nnratio": NNRATIO,
              "timing": "%d warm-up + %d timed windows of at least %.1f s" % (a.warmup, a.windows, a.window_seconds), "rows": []}
    for target in TARGET_NODES:
        levelsup = scene.levelsup_near(target)
        fn, fp, fi, nn = scene.fv[levelsup]["device"]
        host = scene.fv[levelsup]["host"]
        for P in NPAIRS:
            pairs = rng.integers(0, NFRAMES, (P, 2)).astype(np.int32)
            pa, pb = D.from_numpy(np.ascontiguousarray(pairs[:, 0])), D.from_numpy(np.ascontiguousarray(pairs[:, 1]))
            d_m, d_nm = D(4 * P * CAP), D(4 * P)

            def batch():
                mt.search_by_bow_batch_device(scene.d_kps.ptr, scene.d_desc.ptr, scene.d_cnt.ptr, CAP, NFRAMES, fn.ptr, fp.ptr, fi.ptr,
                                              nn.ptr, None, pa.ptr, pb.ptr, P, d_m.ptr, d_nm.ptr, bIfMPOnly=False)

            def loop():
                out = []
                for x, y in pairs:
                    k1, k2 = scene.kps[x, :scene.cnt[x]], scene.kps[y, :scene.cnt[y]]
                    d1, d2 = scene.desc[x, :scene.cnt[x]], scene.desc[y, :scene.cnt[y]]
                    out.append(mt.SearchByBoW(k1, d1, host[x], np.zeros(0, np.uint8), k2, d2, host[y], np.zeros(0, np.uint8), bIfMPOnly=False))
                return out
            if a.trace_run:
                if (target, P) == TRACE_ROW:
                    for _ in range(TRACE_CALLS):
                        batch()
                    mt.sync()
                continue
            batch(); mt.sync()
            m12, nm = d_m.to_numpy(np.int32, (P, CAP)), d_nm.to_numpy(np.int32, (P,))
            for p, (n_l, m_l) in enumerate(loop()):                         # the batch gives what the loop gives
                assert nm[p] == n_l and np.array_equal(m12[p, :len(m_l)], m_l) and (m12[p, len(m_l):] == -1).all(), (levelsup, P, p)

            def batch_window(calls):
                timer.start(mt.stream())
                for _ in range(calls):
                    batch()
                timer.stop(mt.stream())
                return timer.elapsed_ms()                                   # synchronises on the stop event
            calls = 20
            while True:                                                     # calls per window: at least window_seconds
                ms = batch_window(calls)
                if ms >= 1e3 * a.window_seconds:
                    break
                calls = int(calls * max(1.2, 1.2e3 * a.window_seconds / max(ms, 1e-3))) + 1
            dev = stats([batch_window(calls) / calls for w in range(a.warmup + a.windows)][a.warmup:])
            t0 = time.perf_counter(); loop(); one = time.perf_counter() - t0
            passes = max(1, int(np.ceil(a.window_seconds / one)))

            def loop_window():
                t1 = time.perf_counter()
                for _ in range(passes):
                    loop()
                return 1e3 * (time.perf_counter() - t1) / passes
            host_loop = stats([loop_window() for w in range(1 + a.windows)][1:])
            row = {"target_nodes": target, "levelsup": levelsup, "nodes_per_frame": scene.fv[levelsup]["nodes"], "npairs": P,
                   "matches_mean": float(nm.mean()), "batch_calls_per_window": calls, "loop_passes_per_window": passes,
                   "batch_events": dev, "loop_wall": host_loop, "loop_over_batch": host_loop["median_ms"] / dev["median_ms"]}
            row.update(node_shape(scene, levelsup, pairs))
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
    if a.trace_run:
        print("trace run: %d batch calls of the row %s" % (TRACE_CALLS, TRACE_ROW))
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
        name = re.sub(r"\(anonymous namespace\)::", "", r["Name"]).split("(")[0]
        rows.append({"kernel": name, "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "total_ms": float(r["TotalDurationNs"]) / 1e6})
    bow = [r for r in rows if r["kernel"] in ("k_bow_pair_nodes", "k_bow_match_batch", "k_bow_finish_batch")]
    total = sum(r["total_ms"] for r in bow)
    for r in bow:
        r["share"] = r["total_ms"] / total if total else 0.0
    return bow


def markdown(r):
    def c(s):
        return "%.3f (%.3f-%.3f)" % (s["median_ms"], s["p10_ms"], s["p90_ms"])
    o = ["# SearchByBoW: one batch call against one call per pair", "",
         "Written by `tools/search_bow_bench.py`.  Commit %s, %s.  %d synthetic frames of %s features, extracted on the device; vocabulary trained"
         " on them on the device (k = %d, L = %d: %d nodes, %d words); nodes per frame by levelsup: %s.  nnratio %.1f, orientation check on,"
         " bIfMPOnly = false.  Pairs drawn with repetition.  %s.  Times in ms per batch of pairs: median (10th-90th percentile)."
         % (r["commit"], r["machine"], r["frames"], "/".join(str(n) for n in sorted(set(r["features"]))), r["vocabulary"]["k"], r["vocabulary"]["L"],
            r["vocabulary"]["nodes"], r["vocabulary"]["words"], ", ".join("%s: %.0f" % kv for kv in r["nodes_per_levelsup"].items()), r["nnratio"],
            r["timing"]), "",
         "- batch: `se2gpu_search_by_bow_batch_device` on the device arrays, HIP events around a window of back-to-back calls / calls.",
         "- loop: the same pairs through `se2gpu_search_by_bow` one by one from the downloaded arrays, host clock around one pass"
         " (the only route before this entry point existed).", "",
         "| levelsup | nodes per frame | pairs | node pairs per pair | features per node of b (median / max) | matches per pair | batch (events) | loop (wall) | loop / batch | lane utilisation |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for w in r["rows"]:
        o.append("| %d | %.0f | %d | %.0f | %.0f / %d | %.0f | %s | %s | %.1f | %.1f %% |"
                 % (w["levelsup"], w["nodes_per_frame"], w["npairs"], w["node_pairs_mean"], w["node_features_median"], w["node_features_max"],
                    w["matches_mean"], c(w["batch_events"]), c(w["loop_wall"]), w["loop_over_batch"], 100 * w["lane_utilisation"]))
    o += ["", "Lane utilisation: of the 64 lanes of every distance chunk of `k_bow_match_batch` (one chunk per 64 features of the node of frame b,"
          " per feature of the node of frame a), the share that holds a feature; computed from the feature vectors, not measured."]
    if r.get("kernel_stats"):
        o += ["", "## Kernel split", "",
              "`rocprofv3 --kernel-trace --stats` over a run of its own (`--trace-run`: %d batch calls of the row with about %d nodes per frame and %d pairs):" % ((TRACE_CALLS,) + TRACE_ROW),
              "", "| kernel | calls | average, us | total, ms | share |", "|---|---|---|---|---|"]
        for k in r["kernel_stats"]:
            o.append("| %s | %d | %.2f | %.3f | %.1f %% |" % (k["kernel"], k["calls"], k["avg_us"], k["total_ms"], 100 * k["share"]))
        top = max(r["kernel_stats"], key=lambda k: k["share"])
        at = [w for w in r["rows"] if (w["target_nodes"], w["npairs"]) == TRACE_ROW]
        if top["kernel"] == "k_bow_match_batch" and at:
            o += ["", "`k_bow_match_batch` takes %.0f %% of the kernel time of that row while %.0f %% of the lanes of its distance chunks hold a feature"
                  " (nodes of %.0f features against waves of 64): most of every wave idles.  A sub-wave mapping (several nodes per wave) is the"
                  " follow-up this points to; it is not part of this entry point." % (100 * top["share"], 100 * at[0]["lane_utilisation"], at[0]["node_features_median"])]
    ahead = [w for w in r["rows"] if w["npairs"] >= 16]
    if ahead:
        o += ["", "From 16 pairs on the batch call is %.0f to %.0f times faster than the loop (1 pair: %s)." % (
            min(w["loop_over_batch"] for w in ahead), max(w["loop_over_batch"] for w in ahead),
            ", ".join("%.1f" % w["loop_over_batch"] for w in r["rows"] if w["npairs"] == 1))]
    o.append("")
    return "\n".join(o)


if __name__ == "__main__":
    main()
