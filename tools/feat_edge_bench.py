#!/usr/bin/env python3
"""Feature constraints over batches of key-frame pairs: se2gpu_feat_edge_batch with 1 / 16 / 256 pairs per call against the
same pairs one call each (what a caller who follows the reference's per-pair GlobalMapper::CreateFeatEdge would do).

    python tools/feat_edge_bench.py [--out profiles/feat_edge_bench.json] [--mode match|covis]

Inputs: tests/feat_edge_cases.make_pair with 90 .. 110 points per pair (drawn per pair, seed 7), the reference's 30 / 15
iterations.  Host clock around whole calls (host buffers in, host buffers out: uploads, both kernels, downloads) after two
warm-up calls; windows of at least 0.3 s, the median per-call time over the windows with the 10th and 90th percentile.  There
is no speed criterion: the parent commit has no such call and g2o is not installed here."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feat_edge_cases as fc  # noqa: E402
from se2lam_amd import capi, feat_edge as fe  # noqa: E402

NPAIRS = [1, 16, 256]


def timed(fn, min_window=0.3, windows=7):
    fn(); fn()
    out = []
    for _ in range(windows):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= min_window:
                break
        out.append(1e3 * dt / n)
    out.sort()
    return {"median_ms": statistics.median(out), "p10_ms": out[int(0.1 * (len(out) - 1))], "p90_ms": out[int(round(0.9 * (len(out) - 1)))],
            "windows": len(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default="match", choices=["match", "covis"])
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    mode = fe.MATCH if a.mode == "match" else fe.COVIS
    iters, minp = (fe.MATCH_ITERS, fe.MATCH_MIN_POINTS) if mode == fe.MATCH else (fe.COVIS_ITERS, fe.COVIS_MIN_POINTS)
    rng = np.random.default_rng(7)
    pairs = [fc.as_tuple(fc.make_pair(int(rng.integers(90, 111)), 500 + i)) for i in range(max(NPAIRS))]
    rows = []
    for n in NPAIRS:
        flat = fe.flatten(pairs[:n])
        singles = [fe.flatten(pairs[i:i + 1]) for i in range(n)]

        def batch():
            rc, o = fe.feat_edge_raw(n, mode, iters, minp, *flat)
            capi.check(rc)
            return o

        def loop():
            for f in singles:
                capi.check(fe.feat_edge_raw(1, mode, iters, minp, *f)[0])

        o = batch()
        assert (o["info4"][:, 0] == 0).all(), "every pair of the bench must produce a constraint"
        tb, tl = timed(batch), timed(loop)
        row = {"pairs": n, "points": int(flat[1][n]), "trials": int(sum(o["stats"][p].trials for p in range(n))), "batch": tb, "one_call_each": tl,
               "us_per_pair_batch": 1e3 * tb["median_ms"] / n, "us_per_pair_loop": 1e3 * tl["median_ms"] / n}
        rows.append(row)
        print("%4d pairs (%5d points): batch %.3f ms (%.1f us / pair), one call each %.3f ms (%.1f us / pair)"
              % (n, row["points"], tb["median_ms"], row["us_per_pair_batch"], tl["median_ms"], row["us_per_pair_loop"]), flush=True)
    res = {"mode": a.mode, "iters": iters, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
