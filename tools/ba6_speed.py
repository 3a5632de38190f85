"""optimize(10) wall time of the two 6-DoF workloads, ba3_graph(50, 5000, 10) and pose_graph(200), with one build of the library:
median / min / max over --reps timed runs after 5 warm-ups, as one JSON line.  For A/B runs of two builds in alternating fresh
processes (profiles/ba_6dof_args.md).

    python tools/ba6_speed.py [--lib path/to/libse2gpu.so] [--tag name] [--reps 40]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def bench(o, reps):
    ts = []
    for r in range(reps + 5):
        o.reset_estimates()
        t0 = time.perf_counter()
        n = o.optimize(10)           # returns after the run has ended on the stream (the host waits for the last slot)
        t1 = time.perf_counter()
        assert n == 10
        if r >= 5:
            ts.append((t1 - t0) * 1e3)
    return [round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)]


def run(tag, reps):
    from se2lam_amd import optimizer as op, synth
    res = {"tag": tag}
    o = op.SlamOptimizer()
    op.load_se3_graph(o, synth.ba3_graph(50, 5000, 10))
    o.initializeOptimization(0)
    res["ba3_50_5000_10_ms"] = bench(o, reps)
    res["ba3_chi2_final"] = o.stats["chi2_hist"][-1]
    del o
    o = op.SlamOptimizer()
    op.load_pose_graph(o, synth.pose_graph(200))
    o.initializeOptimization(0)
    res["pg_200_ms"] = bench(o, reps)
    res["pg_chi2_final"] = o.stats["chi2_hist"][-1]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="load this build of libse2gpu.so instead of the tree's")
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--reps", type=int, default=40)
    args = ap.parse_args()
    if args.lib:
        from se2lam_amd import capi
        capi.LIB_PATH = os.path.abspath(args.lib)
    run(args.tag, args.reps)
