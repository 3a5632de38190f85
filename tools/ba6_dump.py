"""Outputs of the two 6-DoF pose models (SE3-expmap local BA, pose graph) on small seeded graphs, into one .npz: for A/B runs of
two builds of the library (profiles/ba_6dof_args.md).  No reference, no fixtures.

    python tools/ba6_dump.py --out a.npz [--lib path/to/libse2gpu.so]
    python tools/ba6_dump.py --compare parent1.npz parent2.npz change.npz

Per case: the reduced system at two dampings before and after optimize(10), the final poses and landmarks, the LM histories and
edgeChi2.  --compare: which arrays the first two files (the same build, run twice) reproduce bit for bit, and whether the third
equals the first in those; for the others the largest difference of each pair.
"""
import argparse
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _dump(o, op, g, n_edges, out, tag, iters=10):
    for when in ("pre", "post"):
        if when == "post":
            assert o.optimize(iters) == iters
        for lam in (0.0, 0.7):
            S, b = o.reduced_system(lam)
            out[f"{tag}/S_{when}_{lam}"] = S
            out[f"{tag}/b_{when}_{lam}"] = b
    poses, lms = o.estimates()
    out[f"{tag}/poses"] = poses
    out[f"{tag}/landmarks"] = lms
    for k in ("chi2_hist", "lambda_hist", "trials_hist"):
        out[f"{tag}/{k}"] = np.asarray(o.stats[k])
    out[f"{tag}/edgeChi2"] = op.edgeChi2(o, n_edges)


def run(out_path):
    from se2lam_amd import optimizer as op, synth, capi
    out = {}
    ba3 = [("ba3_%d_%d_%d" % s, synth.ba3_graph(*s)) for s in ((8, 60, 0), (21, 800, 4), (50, 5000, 10))]
    ba3.append(("ba3_21_800_4_hub9", synth.odometry_topology3(synth.ba3_graph(21, 800, 4), "hub9")))
    for tag, g in ba3:
        o = op.SlamOptimizer()
        op.load_se3_graph(o, g)
        o.initializeOptimization(0)
        _dump(o, op, g, g.E, out, tag)
    for P in (12, 60):
        g = synth.pose_graph(P)
        o = op.SlamOptimizer()
        op.load_pose_graph(o, g)
        o.initializeOptimization(0)
        _dump(o, op, g, g.O, out, "pg_%d" % P)
    # GlobalBA's second pass: three gross feature edges, rejected by their chi2 after a first run, then the same optimizer again
    g = copy.copy(synth.pose_graph(60))
    g.o_meas = g.o_meas.copy()
    for k in (7, 40, 111):
        g.o_meas[k] = g.o_meas[k].copy()
        g.o_meas[k][2, 3] += 800.0
    o = op.SlamOptimizer()
    op.load_pose_graph(o, g)
    o.initializeOptimization(0)
    o.optimize(8)
    for k in np.nonzero(op.edgeChi2(o, g.O) > 30.0)[0]:
        capi.check(capi.lib().se2gpu_ba_set_edge_level(o._h, int(k), 1))
    o.initializeOptimization(0)
    _dump(o, op, g, g.O, out, "pg_60_relevel", iters=8)
    np.savez(out_path, **out)
    print("wrote", out_path, len(out), "arrays")


def compare(a_path, b_path, c_path):
    a, b, c = np.load(a_path), np.load(b_path), np.load(c_path)
    assert set(a.files) == set(b.files) == set(c.files)
    bad = 0
    nrep = 0
    for k in sorted(a.files):
        if a[k].tobytes() == b[k].tobytes():
            nrep += 1
            if c[k].tobytes() != a[k].tobytes():
                bad += 1
                print("DIFFERS  %-40s max |change - parent| = %.3e" % (k, np.abs(c[k] - a[k]).max()))
        else:
            dp, dc = np.abs(a[k] - b[k]).max(), np.abs(c[k] - a[k]).max()
            inside = dc <= dp
            bad += 0 if inside else 1
            print("parent does not reproduce %-40s parent/parent %.3e change/parent %.3e %s" % (k, dp, dc, "inside" if inside else "OUTSIDE"))
    print("%d arrays, %d reproduced by the parent run to run, %d failures" % (len(a.files), nrep, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--lib", help="load this build of libse2gpu.so instead of the tree's")
    ap.add_argument("--compare", nargs=3, metavar=("PARENT1", "PARENT2", "CHANGE"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.lib:
        from se2lam_amd import capi
        capi.LIB_PATH = os.path.abspath(args.lib)
    run(args.out)
