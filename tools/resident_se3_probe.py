"""GPU probe of the one-workgroup-per-window BA path for SE3-expmap windows (csrc/ba_window3.hip): parity against the multi-launch
k3_* path on a few windows (with the phase times of SE2GPU_BA_RESIDENT_TRACE=1), then LM iterations/s of uniform batches on path 0
(multi-launch, SE2GPU_BA_RESIDENT=0) and path 2 (resident, =1), the two paths alternating point by point.  Every point is timed with
the device synchronised (optimize_batch returns when every window has reported back), after a warm-up, over at least `min_s` seconds.
usage: python tools/resident_se3_probe.py [min_seconds] [counts...]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from se2lam_amd import capi, synth  # noqa: E402
from se2lam_amd import optimizer as op  # noqa: E402

SHAPE = (21, 800, 4)   # 21 key frames (4 of them fixed reference key frames), 800 landmarks


def opt_of(g):
    o = op.SlamOptimizer()
    op.load_se3_graph(o, g)
    o.initializeOptimization(0)
    return o


def parity():
    gs = [synth.ba3_graph(8, 60, 0), synth.ba3_graph(21, 800, 0), synth.ba3_graph(21, 800, 4), synth.ba3_graph(30, 2000, 6)]
    os.environ["SE2GPU_BA_RESIDENT"] = "0"
    ref = []
    for g in gs:
        o = opt_of(g)
        o.optimize(10)
        ref.append((o.stats, o.estimates()))
    os.environ["SE2GPU_BA_RESIDENT"] = "1"
    opts = [opt_of(g) for g in gs]
    op.optimize_batch(opts, 10)
    assert capi.lib().se2gpu_ba_last_batch_path() == 2
    worst = 0.0
    for g, o, (st, (p, l)) in zip(gs, opts, ref):
        pp, ll = o.estimates()
        rel = abs(o.stats["chi2_final"] - st["chi2_final"]) / st["chi2_final"]
        worst = max(worst, rel)
        same = o.stats["trials_hist"] == st["trials_hist"]
        print("P %3d L %5d E %6d  trials %s  chi2 %.12g | %.12g (rel %.1e)  dpose %.2e dlm %.2e" % (
            g.P, g.L, g.E, "equal" if same else "DIFFER", o.stats["chi2_final"], st["chi2_final"], rel,
            np.abs(pp - p).max(), np.abs(ll - l).max()), flush=True)
        assert same
    print("parity: worst relative chi2 difference %.1e" % worst, flush=True)


def trace():
    """phase times of the last trial of one window (the library prints them to stderr), in a child process: the switch is read once"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from se2lam_amd import synth, optimizer as op\n"
            "g = synth.ba3_graph(*%r)\n"
            "opts = []\n"
            "for _ in range(256):\n"
            "    o = op.SlamOptimizer(); op.load_se3_graph(o, g); o.initializeOptimization(0); opts.append(o)\n"
            "op.optimize_batch(opts, 10)\n") % (ROOT, SHAPE)
    env = dict(os.environ, SE2GPU_BA_RESIDENT="1", SE2GPU_BA_RESIDENT_TRACE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print("trace (256 windows of %s):" % (SHAPE,), r.returncode, flush=True)
    print("\n".join(l for l in r.stderr.splitlines() if "resident" in l), flush=True)


def time_point(opts, path, min_s):
    os.environ["SE2GPU_BA_RESIDENT"] = path
    for _ in range(2):                                      # warm-up: graphs captured, pools grown
        op.reset_estimates_batch(opts)
        op.optimize_batch(opts, 10)
    want = 2 if path == "1" else 0
    got = capi.lib().se2gpu_ba_last_batch_path()
    assert got == want or (path == "0" and got in (0, 1)), (path, got)
    reps, its, t_run = 0, 0, 0.0
    while t_run < min_s:
        op.reset_estimates_batch(opts)
        t0 = time.perf_counter()
        op.optimize_batch(opts, 10)                         # returns when every window has posted its last trial
        t_run += time.perf_counter() - t0
        its += sum(o.stats["iterations"] for o in opts)
        reps += 1
    return its / t_run, t_run / reps


def throughput(counts, min_s):
    g = synth.ba3_graph(*SHAPE)
    print("windows | path 0 LM it/s | path 2 LM it/s | ratio  (%s, optimize(10), >= %.1f s per point)" % (SHAPE, min_s), flush=True)
    for n in counts:
        opts = [opt_of(g) for _ in range(n)]
        r0, d0 = time_point(opts, "0", min_s)
        r2, d2 = time_point(opts, "1", min_s)
        print("%4d | %9.0f (%.2f ms) | %9.0f (%.2f ms) | %.2fx" % (n, r0, d0 * 1e3, r2, d2 * 1e3, r2 / r0), flush=True)
        del opts


if __name__ == "__main__":
    min_s = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
    parity()
    trace()
    throughput([int(a) for a in sys.argv[2:]] or [1, 32, 96, 256], min_s)
