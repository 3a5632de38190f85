"""scratch: start / end stamps of every workgroup of the last k_reduce2 of an optimize(10) on the headline window
usage (cwd = the tree whose binding fits the library): stamps_run.py LIB OUT.txt"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from se2lam_amd import capi  # noqa: E402

capi.LIB_PATH = os.path.abspath(sys.argv[1])
from se2lam_amd import synth  # noqa: E402
from se2lam_amd.optimizer import SlamOptimizer  # noqa: E402

g = synth.ba_graph(200, 20000)
P = g.P
# empty blocks: no shared landmark (fixed or not) and no edge
cov = np.zeros((P, P), bool)
ptr = np.searchsorted(g.e_lm, np.arange(g.L + 1))
for l in range(g.L):
    k = g.e_kf[ptr[l]:ptr[l + 1]]
    cov[np.ix_(k, k)] = True
cov[g.o_i, g.o_j] = cov[g.o_j, g.o_i] = True
o = SlamOptimizer()
o.load(g)
o.initializeOptimization(0)
n = C.c_int(0)
l = capi.lib()
capi.check(l.se2gpu_ba_debug_flat_records(o._h, None, None, 0, C.byref(n)))
grp, flat = np.zeros((n.value, 4), np.int32), np.zeros((n.value, 11, 4), np.int32)
capi.check(l.se2gpu_ba_debug_flat_records(o._h, grp.ctypes.data, flat.ctypes.data, n.value, C.byref(n)))
nwg = n.value // 28
blk = grp[:, 0].reshape(nwg, 28)
a_of, b_of = np.triu_indices(P, 0)   # block index order a * P - a (a - 1) / 2 + (b - a): row-major upper triangle
real = np.zeros(nwg, bool)
for w in range(nwg):
    ks = blk[w][blk[w] >= 0]
    real[w] = cov[a_of[ks], b_of[ks]].any()
launched = nwg
try:
    out = np.zeros(3, np.int32)
    capi.check(l.se2gpu_ba_debug_reduce_grid(o._h, out.ctypes.data))
    launched = int(out[2])
    print("reduce_grid", list(out))
except AttributeError:
    pass
ndiag = (P + 1 + 7) & ~7
npad = (launched + 7) & ~7
lines = []
for run in range(3):
    for _ in range(3):
        o.reset_estimates()
        o.optimize(10)
    st = np.zeros(4096 * 2, np.int64)
    capi.check(l.se2gpu_ba_debug_reduce_stamps(C.c_void_p(st.ctypes.data), C.c_int(st.size)))
    st = st.reshape(-1, 2)
    bid = np.arange(npad)
    wg = (bid & 7) * (npad >> 3) + (bid >> 3)
    ok = wg < launched
    s0, s1 = st[ndiag:ndiag + npad][ok], None
    t0 = min(st[:P, 0].min(), s0[:, 0].min())
    start, end = (s0[:, 0] - t0) / 100.0, (s0[:, 1] - t0) / 100.0    # us (100 MHz)
    dur = end - start
    if (dur <= 0).any():
        lines.append('   WARNING: %d workgroups with end <= start (a launch that returned early overwrote the start)' % int((dur <= 0).sum()))
    r = real[wg[ok]]
    dg0, dg1 = (st[:P, 0] - t0) / 100.0, (st[:P, 1] - t0) / 100.0
    q = lambda x, p: float(np.percentile(x, p)) if x.size else float("nan")
    lines.append("run %d: workgroups launched %d (real %d, all-empty %d) | kernel first start -> last end %.2f us | diagonal end max %.2f" %
                 (run, launched, int(r.sum()), int((~r).sum()), max(end.max(), dg1.max()), dg1.max()))
    lines.append("   real:      start median %.2f p90 %.2f max %.2f | duration median %.2f p90 %.2f max %.2f | end max %.2f" %
                 (q(start[r], 50), q(start[r], 90), start[r].max(), q(dur[r], 50), q(dur[r], 90), dur[r].max(), end[r].max()))
    if (~r).any():
        e = ~r
        lines.append("   all-empty: start median %.2f p90 %.2f max %.2f | duration median %.2f p90 %.2f max %.2f | end max %.2f" %
                     (q(start[e], 50), q(start[e], 90), start[e].max(), q(dur[e], 50), q(dur[e], 90), dur[e].max(), end[e].max()))
    late = start > 5.0
    lines.append("   workgroups that start later than 5 us: %d (real %d, all-empty %d); their duration median %.2f" %
                 (int(late.sum()), int((late & r).sum()), int((late & ~r).sum()), q(dur[late], 50)))
print("\n".join(lines))
open(sys.argv[2], "w").write("\n".join(lines) + "\n")
