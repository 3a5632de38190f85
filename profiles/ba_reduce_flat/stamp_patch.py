"""DATED RECORD, not a tool: the edits that put wall_clock64 stamps into d_reduce2 for section 0 of profiles/ba_reduce_flat.md,
as string replacements on csrc/ba.hip AS IT STOOD WHEN THE STAMPS WERE TAKEN (the variant that still had the per-pose PreEdgeSE2
lists inline).  The anchors are exact text of that state and will not match later revisions of the source; it is kept to show
where each stamp sat, and stamps_summary.py beside it shows how stamps_summary.txt was computed from them.  The stamped library
was never shipped."""
import sys
src, dst = sys.argv[1], sys.argv[2]
s = open(src).read()

def rep(old, new, count=1):
    global s
    assert s.count(old) >= 1, old
    s = s.replace(old, new, count)

# globals + macros in front of d_reduce2's helpers
rep("constexpr int kFlatQ = 11;",
    """constexpr int kFlatQ = 11;
__device__ long long g_r2_stamps[4096 * 8];
#define R2S(i) do { if (threadIdx.x == 0 && bx < 4096) g_r2_stamps[(size_t)bx * 8 + (i)] = wall_clock64(); } while (0)
#define R2S_T(i, T) do { if ((int)threadIdx.x == (T) && bx < 4096) g_r2_stamps[(size_t)bx * 8 + (i)] = wall_clock64(); } while (0)
#define R2USE(v) asm volatile("" ::"v"(v))""")
# off-diagonal: start
rep("        const int wg = (bid & 7) * (nwg_pad >> 3) + (bid >> 3);\n        if (wg >= ra.nwg_off) return;",
    "        const int wg = (bid & 7) * (nwg_pad >> 3) + (bid >> 3);\n        if (wg >= ra.nwg_off) return;\n        R2S(0);")
# record / descriptor there (after the controller too)
rep("        const int r = en / 3, c = en - 3 * r;\n        double acc0 = 0, acc1 = 0;",
    "        R2USE(d.x); R2USE(fq.x);\n        R2S(1);\n        const int r = en / 3, c = en - 3 * r;\n        double acc0 = 0, acc1 = 0;")
# indices there (legacy: pair + block descriptor loads) ; flat: same moment
rep("            // The block's PreEdgeSE2 term (the group that combines the block adds it): with the flat record",
    "            R2USE(my_i0); R2USE(my_j1); R2USE(ca); R2USE(cb); R2USE(od);\n            R2S(2);\n            // The block's PreEdgeSE2 term (the group that combines the block adds it): with the flat record")
# before-loop odo done
rep("            // The group loads every word ONCE", "            R2S(3);\n            // The group loads every word ONCE")
# after round 1 (first iteration) and after all rounds
rep("                    acc1 += w1 * (y[1][0] * hh[1][0] + y[1][1] * hh[1][1] + y[1][2] * hh[1][2]);\n                }\n            }\n            part[g][en] = acc0 + acc1;",
    "                    acc1 += w1 * (y[1][0] * hh[1][0] + y[1][1] * hh[1][1] + y[1][2] * hh[1][2]);\n                }\n                if (q == d.y) { R2USE(acc0); R2USE(acc1); R2S(4); }\n            }\n            R2USE(acc0); R2USE(acc1);\n            R2S(5);\n            part[g][en] = acc0 + acc1;")
rep("        __syncthreads();\n        if (d.x >= 0 && (d.w & 0xff) == g) {\n            const int ng = d.w >> 8;",
    "        __syncthreads();\n        R2S(6);\n        if (d.x >= 0 && (d.w & 0xff) == g) {\n            const int ng = d.w >> 8;")
rep("            ra.S[(size_t)(cb + c) * ra.ld + ca + r] = out;\n        }\n        return;",
    "            ra.S[(size_t)(cb + c) * ra.ld + ca + r] = out;\n            R2USE(out);\n        }\n        R2S(7);\n        return;")
# diagonal
rep("    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // S diag (6 sym), bp (3), g (3)",
    "    R2S(0);\n    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // S diag (6 sym), bp (3), g (3)")
rep("            o[9 + r] = J[r] * omr[0] + J[3 + r] * omr[1] + J[6 + r] * omr[2];\n        }\n    }",
    "            o[9 + r] = J[r] * omr[0] + J[3 + r] * omr[1] + J[6 + r] * omr[2];\n        }\n        R2S_T(3, kBlock - 8);\n    }")
rep("                ee[u] = ra.pose_edges[e0 + min(t, ne - 1)];\n            }",
    "                ee[u] = ra.pose_edges[e0 + min(t, ne - 1)];\n            }\n            if (base == 0) { R2USE(ee[0]); R2USE(ee[3]); R2S(1); }")
rep("#pragma unroll\n    for (int i = 0; i < 12; ++i) acc[i] = wave_sum(acc[i]);",
    "    R2USE(acc[0]); R2USE(acc[11]);\n    R2S(2);\n#pragma unroll\n    for (int i = 0; i < 12; ++i) acc[i] = wave_sum(acc[i]);")
rep("    __syncthreads();\n    if (threadIdx.x < 12) {  // entries 0..8",
    "    __syncthreads();\n    R2S(6);\n    if (threadIdx.x < 12) {  // entries 0..8")
rep("            ra.bp[(size_t)p * 3 + r] = fa ? 0.0 : v;\n        }\n    }\n}",
    "            ra.bp[(size_t)p * 3 + r] = fa ? 0.0 : v;\n        }\n    }\n    R2S(7);\n}")
# accessor
rep("// k_plan_flat's record builder (flat_record, the function the kernel calls) on host arrays",
    """extern "C" int se2gpu_ba_debug_reduce_stamps(long long* out, int n) {
    SE2_HIP(hipDeviceSynchronize());
    SE2_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_r2_stamps), (size_t)n * sizeof(long long)));
    return SE2GPU_OK;
}
// k_plan_flat's record builder (flat_record, the function the kernel calls) on host arrays""")
open(dst, "w").write(s)
