"""DATED RECORD of a scratch build that was never shipped, not a tool: wall_clock64 stamps at the start and the end of every
workgroup of d_reduce2 (thread 0), as string replacements on csrc/ba.hip as it stood for profiles/ba_reduce_empty.md section 1.
usage: stamp_patch.py SRC DST"""
import sys
src, dst = sys.argv[1], sys.argv[2]
s = open(src).read()


def rep(old, new):
    global s
    assert s.count(old) == 1, (s.count(old), old)
    s = s.replace(old, new)


rep("constexpr int kFlatQ = 11;",
    """constexpr int kFlatQ = 11;
__device__ long long g_r2_stamps[4096 * 2];
#define R2S(i) do { if (threadIdx.x == 0 && bx < 4096) g_r2_stamps[(size_t)bx * 2 + (i)] = wall_clock64(); } while (0)""")
rep("        const int lane = threadIdx.x & 63, gw = lane / 9, en = lane - 9 * gw;\n        const int g = gw < 7",
    "        R2S(0);\n        const int lane = threadIdx.x & 63, gw = lane / 9, en = lane - 9 * gw;\n        const int g = gw < 7")
rep("            ra.S[(size_t)(cb + c) * ra.ld + ca + r] = out;\n        }\n        return;",
    "            ra.S[(size_t)(cb + c) * ra.ld + ca + r] = out;\n        }\n        __syncthreads();\n        R2S(1);\n        return;")
rep("    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // S diag (6 sym), bp (3), g (3)",
    "    R2S(0);\n    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // S diag (6 sym), bp (3), g (3)")
rep("            ra.bp[(size_t)p * 3 + r] = fa ? 0.0 : v;\n        }\n    }\n}",
    "            ra.bp[(size_t)p * 3 + r] = fa ? 0.0 : v;\n        }\n    }\n    __syncthreads();\n    R2S(1);\n}")
rep("// k_plan_flat's record builder (flat_record, the function the kernel calls) on host arrays",
    """extern "C" int se2gpu_ba_debug_reduce_stamps(long long* out, int n) {
    SE2_HIP(hipDeviceSynchronize());
    SE2_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_r2_stamps), (size_t)n * sizeof(long long)));
    return SE2GPU_OK;
}
// k_plan_flat's record builder (flat_record, the function the kernel calls) on host arrays""")
open(dst, "w").write(s)
