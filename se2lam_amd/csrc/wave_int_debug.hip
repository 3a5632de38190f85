// Test introspection of wave_int.h: one workgroup of `block` threads walks n values in chunks of `block` and applies one function
// of the header to every chunk, so that a test reads what the batch kernels inline.  Lanes past n contribute the identity.
#include <climits>

#include "common.h"
#include "wave_int.h"

namespace se2gpu {
namespace {

// the workgroup exclusive scan of every chunk on top of the running total of the chunks before it: the looped use of one s_w
template <int BLOCK, bool FRESH, typename T>
__device__ __forceinline__ void scan_chunks(int n, const long long* __restrict__ in, long long* __restrict__ out, T* s_w) {
    T run = 0;
    for (int base = 0; base < n; base += BLOCK) {                   // uniform; FRESH: one chunk (the entry's check)
        const int i = base + (int)threadIdx.x;
        T total;
        // FRESH: s_w is untouched since the kernel began
        const T ex = block_scan_excl<BLOCK / 64, FRESH>(i < n ? (T)in[i] : (T)0, s_w, total);
        if (i < n) out[i] = (long long)(run + ex);
        run += total;
    }
    if (threadIdx.x == 0) out[n] = (long long)run;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_debug_wave_int(int op, int n, const long long* __restrict__ in, long long* __restrict__ out) {
    __shared__ int s_i[BLOCK / 64];
    __shared__ long long s_l[BLOCK / 64];
    switch (op) {                                                   // uniform
    case SE2GPU_WI_BLOCK_SCAN_I32: scan_chunks<BLOCK, false>(n, in, out, s_i); return;
    case SE2GPU_WI_BLOCK_SCAN_I64: scan_chunks<BLOCK, false>(n, in, out, s_l); return;
    case SE2GPU_WI_FRESH_SCAN_I32: scan_chunks<BLOCK, true>(n, in, out, s_i); return;
    case SE2GPU_WI_FRESH_SCAN_I64: scan_chunks<BLOCK, true>(n, in, out, s_l); return;
    default: break;
    }
    for (int base = 0; base < n; base += BLOCK) {                   // uniform: every shuffle sees all 64 lanes
        const int i = base + (int)threadIdx.x;
        const bool live = i < n;
        const long long x = live ? in[i] : 0;
        long long y = 0;
        switch (op) {
        case SE2GPU_WI_SUM: y = wave_sum((int)x); break;
        case SE2GPU_WI_MIN: y = wave_min(live ? (int)x : INT_MAX); break;
        case SE2GPU_WI_MAX: y = wave_max(live ? (int)x : INT_MIN); break;
        case SE2GPU_WI_SCAN_I32: y = wave_scan_incl((int)x); break;
        case SE2GPU_WI_SCAN_I64: y = wave_scan_incl(x); break;
        case SE2GPU_WI_RANK: y = lane_rank(__ballot(x != 0)); break;
        default: break;
        }
        if (live) out[i] = y;
    }
}

}  // namespace
}  // namespace se2gpu

extern "C" int se2gpu_debug_wave_int(int op, int block, int n, const long long* in, long long* out) {
    using namespace se2gpu;
    const char* who = "se2gpu_debug_wave_int";
    SE2_REQUIRE(op >= 0 && op < SE2GPU_WI_OPS, SE2GPU_ERR_INVALID, "%s: op %d is none of the %d", who, op, (int)SE2GPU_WI_OPS);
    SE2_REQUIRE(block == 64 || block == 256 || block == 1024, SE2GPU_ERR_INVALID, "%s: block = %d is none of 64, 256, 1024", who, block);
    SE2_REQUIRE(n >= 0 && n <= (1 << 20), SE2GPU_ERR_INVALID, "%s: n = %d outside [0, 2^20]", who, n);
    const bool fresh = op == SE2GPU_WI_FRESH_SCAN_I32 || op == SE2GPU_WI_FRESH_SCAN_I64;
    const bool scan = fresh || op == SE2GPU_WI_BLOCK_SCAN_I32 || op == SE2GPU_WI_BLOCK_SCAN_I64;
    SE2_REQUIRE(!fresh || n <= block, SE2GPU_ERR_INVALID, "%s: the FRESH scans take one chunk, n = %d > block = %d", who, n, block);
    SE2_NEED_IF(n > 0, in);
    SE2_NEED_IF(n > 0 || scan, out);
    if (n == 0) {
        if (scan) out[0] = 0;
        return SE2GPU_OK;
    }
    SE2_NEED_DEVICE();
    const size_t nout = (size_t)n + (scan ? 1 : 0);
    DevBuf<long long> d_in, d_out;
    SE2_CHECK(d_in.reserve(n));
    SE2_CHECK(d_out.reserve(nout));
    SE2_HIP(hipMemcpy(d_in.p, in, sizeof(long long) * n, hipMemcpyHostToDevice));
    if (block == 64) hipLaunchKernelGGL(k_debug_wave_int<64>, dim3(1), dim3(64), 0, 0, op, n, d_in.p, d_out.p);
    else if (block == 256) hipLaunchKernelGGL(k_debug_wave_int<256>, dim3(1), dim3(256), 0, 0, op, n, d_in.p, d_out.p);
    else hipLaunchKernelGGL(k_debug_wave_int<1024>, dim3(1), dim3(1024), 0, 0, op, n, d_in.p, d_out.p);
    SE2_HIP(hipGetLastError());
    SE2_HIP(hipMemcpy(out, d_out.p, sizeof(long long) * nout, hipMemcpyDeviceToHost));
    return SE2GPU_OK;
}
