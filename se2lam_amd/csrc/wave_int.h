// Integer sums, scans and ranks over a wave of 64 lanes and over a workgroup: the one definition behind every kernel that places
// its output by prefix sums instead of atomic counters.  int and long long only: a floating-point sum depends on its order and stays
// with the kernel that owns it.  Every function is called by all 64 lanes of a wave, with no divergence (block_scan_excl: by every
// thread of the workgroup); lane = threadIdx.x & 63.  Everything is force-inlined.
#pragma once
#include <hip/hip_runtime.h>

namespace se2gpu {

// the sum / minimum / maximum over the wave, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// the inclusive prefix sum over the wave: lane l returns v of the lanes 0..l
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
// the wave's total, given the result of wave_scan_incl, in every lane
template <typename T>
__device__ __forceinline__ T wave_last(T incl) { return __shfl(incl, 63); }

// the number of set bits of a ballot below this lane
__device__ __forceinline__ int lane_rank(unsigned long long mask) { return __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// The exclusive prefix sum of one value per thread over a workgroup of WAVES waves; total: the sum, the same in every thread.  s_w is
// WAVES words of LDS.  Two barriers: the one in front of the LDS write lets a loop call this again on the same s_w while a slower wave
// still reads the words of the round before.  FRESH = true drops it, and holds only where nothing has touched s_w since the
// workgroup's last barrier (or since the kernel began); each such call says why.
template <int WAVES, bool FRESH = false, typename T>
__device__ __forceinline__ T block_scan_excl(T v, T* s_w, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_scan_incl(v);
    if (!FRESH) __syncthreads();
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) base += s_w[w];
        total += s_w[w];
    }
    return base + incl - v;
}

}  // namespace se2gpu
