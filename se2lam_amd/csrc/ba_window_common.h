// Helpers of the one-workgroup-per-window solver (csrc/ba_window_skeleton.h; its models csrc/ba_window.hip: SE(2)-XYZ, csrc/ba_window3.hip: SE3-expmap): cross-lane
// sums by DPP, the packed lower triangle, LDS atomics, the fast reciprocal (square root), the 3x3 landmark factor, the Huber
// weight, workgroup reductions.  Everything is force-inlined and internal to the translation unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// cross-lane moves without the LDS crossbar: DPP on the two halves of a double
// ------------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    const long long b = __double_as_longlong(v);
    int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    // (no "old" operand: every lane reads a lane of its own row, so nothing of the destination survives - with one, the compiler
    // copies the source first and a butterfly step costs five instructions instead of three)
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
constexpr int kDppXor1 = 0xB1;          // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;          // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;   // lane i <-> 7 - i inside every 8 lanes
constexpr int kDppMirror = 0x140;       // lane i <-> 15 - i inside every 16 lanes

// the sum over an aligned group of G lanes (4, 8, 16, 32 or 64), in every lane of the group
template <int G>
__device__ __forceinline__ double gsum(double v) {
    v += dpp_move<kDppXor1>(v);
    v += dpp_move<kDppXor2>(v);
    if (G >= 8) v += dpp_move<kDppHalfMirror>(v);
    if (G >= 16) v += dpp_move<kDppMirror>(v);
    if (G >= 32) v += __shfl_xor(v, 16);
    if (G >= 64) v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ double wsum(double v) { return gsum<64>(v); }
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ int tri(int r, int c) { return r * (r + 1) / 2 + c; }   // packed lower triangle, r >= c

// (a run-time debug switch lived here until r06q - plain read-modify-write instead of the atomic, the pair loop skipped: it put a
// branch around every one of the kernel's atomics and cut the schedule into as many pieces; the two timings it gave are in DESIGN.md)
__device__ __forceinline__ void lds_add(double* p, double v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// 1 / x and 1 / sqrt(x) from the hardware's seeds (v_rcp_f64 / v_rsq_f64: ~26 good bits) and two Newton steps: within an ulp or two of
// the correctly rounded value at 5 / 9 instructions, where the compiler's IEEE division and square root take 12 / 25
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    double h = 0.5 * x;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return y;
}

// A = G^-1 for M = h + lambda I = G G^T (badev::chol_inv3 with the reciprocal square roots above; the same pivot floor)
__device__ __forceinline__ void chol3(const double h[6], double lambda, double a[6]) {
    const double m00 = h[0] + lambda, m10 = h[1], m20 = h[2], m11 = h[3] + lambda, m21 = h[4], m22 = h[5] + lambda;
    const double floor_ = fmax(1e-30 * (m00 + m11 + m22), 1e-300);
    const double a00 = fast_rsqrt(fmax(m00, floor_));
    const double g10 = m10 * a00, g20 = m20 * a00;
    const double a11 = fast_rsqrt(fmax(m11 - g10 * g10, floor_));
    const double g21 = (m21 - g20 * g10) * a11;
    const double a22 = fast_rsqrt(fmax(m22 - g20 * g20 - g21 * g21, floor_));
    const double a10 = -(a11 * g10) * a00;
    const double a21 = -(a22 * g21) * a11;
    const double a20 = -(a21 * g10 + a22 * g20) * a00;
    a[0] = a00; a[1] = a10; a[2] = a11; a[3] = a20; a[4] = a21; a[5] = a22;
}

// RobustKernelHuber (badev::huber) without the branch and with the reciprocal square root above: sqrt(e2) = e2 rsqrt(e2)
__device__ __forceinline__ void huber_w(double e2, double delta, double& rho0, double& rho1) {
    const double dsqr = delta * delta;
    const double rs = fast_rsqrt(fmax(e2, 1e-300));
    const bool in = e2 <= dsqr;
    rho0 = in ? e2 : 2.0 * (e2 * rs) * delta - dsqr;
    rho1 = in ? 1.0 : delta * rs;
}

__device__ __forceinline__ double lane_value(double v, int src) {
    const long long bits = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(bits & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// workgroup sums of two values and a maximum; every thread gets the results
template <int NT>
__device__ __forceinline__ void wg_reduce(double* red, double& s0, double& s1, double& m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s0 = wsum(s0);
    s1 = wsum(s1);
    m = wmax(m);
    __syncthreads();
    if (lane == 0) { red[wave] = s0; red[8 + wave] = s1; red[16 + wave] = m; }
    __syncthreads();
    double a = 0, b = 0, mm = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) { a += red[w]; b += red[8 + w]; mm = fmax(mm, red[16 + w]); }   // fixed order
    s0 = a; s1 = b; m = mm;
}

}  // namespace
