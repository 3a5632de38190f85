// libse2gpu - SE3-expmap local bundle adjustment, ONE WORKGROUP PER WINDOW.
//
// Replaces, per window of a batch, what the multi-launch k3_* kernels of csrc/ba.hip run for the library's second landmark model
// (pose model 1: Map::loadLocalGraph(opt, vpEdgesAll, vnAllIdx) + LocalMapper::removeOutlierChi2):
//   [3P g2o 20160424] VertexSE3Expmap, EdgeProjectXYZ2UV, EdgeSE3ExpmapPrior, EdgeSE3Expmap, SE3Quat - restated as in oracle/ba3_ref.cpp
// with the structure of the SE(2) kernel (csrc/ba_window.hip): a workgroup owns a window for its whole
// optimize(iters), the poses, the reduced system S and its solution never leave LDS, the LM controller runs in the workgroup.
//   OPEN    the landmarks are listed by observation count and the observations copied into that order (28 B each: u v, w, key frame);
//           one pass gives chi^2 of the starting state (projection edges, priors, odometry) and, for LM, the diagonal for lambda_0
//           (k3_pose_diag + k_maxdiag: the landmarks' Hll and the free poses' un-reduced blocks)
//   BUILD   one lane per observation, 4 / 8 / 16 / 64 lanes per landmark: proj3<true>, Huber on w |e|^2, Hll / bl by DPP sums, the
//           factor A = G^-1 of Hll + lambda I, W_e = Hpl_e A^T (6 x 3, registers); Hpp_e - W_e W_e^T (21) and b_e - W_e zeta (6) go to
//           S by LDS atomics, the pair products W_i W_j^T (36 per pair, each pair once) through the per-wave strip; one lane per pose
//           adds its prior (Omega, Omega e) and one per odometry edge its blocks (Oii, Ojj, Oij, obi, obj as k3_terms computes them)
//   SOLVE   left-looking LL^T on 6 x 6 blocks in LDS with the right-hand side as an extra block row; x = L^-T y by one wave
//   UPDATE  the observations stream in again, the Jacobians are recomputed for the back-substitution x_l = A^T A (bl - q) (A from the
//           build pass through WindowArgs::ainv), exp(dx) T for the free poses (k3_oplus), robust chi^2 of the trial state
//           (projection edges, priors, odometry) and the gain denominator; lm_advance decides
// Sums into S are atomic, hence in no fixed order: results agree with the multi-launch path to rounding, not bit for bit.
//
// A landmark with more than 64 observations is refused (BaCtl::error = 2: the caller runs the window on the multi-launch path).
#include "ba_window.h"
#include "ba_window_common.h"
#include "se3_math.h"

using namespace se2gpu;
using namespace se2gpu::badev;

namespace {

constexpr int kStage3 = 19;   // per lane in the staging strip: W_e (18) + the column of the edge's pose (1)

enum { kEval = 0, kDiag = 1, kUpdate = 3 };

struct Ctx3 {
    const Window3Args* a;
    double* S;          // packed lower triangle of the augmented system, rows 0 .. n-1 = S, row n = b_s, rows n+1 .. n+5 zero
    double* x;          // n: the pose step (scratch of the lambda_0 pass: the diagonal of Hpp)
    const double* cur;  // 12P: the estimate
    const double* trl;  // 12P: the trial state
    const int* col;     // P: first column of a pose in the system, -1 = fixed
    double* stage;      // this wave's staging strip: 64 lanes x kStage3
    const double* lms;  // L x 3: the estimate's landmarks
    double* lms_trial;  // L x 3: the other buffer
    const int4* desc;   // L: {landmark, first record, observations, first edge}, class by class (made by the prologue)
    const double2* r_uv;   // the observations of the landmarks with at most 16 of them, in the order of that list
    const double* r_w;
    const int* r_kf;
    int n;
    double lambda;
};

struct Edge3 {
    int kf;
    double u, v, w;
};
struct Group3 {
    int l, beg, k, at;   // landmark, first record, observations, place in the list
    double lx, ly, lz;
    Edge3 ed;
    bool has;
};

__device__ __forceinline__ Edge3 load_edge3(const Window3Args& a, int e) {
    Edge3 r;
    r.kf = a.e_kf[e];
    const double2 uv = reinterpret_cast<const double2*>(a.e_uv)[e];
    r.u = uv.x; r.v = uv.y;
    r.w = a.e_info[3 * (size_t)e];
    return r;
}
__device__ __forceinline__ int4 load_desc(const Ctx3& c, int idx, int end) {
    return idx < end ? c.desc[idx] : make_int4(0, 0, 0, 0);
}
// FIRST: the opening pass - the observations come from the caller's arrays and go to the record arrays on the way
template <int G, bool FIRST = false>
__device__ __forceinline__ Group3 load_group(const Ctx3& c, const int4 d, int lane, int at) {
    const Window3Args& a = *c.a;
    Group3 g;
    g.l = d.x; g.beg = d.y; g.k = d.z; g.at = at; g.lx = 0; g.ly = 0; g.lz = 1; g.has = false;
    g.ed = Edge3{0, 0, 0, 0};
    if (g.k > 0) {
        g.lx = c.lms[3 * (size_t)g.l]; g.ly = c.lms[3 * (size_t)g.l + 1]; g.lz = c.lms[3 * (size_t)g.l + 2];
        const int sub = lane & (G - 1);
        g.has = sub < g.k;
        if (g.has) {
            if (G == 64) {
                g.ed = load_edge3(a, g.beg + sub);   // (a wave per landmark: its observations lie together in the caller's arrays)
            } else if (FIRST) {
                g.ed = load_edge3(a, d.w + sub);
                const int e = g.beg + sub;
                const_cast<double2*>(c.r_uv)[e] = double2{g.ed.u, g.ed.v};
                const_cast<double*>(c.r_w)[e] = g.ed.w;
                const_cast<int*>(c.r_kf)[e] = g.ed.kf;
            } else {
                const int e = g.beg + sub;
                const double2 uv = c.r_uv[e];
                g.ed.kf = c.r_kf[e];
                g.ed.u = uv.x; g.ed.v = uv.y;
                g.ed.w = c.r_w[e];
            }
        }
    }
    return g;
}

// EVAL / DIAG / UPDATE of one landmark (the SE(2) kernel's eval_group with EdgeProjectXYZ2UV: information w I, 2 x 6 pose Jacobian)
template <int MODE, int G>
__device__ __forceinline__ void eval_group(const Ctx3& c, const Group3& g, int lane, double& chi, double& scale, double& dmax) {
    const Window3Args& a = *c.a;
    const int sub = lane & (G - 1);
    const bool has = g.has;
    const int kf = g.ed.kf;
    const double w = g.ed.w;
    const double* T = c.cur + 12 * kf;
    double e0, e1;
    if (MODE == kEval) {
        proj3<false>(a.cam, T, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, nullptr, nullptr);
        double r0, r1;
        huber_w(w * (e0 * e0 + e1 * e1), a.cam.huber, r0, r1);
        if (has) chi += r0;
        return;
    }
    const int c0 = has ? c.col[kf] : -1;
    double2 A01 = {1, 0}, A23 = {1, 0}, A45 = {0, 1};
    if (MODE == kUpdate && g.k > 0) {
        const double2* src = reinterpret_cast<const double2*>(a.ainv + 6 * (size_t)g.at);
        A01 = src[0]; A23 = src[1]; A45 = src[2];
    }
    double Jp[12], Jl[6];
    proj3<true>(a.cam, T, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, Jp, Jl);
    double r0, r1;
    huber_w(w * (e0 * e0 + e1 * e1), a.cam.huber, r0, r1);
    if (MODE == kDiag && has) chi += r0;                       // (the lambda_0 pass is the chi^2 of the starting state as well)
    const double W = r1 * w, o0 = -W * e0, o1 = -W * e1;      // weighted information, omega_r
    double acc[12];   // hll diagonal (the lambda_0 pass only) | bl (3) | q (3)
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = 0.0;
    if (MODE == kDiag) {
        acc[0] = W * (Jl[0] * Jl[0] + Jl[3] * Jl[3]);
        acc[3] = W * (Jl[1] * Jl[1] + Jl[4] * Jl[4]);
        acc[5] = W * (Jl[2] * Jl[2] + Jl[5] * Jl[5]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) acc[6 + r] = Jl[r] * o0 + Jl[3 + r] * o1;
    acc[9] = acc[10] = acc[11] = 0.0;
    if (c0 >= 0) {
        if (MODE == kDiag) {
#pragma unroll
            for (int r = 0; r < 6; ++r) lds_add(c.x + c0 + r, W * (Jp[r] * Jp[r] + Jp[6 + r] * Jp[6 + r]));
        } else {
            double v0 = 0.0, v1 = 0.0;   // Jp dp
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double d = c.x[c0 + r];
                v0 += Jp[r] * d;
                v1 += Jp[6 + r] * d;
            }
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[9 + m] = W * (Jl[m] * v0 + Jl[3 + m] * v1);   // Hlp_e dp_e
            scale += v0 * o0 + v1 * o1;                                                  // dp . b_e
        }
    }
    if (!has) {   // (its arithmetic ran on a made-up edge and may hold infinities: nothing of it may reach the group's sums)
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    }
    if (MODE == kDiag) {   // lambda_0 = 1e-5 max diag H (computeLambdaInit): the landmark blocks' diagonals
        const double h0 = gsum<G>(acc[0]), h3 = gsum<G>(acc[3]), h5 = gsum<G>(acc[5]);
        if (g.k > 0) dmax = fmax(dmax, fmax(fabs(h0), fmax(fabs(h3), fabs(h5))));
        return;
    }
    const double ble[3] = {acc[6], acc[7], acc[8]};
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[6 + i] = gsum<G>(acc[6 + i] - acc[9 + i]);
    double xl[3] = {0, 0, 0};
    if (g.k > 0) {
        const double A[6] = {A01.x, A01.y, A23.x, A23.y, A45.x, A45.y};
        const double g0 = acc[6], g1 = acc[7], g2 = acc[8];
        const double t0 = A[0] * g0, t1 = A[1] * g0 + A[2] * g1, t2 = A[3] * g0 + A[4] * g1 + A[5] * g2;    // A (bl - q)
        xl[0] = A[0] * t0 + A[1] * t1 + A[3] * t2;                                                           // A^T (...)
        xl[1] = A[2] * t1 + A[4] * t2;
        xl[2] = A[5] * t2;
    }
    const double nxl = g.lx + xl[0], nyl = g.ly + xl[1], nzl = g.lz + xl[2];
    scale += xl[0] * ble[0] + xl[1] * ble[1] + xl[2] * ble[2];
    if (g.k > 0 && sub == 0) {
        c.lms_trial[3 * (size_t)g.l] = nxl; c.lms_trial[3 * (size_t)g.l + 1] = nyl; c.lms_trial[3 * (size_t)g.l + 2] = nzl;
        scale += c.lambda * (xl[0] * xl[0] + xl[1] * xl[1] + xl[2] * xl[2]);
    }
    if (has) {   // robust chi^2 of the observation at the trial state
        proj3<false>(a.cam, c.trl + 12 * kf, nxl, nyl, nzl, g.ed.u, g.ed.v, e0, e1, nullptr, nullptr);
        double q0, q1;
        huber_w(w * (e0 * e0 + e1 * e1), a.cam.huber, q0, q1);
        chi += q0;
    }
}

template <int MODE, int G, int NT, bool FIRST = false>
__device__ __forceinline__ void eval_class(const Ctx3& c, int begin, int end, double& chi, double& scale, double& dmax) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (begin >= end) return;
    constexpr int kStep = NT / G;
    Group3 nx = load_group<G, FIRST>(c, load_desc(c, begin + tid / G, end), lane, begin + tid / G);
    int4 d2 = load_desc(c, begin + kStep + tid / G, end);
    for (int i0 = begin; i0 < end; i0 += kStep) {
        const Group3 g = nx;
        nx = load_group<G, FIRST>(c, d2, lane, i0 + kStep + tid / G);
        d2 = load_desc(c, i0 + 2 * kStep + tid / G, end);
        eval_group<MODE, G>(c, g, lane, chi, scale, dmax);
    }
}
template <int NT>
__device__ __forceinline__ void copy_unobserved(const Ctx3& c, int end) {
    for (int i = threadIdx.x; i < end; i += NT) {
        const int l = c.desc[i].x;
#pragma unroll
        for (int m = 0; m < 3; ++m) c.lms_trial[3 * (size_t)l + m] = c.lms[3 * (size_t)l + m];
    }
}

// BUILD of one landmark
template <int G>
__device__ __forceinline__ void build_group(const Ctx3& c, const Group3& g, int lane) {
    const Window3Args& a = *c.a;
    const int sub = lane & (G - 1);
    const int k = g.k;
    const bool has = g.has;
    const int kf = g.ed.kf;
    const double w = g.ed.w;
    const int c0 = has ? c.col[kf] : -1;
    double e0, e1, Jp[12], Jl[6];
    proj3<true>(a.cam, c.cur + 12 * kf, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, Jp, Jl);
    double r0, r1;
    huber_w(w * (e0 * e0 + e1 * e1), a.cam.huber, r0, r1);
    const double W = r1 * w, o0 = -W * e0, o1 = -W * e1;
    double hll[6], b[3];
    hll[0] = W * (Jl[0] * Jl[0] + Jl[3] * Jl[3]);
    hll[1] = W * (Jl[0] * Jl[1] + Jl[3] * Jl[4]);
    hll[2] = W * (Jl[0] * Jl[2] + Jl[3] * Jl[5]);
    hll[3] = W * (Jl[1] * Jl[1] + Jl[4] * Jl[4]);
    hll[4] = W * (Jl[1] * Jl[2] + Jl[4] * Jl[5]);
    hll[5] = W * (Jl[2] * Jl[2] + Jl[5] * Jl[5]);
#pragma unroll
    for (int r = 0; r < 3; ++r) b[r] = Jl[r] * o0 + Jl[3 + r] * o1;
    if (!has) {
#pragma unroll
        for (int i = 0; i < 6; ++i) hll[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) b[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) hll[i] = gsum<G>(hll[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) b[i] = gsum<G>(b[i]);
    double A[6], zt[3];
    chol3(hll, c.lambda, A);
    if (k > 0 && sub == 0) {   // the update pass of this trial takes the factor from here
        double2* dst = reinterpret_cast<double2*>(a.ainv + 6 * (size_t)g.at);
        dst[0] = double2{A[0], A[1]}; dst[1] = double2{A[2], A[3]}; dst[2] = double2{A[4], A[5]};
    }
    zt[0] = A[0] * b[0];
    zt[1] = A[1] * b[0] + A[2] * b[1];
    zt[2] = A[3] * b[0] + A[4] * b[1] + A[5] * b[2];
    const bool fr = c0 >= 0;
    // W_e = Hpl_e A^T, Hpl_e = W Jp^T Jl  (zero for a fixed pose)
    double Wm[18];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double h0 = fr ? W * (Jp[r] * Jl[0] + Jp[6 + r] * Jl[3]) : 0.0;
        const double h1 = fr ? W * (Jp[r] * Jl[1] + Jp[6 + r] * Jl[4]) : 0.0;
        const double h2 = fr ? W * (Jp[r] * Jl[2] + Jp[6 + r] * Jl[5]) : 0.0;
        Wm[r * 3 + 0] = h0 * A[0];
        Wm[r * 3 + 1] = h0 * A[1] + h1 * A[2];
        Wm[r * 3 + 2] = h0 * A[3] + h1 * A[4] + h2 * A[5];
    }
    if (fr) {
        // the pose's own block: Hpp_e - W_e W_e^T (lower triangle, 21 entries) and its right-hand side b_e - W_e zeta
        int ob[6];
        ob[0] = tri(c0, c0);
#pragma unroll
        for (int r = 1; r < 6; ++r) ob[r] = ob[r - 1] + c0 + r;
        const int nrow = tri(c.n, 0) + c0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int m = 0; m <= r; ++m) {
                const double hpp = W * (Jp[r] * Jp[m] + Jp[6 + r] * Jp[6 + m]);
                const double ww = Wm[r * 3] * Wm[m * 3] + Wm[r * 3 + 1] * Wm[m * 3 + 1] + Wm[r * 3 + 2] * Wm[m * 3 + 2];
                lds_add(c.S + ob[r] + m, hpp - ww);
            }
            const double bpe = Jp[r] * o0 + Jp[6 + r] * o1;
            lds_add(c.S + nrow + r, bpe - (Wm[r * 3] * zt[0] + Wm[r * 3 + 1] * zt[1] + Wm[r * 3 + 2] * zt[2]));
        }
    }
    // the pair products: every lane puts W_e and its column into the wave's strip, lane i then takes the partners (i + s) mod k,
    // s = 1 .. k / 2 (the pairs at distance k / 2 of an even k only from the lower half) - as the SE(2) kernel
    double* mine = c.stage + lane * kStage3;
#pragma unroll
    for (int i = 0; i < 18; ++i) mine[i] = Wm[i];
    mine[18] = (double)c0;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const int half = k >> 1;
    int smax = half;
#pragma unroll
    for (int m = G; m < 64; m <<= 1) smax = max(smax, __shfl_xor(smax, m));
    const int gbase = lane & ~(G - 1);
    for (int s = 1; s <= smax; ++s) {
        const bool act = has && s <= half && !(2 * s == k && sub >= half);
        int j = sub + s;
        if (j >= k) j -= k;
        const double* his = c.stage + (gbase + (act ? j : sub)) * kStage3;
        const int cp = (int)his[18];
        if (act && fr && cp >= 0) {
            // block (mine, his) of S loses W_mine W_his^T, stored where row > column (two observations of one landmark by the same
            // key frame land in the pose's own block: P + P^T, lower triangle)
            const bool lower = c0 > cp, same = c0 == cp;
            const int hi = lower ? c0 : cp, lo = lower ? cp : c0;
            int rb[6];
            rb[0] = tri(hi, lo);
#pragma unroll
            for (int r = 1; r < 6; ++r) rb[r] = rb[r - 1] + hi + r;
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                const double p0 = his[m * 3], p1 = his[m * 3 + 1], p2 = his[m * 3 + 2];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    double pr = Wm[r * 3] * p0 + Wm[r * 3 + 1] * p1 + Wm[r * 3 + 2] * p2;
                    int at = rb[r] + m;
                    if (r > m) at = (lower || same) ? rb[r] + m : rb[m] + r;
                    if (r < m) at = lower ? rb[r] + m : rb[m] + r;
                    if (r == m && same) pr *= 2.0;
                    lds_add(c.S + at, -pr);
                }
            }
        }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();   // (the next landmark's strip writes stay behind these reads)
    asm volatile("" ::: "memory");
}

template <int G, int NT>
__device__ __forceinline__ void build_class(const Ctx3& c, int begin, int end) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (begin >= end) return;
    constexpr int kStep = NT / G;
    Group3 nx = load_group<G>(c, load_desc(c, begin + tid / G, end), lane, begin + tid / G);
    int4 d2 = load_desc(c, begin + kStep + tid / G, end);
    for (int i0 = begin; i0 < end; i0 += kStep) {
        const Group3 g = nx;
        nx = load_group<G>(c, d2, lane, i0 + kStep + tid / G);
        d2 = load_desc(c, i0 + 2 * kStep + tid / G, end);
        build_group<G>(c, g, lane);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// the pose terms, one thread each: t < P the prior of pose t (EdgeSE3ExpmapPrior), t >= P odometry edge t - P (EdgeSE3Expmap)
// ------------------------------------------------------------------------------------------------------------------
enum { kTermEval = 0, kTermDiag = 1, kTermBuild = 2, kTermUpdate = 3 };

// e = log(M T^-1), Jacobian -I: H += Omega, b += Omega e (k3_terms); chi^2 e^T Omega e for every pose with a prior (k3_finalize)
template <int MODE>
__device__ __forceinline__ void prior_term(const Ctx3& c, int p, double& chi, double& scale) {
    const Window3Args& a = *c.a;
    if (!a.prior_has[p]) return;
    const double* W = a.prior_info + 36 * (size_t)p;
    const Se3 M = se3_load(a.prior_meas + 12 * (size_t)p);
    double e[6];
    if (MODE == kTermEval || MODE == kTermUpdate) {   // at the estimate / at the trial state
        se3_log(se3_mul(M, se3_inv(se3_load((MODE == kTermEval ? c.cur : c.trl) + 12 * p))), e);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) v += W[6 * r + q] * e[q];
            chi += e[r] * v;
        }
        if (MODE == kTermEval) return;
    }
    const int cp = c.col[p];
    if (cp < 0) return;
    if (MODE == kTermDiag) {
#pragma unroll
        for (int r = 0; r < 6; ++r) lds_add(c.x + cp + r, W[7 * r]);
        return;
    }
    se3_log(se3_mul(M, se3_inv(se3_load(c.cur + 12 * p))), e);
    double g[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        g[r] = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) g[r] += W[6 * r + q] * e[q];
    }
    if (MODE == kTermUpdate) {   // dp . b_p: the prior's share
#pragma unroll
        for (int r = 0; r < 6; ++r) scale += c.x[cp + r] * g[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int q = 0; q <= r; ++q) lds_add(c.S + tri(cp + r, cp + q), W[6 * r + q]);
        lds_add(c.S + tri(c.n, cp + r), g[r]);
    }
}

// e = log(T_j^-1 C T_i), J_i = adj(T_j^-1 C), J_j = -adj(T_i^-1 C^-1): Oii, Ojj, Oij, obi, obj as k3_terms computes them
template <int MODE>
__device__ __forceinline__ void odometry_term(const Ctx3& c, int k, double& chi, double& scale) {
    const Window3Args& a = *c.a;
    const int i = a.o_i[k], j = a.o_j[k];
    const double* W = a.o_info + 36 * (size_t)k;
    const Se3 C = se3_load(a.o_meas + 12 * (size_t)k);
    double e[6];
    if (MODE == kTermEval || MODE == kTermUpdate) {   // chi^2 at the estimate / at the trial state (k3_finalize)
        const double* ps = MODE == kTermEval ? c.cur : c.trl;
        se3_log(se3_mul(se3_mul(se3_inv(se3_load(ps + 12 * j)), C), se3_load(ps + 12 * i)), e);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) v += W[6 * r + q] * e[q];
            chi += e[r] * v;
        }
        if (MODE == kTermEval) return;
    }
    const int ci = c.col[i], cj = c.col[j];
    if (ci < 0 && cj < 0) return;
    const Se3 Ti = se3_load(c.cur + 12 * i), Tj = se3_load(c.cur + 12 * j);
    const Se3 TjC = se3_mul(se3_inv(Tj), C);
    double Ji[36], Jj[36], We[6];
    se3_log(se3_mul(TjC, Ti), e);
    se3_adj(TjC, Ji);
    se3_adj(se3_mul(se3_inv(Ti), se3_inv(C)), Jj);
#pragma unroll
    for (int q = 0; q < 36; ++q) Jj[q] = -Jj[q];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        We[r] = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) We[r] += W[6 * r + q] * e[q];
    }
    if (MODE != kTermDiag) {   // obi = -J_i^T Omega e, obj = -J_j^T Omega e
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double bi = 0, bj = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) { bi += Ji[6 * q + r] * We[q]; bj += Jj[6 * q + r] * We[q]; }
            if (MODE == kTermUpdate) {
                if (ci >= 0) scale += c.x[ci + r] * -bi;
                if (cj >= 0) scale += c.x[cj + r] * -bj;
            } else {
                if (ci >= 0) lds_add(c.S + tri(c.n, ci + r), -bi);
                if (cj >= 0) lds_add(c.S + tri(c.n, cj + r), -bj);
            }
        }
        if (MODE == kTermUpdate) return;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {   // column q of Oii = J_i^T Omega J_i, Ojj, Oij = J_i^T Omega J_j
        double wi[6], wj[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            wi[m] = 0; wj[m] = 0;
#pragma unroll
            for (int t = 0; t < 6; ++t) { wi[m] += W[6 * m + t] * Ji[6 * t + q]; wj[m] += W[6 * m + t] * Jj[6 * t + q]; }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (MODE == kTermDiag && r != q) continue;
            double ii = 0, jj = 0, ij = 0;
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                ii += Ji[6 * m + r] * wi[m];
                jj += Jj[6 * m + r] * wj[m];
                ij += Ji[6 * m + r] * wj[m];
            }
            if (MODE == kTermDiag) {
                if (ci >= 0) lds_add(c.x + ci + r, ii);
                if (cj >= 0) lds_add(c.x + cj + r, jj);
                continue;
            }
            if (ci >= 0 && q <= r) lds_add(c.S + tri(ci + r, ci + q), ii);
            if (cj >= 0 && q <= r) lds_add(c.S + tri(cj + r, cj + q), jj);
            if (ci >= 0 && cj >= 0) lds_add(c.S + (ci > cj ? tri(ci + r, cj + q) : tri(cj + q, ci + r)), ij);   // H(i r, j q)
        }
    }
}

template <int MODE, int NT>
__device__ __forceinline__ void pose_terms(const Ctx3& c, double& chi, double& scale) {
    const Window3Args& a = *c.a;
    for (int t = threadIdx.x; t < a.P + a.O; t += NT) {
        if (t < a.P) prior_term<MODE>(c, t, chi, scale);
        else odometry_term<MODE>(c, t - a.P, chi, scale);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// LL^T of the augmented system in place (left-looking, 6 x 6 blocks, the right-hand side as block row nf): the SE(2) kernel's
// factor_column with 6 x 6 blocks.  T(I, J) = S(I, J) - sum_{K < J} L(I, K) L(J, K)^T, LPB lanes sharing the sum over K; every
// block's first lane factorises T(J, J) (from the strip tjj, 21 words) for itself and solves L(I, J) = T(I, J) L(J, J)^-T.
// ------------------------------------------------------------------------------------------------------------------
template <int NT, int LPB>
__device__ __forceinline__ void factor_column6(double* S, double* invd, double* tjj, int nf, int J, int* fail) {
    const int tid = threadIdx.x, sub = tid & (LPB - 1), grp = tid / LPB;
    for (int I0 = J; I0 <= nf; I0 += NT / LPB) {
        const int I = I0 + grp;
        const bool live = I <= nf;
        const int Ic = live ? I : J;
        double acc[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) acc[i] = 0.0;
        for (int K = sub; K < J; K += LPB) {
            double lj[36];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const double* rj = S + tri(6 * J + q, 6 * K);
#pragma unroll
                for (int m = 0; m < 6; ++m) lj[q * 6 + m] = rj[m];
            }
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double* ri = S + tri(6 * Ic + r, 6 * K);
                double li[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) li[m] = ri[m];
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    acc[r * 6 + q] += li[0] * lj[q * 6] + li[1] * lj[q * 6 + 1] + li[2] * lj[q * 6 + 2] + li[3] * lj[q * 6 + 3] +
                                      li[4] * lj[q * 6 + 4] + li[5] * lj[q * 6 + 5];
            }
        }
        double t[36];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double* ri = S + tri(6 * Ic + r, 6 * J);
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const double s = gsum<LPB>(acc[r * 6 + q]);
                t[r * 6 + q] = (Ic > J || q <= r) ? ri[q] - s : 0.0;
            }
        }
        if (sub == 0 && live && I == J) {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int q = 0; q <= r; ++q) tjj[tri(r, q)] = t[r * 6 + q];
        }
        __syncthreads();
        if (sub == 0 && live) {
            double l[21], iv[6];
            bool bad = false;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                double d = tjj[tri(q, q)];
#pragma unroll
                for (int m = 0; m < q; ++m) d -= l[tri(q, m)] * l[tri(q, m)];
                bad |= !(d > 0.0);
                iv[q] = fast_rsqrt(d > 0.0 ? d : 1.0);
                l[tri(q, q)] = d * iv[q];
#pragma unroll
                for (int r = q + 1; r < 6; ++r) {
                    double v = tjj[tri(r, q)];
#pragma unroll
                    for (int m = 0; m < q; ++m) v -= l[tri(r, m)] * l[tri(q, m)];
                    l[tri(r, q)] = v * iv[q];
                }
            }
            if (I == J) {
                if (bad) *fail = 1;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int q = 0; q <= r; ++q) S[tri(6 * J + r, 6 * J + q)] = l[tri(r, q)];
#pragma unroll
                for (int q = 0; q < 6; ++q) invd[6 * J + q] = iv[q];
            } else {
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    double* o = S + tri(6 * I + r, 6 * J);
                    double xr[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        double v = t[r * 6 + q];
#pragma unroll
                        for (int m = 0; m < q; ++m) v -= xr[m] * l[tri(q, m)];
                        xr[q] = v * iv[q];
                        o[q] = xr[q];
                    }
                }
            }
        }
        __syncthreads();
    }
}
template <int NT>
__device__ __forceinline__ void factorize6(double* S, double* invd, double* tjj, int nf, int* fail) {
    for (int J = 0; J < nf; ++J) {
        const int blocks = nf - J + 1;
        if (blocks * 64 <= NT) factor_column6<NT, 64>(S, invd, tjj, nf, J, fail);
        else if (blocks * 32 <= NT) factor_column6<NT, 32>(S, invd, tjj, nf, J, fail);
        else if (blocks * 16 <= NT) factor_column6<NT, 16>(S, invd, tjj, nf, J, fail);
        else factor_column6<NT, 8>(S, invd, tjj, nf, J, fail);
    }
}

// x = L^-T y by ONE wave: y (row n of the factor) in registers, three unknowns per lane (n <= 192), a pose block per step from the
// last to the first: its six unknowns by scalar broadcasts and its own triangle, then its six rows of L update every earlier y
__device__ __forceinline__ void back_substitute6(const double* S, const double* invd, int nf, double* x) {
    const int lane = threadIdx.x & 63;
    const int n = 6 * nf;
    double y[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int i = lane + 64 * s;
        y[s] = i < n ? S[tri(n, i)] : 0.0;
    }
    for (int J = nf - 1; J >= 0; --J) {
        double rw[6][3], d[21], iv[6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int i = lane + 64 * s;
                rw[r][s] = i < 6 * J ? S[tri(6 * J + r, i)] : 0.0;
            }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q <= r; ++q) d[tri(r, q)] = S[tri(6 * J + r, 6 * J + q)];
#pragma unroll
        for (int q = 0; q < 6; ++q) iv[q] = invd[6 * J + q];
        double yb[6], xb[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int j = 6 * J + r;
            const double ys = j >= 128 ? y[2] : (j >= 64 ? y[1] : y[0]);
            yb[r] = lane_value(ys, j & 63);
        }
#pragma unroll
        for (int q = 5; q >= 0; --q) {
            double v = yb[q];
#pragma unroll
            for (int m = q + 1; m < 6; ++m) v -= d[tri(m, q)] * xb[m];
            xb[q] = v * iv[q];
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) x[6 * J + q] = xb[q];
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)
            y[s] -= rw[0][s] * xb[0] + rw[1][s] * xb[1] + rw[2][s] * xb[2] + rw[3][s] * xb[3] + rw[4][s] * xb[4] + rw[5][s] * xb[5];
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_window_lm3(const Window3Args* __restrict__ all) {
    const Window3Args& a = all[blockIdx.x];
    extern __shared__ double lds[];
    __shared__ BaCtl ctl;
    __shared__ int s_nf, s_fail, s_err, s_stop;
    __shared__ int hist[kWindowMaxDegree + 2], wtot[18][8], rstart[18];
    __shared__ double red[24], tjj[21];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int P = a.P, L = a.L;
    if (a.stamps && tid == 0) a.stamps[5] = wall_clock64();

    // ---- prologue: the controller block (k_ctl_init's rules), columns of the free poses, the landmarks ordered by their counts
    if (tid == 0) {
        const BaCtl* g = a.ctl;
        const int sel = g->sel;
        const double seq = g->seq;
        const unsigned epoch = g->epoch;
        double* w = reinterpret_cast<double*>(&ctl);
        for (int i = 0; i < (int)(sizeof(BaCtl) / 8); ++i) w[i] = 0.0;
        ctl.ni = 2;
        ctl.sel = sel;
        ctl.iters = a.iters;
        ctl.mode = a.mode;
        ctl.seq = seq;
        ctl.epoch = epoch;
        s_fail = 0; s_err = 0;
        s_stop = (a.stop && *(const volatile int*)a.stop) ? 1 : 0;
    }
    for (int i = tid; i < kWindowMaxDegree + 2; i += NT) hist[i] = 0;
    // LDS map (doubles): col P ints | cur 12P | trl 12P | x n | invd n | stage NT x kStage3 | S (n+6)(n+7)/2
    int* col = reinterpret_cast<int*>(lds);
    double* bufA = lds + (P + 1) / 2;
    double* bufB = bufA + 12 * P;
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int p = 0; p < P; ++p) col[p] = a.fixed[p] ? -1 : 6 * cnt++;
        s_nf = cnt;
    }
    {
        const double* src = ctl.sel ? a.poses_b : a.poses_a;
        for (int i = tid; i < 12 * P; i += NT) bufA[i] = src[i];
    }
    for (int l = tid; l < L; l += NT) {
        const int k = a.lm_ptr[l + 1] - a.lm_ptr[l];
        if (k > kWindowMaxDegree) s_err = 2;
        else atomicAdd(&hist[k], 1);
    }
    __syncthreads();
    if (tid == 0) {   // hist[k] -> first position of the landmarks with k observations, rstart[k] -> their first record
        int at = 0, rat = 0;
        for (int k = 0; k <= kWindowMaxDegree + 1; ++k) {
            const int h = hist[k];
            hist[k] = at;
            if (k < 18) rstart[k] = rat;
            at += h;
            rat += h * k;
        }
    }
    __syncthreads();
    const bool refused = s_err != 0;
    if (!refused) {   // the list (the SE(2) kernel's prologue): by count 0 .. 16, more; stable inside a count
        constexpr int kBuckets = 18;
        int next[kBuckets];
#pragma unroll
        for (int b = 0; b < kBuckets; ++b) next[b] = hist[b];
        const int lane = tid & 63;
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        for (int l0 = 0; l0 < L; l0 += NT) {
            const int l = l0 + tid;
            int beg = 0, k = 0, cls = -1;
            if (l < L) {
                beg = a.lm_ptr[l];
                k = a.lm_ptr[l + 1] - beg;
                cls = min(k, kBuckets - 1);
            }
            int rank = 0;
#pragma unroll
            for (int b = 0; b < kBuckets; ++b) {
                const unsigned long long m = __ballot(cls == b);
                if (cls == b) rank = __popcll(m & below);
                if (lane == 0) wtot[b][wave] = __popcll(m);
            }
            __syncthreads();
            if (cls >= 0) {
                int at = rank;
#pragma unroll
                for (int b = 0; b < kBuckets; ++b)
                    if (cls == b) at += next[b];
                for (int w = 0; w < wave; ++w) at += wtot[cls][w];
                a.desc[at] = make_int4(l, cls < kBuckets - 1 ? rstart[cls] + (at - hist[cls]) * k : beg, k, beg);
            }
#pragma unroll
            for (int b = 0; b < kBuckets; ++b)
                for (int w = 0; w < NT / 64; ++w) next[b] += wtot[b][w];
            __syncthreads();
        }
    }
    if (a.stamps && tid == 0) a.stamps[6] = wall_clock64();
    const int nf = s_nf, n = 6 * nf;
    double* xs = bufB + 12 * P;
    double* invd = xs + n;
    double* stage_all = invd + n;
    double* S = stage_all + (size_t)NT * kStage3;
    const int ntri = (n + 6) * (n + 7) / 2;   // rows 0 .. n-1 = S, row n = b_s, five rows of zeros (the last block row)
    if (refused && tid == 0) { ctl.error = 2; ctl.done = 1; }
    __syncthreads();
    const int b1 = hist[1], b5 = hist[5], b9 = hist[9], b17 = hist[17];

    Ctx3 c;
    c.a = &a;
    c.S = S;
    c.x = xs;
    c.cur = bufA; c.trl = bufB;
    c.col = col;
    c.stage = stage_all + (size_t)wave * 64 * kStage3;
    c.lms = ctl.sel ? a.lms_b : a.lms_a;
    c.lms_trial = ctl.sel ? a.lms_a : a.lms_b;
    c.desc = a.desc;
    {   // the record arrays lie behind the list: 16 + 8 + 4 bytes per observation (the caller has checked the room: ba_resident_ok)
        const size_t E = (size_t)a.E;
        c.r_uv = reinterpret_cast<const double2*>(a.desc + L);
        c.r_w = reinterpret_cast<const double*>(c.r_uv + E);
        c.r_kf = reinterpret_cast<const int*>(c.r_w + E);
    }
    c.n = n;
    c.lambda = 0.0;
    double* cur = bufA;
    double* trl = bufB;

    // ---- the opening pass: chi^2 of the starting state (projection edges, priors, odometry), for LM the diagonal of the first
    // linearisation (lambda_0 = 1e-5 max diag H), and the observations into the order of the list
    if (!refused) {
        const bool lm = a.mode == SE2GPU_BA_LM;
        for (int i = tid; i < n; i += NT) xs[i] = 0.0;
        __syncthreads();
        double chi = 0, sc = 0, dm = 0;
        if (lm) {
            eval_class<kDiag, 4, NT, true>(c, b1, b5, chi, sc, dm);
            eval_class<kDiag, 8, NT, true>(c, b5, b9, chi, sc, dm);
            eval_class<kDiag, 16, NT, true>(c, b9, b17, chi, sc, dm);
            eval_class<kDiag, 64, NT, true>(c, b17, L, chi, sc, dm);
            pose_terms<kTermEval, NT>(c, chi, sc);
            pose_terms<kTermDiag, NT>(c, chi, sc);
        } else {
            eval_class<kEval, 4, NT, true>(c, b1, b5, chi, sc, dm);
            eval_class<kEval, 8, NT, true>(c, b5, b9, chi, sc, dm);
            eval_class<kEval, 16, NT, true>(c, b9, b17, chi, sc, dm);
            eval_class<kEval, 64, NT, true>(c, b17, L, chi, sc, dm);
            pose_terms<kTermEval, NT>(c, chi, sc);
        }
        __syncthreads();
        if (lm)
            for (int i = tid; i < n; i += NT) dm = fmax(dm, fabs(xs[i]));
        wg_reduce<NT>(red, chi, sc, dm);
        if (tid == 0) {
            ctl.current_chi = ctl.chi2_init = ctl.chi2_final = chi;
            if (s_stop) { ctl.stopped = 1; ctl.done = 1; }
            if (ctl.iters <= 0) ctl.done = 1;
            if (lm && !ctl.done) { ctl.lambda = 1e-5 * dm; ctl.ni = 2; }
        }
        __syncthreads();
    }
    long long* stamps = a.stamps;
    if (stamps && tid == 0) stamps[7] = wall_clock64();
    // ---- the trials
    while (!ctl.done) {
        const double lambda = ctl.lambda;
        c.lambda = lambda;
        if (stamps && tid == 0) stamps[0] = wall_clock64();
        for (int i = tid; i < ntri; i += NT) S[i] = 0.0;
        if (tid == 0) s_fail = 0;
        __syncthreads();
        {
            double chi = 0, sc = 0;
            build_class<4, NT>(c, b1, b5);
            build_class<8, NT>(c, b5, b9);
            build_class<16, NT>(c, b9, b17);
            build_class<64, NT>(c, b17, L);
            pose_terms<kTermBuild, NT>(c, chi, sc);
        }
        __syncthreads();
        for (int i = tid; i < n; i += NT) S[tri(i, i)] += lambda;
        __syncthreads();
        if (stamps && tid == 0) stamps[1] = wall_clock64();
        factorize6<NT>(S, invd, tjj, nf, &s_fail);
        if (stamps && tid == 0) stamps[2] = wall_clock64();
        if (wave == 0) back_substitute6(S, invd, nf, xs);
        __syncthreads();
        if (stamps && tid == 0) stamps[3] = wall_clock64();
        // ---- oplus into the trial state (VertexSE3Expmap::oplusImpl: exp(dx) T; fixed poses copied)
        double chi = 0, sc = 0, dm = 0;
        for (int p = tid; p < P; p += NT) {
            Se3 T = se3_load(cur + 12 * p);
            const int cp = col[p];
            if (cp >= 0) {
                double u[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    u[r] = xs[cp + r];
                    sc += lambda * (u[r] * u[r]);
                }
                T = se3_mul(se3_exp(u), T);
            }
            se3_store(T, trl + 12 * p);
        }
        __syncthreads();
        copy_unobserved<NT>(c, b1);
        eval_class<kUpdate, 4, NT>(c, b1, b5, chi, sc, dm);
        eval_class<kUpdate, 8, NT>(c, b5, b9, chi, sc, dm);
        eval_class<kUpdate, 16, NT>(c, b9, b17, chi, sc, dm);
        eval_class<kUpdate, 64, NT>(c, b17, L, chi, sc, dm);
        pose_terms<kTermUpdate, NT>(c, chi, sc);
        wg_reduce<NT>(red, chi, sc, dm);
        if (stamps && tid == 0) stamps[4] = wall_clock64();
        if (tid == 0) {
            const int stopped = (a.stop && *(const volatile int*)a.stop) ? 1 : 0;
            const int sel_before = ctl.sel;
            const double v[3] = {chi, sc, s_fail ? 1.0 : 0.0};
            lm_advance(&ctl, v, stopped != 0);
            s_stop = ctl.sel != sel_before;     // (re-used: the trial state became the estimate)
        }
        __syncthreads();
        if (s_stop) {
            double* t = cur; cur = trl; trl = t;
            c.cur = cur; c.trl = trl;
            const double* tl = c.lms; c.lms = c.lms_trial; c.lms_trial = const_cast<double*>(tl);
        }
        __syncthreads();
    }

    // ---- epilogue: the estimate's poses to the buffer the controller names, the block to the handle and its mailbox
    if (!refused) {
        double* dst = ctl.sel ? a.poses_b : a.poses_a;
        for (int i = tid; i < 12 * P; i += NT) dst[i] = cur[i];
    }
    __syncthreads();
    if (tid == 0) ctl.seq += 1.0;
    __syncthreads();
    {
        constexpr int kWords = (int)(sizeof(BaCtl) / 8);
        const double* src = reinterpret_cast<const double*>(&ctl);
        double* gdst = reinterpret_cast<double*>(a.ctl);
        for (int i = tid; i < kWords; i += NT) gdst[i] = src[i];
        if (a.mail) {
            volatile double* mail = a.mail;
            for (int i = tid; i < kWords; i += NT) mail[8 + i] = src[i];
            __threadfence_system();
            __syncthreads();
            if (tid == 0) mail[kMailSeq] = ctl.seq;
        }
    }
}

}  // namespace

namespace se2gpu {

// LDS of an SE3 window: (P + 1) / 2 + 24 P + 2 n + 19 threads + (n + 6)(n + 7) / 2 doubles, n = 6 nfree, and the static part.
// 256 or 128 threads, never 512: at 512 a lane has 256 registers, and the pose terms (6 x 6 adjoints and information) of this kernel
// spill to scratch there, where the wider widths keep everything in registers (VGPRs + AGPRs).  With P = nfree + 1 the largest window
// that fits 160 KiB has 27 free key frames at 256 threads and 29 at 128 (26 / 29 next to 6 fixed reference key frames).
size_t ba_window3_lds_bytes(int P, int nfree, int threads) {
    if (threads != 256 && threads != 128) return 0;
    const size_t n = 6 * (size_t)nfree;
    const size_t doubles = (size_t)(P + 1) / 2 + 24 * (size_t)P + 2 * n + (size_t)threads * kStage3 + (n + 6) * (n + 7) / 2;
    const size_t bytes = doubles * 8;
    // static LDS of the kernel: the controller block, the counts and their lists, the reduction scratch, the T(J, J) strip
    const size_t fixed = sizeof(BaCtl) + (kWindowMaxDegree + 2 + 18 * 8 + 18 + 4) * sizeof(int) + (24 + 21) * 8 + 128;
    if (n > 192 || bytes + fixed > 160 * 1024) return 0;
    return bytes;
}

template <int NT>
static int launch3_nt(const Window3Args* d_args, int count, size_t lds_bytes, hipStream_t st) {
    static size_t allowed = 0;   // (grown under the caller's lock: se2gpu_ba_optimize_batch serialises its resident launches)
    if (lds_bytes > allowed) {
        SE2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_window_lm3<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        allowed = lds_bytes;
    }
    hipLaunchKernelGGL(k_window_lm3<NT>, dim3(count), dim3(NT), lds_bytes, st, d_args);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

int ba_window3_launch(const Window3Args* d_args, int count, int threads, size_t lds_bytes, hipStream_t st) {
    if (count <= 0) return SE2GPU_OK;
    if (threads == 256) return launch3_nt<256>(d_args, count, lds_bytes, st);
    if (threads == 128) return launch3_nt<128>(d_args, count, lds_bytes, st);
    set_error("SE3 window kernel: 128 or 256 threads");
    return SE2GPU_ERR_INVALID;
}

}  // namespace se2gpu
