// libse2gpu - SE(2)-XYZ local bundle adjustment, ONE WORKGROUP PER WINDOW (round 6).
//
// Replaces, per window of a batch, what LocalMapper::localBA runs on one g2o::SparseOptimizer:
//   /root/reference/src/LocalMapper.cpp:259-260      optimizer.initializeOptimization(0); optimizer.optimize(Config::LOCAL_ITER)
//   /root/reference/src/EdgeSE2XYZ.cpp:61-106         per-edge residual + 2x3 / 2x3 Jacobians
//   /root/reference/include/se2lam/EdgeSE2XYZ.h:62-102 PreEdgeSE2
//   [3P g2o 20160424]  Huber, Schur complement of the landmarks, dense pose solve, Levenberg policy (as the multi-launch path restates them)
//
// Why.  The multi-launch path (csrc/ba.hip) spreads ONE window over the chip: four launches per LM trial, per-edge records
// (W_e, Dg_e: 168 B) written by k_linearize and read back 2.2x over by k_reduce2, tile hand-offs of the dense solve through
// L2 - 15.6x the algorithmic bytes in HBM traffic, and a batch of 32-64 windows in lock step tops out at 110 k LM
// iterations/s.  A 50-key-frame window is small enough to LIVE in one compute unit: the lower triangle of the
// reduced system S (147 unknowns: 87 KB) fits the 160 KiB of LDS.  So here a workgroup owns a window for its whole
// optimize(iters): the poses, S, the right-hand sides and the solution never leave LDS, the LM controller runs in the
// workgroup, and nothing per edge and trial is written to memory.
//
// The kernel itself - the list of the landmarks, the passes OPEN / BUILD / SOLVE / UPDATE, the controller - is
// csrc/ba_window_skeleton.h, shared with the SE3-expmap model (csrc/ba_window3.hip).  This file is the SE(2)-XYZ model it is
// instantiated with: EdgeSE2XYZ and PreEdgeSE2, the 44-byte observation record (uv, w01, w2, key frame), the sine and cosine of the
// headings kept next to the poses in LDS, LL^T and the back-substitution on 3x3 blocks, and oplus with the normalised heading.
// Per LM trial a window reads its observations twice, writes and reads A once and writes its landmarks once.  Measured (PMC,
// tools/resident_pmc.sh): 4.6 MB per window and LM iteration = 2.8x the algorithmic 1.66 MB, where the multi-launch path moves 26 MB.
// Sums into S are atomic, hence in no fixed order: results agree with the multi-launch path and the oracle to
// rounding (1e-12 relative on the cost), not bit for bit - the parity bar of this path is north_star's 1e-5.
//
// A landmark with more than 64 observations is refused (BaCtl::error = 2: the caller runs the window on the multi-launch path).
#include <mutex>

#include "ba_window_skeleton.h"

namespace {

// EdgeSE2XYZ (EdgeSE2XYZ.cpp:61-106) with the pose's sine / cosine at hand
template <bool JAC>
__device__ __forceinline__ void edge_se2xyz(const CamDev& cam, double px, double py, double s, double c, double lx, double ly, double lz,
                                            double u, double v, double& e0, double& e1, double* Jp, double* Jl) {
    const double dx = lx - px, dy = ly - py;
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        R[i * 3 + 0] = cam.Rcb[i * 3 + 0] * c - cam.Rcb[i * 3 + 1] * s;
        R[i * 3 + 1] = cam.Rcb[i * 3 + 0] * s + cam.Rcb[i * 3 + 1] * c;
        R[i * 3 + 2] = cam.Rcb[i * 3 + 2];
    }
    const double X = R[0] * dx + R[1] * dy + R[2] * lz + cam.tcb[0];
    const double Y = R[3] * dx + R[4] * dy + R[5] * lz + cam.tcb[1];
    const double Z = R[6] * dx + R[7] * dy + R[8] * lz + cam.tcb[2];
    const double zi = fast_rcp(Z);
    e0 = cam.fx * X * zi + cam.cx - u;
    e1 = cam.fx * Y * zi + cam.cy - v;
    if (JAC) {
        const double zi2 = zi * zi;
        const double j00 = cam.fx * zi, j02 = -cam.fx * X * zi2, j12 = -cam.fx * Y * zi2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Jl[k] = j00 * R[k] + j02 * R[6 + k];
            Jl[3 + k] = j00 * R[3 + k] + j12 * R[6 + k];
        }
        Jp[0] = -Jl[0]; Jp[1] = -Jl[1]; Jp[2] = Jl[0] * dy - Jl[1] * dx;
        Jp[3] = -Jl[3]; Jp[4] = -Jl[4]; Jp[5] = Jl[3] * dy - Jl[4] * dx;
    }
}

struct Se2Model {
    using Args = WindowArgs;
    static constexpr int B = 3;        // a pose block: x, y, theta
    static constexpr int kPose = 3;
    static constexpr int kCache = 2;   // sin, cos of the heading
    static constexpr int kStaticInts = kWindowMaxDegree + 2 + 18 * 8;   // (the histogram and the wave totals; the rest is in the 128 bytes of slack)

    struct Edge {   // one observation as it comes from memory
        int kf;
        double u, v, w0, w1, w2;
    };
    __device__ __forceinline__ static Edge load_edge(const WindowArgs& a, int e) {
        Edge r;
        r.kf = a.e_kf[e];
        const double2 uv = reinterpret_cast<const double2*>(a.e_uv)[e];
        r.u = uv.x; r.v = uv.y;
        r.w0 = a.e_info[3 * (size_t)e]; r.w1 = a.e_info[3 * (size_t)e + 1]; r.w2 = a.e_info[3 * (size_t)e + 2];
        return r;
    }
    struct Records {   // 16 + 16 + 8 + 4 bytes per observation
        double2* uv;
        double2* w01;
        double* w2;
        int* kf;
    };
    __device__ __forceinline__ static Records records(int4* behind_list, size_t E) {
        Records r;
        r.uv = reinterpret_cast<double2*>(behind_list);
        r.w01 = r.uv + E;
        r.w2 = reinterpret_cast<double*>(r.w01 + E);
        r.kf = reinterpret_cast<int*>(r.w2 + E);
        return r;
    }
    __device__ __forceinline__ static void store_record(const Records& r, int e, const Edge& ed) {
        r.uv[e] = double2{ed.u, ed.v};
        r.w01[e] = double2{ed.w0, ed.w1};
        r.w2[e] = ed.w2;
        r.kf[e] = ed.kf;
    }
    __device__ __forceinline__ static Edge load_record(const Records& r, int e) {
        Edge ed;
        const double2 uv = r.uv[e], w01 = r.w01[e];
        ed.kf = r.kf[e];
        ed.u = uv.x; ed.v = uv.y;
        ed.w0 = w01.x; ed.w1 = w01.y; ed.w2 = r.w2[e];
        return ed;
    }

    __device__ __forceinline__ static void cache_pose(const double* pose, double* sc) { sincos(pose[2], &sc[0], &sc[1]); }

    // robust chi^2 of an observation of the landmark (lx, ly, lz) at the state (poses, sc)
    __device__ __forceinline__ static double edge_chi(const WindowArgs& a, const Edge& ed, const double* poses, const double* sc,
                                                      double lx, double ly, double lz) {
        const int kf = ed.kf;
        double e0, e1;
        edge_se2xyz<false>(a.cam, poses[3 * kf], poses[3 * kf + 1], sc[2 * kf], sc[2 * kf + 1], lx, ly, lz, ed.u, ed.v, e0, e1, nullptr, nullptr);
        double r0, r1;
        huber_w(e0 * (ed.w0 * e0 + ed.w1 * e1) + e1 * (ed.w1 * e0 + ed.w2 * e1), a.cam.huber, r0, r1);
        return r0;
    }

    // DIAG / UPDATE of one observation, up to the group's sums
    template <int MODE>
    __device__ __forceinline__ static void eval_front(const Ctx<Se2Model>& c, const GroupIn<Se2Model>& g, int c0, double (&acc)[12], double& chi, double& scale) {
        const WindowArgs& a = *c.a;
        const bool has = g.has;
        const int kf = g.ed.kf;
        const double w0 = g.ed.w0, w1 = g.ed.w1, w2 = g.ed.w2;
        const double px = c.cur[3 * kf], py = c.cur[3 * kf + 1], ps = c.cache_cur[2 * kf], pc = c.cache_cur[2 * kf + 1];
        double e0, e1;
        double Jp[6], Jl[6];
        edge_se2xyz<true>(a.cam, px, py, ps, pc, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, Jp, Jl);
        const double we0 = w0 * e0 + w1 * e1, we1 = w1 * e0 + w2 * e1;
        double r0, r1;
        huber_w(e0 * we0 + e1 * we1, a.cam.huber, r0, r1);
        if (MODE == kDiag && has) chi += r0;                       // (the lambda_0 pass is the chi^2 of the starting state as well)
        const double W0 = r1 * w0, W1 = r1 * w1, W2 = r1 * w2;    // weightedOmega
        const double or0 = -r1 * we0, or1 = -r1 * we1;            // omega_r
        double WJl[6];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            WJl[m] = W0 * Jl[m] + W1 * Jl[3 + m];
            WJl[3 + m] = W1 * Jl[m] + W2 * Jl[3 + m];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[i] = 0.0;
        if (MODE == kDiag) {
            acc[0] = Jl[0] * WJl[0] + Jl[3] * WJl[3];
            acc[3] = Jl[1] * WJl[1] + Jl[4] * WJl[4];
            acc[5] = Jl[2] * WJl[2] + Jl[5] * WJl[5];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[6 + r] = Jl[r] * or0 + Jl[3 + r] * or1;
        acc[9] = acc[10] = acc[11] = 0.0;
        if (c0 >= 0) {
            if (MODE == kDiag) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double wj0 = W0 * Jp[r] + W1 * Jp[3 + r], wj1 = W1 * Jp[r] + W2 * Jp[3 + r];
                    lds_add(c.x + c0 + r, Jp[r] * wj0 + Jp[3 + r] * wj1);
                }
            } else {
                const double d0 = c.x[c0], d1 = c.x[c0 + 1], d2 = c.x[c0 + 2];
                const double v0 = Jp[0] * d0 + Jp[1] * d1 + Jp[2] * d2, v1 = Jp[3] * d0 + Jp[4] * d1 + Jp[5] * d2;   // Jp dp
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[9 + m] = WJl[m] * v0 + WJl[3 + m] * v1;    // Hlp_e dp_e = Jl^T Omega' (Jp dp)
                scale += v0 * or0 + v1 * or1;                                              // dp . b_e, the edge's share of dp . b_p
            }
        }
    }

    // BUILD of one observation, up to the group's sums: what pose_block needs of it (Lin), its shares of Hll and bl
    struct Lin {
        double Jp[6], WJl[6];
        double W0, W1, W2;    // weightedOmega
        double or0, or1;      // omega_r
    };
    __device__ __forceinline__ static void linearize(const Ctx<Se2Model>& c, const GroupIn<Se2Model>& g, Lin& n, double (&hll)[6], double (&b)[3]) {
        const WindowArgs& a = *c.a;
        const int kf = g.ed.kf;
        const double w0 = g.ed.w0, w1 = g.ed.w1, w2 = g.ed.w2;
        const double px = c.cur[3 * kf], py = c.cur[3 * kf + 1], ps = c.cache_cur[2 * kf], pc = c.cache_cur[2 * kf + 1];
        double e0, e1, Jl[6];
        edge_se2xyz<true>(a.cam, px, py, ps, pc, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, n.Jp, Jl);
        const double we0 = w0 * e0 + w1 * e1, we1 = w1 * e0 + w2 * e1;
        double r0, r1;
        huber_w(e0 * we0 + e1 * we1, a.cam.huber, r0, r1);
        n.W0 = r1 * w0; n.W1 = r1 * w1; n.W2 = r1 * w2;
        n.or0 = -r1 * we0; n.or1 = -r1 * we1;
        const double* WJl = n.WJl;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            n.WJl[m] = n.W0 * Jl[m] + n.W1 * Jl[3 + m];
            n.WJl[3 + m] = n.W1 * Jl[m] + n.W2 * Jl[3 + m];
        }
        hll[0] = Jl[0] * WJl[0] + Jl[3] * WJl[3];
        hll[1] = Jl[0] * WJl[1] + Jl[3] * WJl[4];
        hll[2] = Jl[0] * WJl[2] + Jl[3] * WJl[5];
        hll[3] = Jl[1] * WJl[1] + Jl[4] * WJl[4];
        hll[4] = Jl[1] * WJl[2] + Jl[4] * WJl[5];
        hll[5] = Jl[2] * WJl[2] + Jl[5] * WJl[5];
#pragma unroll
        for (int r = 0; r < 3; ++r) b[r] = Jl[r] * n.or0 + Jl[3 + r] * n.or1;
    }
    // W_e = Hpl_e A^T, and the pose's own block of S with its right-hand side
    __device__ __forceinline__ static void pose_block(const Ctx<Se2Model>& c, const Lin& n, int c0, const double (&A)[6], const double (&zt)[3], double (&Wm)[9]) {
        const double *Jp = n.Jp, *WJl = n.WJl;
        const double W0 = n.W0, W1 = n.W1, W2 = n.W2, or0 = n.or0, or1 = n.or1;
        const bool fr = c0 >= 0;
        // W_e = Hpl_e A^T, Hpl_e = Jp^T (Omega' Jl)  (zero for a fixed pose: constructQuadraticForm skips it)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double h0 = fr ? Jp[r] * WJl[0] + Jp[3 + r] * WJl[3] : 0.0;
            const double h1 = fr ? Jp[r] * WJl[1] + Jp[3 + r] * WJl[4] : 0.0;
            const double h2 = fr ? Jp[r] * WJl[2] + Jp[3 + r] * WJl[5] : 0.0;
            Wm[r * 3 + 0] = h0 * A[0];
            Wm[r * 3 + 1] = h0 * A[1] + h1 * A[2];
            Wm[r * 3 + 2] = h0 * A[3] + h1 * A[4] + h2 * A[5];
        }
        if (fr) {
            double WJp[6];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                WJp[m] = W0 * Jp[m] + W1 * Jp[3 + m];
                WJp[3 + m] = W1 * Jp[m] + W2 * Jp[3 + m];
            }
            // the pose's own block: Hpp_e - W_e W_e^T (lower triangle) and its right-hand side b_e - W_e zeta
            int ob[3];   // the block's three rows at its first column: one multiplication, two additions
            ob[0] = tri(c0, c0); ob[1] = ob[0] + c0 + 1; ob[2] = ob[1] + c0 + 2;
            const int nrow = tri(c.n, 0) + c0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int m = 0; m <= r; ++m) {
                    const double hpp = Jp[r] * WJp[m] + Jp[3 + r] * WJp[3 + m];
                    const double ww = Wm[r * 3] * Wm[m * 3] + Wm[r * 3 + 1] * Wm[m * 3 + 1] + Wm[r * 3 + 2] * Wm[m * 3 + 2];
                    lds_add(c.S + ob[r] + m, hpp - ww);
                }
                const double bpe = Jp[r] * or0 + Jp[3 + r] * or1;
                lds_add(c.S + nrow + r, bpe - (Wm[r * 3] * zt[0] + Wm[r * 3 + 1] * zt[1] + Wm[r * 3 + 2] * zt[2]));
            }
        }
    }

    // PreEdgeSE2 (EdgeSE2XYZ.h:62-102), one thread per edge
    template <int MODE>
    __device__ __forceinline__ static void odometry_edge(const Ctx<Se2Model>& c, int k, double& chi, double& scale) {
        const WindowArgs& a = *c.a;
        const int i = a.o_i[k], j = a.o_j[k];
        const double* W = a.o_info + 9 * (size_t)k;
        double e[3], A[9], B[9];
        if (MODE == kUpdate) {   // the gain denominator's share at the estimate's linearisation, chi^2 at the trial state
            pre_se2(c.cur + 3 * i, c.cur + 3 * j, a.o_meas + 3 * (size_t)k, e, A, B);
            const int ci = c.col[i], cj = c.col[j];
            double omr[3];
            for (int r = 0; r < 3; ++r) omr[r] = -(W[r * 3] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2]);
            for (int r = 0; r < 3; ++r) {
                if (ci >= 0) scale += c.x[ci + r] * (A[r] * omr[0] + A[3 + r] * omr[1] + A[6 + r] * omr[2]);
                if (cj >= 0) scale += c.x[cj + r] * (B[r] * omr[0] + B[3 + r] * omr[1] + B[6 + r] * omr[2]);
            }
            pre_se2(c.trl + 3 * i, c.trl + 3 * j, a.o_meas + 3 * (size_t)k, e, A, B);
            for (int r = 0; r < 3; ++r) chi += e[r] * (W[r * 3] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2]);
            return;
        }
        pre_se2(c.cur + 3 * i, c.cur + 3 * j, a.o_meas + 3 * (size_t)k, e, A, B);
        if (MODE == kEval) {
            for (int r = 0; r < 3; ++r) chi += e[r] * (W[r * 3] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2]);
            return;
        }
        const int ci = c.col[i], cj = c.col[j];
        double omr[3], WA[9], WB[9];
        for (int r = 0; r < 3; ++r) {
            omr[r] = -(W[r * 3] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2]);
            for (int q = 0; q < 3; ++q) {
                WA[r * 3 + q] = W[r * 3] * A[q] + W[r * 3 + 1] * A[3 + q] + W[r * 3 + 2] * A[6 + q];
                WB[r * 3 + q] = W[r * 3] * B[q] + W[r * 3 + 1] * B[3 + q] + W[r * 3 + 2] * B[6 + q];
            }
        }
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) {
                const double aa = A[r] * WA[q] + A[3 + r] * WA[3 + q] + A[6 + r] * WA[6 + q];
                const double ab = A[r] * WB[q] + A[3 + r] * WB[3 + q] + A[6 + r] * WB[6 + q];
                const double bb = B[r] * WB[q] + B[3 + r] * WB[3 + q] + B[6 + r] * WB[6 + q];
                if (MODE == kDiag) {
                    if (q == r) {
                        if (ci >= 0) lds_add(c.x + ci + r, aa);
                        if (cj >= 0) lds_add(c.x + cj + r, bb);
                    }
                    continue;
                }
                if (ci >= 0 && q <= r) lds_add(c.S + tri(ci + r, ci + q), aa);
                if (cj >= 0 && q <= r) lds_add(c.S + tri(cj + r, cj + q), bb);
                if (ci >= 0 && cj >= 0) lds_add(c.S + (ci > cj ? tri(ci + r, cj + q) : tri(cj + q, ci + r)), ab);   // H(i r, j q)
            }
            if (MODE == kBuild) {
                if (ci >= 0) lds_add(c.S + tri(c.n, ci + r), A[r] * omr[0] + A[3 + r] * omr[1] + A[6 + r] * omr[2]);
                if (cj >= 0) lds_add(c.S + tri(c.n, cj + r), B[r] * omr[0] + B[3 + r] * omr[1] + B[6 + r] * omr[2]);
            }
        }
    }
    template <int MODE, int NT>
    __device__ __forceinline__ static void pose_terms(const Ctx<Se2Model>& c, double& chi, double& scale) {
        for (int k = threadIdx.x; k < c.a->O; k += NT) {
            if (MODE == kDiag) odometry_edge<kEval>(c, k, chi, scale);   // (the lambda_0 pass is the chi^2 of the starting state as well)
            odometry_edge<MODE>(c, k, chi, scale);
        }
    }

    // ------------------------------------------------------------------------------------------------------------------
    // LL^T of the augmented system in place (left-looking, 3x3 blocks, the right-hand side as row n): the off-diagonal blocks of L
    // overwrite S - the diagonal blocks too (over T(J, J), once everybody has it) - with the reciprocals of the diagonal in invd.  *fail is set
    // when a pivot is not positive (the step is then rejected, as g2o rejects a failed Cholesky).
    // Block column J: T(I, J) = S(I, J) - sum_{K < J} L(I, K) L(J, K)^T for the block rows I >= J, LPB lanes sharing a block's sum over
    // K (8 while the column is long, up to 64 near the end, where few rows are left and the sum is longest); then every block's first
    // lane factorises T(J, J) for itself (six multiplies: cheaper than a hand-off) and solves its own L(I, J) = T(I, J) L(J, J)^-T.
    // ------------------------------------------------------------------------------------------------------------------
    template <int NT, int LPB>
    __device__ __forceinline__ static void factor_column(double* S, double* invd, double* tjj, int nf, int J, int* fail) {
        const int tid = threadIdx.x, sub = tid & (LPB - 1), grp = tid / LPB;
        // (the right-hand side is block row nf: row n and two rows of zeros, so every block row is 3 x 3 and the loops unroll)
        for (int I0 = J; I0 <= nf; I0 += NT / LPB) {
            const int I = I0 + grp;
            const bool live = I <= nf;
            const int Ic = live ? I : J;
            const double* rowI[3] = {S + tri(3 * Ic, 0), S + tri(3 * Ic + 1, 0), S + tri(3 * Ic + 2, 0)};
            const double* rowJ[3] = {S + tri(3 * J, 0), S + tri(3 * J + 1, 0), S + tri(3 * J + 2, 0)};
            double t[9];   // S(I, J), requested before the sum it will be reduced by
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) t[r * 3 + q] = (sub == 0 && (Ic > J || q <= r)) ? rowI[r][3 * J + q] : 0.0;
            double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int K = sub; K < J; K += LPB) {
                double lj[9], li[9];
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int m = 0; m < 3; ++m) lj[q * 3 + m] = rowJ[q][3 * K + m];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int m = 0; m < 3; ++m) li[r * 3 + m] = rowI[r][3 * K + m];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc[r * 3 + q] += li[r * 3] * lj[q * 3] + li[r * 3 + 1] * lj[q * 3 + 1] + li[r * 3 + 2] * lj[q * 3 + 2];
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) t[i] -= gsum<LPB>(acc[i]);
            // T(J, J) goes to everybody through a six-word strip; the other blocks keep their T in registers across the barrier
            if (sub == 0 && live && I == J) { tjj[0] = t[0]; tjj[1] = t[3]; tjj[2] = t[4]; tjj[3] = t[6]; tjj[4] = t[7]; tjj[5] = t[8]; }
            __syncthreads();
            if (sub == 0 && live) {
                const double t00 = tjj[0], t10 = tjj[1], t11 = tjj[2], t20 = tjj[3], t21 = tjj[4], t22 = tjj[5];
                bool bad = !(t00 > 0.0);
                const double i00 = fast_rsqrt(bad ? 1.0 : t00), l00 = t00 * i00;
                const double l10 = t10 * i00, l20 = t20 * i00;
                const double d1 = t11 - l10 * l10;
                bad |= !(d1 > 0.0);
                const double i11 = fast_rsqrt(d1 > 0.0 ? d1 : 1.0), l11 = d1 * i11;
                const double l21 = (t21 - l20 * l10) * i11;
                const double d2 = t22 - l20 * l20 - l21 * l21;
                bad |= !(d2 > 0.0);
                const double i22 = fast_rsqrt(d2 > 0.0 ? d2 : 1.0), l22 = d2 * i22;
                if (I == J) {
                    if (bad) *fail = 1;
                    // L(J, J) over T(J, J) in place (everybody reads T(J, J) from the strip tjj, and no later column reads a diagonal block)
                    S[tri(3 * J, 3 * J)] = l00;
                    S[tri(3 * J + 1, 3 * J)] = l10; S[tri(3 * J + 1, 3 * J + 1)] = l11;
                    S[tri(3 * J + 2, 3 * J)] = l20; S[tri(3 * J + 2, 3 * J + 1)] = l21; S[tri(3 * J + 2, 3 * J + 2)] = l22;
                    invd[3 * J] = i00; invd[3 * J + 1] = i11; invd[3 * J + 2] = i22;
                } else {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        double* o = S + tri(3 * I + r, 3 * J);
                        const double x0 = t[r * 3] * i00;
                        const double x1 = (t[r * 3 + 1] - x0 * l10) * i11;
                        const double x2 = (t[r * 3 + 2] - x0 * l20 - x1 * l21) * i22;
                        o[0] = x0; o[1] = x1; o[2] = x2;
                    }
                }
            }
            __syncthreads();
        }
    }

    // x = L^-T y by ONE wave: y (row n of the factor) in registers, three unknowns per lane, a pose block per step from the last to the
    // first: the block's three unknowns by scalar broadcasts (readlane) and its own 3x3 triangle, then its three rows of L - requested a
    // step ahead - leave every earlier unknown's y.  n <= 192.
    __device__ __forceinline__ static void back_substitute(const double* S, const double* invd, int nf, double* x) {
        const int lane = threadIdx.x & 63;
        const int n = 3 * nf;
        double y[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int i = lane + 64 * s;
            y[s] = i < n ? S[tri(n, i)] : 0.0;
        }
        auto load_rows = [&](int J, double (&rw)[3][3], double (&d)[6], double (&iv)[3]) {
            if (J < 0) return;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int i = lane + 64 * s;
                    rw[r][s] = i < 3 * J ? S[tri(3 * J + r, i)] : 0.0;
                }
            d[0] = S[tri(3 * J, 3 * J)];
            d[1] = S[tri(3 * J + 1, 3 * J)]; d[2] = S[tri(3 * J + 1, 3 * J + 1)];
            d[3] = S[tri(3 * J + 2, 3 * J)]; d[4] = S[tri(3 * J + 2, 3 * J + 1)]; d[5] = S[tri(3 * J + 2, 3 * J + 2)];
#pragma unroll
            for (int i = 0; i < 3; ++i) iv[i] = invd[3 * J + i];
        };
        double rw[3][3], d[6], iv[3], nrw[3][3] = {}, nd[6] = {}, niv[3] = {};
        load_rows(nf - 1, rw, d, iv);
        for (int J = nf - 1; J >= 0; --J) {
            load_rows(J - 1, nrw, nd, niv);
            double yb[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int j = 3 * J + r;
                const double ys = j >= 128 ? y[2] : (j >= 64 ? y[1] : y[0]);
                yb[r] = lane_value(ys, j & 63);
            }
            const double x2 = yb[2] * iv[2];
            const double x1 = (yb[1] - d[4] * x2) * iv[1];
            const double x0 = (yb[0] - d[1] * x1 - d[3] * x2) * iv[0];
            if (lane == 0) { x[3 * J] = x0; x[3 * J + 1] = x1; x[3 * J + 2] = x2; }
#pragma unroll
            for (int s = 0; s < 3; ++s) y[s] -= rw[0][s] * x0 + rw[1][s] * x1 + rw[2][s] * x2;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) rw[r][s] = nrw[r][s];
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = nd[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) iv[i] = niv[i];
        }
    }

    // VertexSE2::oplusImpl: additive x, y; normalised heading (a fixed pose is copied)
    __device__ __forceinline__ static void oplus(const double* cur, int cp, const double* xs, double lambda, double* trl, double* sc, double& scale) {
        double px = cur[0], py = cur[1], th = cur[2];
        if (cp >= 0) {
            const double d0 = xs[cp], d1 = xs[cp + 1], d2 = xs[cp + 2];
            px += d0; py += d1; th = normalize_theta(th + d2);
            scale += lambda * (d0 * d0 + d1 * d1 + d2 * d2);           // the damping's share of x^T (lambda x + b)
        }
        trl[0] = px; trl[1] = py; trl[2] = th;
        sincos(th, &sc[0], &sc[1]);
    }
};

template <int NT>
__global__ __launch_bounds__(NT) void k_window_lm(const WindowArgs* __restrict__ all) {
    __shared__ WindowShared<3> sh;
    window_lm<Se2Model, NT>(all[blockIdx.x], sh);
}

// The same kernel behind a gather that decides on the device which windows run (csrc/local_ba_device.hip): a window whose status is
// not 0 returns before it reads anything else - its pack may name arrays the gather never filled.
template <int NT>
__global__ __launch_bounds__(NT) void k_window_lm_status(const WindowArgs* __restrict__ all, const int* __restrict__ status) {
    __shared__ WindowShared<3> sh;
    if (status[blockIdx.x] != 0) return;   // uniform
    window_lm<Se2Model, NT>(all[blockIdx.x], sh);
}

// (window_launch's counterpart for the two-argument kernel; the raise of the limit is serialised here, not by the caller)
template <int NT>
int window_launch_status(const WindowArgs* d_args, const int* d_status, int count, size_t lds_bytes, hipStream_t st) {
    static std::mutex mu;
    static size_t allowed = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (lds_bytes > allowed) {
            SE2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_window_lm_status<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds_bytes));
            allowed = lds_bytes;
        }
    }
    hipLaunchKernelGGL(k_window_lm_status<NT>, dim3(count), dim3(NT), lds_bytes, st, d_args, d_status);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // namespace

namespace se2gpu {

int ba_window_launch_status(const WindowArgs* d_args, const int* d_status, int count, int threads, size_t lds_bytes, hipStream_t st) {
    if (count <= 0) return SE2GPU_OK;
    if (threads == 512) return window_launch_status<512>(d_args, d_status, count, lds_bytes, st);
    if (threads == 256) return window_launch_status<256>(d_args, d_status, count, lds_bytes, st);
    if (threads == 128) return window_launch_status<128>(d_args, d_status, count, lds_bytes, st);
    set_error("window kernel: 128, 256 or 512 threads");
    return SE2GPU_ERR_INVALID;
}

size_t ba_window_lds_bytes(int P, int nfree, int threads) { return window_lds_bytes<Se2Model>(P, nfree, threads); }

int ba_window_launch(const WindowArgs* d_args, int count, int threads, size_t lds_bytes, hipStream_t st) {
    if (count <= 0) return SE2GPU_OK;
    if (threads == 512) return window_launch<&k_window_lm<512>, 512>(d_args, count, lds_bytes, st);
    if (threads == 256) return window_launch<&k_window_lm<256>, 256>(d_args, count, lds_bytes, st);
    if (threads == 128) return window_launch<&k_window_lm<128>, 128>(d_args, count, lds_bytes, st);
    set_error("window kernel: 128, 256 or 512 threads");
    return SE2GPU_ERR_INVALID;
}

}  // namespace se2gpu
