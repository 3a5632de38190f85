// libse2gpu - SE3-expmap local bundle adjustment, ONE WORKGROUP PER WINDOW.
//
// Replaces, per window of a batch, what the multi-launch k3_* kernels of csrc/ba.hip run for the library's second landmark model
// (pose model 1: Map::loadLocalGraph(opt, vpEdgesAll, vnAllIdx) + LocalMapper::removeOutlierChi2):
//   [3P g2o 20160424] VertexSE3Expmap, EdgeProjectXYZ2UV, EdgeSE3ExpmapPrior, EdgeSE3Expmap, SE3Quat - restated as in oracle/ba3_ref.cpp
// in the one-workgroup-per-window kernel of csrc/ba_window_skeleton.h, which it shares with the SE(2) model
// (csrc/ba_window.hip): a workgroup owns a window for its whole optimize(iters), the poses, the reduced system S and its solution
// never leave LDS, the LM controller runs in the workgroup.  This file is the model: the edge functions, the 28-byte observation
// record, the priors and odometry edges, LL^T and the back-substitution on 6 x 6 blocks, oplus.  With it the passes are
//   OPEN    the landmarks are listed by observation count and the observations copied into that order (28 B each: u v, w, key frame);
//           one pass gives chi^2 of the starting state (projection edges, priors, odometry) and, for LM, the diagonal for lambda_0
//           (k3_pose_diag + k_maxdiag: the landmarks' Hll and the free poses' un-reduced blocks)
//   BUILD   one lane per observation, 4 / 8 / 16 / 64 lanes per landmark: proj3<true>, Huber on w |e|^2, Hll / bl by DPP sums, the
//           factor A = G^-1 of Hll + lambda I, W_e = Hpl_e A^T (6 x 3, registers); Hpp_e - W_e W_e^T (21) and b_e - W_e zeta (6) go to
//           S by LDS atomics, the pair products W_i W_j^T (36 per pair, each pair once) through the per-wave strip; one lane per pose
//           adds its prior (Omega, Omega e) and one per odometry edge its blocks (Oii, Ojj, Oij, obi, obj as k6_terms<Expmap> computes them)
//   SOLVE   left-looking LL^T on 6 x 6 blocks in LDS with the right-hand side as an extra block row; x = L^-T y by one wave
//   UPDATE  the observations stream in again, the Jacobians are recomputed for the back-substitution x_l = A^T A (bl - q) (A from the
//           build pass through WindowArgsBase::ainv), exp(dx) T for the free poses (k6_oplus<Expmap>), robust chi^2 of the trial state
//           (projection edges, priors, odometry) and the gain denominator; lm_advance decides
// Sums into S are atomic, hence in no fixed order: results agree with the multi-launch path to rounding, not bit for bit.
//
// A landmark with more than 64 observations is refused (BaCtl::error = 2: the caller runs the window on the multi-launch path).
#include "ba_window_skeleton.h"
#include "se3_math.h"

namespace {

struct Se3Model {
    using Args = Window3Args;
    static constexpr int B = 6;        // a pose block: the se3 tangent
    static constexpr int kPose = 12;   // Tcw: R row-major, t
    static constexpr int kCache = 0;
    static constexpr int kStaticInts = kWindowMaxDegree + 2 + 18 * 8 + 18 + 4;   // (the histogram, the wave totals, the record starts, four flags)

    struct Edge {
        int kf;
        double u, v, w;
    };
    __device__ __forceinline__ static Edge load_edge(const Window3Args& a, int e) {
        Edge r;
        r.kf = a.e_kf[e];
        const double2 uv = reinterpret_cast<const double2*>(a.e_uv)[e];
        r.u = uv.x; r.v = uv.y;
        r.w = a.e_info[3 * (size_t)e];
        return r;
    }
    struct Records {   // 16 + 8 + 4 bytes per observation
        double2* uv;
        double* w;
        int* kf;
    };
    __device__ __forceinline__ static Records records(int4* behind_list, size_t E) {
        Records r;
        r.uv = reinterpret_cast<double2*>(behind_list);
        r.w = reinterpret_cast<double*>(r.uv + E);
        r.kf = reinterpret_cast<int*>(r.w + E);
        return r;
    }
    __device__ __forceinline__ static void store_record(const Records& r, int e, const Edge& ed) {
        r.uv[e] = double2{ed.u, ed.v};
        r.w[e] = ed.w;
        r.kf[e] = ed.kf;
    }
    __device__ __forceinline__ static Edge load_record(const Records& r, int e) {
        Edge ed;
        const double2 uv = r.uv[e];
        ed.kf = r.kf[e];
        ed.u = uv.x; ed.v = uv.y;
        ed.w = r.w[e];
        return ed;
    }

    // robust chi^2 of an observation of the landmark (lx, ly, lz) at the state `poses`
    __device__ __forceinline__ static double edge_chi(const Window3Args& a, const Edge& ed, const double* poses, const double*,
                                                      double lx, double ly, double lz) {
        double e0, e1;
        proj3<false>(a.cam, poses + 12 * ed.kf, lx, ly, lz, ed.u, ed.v, e0, e1, nullptr, nullptr);
        double r0, r1;
        huber_w(ed.w * (e0 * e0 + e1 * e1), a.cam.huber, r0, r1);
        return r0;
    }

    // DIAG / UPDATE of one observation up to the group's sums (EdgeProjectXYZ2UV: information w I, 2 x 6 pose Jacobian)
    template <int MODE>
    __device__ __forceinline__ static void eval_front(const Ctx<Se3Model>& c, const GroupIn<Se3Model>& g, int c0, double (&acc)[12], double& chi, double& scale) {
        const Window3Args& a = *c.a;
        const bool has = g.has;
        const double w = g.ed.w;
        const double* T = c.cur + 12 * g.ed.kf;
        double e0, e1;
        double Jp[12], Jl[6];
        proj3<true>(a.cam, T, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, Jp, Jl);
        double r0, r1;
        huber_w(w * (e0 * e0 + e1 * e1), a.cam.huber, r0, r1);
        if (MODE == kDiag && has) chi += r0;                       // (the lambda_0 pass is the chi^2 of the starting state as well)
        const double W = r1 * w, o0 = -W * e0, o1 = -W * e1;      // weighted information, omega_r
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
    }

    // BUILD of one observation up to the group's sums: what pose_block needs of it (Lin), its shares of Hll and bl
    struct Lin {
        double Jp[12], Jl[6];
        double W, o0, o1;   // weighted information, omega_r
    };
    __device__ __forceinline__ static void linearize(const Ctx<Se3Model>& c, const GroupIn<Se3Model>& g, Lin& n, double (&hll)[6], double (&b)[3]) {
        const Window3Args& a = *c.a;
        const double w = g.ed.w;
        double e0, e1;
        proj3<true>(a.cam, c.cur + 12 * g.ed.kf, g.lx, g.ly, g.lz, g.ed.u, g.ed.v, e0, e1, n.Jp, n.Jl);
        double r0, r1;
        huber_w(w * (e0 * e0 + e1 * e1), a.cam.huber, r0, r1);
        n.W = r1 * w; n.o0 = -n.W * e0; n.o1 = -n.W * e1;
        const double W = n.W;
        const double* Jl = n.Jl;
        hll[0] = W * (Jl[0] * Jl[0] + Jl[3] * Jl[3]);
        hll[1] = W * (Jl[0] * Jl[1] + Jl[3] * Jl[4]);
        hll[2] = W * (Jl[0] * Jl[2] + Jl[3] * Jl[5]);
        hll[3] = W * (Jl[1] * Jl[1] + Jl[4] * Jl[4]);
        hll[4] = W * (Jl[1] * Jl[2] + Jl[4] * Jl[5]);
        hll[5] = W * (Jl[2] * Jl[2] + Jl[5] * Jl[5]);
#pragma unroll
        for (int r = 0; r < 3; ++r) b[r] = Jl[r] * n.o0 + Jl[3 + r] * n.o1;
    }
    // W_e = Hpl_e A^T, and the pose's own block of S with its right-hand side
    __device__ __forceinline__ static void pose_block(const Ctx<Se3Model>& c, const Lin& n, int c0, const double (&A)[6], const double (&zt)[3], double (&Wm)[18]) {
        const double *Jp = n.Jp, *Jl = n.Jl;
        const double W = n.W, o0 = n.o0, o1 = n.o1;
        const bool fr = c0 >= 0;
        // W_e = Hpl_e A^T, Hpl_e = W Jp^T Jl  (zero for a fixed pose)
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
    }

    // ------------------------------------------------------------------------------------------------------------------
    // the pose terms, one thread each: t < P the prior of pose t (EdgeSE3ExpmapPrior), t >= P odometry edge t - P (EdgeSE3Expmap)
    // ------------------------------------------------------------------------------------------------------------------

    // e = log(M T^-1), Jacobian -I: H += Omega, b += Omega e (k6_terms<Expmap>); chi^2 e^T Omega e for every pose with a prior (k6_finalize<Expmap>)
    template <int MODE>
    __device__ __forceinline__ static void prior_term(const Ctx<Se3Model>& c, int p, double& chi, double& scale) {
        const Window3Args& a = *c.a;
        if (!a.prior_has[p]) return;
        const double* W = a.prior_info + 36 * (size_t)p;
        const Se3 M = se3_load(a.prior_meas + 12 * (size_t)p);
        double e[6];
        if (MODE == kEval || MODE == kUpdate) {   // at the estimate / at the trial state
            se3_log(se3_mul(M, se3_inv(se3_load((MODE == kEval ? c.cur : c.trl) + 12 * p))), e);
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double v = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) v += W[6 * r + q] * e[q];
                chi += e[r] * v;
            }
            if (MODE == kEval) return;
        }
        const int cp = c.col[p];
        if (cp < 0) return;
        if (MODE == kDiag) {
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
        if (MODE == kUpdate) {   // dp . b_p: the prior's share
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

    // e = log(T_j^-1 C T_i), J_i = adj(T_j^-1 C), J_j = -adj(T_i^-1 C^-1): Oii, Ojj, Oij, obi, obj as k6_terms<Expmap> computes them
    template <int MODE>
    __device__ __forceinline__ static void odometry_term(const Ctx<Se3Model>& c, int k, double& chi, double& scale) {
        const Window3Args& a = *c.a;
        const int i = a.o_i[k], j = a.o_j[k];
        const double* W = a.o_info + 36 * (size_t)k;
        const Se3 C = se3_load(a.o_meas + 12 * (size_t)k);
        double e[6];
        if (MODE == kEval || MODE == kUpdate) {   // chi^2 at the estimate / at the trial state (k6_finalize<Expmap>)
            const double* ps = MODE == kEval ? c.cur : c.trl;
            se3_log(se3_mul(se3_mul(se3_inv(se3_load(ps + 12 * j)), C), se3_load(ps + 12 * i)), e);
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double v = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) v += W[6 * r + q] * e[q];
                chi += e[r] * v;
            }
            if (MODE == kEval) return;
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
        if (MODE != kDiag) {   // obi = -J_i^T Omega e, obj = -J_j^T Omega e
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double bi = 0, bj = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { bi += Ji[6 * q + r] * We[q]; bj += Jj[6 * q + r] * We[q]; }
                if (MODE == kUpdate) {
                    if (ci >= 0) scale += c.x[ci + r] * -bi;
                    if (cj >= 0) scale += c.x[cj + r] * -bj;
                } else {
                    if (ci >= 0) lds_add(c.S + tri(c.n, ci + r), -bi);
                    if (cj >= 0) lds_add(c.S + tri(c.n, cj + r), -bj);
                }
            }
            if (MODE == kUpdate) return;
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
                if (MODE == kDiag && r != q) continue;
                double ii = 0, jj = 0, ij = 0;
#pragma unroll
                for (int m = 0; m < 6; ++m) {
                    ii += Ji[6 * m + r] * wi[m];
                    jj += Jj[6 * m + r] * wj[m];
                    ij += Ji[6 * m + r] * wj[m];
                }
                if (MODE == kDiag) {
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
    __device__ __forceinline__ static void pose_terms(const Ctx<Se3Model>& c, double& chi, double& scale) {
        const Window3Args& a = *c.a;
        for (int t = threadIdx.x; t < a.P + a.O; t += NT) {
            if (t < a.P) {
                if (MODE == kDiag) prior_term<kEval>(c, t, chi, scale);
                prior_term<MODE>(c, t, chi, scale);
            } else {
                if (MODE == kDiag) odometry_term<kEval>(c, t - a.P, chi, scale);
                odometry_term<MODE>(c, t - a.P, chi, scale);
            }
        }
    }

    // ------------------------------------------------------------------------------------------------------------------
    // LL^T of the augmented system in place (left-looking, 6 x 6 blocks, the right-hand side as block row nf), block column J:
    // T(I, J) = S(I, J) - sum_{K < J} L(I, K) L(J, K)^T, LPB lanes sharing the sum over K; every block's first lane factorises
    // T(J, J) (from the strip tjj, 21 words) for itself and solves L(I, J) = T(I, J) L(J, J)^-T.  (The plan of the SE(2) model's
    // factor_column, csrc/ba_window.hip, but S(I, J) is read after the sum and nothing is requested ahead: the registers are full.)
    // ------------------------------------------------------------------------------------------------------------------
    template <int NT, int LPB>
    __device__ __forceinline__ static void factor_column(double* S, double* invd, double* tjj, int nf, int J, int* fail) {
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

    // x = L^-T y by ONE wave: y (row n of the factor) in registers, three unknowns per lane (n <= 192), a pose block per step from the
    // last to the first: its six unknowns by scalar broadcasts and its own triangle, then its six rows of L update every earlier y
    __device__ __forceinline__ static void back_substitute(const double* S, const double* invd, int nf, double* x) {
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

    // VertexSE3Expmap::oplusImpl: exp(dx) T (a fixed pose is copied)
    __device__ __forceinline__ static void oplus(const double* cur, int cp, const double* xs, double lambda, double* trl, double*, double& scale) {
        Se3 T = se3_load(cur);
        if (cp >= 0) {
            double u[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                u[r] = xs[cp + r];
                scale += lambda * (u[r] * u[r]);
            }
            T = se3_mul(se3_exp(u), T);
        }
        se3_store(T, trl);
    }
};

template <int NT>
__global__ __launch_bounds__(NT) void k_window_lm3(const Window3Args* __restrict__ all) {
    __shared__ WindowShared<6> sh;
    window_lm<Se3Model, NT>(all[blockIdx.x], sh);
}

}  // namespace

namespace se2gpu {

// 256 or 128 threads, never 512: at 512 a lane has 256 registers, and the pose terms (6 x 6 adjoints and information) of this kernel
// spill to scratch there, where the wider widths keep everything in registers (VGPRs + AGPRs).  With P = nfree + 1 the largest window
// that fits 160 KiB has 27 free key frames at 256 threads and 29 at 128 (26 / 29 next to 6 fixed reference key frames).
size_t ba_window3_lds_bytes(int P, int nfree, int threads) {
    if (threads != 256 && threads != 128) return 0;
    return window_lds_bytes<Se3Model>(P, nfree, threads);
}

int ba_window3_launch(const Window3Args* d_args, int count, int threads, size_t lds_bytes, hipStream_t st) {
    if (count <= 0) return SE2GPU_OK;
    if (threads == 256) return window_launch<&k_window_lm3<256>, 256>(d_args, count, lds_bytes, st);
    if (threads == 128) return window_launch<&k_window_lm3<128>, 128>(d_args, count, lds_bytes, st);
    set_error("SE3 window kernel: 128 or 256 threads");
    return SE2GPU_ERR_INVALID;
}

}  // namespace se2gpu
