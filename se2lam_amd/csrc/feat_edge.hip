// libse2gpu - GlobalMapper::CreateFeatEdge (/root/reference/src/GlobalMapper.cpp:737-843) for a BATCH of key-frame pairs: the
// two-key-frame bundle adjustment OptKFPair (:847-927, key frame 0 fixed) / OptKFPairMatch (:929-1032, both free, chi2
// rejection of points) and, on the same stream with no host round trip, Sparsifier::DoMarginalizeSE3XYZ (sparsify.hip) on the
// optimised poses and the surviving points.
//
// The graph: two g2o::VertexSE3 (T_w_c, update X <- X * fromVectorMQT(d)) with the EdgeSE3Prior of addVertexSE3PlaneMotion
// each, N marginalised VertexPointXYZ, and per point one EdgeSE3PointXYZ to each key frame (offset = identity):
//     e = R' (p - t) - z,   d e / d pose = [-I | 2 [z_c]x],   d e / d p = R',   Huber on e' W e (first order: W rho').
// One wave per pair for the whole optimize(iters).  Lane l owns the points l, l + 64, ... in every pass, so no pass reads
// what another lane wrote.  Per trial: the points' 3x3 factors (chol3) and their Schur terms of the 12x12 pose system are
// summed per lane in point order (in the lane's own column of an LDS strip: 90 accumulators next to the edge temporaries do
// not fit the register file) and over the wave by a fixed butterfly (no atomics: a pair's result depends neither on the run
// nor on the batch around it); every lane then holds the same system and factors it itself; back-substitution and
// the trial's chi2 are a second pass over the lane's points.  g2o's Levenberg-Marquardt controller as in oracle/pg_ref.cpp.
// A fixed key frame 0 keeps the 12x12 shape: its rows are the identity and its couplings zero, its update is exactly 0.
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.h"
#include "se3_math.h"
#include "ba_window_common.h"

using namespace se2gpu;

namespace {

// (translation, compact quaternion) Jacobian of one edge w.r.t. its pose: column c of [-I | 2 [zc]x], as a 3-vector
__device__ __forceinline__ void pose_jac(const double zc[3], double J[18]) {   // 3 x 6 row-major
    J[0] = -1; J[1] = 0; J[2] = 0; J[3] = 0; J[4] = -2 * zc[2]; J[5] = 2 * zc[1];
    J[6] = 0; J[7] = -1; J[8] = 0; J[9] = 2 * zc[2]; J[10] = 0; J[11] = -2 * zc[0];
    J[12] = 0; J[13] = 0; J[14] = -1; J[15] = -2 * zc[1]; J[16] = 2 * zc[0]; J[17] = 0;
}

// e = R' (p - t) - z and e' W e
__device__ __forceinline__ double edge_error(const Se3& X, const double p[3], const double* z, const double* W, double zc[3],
                                             double e[3]) {
    const double d[3] = {p[0] - X.t[0], p[1] - X.t[1], p[2] - X.t[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        zc[i] = X.R[i] * d[0] + X.R[3 + i] * d[1] + X.R[6 + i] * d[2];
        e[i] = zc[i] - z[i];
    }
    double chi = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) chi += e[r] * (W[3 * r] * e[0] + W[3 * r + 1] * e[1] + W[3 * r + 2] * e[2]);
    return chi;
}

// Both edges of one point at (X, p): the point's block hll (packed as chol3 reads it: 00, 10, 20, 11, 21, 22), bl, the
// 12 x 3 coupling hpl; with POSE also the key frames' diagonal blocks (hpp: two packed lower triangles of 21) and their b
// added to g.  Returns the robust cost of the two edges.
template <bool POSE>
__device__ __forceinline__ double linearize_point(const Se3* X, bool fixed0, const double p[3], const double* z6, const double* W18,
                                                  double delta, double hll[6], double bl[3], double hpl[36], double* hpp, double* g) {
    double cost = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) hll[i] = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) bl[i] = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const Se3& T = X[k];
        double W[9], zc[3], e[3], rho0, rho1;
#pragma unroll
        for (int i = 0; i < 9; ++i) W[i] = W18[9 * k + i];
        const double chi = edge_error(T, p, z6 + 3 * k, W, zc, e);
        huber_w(chi, delta, rho0, rho1);
        cost += rho0;
#pragma unroll
        for (int i = 0; i < 9; ++i) W[i] *= rho1;
        double We[3], WR[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            We[r] = W[3 * r] * e[0] + W[3 * r + 1] * e[1] + W[3 * r + 2] * e[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) WR[3 * r + c] = W[3 * r] * T.R[3 * c] + W[3 * r + 1] * T.R[3 * c + 1] + W[3 * r + 2] * T.R[3 * c + 2];
        }
        // hll += R W R', bl -= R W e
        hll[0] += T.R[0] * WR[0] + T.R[1] * WR[3] + T.R[2] * WR[6];
        hll[1] += T.R[3] * WR[0] + T.R[4] * WR[3] + T.R[5] * WR[6];
        hll[2] += T.R[6] * WR[0] + T.R[7] * WR[3] + T.R[8] * WR[6];
        hll[3] += T.R[3] * WR[1] + T.R[4] * WR[4] + T.R[5] * WR[7];
        hll[4] += T.R[6] * WR[1] + T.R[7] * WR[4] + T.R[8] * WR[7];
        hll[5] += T.R[6] * WR[2] + T.R[7] * WR[5] + T.R[8] * WR[8];
#pragma unroll
        for (int a = 0; a < 3; ++a) bl[a] -= T.R[3 * a] * We[0] + T.R[3 * a + 1] * We[1] + T.R[3 * a + 2] * We[2];
        if (k == 0 && fixed0) {
#pragma unroll
            for (int i = 0; i < 18; ++i) hpl[i] = 0;
            if (POSE)
#pragma unroll
                for (int i = 0; i < 21; ++i) hpp[i] = 0;
            continue;
        }
        double J[18];
        pose_jac(zc, J);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) hpl[3 * (6 * k + a) + b] = J[a] * WR[b] + J[6 + a] * WR[3 + b] + J[12 + a] * WR[6 + b];
        if (POSE) {
            double WJ[18];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) WJ[6 * r + c] = W[3 * r] * J[c] + W[3 * r + 1] * J[6 + c] + W[3 * r + 2] * J[12 + c];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int c = 0; c <= a; ++c) hpp[21 * k + tri(a, c)] = J[a] * WJ[c] + J[6 + a] * WJ[6 + c] + J[12 + a] * WJ[12 + c];
                g[6 * k + a] -= J[a] * We[0] + J[6 + a] * We[1] + J[12 + a] * We[2];
            }
        }
    }
    return cost;
}

// Y = G^-1 hpl' (row r of Y = G^-1 applied to row r of hpl) and u = G^-1 bl for the factor a = G^-1 of hll + lambda I
__device__ __forceinline__ void point_factor(const double a[6], const double hpl[36], const double bl[3], double Y[36], double u[3]) {
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        Y[3 * r] = a[0] * hpl[3 * r];
        Y[3 * r + 1] = a[1] * hpl[3 * r] + a[2] * hpl[3 * r + 1];
        Y[3 * r + 2] = a[3] * hpl[3 * r] + a[4] * hpl[3 * r + 1] + a[5] * hpl[3 * r + 2];
    }
    u[0] = a[0] * bl[0];
    u[1] = a[1] * bl[0] + a[2] * bl[1];
    u[2] = a[3] * bl[0] + a[4] * bl[1] + a[5] * bl[2];
}

// EdgeSE3Prior of key frame k: error toVectorMQT(Z^-1 X), Jacobian mqt_jac_right.  With LIN: H and b into the system.
// (a template flag, not a NULL test of S: comparing the array's address keeps it out of registers)
template <bool LIN>
__device__ __forceinline__ double prior_terms(const double* Z12, const Se3& X, const double* info, int k, double* S, double* g) {
    const Se3 E = iso_mul(se3_inv(se3_load(Z12)), X);   // (the measurement is read where it is used: 24 doubles less to keep)
    double e[6], We[6];
    to_mqt(E, e);
    double chi = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double v = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) v += info[6 * r + c] * e[c];
        We[r] = v;
        chi += e[r] * v;
    }
    if (LIN) {
        double J[36], WJ[36];
        mqt_jac_right(E, J);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) v += info[6 * r + q] * J[6 * q + c];
                WJ[6 * r + c] = v;
            }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int c = 0; c <= a; ++c) {
                double v = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) v += J[6 * q + a] * WJ[6 * q + c];
                S[tri(6 * k + a, 6 * k + c)] += v;
            }
            double v = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) v += J[6 * q + a] * We[q];
            g[6 * k + a] -= v;
        }
    }
    return chi;
}

// the diagonal of the prior's J' W J (for lambda_0)
__device__ __forceinline__ void prior_diag(const double* Z12, const Se3& X, const double* info, double d[6]) {
    double J[36];
    mqt_jac_right(iso_mul(se3_inv(se3_load(Z12)), X), J);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double v = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int r = 0; r < 6; ++r) v += J[6 * q + a] * info[6 * q + r] * J[6 * r + a];
        d[a] = v;
    }
}

// dense L L' of the packed 12 x 12 and the solve x <- S^-1 x; false when a pivot is not positive
__device__ __forceinline__ bool chol12_solve(double* S, double* x) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        double d = S[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= S[tri(j, k)] * S[tri(j, k)];
        ok = ok && d > 0.0;
        d = sqrt(d);
        S[tri(j, j)] = d;
        const double inv = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < 12; ++i) {
            double v = S[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= S[tri(i, k)] * S[tri(j, k)];
            S[tri(i, j)] = v * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        double v = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= S[tri(i, k)] * x[k];
        x[i] = v / S[tri(i, i)];
    }
#pragma unroll
    for (int i = 11; i >= 0; --i) {
        double v = x[i];
#pragma unroll
        for (int k = i + 1; k < 12; ++k) v -= S[tri(k, i)] * x[k];
        x[i] = v / S[tri(i, i)];
    }
    return ok;
}

using FeatArgs = FeatEdgeArgs;   // common.h

__global__ __launch_bounds__(64) void k_feat_edge(const FeatArgs A) {
    const int p = blockIdx.x;
    if (p >= A.npairs) return;
    const int lane = threadIdx.x;
    __shared__ double strip[78 * 64];
    const int j0 = A.mp_ptr[p], N = A.mp_cnt ? A.mp_cnt[p] : A.mp_ptr[p + 1] - j0;
    const double* z = A.m_z + 6 * (size_t)j0;
    const double* W = A.m_info + 18 * (size_t)j0;
    double* cur = A.pa + 3 * (size_t)j0;
    double* trial = A.pb + 3 * (size_t)j0;
    Se3 X[2] = {se3_load(A.kf12 + 24 * (size_t)p), se3_load(A.kf12 + 24 * (size_t)p + 12)};
    if ((A.raw_cnt ? A.raw_cnt[p] : N) < A.min_points) {   // nothing is run: poses and points as given, no constraint
        for (int j = lane; j < N; j += 64)
            for (int i = 0; i < 3; ++i) A.mp_out[3 * (size_t)(j0 + j) + i] = cur[3 * j + i];
        if (lane == 0) {
            se3_store(X[0], A.kf12_out + 24 * (size_t)p);
            se3_store(X[1], A.kf12_out + 24 * (size_t)p + 12);
            A.info4[4 * p] = 1; A.info4[4 * p + 1] = N; A.info4[4 * p + 2] = 0; A.info4[4 * p + 3] = 0;
            A.sp_cnt[p] = 0;
        }
        return;
    }
    const bool fixed0 = A.mode == SE2GPU_FEAT_EDGE_COVIS;
    const double delta = A.huber_delta;
    const double* pmeas = A.prior_meas + 24 * (size_t)p;
    const double* pinfo = A.prior_info + 72 * (size_t)p;

    // cost at the start
    double chi_cur = 0;
    for (int j = lane; j < N; j += 64) {
        const double pt[3] = {cur[3 * j], cur[3 * j + 1], cur[3 * j + 2]};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double zc[3], e[3], r0, r1;
            huber_w(edge_error(X[k], pt, z + 6 * j + 3 * k, W + 18 * j + 9 * k, zc, e), delta, r0, r1);
            chi_cur += r0;
        }
    }
    chi_cur = wsum(chi_cur);
    chi_cur += prior_terms<false>(pmeas, X[0], pinfo, 0, nullptr, nullptr) + prior_terms<false>(pmeas + 12, X[1], pinfo + 36, 1, nullptr, nullptr);
    const double chi_init = chi_cur;

    double lambda = 0, ni = 2;
    int trials = 0, iterations = 0, terminated = 0;
    se2gpu_ba_stats* st = A.stats ? A.stats + p : nullptr;
    for (int it = 0; it < A.iters; ++it) {
        if (it == 0) {   // lambda_0 = 1e-5 * the largest diagonal entry of H over the free vertices, poses and points
            double dsum[12], g[12], maxd = 0;
#pragma unroll
            for (int i = 0; i < 12; ++i) dsum[i] = g[i] = 0;
            for (int j = lane; j < N; j += 64) {
                const double pt[3] = {cur[3 * j], cur[3 * j + 1], cur[3 * j + 2]};
                double hll[6], bl[3], hpl[36], hpp[42];
                (void)linearize_point<true>(X, fixed0, pt, z + 6 * j, W + 18 * j, delta, hll, bl, hpl, hpp, g);
#pragma unroll
                for (int r = 0; r < 12; ++r) dsum[r] += hpp[21 * (r / 6) + tri(r % 6, r % 6)];
                maxd = fmax(maxd, fmax(fabs(hll[0]), fmax(fabs(hll[3]), fabs(hll[5]))));
            }
            maxd = wmax(maxd);
            double D[12];
            prior_diag(pmeas, X[0], pinfo, D);
            prior_diag(pmeas + 12, X[1], pinfo + 36, D + 6);
#pragma unroll
            for (int r = 0; r < 12; ++r) {
                const double d = wsum(dsum[r]) + D[r];
                if (r >= 6 || !fixed0) maxd = fmax(maxd, fabs(d));
            }
            lambda = 1e-5 * maxd;
            ni = 2;
        }
        double rho = 0;
        int qmax = 0;
        do {
            // pass 1: the reduced pose system at this lambda
            // A lane's 78 sums live in its own column of the LDS strip (the registers go to the point's temporaries): written and
            // read by that lane alone, in point order, so nothing is shared before the butterfly
            // The two priors enter through lane 0's column, computed here while nothing else is live.
            double S[78], g[12];
#pragma unroll
            for (int i = 0; i < 78; ++i) S[i] = 0;
#pragma unroll
            for (int i = 0; i < 12; ++i) g[i] = 0;
            if (!fixed0) (void)prior_terms<true>(pmeas, X[0], pinfo, 0, S, g);
            (void)prior_terms<true>(pmeas + 12, X[1], pinfo + 36, 1, S, g);
#pragma unroll
            for (int i = 0; i < 78; ++i) strip[64 * i + lane] = lane == 0 ? S[i] : 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) g[i] = lane == 0 ? g[i] : 0.0;
            for (int j = lane; j < N; j += 64) {
                const double pt[3] = {cur[3 * j], cur[3 * j + 1], cur[3 * j + 2]};
                double hll[6], bl[3], hpl[36], hpp[42], a[6], Y[36], u[3];
                (void)linearize_point<true>(X, fixed0, pt, z + 6 * j, W + 18 * j, delta, hll, bl, hpl, hpp, g);
                chol3(hll, lambda, a);
                point_factor(a, hpl, bl, Y, u);
#pragma unroll
                for (int r = 0; r < 12; ++r) {
#pragma unroll
                    for (int c = 0; c <= r; ++c) {
                        double v = -(Y[3 * r] * Y[3 * c] + Y[3 * r + 1] * Y[3 * c + 1] + Y[3 * r + 2] * Y[3 * c + 2]);
                        if (r / 6 == c / 6) v += hpp[21 * (r / 6) + tri(r % 6, c % 6)];
                        strip[64 * tri(r, c) + lane] += v;
                    }
                    g[r] -= Y[3 * r] * u[0] + Y[3 * r + 1] * u[1] + Y[3 * r + 2] * u[2];
                }
            }
#pragma unroll
            for (int i = 0; i < 78; ++i) S[i] = wsum(strip[64 * i + lane]);
#pragma unroll
            for (int i = 0; i < 12; ++i) g[i] = wsum(g[i]);
#pragma unroll
            for (int r = 0; r < 12; ++r) {
                if (r < 6 && fixed0) { S[tri(r, r)] = 1.0; g[r] = 0.0; }
                else S[tri(r, r)] += lambda;
            }
            double dp[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) dp[i] = g[i];
            const bool ok = chol12_solve(S, dp);
            double chi_t = DBL_MAX, scale = 0;
            Se3 T[2] = {X[0], X[1]};
            if (ok) {
                if (!fixed0) T[0] = iso_mul(X[0], from_mqt(dp));
                T[1] = iso_mul(X[1], from_mqt(dp + 6));
                // pass 2: the points' steps, the trial's cost and the gain's denominator sum x (lambda x + b) over every vertex.  The
                // poses' b is g + sum hpl A bl; its share dp' hpl A bl = (Y' dp) . u is added point by point
                double ct = 0, sc = 0;
                for (int j = lane; j < N; j += 64) {
                    const double pt[3] = {cur[3 * j], cur[3 * j + 1], cur[3 * j + 2]};
                    double hll[6], bl[3], hpl[36], a[6], Y[36], u[3];
                    (void)linearize_point<false>(X, fixed0, pt, z + 6 * j, W + 18 * j, delta, hll, bl, hpl, nullptr, nullptr);
                    chol3(hll, lambda, a);
                    point_factor(a, hpl, bl, Y, u);
                    double yd[3] = {0, 0, 0};
#pragma unroll
                    for (int r = 0; r < 12; ++r) {
                        yd[0] += Y[3 * r] * dp[r]; yd[1] += Y[3 * r + 1] * dp[r]; yd[2] += Y[3 * r + 2] * dp[r];
                    }
                    const double v[3] = {u[0] - yd[0], u[1] - yd[1], u[2] - yd[2]};
                    const double dl[3] = {a[0] * v[0] + a[1] * v[1] + a[3] * v[2], a[2] * v[1] + a[4] * v[2], a[5] * v[2]};
                    sc += yd[0] * u[0] + yd[1] * u[1] + yd[2] * u[2];
#pragma unroll
                    for (int i = 0; i < 3; ++i) sc += dl[i] * (lambda * dl[i] + bl[i]);
                    const double pn[3] = {pt[0] + dl[0], pt[1] + dl[1], pt[2] + dl[2]};
#pragma unroll
                    for (int i = 0; i < 3; ++i) trial[3 * j + i] = pn[i];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        double zc[3], e[3], r0, r1;
                        huber_w(edge_error(T[k], pn, z + 6 * j + 3 * k, W + 18 * j + 9 * k, zc, e), delta, r0, r1);
                        ct += r0;
                    }
                }
                chi_t = wsum(ct);
                scale = wsum(sc);
                chi_t += prior_terms<false>(pmeas, T[0], pinfo, 0, nullptr, nullptr) + prior_terms<false>(pmeas + 12, T[1], pinfo + 36, 1, nullptr, nullptr);
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    if (i >= 6 || !fixed0) scale += dp[i] * (lambda * dp[i] + g[i]);
            }
            ++trials; ++qmax;
            rho = (chi_cur - chi_t) / (scale + 1e-3);
            if (rho > 0 && isfinite(chi_t)) {
                double alpha = 1. - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                chi_cur = chi_t;
                X[0] = T[0]; X[1] = T[1];
                double* t = cur; cur = trial; trial = t;
            } else {
                lambda *= ni; ni *= 2;
            }
        } while (rho < 0 && qmax < 10);
        if (st && lane == 0) { st->chi2_hist[it] = chi_cur; st->lambda_hist[it] = lambda; st->trials_hist[it] = qmax; }
        iterations = it + 1;
        if (qmax == 10 || rho == 0) { terminated = 1; break; }
    }

    // the non-robust chi2 of every edge; in match mode a point with either edge above the threshold is an outlier
    const bool reject = A.mode == SE2GPU_FEAT_EDGE_MATCH && A.outlier_chi2 > 0;
    bool finite = isfinite(chi_cur);
#pragma unroll
    for (int i = 0; i < 9; ++i) finite = finite && isfinite(X[0].R[i]) && isfinite(X[1].R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) finite = finite && isfinite(X[0].t[i]) && isfinite(X[1].t[i]);
    int nout = 0, nin = 0;
    for (int base = 0; base < N; base += 64) {   // whole-wave steps: the ballot orders the survivors as they were given
        const int j = base + lane;
        bool in = false, bad = false;
        double pt[3] = {0, 0, 0};
        if (j < N) {
            double zc[3], e[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) pt[i] = cur[3 * j + i];
            const double c0 = edge_error(X[0], pt, z + 6 * j, W + 18 * j, zc, e);
            const double c1 = edge_error(X[1], pt, z + 6 * j + 3, W + 18 * j + 9, zc, e);
            const bool out = reject && (c0 > A.outlier_chi2 || c1 > A.outlier_chi2);
            A.edge_chi2[2 * (size_t)(j0 + j)] = c0;
            A.edge_chi2[2 * (size_t)(j0 + j) + 1] = c1;
            A.outlier[j0 + j] = out ? 1 : 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) A.mp_out[3 * (size_t)(j0 + j) + i] = pt[i];
            in = !out;
            bad = !(isfinite(pt[0]) && isfinite(pt[1]) && isfinite(pt[2]) && isfinite(c0) && isfinite(c1));
        }
        const unsigned long long m = __ballot(in);
        if (__ballot(bad)) finite = false;
        if (in) {
            const int slot = j0 + nin + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
            for (int i = 0; i < 3; ++i) A.sp_xyz[3 * (size_t)slot + i] = pt[i];
            for (int i = 0; i < 18; ++i) A.sp_info[18 * (size_t)slot + i] = W[18 * j + i];
        }
        const int cnt = __popcll(m);
        nin += cnt;
        nout += min(64, N - base) - cnt;
    }
    if (lane == 0) {
        se3_store(X[0], A.kf12_out + 24 * (size_t)p);
        se3_store(X[1], A.kf12_out + 24 * (size_t)p + 12);
        A.info4[4 * p] = finite ? 0 : 2;
        A.info4[4 * p + 1] = N;
        A.info4[4 * p + 2] = nout;
        A.info4[4 * p + 3] = finite ? nin : 0;
        A.sp_cnt[p] = finite ? nin : 0;
        if (st) {
            st->iterations = iterations; st->trials = trials; st->terminated = terminated; st->stopped = 0;
            st->chi2_init = chi_init; st->chi2_final = chi_cur; st->lambda_final = lambda;
        }
    }
}

}  // namespace

namespace se2gpu {

int launch_feat_edge(hipStream_t st, const FeatEdgeArgs& args) {
    hipLaunchKernelGGL(k_feat_edge, dim3(args.npairs), dim3(64), 0, st, args);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // namespace se2gpu

extern "C" {

int se2gpu_feat_edge_batch(int npairs, int mode, int iters, int min_points, const double* kf12, const double* Tbc12,
                           double xrot_info, double yrot_info, double z_info, const int32_t* mp_ptr, const double* mp_xyz,
                           const double* m_z, const double* m_info, double huber_delta, double outlier_chi2, double* kf12_out,
                           double* mp_xyz_out, uint8_t* outlier, double* edge_chi2, int32_t* info4, se2gpu_ba_stats* stats,
                           double* z_out12, double* info_out36) {
    // every refusal comes before the first use of a device
    SE2_REQUIRE(npairs >= 0, SE2GPU_ERR_INVALID, "feat_edge: negative pair count");
    SE2_REQUIRE(kf12 && Tbc12 && mp_ptr && kf12_out && info4 && z_out12 && info_out36, SE2GPU_ERR_INVALID, "feat_edge: NULL argument");
    SE2_REQUIRE(mode == SE2GPU_FEAT_EDGE_COVIS || mode == SE2GPU_FEAT_EDGE_MATCH, SE2GPU_ERR_INVALID, "feat_edge: mode %d", mode);
    SE2_REQUIRE(iters >= 1 && iters <= 64, SE2GPU_ERR_INVALID, "feat_edge: %d iterations (1..64, the length of the se2gpu_ba_stats histories)", iters);
    SE2_REQUIRE(npairs < 65536, SE2GPU_ERR_CAPACITY, "feat_edge: %d pairs in one call (at most 65535)", npairs);
    SE2_REQUIRE(mp_ptr[0] == 0, SE2GPU_ERR_INVALID, "feat_edge: mp_ptr must start at 0");
    for (int p = 0; p < npairs; ++p)
        SE2_REQUIRE(mp_ptr[p + 1] >= mp_ptr[p], SE2GPU_ERR_INVALID, "feat_edge: mp_ptr decreases at pair %d", p);
    const int NP = mp_ptr[npairs];
    SE2_REQUIRE(NP == 0 || (mp_xyz && m_z && m_info && mp_xyz_out && outlier && edge_chi2), SE2GPU_ERR_INVALID, "feat_edge: NULL array");
    SE2_REQUIRE(have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)");
    if (npairs == 0) return SE2GPU_OK;
    // the EdgeSE3Prior of every key frame, from its INPUT pose (addVertexSE3PlaneMotion)
    std::vector<double> pmeas(24 * (size_t)npairs), pinfo(72 * (size_t)npairs);
    for (size_t k = 0; k < 2 * (size_t)npairs; ++k)
        SE2_CHECK(se2gpu_plane_motion_prior_iso3(kf12 + 12 * k, Tbc12, xrot_info, yrot_info, z_info, &pmeas[12 * k], &pinfo[36 * k]));
    // k_sparsify's index arrays for the dense layout: point j has the measurements 2j (key frame 0) and 2j + 1, listed in
    // that order (GlobalMapper.cpp:798-833)
    const size_t np1 = (size_t)std::max(NP, 1);
    std::vector<int> mm_ptr((size_t)NP + 1), m_kf(2 * np1), ord(2 * np1), ord_ptr((size_t)npairs + 1);
    for (int j = 0; j <= NP; ++j) mm_ptr[j] = 2 * j;
    for (size_t i = 0; i < 2 * np1; ++i) { m_kf[i] = (int)(i & 1); ord[i] = (int)i; }
    for (int p = 0; p <= npairs; ++p) ord_ptr[p] = 2 * mp_ptr[p];
    DevBuf<double> d_kf, d_pm, d_pi, d_z, d_w, d_pa, d_pb, d_kfo, d_mpo, d_chi, d_spx, d_spi, d_blk, d_schur, d_zo, d_io;
    DevBuf<int> d_mpp, d_mmp, d_mkf, d_ordp, d_ord, d_cnt, d_info4;
    DevBuf<uint8_t> d_outl;
    DevBuf<se2gpu_ba_stats> d_stats;
    hipStream_t st = nullptr;
    SE2_CHECK(d_kf.upload(kf12, 24 * (size_t)npairs, st));
    SE2_CHECK(d_pm.upload(pmeas, st));
    SE2_CHECK(d_pi.upload(pinfo, st));
    SE2_CHECK(d_mpp.upload(mp_ptr, (size_t)npairs + 1, st));
    SE2_CHECK(d_z.reserve(6 * np1));
    SE2_CHECK(d_w.reserve(18 * np1));
    SE2_CHECK(d_pa.reserve(3 * np1));
    if (NP) {
        SE2_HIP(hipMemcpyAsync(d_z.p, m_z, 6 * (size_t)NP * 8, hipMemcpyHostToDevice, st));
        SE2_HIP(hipMemcpyAsync(d_w.p, m_info, 18 * (size_t)NP * 8, hipMemcpyHostToDevice, st));
        SE2_HIP(hipMemcpyAsync(d_pa.p, mp_xyz, 3 * (size_t)NP * 8, hipMemcpyHostToDevice, st));
    }
    SE2_CHECK(d_pb.reserve(3 * np1));
    SE2_CHECK(d_kfo.reserve(24 * (size_t)npairs));
    SE2_CHECK(d_mpo.reserve(3 * np1));
    SE2_CHECK(d_chi.reserve(2 * np1));
    SE2_CHECK(d_outl.reserve(np1));
    SE2_CHECK(d_info4.reserve(4 * (size_t)npairs));
    SE2_CHECK(d_spx.reserve(3 * np1));
    SE2_CHECK(d_spi.reserve(18 * np1));
    SE2_CHECK(d_cnt.reserve((size_t)npairs));
    SE2_CHECK(d_stats.reserve((size_t)npairs));
    SE2_HIP(hipMemsetAsync(d_chi.p, 0, 2 * np1 * 8, st));
    SE2_HIP(hipMemsetAsync(d_outl.p, 0, np1, st));
    SE2_HIP(hipMemsetAsync(d_stats.p, 0, (size_t)npairs * sizeof(se2gpu_ba_stats), st));
    SE2_CHECK(d_mmp.upload(mm_ptr, st));
    SE2_CHECK(d_mkf.upload(m_kf, st));
    SE2_CHECK(d_ord.upload(ord, st));
    SE2_CHECK(d_ordp.upload(ord_ptr, st));
    SE2_CHECK(d_blk.reserve(2 * np1 * 36));
    SE2_CHECK(d_schur.reserve(np1 * 144));
    SE2_CHECK(d_zo.reserve(12 * (size_t)npairs));
    SE2_CHECK(d_io.reserve(36 * (size_t)npairs));
    FeatArgs a;
    a.npairs = npairs; a.mode = mode; a.iters = iters; a.min_points = min_points;
    a.kf12 = d_kf.p; a.prior_meas = d_pm.p; a.prior_info = d_pi.p; a.mp_ptr = d_mpp.p; a.m_z = d_z.p; a.m_info = d_w.p;
    a.mp_cnt = nullptr; a.raw_cnt = nullptr;   // dense rows: every point of [mp_ptr[p], mp_ptr[p+1]) counts
    a.huber_delta = huber_delta; a.outlier_chi2 = outlier_chi2;
    a.pa = d_pa.p; a.pb = d_pb.p; a.kf12_out = d_kfo.p; a.mp_out = d_mpo.p; a.outlier = d_outl.p; a.edge_chi2 = d_chi.p;
    a.info4 = d_info4.p; a.stats = d_stats.p; a.sp_xyz = d_spx.p; a.sp_info = d_spi.p; a.sp_cnt = d_cnt.p;
    SE2_CHECK(launch_feat_edge(st, a));
    SE2_CHECK(launch_sparsify(st, npairs, d_kfo.p, d_mpp.p, d_spx.p, d_mmp.p, d_mkf.p, d_spi.p, d_ordp.p, d_ord.p, d_blk.p, d_schur.p,
                              d_cnt.p, d_zo.p, d_io.p));
    SE2_HIP(hipMemcpyAsync(kf12_out, d_kfo.p, 24 * (size_t)npairs * 8, hipMemcpyDeviceToHost, st));
    SE2_HIP(hipMemcpyAsync(info4, d_info4.p, 4 * (size_t)npairs * 4, hipMemcpyDeviceToHost, st));
    if (NP) {
        SE2_HIP(hipMemcpyAsync(mp_xyz_out, d_mpo.p, 3 * (size_t)NP * 8, hipMemcpyDeviceToHost, st));
        SE2_HIP(hipMemcpyAsync(outlier, d_outl.p, (size_t)NP, hipMemcpyDeviceToHost, st));
        SE2_HIP(hipMemcpyAsync(edge_chi2, d_chi.p, 2 * (size_t)NP * 8, hipMemcpyDeviceToHost, st));
    }
    if (stats) SE2_HIP(hipMemcpyAsync(stats, d_stats.p, (size_t)npairs * sizeof(se2gpu_ba_stats), hipMemcpyDeviceToHost, st));
    SE2_HIP(hipMemcpyAsync(z_out12, d_zo.p, 12 * (size_t)npairs * 8, hipMemcpyDeviceToHost, st));
    SE2_HIP(hipMemcpyAsync(info_out36, d_io.p, 36 * (size_t)npairs * 8, hipMemcpyDeviceToHost, st));
    SE2_HIP(hipStreamSynchronize(st));
    // no constraint for a pair that was not run (1) or whose result is not finite (2)
    for (int p = 0; p < npairs; ++p) {
        bool fin = true;
        for (int i = 0; i < 12; ++i) fin = fin && std::isfinite(z_out12[12 * (size_t)p + i]);
        for (int i = 0; i < 36; ++i) fin = fin && std::isfinite(info_out36[36 * (size_t)p + i]);
        if (info4[4 * p] == 0 && !fin) { info4[4 * p] = 2; info4[4 * p + 3] = 0; }
        if (info4[4 * p] != 0) {
            std::memset(z_out12 + 12 * (size_t)p, 0, 96);
            std::memset(info_out36 + 36 * (size_t)p, 0, 288);
        }
    }
    return SE2GPU_OK;
}

}  // extern "C"
