// The one-workgroup-per-window local-BA kernel, once, for every pose model (csrc/ba_window.hip: SE(2)-XYZ, csrc/ba_window3.hip:
// SE3-expmap).  A workgroup owns a window for its whole optimize(iters): the poses, the reduced system S, the
// right-hand sides and the solution never leave LDS, and the LM controller runs in the workgroup:
//   OPEN    (once per optimize) the landmarks are listed by observation count, and one pass gives chi^2 of the starting state,
//           the diagonal for lambda_0 and a copy of the observations in the order of that list (whole cache lines from then on)
//   BUILD   the observations stream in once, one lane each, 4 / 8 / 16 / 64 lanes per landmark by its count: the model's residual,
//           Jacobians and weights, Hll / bl by a DPP butterfly inside the group, the 3x3 factor A = G^-1 of Hll + lambda I,
//           W_e = Hpl_e A^T in registers; the pose blocks Hpp_e - W_e W_e^T and b_e - W_e zeta go to S / b_s by LDS atomics
//           (ds_add_f64), the pair products W_i W_j^T of a landmark's observations through a per-wave staging strip (each pair
//           once: lane i takes the partners i + 1 .. i + k/2 cyclically); A (48 B per landmark) is left in memory for UPDATE
//   SOLVE   the model's left-looking LL^T on B x B blocks in LDS with the right-hand side as an extra block row, x = L^-T y by one wave
//   UPDATE  the observations stream in a second time: the Jacobians are RECOMPUTED (nothing per edge is kept) for the
//           back-substitution x_l = A^T (A (bl - sum_e Hlp_e dp_e)), the trial landmark goes to the other estimate buffer,
//           robust chi^2 at the trial state, the gain denominator; then g2o's accept / reject on the controller block
// Sums into S are atomic, hence in no fixed order: results agree with the multi-launch path to rounding, not bit for bit.
// A landmark with more than 64 observations is refused (BaCtl::error = 2: the caller runs the window on the multi-launch path).
//
// The pose model M is a type of static members; everything below is a force-inlined template over it, so each model's kernel is
// compiled as if written out by hand.  M gives
//   Args                    its argument pack (WindowArgsBase + camera and what else its pose terms read)
//   B                       rows of a pose block (3 / 6);    kPose, kCache   doubles of a pose in memory and LDS (3 / 12) and of what
//                           the model keeps next to each pose in LDS (sine and cosine of the heading: 2 / 0)
//   kStaticInts             the ints of static LDS its lds_bytes has always allowed for (decides which windows fit: not to be "fixed")
//   Edge, Records           an observation in registers; the arrays the opening pass copies the observations to, in list order, with
//                           load_edge (from the caller's arrays), store_record / load_record and records (their places behind the list)
//   cache_pose              fills a pose's kCache words
//   edge_chi                robust chi^2 of one observation at a given state
//   eval_front              the lambda_0 / UPDATE pass of one observation up to the group's sums: acc = hll diagonal | bl | q
//   Lin, linearize          the BUILD pass of one observation up to the group's sums: Jacobians and weights (Lin), its Hll and bl
//   pose_block              W_e = Hpl_e A^T, and the pose's own block and right-hand side into S
//   pose_terms<MODE, NT>    what is not an observation: odometry edges, priors
//   factor_column<NT, LPB>, back_substitute     the dense solve on B x B blocks
//   oplus                   a pose's trial state and the damping's share of the gain denominator
// and its .hip ends in the __global__ wrapper, which declares the kernel's static LDS (WindowShared<B>) and calls window_lm<M, NT>.
#pragma once
#include "ba_window.h"
#include "ba_window_common.h"

namespace {

using namespace se2gpu;
using namespace se2gpu::badev;

enum { kEval = 0, kDiag = 1, kBuild = 2, kUpdate = 3 };   // the passes (of the observations and of M::pose_terms)

// what a pass needs of the window, all in LDS except the edge arrays, the landmarks and the landmark order
template <class M>
struct Ctx {
    const typename M::Args* a;
    double* S;           // packed lower triangle of the augmented system, rows 0 .. n-1 = S, row n = b_s, rows n+1 .. n+B-1 zero
    double* x;           // n: the pose step (scratch of the lambda_0 pass: the diagonal of Hpp)
    const double* cur;   // kPose P: the estimate
    const double* cache_cur;  // kCache P: what the model keeps next to it
    const double* trl;   // kPose P: the trial state
    const double* cache_trl;  // kCache P
    const int* col;      // P: first column of a pose in the system, -1 = fixed
    double* stage;       // this wave's staging strip: 64 lanes x (3 B + 1)
    const double* lms;   // L x 3: the estimate's landmarks
    double* lms_trial;   // L x 3: the other buffer
    const int4* desc;    // L: {landmark, first record, observations, first edge}: the landmarks class by class (made by the prologue)
    // the observations of the landmarks with at most 16 of them, copied by the prologue in the ORDER OF THAT LIST (one array per field)
    typename M::Records rec;
    int n;
    double lambda;
};

// ------------------------------------------------------------------------------------------------------------------
// All passes: one lane per OBSERVATION, an aligned group of G lanes per landmark (G = 4, 8, 16 or 64 by the landmark's count; the
// landmarks are visited in ascending order of their counts, so a wave's groups are of a kind and consecutive lanes read consecutive
// edges).
// ------------------------------------------------------------------------------------------------------------------
template <class M>
struct GroupIn {
    int l, beg, k, at;   // landmark, first record, observations, place in the list
    double lx, ly, lz;
    typename M::Edge ed;
    bool has;
};
// a landmark's descriptor {landmark, first record, observations, first edge} from the list the prologue made; zero beyond the class's end
template <class M>
__device__ __forceinline__ int4 load_desc(const Ctx<M>& c, int idx, int end) {
    return idx < end ? c.desc[idx] : make_int4(0, 0, 0, 0);
}
// FIRST: the opening pass of an optimize() - the observations still come from the caller's arrays (d.w) and go to the record arrays
// on the way, so that every later pass reads them in the order of the list
template <class M, int G, bool FIRST = false>
__device__ __forceinline__ GroupIn<M> load_group(const Ctx<M>& c, const int4 d, int lane, int at) {
    const typename M::Args& a = *c.a;
    GroupIn<M> g;
    g.l = d.x; g.beg = d.y; g.k = d.z; g.at = at; g.lx = 0; g.ly = 0; g.lz = 1; g.has = false;
    g.ed = typename M::Edge{};
    if (g.k > 0) {
        g.lx = c.lms[3 * (size_t)g.l]; g.ly = c.lms[3 * (size_t)g.l + 1]; g.lz = c.lms[3 * (size_t)g.l + 2];
        const int sub = lane & (G - 1);
        g.has = sub < g.k;
        if (g.has) {
            if (G == 64) {
                g.ed = M::load_edge(a, g.beg + sub);   // (a wave per landmark: its observations lie together in the caller's arrays as they are)
            } else if (FIRST) {
                g.ed = M::load_edge(a, d.w + sub);
                M::store_record(c.rec, g.beg + sub, g.ed);
            } else {
                g.ed = M::load_record(c.rec, g.beg + sub);
            }
        }
    }
    return g;
}

// EVAL / DIAG / UPDATE of one landmark.  Nothing but sums crosses lanes: for the back-substitution bl - q with
// q = sum_e Hlp_e dp_e, and then   x_l = (Hll + lambda I)^-1 (bl - q) = A^T A (bl - q)   needs neither W_e nor a second look at the
// Jacobians (sum_e W_e^T dp_e = A q: the factor A comes out of the sum).  A itself - 48 bytes per landmark - is what the build pass of
// the same trial computed: it travels through memory (WindowArgsBase::ainv, list order), which spares this pass the six sums of Hll and
// its factorisation, a third of its instructions.
template <class M, int MODE, int G>
__device__ __forceinline__ void eval_group(const Ctx<M>& c, const GroupIn<M>& g, int lane, double& chi, double& scale, double& dmax) {
    const typename M::Args& a = *c.a;
    const int sub = lane & (G - 1);
    const bool has = g.has;
    const int kf = g.ed.kf;
    if (MODE == kEval) {
        const double r0 = M::edge_chi(a, g.ed, c.cur, c.cache_cur, g.lx, g.ly, g.lz);
        if (has) chi += r0;
        return;
    }
    const int c0 = has ? c.col[kf] : -1;
    // the update pass: A = G^-1 of Hll + lambda I as this trial's build pass left it (requested here, needed after the sums)
    double2 A01 = {1, 0}, A23 = {1, 0}, A45 = {0, 1};
    if (MODE == kUpdate && g.k > 0) {
        const double2* src = reinterpret_cast<const double2*>(a.ainv + 6 * (size_t)g.at);
        A01 = src[0]; A23 = src[1]; A45 = src[2];
    }
    double acc[12];   // hll (6: the lambda_0 pass only) | bl (3) | q (3); the update pass sums bl - q as one vector (slots 6..8)
    M::template eval_front<MODE>(c, g, c0, acc, chi, scale);
    if (!has) {   // (its arithmetic ran on a made-up edge and may hold infinities: nothing of it may reach the group's sums)
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    }
    if (MODE == kDiag) {   // lambda_0 = 1e-5 max diag H (computeLambdaInit): the landmark blocks' diagonals
        const double h0 = gsum<G>(acc[0]), h3 = gsum<G>(acc[3]), h5 = gsum<G>(acc[5]);
        if (g.k > 0) dmax = fmax(dmax, fmax(fabs(h0), fmax(fabs(h3), fabs(h5))));
        return;
    }
    const double ble[3] = {acc[6], acc[7], acc[8]};   // this observation's own b_l share: x_l . b_l is summed observation by observation
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
    scale += xl[0] * ble[0] + xl[1] * ble[1] + xl[2] * ble[2];   // (zero without an observation)
    if (g.k > 0 && sub == 0) {
        c.lms_trial[3 * (size_t)g.l] = nxl; c.lms_trial[3 * (size_t)g.l + 1] = nyl; c.lms_trial[3 * (size_t)g.l + 2] = nzl;
        scale += c.lambda * (xl[0] * xl[0] + xl[1] * xl[1] + xl[2] * xl[2]);
    }
    if (has) chi += M::edge_chi(a, g.ed, c.trl, c.cache_trl, nxl, nyl, nzl);   // robust chi^2 of the observation at the trial state
}

// the landmarks [begin, end) of the list, G lanes each; the next group's operands and the descriptor after that are in flight while
// this one is worked on
template <class M, int MODE, int G, int NT, bool FIRST = false>
__device__ __forceinline__ void eval_class(const Ctx<M>& c, int begin, int end, double& chi, double& scale, double& dmax) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (begin >= end) return;
    constexpr int kStep = NT / G;
    GroupIn<M> nx = load_group<M, G, FIRST>(c, load_desc(c, begin + tid / G, end), lane, begin + tid / G);
    int4 d2 = load_desc(c, begin + kStep + tid / G, end);
    for (int i0 = begin; i0 < end; i0 += kStep) {
        const GroupIn<M> g = nx;
        nx = load_group<M, G, FIRST>(c, d2, lane, i0 + kStep + tid / G);
        d2 = load_desc(c, i0 + 2 * kStep + tid / G, end);
        eval_group<M, MODE, G>(c, g, lane, chi, scale, dmax);
    }
}
// one pass over all four classes: landmarks with 1-4 observations take 4 lanes, 5-8 take 8, 9-16 take 16, the rest a wave
template <class M, int MODE, int NT, bool FIRST = false>
__device__ __forceinline__ void eval_pass(const Ctx<M>& c, const int (&cls)[5], double& chi, double& scale, double& dmax) {
    eval_class<M, MODE, 4, NT, FIRST>(c, cls[0], cls[1], chi, scale, dmax);
    eval_class<M, MODE, 8, NT, FIRST>(c, cls[1], cls[2], chi, scale, dmax);
    eval_class<M, MODE, 16, NT, FIRST>(c, cls[2], cls[3], chi, scale, dmax);
    eval_class<M, MODE, 64, NT, FIRST>(c, cls[3], cls[4], chi, scale, dmax);
}
// landmarks without an observation keep their place: their trial position is their position
template <class M, int NT>
__device__ __forceinline__ void copy_unobserved(const Ctx<M>& c, int end) {
    for (int i = threadIdx.x; i < end; i += NT) {
        const int l = c.desc[i].x;
#pragma unroll
        for (int m = 0; m < 3; ++m) c.lms_trial[3 * (size_t)l + m] = c.lms[3 * (size_t)l + m];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// BUILD of one landmark
// ------------------------------------------------------------------------------------------------------------------
// The pair products of the landmark's observations: every lane puts W_e (B x 3) and its column into the wave's strip, lane i then
// takes the partners (i + s) mod k, s = 1 .. k / 2 (the pairs at distance k / 2 of an even k only from the lower half)
template <class M, int G>
__device__ __forceinline__ void pair_products(const Ctx<M>& c, int k, bool has, int lane, int c0, const double (&Wm)[3 * M::B]) {
    constexpr int B = M::B, kStage = 3 * B + 1;
    const int sub = lane & (G - 1);
    const bool fr = c0 >= 0;
    double* mine = c.stage + lane * kStage;   // (32-bit index arithmetic: LDS)
#pragma unroll
    for (int i = 0; i < 3 * B; ++i) mine[i] = Wm[i];
    mine[3 * B] = (double)c0;
    // (the strip is this wave's alone and a wave's LDS operations execute in the order they were issued: what the other lanes wrote
    // is there when the reads below arrive - only the compiler has to keep the order)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const int half = k >> 1;
    int smax = half;
#pragma unroll
    for (int m = G; m < 64; m <<= 1) smax = max(smax, __shfl_xor(smax, m));   // the wave's longest landmark sets the trip count
    const int gbase = lane & ~(G - 1);
    // (requesting the partner of step s + 1 before the atomics of step s go out - so that its products run while those drain - was
    // measured on the SE(2) kernel and is slower: 406 k against 414 k LM it/s at 256 windows; ten more live registers per lane)
    for (int s = 1; s <= smax; ++s) {
        const bool act = has && s <= half && !(2 * s == k && sub >= half);
        int j = sub + s;
        if (j >= k) j -= k;
        const double* his = c.stage + (gbase + (act ? j : sub)) * kStage;
        double Wp[3 * B];
#pragma unroll
        for (int i = 0; i < 3 * B; ++i) Wp[i] = his[i];
        const int cp = (int)his[3 * B];
        if (act && fr && cp >= 0) {
            // block (mine, his) of S loses W_mine W_his^T; it is stored where row > column.  (Two observations of one landmark by
            // the SAME key frame - the reference never builds that - land in the pose's own block: P + P^T, lower triangle.)
            // One multiplication for the block's place - the first of its B rows, the others follow by additions - and one
            // select per entry between "my rows, his columns" and the transposed place.
            const bool lower = c0 > cp, same = c0 == cp;
            const int hi = lower ? c0 : cp, lo = lower ? cp : c0;
            int rb[B];
            rb[0] = tri(hi, lo);
#pragma unroll
            for (int r = 1; r < B; ++r) rb[r] = rb[r - 1] + hi + r;
#pragma unroll
            for (int r = 0; r < B; ++r)
#pragma unroll
                for (int m = 0; m < B; ++m) {
                    double pr = Wm[r * 3] * Wp[m * 3] + Wm[r * 3 + 1] * Wp[m * 3 + 1] + Wm[r * 3 + 2] * Wp[m * 3 + 2];
                    int at = rb[r] + m;                                   // r == m: the same place either way
                    if (r > m) at = (lower || same) ? rb[r] + m : rb[m] + r;
                    if (r < m) at = lower ? rb[r] + m : rb[m] + r;        // (same: not lower, row m = max(r, m))
                    if (r == m && same) pr *= 2.0;
                    lds_add(c.S + at, -pr);
                }
        }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();   // (the next landmark's strip writes stay behind these reads)
    asm volatile("" ::: "memory");
}

template <class M, int G>
__device__ __forceinline__ void build_group(const Ctx<M>& c, const GroupIn<M>& g, int lane) {
    const typename M::Args& a = *c.a;
    const int sub = lane & (G - 1);
    const int c0 = g.has ? c.col[g.ed.kf] : -1;
    typename M::Lin lin;
    double hll[6], b[3];
    M::linearize(c, g, lin, hll, b);
    if (!g.has) {   // (its arithmetic ran on a made-up edge and may hold infinities: nothing of it may reach the group's sums)
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
    if (g.k > 0 && sub == 0) {   // the update pass of this trial takes the factor from here instead of summing Hll and factorising it again
        double2* dst = reinterpret_cast<double2*>(a.ainv + 6 * (size_t)g.at);
        dst[0] = double2{A[0], A[1]}; dst[1] = double2{A[2], A[3]}; dst[2] = double2{A[4], A[5]};
    }
    zt[0] = A[0] * b[0];
    zt[1] = A[1] * b[0] + A[2] * b[1];
    zt[2] = A[3] * b[0] + A[4] * b[1] + A[5] * b[2];
    double Wm[3 * M::B];
    M::pose_block(c, lin, c0, A, zt, Wm);
    pair_products<M, G>(c, g.k, g.has, lane, c0, Wm);
}

// the landmarks [begin, end) of the list, G lanes each; the next group's operands and the descriptor after that are in flight while
// this one is worked on
template <class M, int G, int NT>
__device__ __forceinline__ void build_class(const Ctx<M>& c, int begin, int end) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (begin >= end) return;
    constexpr int kStep = NT / G;
    GroupIn<M> nx = load_group<M, G>(c, load_desc(c, begin + tid / G, end), lane, begin + tid / G);
    int4 d2 = load_desc(c, begin + kStep + tid / G, end);
    for (int i0 = begin; i0 < end; i0 += kStep) {
        const GroupIn<M> g = nx;
        nx = load_group<M, G>(c, d2, lane, i0 + kStep + tid / G);
        d2 = load_desc(c, i0 + 2 * kStep + tid / G, end);
        build_group<M, G>(c, g, lane);
    }
}

// LL^T of the augmented system in place, block column by block column (M::factor_column): LPB lanes share a block's sum over the
// columns to its left - 8 while the column is long, up to 64 near the end, where few rows are left and the sum is longest
template <class M, int NT>
__device__ __forceinline__ void factorize(double* S, double* invd, double* tjj, int nf, int* fail) {
    for (int J = 0; J < nf; ++J) {
        const int blocks = nf - J + 1;
        if (blocks * 64 <= NT) M::template factor_column<NT, 64>(S, invd, tjj, nf, J, fail);
        else if (blocks * 32 <= NT) M::template factor_column<NT, 32>(S, invd, tjj, nf, J, fail);
        else if (blocks * 16 <= NT) M::template factor_column<NT, 16>(S, invd, tjj, nf, J, fail);
        else M::template factor_column<NT, 8>(S, invd, tjj, nf, J, fail);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// the kernel: workgroup blockIdx.x of NT threads runs optimize(a.iters) of its window
// ------------------------------------------------------------------------------------------------------------------
// The kernel's static LDS: the controller block, the flags, the counts and their lists, the reduction scratch, the T(J, J) strip.
// The __global__ wrapper declares it and hands it in.  (Declared as __shared__ variables inside window_lm - a device function, though
// inlined - the compiler no longer folds their addresses: the SE(2) kernels then spill 165 SGPRs instead of 147 and hold 228 VGPRs
// instead of 226.)
template <int B>
struct WindowShared {
    BaCtl ctl;
    int s_nf, s_fail, s_err, s_stop;
    int hist[kWindowMaxDegree + 2], wtot[18][8], rstart[18];
    double red[24], tjj[B * (B + 1) / 2];
};
template <class M, int NT>
__device__ __forceinline__ void window_lm(const typename M::Args& a, WindowShared<M::B>& sh) {
    constexpr int B = M::B, kPose = M::kPose, kCache = M::kCache, kStage = 3 * B + 1;
    extern __shared__ double lds[];
    BaCtl& ctl = sh.ctl;
    int &s_nf = sh.s_nf, &s_fail = sh.s_fail, &s_err = sh.s_err, &s_stop = sh.s_stop;
    int (&hist)[kWindowMaxDegree + 2] = sh.hist; int (&wtot)[18][8] = sh.wtot; int (&rstart)[18] = sh.rstart;
    double (&red)[24] = sh.red; double (&tjj)[B * (B + 1) / 2] = sh.tjj;
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
    // LDS map (doubles): col P ints | cur kPose P | trl kPose P | cache_cur kCache P | cache_trl kCache P | x n | invd n |
    // stage NT x (3 B + 1) | S (n + B)(n + B + 1) / 2     (window_lds_bytes below counts the same)
    int* col = reinterpret_cast<int*>(lds);
    double* bufA = lds + (P + 1) / 2;
    double* bufB = bufA + kPose * P;
    double* cacheA = bufB + kPose * P;
    double* cacheB = cacheA + kCache * P;
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int p = 0; p < P; ++p) col[p] = a.fixed[p] ? -1 : B * cnt++;
        s_nf = cnt;
    }
    {
        const double* src = ctl.sel ? a.poses_b : a.poses_a;
        for (int i = tid; i < kPose * P; i += NT) bufA[i] = src[i];
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
    const bool refused = s_err != 0;   // a landmark this kernel does not take: nothing is touched, the caller runs the window elsewhere
    if (!refused) {
        // the list: the landmarks by their number of observations (0, 1, ... 16, more), STABLE inside a count, so that the groups of
        // a wave are alike (the longest landmark of a wave sets the trip count of its pair loop) and consecutive groups read
        // ascending addresses of the edge arrays (a list in arbitrary order inside a count fetched every cache line of the edges
        // about twice: PMC, profiles/r06h).  Rounds of NT landmarks; a landmark's place = its count's start + the members before
        // it (ballot ranks inside the wave, wave totals through LDS, the rounds' totals in registers).
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
                // (all landmarks of a count below 17 have that many records: the place of a landmark's first one follows from its own)
                a.desc[at] = make_int4(l, cls < kBuckets - 1 ? rstart[cls] + (at - hist[cls]) * k : beg, k, beg);
            }
#pragma unroll
            for (int b = 0; b < kBuckets; ++b)
                for (int w = 0; w < NT / 64; ++w) next[b] += wtot[b][w];
            __syncthreads();
        }
    }
    if (a.stamps && tid == 0) a.stamps[6] = wall_clock64();   // (the list is made)
    const int nf = s_nf, n = B * nf;
    double* xs = cacheB + kCache * P;
    double* invd = xs + n;
    double* stage_all = invd + n;
    double* S = stage_all + (size_t)NT * kStage;
    const int ntri = (n + B) * (n + B + 1) / 2;   // rows 0 .. n-1 = S, row n = b_s, B - 1 rows of zeros (the factorisation's last block row)
    if constexpr (kCache > 0)
        for (int p = tid; p < P; p += NT) M::cache_pose(bufA + kPose * p, cacheA + kCache * p);
    if (refused && tid == 0) { ctl.error = 2; ctl.done = 1; }
    __syncthreads();
    // classes of the passes: landmarks with 1-4 observations take 4 lanes, 5-8 take 8, 9-16 take 16, the rest a wave
    const int cls[5] = {hist[1], hist[5], hist[9], hist[17], L};

    Ctx<M> c;
    c.a = &a;
    c.S = S;
    c.x = xs;
    c.cur = bufA; c.cache_cur = cacheA; c.trl = bufB; c.cache_trl = cacheB;
    c.col = col;
    c.stage = stage_all + (size_t)wave * 64 * kStage;
    c.lms = ctl.sel ? a.lms_b : a.lms_a;
    c.lms_trial = ctl.sel ? a.lms_a : a.lms_b;
    c.desc = a.desc;
    c.rec = M::records(a.desc + L, (size_t)a.E);   // the record arrays lie behind the list (the caller has checked the room: ba_resident_ok)
    c.n = n;
    c.lambda = 0.0;
    double* cur = bufA;
    double* trl = bufB;
    double* cache_cur = cacheA;
    double* cache_trl = cacheB;

    // ---- the opening pass: chi^2 of the starting state (computeActiveErrors + activeRobustChi2 in front of the first iteration),
    // for Levenberg-Marquardt together with the diagonal of the first linearisation (lambda_0 = 1e-5 max diag H, computeLambdaInit;
    // Gauss-Newton keeps lambda = 0) - and on the way the observations go into the ORDER OF THE LIST.  The passes visit the landmarks
    // class by class; in the caller's arrays a class's landmarks alternate with the others', and every cache line of the edge arrays
    // came in once PER CLASS that has a landmark in it (PMC, profiles/r06k: 6.6 MB per window and iteration for 3.0 MB of operands).
    // One gapped read here, and every pass of every trial reads whole lines.
    if (!refused) {
        const bool lm = a.mode == SE2GPU_BA_LM;
        for (int i = tid; i < n; i += NT) xs[i] = 0.0;
        __syncthreads();
        double chi = 0, sc = 0, dm = 0;
        if (lm) {
            eval_pass<M, kDiag, NT, true>(c, cls, chi, sc, dm);
            M::template pose_terms<kDiag, NT>(c, chi, sc);
        } else {
            eval_pass<M, kEval, NT, true>(c, cls, chi, sc, dm);
            M::template pose_terms<kEval, NT>(c, chi, sc);
        }
        __syncthreads();   // (the diagonal's atomics have landed; the records are written)
        if (lm)
            for (int i = tid; i < n; i += NT) dm = fmax(dm, fabs(xs[i]));
        wg_reduce<NT>(red, chi, sc, dm);
        if (tid == 0) {
            lm_begin(&ctl, chi, s_stop != 0);
            if (lm && !ctl.done) { ctl.lambda = 1e-5 * dm; ctl.ni = 2; }
        }
        __syncthreads();
    }
    long long* stamps = a.stamps;
    if (stamps && tid == 0) stamps[7] = wall_clock64();       // (the opening pass)
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
            build_class<M, 4, NT>(c, cls[0], cls[1]);
            build_class<M, 8, NT>(c, cls[1], cls[2]);
            build_class<M, 16, NT>(c, cls[2], cls[3]);
            build_class<M, 64, NT>(c, cls[3], cls[4]);
            M::template pose_terms<kBuild, NT>(c, chi, sc);
        }
        __syncthreads();
        for (int i = tid; i < n; i += NT) S[tri(i, i)] += lambda;      // setLambda: the damping on the pose diagonal (the landmarks' went into A)
        __syncthreads();
        if (stamps && tid == 0) stamps[1] = wall_clock64();
        factorize<M, NT>(S, invd, tjj, nf, &s_fail);
        if (stamps && tid == 0) stamps[2] = wall_clock64();
        if (wave == 0) M::back_substitute(S, invd, nf, xs);
        __syncthreads();
        if (stamps && tid == 0) stamps[3] = wall_clock64();
        // ---- oplus into the trial state (fixed poses copied)
        double chi = 0, sc = 0, dm = 0;
        for (int p = tid; p < P; p += NT) M::oplus(cur + kPose * p, col[p], xs, lambda, trl + kPose * p, cache_trl + kCache * p, sc);
        __syncthreads();
        copy_unobserved<M, NT>(c, cls[0]);
        eval_pass<M, kUpdate, NT>(c, cls, chi, sc, dm);
        M::template pose_terms<kUpdate, NT>(c, chi, sc);
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
            t = cache_cur; cache_cur = cache_trl; cache_trl = t;
            c.cur = cur; c.cache_cur = cache_cur; c.trl = trl; c.cache_trl = cache_trl;
            const double* tl = c.lms; c.lms = c.lms_trial; c.lms_trial = const_cast<double*>(tl);
        }
        __syncthreads();
    }

    // ---- epilogue: the estimate's poses to the buffer the controller names, the block to the handle and its mailbox
    if (!refused) {
        double* dst = ctl.sel ? a.poses_b : a.poses_a;
        for (int i = tid; i < kPose * P; i += NT) dst[i] = cur[i];
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

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
// dynamic LDS of a window of P poses, nfree of them free, with `threads` threads: the map of window_lm (0: the window does not fit)
template <class M>
size_t window_lds_bytes(int P, int nfree, int threads) {
    constexpr size_t B = M::B;
    const size_t n = B * (size_t)nfree;
    const size_t doubles = (size_t)(P + 1) / 2 + 2 * (size_t)(M::kPose + M::kCache) * (size_t)P + 2 * n +
                           (size_t)threads * (3 * B + 1) + (n + B) * (n + B + 1) / 2;
    const size_t bytes = doubles * 8;
    // static LDS of the kernel: the controller block, the counts and their lists, the reduction scratch, the T(J, J) strip
    const size_t fixed = sizeof(BaCtl) + M::kStaticInts * sizeof(int) + (24 + B * (B + 1) / 2) * 8 + 128;
    if (n > 192 || bytes + fixed > 160 * 1024) return 0;   // (192: back_substitute keeps three unknowns per lane of one wave)
    return bytes;
}

// one launch of `count` workgroups of a kernel instantiation; its dynamic-LDS limit is raised when a launch needs more than any before
template <auto Kernel, int NT, class Args>
int window_launch(const Args* d_args, int count, size_t lds_bytes, hipStream_t st) {
    static size_t allowed = 0;   // (grown under the caller's lock: se2gpu_ba_optimize_batch serialises its resident launches)
    if (lds_bytes > allowed) {
        SE2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        allowed = lds_bytes;
    }
    hipLaunchKernelGGL(Kernel, dim3(count), dim3(NT), lds_bytes, st, d_args);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // namespace
