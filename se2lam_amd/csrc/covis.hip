// libse2gpu - covisibility on gfx950 (MI355X): Map::compareViewMPs (src/Map.cpp:354-400 of the reference, both overloads)
// for batches of key-frame pairs and of key frames against reference sets, on the observation CSR in device memory.
//   k_covis_scatter   one thread per map point: the bit (f, p) of every valid entry of the point's list (64-bit atomicOr), and
//                     the two point rows "not null" and "not null and good parallax" by ballot, one word per wave
//   k_covis_rowcount  one wave per key frame: KeyFrame::getSizeObsMP() = the popcount of its row
//   k_covis_pairs     one wave per pair: nSameMP, the two sizes, the two ratios (:367-368), the tests of
//                     Map::updateCovisibility (:794) and Localizer::UpdateCovisKFCurr (Localizer.cpp:683), and spMPs in ascending
//                     point order by an exclusive prefix sum of the lanes' popcounts - no atomics, the same list in every run
//   k_covis_refset    one wave per job: the points of a key frame seen by at least k of the listed reference frames, counted in
//                     a bit-sliced saturating counter of three planes held in registers (:381-396)
// d_bits is (nframes + 2) rows of W = ceil(m / 64) 64-bit words: row f < nframes = the observation set of key frame slot f, row
// nframes = point is not null, row nframes + 1 = not null and good parallax.  Bits past m are zero in every row.
// A thread per point and not per CSR entry: d_mp_ptr is clamped and its segments need not ascend or be disjoint, so an entry has
// no single owner to search for.  Integer atomics only; every index read from an array is checked before it is used, the
// observation lists by obs_table.h's entry and segment rule (a null key frame is not skipped: compareViewMPs does not).
// Compiled with -ffp-contract=off: the ratios and the threshold tests are single IEEE operations.
#include "common.h"
#include "obs_table.h"
#include "wave_int.h"

using namespace se2gpu;

namespace {

typedef unsigned long long u64;

constexpr int MAX_WAVES = (1 << 26) - 1;   // one 64-thread block per pair / job; a launch's threads stay below 2^32

struct CsrArgs {
    const int* counts;
    const int* mp_ptr;
    const int* obs_frame;
    const int* obs_ftr;
    int cap, nframes, m, nobs;
    // no frame_null: compareViewMPs does not skip a null key frame, and the rule's test folds away
    __device__ __forceinline__ FrameSlots slots() const { return FrameSlots{counts, nullptr, cap, nframes}; }
    __device__ __forceinline__ ObsCsr csr() const { return ObsCsr{mp_ptr, obs_frame, obs_ftr, m, nobs}; }
};

__global__ __launch_bounds__(256) void k_covis_scatter(CsrArgs c, const uint8_t* mp_null, const uint8_t* good_prl, u64* bits,
                                                       int W) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool in = p < c.m;
    const bool notnull = in && !(mp_null && mp_null[p]);
    const bool good = notnull && (!good_prl || good_prl[p]);
    if (in) {
        const FrameSlots fs = c.slots();
        int s, e;
        point_range(c.csr(), p, s, e);
        const u64 bit = 1ull << (p & 63);
        for (int i = s; i < e; ++i) {
            const int f = c.obs_frame[i];
            if (entry_valid(fs, f, c.obs_ftr[i])) atomicOr(&bits[(size_t)f * W + (p >> 6)], bit);
        }
    }
    const u64 bn = __ballot(notnull), bg = __ballot(good);
    const int word = p >> 6;                                           // the same for the 64 lanes of a wave
    if ((threadIdx.x & 63) == 0 && word < W) {
        bits[(size_t)c.nframes * W + word] = bn;
        bits[(size_t)(c.nframes + 1) * W + word] = bg;
    }
}

__global__ __launch_bounds__(64) void k_covis_rowcount(const u64* bits, int W, int* size_obs) {
    const u64* row = bits + (size_t)blockIdx.x * W;
    int n = 0;
    for (int w = threadIdx.x; w < W; w += 64) n += __popcll(row[w]);
    n = wave_sum(n);
    if (threadIdx.x == 0) size_obs[blockIdx.x] = n;
}

struct PairArgs {
    CsrArgs c;                  // read for the list only
    const u64* bits;
    const int* pair_a;
    const int* pair_b;
    int* out;
    float* ratio;
    int* common;
    int W, list_cap;
    float ratio_f;
    double ratio_d;
};

__global__ __launch_bounds__(64) void k_covis_pairs(PairArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int fa = a.pair_a[p], fb = a.pair_b[p];
    const int nframes = a.c.nframes, W = a.W;
    const FrameSlots fs = a.c.slots();
    int* out = a.out + 4 * (size_t)p;
    if ((unsigned)fa >= (unsigned)nframes || (unsigned)fb >= (unsigned)nframes) {
        if (lane == 0) { out[0] = -1; out[1] = 0; out[2] = 0; out[3] = 0; }
        return;
    }
    const u64* ra = a.bits + (size_t)fa * W;
    const u64* rb = a.bits + (size_t)fb * W;
    const u64* rn = a.bits + (size_t)nframes * W;
    int* list = a.common + 3 * (size_t)p * a.list_cap;                 // not dereferenced with list_cap == 0
    int na = 0, nb = 0, same = 0, base = 0;                            // base: common points of the chunks before this one
    for (int w0 = 0; w0 < W; w0 += 64) {                               // uniform trip count: the shuffles see all 64 lanes
        const int w = w0 + lane;
        u64 A = 0, B = 0, N = 0;
        if (w < W) { A = ra[w]; B = rb[w]; N = rn[w]; }
        u64 x = A & B & N;                                             // getAllObsMPs(false) drops the null points (:358)
        const int pc = __popcll(x);
        na += __popcll(A);
        nb += __popcll(B);
        same += pc;
        if (base < a.list_cap) {                                       // uniform
            const int incl = wave_scan_incl(pc);
            int at = base + incl - pc;                                 // exclusive prefix: this lane's first place in the list
            base += wave_last(incl);
            while (x && at < a.list_cap) {
                const int pt = 64 * w + __ffsll((long long)x) - 1;
                x &= x - 1;
                int ea = -1, eb = -1;                                  // the first valid entry of either frame
                int s = 0, e = 0;
                if (pt < a.c.m) point_range(a.c.csr(), pt, s, e);     // (a d_bits of this m has no bit past it)
                for (int i = s; i < e; ++i) {
                    const int f = a.c.obs_frame[i];
                    if ((f != fa && f != fb) || !entry_valid(fs, f, a.c.obs_ftr[i])) continue;
                    if (f == fa && ea < 0) ea = i;
                    if (f == fb && eb < 0) eb = i;
                }
                list[3 * (size_t)at] = pt;
                list[3 * (size_t)at + 1] = ea;
                list[3 * (size_t)at + 2] = eb;
                ++at;
            }
        }
    }
    na = wave_sum(na);
    nb = wave_sum(nb);
    same = wave_sum(same);
    if (lane == 0) {
        int flags = 0;
        if ((float)same > a.ratio_f * (float)na) flags |= 1;           // Map.cpp:794
        if ((double)same > a.ratio_d * (double)na) flags |= 2;         // Localizer.cpp:683
        out[0] = same; out[1] = na; out[2] = nb; out[3] = flags;
        a.ratio[2 * (size_t)p] = (float)same / (float)na;              // :367-368; 0 / 0 is NaN there too
        a.ratio[2 * (size_t)p + 1] = (float)same / (float)nb;
    }
}

struct RefArgs {
    const u64* bits;
    const int* job_kf;
    const int* ref_ptr;
    const int* ref_idx;
    int* out;
    double* ratio;
    int W, nframes, nref, k;
    double thresh;
};

__global__ __launch_bounds__(64) void k_covis_refset(RefArgs a) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int kf = a.job_kf[j], W = a.W;
    int* out = a.out + 3 * (size_t)j;
    if ((unsigned)kf >= (unsigned)a.nframes) {
        if (lane == 0) { out[0] = -1; out[1] = 0; out[2] = 0; }
        return;
    }
    const int s = min(max(a.ref_ptr[j], 0), a.nref), e = min(max(a.ref_ptr[j + 1], 0), a.nref);
    const u64* rk = a.bits + (size_t)kf * W;
    const u64* rg = a.bits + (size_t)(a.nframes + 1) * W;              // getAllObsMPs() checks the parallax (:376, KeyFrame.h:69)
    const u64 k0 = (a.k & 1) ? ~0ull : 0ull, k1 = (a.k & 2) ? ~0ull : 0ull, k2 = (a.k & 4) ? ~0ull : 0ull;
    int all = 0, cnt = 0;
    for (int w = lane; w < W; w += 64) {
        const u64 mine = rk[w] & rg[w];
        all += __popcll(mine);
        u64 c0 = 0, c1 = 0, c2 = 0;                                    // per point: references that see it, saturating at 7
        for (int r = s; r < e; ++r) {
            const int f = a.ref_idx[r];
            if ((unsigned)f >= (unsigned)a.nframes) continue;
            const u64 x = a.bits[(size_t)f * W + w] & mine;
            const u64 t0 = c0 & x;
            c0 ^= x;
            const u64 t1 = c1 & t0;
            c1 ^= t0;
            const u64 t2 = c2 & t1;
            c2 ^= t1;
            c0 |= t2; c1 |= t2; c2 |= t2;                              // 7 + 1 stays 7
        }
        u64 gt = 0, eq = ~0ull;                                        // count >= k, from the top plane down
        gt |= eq & c2 & ~k2; eq &= ~(c2 ^ k2);
        gt |= eq & c1 & ~k1; eq &= ~(c1 ^ k1);
        gt |= eq & c0 & ~k0; eq &= ~(c0 ^ k0);
        cnt += __popcll((gt | eq) & mine);
    }
    all = wave_sum(all);
    cnt = wave_sum(cnt);
    if (lane == 0) {
        const double r = all == 0 ? -1.0 : (double)cnt * 1.0 / (double)all;   // :377-379, :398
        out[0] = cnt; out[1] = all; out[2] = (all != 0 && r >= a.thresh) ? 1 : 0;   // Map.cpp:196
        a.ratio[j] = r;
    }
}

long long words_of(int m) { return ((long long)m + 63) / 64; }

int check_bits(const char* who, int nframes, int m) {
    SE2_REQUIRE(nframes >= 1, SE2GPU_ERR_INVALID, "%s: nframes = %d is below 1", who, nframes);
    SE2_REQUIRE(m >= 0, SE2GPU_ERR_INVALID, "%s: m = %d is negative", who, m);
    SE2_REQUIRE(((long long)nframes + 2) * words_of(m) <= INT_MAX, SE2GPU_ERR_CAPACITY,
                "%s: (nframes + 2) * ceil(m / 64) = %lld words of d_bits exceed the limit %d", who,
                ((long long)nframes + 2) * words_of(m), INT_MAX);
    return SE2GPU_OK;
}

}  // namespace

extern "C" long long se2gpu_covis_bits_words(int nframes, int m) {
    if (nframes < 1 || m < 0) return -1;
    return ((long long)nframes + 2) * words_of(m);
}

extern "C" int se2gpu_covis_build_device(se2gpu_matcher* h, const int32_t* d_counts, int cap, int nframes,
                                         const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr, int m,
                                         int nobs, const uint8_t* d_mp_null, const uint8_t* d_good_prl, uint64_t* d_bits,
                                         int32_t* d_size_obs) {
    const char* who = "covis_build";
    SE2_NEED(h);
    SE2_CHECK(check_bits(who, nframes, m));
    SE2_CHECK(check_obs_csr(who, d_mp_ptr, d_obs_frame, d_obs_ftr, m, nobs));
    SE2_CHECK(check_frame_slots(who, d_counts, cap, nframes));
    SE2_NEED(d_bits); SE2_NEED(d_size_obs);
    if (m == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    const int W = (int)words_of(m);
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    SE2_HIP(hipMemsetAsync(d_bits, 0, (size_t)nframes * W * sizeof(u64), st));   // the two point rows are written whole
    const CsrArgs c{d_counts, d_mp_ptr, d_obs_frame, d_obs_ftr, cap, nframes, m, nobs};
    hipLaunchKernelGGL(k_covis_scatter, dim3(((unsigned)m + 255u) / 256u), dim3(256), 0, st, c, d_mp_null, d_good_prl,
                       (u64*)d_bits, W);
    hipLaunchKernelGGL(k_covis_rowcount, dim3((unsigned)nframes), dim3(64), 0, st, (const u64*)d_bits, W, d_size_obs);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

extern "C" int se2gpu_covis_pairs_device(se2gpu_matcher* h, const uint64_t* d_bits, int nframes, int m, const int32_t* d_pair_a,
                                         const int32_t* d_pair_b, int npairs, float ratio_f, double ratio_d, int32_t* d_pair_out,
                                         float* d_pair_ratio, int32_t* d_common, int list_cap, const int32_t* d_counts, int cap,
                                         const int32_t* d_mp_ptr, const int32_t* d_obs_frame, const int32_t* d_obs_ftr,
                                         int nobs) {
    const char* who = "covis_pairs";
    SE2_NEED(h);
    SE2_CHECK(check_bits(who, nframes, m));
    SE2_NEED(d_bits); SE2_NEED(d_pair_a); SE2_NEED(d_pair_b); SE2_NEED(d_pair_out); SE2_NEED(d_pair_ratio);
    SE2_REQUIRE(npairs >= 0, SE2GPU_ERR_INVALID, "%s: npairs = %d is negative", who, npairs);
    SE2_REQUIRE(list_cap >= 0, SE2GPU_ERR_INVALID, "%s: list_cap = %d is negative", who, list_cap);
    if (d_common) SE2_CHECK(check_obs_csr(who, d_mp_ptr, d_obs_frame, d_obs_ftr, m, nobs));   // without a list the table is not read
    if (d_common) SE2_CHECK(check_frame_slots(who, d_counts, cap, nframes));
    SE2_REQUIRE(npairs <= MAX_WAVES, SE2GPU_ERR_CAPACITY, "%s: npairs = %d exceeds the limit %d", who, npairs, MAX_WAVES);
    if (npairs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    PairArgs a;
    a.c = CsrArgs{d_counts, d_mp_ptr, d_obs_frame, d_obs_ftr, cap, nframes, m, nobs};
    a.bits = (const u64*)d_bits; a.pair_a = d_pair_a; a.pair_b = d_pair_b; a.out = d_pair_out; a.ratio = d_pair_ratio;
    a.common = d_common; a.W = (int)words_of(m); a.list_cap = d_common ? list_cap : 0;
    a.ratio_f = ratio_f; a.ratio_d = ratio_d;
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    hipLaunchKernelGGL(k_covis_pairs, dim3((unsigned)npairs), dim3(64), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

extern "C" int se2gpu_covis_refset_device(se2gpu_matcher* h, const uint64_t* d_bits, int nframes, int m, const int32_t* d_job_kf,
                                          const int32_t* d_ref_ptr, const int32_t* d_ref_idx, int nref, int njobs, int k,
                                          double thresh, int32_t* d_job_out, double* d_job_ratio) {
    const char* who = "covis_refset";
    SE2_NEED(h);
    SE2_CHECK(check_bits(who, nframes, m));
    SE2_NEED(d_bits); SE2_NEED(d_job_kf); SE2_NEED(d_ref_ptr); SE2_NEED(d_job_out); SE2_NEED(d_job_ratio);
    SE2_REQUIRE(njobs >= 0, SE2GPU_ERR_INVALID, "%s: njobs = %d is negative", who, njobs);
    SE2_REQUIRE(nref >= 0, SE2GPU_ERR_INVALID, "%s: nref = %d is negative", who, nref);
    SE2_REQUIRE(nref == 0 || d_ref_idx, SE2GPU_ERR_INVALID, "%s: d_ref_idx is NULL with nref = %d", who, nref);
    SE2_REQUIRE(k >= 1 && k <= 7, SE2GPU_ERR_CAPACITY, "%s: k = %d is outside 1..7 (three counter planes)", who, k);
    SE2_REQUIRE(njobs <= MAX_WAVES, SE2GPU_ERR_CAPACITY, "%s: njobs = %d exceeds the limit %d", who, njobs, MAX_WAVES);
    if (njobs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    RefArgs a;
    a.bits = (const u64*)d_bits; a.job_kf = d_job_kf; a.ref_ptr = d_ref_ptr; a.ref_idx = d_ref_idx; a.out = d_job_out;
    a.ratio = d_job_ratio; a.W = (int)words_of(m); a.nframes = nframes; a.nref = nref; a.k = k; a.thresh = thresh;
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    hipLaunchKernelGGL(k_covis_refset, dim3((unsigned)njobs), dim3(64), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}
