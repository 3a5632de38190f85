// libse2gpu - the local window on gfx950 (MI355X): the covisibility graph KeyFrame::mCovisibleKFs as a bit matrix in device
// memory with its upkeep, and Map::updateLocalGraph (src/Map.cpp:285-331 of the reference) for batches of current key frames.
//   k_adj_connect      one thread per pair: addCovisibleKF both ways (64-bit atomicOr), all pairs or those whose flag word
//                      se2gpu_covis_pairs_device set (Map.cpp:794-797)
//   k_adj_clear        one wave per listed slot s: the bit (b, s) of every b in row s (64-bit atomicAnd), KeyFrame.cpp:106-114
//   k_adj_zero         one wave per listed slot: its row; a launch of its own, after every k_adj_clear wave has read its row
//   k_local_window     one workgroup of 256 threads per job: the hops over d_adj with the two key-frame rows, the frontier and
//                      the compacted member list in LDS; the point row as an OR of observation rows, each thread its own
//                      words; a wave per eight candidate frames at a time for the reference test and the edge count; the three
//                      lists by a prefix sum over the workgroup in the order of the id permutations
// d_adj is nframes rows of WF = ceil(nframes / 64) 64-bit words, bit (a, b) = slot b is in slot a's mCovisibleKFs; d_bits_kf /
// d_bits_mp are the bit matrices of covis.hip, (nframes + 2) rows of W = ceil(m / 64) words.
// The hops expand the members found in the round before only, against the set as it stood at the start of the round: the
// frontier of the next round is collected in a row of its own (s_next) and merged after a barrier, so a member added in a
// round is never expanded in that same round (an in-place sweep in ascending slot order would run down a whole chain in one).
// Integers only; LDS and global integer atomics (OR / AND, order-free); every slot, order entry and tail bit is checked.
#include "common.h"
#include "wave_int.h"

using namespace se2gpu;

namespace {

typedef unsigned long long u64;

constexpr int MAX_FRAMES = SE2GPU_LOCAL_WINDOW_MAX_FRAMES;   // 4096: WF <= 64 words, one per lane of a wave
constexpr int MAX_WF = MAX_FRAMES / 64;
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int FRAMES = 8;                                    // candidate frames a wave tests at a time
constexpr int EMIT = 4;                                      // order entries a thread takes per barrier of a list
constexpr int MAX_BLOCKS = (1 << 24) - 1;                    // 256 threads each; a launch's threads stay below 2^32
constexpr int MAX_PAIRS = INT_MAX - 255;                     // the grid of k_adj_connect is computed in unsigned

// the bits of word w that name an index below n
__device__ __forceinline__ u64 tail_mask(int w, int n) {
    const int left = n - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

__global__ __launch_bounds__(BLOCK) void k_adj_connect(u64* adj, int nframes, int WF, const int* pair_a, const int* pair_b, int npairs,
                                                       const int* pair_out, int flag_mask) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= npairs) return;
    const int a = pair_a[p], b = pair_b[p];
    if ((unsigned)a >= (unsigned)nframes || (unsigned)b >= (unsigned)nframes) return;
    if (pair_out && !(pair_out[4 * (size_t)p + 3] & flag_mask)) return;
    atomicOr(&adj[(size_t)a * WF + (b >> 6)], 1ull << (b & 63));
    atomicOr(&adj[(size_t)b * WF + (a >> 6)], 1ull << (a & 63));
}

__global__ __launch_bounds__(64) void k_adj_clear(u64* adj, int nframes, int WF, const int* slots) {
    const int s = slots[blockIdx.x], lane = threadIdx.x;
    if ((unsigned)s >= (unsigned)nframes) return;
    const u64 clear = ~(1ull << (s & 63));
    for (int w = lane; w < WF; w += 64) {
        u64 x = adj[(size_t)s * WF + w] & tail_mask(w, nframes);
        while (x) {
            const int b = 64 * w + __ffsll((long long)x) - 1;          // below nframes by the mask
            x &= x - 1;
            atomicAnd(&adj[(size_t)b * WF + (s >> 6)], clear);
        }
    }
}

__global__ __launch_bounds__(64) void k_adj_zero(u64* adj, int nframes, int WF, const int* slots) {
    const int s = slots[blockIdx.x], lane = threadIdx.x;
    if ((unsigned)s >= (unsigned)nframes) return;
    for (int w = lane; w < WF; w += 64) adj[(size_t)s * WF + w] = 0;
}

struct WindowArgs {
    const u64* bits_kf;
    const u64* bits_mp;
    const u64* adj;
    const uint8_t* frame_null;
    const int* job_kf;
    const int* kf_order;
    const int* mp_order;
    u64* win_kf;
    u64* win_mp;
    int* win_out;
    int* local_list;
    int* ref_list;
    int* mp_list;
    int nframes, m, W, WF, search_level, kf_list_cap, mp_list_cap;
};

// The set bits of row[0..WF) as ascending indices in list[]; returns their number.  Called by the first wave, WF <= 64 and
// the bits past nframes already masked away: an exclusive prefix sum of the lanes' popcounts gives each word its place.
__device__ __forceinline__ int compact_row(const u64* row, int WF, int* list, int lane) {
    u64 x = lane < WF ? row[lane] : 0ull;
    const int pc = __popcll(x);
    const int incl = wave_scan_incl(pc);
    int at = incl - pc;
    while (x) {
        list[at++] = 64 * lane + __ffsll((long long)x) - 1;
        x &= x - 1;
    }
    return wave_last(incl);
}

// The members of a set, given as a bit row over n indices, in ascending position of order[] (NULL: index order) into
// out[0 .. min(count, cap)).  All 256 threads call it; s_cnt is 2 x EMIT x WAVES ints of LDS.  One barrier per EMIT x 256 order
// entries: a thread takes EMIT entries 256 apart, its loads are unconditional (clamped indices) so that they are in flight
// together, and the waves' counts alternate between the two halves of s_cnt.
__device__ __forceinline__ void emit_list(const u64* row, int n, const int* order, int* out, int cap, int (*s_cnt)[EMIT * WAVES]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, buf = 0;
    for (int i0 = 0; i0 < n && base < cap; i0 += EMIT * BLOCK, buf ^= 1) {   // uniform: base is the same in every thread
        int s[EMIT];
        u64 word[EMIT], bal[EMIT];
        bool in[EMIT];
#pragma unroll
        for (int k = 0; k < EMIT; ++k) {
            const int i = i0 + k * BLOCK + tid, ic = min(i, n - 1);
            const int v = order ? order[ic] : ic;
            s[k] = i < n ? v : -1;
        }
#pragma unroll
        for (int k = 0; k < EMIT; ++k) word[k] = row[((unsigned)s[k] < (unsigned)n ? s[k] : 0) >> 6];
#pragma unroll
        for (int k = 0; k < EMIT; ++k) {
            in[k] = (unsigned)s[k] < (unsigned)n && ((word[k] >> (s[k] & 63)) & 1ull);
            bal[k] = __ballot(in[k]);
            if (lane == 0) s_cnt[buf][k * WAVES + wave] = __popcll(bal[k]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EMIT; ++k) {
            int at = base;
#pragma unroll
            for (int v = 0; v < WAVES; ++v) {
                const int c = s_cnt[buf][k * WAVES + v];
                if (v < wave) at += c;
                base += c;
            }
            at += lane_rank(bal[k]);
            if (in[k] && at < cap) out[at] = s[k];
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_local_window(WindowArgs a) {
    __shared__ u64 s_local[MAX_WF], s_ref[MAX_WF], s_front[MAX_WF], s_next[MAX_WF];
    __shared__ int s_list[MAX_FRAMES];
    __shared__ int s_n, s_cnt[2][EMIT * WAVES], s_mp[WAVES];
    __shared__ long long s_obs[WAVES];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nframes = a.nframes, W = a.W, WF = a.WF;
    const int cur = a.job_kf[j];
    int* out = a.win_out + 4 * (size_t)j;
    if ((unsigned)cur >= (unsigned)nframes) {                           // uniform
        if (tid == 0) { out[0] = -1; out[1] = 0; out[2] = 0; out[3] = 0; }
        return;
    }
    if (tid < WF) {
        const u64 b = (tid == (cur >> 6)) ? 1ull << (cur & 63) : 0ull;
        s_local[tid] = b; s_front[tid] = b; s_next[tid] = 0; s_ref[tid] = 0;
    }
    __syncthreads();
    // Map.cpp:300-308
    for (int level = 0; level < a.search_level; ++level) {
        if (wave == 0) {
            const int n = compact_row(s_front, WF, s_list, lane);
            if (lane == 0) s_n = n;
        }
        __syncthreads();
        const int total = s_n * WF;                                     // at most 4096 * 64
        for (int idx = tid; idx < total; idx += BLOCK) {
            const int f = s_list[idx / WF], w = idx - (idx / WF) * WF;
            const u64 v = a.adj[(size_t)f * WF + w] & ~s_local[w];      // s_local does not change inside a round
            if (v) atomicOr(&s_next[w], v);
        }
        __syncthreads();
        u64 found = 0;
        if (tid < WF) {
            found = s_next[tid] & tail_mask(tid, nframes);
            s_local[tid] |= found; s_front[tid] = found; s_next[tid] = 0;
        }
        if (!__syncthreads_or(found != 0)) break;                       // uniform: a round that finds nothing ends the hops
    }
    if (wave == 0) {
        const int n = compact_row(s_local, WF, s_list, lane);
        if (lane == 0) s_n = n;
    }
    __syncthreads();
    const int n_local = s_n;
    // :310-315: each thread owns the words tid, tid + 256, ...
    u64* mp_row = a.win_mp + (size_t)j * W;
    const u64* notnull = a.bits_kf + (size_t)nframes * W;
    int n_mp = 0;
    for (int w = tid; w < W; w += BLOCK) {
        u64 acc = 0;
#pragma unroll 4
        for (int i = 0; i < n_local; ++i) acc |= a.bits_kf[(size_t)s_list[i] * W + w];
        acc &= notnull[w] & tail_mask(w, a.m);
        mp_row[w] = acc;
        n_mp += __popcll(acc);
    }
    n_mp = wave_sum(n_mp);
    if (lane == 0) s_mp[wave] = n_mp;
    __syncthreads();                                                    // mp_row is read back below by other threads of this block
    // :317-326 and the edge count: one wave per frame that is not null
    // FRAMES of them at a time: a point word is loaded once and the row loads are unconditional, so they are in flight together
    long long n_obs = 0;
    for (int f0 = wave * FRAMES; f0 < nframes; f0 += WAVES * FRAMES) {
        bool on[FRAMES];                                                // uniform in the wave
        const u64* row[FRAMES];
        int c[FRAMES];
#pragma unroll
        for (int k = 0; k < FRAMES; ++k) {
            const int f = min(f0 + k, nframes - 1);                     // loads without a branch; what !on[k] counts is dropped
            on[k] = f0 + k < nframes && !(a.frame_null && a.frame_null[f]);
            row[k] = a.bits_mp + (size_t)f * W;
            c[k] = 0;
        }
        for (int w = lane; w < W; w += 64) {
            const u64 pts = mp_row[w];
#pragma unroll
            for (int k = 0; k < FRAMES; ++k) c[k] += __popcll(row[k][w] & pts);
        }
#pragma unroll
        for (int k = 0; k < FRAMES; ++k) {
            if (!on[k]) continue;
            const int f = f0 + k, n = wave_sum(c[k]);
            const bool local = (s_local[f >> 6] >> (f & 63)) & 1ull;
            if (!local && n > 0 && lane == 0) atomicOr(&s_ref[f >> 6], 1ull << (f & 63));
            n_obs += n;                                                 // a frame that is neither local nor ref has n == 0
        }
    }
    if (lane == 0) s_obs[wave] = n_obs;
    __syncthreads();
    u64* kf_rows = a.win_kf + 2 * (size_t)j * WF;
    int n_ref = 0;
    if (tid < WF) {
        kf_rows[tid] = s_local[tid];
        kf_rows[WF + tid] = s_ref[tid];
        n_ref = __popcll(s_ref[tid]);
    }
    if (wave == 0) {
        n_ref = wave_sum(n_ref);
        if (lane == 0) {
            long long obs = 0;
            int mp = 0;
            for (int v = 0; v < WAVES; ++v) { obs += s_obs[v]; mp += s_mp[v]; }
            out[0] = n_local; out[1] = n_ref; out[2] = mp; out[3] = (int)(obs > INT_MAX ? INT_MAX : obs);
        }
    }
    if (a.local_list) emit_list(s_local, nframes, a.kf_order, a.local_list + (size_t)j * a.kf_list_cap, a.kf_list_cap, s_cnt);
    __syncthreads();                                                    // s_cnt is taken up again
    if (a.ref_list) emit_list(s_ref, nframes, a.kf_order, a.ref_list + (size_t)j * a.kf_list_cap, a.kf_list_cap, s_cnt);
    __syncthreads();
    if (a.mp_list) emit_list(mp_row, a.m, a.mp_order, a.mp_list + (size_t)j * a.mp_list_cap, a.mp_list_cap, s_cnt);
}

long long words_of(int n) { return ((long long)n + 63) / 64; }

int check_adj(const char* who, int nframes) {
    SE2_REQUIRE(nframes >= 1, SE2GPU_ERR_INVALID, "%s: nframes = %d is below 1", who, nframes);
    SE2_REQUIRE(nframes <= MAX_FRAMES, SE2GPU_ERR_CAPACITY, "%s: nframes = %d exceeds the limit %d", who, nframes, MAX_FRAMES);
    return SE2GPU_OK;
}

}  // namespace

extern "C" long long se2gpu_covis_adj_words(int nframes) {
    if (nframes < 1) return -1;
    return (long long)nframes * words_of(nframes);
}

extern "C" int se2gpu_covis_connect_device(se2gpu_matcher* h, uint64_t* d_adj, int nframes, const int32_t* d_pair_a,
                                           const int32_t* d_pair_b, int npairs, const int32_t* d_pair_out, int flag_mask) {
    const char* who = "covis_connect";
    SE2_NEED(h);
    SE2_NEED(d_adj); SE2_NEED(d_pair_a); SE2_NEED(d_pair_b);
    SE2_REQUIRE(npairs >= 0, SE2GPU_ERR_INVALID, "%s: npairs = %d is negative", who, npairs);
    SE2_CHECK(check_adj(who, nframes));
    SE2_REQUIRE(npairs <= MAX_PAIRS, SE2GPU_ERR_CAPACITY, "%s: npairs = %d exceeds the limit %d", who, npairs, MAX_PAIRS);
    if (npairs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    hipLaunchKernelGGL(k_adj_connect, dim3(((unsigned)npairs + BLOCK - 1u) / BLOCK), dim3(BLOCK), 0, st, (u64*)d_adj, nframes,
                       (int)words_of(nframes), d_pair_a, d_pair_b, npairs, d_pair_out, flag_mask);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

extern "C" int se2gpu_covis_disconnect_device(se2gpu_matcher* h, uint64_t* d_adj, int nframes, const int32_t* d_slots,
                                              int nslots) {
    const char* who = "covis_disconnect";
    SE2_NEED(h);
    SE2_NEED(d_adj); SE2_NEED(d_slots);
    SE2_REQUIRE(nslots >= 0, SE2GPU_ERR_INVALID, "%s: nslots = %d is negative", who, nslots);
    SE2_CHECK(check_adj(who, nframes));
    SE2_REQUIRE(nslots <= MAX_BLOCKS, SE2GPU_ERR_CAPACITY, "%s: nslots = %d exceeds the limit %d", who, nslots, MAX_BLOCKS);
    if (nslots == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    const int WF = (int)words_of(nframes);
    hipLaunchKernelGGL(k_adj_clear, dim3((unsigned)nslots), dim3(64), 0, st, (u64*)d_adj, nframes, WF, d_slots);
    hipLaunchKernelGGL(k_adj_zero, dim3((unsigned)nslots), dim3(64), 0, st, (u64*)d_adj, nframes, WF, d_slots);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

extern "C" int se2gpu_local_window_batch_device(se2gpu_matcher* h, const uint64_t* d_bits_kf, const uint64_t* d_bits_mp,
                                                int nframes, int m, const uint64_t* d_adj, const uint8_t* d_frame_null,
                                                const int32_t* d_job_kf, int njobs, int search_level, const int32_t* d_kf_order,
                                                const int32_t* d_mp_order, uint64_t* d_win_kf, uint64_t* d_win_mp,
                                                int32_t* d_win_out, int32_t* d_local_list, int32_t* d_ref_list, int kf_list_cap,
                                                int32_t* d_mp_list, int mp_list_cap) {
    const char* who = "local_window";
    SE2_NEED(h);
    SE2_NEED(d_bits_kf); SE2_NEED(d_bits_mp); SE2_NEED(d_adj); SE2_NEED(d_job_kf);
    SE2_NEED(d_win_kf); SE2_NEED(d_win_mp); SE2_NEED(d_win_out);
    SE2_REQUIRE(m >= 0, SE2GPU_ERR_INVALID, "%s: m = %d is negative", who, m);
    SE2_REQUIRE(njobs >= 0, SE2GPU_ERR_INVALID, "%s: njobs = %d is negative", who, njobs);
    SE2_REQUIRE(search_level >= 0, SE2GPU_ERR_INVALID, "%s: search_level = %d is negative", who, search_level);
    SE2_REQUIRE(kf_list_cap >= 0, SE2GPU_ERR_INVALID, "%s: kf_list_cap = %d is negative", who, kf_list_cap);
    SE2_REQUIRE(mp_list_cap >= 0, SE2GPU_ERR_INVALID, "%s: mp_list_cap = %d is negative", who, mp_list_cap);
    SE2_CHECK(check_adj(who, nframes));
    SE2_REQUIRE(((long long)nframes + 2) * words_of(m) <= INT_MAX, SE2GPU_ERR_CAPACITY,
                "%s: (nframes + 2) * ceil(m / 64) = %lld words of d_bits exceed the limit %d", who,
                ((long long)nframes + 2) * words_of(m), INT_MAX);
    SE2_REQUIRE(njobs <= MAX_BLOCKS, SE2GPU_ERR_CAPACITY, "%s: njobs = %d exceeds the limit %d", who, njobs, MAX_BLOCKS);
    if (njobs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    WindowArgs a;
    a.bits_kf = (const u64*)d_bits_kf; a.bits_mp = (const u64*)d_bits_mp; a.adj = (const u64*)d_adj;
    a.frame_null = d_frame_null; a.job_kf = d_job_kf; a.kf_order = d_kf_order; a.mp_order = d_mp_order;
    a.win_kf = (u64*)d_win_kf; a.win_mp = (u64*)d_win_mp; a.win_out = d_win_out;
    a.local_list = d_local_list; a.ref_list = d_ref_list; a.mp_list = d_mp_list;
    a.nframes = nframes; a.m = m; a.W = (int)words_of(m); a.WF = (int)words_of(nframes);
    a.search_level = search_level; a.kf_list_cap = kf_list_cap; a.mp_list_cap = mp_list_cap;
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    hipLaunchKernelGGL(k_local_window, dim3((unsigned)njobs), dim3(BLOCK), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}
