// libse2gpu - MapPoint::updateMainKFandDescriptor for batches of map points on gfx950 (MI355X).
//
// Replaces the body of se2lam::MapPoint::updateMainKFandDescriptor (src/MapPoint.cpp:228-292 of the reference): of a point's
// observations the one whose descriptor has the least median Hamming distance to all of them (self-distance 0 included,
// median = element (N-1)/2 of the sorted row) becomes the main observation, the first in container order on a tie
// (`median < bestMedian`, :272).  The reference fills an N x N table and sorts every row; here
//   - lane j of a group of G lanes holds the descriptor of observation j as four 64-bit words,
//   - row i is handed to the group (a shuffle in the packed kernel, a readlane in the one-point-per-wave kernel),
//   - the row's k-th smallest distance comes from a 9-step bisection on 0..256: count(d <= mid) by ballot + popcount,
// so no row is stored or sorted and a point's result is a function of its own list alone (no atomics, no reduction whose
// order could vary).  Two launches:
//   k_mappoint_small  a wave takes 8 consecutive points; those with up to 8 observations run eight at a time in groups of 8
//                     lanes, then the ones with 9..16 four at a time (G = 16), 17..32 two at a time, 33..64 one at a time
//   k_mappoint_large  points with more than 64 observations, one workgroup per point, its waves taking the rows in turn:
//                     kRegTiles tiles of 64 observations live in registers (descriptor + distance of the current row), the
//                     tiles beyond are recomputed from memory in every bisection step - N is bounded by the CSR alone
// Which observations count and where a point's list lies is obs_table.h's entry and segment rule, with the null key frames
// skipped as the reference skips them (:242).
// Compiled with -ffp-contract=off: mMinDist / mMaxDist (:287-291) are IEEE operations, equal to the host's to the bit.
#include "common.h"
#include "obs_table.h"

using namespace se2gpu;

namespace {

constexpr int kMaxLevels = 32;   // scale factors travel by value in the kernel arguments
constexpr int kRegTiles = 4;     // k_mappoint_large: observations 0..255 of a point stay in registers
constexpr int kLargeWaves = 8;   // k_mappoint_large: waves that share the rows of one point

typedef unsigned long long u64;

// The table's fields keep the places they had in the kernel arguments before obs_table.h: the kernels fetch them in the same
// pieces and compile to the same instructions.  slots() and csr() hand them to the shared rules.
struct MpArgs {
    const se2gpu_keypoint* kps;
    const uint8_t* desc;
    const int* counts;
    const uint8_t* frame_null;
    const float* view_pos;
    const int* mp_ptr;
    const int* obs_frame;
    const int* obs_ftr;
    const int* prev;
    int* info;
    uint8_t* main_desc;
    int* main_frame;
    int* main_octave;
    float* dist;
    int cap, nframes, nlevels, m, nobs;
    float sf[kMaxLevels];
    __device__ __forceinline__ FrameSlots slots() const { return FrameSlots{counts, frame_null, cap, nframes}; }
    __device__ __forceinline__ ObsCsr csr() const { return ObsCsr{mp_ptr, obs_frame, obs_ftr, m, nobs}; }
};

__device__ __forceinline__ void load_desc(const MpArgs& a, int off, u64 d[4]) {
    const u64* p = (const u64*)(a.desc + 32 * (size_t)off);
    d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; d[3] = p[3];
}

__device__ __forceinline__ int hamming256(const u64 a[4], const u64 b[4]) {
    return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}

__device__ __forceinline__ void write_none(const MpArgs& a, int p) {
    int* o = a.info + 4 * (size_t)p;
    o[0] = -1; o[1] = 0; o[2] = 0; o[3] = 0;
}

// MapPoint.cpp:278-291, run by one lane: `pos` is the main observation's place in the point's list, `off` its feature
__device__ __forceinline__ void write_main(const MpArgs& a, int p, int pos, int median, int N, int frame, int off,
                                           const u64 d[4]) {
    u64* md = (u64*)(a.main_desc + 32 * (size_t)p);
    md[0] = d[0]; md[1] = d[1]; md[2] = d[2]; md[3] = d[3];              // :278, always
    a.main_frame[p] = frame;
    int changed = !a.prev || a.prev[p] != frame;                       // :280
    if (changed) {
        const int octave = a.kps[off].octave;
        a.main_octave[p] = octave;                                      // :285
        if ((unsigned)octave >= (unsigned)a.nlevels) {
            changed |= 2;
        } else if (a.view_pos) {
            const float* v = a.view_pos + 3 * (size_t)off;
            const double x = v[0], y = v[1], z = v[2];
            const float dist = (float)__dsqrt_rn(x * x + y * y + z * z);   // cv::norm(Point3f), :287
            const float mx = dist * a.sf[octave];                           // :290
            a.dist[2 * (size_t)p] = mx / a.sf[a.nlevels - 1];               // :291
            a.dist[2 * (size_t)p + 1] = mx;
        }
    }
    int* o = a.info + 4 * (size_t)p;
    o[0] = pos; o[1] = median; o[2] = N; o[3] = changed;
}

// the bits of a wave ballot that belong to the group of G lanes starting at lane `base`
__device__ __forceinline__ u64 group_bits(u64 ballot, int base, int G) {
    return G == 64 ? ballot : (ballot >> base) & ((1ull << G) - 1);
}

// One point per group of G lanes (G = 8, 16, 32 or 64; the point has n <= G observations from s), every group of the wave
// at once.  Called by the whole wave; a group without a point has active = false and only takes part in the ballots.
__device__ __forceinline__ void group_pass(const MpArgs& a, int G, bool active, int p, int s, int n) {
    const int lane = threadIdx.x & 63, sub = lane & (G - 1), base = lane - sub;
    int frame = -1, off = -1;
    u64 d[4] = {0, 0, 0, 0};
    if (active && sub < n) {
        frame = a.obs_frame[s + sub];
        off = entry_offset(a.slots(), a.csr(), s + sub);
        if (off >= 0) load_desc(a, off, d);
    }
    const bool valid = off >= 0;
    const u64 vm = group_bits(__ballot(valid), base, G);   // the point's valid observations, bit = place in its list
    const int N = __popcll(vm);
    const int k1 = ((N - 1) >> 1) + 1;                     // the median is the smallest t with count(d <= t) >= k1
    int best = -1, bestMedian = INT_MAX;
    for (int i = 0; i < G; ++i) {
        if (!__ballot((vm >> i) & 1)) continue;            // row i is valid in no group of the wave
        u64 r[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) r[w] = __shfl(d[w], base + i);
        const int dist = hamming256(r, d);
        int lo = 0, hi = 256;
#pragma unroll
        for (int step = 0; step < 9; ++step) {
            const int mid = (lo + hi) >> 1;
            const int c = __popcll(group_bits(__ballot(valid && dist <= mid), base, G));
            if (c >= k1) hi = mid; else lo = mid + 1;
        }
        if (((vm >> i) & 1) && lo < bestMedian) { bestMedian = lo; best = i; }   // strictly smaller: the first wins (:272)
    }
    if (!active) return;
    if (N == 0) {
        if (sub == 0) write_none(a, p);
    } else if (sub == best) {
        write_main(a, p, best, bestMedian, N, frame, off, d);
    }
}

__global__ __launch_bounds__(256) void k_mappoint_small(MpArgs a) {
    const int lane = threadIdx.x & 63;
    const int p0 = 8 * (int)((blockIdx.x * 256u + threadIdx.x) >> 6);
    if (p0 >= a.m) return;
    int ps = 0, pn = -1;                                   // lane l < 8: the segment of point p0 + l
    if (lane < 8 && p0 + lane < a.m) {
        point_segment(a.csr(), p0 + lane, ps, pn);
        if (pn == 0) write_none(a, p0 + lane);
    }
    for (int G = 8; G <= 64; G <<= 1) {
        const int least = G == 8 ? 1 : (G >> 1) + 1;
        unsigned cm = (unsigned)__ballot(pn >= least && pn <= G) & 0xffu;   // the wave's points of this class
        const int per_round = 64 / G, g = lane / G;
        while (cm) {
            unsigned t = cm;
            for (int j = 0; j < g; ++j) t &= t - 1;        // group g takes the g-th point of the class
            const bool active = t != 0;
            const int l = active ? __ffs(t) - 1 : 0;
            const int s = __shfl(ps, l), n = __shfl(pn, l);
            group_pass(a, G, active, p0 + l, s, n);
            for (int j = 0; j < per_round && cm; ++j) cm &= cm - 1;
        }
    }
}

__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// Points with more than 64 observations.  Workgroup b looks at points 64 b .. 64 b + 63 (one per lane, every wave the same)
// and runs the large ones one after the other: each of its kLargeWaves waves holds the point's tiles and takes the rows
// w, w + kLargeWaves, ..; the waves' candidates meet in LDS, where the least (median, row) wins - the first row of the
// least median, whatever the order the waves arrive in.
__global__ __launch_bounds__(64 * kLargeWaves) void k_mappoint_large(MpArgs a) {
    __shared__ int s_best[kLargeWaves][3];   // median, row, feature
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int pl = 64 * (int)blockIdx.x + lane;
    int ps = 0, pn = 0;
    if (pl < a.m) point_segment(a.csr(), pl, ps, pn);
    for (u64 todo = __ballot(pn > 64); todo; todo &= todo - 1) {
        const int l = __ffsll((long long)todo) - 1;
        const int p = 64 * (int)blockIdx.x + l;
        const int s = __builtin_amdgcn_readlane(ps, l), n = __builtin_amdgcn_readlane(pn, l);
        int off[kRegTiles];
        u64 d[kRegTiles][4];
        int N = 0;
#pragma unroll
        for (int r = 0; r < kRegTiles; ++r) {
            const int j = 64 * r + lane;
            off[r] = -1;
            d[r][0] = d[r][1] = d[r][2] = d[r][3] = 0;
            if (j < n) {
                off[r] = entry_offset(a.slots(), a.csr(), s + j);
                if (off[r] >= 0) load_desc(a, off[r], d[r]);
            }
            N += __popcll(__ballot(off[r] >= 0));
        }
        for (int j0 = 64 * kRegTiles; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const int o = j < n ? entry_offset(a.slots(), a.csr(), s + j) : -1;
            N += __popcll(__ballot(o >= 0));
        }
        if (N == 0) {                                     // (every wave counts the same N)
            if (threadIdx.x == 0) write_none(a, p);
            continue;
        }
        const int k1 = ((N - 1) >> 1) + 1;
        int best = -1, bestMedian = INT_MAX, bestOff = -1;
        for (int i = wave; i < n; i += kLargeWaves) {
            int ro = -1;
            u64 rd[4] = {0, 0, 0, 0};
            if (i < 64 * kRegTiles) {
#pragma unroll
                for (int r = 0; r < kRegTiles; ++r)
                    if (r == (i >> 6)) {
                        ro = __builtin_amdgcn_readlane(off[r], i & 63);
#pragma unroll
                        for (int w = 0; w < 4; ++w) rd[w] = readlane64(d[r][w], i & 63);
                    }
            } else {
                ro = entry_offset(a.slots(), a.csr(), s + i);
                if (ro >= 0) load_desc(a, ro, rd);
            }
            if (ro < 0) continue;
            int dist[kRegTiles];
#pragma unroll
            for (int r = 0; r < kRegTiles; ++r) dist[r] = off[r] >= 0 ? hamming256(rd, d[r]) : INT_MAX;
            int lo = 0, hi = 256;
            for (int step = 0; step < 9; ++step) {
                const int mid = (lo + hi) >> 1;
                int c = 0;
#pragma unroll
                for (int r = 0; r < kRegTiles; ++r) c += __popcll(__ballot(dist[r] <= mid));
                for (int j0 = 64 * kRegTiles; j0 < n; j0 += 64) {   // beyond the register tiles: from memory again
                    const int j = j0 + lane;
                    bool in = false;
                    if (j < n) {
                        const int o = entry_offset(a.slots(), a.csr(), s + j);
                        if (o >= 0) {
                            u64 dj[4];
                            load_desc(a, o, dj);
                            in = hamming256(rd, dj) <= mid;
                        }
                    }
                    c += __popcll(__ballot(in));
                }
                if (c >= k1) hi = mid; else lo = mid + 1;
            }
            if (lo < bestMedian) { bestMedian = lo; best = i; bestOff = ro; }
        }
        if (lane == 0) { s_best[wave][0] = bestMedian; s_best[wave][1] = best; s_best[wave][2] = bestOff; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 0; w < kLargeWaves; ++w)
                if (s_best[w][1] >= 0 && (best < 0 || s_best[w][0] < bestMedian || (s_best[w][0] == bestMedian && s_best[w][1] < best))) {
                    bestMedian = s_best[w][0]; best = s_best[w][1]; bestOff = s_best[w][2];
                }
            u64 bd[4];
            load_desc(a, bestOff, bd);
            write_main(a, p, best, bestMedian, N, a.obs_frame[s + best], bestOff, bd);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int se2gpu_mappoint_main_batch_device(se2gpu_matcher* h, const se2gpu_keypoint* d_kps, const uint8_t* d_desc,
                                                 const int32_t* d_counts, int cap, int nframes,
                                                 const uint8_t* d_frame_null, const float* d_view_pos,
                                                 const float* scale_factors, int nlevels, const int32_t* d_mp_ptr,
                                                 const int32_t* d_obs_frame, const int32_t* d_obs_ftr, int m, int nobs,
                                                 const int32_t* d_prev_main_frame, int32_t* d_info, uint8_t* d_main_desc,
                                                 int32_t* d_main_frame, int32_t* d_main_octave, float* d_dist) {
    const char* who = "mappoint_main_batch";
    SE2_NEED(h); SE2_NEED(d_kps); SE2_NEED(d_desc);
    SE2_NEED(d_info); SE2_NEED(d_main_desc); SE2_NEED(d_main_frame); SE2_NEED(d_main_octave);
    SE2_CHECK(check_obs_csr(who, d_mp_ptr, d_obs_frame, d_obs_ftr, m, nobs));
    SE2_REQUIRE(nlevels >= 1, SE2GPU_ERR_INVALID, "%s: nlevels = %d is below 1", who, nlevels);
    SE2_REQUIRE(!d_view_pos || (scale_factors && d_dist), SE2GPU_ERR_INVALID, "%s: d_view_pos needs scale_factors and d_dist", who);
    SE2_CHECK(check_frame_slots(who, d_counts, cap, nframes));   // its nframes * cap refusal is the first of the capacity ones
    SE2_REQUIRE(nlevels <= kMaxLevels, SE2GPU_ERR_CAPACITY, "%s: %d levels exceed the limit %d", who, nlevels, kMaxLevels);
    if (m == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    MpArgs a;
    a.kps = d_kps; a.desc = d_desc; a.counts = d_counts; a.frame_null = d_frame_null; a.view_pos = d_view_pos;
    a.mp_ptr = d_mp_ptr; a.obs_frame = d_obs_frame; a.obs_ftr = d_obs_ftr; a.prev = d_prev_main_frame;
    a.info = d_info; a.main_desc = d_main_desc; a.main_frame = d_main_frame; a.main_octave = d_main_octave; a.dist = d_dist;
    a.cap = cap; a.nframes = nframes; a.nlevels = nlevels; a.m = m; a.nobs = nobs;
    for (int i = 0; i < kMaxLevels; ++i) a.sf[i] = scale_factors && i < nlevels ? scale_factors[i] : 1.0f;
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    const unsigned waves = ((unsigned)m + 7u) / 8u;
    hipLaunchKernelGGL(k_mappoint_small, dim3((waves + 3u) / 4u), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_mappoint_large, dim3(((unsigned)m + 63u) / 64u), dim3(64 * kLargeWaves), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}
