// libse2gpu - the map's observation table under new key frames and pruned ones on gfx950 (MI355X): the bookkeeping of
// LocalMapper::findCorrespd (src/LocalMapper.cpp:95-168 of the reference), MapPoint::addObservation's normal vector
// (src/MapPoint.cpp:104-122) and the erasures of KeyFrame::setNull / MapPoint::eraseObservation / MapPoint::setNull
// (src/KeyFrame.cpp:100-113, src/MapPoint.cpp:54-101) on the tables of obs_table.h in device memory.
//   k_begin       the sizes at entry, read from device memory and clamped to the capacities
//   k_claim       one thread per row of a job: the point a row of kind 1 or 2 names, claim[job][point] = max j (atomicMax),
//                 born[job][src] = max j for kind 3
//   k_job_rank    one workgroup per job: the rank of every kind-3 row among its job's, by ascending src (__shfl_up wave scans,
//                 the four wave totals through LDS)
//   k_count       one thread per point: the entries it keeps, which of its claims are taken (job order), its new length;
//                 the sums of its workgroup
//   k_scan_sums   one workgroup: exclusive scans of the workgroup sums and of the jobs' new points; the sizes and the status
//   k_points      one thread per point: its place (a scan inside the workgroup on top of the workgroup's offset), the erasures,
//                 the float chain of its normal vector in list order, the source of every entry it keeps or gains
//   k_null_rows   the ftr_mp / kf_observed rows of null key frames (a stride loop over all features)
//   k_features    one thread per row: the feature tables of the new key frame, the new points of kind 3
//   k_rows        one thread per word of the new entry arrays, in output order: contiguous stores, sources looked up per entry
// No atomic decides a place: atomicMax picks the winner of a claim, integer atomicAdd only sums counters.  Every output word is
// the same in every run.  Nothing in place is written before the status is known, and the writing kernels return on it.
// Every index read from an array is checked before it is used (obs_table.h); the normal vector is map_normal.h's text, shared
// with the host mirror include/se2lam_amd/MapUpdate.h.  Compiled with -ffp-contract=off like new_kf.hip.
#include "common.h"
#include "obs_table.h"
#include "wave_int.h"
#include "../../include/se2lam_amd/map_normal.h"

using namespace se2gpu;

namespace {

enum { H_M_OLD = 0, H_NOBS_OLD, H_STATUS, H_M_NEW, H_NOBS_NEW, H_ADDED, H_ERASED, H_CREATED, H_NULLED, H_SKIPPED, H_DUP, H_KEPT,
       H_WORDS = 16 };
constexpr int kBlock = 256, kWaves = kBlock / 64;   // the workgroups that scan; their lds is kWaves ints

struct ApplyArgs {
    const int* counts;
    const uint8_t* frame_null;
    const int* mp_ptr;
    const int* obs_frame;
    const int* obs_ftr;
    const float* obs_view;
    const float* obs_info;
    const int* sizes_in;
    const int* job_prev;
    const int* job_new;
    const uint8_t* kind;
    const int* src;
    const float* view;
    const float* info;
    const float* new_pos_w;
    const float* info_prev;
    const float* local_pos;
    const uint8_t* good_prl_row;
    const int* parallax_status;
    float* pos;
    uint8_t* good_prl;
    uint8_t* mp_null;
    float* mp_normal;
    int* ftr_mp;
    uint8_t* kf_observed;
    float* view_pos;
    float* view_info;
    int* mp_ptr_new;
    int* obs_frame_new;
    int* obs_ftr_new;
    float* obs_view_new;
    float* obs_info_new;
    int* new_frame;
    int* sizes_out;
    int* job_counts;
    // work space
    int* hdr;
    int* claim;      // B * m_cap: -1 none, j taken, -(j + 2) refused
    int* born;       // B * cap, by src: the row that creates a point, -1 none
    int* target;     // B * cap: the point a row of kind 1 or 2 names, -1 none
    int* rank3;      // B * cap, by src
    int* n3;         // B
    int* job_base;   // B
    int* job_ok;     // B
    int* cnt;        // m_cap
    int* bsum;       // workgroups of k_count
    int* boff;
    int* srcmap;     // nobs_cap: an old entry (>= 0) or -(1 + 2 row + which)
    int cap, nframes, m_cap, nobs_cap, B, kinds, nblk;

    __device__ __forceinline__ FrameSlots slots() const { return FrameSlots{counts, nullptr, cap, nframes}; }
    __device__ __forceinline__ ObsCsr old_csr() const { return ObsCsr{mp_ptr, obs_frame, obs_ftr, hdr[H_M_OLD], hdr[H_NOBS_OLD]}; }
    __device__ __forceinline__ bool is_null_frame(int f) const { return frame_null && frame_null[f]; }
    __device__ __forceinline__ bool dead(int p) const { return mp_null[p] || (parallax_status && parallax_status[p] == 2); }
    __device__ __forceinline__ bool job_valid(int fp, int fn) const {
        return (unsigned)fp < (unsigned)nframes && (unsigned)fn < (unsigned)nframes && fp != fn && !is_null_frame(fp) &&
               !is_null_frame(fn);
    }
};

// out[i] = in[0] + .. + in[i - 1] for i < n by one workgroup; returns the sum
__device__ int scan_array(const int* in, int* out, int n, int* lds) {
    int run = 0;
    for (int at = 0; at < n; at += kBlock) {
        const int i = at + (int)threadIdx.x, v = i < n ? in[i] : 0;
        int total;
        const int ex = block_scan_excl<kWaves>(v, lds, total);
        if (i < n) out[i] = run + ex;
        run += total;
    }
    return run;
}

__global__ void k_begin(ApplyArgs a) {
    if (threadIdx.x >= H_WORDS) return;
    int v = 0;
    if (threadIdx.x == H_M_OLD) v = ot_min(ot_max(a.sizes_in[0], 0), a.m_cap);
    if (threadIdx.x == H_NOBS_OLD) v = ot_min(ot_max(a.sizes_in[1], 0), a.nobs_cap);
    a.hdr[threadIdx.x] = v;
}

__global__ __launch_bounds__(128) void k_claim(ApplyArgs a) {
    const int b = blockIdx.y, j = blockIdx.x * 128 + threadIdx.x;
    const int fp = a.job_prev[b], fn = a.job_new[b];
    const bool ok = a.job_valid(fp, fn);
    if (j == 0) a.job_ok[b] = ok;
    if (!ok) return;
    const FrameSlots fs = a.slots();
    if (j >= feature_count(fs, fn)) return;
    const size_t row = (size_t)b * a.cap;
    const int k = a.kind[row + j], i = a.src[row + j];
    if (k < 1 || k > 3 || !((a.kinds >> k) & 1)) return;
    const bool i_in_prev = i >= 0 && i < feature_count(fs, fp);
    if (k == 3) {
        if (i_in_prev) atomicMax(&a.born[row + i], j);
        return;
    }
    int p = k == 2 ? i : (i_in_prev ? a.ftr_mp[(size_t)fp * a.cap + i] : -1);   // pPrefKF->getObservation(i) (:97)
    if (p < 0 || p >= a.hdr[H_M_OLD]) p = -1;
    a.target[row + j] = p;
    if (p >= 0) atomicMax(&a.claim[(size_t)b * a.m_cap + p], j);
}

__global__ __launch_bounds__(kBlock) void k_job_rank(ApplyArgs a) {
    __shared__ int lds[kWaves];
    const int b = blockIdx.x;
    const size_t row = (size_t)b * a.cap;
    int run = 0;
    for (int at = 0; at < a.cap; at += kBlock) {
        const int i = at + (int)threadIdx.x;
        const int has = i < a.cap && a.born[row + i] >= 0;
        int total;
        const int ex = block_scan_excl<kWaves>(has, lds, total);
        if (i < a.cap) a.rank3[row + i] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) a.n3[b] = run;
}

__global__ __launch_bounds__(kBlock) void k_count(ApplyArgs a) {
    __shared__ int lds[kWaves];
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int m_old = a.hdr[H_M_OLD];
    int len = 0, erased = 0, nulled = 0, added = 0;
    if (p < m_old) {
        const FrameSlots fs = a.slots();
        const ObsCsr csr = a.old_csr();
        int s, e, kept = 0;
        point_range(csr, p, s, e);
        for (int i = s; i < e; ++i)
            if (entry_offset(fs, csr, i) >= 0 && !a.is_null_frame(a.obs_frame[i])) ++kept;
        if (a.dead(p)) kept = 0;
        erased = ot_max(e - s, 0) - kept;
        nulled = kept == 0 && !a.mp_null[p];
        len = kept;
        for (int b = 0; b < a.B; ++b) {                               // the jobs that name the point, in job order
            int* c = &a.claim[(size_t)b * a.m_cap + p];
            const int j = *c;
            if (j < 0) continue;
            const int fn = a.job_new[b];
            bool refuse = kept == 0;                                  // KeyFrame::addObservation returns on a null point (:197)
            for (int i = s; i < e && !refuse; ++i)                    // std::map::insert keeps the old entry (:108)
                refuse = a.obs_frame[i] == fn && entry_offset(fs, csr, i) >= 0;
            if (refuse) *c = -(j + 2); else { ++len; ++added; }
        }
    }
    if (p < a.m_cap) a.cnt[p] = len;
    int total, t2;
    block_scan_excl<kWaves>(len, lds, total);
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
    block_scan_excl<kWaves>(erased, lds, total);
    block_scan_excl<kWaves>(added, lds, t2);
    if (threadIdx.x == 0 && total) atomicAdd(&a.hdr[H_ERASED], total);
    if (threadIdx.x == 0 && t2) atomicAdd(&a.hdr[H_ADDED], t2);
    block_scan_excl<kWaves>(nulled, lds, total);
    if (threadIdx.x == 0 && total) atomicAdd(&a.hdr[H_NULLED], total);
}

__global__ __launch_bounds__(kBlock) void k_scan_sums(ApplyArgs a) {
    __shared__ int lds[kWaves];
    const int kept = scan_array(a.bsum, a.boff, a.nblk, lds);
    const int born = a.B > 0 ? scan_array(a.n3, a.job_base, a.B, lds) : 0;
    if (threadIdx.x) return;
    const long long m_new = (long long)a.hdr[H_M_OLD] + born, nobs_new = (long long)kept + 2ll * born;
    const bool over = m_new > a.m_cap || nobs_new > a.nobs_cap;
    a.hdr[H_KEPT] = kept;
    a.hdr[H_CREATED] = born;
    a.hdr[H_ADDED] += 2 * born;
    a.hdr[H_M_NEW] = (int)m_new;            // both fit: m_cap + B cap and nobs_cap + 2 B cap stay below 2^31 (the C ABI's check)
    a.hdr[H_NOBS_NEW] = (int)nobs_new;
    a.hdr[H_STATUS] = over ? 2 : 0;
}

__global__ __launch_bounds__(kBlock) void k_points(ApplyArgs a) {
    __shared__ int lds[kWaves];
    if (a.hdr[H_STATUS]) return;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int m_old = a.hdr[H_M_OLD], m_new = a.hdr[H_M_NEW], kept_all = a.hdr[H_KEPT];
    int total;
    const int at0 = a.boff[blockIdx.x] + block_scan_excl<kWaves>(p < a.m_cap ? a.cnt[p] : 0, lds, total);
    if (p > a.m_cap) return;
    if (p >= m_old) {                                                 // new points (k_features fills them) and the padding
        a.mp_ptr_new[p] = kept_all + 2 * (ot_min(p, m_new) - m_old);
        if (p >= m_new && p < a.m_cap) {
            a.mp_null[p] = 1;
            a.good_prl[p] = 0;
            a.new_frame[p] = -1;
        }
        return;
    }
    a.mp_ptr_new[p] = at0;
    const FrameSlots fs = a.slots();
    const ObsCsr csr = a.old_csr();
    int s, e, size = 0, at = at0, fnew = -1;
    point_range(csr, p, s, e);
    const bool gone = a.dead(p);
    float nv[3] = {a.mp_normal[3 * (size_t)p], a.mp_normal[3 * (size_t)p + 1], a.mp_normal[3 * (size_t)p + 2]};
    bool touched = false;
    for (int i = s; i < e; ++i) size += entry_offset(fs, csr, i) >= 0;
    for (int i = s; i < e; ++i) {
        const int o = entry_offset(fs, csr, i);
        if (o < 0) continue;
        if (gone) {                                                   // MapPoint::setNull -> pKF->eraseObservation(idx) (:73-74)
            a.ftr_mp[o] = -1;
            a.kf_observed[o] = 0;
        } else if (a.is_null_frame(a.obs_frame[i])) {                 // MapPoint::eraseObservation (:86-101)
            if (--size > 0) {
                const float v[3] = {a.view_pos[3 * (size_t)o], a.view_pos[3 * (size_t)o + 1], a.view_pos[3 * (size_t)o + 2]};
                normal_erase(nv, v, size);
                touched = true;
            }
        } else {
            a.srcmap[at++] = i;
        }
    }
    if (at == at0) {                                                  // :56-57, :93-94
        a.mp_null[p] = 1;
        a.good_prl[p] = 0;
    }
    for (int b = 0; b < a.B; ++b) {                                   // :103-105, :138-140, in job order
        const int j = a.claim[(size_t)b * a.m_cap + p];
        if (j < 0) continue;
        const size_t r = (size_t)b * a.cap + j;
        const float v[3] = {a.view[3 * r], a.view[3 * r + 1], a.view[3 * r + 2]};
        normal_add(nv, v, at - at0);
        touched = true;
        a.srcmap[at++] = -(1 + 2 * (int)r);
        fnew = a.job_new[b];
    }
    if (touched) {
        a.mp_normal[3 * (size_t)p] = nv[0];
        a.mp_normal[3 * (size_t)p + 1] = nv[1];
        a.mp_normal[3 * (size_t)p + 2] = nv[2];
    }
    a.new_frame[p] = fnew;
}

__global__ __launch_bounds__(128) void k_null_rows(ApplyArgs a) {
    if (a.hdr[H_STATUS]) return;
    const long long n = (long long)a.nframes * a.cap;                 // <= INT_MAX (check_frame_slots)
    for (long long o = (long long)blockIdx.x * 128 + threadIdx.x; o < n; o += (long long)gridDim.x * 128) {
        if (!a.frame_null[o / a.cap]) continue;                       // KeyFrame::setNull (:110-111)
        a.ftr_mp[o] = -1;
        a.kf_observed[o] = 0;
    }
}

__device__ __forceinline__ void copy3(float* d, const float* s) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; }
__device__ __forceinline__ void copy9(float* d, const float* s) {
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = s[i];
}

__global__ __launch_bounds__(128) void k_features(ApplyArgs a) {
    const int b = blockIdx.y, j = blockIdx.x * 128 + threadIdx.x;
    const bool write = a.hdr[H_STATUS] == 0;
    const bool ok = a.job_ok[b] != 0;
    if (j == 0) a.job_counts[6 * b] = !ok;
    int applied = 0;
    bool skipped = false, dup = false;
    const int fp = a.job_prev[b], fn = a.job_new[b];
    const FrameSlots fs = a.slots();
    if (ok && j < feature_count(fs, fn)) {
        const size_t row = (size_t)b * a.cap, r = row + j;
        const int k = a.kind[r], i = a.src[r];
        const size_t onew = (size_t)fn * a.cap + j;
        int p = -1;
        if (k >= 1 && k <= 3 && ((a.kinds >> k) & 1)) {
            if (k == 3) {
                if (i >= 0 && i < feature_count(fs, fp)) {
                    if (a.born[row + i] == j) {
                        applied = 3;
                        p = a.hdr[H_M_OLD] + a.job_base[b] + a.rank3[row + i];
                    } else {
                        skipped = dup = true;
                    }
                } else {
                    skipped = true;
                }
            } else {
                const int t = a.target[r];
                const int c = t >= 0 ? a.claim[(size_t)b * a.m_cap + t] : -1;
                if (t >= 0 && c == j) {
                    applied = k;
                    p = t;
                } else {
                    skipped = true;
                    dup = t >= 0 && c != -(j + 2);
                }
            }
        }
        if (write && skipped) a.kf_observed[onew] = 0;
        if (write && applied) {                                       // mNewKF->setViewMP, mNewKF->addObservation (:103-104, :138-139, :155, :163)
            copy3(a.view_pos + 3 * onew, a.view + 3 * r);
            copy9(a.view_info + 9 * onew, a.info + 9 * r);
            a.ftr_mp[onew] = p;
            a.kf_observed[onew] = 1;
        }
        if (write && applied == 3) {                                  // :150-165
            const size_t oprev = (size_t)fp * a.cap + i;
            const float* lp = a.local_pos + 3 * (row + i);
            copy3(a.view_pos + 3 * oprev, lp);                        // pPrefKF->setViewMP(localMPs[i], i, xyzinfo0) (:156)
            copy9(a.view_info + 9 * oprev, a.info_prev + 9 * r);
            a.ftr_mp[oprev] = p;
            a.kf_observed[oprev] = 1;
            copy3(a.pos + 3 * (size_t)p, a.new_pos_w + 3 * r);        // MapPoint(posW, vbGoodPrl[i]) (:158)
            a.good_prl[p] = a.good_prl_row[row + i] ? 1 : 0;
            a.mp_null[p] = 0;
            float nv[3] = {0.f, 0.f, 0.f};
            const float v0[3] = {lp[0], lp[1], lp[2]}, v1[3] = {a.view[3 * r], a.view[3 * r + 1], a.view[3 * r + 2]};
            normal_add(nv, v0, 0);                                    // pMP->addObservation(pPrefKF, i) (:160)
            normal_add(nv, v1, 1);                                    // pMP->addObservation(mNewKF, vMatched12[i]) (:161)
            copy3(a.mp_normal + 3 * (size_t)p, nv);
            a.new_frame[p] = fn;
            const int at = a.hdr[H_KEPT] + 2 * (p - a.hdr[H_M_OLD]);
            a.srcmap[at] = -(2 + 2 * (int)r);
            a.srcmap[at + 1] = -(1 + 2 * (int)r);
        }
    }
    for (int k = 1; k <= 5; ++k) {                                    // one atomic per wave and counter
        const unsigned long long bal = __ballot(k <= 3 ? applied == k : (k == 4 ? skipped : dup));
        if ((threadIdx.x & 63) == 0 && bal) {
            atomicAdd(&a.job_counts[6 * b + k], __popcll(bal));
            if (k >= 4) atomicAdd(&a.hdr[k == 4 ? H_SKIPPED : H_DUP], __popcll(bal));
        }
    }
}

// word w of the output: the frames, the features, then the view and the information rows, each array in output order
__global__ __launch_bounds__(kBlock) void k_rows(ApplyArgs a) {
    const long long w = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (w == 0) {
        a.sizes_out[SE2GPU_MAP_APPLY_STATUS] = a.hdr[H_STATUS];
        a.sizes_out[SE2GPU_MAP_APPLY_M_NEW] = a.hdr[H_M_NEW];
        a.sizes_out[SE2GPU_MAP_APPLY_NOBS_NEW] = a.hdr[H_NOBS_NEW];
        a.sizes_out[SE2GPU_MAP_APPLY_ADDED] = a.hdr[H_ADDED];
        a.sizes_out[SE2GPU_MAP_APPLY_ERASED] = a.hdr[H_ERASED];
        a.sizes_out[SE2GPU_MAP_APPLY_CREATED] = a.hdr[H_CREATED];
        a.sizes_out[SE2GPU_MAP_APPLY_NULLED] = a.hdr[H_NULLED];
        a.sizes_out[SE2GPU_MAP_APPLY_SKIPPED] = a.hdr[H_SKIPPED];
        a.sizes_out[SE2GPU_MAP_APPLY_DUP] = a.hdr[H_DUP];
        if (a.hdr[H_STATUS] == 0) a.mp_ptr_new[a.m_cap] = a.hdr[H_NOBS_NEW];
    }
    if (a.hdr[H_STATUS]) return;
    const long long n = a.hdr[H_NOBS_NEW];
    const bool rows = a.obs_view_new != nullptr;
    if (w >= (rows ? 14 : 2) * n) return;
    // the array, the entry and the word within its row
    int part, e, c;
    if (w < 2 * n) { part = (int)(w / n); e = (int)(w % n); c = 0; }
    else if (w < 5 * n) { part = 2; e = (int)((w - 2 * n) / 3); c = (int)((w - 2 * n) % 3); }
    else { part = 3; e = (int)((w - 5 * n) / 9); c = (int)((w - 5 * n) % 9); }
    const int code = a.srcmap[e];
    if (code >= 0) {                                                  // an entry the point keeps
        if (part == 0) a.obs_frame_new[e] = a.obs_frame[code];
        else if (part == 1) a.obs_ftr_new[e] = a.obs_ftr[code];
        else if (part == 2) a.obs_view_new[3 * (size_t)e + c] = a.obs_view[3 * (size_t)code + c];
        else a.obs_info_new[9 * (size_t)e + c] = a.obs_info[9 * (size_t)code + c];
        return;
    }
    const int r = (-code - 1) >> 1, prev = (-code - 1) & 1;           // a row's entry: of the new key frame, or of the previous one
    const int b = r / a.cap;
    if (part == 0) a.obs_frame_new[e] = prev ? a.job_prev[b] : a.job_new[b];
    else if (part == 1) a.obs_ftr_new[e] = prev ? a.src[r] : r - b * a.cap;
    else if (part == 2) a.obs_view_new[3 * (size_t)e + c] = prev ? a.local_pos[3 * ((size_t)b * a.cap + a.src[r]) + c] : a.view[3 * (size_t)r + c];
    else a.obs_info_new[9 * (size_t)e + c] = prev ? a.info_prev[9 * (size_t)r + c] : a.info[9 * (size_t)r + c];
}

// the work space, in ints
struct WsLayout {
    long long hdr, claim, born, target, rank3, n3, job_base, job_ok, cnt, bsum, boff, srcmap, words;
};
bool ws_layout(int B, int cap, int m_cap, int nobs_cap, WsLayout& l) {
    if (B < 0 || cap < 1 || m_cap < 0 || nobs_cap < 0) return false;
    const long long rows = (long long)B * cap, nblk = ((long long)m_cap + kBlock) / kBlock;   // points 0..m_cap
    auto pad = [](long long n) { return (n + 3) & ~3ll; };
    long long at = 0;
    l.hdr = at; at += H_WORDS;
    l.claim = at; at += pad((long long)B * m_cap);
    l.born = at; at += pad(rows);
    l.target = at; at += pad(rows);
    l.rank3 = at; at += pad(rows);
    l.n3 = at; at += pad(B);
    l.job_base = at; at += pad(B);
    l.job_ok = at; at += pad(B);
    l.cnt = at; at += pad(m_cap);
    l.bsum = at; at += pad(nblk);
    l.boff = at; at += pad(nblk);
    l.srcmap = at; at += pad(nobs_cap);
    l.words = at;
    return true;
}

}  // namespace

extern "C" long long se2gpu_map_apply_ws_bytes(int B, int cap, int m_cap, int nobs_cap) {
    WsLayout l;
    if (!ws_layout(B, cap, m_cap, nobs_cap, l)) return -1;
    if (B > 65535 || (long long)B * m_cap > INT_MAX || (long long)m_cap + (long long)B * cap >= INT_MAX ||
        (long long)nobs_cap + 2ll * B * cap + 1 >= INT_MAX)
        return -1;
    return l.words * (long long)sizeof(int32_t);
}

extern "C" int se2gpu_map_apply_batch_device(
    se2gpu_matcher* h, const int32_t* d_counts, int cap, int nframes, const uint8_t* d_frame_null, const int32_t* d_mp_ptr,
    const int32_t* d_obs_frame, const int32_t* d_obs_ftr, const float* d_obs_view, const float* d_obs_info,
    const int32_t* d_sizes_in, int m_cap, int nobs_cap, const int32_t* d_job_prev, const int32_t* d_job_new, int B,
    const uint8_t* d_kind, const int32_t* d_src, const float* d_view, const float* d_info, const float* d_new_pos_w,
    const float* d_info_prev, const float* d_local_pos, const uint8_t* d_good_prl_row, int kinds,
    const int32_t* d_parallax_status, float* d_pos, uint8_t* d_good_prl, uint8_t* d_mp_null, float* d_mp_normal,
    int32_t* d_ftr_mp, uint8_t* d_kf_observed, float* d_view_pos, float* d_view_info, int32_t* d_mp_ptr_new,
    int32_t* d_obs_frame_new, int32_t* d_obs_ftr_new, float* d_obs_view_new, float* d_obs_info_new, int32_t* d_new_frame,
    int32_t* d_sizes_out, int32_t* d_job_counts, void* d_ws, long long ws_bytes) {
    const char* who = "map_apply_batch";
    SE2_NEED(h);
    SE2_REQUIRE(B >= 0, SE2GPU_ERR_INVALID, "%s: B = %d is negative", who, B);
    SE2_REQUIRE((kinds & ~14) == 0, SE2GPU_ERR_INVALID, "%s: kinds = %d has bits outside 1..3", who, kinds);
    SE2_CHECK(check_obs_csr(who, d_mp_ptr, d_obs_frame, d_obs_ftr, m_cap, nobs_cap));
    SE2_CHECK(check_frame_slots(who, d_counts, cap, nframes));
    SE2_NEED(d_sizes_in);
    SE2_REQUIRE(!d_obs_view == !d_obs_info && !d_obs_view == !d_obs_view_new && !d_obs_view == !d_obs_info_new,
                SE2GPU_ERR_INVALID, "%s: d_obs_view, d_obs_info, d_obs_view_new and d_obs_info_new go together", who);
    SE2_NEED_IF(B > 0, d_job_prev); SE2_NEED_IF(B > 0, d_job_new); SE2_NEED_IF(B > 0, d_kind); SE2_NEED_IF(B > 0, d_src);
    SE2_NEED_IF(B > 0, d_view); SE2_NEED_IF(B > 0, d_info); SE2_NEED_IF(B > 0, d_job_counts);
    SE2_REQUIRE(B == 0 || !(kinds & 8) || (d_new_pos_w && d_info_prev && d_local_pos && d_good_prl_row), SE2GPU_ERR_INVALID,
                "%s: kind 3 needs d_new_pos_w, d_info_prev, d_local_pos and d_good_prl_row", who);
    SE2_NEED(d_pos); SE2_NEED(d_good_prl); SE2_NEED(d_mp_null); SE2_NEED(d_mp_normal);
    SE2_NEED(d_ftr_mp); SE2_NEED(d_kf_observed); SE2_NEED(d_view_pos); SE2_NEED(d_view_info);
    SE2_NEED(d_mp_ptr_new); SE2_NEED_IF(nobs_cap > 0, d_obs_frame_new); SE2_NEED_IF(nobs_cap > 0, d_obs_ftr_new);
    SE2_NEED(d_new_frame); SE2_NEED(d_sizes_out); SE2_NEED(d_ws);
    SE2_REQUIRE(d_mp_ptr_new != d_mp_ptr && (!d_obs_frame_new || d_obs_frame_new != d_obs_frame) &&
                    (!d_obs_ftr_new || d_obs_ftr_new != d_obs_ftr) && (!d_obs_view_new || d_obs_view_new != d_obs_view) &&
                    (!d_obs_info_new || d_obs_info_new != d_obs_info),
                SE2GPU_ERR_INVALID, "%s: the new table must not be the old one", who);
    SE2_REQUIRE(((uintptr_t)d_ws & 15) == 0, SE2GPU_ERR_INVALID, "%s: d_ws is not 16-byte aligned", who);
    SE2_REQUIRE(B <= 65535 && (long long)B * m_cap <= INT_MAX && (long long)m_cap + (long long)B * cap < INT_MAX &&
                    (long long)nobs_cap + 2ll * B * cap + 1 < INT_MAX && 14ll * nobs_cap / kBlock < INT_MAX,
                SE2GPU_ERR_CAPACITY,
                "%s: %d jobs of %d features on %d points and %d entries exceed the limit (65535 jobs; B m_cap, m_cap + B cap and "
                "nobs_cap + 2 B cap + 1 below %d)", who, B, cap, m_cap, nobs_cap, INT_MAX);
    WsLayout l;
    ws_layout(B, cap, m_cap, nobs_cap, l);
    SE2_REQUIRE(ws_bytes >= l.words * (long long)sizeof(int32_t), SE2GPU_ERR_CAPACITY,
                "%s: the work space has %lld bytes, se2gpu_map_apply_ws_bytes asks for %lld", who, ws_bytes,
                l.words * (long long)sizeof(int32_t));
    if (B == 0 && m_cap == 0) return SE2GPU_OK;   // no job and a table without a point slot: nothing to erase, nothing written (d_sizes_out neither)
    SE2_NEED_DEVICE();
    int* ws = (int*)d_ws;
    ApplyArgs a;
    a.counts = d_counts; a.frame_null = d_frame_null; a.mp_ptr = d_mp_ptr; a.obs_frame = d_obs_frame; a.obs_ftr = d_obs_ftr;
    a.obs_view = d_obs_view; a.obs_info = d_obs_info; a.sizes_in = d_sizes_in; a.job_prev = d_job_prev; a.job_new = d_job_new;
    a.kind = d_kind; a.src = d_src; a.view = d_view; a.info = d_info; a.new_pos_w = d_new_pos_w; a.info_prev = d_info_prev;
    a.local_pos = d_local_pos; a.good_prl_row = d_good_prl_row; a.parallax_status = d_parallax_status; a.pos = d_pos;
    a.good_prl = d_good_prl; a.mp_null = d_mp_null; a.mp_normal = d_mp_normal; a.ftr_mp = d_ftr_mp; a.kf_observed = d_kf_observed;
    a.view_pos = d_view_pos; a.view_info = d_view_info; a.mp_ptr_new = d_mp_ptr_new; a.obs_frame_new = d_obs_frame_new;
    a.obs_ftr_new = d_obs_ftr_new; a.obs_view_new = d_obs_view_new; a.obs_info_new = d_obs_info_new; a.new_frame = d_new_frame;
    a.sizes_out = d_sizes_out; a.job_counts = d_job_counts;
    a.hdr = ws + l.hdr; a.claim = ws + l.claim; a.born = ws + l.born; a.target = ws + l.target; a.rank3 = ws + l.rank3;
    a.n3 = ws + l.n3; a.job_base = ws + l.job_base; a.job_ok = ws + l.job_ok; a.cnt = ws + l.cnt; a.bsum = ws + l.bsum;
    a.boff = ws + l.boff; a.srcmap = ws + l.srcmap;
    a.cap = cap; a.nframes = nframes; a.m_cap = m_cap; a.nobs_cap = nobs_cap; a.B = B; a.kinds = kinds;
    a.nblk = (int)(((long long)m_cap + kBlock) / kBlock);
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    const dim3 job_grid(((unsigned)cap + 127u) / 128u, (unsigned)B);
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(64), 0, st, a);
    if (B > 0) {
        SE2_HIP(hipMemsetAsync(a.claim, 0xff, (size_t)(l.target - l.claim) * sizeof(int32_t), st));   // claim and born: -1
        SE2_HIP(hipMemsetAsync(d_job_counts, 0, 6 * (size_t)B * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_claim, job_grid, dim3(128), 0, st, a);
        hipLaunchKernelGGL(k_job_rank, dim3((unsigned)B), dim3(kBlock), 0, st, a);
    }
    hipLaunchKernelGGL(k_count, dim3((unsigned)a.nblk), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_points, dim3((unsigned)a.nblk), dim3(kBlock), 0, st, a);
    if (d_frame_null)
        hipLaunchKernelGGL(k_null_rows, dim3((unsigned)ot_min((int)(((long long)nframes * cap + 127) / 128), 65536)), dim3(128), 0,
                           st, a);   // a stride loop over the features: no limit on nframes beyond nframes * cap
    if (B > 0) hipLaunchKernelGGL(k_features, job_grid, dim3(128), 0, st, a);
    const long long words = (d_obs_view_new ? 14ll : 2ll) * nobs_cap;
    hipLaunchKernelGGL(k_rows, dim3((unsigned)(words / kBlock + 1)), dim3(kBlock), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}
