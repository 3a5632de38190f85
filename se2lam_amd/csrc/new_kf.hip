// libse2gpu - the observations of a new key frame on gfx950 (MI355X): LocalMapper::findCorrespd and what its
// addObservation calls run, on arrays in device memory.
//   k_parallax      MapPoint::updateParallax (src/MapPoint.cpp:124-185 of the reference) for a batch of points, one thread per
//                   point: the oldest key frame of the last six, cvu::triangulate against the new one, the depth and parallax
//                   gates, then promotion (position, mViewMPs / mViewMPsInfo of every observation), abandonment
//                   (MapPoint::setNull, :68-78: the hasObservation flags of its features) or nothing
//   k_invert_match  inv[j] = i of a key frame's vMatched12 row
//   k_correspd      the three passes of LocalMapper::findCorrespd (src/LocalMapper.cpp:87-170) for a batch of new key frames,
//                   one thread per feature of the new key frame: which feature becomes an observation, its mViewMPs and
//                   mViewMPsInfo
// The arithmetic is view_info.h's, shared with the host mirror (include/se2lam_amd/FindCorrespd.h).  A point's and a
// feature's outputs are functions of their own inputs alone: integer atomics for the counters, no float atomics.
// The frame slots of a batch's jobs are pairwise distinct (the caller's duty, se2gpu.h): a job owns the flags of its two frames.
// Every index read from an array is checked before it is used (obs_table.h; a null key frame is not skipped): nothing is indexed outside them.
// Compiled with -ffp-contract=off like the matchers and triangulate.hip.
#include "common.h"
#include "obs_table.h"
#include "view_info.h"

using namespace se2gpu;

namespace {

struct FrameArgs {
    const se2gpu_keypoint* kps_un;
    const int* counts;
    const float* Tcw;
    const float* Twc;
    const float* P;
    int cap, nframes;
    // no frame_null: updateParallax and findCorrespd do not skip a null key frame, and the rule's test folds away
    __device__ __forceinline__ FrameSlots slots() const { return FrameSlots{counts, nullptr, cap, nframes}; }
};

struct PrlArgs {
    FrameArgs fr;
    const int* idkf;
    const int* mp_ptr;
    const int* obs_frame;
    const int* obs_ftr;
    const uint8_t* good_prl;
    const int* new_frame;
    uint8_t* kf_observed;
    int* status;
    int* pkf0_place;
    float* pos;
    float* obs_view;
    float* obs_info;
    int m, nobs;
    float fx, lower, upper;
    __device__ __forceinline__ ObsCsr csr() const { return ObsCsr{mp_ptr, obs_frame, obs_ftr, m, nobs}; }
};
__device__ __forceinline__ void store3(float* dst, const float v[3]) {
    dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
}
__device__ __forceinline__ void store9(float* dst, const float v[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) dst[i] = v[i];
}

__global__ __launch_bounds__(128) void k_parallax(PrlArgs a) {
    const int p = blockIdx.x * 128 + threadIdx.x;
    if (p >= a.m) return;
    const FrameArgs& fr = a.fr;
    const FrameSlots fs = fr.slots();
    const ObsCsr csr = a.csr();
    int status = 0, place0 = -1, s, n;
    point_segment(csr, p, s, n);
    const int fnew = a.new_frame[p];
    do {
        if (a.good_prl[p]) break;                                      // :125
        int N = 0, place1 = -1, off1 = -1;                             // pKF: the first valid entry of the new frame
        for (int i = 0; i < n; ++i) {
            const int f = a.obs_frame[s + i], off = entry_offset(fs, csr, s + i);
            if (off < 0) continue;
            ++N;
            if (f == fnew && place1 < 0) { place1 = i; off1 = off; }
        }
        if (N <= 2 || place1 < 0) break;                               // :125
        const long long id1 = a.idkf[fnew];
        long long id0 = 0;
        int f0 = -1, off0 = -1;
        for (int i = 0; i < n; ++i) {                                  // :129-139, the oldest key frame of the last six
            const int f = a.obs_frame[s + i], off = entry_offset(fs, csr, s + i);
            if (off < 0) continue;
            const long long id = a.idkf[f];
            if (id1 - id > 6) continue;
            if (place0 < 0 || id < id0) { place0 = i; id0 = id; f0 = f; off0 = off; }
        }
        status = 3;
        if (f0 == fnew) break;                                         // a ray against itself: no parallax, age 0
        const float* Tcw0 = fr.Tcw + 12 * (size_t)f0;
        const float* Tcw1 = fr.Tcw + 12 * (size_t)fnew;
        const float* Twc0 = fr.Twc + 12 * (size_t)f0;
        const float* Twc1 = fr.Twc + 12 * (size_t)fnew;
        const float pt0[2] = {fr.kps_un[off0].x, fr.kps_un[off0].y}, pt1[2] = {fr.kps_un[off1].x, fr.kps_un[off1].y};
        float posW[3], pos0[3], pos1[3];
        triangulate_dlt(pt0, pt1, fr.P + 12 * (size_t)f0, fr.P + 12 * (size_t)fnew, posW);   // :142-146
        se3map(Tcw0, posW, pos0);
        se3map(Tcw1, posW, pos1);
        bool good = false;
        if (pos0[2] >= a.lower && pos0[2] <= a.upper && pos1[2] >= a.lower && pos1[2] <= a.upper) {   // :150
            const float O0[3] = {Twc0[3], Twc0[7], Twc0[11]}, O1[3] = {Twc1[3], Twc1[7], Twc1[11]};
            good = cos_parallax(O0, O1, posW) < 0.9994f;                                              // :153, minDegree 2
        }
        if (!good) {
            if (id1 - id0 >= 6) {                                      // :182-184, MapPoint::setNull (:68-78)
                status = 2;
                if (a.kf_observed)
                    for (int i = 0; i < n; ++i) {
                        const int off = entry_offset(fs, csr, s + i);
                        if (off >= 0) a.kf_observed[off] = 0;
                    }
            }
            break;
        }
        status = 1;
        store3(a.pos + 3 * (size_t)p, posW);                           // :154
        float info0[9], info1[9], infoW[9], R[9];
        se3_to_xyz_info(pos0, Twc0, Tcw1, Twc1, a.fx, info0, info1, nullptr);   // :159
        rot_of(Tcw0, R);
        mat3_at_m_a(R, info0, infoW);                                  // :163-164
        for (int i = 0; i < n; ++i) {                                  // :160-161, :167-177
            const int f = a.obs_frame[s + i], off = entry_offset(fs, csr, s + i);
            if (off < 0) continue;
            float* view = a.obs_view + 3 * (size_t)(s + i);
            float* info = a.obs_info + 9 * (size_t)(s + i);
            if (i == place0) {
                store3(view, pos0);
                store9(info, info0);
            } else if (i == place1) {
                store3(view, pos1);
                store9(info, info1);
            } else {
                const long long id = a.idkf[f];
                if (id == id1 || id == id0) continue;                  // :169
                float posk[3], infok[9];
                se3map(fr.Tcw + 12 * (size_t)f, posW, posk);
                rot_of(fr.Tcw + 12 * (size_t)f, R);
                mat3_a_m_at(R, infoW, infok);
                store3(view, posk);
                store9(info, infok);
            }
        }
    } while (false);
    a.status[p] = status;
    a.pkf0_place[p] = place0;
}

struct CorArgs {
    FrameArgs fr;
    uint8_t* kf_observed;
    const float* view_pos;
    const int* job_prev;
    const int* job_new;
    const float* Tcr;
    const float* Trc;
    const int* matched12;
    const float* local_pos;
    const int* match_idx_mp;
    const int* mp_main_frame;
    const int* mp_main_ftr;
    const int* mp_main_octave;
    const float* mp_normal;
    const float* mp_dist;
    int* inv;
    uint8_t* kind;
    int* src;
    float* view;
    float* info;
    float* new_pos_w;
    float* info_prev;
    int* counts_out;
    int B, m, passes;
    float fx, lower, upper;
};

// inv[b * cap + j] = the greatest i with matched12[b * cap + i] == j; counts_out[5 b + 4] = features j claimed more than once
__global__ __launch_bounds__(128) void k_invert_match(CorArgs a) {
    const int b = blockIdx.y, i = blockIdx.x * 128 + threadIdx.x;
    const int fp = a.job_prev[b], fn = a.job_new[b];
    const FrameSlots fs = a.fr.slots();
    if ((unsigned)fp >= (unsigned)fs.nframes || (unsigned)fn >= (unsigned)fs.nframes) return;
    if (i >= feature_count(fs, fp)) return;
    const int j = a.matched12[(size_t)b * fs.cap + i];
    if (j < 0 || j >= feature_count(fs, fn)) return;
    if (atomicMax(&a.inv[(size_t)b * fs.cap + j], i) >= 0) atomicAdd(&a.counts_out[5 * b + 4], 1);
}

__global__ __launch_bounds__(128) void k_correspd(CorArgs a) {
    const FrameArgs& fr = a.fr;
    const int b = blockIdx.y, j = blockIdx.x * 128 + threadIdx.x;
    const int cap = fr.cap, nframes = fr.nframes;
    int kind = 0, src = -1;
    bool in_row = false;
    if (j < cap) {
        const int fp = a.job_prev[b], fn = a.job_new[b];
        const size_t row = (size_t)b * cap;
        if ((unsigned)fp < (unsigned)nframes && (unsigned)fn < (unsigned)nframes && fp != fn && j < feature_count(fr.slots(), fn)) {
            in_row = true;
            const size_t onew = (size_t)fn * cap + j;
            const bool was_observed = a.kf_observed[onew] != 0;
            const int i = a.inv[row + j];                              // < counts[prev] by k_invert_match
            const size_t oprev = (size_t)fp * cap + (i >= 0 ? i : 0);
            const bool prev_observed = i >= 0 && a.kf_observed[oprev] != 0;
            const float* Tcr = a.Tcr + 12 * (size_t)b;
            float view[3], info[9];
            if ((a.passes & 1) && i >= 0 && prev_observed) {          // LocalMapper.cpp:95-107
                const float I12[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
                const float* vp = a.view_pos + 3 * oprev;
                const float xyz1[3] = {vp[0], vp[1], vp[2]};
                float info0[9];
                se3_to_xyz_info(xyz1, I12, Tcr, a.Trc + 12 * (size_t)b, a.fx, info0, info, nullptr);
                se3map(Tcr, xyz1, view);
                kind = 1;
                src = i;
            }
            if (kind == 0 && (a.passes & 2) && !was_observed) {        // :119-141
                const int q = a.match_idx_mp[row + j];
                if (q >= 0 && q < a.m) {
                    const int fm = a.mp_main_frame[q];
                    const int om = feature_offset(fr.slots(), fm, a.mp_main_ftr[q]);
                    if (om >= 0) {
                        const float pt1[2] = {fr.kps_un[om].x, fr.kps_un[om].y};
                        const float pt2[2] = {fr.kps_un[onew].x, fr.kps_un[onew].y};
                        float x3d[3], posNew[3];
                        triangulate_dlt(pt1, pt2, fr.P + 12 * (size_t)fm, fr.P + 12 * (size_t)fn, x3d);
                        se3map(fr.Tcw + 12 * (size_t)fn, x3d, posNew);
                        const float* nv = a.mp_normal + 3 * (size_t)q;
                        const float normal[3] = {nv[0], nv[1], nv[2]};
                        if (accept_new_observe(posNew, normal, a.mp_main_octave[q], fr.kps_un[onew].octave,
                                               a.mp_dist[2 * (size_t)q], a.mp_dist[2 * (size_t)q + 1]) &&
                            !(posNew[2] > a.upper || posNew[2] < a.lower)) {
                            float infoOld[9];
                            se3_to_xyz_info(posNew, fr.Twc + 12 * (size_t)fn, fr.Tcw + 12 * (size_t)fm,
                                            fr.Twc + 12 * (size_t)fm, a.fx, info, infoOld, nullptr);
                            view[0] = posNew[0]; view[1] = posNew[1]; view[2] = posNew[2];
                            kind = 2;
                            src = q;
                        }
                    }
                }
            }
            if (kind == 0 && (a.passes & 4) && !was_observed && i >= 0 && !prev_observed) {   // :145-168
                const float* lp = a.local_pos + 3 * (row + i);
                const float xyz1[3] = {lp[0], lp[1], lp[2]};
                float posW[3], infoPrev[9];
                se3map(fr.Twc + 12 * (size_t)fp, xyz1, posW);
                se3map(Tcr, xyz1, view);
                se3_to_xyz_info(xyz1, fr.Twc + 12 * (size_t)fp, fr.Tcw + 12 * (size_t)fn, fr.Twc + 12 * (size_t)fn, a.fx,
                                infoPrev, info, nullptr);
                store3(a.new_pos_w + 3 * (row + j), posW);
                store9(a.info_prev + 9 * (row + j), infoPrev);
                a.kf_observed[oprev] = 1;
                kind = 3;
                src = i;
            }
            if (kind) {
                store3(a.view + 3 * (row + j), view);
                store9(a.info + 9 * (row + j), info);
                a.kf_observed[onew] = 1;
            }
        }
        a.kind[row + j] = (uint8_t)kind;
        a.src[row + j] = src;
    }
    for (int k = 0; k < 4; ++k) {                                      // one atomic per wave and kind
        const unsigned long long bal = __ballot(in_row && kind == k);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&a.counts_out[5 * b + k], __popcll(bal));
    }
}

}  // namespace

extern "C" int se2gpu_mappoint_parallax_batch_device(se2gpu_matcher* h, const se2gpu_keypoint* d_kps_un,
                                                     const int32_t* d_counts, int cap, int nframes,
                                                     const float* d_frame_Tcw, const float* d_frame_Twc,
                                                     const float* d_frame_P, const int32_t* d_frame_idkf,
                                                     const int32_t* d_mp_ptr, const int32_t* d_obs_frame,
                                                     const int32_t* d_obs_ftr, int m, int nobs, const uint8_t* d_good_prl,
                                                     const int32_t* d_new_frame, float fx, float lower_depth,
                                                     float upper_depth, uint8_t* d_kf_observed, int32_t* d_status,
                                                     int32_t* d_pkf0_place, float* d_pos, float* d_obs_view,
                                                     float* d_obs_info) {
    const char* who = "mappoint_parallax_batch";
    SE2_NEED(h);
    SE2_CHECK(check_obs_csr(who, d_mp_ptr, d_obs_frame, d_obs_ftr, m, nobs));
    SE2_NEED(d_kps_un); SE2_NEED(d_frame_Tcw); SE2_NEED(d_frame_Twc); SE2_NEED(d_frame_P);
    SE2_CHECK(check_frame_slots(who, d_counts, cap, nframes));
    SE2_NEED(d_frame_idkf); SE2_NEED(d_good_prl); SE2_NEED(d_new_frame);
    SE2_NEED(d_status); SE2_NEED(d_pkf0_place); SE2_NEED(d_pos);
    SE2_NEED_IF(nobs > 0, d_obs_view); SE2_NEED_IF(nobs > 0, d_obs_info);
    if (m == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    PrlArgs a;
    a.fr = FrameArgs{d_kps_un, d_counts, d_frame_Tcw, d_frame_Twc, d_frame_P, cap, nframes};
    a.idkf = d_frame_idkf; a.mp_ptr = d_mp_ptr; a.obs_frame = d_obs_frame; a.obs_ftr = d_obs_ftr; a.m = m; a.nobs = nobs;
    a.good_prl = d_good_prl; a.new_frame = d_new_frame; a.kf_observed = d_kf_observed;
    a.status = d_status; a.pkf0_place = d_pkf0_place; a.pos = d_pos; a.obs_view = d_obs_view; a.obs_info = d_obs_info;
    a.fx = fx; a.lower = lower_depth; a.upper = upper_depth;
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    hipLaunchKernelGGL(k_parallax, dim3(((unsigned)m + 127u) / 128u), dim3(128), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

extern "C" int se2gpu_kf_correspd_batch_device(se2gpu_matcher* h, const se2gpu_keypoint* d_kps_un, const int32_t* d_counts,
                                               int cap, int nframes, const float* d_frame_Tcw, const float* d_frame_Twc,
                                               const float* d_frame_P, uint8_t* d_kf_observed, const float* d_view_pos,
                                               const int32_t* d_job_prev, const int32_t* d_job_new, const float* d_Tcr,
                                               const float* d_Trc, const int32_t* d_matched12, const float* d_local_pos,
                                               const int32_t* d_match_idx_mp, int B, const int32_t* d_mp_main_frame,
                                               const int32_t* d_mp_main_ftr, const int32_t* d_mp_main_octave,
                                               const float* d_mp_normal, const float* d_mp_dist, int m, float fx,
                                               float lower_depth, float upper_depth, int passes, int32_t* d_inv,
                                               uint8_t* d_kind, int32_t* d_src, float* d_view, float* d_info,
                                               float* d_new_pos_w, float* d_info_prev, int32_t* d_counts_out) {
    const char* who = "kf_correspd_batch";
    SE2_NEED(h);
    SE2_REQUIRE(B >= 0 && m >= 0, SE2GPU_ERR_INVALID, "%s: bad sizes (B %d, m %d)", who, B, m);
    SE2_REQUIRE(passes >= 1 && passes <= 7, SE2GPU_ERR_INVALID, "%s: passes = %d is outside 1..7", who, passes);
    SE2_NEED(d_kps_un); SE2_NEED(d_frame_Tcw); SE2_NEED(d_frame_Twc); SE2_NEED(d_frame_P);
    SE2_CHECK(check_frame_slots(who, d_counts, cap, nframes));
    SE2_NEED(d_kf_observed); SE2_NEED(d_job_prev); SE2_NEED(d_job_new); SE2_NEED(d_Tcr); SE2_NEED(d_matched12);
    SE2_NEED(d_inv); SE2_NEED(d_kind); SE2_NEED(d_src); SE2_NEED(d_view); SE2_NEED(d_info); SE2_NEED(d_counts_out);
    SE2_REQUIRE(!(passes & 1) || (d_view_pos && d_Trc), SE2GPU_ERR_INVALID, "%s: pass 1 needs d_view_pos and d_Trc", who);
    SE2_REQUIRE(!(passes & 2) || d_match_idx_mp, SE2GPU_ERR_INVALID, "%s: pass 2 needs d_match_idx_mp", who);
    SE2_REQUIRE(!(passes & 2) || m == 0 || (d_mp_main_frame && d_mp_main_ftr && d_mp_main_octave && d_mp_normal && d_mp_dist),
                SE2GPU_ERR_INVALID, "%s: pass 2 needs the map-point table", who);
    SE2_REQUIRE(!(passes & 4) || (d_local_pos && d_new_pos_w && d_info_prev), SE2GPU_ERR_INVALID,
                "%s: pass 3 needs d_local_pos, d_new_pos_w and d_info_prev", who);
    SE2_REQUIRE((long long)B * cap <= INT_MAX && B <= 65535, SE2GPU_ERR_CAPACITY,
                "%s: %d jobs of %d features exceed the limit (65535 jobs, B * cap <= %d)", who, B, cap, INT_MAX);
    if (B == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();
    CorArgs a;
    a.fr = FrameArgs{d_kps_un, d_counts, d_frame_Tcw, d_frame_Twc, d_frame_P, cap, nframes};
    a.kf_observed = d_kf_observed; a.view_pos = d_view_pos; a.job_prev = d_job_prev; a.job_new = d_job_new;
    a.Tcr = d_Tcr; a.Trc = d_Trc; a.matched12 = d_matched12; a.local_pos = d_local_pos; a.match_idx_mp = d_match_idx_mp;
    a.mp_main_frame = d_mp_main_frame; a.mp_main_ftr = d_mp_main_ftr; a.mp_main_octave = d_mp_main_octave;
    a.mp_normal = d_mp_normal; a.mp_dist = d_mp_dist; a.inv = d_inv; a.kind = d_kind; a.src = d_src; a.view = d_view;
    a.info = d_info; a.new_pos_w = d_new_pos_w; a.info_prev = d_info_prev; a.counts_out = d_counts_out;
    a.B = B; a.m = m; a.passes = passes; a.fx = fx; a.lower = lower_depth; a.upper = upper_depth;
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    SE2_HIP(hipMemsetAsync(d_inv, 0xff, (size_t)B * cap * sizeof(int32_t), st));   // -1
    SE2_HIP(hipMemsetAsync(d_counts_out, 0, 5 * (size_t)B * sizeof(int32_t), st));
    const dim3 grid(((unsigned)cap + 127u) / 128u, (unsigned)B);
    hipLaunchKernelGGL(k_invert_match, grid, dim3(128), 0, st, a);
    hipLaunchKernelGGL(k_correspd, grid, dim3(128), 0, st, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}
