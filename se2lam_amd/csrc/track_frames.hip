// Track::removeOutliers followed by Track::doTriangulate (src/Track.cpp:308-344, 378-419 of the reference) for a batch of
// (reference key frame, current frame) pairs whose frames and MatchByWindow rows lie in HBM: se2gpu_track_frames_batch_device.
// The epipolar filter is the launch sequence of the loop verification (ransac.hip, lv_filter_batch) run without map-point flags:
// it leaves the surviving rows in d_matched12 and its 8 info words per pair in d_info.  k_track_frames then finishes both in
// place, one workgroup per pair, the threads striding over the features:
//   fewer than 10 inliers    the row becomes -1 (Track.cpp:337-340)
//   flag bit 0               the row stays as filtered, no position is formed (Track.cpp:379-381)
//   otherwise per surviving match: the key frame's own map point where it has one (Track.cpp:394-398), else triangulate_dlt,
//   Config::acceptDepth and cvu::checkParallax in the words of k_triangulate (triangulate.hip), so a position and a flag equal
//   the single call's bit for bit.
// Every word of the three output rows is written.  The counts are ballots added per wave and summed through LDS: no global
// atomic, no memset in front, and the same result in every run.
// Compiled with -ffp-contract=off like triangulate.hip.
#include <algorithm>

#include "track_ws.h"
#include "view_info.h"

namespace se2gpu {
namespace {

constexpr int kTfMinInliers = 10;   // Track.cpp:338
constexpr int kTfCounters = 4;      // tracked old, good parallax, rejected by depth, observed features of the key frame

struct TfArgs {
    const se2gpu_keypoint* kps;
    const int32_t* counts;
    const uint8_t* kf_observed;
    const float* view_pos;
    const int32_t *pair_ref, *pair_cur;
    const float *Trc, *P;
    const uint8_t* pair_flags;
    int32_t* matched12;
    float* local_pos;
    uint8_t* good_prl;
    int32_t* info;
    float P_ref[12];
    float lower, upper, min_cos;
    int cap, nframes;
};

// info[p] on entry = what k_lv_select wrote: {n_raw, n_good, ., ., path, ...}
__global__ __launch_bounds__(256) void k_track_frames(const TfArgs a) {
    __shared__ int s_cnt[4][kTfCounters];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cap = a.cap;
    int32_t* info = a.info + (size_t)p * 8;
    const int n_raw = info[0], n_good = info[1], path = info[4];
    const int fa = a.pair_ref[p], fb = a.pair_cur[p];
    const bool ok = fa >= 0 && fa < a.nframes && fb >= 0 && fb < a.nframes;
    const int na = ok ? min(max(a.counts[fa], 0), cap) : 0, nb = ok ? min(max(a.counts[fb], 0), cap) : 0;
    const bool dropped = n_good < kTfMinInliers;
    const bool skipped = a.pair_flags && (a.pair_flags[p] & 1);
    const int status = !ok ? 1 : dropped ? 2 : skipped ? 3 : 0;
    const size_t fa0 = (size_t)(ok ? fa : 0) * cap, fb0 = (size_t)(ok ? fb : 0) * cap;
    float P2[12];
    for (int k = 0; k < 12; ++k) P2[k] = a.P[(size_t)p * 12 + k];
    const float* Trc = a.Trc + (size_t)p * 12;
    const float ox = Trc[3], oy = Trc[7], oz = Trc[11];   // Ocam = cvu::inv(Tcr).rowRange(0,3).col(3)
    int32_t* row = a.matched12 + (size_t)p * cap;
    float* lp = a.local_pos + (size_t)p * cap * 3;
    uint8_t* gp = a.good_prl + (size_t)p * cap;
    int n_old = 0, n_prl = 0, n_rej = 0, n_obs = 0;   // the same in every lane of a wave
    for (int c0 = 0; c0 < cap; c0 += 256) {
        const int i = c0 + tid;
        int m = -1;
        bool obs = false;
        if (i < na) {
            obs = a.kf_observed && a.kf_observed[fa0 + i] != 0;
            if (!dropped) {
                m = row[i];
                if (m < 0 || m >= nb) m = -1;
            }
        }
        float px = 0.f, py = 0.f, pz = 0.f;
        bool old = false, good = false, rej = false;
        if (m >= 0 && !skipped) {
            if (obs) {   // Track.cpp:394-398: the key frame's map point stands for the feature
                const float* v = a.view_pos + (fa0 + i) * 3;
                px = v[0]; py = v[1]; pz = v[2];
                old = true;
            } else {
                const float pt1[2] = {a.kps[fa0 + i].x, a.kps[fa0 + i].y}, pt2[2] = {a.kps[fb0 + m].x, a.kps[fb0 + m].y};
                float x3d[3];
                triangulate_dlt(pt1, pt2, a.P_ref, P2, x3d);   // view_info.h
                if (x3d[2] >= a.lower && x3d[2] <= a.upper) {
                    px = x3d[0]; py = x3d[1]; pz = x3d[2];
                    // checkParallax(o1 = 0, o2 = Ocam, pt3 = pos), as k_triangulate states it
                    const float q0 = px - ox, q1 = py - oy, q2 = pz - oz;
                    const float dotf = px * q0 + py * q1 + pz * q2;
                    const double dot = (double)dotf;
                    const double n1 = sqrt((double)px * px + (double)py * py + (double)pz * pz);
                    const double n2 = sqrt((double)q0 * q0 + (double)q1 * q1 + (double)q2 * q2);
                    const float cosp = (float)(fabs(dot) / (n1 * n2));
                    good = cosp < a.min_cos;
                } else {
                    m = -1;   // Track.cpp:413-415
                    rej = true;
                }
            }
        }
        if (i < cap) {
            row[i] = m;
            lp[3 * (size_t)i] = px;
            lp[3 * (size_t)i + 1] = py;
            lp[3 * (size_t)i + 2] = pz;
            gp[i] = good ? 1 : 0;
        }
        n_old += __popcll(__ballot(old));
        n_prl += __popcll(__ballot(good));
        n_rej += __popcll(__ballot(rej));
        n_obs += __popcll(__ballot(obs));
    }
    if (lane == 0) {
        s_cnt[wv][0] = n_old; s_cnt[wv][1] = n_prl; s_cnt[wv][2] = n_rej; s_cnt[wv][3] = n_obs;
    }
    __syncthreads();   // also: every thread has read info[] by now
    if (tid == 0) {
        int t[kTfCounters];
        for (int k = 0; k < kTfCounters; ++k) t[k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
        info[0] = n_raw;
        info[1] = dropped ? 0 : n_good;
        info[2] = t[0];
        info[3] = t[1];
        info[4] = t[3];
        info[5] = path;
        info[6] = t[2];
        info[7] = status;
    }
}

}  // namespace
}  // namespace se2gpu

using namespace se2gpu;

extern "C" int se2gpu_track_frames_batch_device(se2gpu_track* h, const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap,
                                                int nframes, const uint8_t* d_kf_observed, const float* d_view_pos,
                                                const int32_t* d_pair_ref, const int32_t* d_pair_cur, int npairs,
                                                const float* d_Trc, const float* d_P, const uint8_t* d_pair_flags,
                                                const float* P_ref, const int32_t* d_matches12, float lower_depth,
                                                float upper_depth, int min_degree, int32_t* d_matched12, float* d_local_pos,
                                                uint8_t* d_good_prl, int32_t* d_info) {
    // the argument checks touch neither the handle nor a device
    SE2_REQUIRE(h && d_kps_un && d_counts && d_pair_ref && d_pair_cur && d_Trc && d_P && P_ref && d_matches12 && d_matched12 &&
                    d_local_pos && d_good_prl && d_info,
                SE2GPU_ERR_INVALID, "track_frames_batch: NULL argument");
    SE2_REQUIRE(!d_kf_observed || d_view_pos, SE2GPU_ERR_INVALID, "track_frames_batch: d_kf_observed without d_view_pos");
    SE2_REQUIRE(npairs >= 1 && cap >= 1 && nframes >= 1, SE2GPU_ERR_INVALID, "track_frames_batch: bad sizes");
    SE2_REQUIRE(min_degree >= 1 && min_degree <= 4, SE2GPU_ERR_INVALID, "track_frames_batch: minDegree must be 1..4");
    SE2_REQUIRE(cap <= kLvMaxCap, SE2GPU_ERR_CAPACITY, "track_frames_batch: cap %d exceeds the limit %d", cap, kLvMaxCap);
    SE2_REQUIRE(npairs <= kLvMaxPairs, SE2GPU_ERR_CAPACITY, "track_frames_batch: %d pairs exceed the limit %d", npairs, kLvMaxPairs);
    // removeOutliers: the surviving rows go to d_matched12, the filter's info words to d_info
    SE2_CHECK(lv_filter_batch(h, d_kps_un, d_counts, cap, nframes, nullptr, nullptr, d_pair_ref, d_pair_cur, npairs, d_matches12,
                              d_matched12, nullptr, d_info));
    const float minCos[4] = {0.9998f, 0.9994f, 0.9986f, 0.9976f};   // cvutil.cpp:96
    TfArgs a;
    a.kps = d_kps_un; a.counts = d_counts; a.kf_observed = d_kf_observed; a.view_pos = d_view_pos;
    a.pair_ref = d_pair_ref; a.pair_cur = d_pair_cur; a.Trc = d_Trc; a.P = d_P; a.pair_flags = d_pair_flags;
    a.matched12 = d_matched12; a.local_pos = d_local_pos; a.good_prl = d_good_prl; a.info = d_info;
    std::copy(P_ref, P_ref + 12, a.P_ref);
    a.lower = lower_depth; a.upper = upper_depth; a.min_cos = minCos[min_degree - 1];
    a.cap = cap; a.nframes = nframes;
    hipLaunchKernelGGL(k_track_frames, dim3(npairs), dim3(256), 0, h->stream, a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}
