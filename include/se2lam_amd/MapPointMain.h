// MapPoint::updateMainKFandDescriptor (src/MapPoint.cpp:228-292 of the reference) - header-only mirror, C++17:
//   mainObservation(...)                   the function on the host, written as the reference writes it (N x N table, std::sort
//                                          of every row, element (N-1)/2, `median < bestMedian`): the CPU stand-in and the
//                                          baseline tools/mappoint_main_bench.py times
//   MapPointTable::updateMainBatchDevice   the same for a batch of points in device memory (se2gpu_mappoint_main_batch_device)
// Both read the frame arrays se2gpu_orb_extract_batch_device writes (DeviceFrameSet; for the host function the same layout in
// host memory) and a point's observations as (frame, feature) pairs IN THE ORDER THE CALLER'S CONTAINER ITERATES THEM: on equal
// medians the first one wins, so the order is part of the input.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../se2gpu.h"
#include "ORBmatcher.h"
#include "obs_table.h"
#include "types.h"

namespace se2lam_amd {

// d_info of se2gpu_mappoint_main_batch_device, 4 ints per point
struct MainObservationInfo {
    int32_t pos;       // place of the main observation in the point's list, -1: no valid observation (nothing else written)
    int32_t median;    // its median distance
    int32_t N;         // valid observations
    int32_t changed;   // bit 0: mMainKF changed (octave and distances rewritten), bit 1: octave outside the scale factors
};
static_assert(sizeof(MainObservationInfo) == 4 * sizeof(int32_t), "MainObservationInfo is the 4 ints of the C ABI");

inline int descriptorDistance256(const uint8_t* a, const uint8_t* b) {   // ORBmatcher::DescriptorDistance
    int d = 0;
    for (int w = 0; w < 4; ++w) {
        uint64_t x, y;
        std::memcpy(&x, a + 8 * w, 8);
        std::memcpy(&y, b + 8 * w, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

// One point.  Which observations count is obs_table.h's entry rule, the kernels' own text.  frames: HOST arrays in the
// DeviceFrameSet layout; frameNull (nframes bytes), viewMPs (nframes * cap) and
// scaleFactors may be null as in the C ABI.  obsFrame / obsFtr: the point's n observations in container order.
// prevMainFrame: the frame of mMainKF, -1 = none.  mainDescriptor (32 bytes), mainFrame, mainOctave and minMaxDist (2 floats)
// are written under the rules of the C ABI (the last two only when the main key frame changed).
inline MainObservationInfo mainObservation(const DeviceFrameSet& frames, const uint8_t* frameNull, const Point3f* viewMPs,
                                           const float* scaleFactors, int nlevels, const int32_t* obsFrame,
                                           const int32_t* obsFtr, int n, int prevMainFrame, uint8_t* mainDescriptor,
                                           int32_t* mainFrame, int32_t* mainOctave, float* minMaxDist) {
    const se2gpu::FrameSlots slots{frames.counts, frameNull, frames.cap, frames.nframes};
    std::vector<int> vPos;            // vKFs / vDes of :234-246 as places in the list
    std::vector<size_t> vOff;
    vPos.reserve(std::max(n, 0));
    vOff.reserve(std::max(n, 0));
    for (int i = 0; i < n; ++i) {
        const int off = se2gpu::feature_offset(slots, obsFrame[i], obsFtr[i]);   // skips the null key frames (:242)
        if (off < 0) continue;
        vPos.push_back(i);
        vOff.push_back((size_t)off);
    }
    if (vOff.empty()) return MainObservationInfo{-1, 0, 0, 0};        // :248
    const int N = (int)vOff.size();
    std::vector<int> Distances((size_t)N * N);                        // :254-263
    for (int i = 0; i < N; ++i) {
        Distances[(size_t)i * N + i] = 0;
        for (int j = i + 1; j < N; ++j) {
            const int distij = descriptorDistance256(frames.desc + 32 * vOff[i], frames.desc + 32 * vOff[j]);
            Distances[(size_t)i * N + j] = distij;
            Distances[(size_t)j * N + i] = distij;
        }
    }
    int bestMedian = INT_MAX, bestIdx = 0;                            // :266-276
    std::vector<int> vDists(N);
    for (int i = 0; i < N; ++i) {
        std::copy(Distances.begin() + (size_t)i * N, Distances.begin() + (size_t)(i + 1) * N, vDists.begin());
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(N - 1) / 2];                       // vDists[0.5*(N-1)]
        if (median < bestMedian) {
            bestMedian = median;
            bestIdx = i;
        }
    }
    const size_t off = vOff[bestIdx];
    const int frame = obsFrame[vPos[bestIdx]];
    std::memcpy(mainDescriptor, frames.desc + 32 * off, 32);          // :278
    *mainFrame = frame;
    MainObservationInfo r{vPos[bestIdx], bestMedian, N, prevMainFrame != frame ? 1 : 0};
    if (!r.changed) return r;                                         // :280
    const int octave = frames.kps[off].octave;
    *mainOctave = octave;                                             // :285
    if (octave < 0 || octave >= nlevels) {
        r.changed |= 2;
    } else if (viewMPs && scaleFactors) {
        const Point3f& v = viewMPs[off];
        const float dist = (float)std::sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z);   // cv::norm, :287
        const float maxDist = dist * scaleFactors[octave];            // :290
        minMaxDist[0] = maxDist / scaleFactors[nlevels - 1];          // :291
        minMaxDist[1] = maxDist;
    }
    return r;
}

// The map-point side of a batch in device memory: the observation lists in CSR form and the per-point fields the call
// rewrites.  The caller owns every array.
struct MapPointTable {
    int M = 0, nobs = 0;
    const int32_t* mpPtr = nullptr;          // M + 1
    const int32_t* obsFrame = nullptr;       // nobs, container order within a point
    const int32_t* obsFtr = nullptr;         // nobs
    const int32_t* prevMainFrame = nullptr;  // M, -1 = none; null = every point counts as changed
    MainObservationInfo* info = nullptr;     // M
    uint8_t* mainDescriptor = nullptr;       // M x 32  (MapPointView::mainDescriptor of MatchByProjectionDevice)
    int32_t* mainFrame = nullptr;            // M
    int32_t* mainOctave = nullptr;           // M       (MapPointView::mainOctave)
    float* minMaxDist = nullptr;             // M x 2, needed with d_viewMPs

    // Asynchronous on the matcher's stream; matcher.sync() before the outputs are read on the host,
    // matcher.MatchByProjectionDevice right behind it consumes mainDescriptor / mainOctave in place.
    void updateMainBatchDevice(ORBmatcher& matcher, const DeviceFrameSet& frames, const uint8_t* d_frameNull,
                               const Point3f* d_viewMPs, const std::vector<float>& mvScaleFactors) {
        check(se2gpu_mappoint_main_batch_device(matcher.handle(), reinterpret_cast<const se2gpu_keypoint*>(frames.kps),
                                                frames.desc, frames.counts, frames.cap, frames.nframes, d_frameNull,
                                                reinterpret_cast<const float*>(d_viewMPs), mvScaleFactors.data(),
                                                (int)mvScaleFactors.size(), mpPtr, obsFrame, obsFtr, M, nobs, prevMainFrame,
                                                reinterpret_cast<int32_t*>(info), mainDescriptor, mainFrame, mainOctave,
                                                minMaxDist),
              "MapPointTable::updateMainBatchDevice");
    }
};

}  // namespace se2lam_amd
