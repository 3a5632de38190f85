// Device workspace of one tracking thread, shared by ransac.hip (removeOutliers, the batched loop verification),
// triangulate.hip (doTriangulate) and track_frames.hip (both, for batches of frame pairs in HBM).
#pragma once
#include "common.h"

struct se2gpu_track;

namespace se2gpu {
constexpr int kLvMaxCap = 64 * 1024;   // the limits of se2gpu_search_by_bow_batch_device
constexpr int kLvMaxPairs = 65535;
// The gather / draw / models / score / select launches of se2gpu_track_loop_verify_batch_device on the handle's stream, in
// slices of the handle's scratch (ransac.hip); the arguments are that call's, already checked by the caller.
int lv_filter_batch(se2gpu_track* h, const se2gpu_keypoint* d_kps, const int32_t* d_counts, int cap, int nframes,
                    const uint8_t* d_has_mp, const int32_t* d_num_mps, const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs,
                    const int32_t* d_matches12, int32_t* d_matches_good, int32_t* d_matches_mp, int32_t* d_info);
}  // namespace se2gpu

struct se2gpu_track {
    hipStream_t own_stream = nullptr, stream = nullptr;   // stream: own_stream, or the one se2gpu_track_set_stream lent
    se2gpu::PinBuf<uint8_t> h_in, h_out;
    se2gpu::DevBuf<uint8_t> d_in, d_out;
    se2gpu::DevBuf<double> d_F, d_score;
    se2gpu::DevBuf<int> d_nm;
    std::vector<int> subsets;   // RANSAC sample indices; depend on the point count only
    int subsets_n = -1;
    std::vector<float> pt1, pt2;
    std::vector<int> idx;
    std::vector<uint8_t> mask;
    int last_info[4] = {0, -1, -1, 0};
    // se2gpu_track_loop_verify_batch_device: the scratch of one slice of pairs (ransac.hip, LvScratch)
    se2gpu::DevBuf<uint32_t> lv_raw;    // head of cv::RNG(-1)'s raw stream, uploaded by the first call
    uint64_t lv_raw_state = 0;          // generator state behind lv_raw
    se2gpu::DevBuf<float2> lv_pts;      // slice x 2 x cap: the matched positions of frame a, then of frame b
    se2gpu::DevBuf<int> lv_slot;        // slice x cap: position of feature i's match in the point lists, -1 = no match
    se2gpu::DevBuf<int> lv_meta;        // slice x 4: {n_raw, path, n_mps_a, samples to run}
    se2gpu::DevBuf<int> lv_sub;         // slice x 1000 x 7 sample indices
    se2gpu::DevBuf<double> lv_F;        // slice x 1000 x 27
    se2gpu::DevBuf<int> lv_nm;          // slice x 1000
    se2gpu::DevBuf<double> lv_score;    // slice x 3000
    se2gpu::DevBuf<uint8_t> lv_mask;    // slice x cap
};
