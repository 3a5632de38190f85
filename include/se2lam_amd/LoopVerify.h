// Loop verification on the device - header-only mirror over the C ABI (include/se2gpu.h) of what follows SearchByBoW in
//   GlobalMapper::VerifyLoopClose   src/GlobalMapper.cpp:256-326 of the reference (RemoveMatchOutlierRansac :1207-1248,
//                                   RemoveKPMatch :1251-1276)
//   Localizer::VerifyLoopClose      src/Localizer.cpp:394-431 of the reference (RemoveMatchOutlierRansac :571-612)
// for a batch of key-frame pairs whose frames and match rows lie in device memory (ORBmatcher::SearchByBoWBatchDevice writes
// the rows).  The reference verifies one candidate at a time on the host; here every pair of the batch goes through the same
// five launches and the host sees 8 ints per pair.  The verified pairs' CreateFeatEdge is CreateFeatEdgeMatchBatch of FeatEdge.h;
// Map::mergeLoopClose stays with the caller.
#pragma once
#include <cstdint>

#include "../se2gpu.h"
#include "ORBmatcher.h"
#include "types.h"

namespace se2lam_amd {

// one pair's record as se2gpu_track_loop_verify_batch_device writes it (8 ints)
struct LoopVerifyInfo {
    int32_t nRaw;         // _mapMatchRaw.size() among the first counts[a] features, values inside frame b
    int32_t nGood;        // _mapMatchGood.size(): survivors of RemoveMatchOutlierRansac
    int32_t nGoodMP;      // _mapMatchMP.size(): survivors of RemoveKPMatch (0 when no map-point flags were given)
    int32_t nMPsCurr;     // mpKFCurr->getAllObsMPs().size()
    int32_t path;         // 0 = fewer than 10 raw matches, nothing survives; 1 = LMedS (10..14); 2 = RANSAC
    int32_t bestSample;   // as se2gpu_track_last_ransac; -1, -1, 0 on path 0
    int32_t bestModel;
    int32_t iterations;
};
static_assert(sizeof(LoopVerifyInfo) == 8 * sizeof(int32_t), "LoopVerifyInfo is the 8 ints of the C ABI");

// GlobalMapper.cpp:295-297 with Config::GM_VCL_NUM_MIN_MATCH_MP / _KP / GM_VCL_RATIO_MIN_MATCH_MP.  The ratio is the
// reference's floating-point division: 0 / 0 is NaN and fails the comparison, n / 0 is +inf and passes it.
inline bool verifiedGlobalMapper(const LoopVerifyInfo& r, int numMinMatchMP, int numMinMatchKP, double ratioMinMatchMP) {
    const double ratioMPMatched = r.nGoodMP * 1.0 / r.nMPsCurr;
    return r.nGoodMP >= numMinMatchMP && r.nGood >= numMinMatchKP && ratioMPMatched >= ratioMinMatchMP;
}

// Localizer.cpp:403, 421
inline bool verifiedLocalizer(const LoopVerifyInfo& r, int numMinMatch = 45) { return r.nGood >= numMinMatch; }

class LoopVerifier {
public:
    LoopVerifier() { check(se2gpu_track_create(&h_), "se2gpu_track_create"); }
    ~LoopVerifier() { se2gpu_track_destroy(h_); }
    LoopVerifier(const LoopVerifier&) = delete;
    LoopVerifier& operator=(const LoopVerifier&) = delete;

    // d_hasMapPoint (frames.nframes * frames.cap bytes), d_numMPs (frames.nframes) and d_matchesMP may be null; every
    // pointer is device memory, d_matches12 / d_matchesGood / d_matchesMP are npairs rows of frames.cap ints, d_info npairs
    // LoopVerifyInfo.  The positions tested are frames.kps (the reference passes keyPointsUn).  Asynchronous on this
    // object's stream: sync() before the outputs are read; give the matcher and this object one stream (setStream) and
    // the two batch calls follow each other without a host wait.
    void VerifyBatchDevice(const DeviceFrameSet& frames, const uint8_t* d_hasMapPoint, const int32_t* d_numMPs,
                           const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs, const int32_t* d_matches12,
                           int32_t* d_matchesGood, int32_t* d_matchesMP, LoopVerifyInfo* d_info) {
        check(se2gpu_track_loop_verify_batch_device(h_, reinterpret_cast<const se2gpu_keypoint*>(frames.kps), frames.counts,
                                                    frames.cap, frames.nframes, d_hasMapPoint, d_numMPs, d_pair_a, d_pair_b,
                                                    npairs, d_matches12, d_matchesGood, d_matchesMP,
                                                    reinterpret_cast<int32_t*>(d_info)),
              "LoopVerifier::VerifyBatchDevice");
    }
    void sync() { check(se2gpu_track_sync(h_), "LoopVerifier::sync"); }
    void setStream(void* hipStream) { check(se2gpu_track_set_stream(h_, hipStream), "LoopVerifier::setStream"); }
    void* stream() { return se2gpu_track_stream(h_); }

private:
    se2gpu_track* h_ = nullptr;
};

}  // namespace se2lam_amd
