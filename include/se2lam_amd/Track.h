// Front-end geometry of se2lam::Track on the device - header-only mirror over the C ABI (include/se2gpu.h).
//   Track::removeOutliers  /root/reference/src/Track.cpp:308-344   (cv::findFundamentalMat RANSAC mask, < 10 inliers => none)
//   Track::doTriangulate   /root/reference/src/Track.cpp:378-419   (cvu::triangulate, Config::acceptDepth, cvu::checkParallax)
// The reference loops over the matches on the host, one 4x4 SVD each; here all matches of the frame pair go through one
// kernel.  Map-point bookkeeping (mLocalMPs[i] = mpKF->mViewMPs[i] for features that already have an observation)
// stays with the caller, exactly where the reference has it.
//   TrackGeometry::TrackFramesBatchDevice   both members, one after the other, for a batch of (key frame, frame) pairs whose
//   frames and MatchByWindow rows lie in device memory; the host sees 8 ints per pair (TrackFrameInfo), which is all that the
//   count tests of Track::needNewKF (Track.cpp:346-353) read: needNewKFByCounts.
#pragma once
#include <cstdint>
#include <vector>

#include "../se2gpu.h"
#include "ORBmatcher.h"
#include "types.h"

namespace se2lam_amd {

struct TriangulationResult {
    std::vector<Point3f> localMPs;      // mLocalMPs[i] for the features triangulated now (zero elsewhere)
    std::vector<uint8_t> goodPrl;       // mvbGoodPrl
    int nGoodPrl = 0;                   // mnGoodPrl
    int nTrackedOld = 0;                // return value of Track::doTriangulate
};

// keyPointsUnRef / keyPointsUnCur: undistorted key points of the key frame and of the current frame; matchIdx =
// Track::mMatchIdx (set to -1 where the depth gate rejects the point); hasObservation[i] = mpKF->hasObservation(i);
// PrjMtrxEye = Config::PrjMtrxEye, P = Config::Kcam * mFrame.Tcr.rowRange(0,3) (3x4 row-major float);
// Ocam = translation of cvu::inv(mFrame.Tcr).
inline TriangulationResult doTriangulate(const std::vector<KeyPoint>& keyPointsUnRef,
                                         const std::vector<KeyPoint>& keyPointsUnCur, std::vector<int>& matchIdx,
                                         const std::vector<uint8_t>& hasObservation, const float PrjMtrxEye[12],
                                         const float P[12], const float Ocam[3], float lowerDepth, float upperDepth,
                                         int minDegree = 2) {
    TriangulationResult r;
    const int n = (int)keyPointsUnRef.size();
    r.localMPs.assign(n, Point3f{0, 0, 0});
    r.goodPrl.assign(n, 0);
    if (n == 0) return r;
    check(se2gpu_triangulate(n, reinterpret_cast<const se2gpu_keypoint*>(keyPointsUnRef.data()),
                             reinterpret_cast<const se2gpu_keypoint*>(keyPointsUnCur.data()),
                             (int)keyPointsUnCur.size(), matchIdx.data(),
                             hasObservation.empty() ? nullptr : hasObservation.data(), PrjMtrxEye, P, Ocam, lowerDepth,
                             upperDepth, minDegree, reinterpret_cast<float*>(r.localMPs.data()), r.goodPrl.data(),
                             &r.nGoodPrl, &r.nTrackedOld),
          "se2gpu_triangulate");
    return r;
}

// one pair's record as se2gpu_track_frames_batch_device writes it (8 ints)
struct TrackFrameInfo {
    int32_t nRaw;             // matches of MatchByWindow among the first counts[ref] features, values inside the current frame
    int32_t nMatched;         // return value of Track::removeOutliers (0 when fewer than 10 inliers dropped the row)
    int32_t nTrackedOld;      // return value of Track::doTriangulate
    int32_t nGoodPrl;         // mnGoodPrl
    int32_t nOldKP;           // mpKF->getSizeObsMP() (0 when no observation table was given)
    int32_t path;             // 0 = fewer than 10 raw matches, 1 = LMedS (10..14), 2 = RANSAC
    int32_t nDepthRejected;   // matches Config::acceptDepth dropped
    int32_t status;           // 0 run, 1 frame index out of range, 2 fewer than 10 inliers, 3 triangulation skipped by flag
};
static_assert(sizeof(TrackFrameInfo) == 8 * sizeof(int32_t), "TrackFrameInfo is the 8 ints of the C ABI");

struct NewKFByCounts {
    bool need;       // c0 && ((c1 && c2) || c3 || c4): Track::needNewKF before its odometry tests
    bool abortBA;    // c0 && (c4 || c3): with the odometry test, what makes the reference call setAbortBA
};

// The tests of Track::needNewKF (Track.cpp:346-353) that read counts: frameGap = mFrame.id - mpKF->id, maxFtrNumber =
// Config::MaxFtrNumber.  The odometry tests (c5, c6) and LocalMapper::acceptNewKF stay with the caller.
inline NewKFByCounts needNewKFByCounts(const TrackFrameInfo& r, int frameGap, int nMinFrames, int nMaxFrames, int maxFtrNumber) {
    const bool c0 = frameGap > nMinFrames;
    const bool c1 = (float)r.nTrackedOld <= (float)r.nOldKP * 0.5f;
    const bool c2 = r.nGoodPrl > 40;
    const bool c3 = frameGap > nMaxFrames;
    const bool c4 = r.nMatched < 0.1f * maxFtrNumber || r.nMatched < 20;
    return NewKFByCounts{c0 && ((c1 && c2) || c3 || c4), c0 && (c4 || c3)};
}

// Device workspace of the tracking thread; removeOutliers has the reference's signature and semantics
// (Track.cpp:134: nMatched = removeOutliers(mRefFrame.keyPointsUn, mFrame.keyPointsUn, mMatchIdx)).
class TrackGeometry {
public:
    TrackGeometry() { check(se2gpu_track_create(&h_), "se2gpu_track_create"); }
    ~TrackGeometry() { se2gpu_track_destroy(h_); }
    TrackGeometry(const TrackGeometry&) = delete;
    TrackGeometry& operator=(const TrackGeometry&) = delete;

    int removeOutliers(const std::vector<KeyPoint>& kp1, const std::vector<KeyPoint>& kp2, std::vector<int>& matches) {
        int nInlier = 0;
        check(se2gpu_track_remove_outliers(h_, reinterpret_cast<const se2gpu_keypoint*>(kp1.data()), (int)kp1.size(),
                                           reinterpret_cast<const se2gpu_keypoint*>(kp2.data()), (int)kp2.size(),
                                           matches.data(), &nInlier),
              "se2gpu_track_remove_outliers");
        return nInlier;
    }

    // Track::doTriangulate on this workspace (no allocation per call); arguments as the free function above
    TriangulationResult doTriangulate(const std::vector<KeyPoint>& keyPointsUnRef,
                                      const std::vector<KeyPoint>& keyPointsUnCur, std::vector<int>& matchIdx,
                                      const std::vector<uint8_t>& hasObservation, const float PrjMtrxEye[12],
                                      const float P[12], const float Ocam[3], float lowerDepth, float upperDepth,
                                      int minDegree = 2) {
        TriangulationResult r;
        const int n = (int)keyPointsUnRef.size();
        r.localMPs.assign(n, Point3f{0, 0, 0});
        r.goodPrl.assign(n, 0);
        if (n == 0) return r;
        check(se2gpu_track_triangulate(h_, n, reinterpret_cast<const se2gpu_keypoint*>(keyPointsUnRef.data()),
                                       reinterpret_cast<const se2gpu_keypoint*>(keyPointsUnCur.data()),
                                       (int)keyPointsUnCur.size(), matchIdx.data(),
                                       hasObservation.empty() ? nullptr : hasObservation.data(), PrjMtrxEye, P, Ocam,
                                       lowerDepth, upperDepth, minDegree, reinterpret_cast<float*>(r.localMPs.data()),
                                       r.goodPrl.data(), &r.nGoodPrl, &r.nTrackedOld),
              "se2gpu_track_triangulate");
        return r;
    }

    // cv::findFundamentalMat(pt1, pt2, mask): pt = (x, y) pairs
    int findFundamentalMask(const std::vector<float>& pt1, const std::vector<float>& pt2, std::vector<uint8_t>& mask) {
        const int n = (int)(pt1.size() / 2);
        mask.assign(n, 0);
        int nInlier = 0;
        check(se2gpu_track_fundamental_mask(h_, pt1.data(), pt2.data(), n, mask.data(), &nInlier),
              "se2gpu_track_fundamental_mask");
        return nInlier;
    }

    // removeOutliers and then doTriangulate for npairs pairs (d_pair_ref[p], d_pair_cur[p]) of `frames` (frames.kps = the
    // undistorted key points).  Every d_ pointer is device memory: d_matches12 = the rows ORBmatcher's batched MatchByWindow
    // wrote; d_kfObserved (frames.nframes * frames.cap bytes) with d_viewPos (x 3 floats, mViewMPs) and d_pairFlags (bit 0:
    // mFrame.id - mpKF->id < nMinFrames, no triangulation) may be null; d_Trc / d_P = npairs x 12 floats, rows 0-2 of
    // cvu::inv(Tcr) and Config::Kcam * Tcr.rowRange(0,3).  d_matched12 / d_localPos are what FindCorrespd's batch call reads,
    // d_goodPrl = mvbGoodPrl, d_info npairs TrackFrameInfo.  Asynchronous on this object's stream: sync() before the outputs
    // are read; give the matcher and this object one stream (setStream) and the calls follow each other without a host wait.
    void TrackFramesBatchDevice(const DeviceFrameSet& frames, const uint8_t* d_kfObserved, const float* d_viewPos,
                                const int32_t* d_pair_ref, const int32_t* d_pair_cur, int npairs, const float* d_Trc,
                                const float* d_P, const uint8_t* d_pairFlags, const float PrjMtrxEye[12],
                                const int32_t* d_matches12, float lowerDepth, float upperDepth, int minDegree,
                                int32_t* d_matched12, Point3f* d_localPos, uint8_t* d_goodPrl, TrackFrameInfo* d_info) {
        check(se2gpu_track_frames_batch_device(h_, reinterpret_cast<const se2gpu_keypoint*>(frames.kps), frames.counts, frames.cap,
                                               frames.nframes, d_kfObserved, d_viewPos, d_pair_ref, d_pair_cur, npairs, d_Trc,
                                               d_P, d_pairFlags, PrjMtrxEye, d_matches12, lowerDepth, upperDepth, minDegree,
                                               d_matched12, reinterpret_cast<float*>(d_localPos), d_goodPrl,
                                               reinterpret_cast<int32_t*>(d_info)),
              "TrackGeometry::TrackFramesBatchDevice");
    }
    void sync() { check(se2gpu_track_sync(h_), "TrackGeometry::sync"); }
    void setStream(void* hipStream) { check(se2gpu_track_set_stream(h_, hipStream), "TrackGeometry::setStream"); }
    void* stream() { return se2gpu_track_stream(h_); }

private:
    se2gpu_track* h_ = nullptr;
};

}  // namespace se2lam_amd
