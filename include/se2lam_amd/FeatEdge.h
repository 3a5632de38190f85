// Feature constraints on the device - header-only mirror over se2gpu_feat_edge_batch (include/se2gpu.h) of
//   GlobalMapper::CreateFeatEdge(pKFFrom, pKFTo, SE3CnstrOutput)             src/GlobalMapper.cpp:737-779 of the reference
//   GlobalMapper::CreateFeatEdge(pKFFrom, pKFTo, mapMatch, SE3CnstrOutput)   src/GlobalMapper.cpp:781-843
// for a BATCH of key-frame pairs: the two-key-frame bundle adjustment (OptKFPair :847-927 / OptKFPairMatch :929-1032) and
// Sparsifier::DoMarginalizeSE3XYZ on its result, one wave per pair, one call for every pair of a Map::UpdateFeatGraph pass
// (src/Map.cpp:857-889) or every verified loop candidate (GlobalMapper.cpp:300).  The reference builds a g2o graph per pair.
//
// Where each argument comes from in the reference:
//   kf[0], kf[1]   toIsometry3D(pKF->getPose().inv()) of _pKFFrom / _pKFTo: T_w_c                             :860-861, :940-946
//   Tbc, xrotInfo, yrotInfo, zInfo
//                  Config::bTc and Config::PLANEMOTION_XROT_INFO / _YROT_INFO / _Z_INFO of addVertexSE3PlaneMotion
//                  (src/optimizer.cpp:336-470); key frame 0 is fixed in the covisibility form only              :864-867, :942-947
//   mp[j]          toVector3d(pMP->getPos()): the start value of point j; compareViewMPs' set (:742) or, per
//                  match, the point key frame 1 observes (:960-969)                                              :877, :968
//   z[j][k], info[j][k]
//                  pKF->mViewMPs[idx] and pKF->mViewMPsInfo[idx] of key frame k for point j                      :898-899, :971-976
//   huberDelta     the last argument of addEdgeSE3XYZ                                                            :901, :973, :977
//   iters          optimizer.optimize(15) / optimize(30)                                                         :911, :985
//   minPoints      numMinMPs = 10 on spMPs.size() / mapMatch.size() < 3 - on the RAW match count: OptKFPairMatch
//                  erases nothing from mapMatch                                                                  :747-750, :790
//   outlierChi2    dThreshChi2 = 5.0 on EdgeSE3PointXYZ::chi2() of either edge of a point                        :989-1003
// The result per pair: status (the reference's return value: 0 = SE3CnstrOutput written, 1 = too few points; 2 = a
// non-finite result, which the reference would have stored), the SE3Constraint, and what OptKFPair(Match) returned.
// SelectKFPairFeat, Map::compareViewMPs and Map::mergeLoopClose stay with the caller.
#pragma once
#include <cstdint>
#include <vector>

#include "../se2gpu.h"
#include "Covisibility.h"
#include "optimizer.h"
#include "types.h"

namespace se2lam_amd {

struct SE3Constraint {          // KeyFrame.h:23-33 (cv::Mat measure 4x4, info 6x6) in double
    SE3Quat measure;            // T_from_to = KF0^-1 KF1
    Matrix6d info;              // order (translation, rotation)
};

// the reference's constants
constexpr int kFeatEdgeCovisIters = 15;         // GlobalMapper.cpp:911
constexpr int kFeatEdgeCovisMinPoints = 10;     // :747
constexpr int kFeatEdgeMatchIters = 30;         // :985
constexpr int kFeatEdgeMatchMinPoints = 3;      // :790
constexpr double kFeatEdgeHuberDelta = 5.99;    // :901
constexpr double kFeatEdgeOutlierChi2 = 5.0;    // :989

// POD view of a batch: pair p has the points [mp_ptr[p], mp_ptr[p+1])
struct FeatEdgeView {
    int32_t npairs = 0;
    const double* kf12 = nullptr;       // npairs x 2 x 12: rotation row-major, translation (T_w_c)
    const int32_t* mp_ptr = nullptr;    // npairs + 1
    const double* mp_xyz = nullptr;     // per point 3
    const double* m_z = nullptr;        // per point 2 x 3 (key frame 0, key frame 1)
    const double* m_info = nullptr;     // per point 2 x 9, row-major
};

struct FeatEdgeParams {
    double Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    double xrotInfo = 1e6, yrotInfo = 1e6, zInfo = 1;     // src/Config.cpp:46-48
    double huberDelta = kFeatEdgeHuberDelta;
    double outlierChi2 = kFeatEdgeOutlierChi2;
};

struct FeatEdgeResult {
    std::vector<int32_t> status, nPoints, nOutliers, nSparsified;     // per pair
    std::vector<SE3Constraint> constraint;                            // per pair (zero unless status == 0)
    std::vector<SE3Quat> kf;                                          // per pair x 2: vSe3KFs
    std::vector<Vector3D> mp;                                         // per point: the optimised points, outliers included
    std::vector<uint8_t> outlier;                                     // per point: sIdMPin1Outlier
    std::vector<double> edgeChi2;                                     // per point x 2
    std::vector<se2gpu_ba_stats> stats;                               // per pair
};

inline void CreateFeatEdgeBatch(const FeatEdgeView& v, int mode, int iters, int minPoints, const FeatEdgeParams& par,
                                FeatEdgeResult& out) {
    const size_t n = v.npairs > 0 ? (size_t)v.npairs : 0;
    const size_t np = n && v.mp_ptr ? (size_t)v.mp_ptr[n] : 0;
    std::vector<double> kf(24 * n + 1), xyz(3 * np + 1), z(12 * n + 1), info(36 * n + 1);
    std::vector<int32_t> info4(4 * n + 1);
    out.outlier.assign(np + 1, 0);
    out.edgeChi2.assign(2 * np + 1, 0.0);
    out.stats.assign(n + 1, se2gpu_ba_stats());
    check(se2gpu_feat_edge_batch(v.npairs, mode, iters, minPoints, v.kf12, par.Tbc12, par.xrotInfo, par.yrotInfo, par.zInfo, v.mp_ptr,
                                 v.mp_xyz, v.m_z, v.m_info, par.huberDelta, par.outlierChi2, kf.data(), xyz.data(), out.outlier.data(),
                                 out.edgeChi2.data(), info4.data(), out.stats.data(), z.data(), info.data()),
          "CreateFeatEdgeBatch");
    out.outlier.resize(np);
    out.edgeChi2.resize(2 * np);
    out.stats.resize(n);
    out.status.resize(n); out.nPoints.resize(n); out.nOutliers.resize(n); out.nSparsified.resize(n);
    out.constraint.resize(n);
    out.kf.resize(2 * n);
    out.mp.resize(np);
    for (size_t p = 0; p < n; ++p) {
        out.status[p] = info4[4 * p]; out.nPoints[p] = info4[4 * p + 1];
        out.nOutliers[p] = info4[4 * p + 2]; out.nSparsified[p] = info4[4 * p + 3];
        out.constraint[p].measure = se3QuatOf(&z[12 * p]);
        for (int i = 0; i < 36; ++i) out.constraint[p].info.m[i] = info[36 * p + i];
        out.kf[2 * p] = se3QuatOf(&kf[24 * p]);
        out.kf[2 * p + 1] = se3QuatOf(&kf[24 * p + 12]);
    }
    for (size_t j = 0; j < np; ++j) out.mp[j] = Vector3D(&xyz[3 * j]);
}

// GlobalMapper::CreateFeatEdge(pKFFrom, pKFTo, SE3CnstrOutput) for every pair of the view: key frame 0 fixed, no rejection
inline void CreateFeatEdgeCovisBatch(const FeatEdgeView& v, const FeatEdgeParams& par, FeatEdgeResult& out,
                                     int iters = kFeatEdgeCovisIters, int minPoints = kFeatEdgeCovisMinPoints) {
    CreateFeatEdgeBatch(v, SE2GPU_FEAT_EDGE_COVIS, iters, minPoints, par, out);
}
// GlobalMapper::CreateFeatEdge(pKFFrom, pKFTo, mapMatch, SE3CnstrOutput): both free, chi2 rejection (par.outlierChi2)
inline void CreateFeatEdgeMatchBatch(const FeatEdgeView& v, const FeatEdgeParams& par, FeatEdgeResult& out,
                                     int iters = kFeatEdgeMatchIters, int minPoints = kFeatEdgeMatchMinPoints) {
    CreateFeatEdgeBatch(v, SE2GPU_FEAT_EDGE_MATCH, iters, minPoints, par, out);
}

// ---- The same two calls on the tables where they lie in device memory (se2gpu_feat_edge_batch_device): the outputs of
// CovisibilityTable::pairsBatchDevice or LoopVerifier::VerifyBatchDevice go in as they are, nothing passes through the host.
// Where each field comes from in the reference:
//   pairA[p], pairB[p]  the frame slots of _pKFFrom / _pKFTo                                                       :737, :781
//   frameTwc            per slot rows 0-2 of cvu::inv(pKF->getPose()) in float, the table of the parallax call; the gather
//                       turns a row into toIsometry3D's rotation and translation                                   :860-861, :940-946
//   pos                 MapPoint::getPos() per point slot (float, as the parallax call writes it)                  :877, :968
//   covisibility form:  CovisPair / CovisCommon of compareViewMPs(_pKFFrom, _pKFTo, spMPs) - the set becomes vPtrMPs in
//                       ascending point index                                                                     :741-750
//                       obsView / obsInfo: pKF->mViewMPs[idx] / mViewMPsInfo[idx] per CSR entry, the arrays the parallax
//                       call writes                                                                               :898-899
//   match form:         matchesMP = _mapMatchMP as VerifyBatchDevice leaves it: feature i of key frame a -> feature of b
//                       or -1, walked in ascending i (std::map<int,int>)                                          :790, :956
//                       ftrMP[f][idx] = the point slot of pKF->getObservation(idx), -1 without one                :957-965
//                       viewPos / viewInfo: pKF->mViewMPs[idx] / mViewMPsInfo[idx] per feature                    :971-976
// The reference indexes vIdMPin1 by the match counter and the points by the kept-point counter (:956-962 against :1000); this
// library does not reproduce that: a point's outlier flag is that point's.
// d_info8 per pair: FeatEdgeDeviceInfo.  rowCap = the point slots of a pair in the per-point outputs (mpXyz, outlier,
// edgeChi2: may be null).  ws: wsBytes() bytes of device memory, no initialisation.  Asynchronous on the matcher's stream.
struct FeatEdgeDeviceInfo {
    int32_t status, nPoints, nOutliers, nSparsified;   // as FeatEdgeResult
    int32_t nRaw;        // spMPs.size() / mapMatch.size(): what minPoints is tested against                        :747, :790
    int32_t nDropped;    // entries with an index out of range / matches without both map points
    int32_t cut;         // 1: listCap or rowCap truncated the pair
    int32_t reserved;
};
static_assert(sizeof(FeatEdgeDeviceInfo) == 32, "the 8 ints of the C ABI");

struct FeatEdgeDeviceTable {
    int nframes = 0, M = 0, rowCap = 0;
    const float* frameTwc = nullptr;        // nframes x 12
    const float* pos = nullptr;             // M x 3
    // covisibility form
    int nobs = 0;
    const float* obsView = nullptr;         // nobs x 3
    const float* obsInfo = nullptr;         // nobs x 9
    // match form
    int cap = 1;
    const int32_t* counts = nullptr;        // nframes
    const int32_t* ftrMP = nullptr;         // nframes x cap
    const float* viewPos = nullptr;         // nframes x cap x 3
    const float* viewInfo = nullptr;        // nframes x cap x 9
    // work space and outputs (device memory, the caller's)
    void* ws = nullptr;
    FeatEdgeDeviceInfo* info = nullptr;     // npairs
    double* kf12 = nullptr;                 // npairs x 24
    double* z12 = nullptr;                  // npairs x 12
    double* info36 = nullptr;               // npairs x 36
    double* mpXyz = nullptr;                // npairs x rowCap x 3, may be null
    uint8_t* outlier = nullptr;             // npairs x rowCap, may be null
    double* edgeChi2 = nullptr;             // npairs x rowCap x 2, may be null
    se2gpu_ba_stats* stats = nullptr;       // npairs, may be null

    long long wsBytes(int npairs) const { return se2gpu_feat_edge_ws_bytes(npairs, rowCap); }

    // CreateFeatEdge(pKFFrom, pKFTo, SE3CnstrOutput) for the pairs CovisibilityTable::pairsBatchDevice was given
    void CreateFeatEdgeCovisBatchDevice(ORBmatcher& matcher, const int32_t* pairA, const int32_t* pairB, int npairs,
                                        const CovisPair* pairOut, const CovisCommon* common, int listCap, const FeatEdgeParams& par,
                                        int iters = kFeatEdgeCovisIters, int minPoints = kFeatEdgeCovisMinPoints) {
        check(se2gpu_feat_edge_batch_device(matcher.handle(), SE2GPU_FEAT_EDGE_COVIS, iters, minPoints, par.huberDelta, par.outlierChi2,
                                            par.Tbc12, par.xrotInfo, par.yrotInfo, par.zInfo, pairA, pairB, npairs, nframes, frameTwc,
                                            pos, M, rowCap, reinterpret_cast<const int32_t*>(pairOut),
                                            reinterpret_cast<const int32_t*>(common), listCap, obsView, obsInfo, nobs, nullptr, nullptr,
                                            cap, nullptr, nullptr, nullptr, ws, reinterpret_cast<int32_t*>(info), kf12, z12, info36,
                                            mpXyz, outlier, edgeChi2, stats),
              "FeatEdgeDeviceTable::CreateFeatEdgeCovisBatchDevice");
    }
    // CreateFeatEdge(pKFFrom, pKFTo, mapMatch, SE3CnstrOutput) for the pairs LoopVerifier::VerifyBatchDevice was given
    void CreateFeatEdgeMatchBatchDevice(ORBmatcher& matcher, const int32_t* pairA, const int32_t* pairB, int npairs,
                                        const int32_t* matchesMP, const FeatEdgeParams& par, int iters = kFeatEdgeMatchIters,
                                        int minPoints = kFeatEdgeMatchMinPoints) {
        check(se2gpu_feat_edge_batch_device(matcher.handle(), SE2GPU_FEAT_EDGE_MATCH, iters, minPoints, par.huberDelta, par.outlierChi2,
                                            par.Tbc12, par.xrotInfo, par.yrotInfo, par.zInfo, pairA, pairB, npairs, nframes, frameTwc,
                                            pos, M, rowCap, nullptr, nullptr, 1, nullptr, nullptr, nobs, matchesMP, counts, cap, ftrMP,
                                            viewPos, viewInfo, ws, reinterpret_cast<int32_t*>(info), kf12, z12, info36, mpXyz, outlier,
                                            edgeChi2, stats),
              "FeatEdgeDeviceTable::CreateFeatEdgeMatchBatchDevice");
    }
};

}  // namespace se2lam_amd
