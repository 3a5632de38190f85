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

}  // namespace se2lam_amd
