// Pose-only bundle adjustment of se2lam::Localizer on the device - header-only mirror over the C ABI (include/se2gpu.h).
//   Localizer::DoLocalBA           /root/reference/src/Localizer.cpp:233-302
//   addPlaneMotionSE3Expmap        /root/reference/src/optimizer.cpp:236-314   (+ EdgeSE3ExpmapPrior :159-197)
// The reference builds a g2o graph on the heap for every call (one VertexSE3Expmap, the observed map points as fixed
// vertices, one EdgeProjectXYZ2UV each, the plane-motion prior) and runs optimize(30); here the observations go down
// as three flat arrays and the whole optimisation is one kernel launch.  Two routes:
//   LocalizerBA::DoLocalBA             host arrays in, one pose out (se2gpu_track_pose_ba).  On this route the caller collects
//                                      the observations of mpKFCurr (Localizer.cpp:257-281: good-parallax map points,
//                                      keyPointsUn[ftrIdx].pt, mvInvLevelSigma2[octave]) and writes the pose back (:298-299).
//   LocalizerBA::DoLocalBABatchDevice  a batch of frames on the map's tables in device memory (LocalizerDeviceTable,
//                                      se2gpu_localizer_ba_batch_device): the renewal of MatchLocalMap (:220-227), the
//                                      numMPCurr > 30 gate (:95-98), the collecting, the prior, optimize(30) and
//                                      KeyFrame::setPose happen on the device, asynchronously on the matcher's stream.
//                                      Twb is formed in FP64 (the reference uses OpenCV's float Mat arithmetic [3P]): the table
//                                      value may differ from the reference's by float rounding.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../se2gpu.h"
#include "ORBmatcher.h"
#include "types.h"

namespace se2lam_amd {

struct PlaneMotionPrior {
    SE3Quat measurement;     // EdgeSE3ExpmapPrior::setMeasurement
    double information[36];  // row-major 6x6, vector order (rotation, translation)
};

// addPlaneMotionSE3Expmap(opt, pose, vId, extPara): pose = Tcw of the vertex, extPara = Config::bTc;
// infoXrot / infoYrot / infoZ = Config::PLANEMOTION_XROT_INFO / YROT_INFO / Z_INFO
inline PlaneMotionPrior planeMotionSE3Expmap(const SE3Quat& pose, const SE3Quat& bTc, double infoXrot, double infoYrot,
                                             double infoZ) {
    double a[12], b[12], m[12];
    std::memcpy(a, pose.R, sizeof(pose.R)); std::memcpy(a + 9, pose.t, sizeof(pose.t));
    std::memcpy(b, bTc.R, sizeof(bTc.R)); std::memcpy(b + 9, bTc.t, sizeof(bTc.t));
    PlaneMotionPrior p;
    check(se2gpu_plane_motion_prior(a, b, infoXrot, infoYrot, infoZ, m, p.information), "se2gpu_plane_motion_prior");
    std::memcpy(p.measurement.R, m, sizeof(p.measurement.R));
    std::memcpy(p.measurement.t, m + 9, sizeof(p.measurement.t));
    return p;
}

// d_status of se2gpu_localizer_ba_batch_device
enum LocalizerBAStatus : int32_t {
    kLocalizerBARun = 0,            // gathered, run, written back
    kLocalizerBAOutOfRange = 1,     // the frame slot is outside the table
    kLocalizerBATooFew = 5,         // n_obs <= minObs: not run, d_pose_out is the start pose, the tables are left alone
    kLocalizerBANonFinite = 6,      // run, the pose came out non-finite and was not written back
};

// d_info of the C ABI
struct LocalizerBAInfo {
    int32_t nFeatures, nObs, nEdges, renewed, duplicates, flags, zero0, zero1;   // flags: bit 0 an entry outside -1..M-1, bit 1 an octave
};
static_assert(sizeof(LocalizerBAInfo) == 8 * sizeof(int32_t), "the ints of the C ABI");

struct LocalizerBAParams {
    float fx = 0.f, cx = 0.f, cy = 0.f;      // Config::Kcam
    double Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // Config::bTc: rotation row-major, translation
    double huberDelta = 5.991;               // Config::TH_HUBER
    double xrotInfo = 1e6, yrotInfo = 1e6, zInfo = 1.0;   // Config::PLANEMOTION_*_INFO
    int iters = 30;
    int minObs = 30;                         // -1 = run always (the relocalisation branch, Localizer.cpp:133, :139)
};

// The frame, feature and point tables of a map where they lie in device memory, and the outputs of a batch.  The caller owns
// every array.  The frame slots of a batch must be pairwise distinct.
struct LocalizerDeviceTable {
    int nframes = 0, cap = 0, M = 0, nlevels = 0;
    float* frameTcw = nullptr;               // x 12: rows 0-2 of Tcw, in / out
    float* frameTwb = nullptr;               // x 3, out, may be null
    const se2gpu_keypoint* kpsUn = nullptr;  // nframes x cap
    const int32_t* counts = nullptr;
    int32_t* ftrMP = nullptr;                // nframes x cap: mDualObservations, feature -> point or -1, in / out
    uint8_t* kfObserved = nullptr;           // nframes x cap, in / out, may be null
    const float* pos = nullptr;              // M x 3
    const uint8_t* mpNull = nullptr;         // M, may be null
    const uint8_t* goodPrl = nullptr;        // M, may be null
    const float* invLevelSigma2 = nullptr;   // HOST: mvInvLevelSigma2, nlevels <= 32
    void* ws = nullptr;                      // wsBytes(njobs) bytes, 16-byte aligned, no initialisation
    int32_t* status = nullptr;               // njobs
    double* poseOut = nullptr;               // njobs x 12: R row-major, t
    se2gpu_ba_stats* stats = nullptr;        // njobs, may be null
    LocalizerBAInfo* info = nullptr;         // njobs

    long long wsBytes(int njobs) const { return se2gpu_localizer_ba_ws_bytes(njobs, cap); }
};

class LocalizerBA {
public:
    LocalizerBA() { check(se2gpu_track_create(&h_), "se2gpu_track_create"); }
    ~LocalizerBA() { se2gpu_track_destroy(h_); }
    LocalizerBA(const LocalizerBA&) = delete;
    LocalizerBA& operator=(const LocalizerBA&) = delete;

    // Localizer::DoLocalBA: Tcw = toSE3Quat(mpKFCurr->getPose()); mapPoints[i] = toVector3d(pMP->getPos()),
    // uv[i] = keyPointsUn[ftrIdx].pt, invSigma2[i] = mvInvLevelSigma2[octave] of the i-th good-parallax observation;
    // f, cx, cy from Config::Kcam (addCamPara uses K(0,0) for both axes); thHuber = Config::TH_HUBER.
    // Returns estimateVertexSE3Expmap after optimize(iterations).
    SE3Quat DoLocalBA(const SE3Quat& Tcw, const SE3Quat& bTc, const std::vector<Vector3D>& mapPoints,
                      const std::vector<Vector2D>& uv, const std::vector<double>& invSigma2, double f, double cx, double cy,
                      double thHuber, double infoXrot, double infoYrot, double infoZ, int iterations = 30,
                      se2gpu_ba_stats* stats = nullptr) {
        const PlaneMotionPrior prior = planeMotionSE3Expmap(Tcw, bTc, infoXrot, infoYrot, infoZ);
        double a[12], m[12], out[12];
        std::memcpy(a, Tcw.R, sizeof(Tcw.R)); std::memcpy(a + 9, Tcw.t, sizeof(Tcw.t));
        std::memcpy(m, prior.measurement.R, sizeof(prior.measurement.R));
        std::memcpy(m + 9, prior.measurement.t, sizeof(prior.measurement.t));
        const int n = (int)mapPoints.size();
        if (uv.size() != mapPoints.size() || invSigma2.size() != mapPoints.size())
            throw std::runtime_error("DoLocalBA: observation arrays differ in length");
        check(se2gpu_track_pose_ba(h_, a, m, prior.information, n, n ? mapPoints[0].v : nullptr, n ? uv[0].v : nullptr,
                                   invSigma2.data(), f, cx, cy, thHuber, iterations, out, stats),
              "se2gpu_track_pose_ba");
        SE3Quat r;
        std::memcpy(r.R, out, sizeof(r.R));
        std::memcpy(r.t, out + 9, sizeof(r.t));
        return r;
    }

    // MatchLocalMap's renewal, the gate, DoLocalBA and setPose for njobs frames jobFrame[b] (device memory) of the table.
    // matchIdxMP: njobs x cap, row b as ORBmatcher::MatchByProjection's device call wrote it for job b's frame, or null (no
    // renewal).  Asynchronous on the matcher's stream; matcher.sync() before outputs are read on the host.
    static void DoLocalBABatchDevice(ORBmatcher& matcher, const LocalizerDeviceTable& t, const int32_t* jobFrame, int njobs,
                                     const int32_t* matchIdxMP, const LocalizerBAParams& par) {
        check(se2gpu_localizer_ba_batch_device(matcher.handle(), jobFrame, njobs, t.nframes, t.frameTcw, t.frameTwb, t.kpsUn, t.counts,
                                               t.cap, t.ftrMP, t.kfObserved, matchIdxMP, t.pos, t.M, t.mpNull, t.goodPrl,
                                               t.invLevelSigma2, t.nlevels, par.fx, par.cx, par.cy, par.Tbc12, par.huberDelta,
                                               par.xrotInfo, par.yrotInfo, par.zInfo, par.iters, par.minObs, t.ws, t.status, t.poseOut,
                                               t.stats, reinterpret_cast<int32_t*>(t.info)),
              "LocalizerBA::DoLocalBABatchDevice");
    }

private:
    se2gpu_track* h_ = nullptr;
};

}  // namespace se2lam_amd
