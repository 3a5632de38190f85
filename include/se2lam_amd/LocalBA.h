// Local bundle adjustment on the map's tables in device memory - header-only mirror, C++17, of
//   Map::loadLocalGraph + LocalMapper::localBA's optimize   src/Map.cpp:891-1053, src/LocalMapper.cpp:232-302
// for batches of windows: LocalBADeviceTable names the frame, feature and point tables where they lie in device memory, and
// LoadAndOptimizeLocalGraphBatchDevice chains se2gpu_local_ba_batch_device to the lists LocalWindowTable::updateLocalGraphBatchDevice
// wrote (LocalWindow.h), on the matcher's stream, without the host in between.  The caller owns every array.
// Write-back into the tables (Map::optimizeLocalGraph, :754-783) is the caller's: windows of a batch overlap.
#pragma once
#include <cstdint>

#include "../se2gpu.h"
#include "LocalWindow.h"
#include "ORBmatcher.h"

namespace se2lam_amd {

// d_status of the C ABI
enum LocalBAStatus : int32_t {
    kLocalBARun = 0,             // gathered and run
    kLocalBAOutOfRange = 1,      // job slot or list entry outside its table
    kLocalBADoesNotFit = 2,      // a cap, more than 64 free key frames, or an odometry self loop
    kLocalBANullKeyFrame = 3,    // a local key frame of the window is null
    kLocalBADegree = 4,          // a landmark with more than 64 edges
    kLocalBANothing = 5,         // no free key frame or no edge: the outputs are the start values
    kLocalBANonFinite = 6,       // run, and a pose or landmark came out non-finite
};

// d_info of the C ABI
struct LocalBAInfo {
    int32_t nPose, nFree, nLm, nEdge, nOdo, skippedEntries, flags, zero;
};
static_assert(sizeof(LocalBAInfo) == 8 * sizeof(int32_t), "the ints of the C ABI");

struct LocalBAParams {
    float fx = 0.f, cx = 0.f, cy = 0.f;      // Config::Kcam
    double Tbc12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // Config::bTc: rotation row-major, translation
    double huberDelta = 5.991;               // Config::TH_HUBER
    double xrotInfo = 1e6, zInfo = 1.0;      // Config::PLANEMOTION_XROT_INFO, PLANEMOTION_Z_INFO
    int iters = 10;                          // Config::LOCAL_ITER
    int mode = SE2GPU_BA_LM;
};

struct LocalBADeviceTable {
    int nframes = 0, cap = 0, M = 0, nobs = 0, nlevels = 0;
    // frame tables
    const int32_t* frameId = nullptr;        // KeyFrame::id
    const float* frameTwb = nullptr;         // x 3
    const float* frameTcw = nullptr;         // x 12: rows 0-2 of Tcw
    const uint8_t* frameNull = nullptr;      // may be null
    const int32_t* odoTo = nullptr;          // preOdomFromSelf: slot of .first or -1; the three may be null together
    const double* odoMeas = nullptr;         // x 3
    const double* odoCov = nullptr;          // x 9
    // feature tables
    const se2gpu_keypoint* kpsUn = nullptr;  // nframes x cap
    const int32_t* counts = nullptr;
    const float* viewPos = nullptr;          // nframes x cap x 3: mViewMPs
    const float* levelSigma2 = nullptr;      // HOST: mvLevelSigma2, nlevels <= 32
    // point tables: positions and MapPoint::mObservations as the CSR of obs_table.h
    const float* pos = nullptr;              // M x 3
    const int32_t* mpPtr = nullptr;
    const int32_t* obsFrame = nullptr;
    const int32_t* obsFtr = nullptr;
    // the sizes the work space and the launch are cut for
    int maxLocal = 0, maxRef = 0, maxMP = 0, maxObs = 0;
    void* ws = nullptr;                      // wsBytes(njobs) bytes, 16-byte aligned, no initialisation
    // outputs
    int32_t* status = nullptr;               // njobs
    double* kfOut = nullptr;                 // njobs x (maxLocal + maxRef) x 3
    double* mpOut = nullptr;                 // njobs x maxMP x 3
    se2gpu_ba_stats* stats = nullptr;        // njobs, may be null
    LocalBAInfo* info = nullptr;             // njobs

    long long wsBytes(int njobs) const { return se2gpu_local_ba_ws_bytes(njobs, maxLocal, maxRef, maxMP, maxObs); }

    // Asynchronous on the matcher's stream; matcher.sync() before outputs are read on the host.
    // out / localList / refList / mpList as LocalWindowTable::updateLocalGraphBatchDevice wrote them for jobKF.
    void LoadAndOptimizeLocalGraphBatchDevice(ORBmatcher& matcher, const int32_t* jobKF, int njobs, const LocalWindowCounts* out,
                                              const int32_t* localList, const int32_t* refList, int kfListCap, const int32_t* mpList,
                                              int mpListCap, const LocalBAParams& par) {
        check(se2gpu_local_ba_batch_device(matcher.handle(), jobKF, njobs, reinterpret_cast<const int32_t*>(out), localList, refList,
                                           kfListCap, mpList, mpListCap, nframes, frameId, frameTwb, frameTcw, frameNull, odoTo, odoMeas,
                                           odoCov, kpsUn, counts, cap, viewPos, levelSigma2, nlevels, pos, M, mpPtr, obsFrame, obsFtr, nobs,
                                           par.fx, par.cx, par.cy, par.Tbc12, par.huberDelta, par.xrotInfo, par.zInfo, par.iters, par.mode,
                                           maxLocal, maxRef, maxMP, maxObs, ws, status, kfOut, mpOut, stats,
                                           reinterpret_cast<int32_t*>(info)),
              "LocalBADeviceTable::LoadAndOptimizeLocalGraphBatchDevice");
    }
};

}  // namespace se2lam_amd
