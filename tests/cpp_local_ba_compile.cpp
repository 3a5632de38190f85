// LocalBADeviceTable of include/se2lam_amd/LocalBA.h compiles as plain C++17 and links against libse2gpu
// (tests/test_local_ba_abi.py).  The member is named with its signature, the record of d_info and the host-only work-space
// helpers are checked; without a device the C ABI is called for its refusals (a handle the checks never follow), with one an
// empty batch goes through the member.
#include <cstdio>
#include <vector>

#include "se2lam_amd/LocalBA.h"

using namespace se2lam_amd;

int main() {
    static_assert(sizeof(LocalBAInfo) == 8 * sizeof(int32_t), "d_info");
    static_assert(SE2GPU_LOCAL_BA_WS_ARRAYS == 12, "counts, fixed, poses, o_i, o_j, o_meas, o_info, lm_ptr, e_kf, e_uv, e_info, landmarks");
    static_assert(kLocalBANonFinite == 6, "the status table");
    void (LocalBADeviceTable::*run)(ORBmatcher&, const int32_t*, int, const LocalWindowCounts*, const int32_t*, const int32_t*, int,
                                    const int32_t*, int, const LocalBAParams&) = &LocalBADeviceTable::LoadAndOptimizeLocalGraphBatchDevice;
    if (!run) return 1;

    LocalBADeviceTable t;
    t.maxLocal = 6; t.maxRef = 4; t.maxMP = 60; t.maxObs = 300;
    long long off[SE2GPU_LOCAL_BA_WS_ARRAYS], stride[SE2GPU_LOCAL_BA_WS_ARRAYS];
    if (t.wsBytes(3) <= 0 || t.wsBytes(-1) != -1 || t.wsBytes(65536) != -1) return 2;
    if (se2gpu_local_ba_ws_layout(3, 6, 4, 60, 300, off, stride, SE2GPU_LOCAL_BA_WS_ARRAYS) != SE2GPU_OK) return 3;
    for (int i = 1; i < SE2GPU_LOCAL_BA_WS_ARRAYS; ++i)
        if (off[i] < off[i - 1] + 3 * stride[i - 1] || off[i] % 16 || stride[i] % 16) return 4;
    if (off[SE2GPU_LOCAL_BA_WS_ARRAYS - 1] + 3 * stride[SE2GPU_LOCAL_BA_WS_ARRAYS - 1] > t.wsBytes(3)) return 5;
    if (se2gpu_local_ba_ws_layout(3, 6, 4, 60, 300, off, stride, 11) != SE2GPU_ERR_INVALID ||
        se2gpu_local_ba_ws_layout(3, 0, 4, 60, 300, off, stride, 12) != SE2GPU_ERR_INVALID)
        return 6;

    LocalBAParams par;
    par.fx = 500.f; par.cx = 320.f; par.cy = 240.f;
    alignas(16) static int32_t ints[64] = {};
    std::vector<float> floats(64, 1.f);
    std::vector<double> doubles(64, 0.0);
    if (se2gpu_device_count() <= 0) {
        se2gpu_matcher* fake = reinterpret_cast<se2gpu_matcher*>(ints);   // never followed: the refusals come first
        auto call = [&](int njobs, int nframes, int iters, int nlevels, void* ws) {
            return se2gpu_local_ba_batch_device(fake, ints, njobs, ints, ints, ints, 8, ints, 64, nframes, ints, floats.data(), floats.data(),
                                                nullptr, nullptr, nullptr, nullptr, reinterpret_cast<const se2gpu_keypoint*>(floats.data()),
                                                ints, 16, floats.data(), floats.data(), nlevels, floats.data(), 5, ints, ints, ints, 5,
                                                par.fx, par.cx, par.cy, par.Tbc12, par.huberDelta, par.xrotInfo, par.zInfo, iters, par.mode,
                                                6, 4, 60, 300, ws, ints, doubles.data(), doubles.data(), nullptr, ints);
        };
        if (call(2, 4, 65, 8, ints) != SE2GPU_ERR_INVALID) return 7;
        if (call(2, 4, 10, 33, ints) != SE2GPU_ERR_INVALID) return 8;
        if (call(2, 4, 10, 8, nullptr) != SE2GPU_ERR_INVALID) return 9;
        if (call(2, 4097, 10, 8, ints) != SE2GPU_ERR_CAPACITY) return 10;
        if (call(65536, 4, 10, 8, ints) != SE2GPU_ERR_CAPACITY) return 11;
        if (call(0, 4, 10, 8, ints) != SE2GPU_OK) return 12;
        if (call(2, 4, 10, 8, ints) != SE2GPU_ERR_NO_DEVICE) return 13;
        std::printf("OK (no device)\n");
        return 0;
    }
    // an empty batch launches nothing and reads nothing: host memory stands in for the tables
    ORBmatcher matcher;
    t.nframes = 4; t.cap = 16; t.M = 5; t.nobs = 5; t.nlevels = 8;
    t.frameId = ints; t.frameTwb = floats.data(); t.frameTcw = floats.data();
    t.kpsUn = reinterpret_cast<const se2gpu_keypoint*>(floats.data()); t.counts = ints; t.viewPos = floats.data();
    t.levelSigma2 = floats.data(); t.pos = floats.data(); t.mpPtr = ints; t.obsFrame = ints; t.obsFtr = ints;
    t.ws = ints; t.status = ints; t.kfOut = doubles.data(); t.mpOut = doubles.data();
    t.info = reinterpret_cast<LocalBAInfo*>(ints);
    (t.*run)(matcher, ints, 0, reinterpret_cast<const LocalWindowCounts*>(ints), ints, ints, 8, ints, 64, par);
    matcher.sync();
    std::printf("OK (an empty batch on the device)\n");
    return 0;
}
