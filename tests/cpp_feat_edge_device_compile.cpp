// FeatEdgeDeviceTable of include/se2lam_amd/FeatEdge.h compiles as plain C++17 and links against libse2gpu
// (tests/test_feat_edge_device_abi.py).  The two members are named with their signatures, the record of d_info8 and the host-only
// work-space helpers are checked; without a device the C ABI is called for its refusals (a handle the checks never follow),
// with one an empty batch goes through both members.
#include <cstdio>
#include <vector>

#include "se2lam_amd/FeatEdge.h"

using namespace se2lam_amd;

int main() {
    static_assert(sizeof(FeatEdgeDeviceInfo) == 8 * sizeof(int32_t), "d_info8");
    static_assert(SE2GPU_FEAT_EDGE_WS_ARRAYS == 7, "counts, kf12, prior measurement, prior information, xyz, m_z, m_info");
    void (FeatEdgeDeviceTable::*covis)(ORBmatcher&, const int32_t*, const int32_t*, int, const CovisPair*, const CovisCommon*, int,
                                       const FeatEdgeParams&, int, int) = &FeatEdgeDeviceTable::CreateFeatEdgeCovisBatchDevice;
    void (FeatEdgeDeviceTable::*match)(ORBmatcher&, const int32_t*, const int32_t*, int, const int32_t*, const FeatEdgeParams&, int,
                                       int) = &FeatEdgeDeviceTable::CreateFeatEdgeMatchBatchDevice;
    if (!covis || !match) return 1;

    FeatEdgeDeviceTable t;
    t.rowCap = 65;
    long long off[SE2GPU_FEAT_EDGE_WS_ARRAYS];
    if (t.wsBytes(3) <= 0 || t.wsBytes(-1) != -1 || t.wsBytes(65536) != -1) return 2;
    if (se2gpu_feat_edge_ws_layout(3, 65, off, SE2GPU_FEAT_EDGE_WS_ARRAYS) != SE2GPU_OK) return 3;
    for (int i = 1; i < SE2GPU_FEAT_EDGE_WS_ARRAYS; ++i)
        if (off[i] <= off[i - 1]) return 4;
    if (off[SE2GPU_FEAT_EDGE_WS_ARRAYS - 1] + 8LL * 18 * 3 * 65 > t.wsBytes(3)) return 5;
    if (se2gpu_feat_edge_ws_layout(3, 65, off, 6) != SE2GPU_ERR_INVALID || se2gpu_feat_edge_ws_layout(3, 0, off, 7) != SE2GPU_ERR_INVALID)
        return 6;

    FeatEdgeParams par;
    std::vector<int32_t> ints(64, 0);
    std::vector<float> floats(64, 0.f);
    std::vector<double> doubles(64, 0.0);
    if (se2gpu_device_count() <= 0) {
        se2gpu_matcher* fake = reinterpret_cast<se2gpu_matcher*>(ints.data());   // never followed: the refusals come first
        auto call = [&](int mode, int iters, int npairs, int rowCap, void* ws) {
            return se2gpu_feat_edge_batch_device(fake, mode, iters, 10, par.huberDelta, par.outlierChi2, par.Tbc12, par.xrotInfo,
                                                 par.yrotInfo, par.zInfo, ints.data(), ints.data(), npairs, 4, floats.data(), floats.data(),
                                                 5, rowCap, ints.data(), ints.data(), 8, floats.data(), floats.data(), 5, ints.data(),
                                                 ints.data(), 16, ints.data(), floats.data(), floats.data(), ws, ints.data(), doubles.data(),
                                                 doubles.data(), doubles.data(), nullptr, nullptr, nullptr, nullptr);
        };
        if (call(2, 15, 2, 8, ints.data()) != SE2GPU_ERR_INVALID) return 7;
        if (call(0, 65, 2, 8, ints.data()) != SE2GPU_ERR_INVALID) return 8;
        if (call(0, 15, 2, 8, nullptr) != SE2GPU_ERR_INVALID) return 9;
        if (call(1, 30, 65536, 8, ints.data()) != SE2GPU_ERR_CAPACITY) return 10;
        if (call(1, 30, 0, 8, ints.data()) != SE2GPU_OK) return 11;
        if (call(0, 15, 2, 8, ints.data()) != SE2GPU_ERR_NO_DEVICE || call(1, 30, 2, 8, ints.data()) != SE2GPU_ERR_NO_DEVICE) return 12;
        std::printf("OK (no device)\n");
        return 0;
    }
    // an empty batch launches nothing and reads nothing: host memory stands in for the tables
    ORBmatcher matcher;
    t.nframes = 4; t.M = 5; t.nobs = 5; t.cap = 16;
    t.frameTwc = floats.data(); t.pos = floats.data(); t.obsView = floats.data(); t.obsInfo = floats.data();
    t.counts = ints.data(); t.ftrMP = ints.data(); t.viewPos = floats.data(); t.viewInfo = floats.data();
    t.ws = ints.data(); t.info = reinterpret_cast<FeatEdgeDeviceInfo*>(ints.data());
    t.kf12 = doubles.data(); t.z12 = doubles.data(); t.info36 = doubles.data();
    (t.*covis)(matcher, ints.data(), ints.data(), 0, reinterpret_cast<const CovisPair*>(ints.data()),
               reinterpret_cast<const CovisCommon*>(ints.data()), 8, par, kFeatEdgeCovisIters, kFeatEdgeCovisMinPoints);
    (t.*match)(matcher, ints.data(), ints.data(), 0, ints.data(), par, kFeatEdgeMatchIters, kFeatEdgeMatchMinPoints);
    matcher.sync();
    std::printf("OK (empty batches on the device)\n");
    return 0;
}
