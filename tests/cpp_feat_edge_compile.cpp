// include/se2lam_amd/FeatEdge.h compiles as plain C++17 and links against libse2gpu (tests/test_feat_edge_abi.py).  The
// reference's constants are checked here; without a device the C ABI is called for its refusals only, with one a batch of two
// pairs below the minimum number of points runs (status 1: nothing is optimised, the poses come back as given).
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "se2lam_amd/FeatEdge.h"

using namespace se2lam_amd;

int main() {
    static_assert(kFeatEdgeCovisIters == 15 && kFeatEdgeCovisMinPoints == 10, "OptKFPair: 15 iterations, 10 points");
    static_assert(kFeatEdgeMatchIters == 30 && kFeatEdgeMatchMinPoints == 3, "OptKFPairMatch: 30 iterations, 3 matches");
    static_assert(SE2GPU_FEAT_EDGE_COVIS == 0 && SE2GPU_FEAT_EDGE_MATCH == 1, "the two modes");
    if (kFeatEdgeHuberDelta != 5.99 || kFeatEdgeOutlierChi2 != 5.0) return 1;
    FeatEdgeParams par;
    if (par.huberDelta != 5.99 || par.outlierChi2 != 5.0 || par.xrotInfo != 1e6 || par.yrotInfo != 1e6 || par.zInfo != 1) return 2;
    void (*covis)(const FeatEdgeView&, const FeatEdgeParams&, FeatEdgeResult&, int, int) = &CreateFeatEdgeCovisBatch;
    void (*match)(const FeatEdgeView&, const FeatEdgeParams&, FeatEdgeResult&, int, int) = &CreateFeatEdgeMatchBatch;
    if (!covis || !match) return 3;

    const std::vector<double> kf = {1, 0, 0, 0, 1, 0, 0, 0, 1, 10, 20, 30, 0, -1, 0, 1, 0, 0, 0, 0, 1, -5, 6, 7,
                                    1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 3, 1, 0, 0, 0, 1, 0, 0, 0, 1, 4, 5, 6};
    const std::vector<int32_t> ptr = {0, 2, 2};
    const std::vector<double> xyz = {1, 2, 3, 4, 5, 6}, z(12, 1.0), info = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1,
                                                                             1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    FeatEdgeView v;
    v.npairs = 2; v.kf12 = kf.data(); v.mp_ptr = ptr.data(); v.mp_xyz = xyz.data(); v.m_z = z.data(); v.m_info = info.data();
    FeatEdgeResult r;
    if (se2gpu_device_count() <= 0) {
        // the refusals of the arguments come first; with valid arguments the missing device is the error
        try { CreateFeatEdgeBatch(v, 2, 30, 3, par, r); return 4; } catch (const std::runtime_error&) {}
        if (se2gpu_feat_edge_batch(2, 1, 65, 3, kf.data(), par.Tbc12, 1e6, 1e6, 1, ptr.data(), xyz.data(), z.data(), info.data(), 5.99, 5.0,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SE2GPU_ERR_INVALID)
            return 5;
        try { (*match)(v, par, r, kFeatEdgeMatchIters, kFeatEdgeMatchMinPoints); return 6; } catch (const std::runtime_error&) {}
        std::printf("OK (no device)\n");
        return 0;
    }
    (*match)(v, par, r, kFeatEdgeMatchIters, kFeatEdgeMatchMinPoints);
    if (r.status.size() != 2 || r.status[0] != 1 || r.status[1] != 1 || r.nPoints[0] != 2 || r.nPoints[1] != 0) return 7;
    for (int p = 0; p < 2; ++p) {
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 12; ++i)
                if ((i < 9 ? r.kf[2 * p + k].R[i] : r.kf[2 * p + k].t[i - 9]) != kf[24 * p + 12 * k + i]) return 8;
        for (int i = 0; i < 36; ++i)
            if (r.constraint[p].info.m[i] != 0) return 9;
        if (r.stats[p].iterations != 0 || r.nSparsified[p] != 0) return 10;
    }
    if (r.mp.size() != 2 || r.mp[1](2) != 6 || r.outlier[0] || r.outlier[1]) return 11;
    std::printf("OK (two pairs below the minimum on the device)\n");
    return 0;
}
