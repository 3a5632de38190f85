// include/se2lam_amd/LoopVerify.h compiles as plain C++17 and links against libse2gpu (tests/test_loop_verify_abi.py).  The
// verdict helpers are checked here; without a device the C ABI is called with a NULL handle only, with one a batch of two
// empty key frames runs.
#include <cstdio>
#include <vector>

#include "se2lam_amd/LoopVerify.h"

using namespace se2lam_amd;

template <class T>
static T* upload(const std::vector<T>& v) {
    void* d = nullptr;
    check(se2gpu_malloc(&d, v.size() * sizeof(T)), "malloc");
    check(se2gpu_memcpy_h2d(d, v.data(), v.size() * sizeof(T)), "h2d");
    return static_cast<T*>(d);
}

static LoopVerifyInfo rec(int nRaw, int nGood, int nGoodMP, int nMPs) { return LoopVerifyInfo{nRaw, nGood, nGoodMP, nMPs, 2, 0, 0, 1000}; }

int main() {
    // GlobalMapper's rule with the reference's shipped thresholds 15 / 30 / 0.05 as an example
    if (!verifiedGlobalMapper(rec(300, 120, 40, 200), 15, 30, 0.05)) return 10;
    if (verifiedGlobalMapper(rec(300, 120, 14, 200), 15, 30, 0.05)) return 11;    // too few map-point matches
    if (verifiedGlobalMapper(rec(300, 29, 20, 200), 15, 30, 0.05)) return 12;     // too few key-point matches
    if (verifiedGlobalMapper(rec(300, 120, 20, 401), 15, 30, 0.05)) return 13;    // 20 / 401 < 0.05
    if (!verifiedGlobalMapper(rec(300, 120, 20, 400), 15, 30, 0.05)) return 14;   // 20 / 400 = 0.05
    if (verifiedGlobalMapper(rec(0, 0, 0, 0), 0, 0, 0.0)) return 15;              // 0 / 0 is NaN: false whatever the thresholds
    if (!verifiedGlobalMapper(rec(300, 120, 20, 0), 15, 30, 0.05)) return 16;     // n / 0 is +inf, as in the reference
    // Localizer's rule
    if (!verifiedLocalizer(rec(300, 45, 0, 0))) return 20;
    if (verifiedLocalizer(rec(300, 44, 0, 0))) return 21;
    if (!verifiedLocalizer(rec(300, 44, 0, 0), 44)) return 22;

    void (LoopVerifier::*batch)(const DeviceFrameSet&, const uint8_t*, const int32_t*, const int32_t*, const int32_t*, int,
                                const int32_t*, int32_t*, int32_t*, LoopVerifyInfo*) = &LoopVerifier::VerifyBatchDevice;
    void (LoopVerifier::*sync)() = &LoopVerifier::sync;
    void (LoopVerifier::*setStream)(void*) = &LoopVerifier::setStream;
    if (!batch || !sync || !setStream) return 1;
    if (se2gpu_device_count() <= 0) {
        if (se2gpu_track_loop_verify_batch_device(nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, 1, nullptr,
                                                  nullptr, nullptr, nullptr) != SE2GPU_ERR_INVALID)
            return 2;
        if (se2gpu_track_set_stream(nullptr, nullptr) != SE2GPU_ERR_INVALID || se2gpu_track_sync(nullptr) != SE2GPU_ERR_INVALID)
            return 3;
        std::printf("OK (no device)\n");
        return 0;
    }
    const int cap = 8, nframes = 2, npairs = 2;
    DeviceFrameSet frames;
    frames.kps = upload(std::vector<KeyPoint>(nframes * cap));
    frames.counts = upload(std::vector<int32_t>(nframes, 0));
    frames.cap = cap;
    frames.nframes = nframes;
    const int32_t* pa = upload(std::vector<int32_t>{0, 1});
    const int32_t* pb = upload(std::vector<int32_t>{1, 0});
    const int32_t* m12 = upload(std::vector<int32_t>(npairs * cap, 3));
    int32_t* good = upload(std::vector<int32_t>(npairs * cap, 7));
    LoopVerifyInfo* info = upload(std::vector<LoopVerifyInfo>(npairs, rec(7, 7, 7, 7)));
    LoopVerifier verifier;
    verifier.setStream(nullptr);
    (verifier.*batch)(frames, nullptr, nullptr, pa, pb, npairs, m12, good, nullptr, info);
    verifier.sync();
    std::vector<int32_t> h_good(npairs * cap);
    std::vector<LoopVerifyInfo> h_info(npairs);
    check(se2gpu_memcpy_d2h(h_good.data(), good, h_good.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(h_info.data(), info, h_info.size() * sizeof(LoopVerifyInfo)), "d2h");
    for (int32_t v : h_good)
        if (v != -1) return 4;
    for (const LoopVerifyInfo& r : h_info)
        if (r.nRaw || r.nGood || r.nGoodMP || r.nMPsCurr || r.path || r.bestSample != -1 || r.bestModel != -1 || r.iterations)
            return 5;
    std::printf("OK (two empty key frames on the device)\n");
    return 0;
}
