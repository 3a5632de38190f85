// include/se2lam_amd/ORBmatcher.h compiles as plain C++17 with DeviceFrameSet, DeviceFeatureVectorSet and
// ORBmatcher::SearchByBoWBatchDevice, and links against libse2gpu (tests/test_search_bow_batch_abi.py).  Without a device it
// only takes the method's address and calls the C ABI with a NULL handle; with one it runs a batch of two empty key frames.
#include <cstdio>
#include <vector>

#include "se2lam_amd/ORBmatcher.h"

using namespace se2lam_amd;

template <class T>
static T* upload(const std::vector<T>& v) {
    void* d = nullptr;
    check(se2gpu_malloc(&d, v.size() * sizeof(T)), "malloc");
    check(se2gpu_memcpy_h2d(d, v.data(), v.size() * sizeof(T)), "h2d");
    return static_cast<T*>(d);
}

int main() {
    void (ORBmatcher::*batch)(const DeviceFrameSet&, const DeviceFeatureVectorSet&, const int32_t*, const int32_t*, int, int32_t*,
                              int32_t*, bool) = &ORBmatcher::SearchByBoWBatchDevice;
    void (ORBmatcher::*sync)() = &ORBmatcher::sync;
    void (ORBmatcher::*setStream)(void*) = &ORBmatcher::setStream;
    DeviceFrameSet frames;
    DeviceFeatureVectorSet fvs;
    if (!batch || !sync || !setStream || frames.kps || frames.cap || fvs.nodes || fvs.hasMapPoint) return 1;
    if (se2gpu_device_count() <= 0) {
        if (se2gpu_search_by_bow_batch_device(nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, 1, 0, 0.6f, 1, nullptr, nullptr) != SE2GPU_ERR_INVALID)
            return 2;
        std::printf("OK (no device)\n");
        return 0;
    }
    const int cap = 8, nframes = 2, npairs = 2;
    frames.kps = upload(std::vector<KeyPoint>(nframes * cap));
    frames.desc = upload(std::vector<uint8_t>(nframes * cap * 32));
    frames.counts = upload(std::vector<int32_t>(nframes, 0));
    frames.cap = cap;
    frames.nframes = nframes;
    fvs.nodes = upload(std::vector<int32_t>(nframes * cap, 0));
    fvs.ptr = upload(std::vector<int32_t>(nframes * (cap + 1), 0));
    fvs.idx = upload(std::vector<int32_t>(nframes * cap, 0));
    fvs.nn = upload(std::vector<int32_t>(nframes, 0));
    const int32_t* pa = upload(std::vector<int32_t>{0, 1});
    const int32_t* pb = upload(std::vector<int32_t>{1, 0});
    int32_t* m12 = upload(std::vector<int32_t>(npairs * cap, 7));
    int32_t* nm = upload(std::vector<int32_t>(npairs, 7));
    ORBmatcher matcher(0.9f, true);
    matcher.setStream(nullptr);
    (matcher.*batch)(frames, fvs, pa, pb, npairs, m12, nm, false);
    matcher.sync();
    std::vector<int32_t> h_m(npairs * cap), h_n(npairs);
    check(se2gpu_memcpy_d2h(h_m.data(), m12, h_m.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(h_n.data(), nm, h_n.size() * sizeof(int32_t)), "d2h");
    for (int32_t v : h_m)
        if (v != -1) return 3;
    for (int32_t v : h_n)
        if (v != 0) return 4;
    std::printf("OK (two empty key frames on the device)\n");
    return 0;
}
