// include/se2lam_amd/MapUpdate.h compiles as plain C++17 and links against libse2gpu (tests/test_map_apply_abi.py).  Without a
// device the C ABI is called with a NULL handle only; with one, MapObservationTable::applyBatchDevice creates one point on an
// empty map of four slots and the sizes it leaves are read back.
#include <cstdio>
#include <vector>

#include "se2lam_amd/MapUpdate.h"

using namespace se2lam_amd;

template <class T>
static T* upload(const std::vector<T>& v) {
    void* d = nullptr;
    check(se2gpu_malloc(&d, v.size() * sizeof(T)), "malloc");
    check(se2gpu_memcpy_h2d(d, v.data(), v.size() * sizeof(T)), "h2d");
    return static_cast<T*>(d);
}

int main() {
    void (MapObservationTable::*apply)(ORBmatcher&, void*, long long) = &MapObservationTable::applyBatchDevice;
    int (*mirror)(const MapApplyTables&) = &applyObservations;
    if (!apply || !mirror) return 1;
    if (MapObservationTable::workspaceBytes(1, 8, 4, 8) <= 0 || MapObservationTable::workspaceBytes(-1, 8, 4, 8) != -1) return 2;
    if (se2gpu_device_count() <= 0) {
        MapObservationTable t;
        if (se2gpu_map_apply_batch_device(nullptr, t.counts, 8, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 4, 8,
                                          nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          14, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) != SE2GPU_ERR_INVALID)
            return 3;
        std::printf("OK (no device)\n");
        return 0;
    }
    const int cap = 8, nframes = 2, mCap = 4, nobsCap = 8, B = 1, nf = nframes * cap, nr = B * cap;
    MapObservationTable t;
    t.counts = upload(std::vector<int32_t>(nframes, cap)); t.cap = cap; t.nframes = nframes;
    t.mpPtr = upload(std::vector<int32_t>(mCap + 1, 0));
    t.obsFrame = upload(std::vector<int32_t>(nobsCap, 0)); t.obsFtr = upload(std::vector<int32_t>(nobsCap, 0));
    t.sizesIn = upload(std::vector<int32_t>{0, 0}); t.mCap = mCap; t.nobsCap = nobsCap;
    std::vector<uint8_t> kind(nr, 0);
    std::vector<int32_t> src(nr, -1);
    kind[2] = 3; src[2] = 5;                                        // feature 2 of the new key frame, from feature 5 of the previous one
    t.B = B; t.jobPrev = upload(std::vector<int32_t>{0}); t.jobNew = upload(std::vector<int32_t>{1});
    t.kind = upload(kind); t.src = upload(src);
    t.view = upload(std::vector<float>(3 * nr, 1.f)); t.info = upload(std::vector<float>(9 * nr, 2.f));
    t.newPosW = upload(std::vector<float>(3 * nr, 3.f)); t.infoPrev = upload(std::vector<float>(9 * nr, 4.f));
    t.localPos = upload(std::vector<float>(3 * nr, 5.f)); t.goodPrlRow = upload(std::vector<uint8_t>(nr, 1));
    t.pos = upload(std::vector<float>(3 * mCap, 0.f)); t.goodPrl = upload(std::vector<uint8_t>(mCap, 0));
    t.mpNull = upload(std::vector<uint8_t>(mCap, 1)); t.mpNormal = upload(std::vector<float>(3 * mCap, 0.f));
    t.ftrMP = upload(std::vector<int32_t>(nf, -1)); t.kfObserved = upload(std::vector<uint8_t>(nf, 0));
    t.viewPos = upload(std::vector<float>(3 * nf, 0.f)); t.viewInfo = upload(std::vector<float>(9 * nf, 0.f));
    t.mpPtrNew = upload(std::vector<int32_t>(mCap + 1, -9));
    t.obsFrameNew = upload(std::vector<int32_t>(nobsCap, -9)); t.obsFtrNew = upload(std::vector<int32_t>(nobsCap, -9));
    t.newFrame = upload(std::vector<int32_t>(mCap, -9)); t.sizesOut = upload(std::vector<int32_t>(SE2GPU_MAP_APPLY_NSIZES, -9));
    t.jobCounts = upload(std::vector<int32_t>(6 * B, -9));
    const long long wsBytes = MapObservationTable::workspaceBytes(B, cap, mCap, nobsCap);
    void* ws = nullptr;
    check(se2gpu_malloc(&ws, (size_t)wsBytes), "malloc");
    ORBmatcher matcher;
    (t.*apply)(matcher, ws, wsBytes);
    check(se2gpu_matcher_sync(matcher.handle()), "sync");
    std::vector<int32_t> sizes(SE2GPU_MAP_APPLY_NSIZES), ptr(mCap + 1), frame(nobsCap), ftr(nobsCap), held(nf);
    check(se2gpu_memcpy_d2h(sizes.data(), t.sizesOut, sizes.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(ptr.data(), t.mpPtrNew, ptr.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(frame.data(), t.obsFrameNew, frame.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(ftr.data(), t.obsFtrNew, ftr.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(held.data(), t.ftrMP, held.size() * sizeof(int32_t)), "d2h");
    const std::vector<int32_t> want{0, 1, 2, 2, 0, 1, 0, 0, 0};
    if (sizes != want) return 4;
    if (ptr != std::vector<int32_t>{0, 2, 2, 2, 2}) return 5;
    if (frame[0] != 0 || ftr[0] != 5 || frame[1] != 1 || ftr[1] != 2) return 6;
    if (held[5] != 0 || held[cap + 2] != 0) return 7;
    std::printf("OK (one point created on the device)\n");
    return 0;
}
