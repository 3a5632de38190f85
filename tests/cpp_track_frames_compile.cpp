// include/se2lam_amd/Track.h compiles as plain C++17 and links against libse2gpu (tests/test_track_frames_abi.py).  The count
// tests of needNewKF are checked here; without a device the C ABI is called with a NULL handle only, with one a batch of two
// pairs of empty frames runs.
#include <cstdio>
#include <vector>

#include "se2lam_amd/Track.h"

using namespace se2lam_amd;

template <class T>
static T* upload(const std::vector<T>& v) {
    void* d = nullptr;
    check(se2gpu_malloc(&d, v.size() * sizeof(T)), "malloc");
    check(se2gpu_memcpy_h2d(d, v.data(), v.size() * sizeof(T)), "h2d");
    return static_cast<T*>(d);
}

static TrackFrameInfo rec(int nMatched, int nTrackedOld, int nGoodPrl, int nOldKP) {
    return TrackFrameInfo{300, nMatched, nTrackedOld, nGoodPrl, nOldKP, 2, 0, 0};
}

int main() {
    // Track::needNewKF's count tests with nMinFrames = 8, nMaxFrames = 45, Config::MaxFtrNumber = 1000 as an example
    if (needNewKFByCounts(rec(200, 10, 50, 100), 8, 8, 45, 1000).need) return 10;     // c0: the gap has to exceed nMinFrames
    if (!needNewKFByCounts(rec(200, 50, 41, 100), 9, 8, 45, 1000).need) return 11;    // c1 (50 <= 100 * 0.5) and c2 (41 > 40)
    if (needNewKFByCounts(rec(200, 51, 41, 100), 9, 8, 45, 1000).need) return 12;     // c1 fails
    if (needNewKFByCounts(rec(200, 50, 40, 100), 9, 8, 45, 1000).need) return 13;     // c2 fails
    if (!needNewKFByCounts(rec(200, 90, 0, 100), 46, 8, 45, 1000).need) return 14;    // c3: the gap exceeds nMaxFrames
    if (!needNewKFByCounts(rec(99, 90, 0, 100), 9, 8, 45, 1000).need) return 15;      // c4: nMatched < 0.1 * MaxFtrNumber
    if (needNewKFByCounts(rec(100, 90, 0, 100), 9, 8, 45, 1000).need) return 16;
    if (!needNewKFByCounts(rec(19, 90, 0, 100), 9, 8, 45, 100).need) return 17;       // c4: nMatched < 20
    if (needNewKFByCounts(rec(200, 50, 41, 100), 9, 8, 45, 1000).abortBA) return 18;  // c1 && c2 alone does not abort the BA
    if (!needNewKFByCounts(rec(99, 90, 0, 100), 9, 8, 45, 1000).abortBA) return 19;
    if (needNewKFByCounts(rec(99, 90, 0, 100), 8, 8, 45, 1000).abortBA) return 20;

    void (TrackGeometry::*batch)(const DeviceFrameSet&, const uint8_t*, const float*, const int32_t*, const int32_t*, int,
                                 const float*, const float*, const uint8_t*, const float*, const int32_t*, float, float, int,
                                 int32_t*, Point3f*, uint8_t*, TrackFrameInfo*) = &TrackGeometry::TrackFramesBatchDevice;
    void (TrackGeometry::*sync)() = &TrackGeometry::sync;
    void (TrackGeometry::*setStream)(void*) = &TrackGeometry::setStream;
    if (!batch || !sync || !setStream) return 1;
    const float eye[12] = {400, 0, 320, 0, 0, 400, 240, 0, 0, 0, 1, 0};
    if (se2gpu_device_count() <= 0) {
        if (se2gpu_track_frames_batch_device(nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr,
                                             nullptr, eye, nullptr, 500.f, 8000.f, 2, nullptr, nullptr, nullptr,
                                             nullptr) != SE2GPU_ERR_INVALID)
            return 2;
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
    const float* Trc = upload(std::vector<float>(npairs * 12, 0.f));
    const float* P = upload(std::vector<float>(npairs * 12, 0.f));
    const int32_t* m12 = upload(std::vector<int32_t>(npairs * cap, 3));
    int32_t* matched = upload(std::vector<int32_t>(npairs * cap, 7));
    Point3f* pos = upload(std::vector<Point3f>(npairs * cap, Point3f{7, 7, 7}));
    uint8_t* good = upload(std::vector<uint8_t>(npairs * cap, 7));
    TrackFrameInfo* info = upload(std::vector<TrackFrameInfo>(npairs, rec(7, 7, 7, 7)));
    TrackGeometry geom;
    geom.setStream(nullptr);
    (geom.*batch)(frames, nullptr, nullptr, pa, pb, npairs, Trc, P, nullptr, eye, m12, 500.f, 8000.f, 2, matched, pos, good, info);
    geom.sync();
    std::vector<int32_t> h_m(npairs * cap);
    std::vector<Point3f> h_pos(npairs * cap);
    std::vector<uint8_t> h_good(npairs * cap);
    std::vector<TrackFrameInfo> h_info(npairs);
    check(se2gpu_memcpy_d2h(h_m.data(), matched, h_m.size() * sizeof(int32_t)), "d2h");
    check(se2gpu_memcpy_d2h(h_pos.data(), pos, h_pos.size() * sizeof(Point3f)), "d2h");
    check(se2gpu_memcpy_d2h(h_good.data(), good, h_good.size()), "d2h");
    check(se2gpu_memcpy_d2h(h_info.data(), info, h_info.size() * sizeof(TrackFrameInfo)), "d2h");
    for (int32_t v : h_m)
        if (v != -1) return 4;
    for (const Point3f& v : h_pos)
        if (v.x != 0 || v.y != 0 || v.z != 0) return 5;
    for (uint8_t v : h_good)
        if (v) return 6;
    for (const TrackFrameInfo& r : h_info)
        if (r.nRaw || r.nMatched || r.nTrackedOld || r.nGoodPrl || r.nOldKP || r.path || r.nDepthRejected || r.status != 2) return 7;
    std::printf("OK (two pairs of empty frames on the device)\n");
    return 0;
}
