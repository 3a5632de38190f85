// The host mirror of the map update (include/se2lam_amd/MapUpdate.h, applyObservations) on cases dumped by
// tests/map_apply_model.py: reads a case file, writes every array the call writes.  Host compiler only, no device, no library:
//   cpp_map_apply in.bin out.bin [in.bin out.bin ...]
// File layout (little endian): 9 ints {cap, nframes, m_cap, nobs_cap, B, kinds, has_frame_null, has_rows, has_status}, then the
// arrays of map_apply_model.CASE_FIELDS in that order; the output holds map_apply_model.OUT_FIELDS in that order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "se2lam_amd/MapUpdate.h"

namespace {

template <typename T>
std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "cpp_map_apply: short read\n");
        std::exit(2);
    }
    return v;
}
template <typename T>
void put(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3);
}
template <typename T>
const T* opt(const std::vector<T>& v, bool on) { return on ? v.data() : nullptr; }

int run(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 1;
    const auto z = take<int32_t>(f, 9);
    const size_t cap = z[0], nframes = z[1], mCap = z[2], nobsCap = z[3], B = z[4], nf = nframes * cap, nr = B * cap;
    const auto counts = take<int32_t>(f, nframes);
    const auto frameNull = take<uint8_t>(f, nframes);
    const auto mpPtr = take<int32_t>(f, mCap + 1);
    const auto obsFrame = take<int32_t>(f, nobsCap), obsFtr = take<int32_t>(f, nobsCap);
    const auto obsView = take<float>(f, 3 * nobsCap), obsInfo = take<float>(f, 9 * nobsCap);
    const auto sizesIn = take<int32_t>(f, 2);
    const auto jobPrev = take<int32_t>(f, B), jobNew = take<int32_t>(f, B);
    const auto kind = take<uint8_t>(f, nr);
    const auto src = take<int32_t>(f, nr);
    const auto view = take<float>(f, 3 * nr), info = take<float>(f, 9 * nr), newPosW = take<float>(f, 3 * nr);
    const auto infoPrev = take<float>(f, 9 * nr), localPos = take<float>(f, 3 * nr);
    const auto goodPrlRow = take<uint8_t>(f, nr);
    const auto status = take<int32_t>(f, mCap);
    auto pos = take<float>(f, 3 * mCap);
    auto goodPrl = take<uint8_t>(f, mCap), mpNull = take<uint8_t>(f, mCap);
    auto normal = take<float>(f, 3 * mCap);
    auto ftrMP = take<int32_t>(f, nf);
    auto kfObserved = take<uint8_t>(f, nf);
    auto viewPos = take<float>(f, 3 * nf), viewInfo = take<float>(f, 9 * nf);
    std::fclose(f);
    // what the call leaves alone keeps the sentinels the model's outputs start from
    std::vector<int32_t> mpPtrNew(mCap + 1, -9), obsFrameNew(nobsCap, -9), obsFtrNew(nobsCap, -9), newFrame(mCap, -9), sizesOut(9, -9),
        jobCounts(6 * B, -9);
    std::vector<float> obsViewNew(3 * nobsCap, -7.f), obsInfoNew(9 * nobsCap, -7.f);

    se2lam_amd::MapApplyTables t;
    t.counts = counts.data(); t.cap = (int)cap; t.nframes = (int)nframes; t.frameNull = opt(frameNull, z[6] != 0);
    t.mpPtr = mpPtr.data(); t.obsFrame = obsFrame.data(); t.obsFtr = obsFtr.data();
    t.obsView = opt(obsView, z[7] != 0); t.obsInfo = opt(obsInfo, z[7] != 0);
    t.sizesIn = sizesIn.data(); t.mCap = (int)mCap; t.nobsCap = (int)nobsCap;
    t.B = (int)B; t.jobPrev = jobPrev.data(); t.jobNew = jobNew.data(); t.kind = kind.data(); t.src = src.data();
    t.view = view.data(); t.info = info.data(); t.newPosW = newPosW.data(); t.infoPrev = infoPrev.data();
    t.localPos = localPos.data(); t.goodPrlRow = goodPrlRow.data(); t.kinds = z[5];
    t.parallaxStatus = opt(status, z[8] != 0);
    t.pos = pos.data(); t.goodPrl = goodPrl.data(); t.mpNull = mpNull.data(); t.mpNormal = normal.data();
    t.ftrMP = ftrMP.data(); t.kfObserved = kfObserved.data(); t.viewPos = viewPos.data(); t.viewInfo = viewInfo.data();
    t.mpPtrNew = mpPtrNew.data(); t.obsFrameNew = obsFrameNew.data(); t.obsFtrNew = obsFtrNew.data();
    t.obsViewNew = z[7] ? obsViewNew.data() : nullptr; t.obsInfoNew = z[7] ? obsInfoNew.data() : nullptr;
    t.newFrame = newFrame.data(); t.sizesOut = sizesOut.data(); t.jobCounts = jobCounts.data();
    const int rc = se2lam_amd::applyObservations(t);
    if (rc != sizesOut[0]) return 4;

    FILE* g = std::fopen(out, "wb");
    if (!g) return 1;
    put(g, pos); put(g, goodPrl); put(g, mpNull); put(g, normal); put(g, ftrMP); put(g, kfObserved); put(g, viewPos); put(g, viewInfo);
    put(g, mpPtrNew); put(g, obsFrameNew); put(g, obsFtrNew); put(g, obsViewNew); put(g, obsInfoNew); put(g, newFrame);
    put(g, sizesOut); put(g, jobCounts);
    std::fclose(g);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        const int rc = run(argv[i], argv[i + 1]);
        if (rc) {
            std::fprintf(stderr, "cpp_map_apply: %s failed (%d)\n", argv[i], rc);
            return rc;
        }
    }
    std::printf("map apply mirror: %d cases\n", (argc - 1) / 2);
    return 0;
}
