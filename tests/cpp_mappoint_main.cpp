// include/se2lam_amd/MapPointMain.h's host mainObservation on a case file written by tests/test_mappoint_main_model.py.
// Everything is whitespace-separated integers (floats as their 32-bit patterns):
//   nframes cap nlevels m nobs has_null has_view has_prev
//   counts[nframes]  null[nframes]?  scale_factors[nlevels]  octave[nframes*cap]  desc[nframes*cap*32]
//   view[nframes*cap*3]?  mp_ptr[m+1]  obs_frame[nobs]  obs_ftr[nobs]  prev[m]?
// Output, one line per point: info[4] main_frame main_octave dist[2] (bit patterns) main_desc[32]; outputs the function leaves
// alone keep the sentinels frame -55, octave -77, dist -1.0f, descriptor bytes 0xAB.
//   cpp_mappoint_main <case file>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "se2lam_amd/MapPointMain.h"

using namespace se2lam_amd;

static FILE* g_in;
static long long next() {
    long long v = 0;
    if (std::fscanf(g_in, "%lld", &v) != 1) {
        std::fprintf(stderr, "short case file\n");
        std::exit(2);
    }
    return v;
}
static float next_float() {
    const uint32_t b = (uint32_t)next();
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static unsigned bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

int main(int argc, char** argv) {
    if (argc < 2 || !(g_in = std::fopen(argv[1], "r"))) return 1;
    const int nframes = (int)next(), cap = (int)next(), nlevels = (int)next(), m = (int)next(), nobs = (int)next();
    const bool has_null = next() != 0, has_view = next() != 0, has_prev = next() != 0;
    const size_t nf = (size_t)nframes * cap;
    std::vector<int32_t> counts(nframes), mp_ptr(m + 1), obs_frame(nobs), obs_ftr(nobs), prev(m, -1);
    std::vector<uint8_t> null(nframes, 0), desc(nf * 32);
    std::vector<float> sf(nlevels);
    std::vector<KeyPoint> kps(nf);
    std::vector<Point3f> view(nf);
    for (auto& v : counts) v = (int32_t)next();
    if (has_null) for (auto& v : null) v = (uint8_t)next();
    for (auto& v : sf) v = next_float();
    for (auto& k : kps) k.octave = (int)next();
    for (auto& v : desc) v = (uint8_t)next();
    if (has_view) for (auto& v : view) { v.x = next_float(); v.y = next_float(); v.z = next_float(); }
    for (auto& v : mp_ptr) v = (int32_t)next();
    for (auto& v : obs_frame) v = (int32_t)next();
    for (auto& v : obs_ftr) v = (int32_t)next();
    if (has_prev) for (auto& v : prev) v = (int32_t)next();
    DeviceFrameSet frames;
    frames.kps = kps.data(); frames.desc = desc.data(); frames.counts = counts.data(); frames.cap = cap; frames.nframes = nframes;
    for (int p = 0; p < m; ++p) {
        uint8_t md[32];
        for (auto& b : md) b = 0xAB;
        int32_t frame = -55, octave = -77;
        float dist[2] = {-1.0f, -1.0f};
        int s, n;
        se2gpu::point_segment(se2gpu::ObsCsr{mp_ptr.data(), obs_frame.data(), obs_ftr.data(), m, nobs}, p, s, n);
        const MainObservationInfo r = mainObservation(frames, has_null ? null.data() : nullptr, has_view ? view.data() : nullptr,
                                                      sf.data(), nlevels, obs_frame.data() + s, obs_ftr.data() + s, n, prev[p],
                                                      md, &frame, &octave, dist);
        std::printf("%d %d %d %d %d %d %u %u", r.pos, r.median, r.N, r.changed, frame, octave, bits(dist[0]), bits(dist[1]));
        for (auto b : md) std::printf(" %u", (unsigned)b);
        std::printf("\n");
    }
    return 0;
}
