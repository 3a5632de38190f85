// One host thread doing the arithmetic of se2gpu_kf_correspd_batch_device and se2gpu_mappoint_parallax_batch_device with the
// host functions of include/se2lam_amd/FindCorrespd.h: the baseline of tools/new_kf_bench.py.  The selection (which pass took
// a feature) is read from the device's kind / src arrays; per feature the program does what that pass computes, and for a
// feature pass 2 looked at and refused the triangulation and the acceptance test.  Reads raw arrays from a directory, writes
// host_view.f32 / host_status.i32 for the comparison, prints "correspd <windows> <median> <p10> <p90>" and "parallax ..." (ms).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "se2lam_amd/FindCorrespd.h"

using namespace se2lam_amd;

template <typename T>
static std::vector<T> load(const std::string& dir, const char* name) {
    std::ifstream f(dir + "/" + name, std::ios::binary | std::ios::ate);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read((char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}
template <typename T>
static void save(const std::string& dir, const char* name, const std::vector<T>& v) {
    std::ofstream f(dir + "/" + name, std::ios::binary);
    f.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
}

template <typename F>
static void windows(const char* what, F fn) {
    fn();
    std::vector<double> ms;
    for (int w = 0; w < 7; ++w) {
        int n = 0;
        const auto t0 = std::chrono::steady_clock::now();
        double dt;
        do {
            fn();
            ++n;
            dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        } while (dt < 0.3);
        ms.push_back(1e3 * dt / n);
    }
    std::sort(ms.begin(), ms.end());
    std::printf("%s %d %.6g %.6g %.6g\n", what, (int)ms.size(), ms[3], ms[1], ms[5]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    const auto head = load<int32_t>(d, "head.i32");   // nframes, cap, B, points, nobs
    const int nframes = head[0], cap = head[1], B = head[2], npts = head[3];
    const auto par = load<float>(d, "par.f32");       // fx, lower, upper
    const auto counts = load<int32_t>(d, "counts.i32"), idkf = load<int32_t>(d, "idkf.i32");
    const auto Tcw = load<float>(d, "Tcw.f32"), Twc = load<float>(d, "Twc.f32"), P = load<float>(d, "P.f32");
    const auto kps = load<KeyPoint>(d, "kps.bin");
    const auto view_pos = load<float>(d, "view_pos.f32"), local_pos = load<float>(d, "local_pos.f32");
    const auto job_prev = load<int32_t>(d, "job_prev.i32"), job_new = load<int32_t>(d, "job_new.i32");
    const auto Tcr = load<float>(d, "Tcr.f32"), Trc = load<float>(d, "Trc.f32");
    const auto kind = load<uint8_t>(d, "kind.u8");
    const auto src = load<int32_t>(d, "src.i32"), midx = load<int32_t>(d, "match_idx_mp.i32");
    const auto main_frame = load<int32_t>(d, "main_frame.i32"), main_ftr = load<int32_t>(d, "main_ftr.i32"),
               main_octave = load<int32_t>(d, "main_octave.i32");
    const auto normal = load<float>(d, "normal.f32"), dist = load<float>(d, "dist.f32");
    const auto ptr = load<int32_t>(d, "ptr.i32"), of = load<int32_t>(d, "obs_frame.i32"), ok = load<int32_t>(d, "obs_ftr.i32"),
               nw = load<int32_t>(d, "new_frame.i32");
    const float fx = par[0], lower = par[1], upper = par[2];
    const float I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<float> view((size_t)B * cap * 3, -7.f), info((size_t)B * cap * 9), infoPrev((size_t)B * cap * 9), posW((size_t)B * cap * 3);

    auto correspd = [&]() {
        for (int b = 0; b < B; ++b) {
            const int fp = job_prev[b], fn = job_new[b];
            const float* tcr = &Tcr[12 * (size_t)b];
            for (int j = 0; j < counts[fn]; ++j) {
                const size_t r = (size_t)b * cap + j;
                const int k = kind[r], s = src[r];
                float* v = &view[3 * r];
                float other[9];
                if (k == 1) {
                    const float* x = &view_pos[3 * ((size_t)fp * cap + s)];
                    calcSE3toXYZInfo(Point3f{x[0], x[1], x[2]}, I12, tcr, &Trc[12 * (size_t)b], fx, other, &info[9 * r]);
                    se2gpu::se3map(tcr, x, v);
                } else if (k == 3) {
                    const float* x = &local_pos[3 * ((size_t)b * cap + s)];
                    se2gpu::se3map(&Twc[12 * (size_t)fp], x, &posW[3 * r]);
                    se2gpu::se3map(tcr, x, v);
                    calcSE3toXYZInfo(Point3f{x[0], x[1], x[2]}, &Twc[12 * (size_t)fp], &Tcw[12 * (size_t)fn], &Twc[12 * (size_t)fn], fx,
                                     &infoPrev[9 * r], &info[9 * r]);
                } else if (midx[r] >= 0) {
                    const int q = midx[r], fm = main_frame[q];
                    const KeyPoint &k1 = kps[(size_t)fm * cap + main_ftr[q]], &k2 = kps[(size_t)fn * cap + j];
                    const float pt1[2] = {k1.pt.x, k1.pt.y}, pt2[2] = {k2.pt.x, k2.pt.y};
                    float x3d[3], pn[3];
                    se2gpu::triangulate_dlt(pt1, pt2, &P[12 * (size_t)fm], &P[12 * (size_t)fn], x3d);
                    se2gpu::se3map(&Tcw[12 * (size_t)fn], x3d, pn);
                    const bool acc = acceptNewObserve(Point3f{pn[0], pn[1], pn[2]}, Point3f{normal[3 * q], normal[3 * q + 1], normal[3 * q + 2]},
                                                      main_octave[q], k2.octave, dist[2 * q], dist[2 * q + 1]);
                    if (acc && !(pn[2] > upper || pn[2] < lower)) {   // LocalMapper.cpp:134
                        calcSE3toXYZInfo(Point3f{pn[0], pn[1], pn[2]}, &Twc[12 * (size_t)fn], &Tcw[12 * (size_t)fm], &Twc[12 * (size_t)fm], fx,
                                         &info[9 * r], other);
                        v[0] = pn[0]; v[1] = pn[1]; v[2] = pn[2];
                    }
                }
            }
        }
    };
    DeviceFrameSet fs;
    fs.kps = kps.data(); fs.counts = counts.data(); fs.cap = cap; fs.nframes = nframes;
    FramePoseSet ps;
    ps.Tcw = Tcw.data(); ps.Twc = Twc.data(); ps.P = P.data(); ps.idKF = idkf.data();
    std::vector<int32_t> status(npts);
    std::vector<Point3f> pos(npts), oview(of.size() + 1);
    std::vector<float> oinfo(9 * of.size() + 9);
    auto parallax = [&]() {
        for (int p = 0; p < npts; ++p)
            status[p] = updateParallax(fs, ps, &of[ptr[p]], &ok[ptr[p]], ptr[p + 1] - ptr[p], false, nw[p], fx, lower, upper, nullptr,
                                       &pos[p], &oview[ptr[p]], &oinfo[9 * (size_t)ptr[p]]).status;
    };
    correspd();
    parallax();
    save(d, "host_view.f32", view);
    save(d, "host_status.i32", status);
    windows("correspd", correspd);
    windows("parallax", parallax);
    return 0;
}
