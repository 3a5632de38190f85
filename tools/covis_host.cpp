// Host baseline of tools/covis_bench.py: the host functions of include/se2lam_amd/Covisibility.h on ONE thread over the tables
// the bench dumped into a directory (raw little-endian arrays).
//   head.i32 = {nframes, cap, m, nobs, jobs, nlocal, nref}; counts / ptr / obs_frame / obs_ftr (.i32), null / good (.u8);
//   job_new.i32 (jobs), local.i32 (jobs x nlocal), refs.i32 (jobs x nlocal x nref)
// Per job: updateCovisibility(new, local) and isRedundant(local[i], refs[i]) for every local key frame.
// Writes host_connect.u8 and host_redundant.u8 (jobs x nlocal) and prints, in ms, median / p10 / p90 over 5 windows of at
// least 0.3 s each:  "index <3>  covis <3>  redundant <3>".
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "se2lam_amd/Covisibility.h"

using namespace se2lam_amd;

template <typename T>
static std::vector<T> load(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename F>
static void windows(const char* name, F fn) {
    using clk = std::chrono::steady_clock;
    fn();
    std::vector<double> ms;
    for (int w = 0; w < 5; ++w) {
        int n = 0;
        const auto t0 = clk::now();
        double dt = 0;
        do {
            fn();
            ++n;
            dt = std::chrono::duration<double>(clk::now() - t0).count();
        } while (dt < 0.3);
        ms.push_back(1e3 * dt / n);
    }
    std::sort(ms.begin(), ms.end());
    std::printf("%s %.6f %.6f %.6f ", name, ms[2], ms[0], ms[4]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    const auto head = load<int32_t>(d + "head.i32");
    const auto counts = load<int32_t>(d + "counts.i32"), ptr = load<int32_t>(d + "ptr.i32"), of = load<int32_t>(d + "obs_frame.i32"),
               ok = load<int32_t>(d + "obs_ftr.i32"), jobNew = load<int32_t>(d + "job_new.i32"), local = load<int32_t>(d + "local.i32"),
               refs = load<int32_t>(d + "refs.i32");
    const auto null = load<uint8_t>(d + "null.u8"), good = load<uint8_t>(d + "good.u8");
    const int jobs = head[4], nlocal = head[5], nref = head[6];
    CovisHostView view;
    view.nframes = head[0]; view.cap = head[1]; view.m = head[2]; view.nobs = head[3];
    view.counts = counts.data(); view.mpPtr = ptr.data(); view.obsFrame = of.data(); view.obsFtr = ok.data();
    view.mpNull = null.data(); view.goodPrl = good.data();
    windows("index", [&] { view.index(); });
    std::vector<uint8_t> connect((size_t)jobs * nlocal, 0), redundant((size_t)jobs * nlocal, 0);
    windows("covis", [&] {
        for (int j = 0; j < jobs; ++j) {
            const std::vector<int> loc(local.begin() + (size_t)j * nlocal, local.begin() + (size_t)(j + 1) * nlocal);
            std::fill(connect.begin() + (size_t)j * nlocal, connect.begin() + (size_t)(j + 1) * nlocal, 0);
            for (int kf : updateCovisibility(view, jobNew[j], loc))
                connect[(size_t)j * nlocal + (std::find(loc.begin(), loc.end(), kf) - loc.begin())] = 1;
        }
    });
    windows("redundant", [&] {
        for (size_t i = 0; i < (size_t)jobs * nlocal; ++i) {
            const std::vector<int> r(refs.begin() + i * nref, refs.begin() + (i + 1) * nref);
            redundant[i] = isRedundant(view, local[i], r) ? 1 : 0;
        }
    });
    std::printf("\n");
    std::ofstream(d + "host_connect.u8", std::ios::binary).write(reinterpret_cast<const char*>(connect.data()), (std::streamsize)connect.size());
    std::ofstream(d + "host_redundant.u8", std::ios::binary).write(reinterpret_cast<const char*>(redundant.data()), (std::streamsize)redundant.size());
    return 0;
}
