// Driver of the host mirror's vocabulary training, ORBVocabulary::create (include/se2lam_amd/ORBVocabulary.h), for
// tests/test_voc_train.py, tests/test_voc_train_gpu.py and tools/voc_train_bench.py (host only, no device).  Raw little-endian
// binary both ways.
//   cpp_voc_train <in.bin> <out.bin> [<voc_out.bin> | - [repeats]]
//       in:  int32 ndocs, k, L, weighting, scoring, max_iters; uint64 seed; int32 counts[ndocs]; uint8 desc[sum(counts) * 32]
//       out: int32 ok; int32 stats[10]; int32 nodes; int32 parent[nodes]; uint8 desc[nodes * 32]; double weight[nodes];
//            uint8 leaf[nodes]      (ok = 0: the parameters were refused, nothing follows)
//       voc_out: the file saveToBinaryFile writes
// create alone is timed `repeats` times and printed as "SECONDS <s> <s> ...".
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "se2lam_amd/ORBVocabulary.h"

using namespace se2lam_amd;

template <class T>
static void put(std::vector<uint8_t>& o, const T* p, size_t n) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
    o.insert(o.end(), b, b + n * sizeof(T));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::vector<uint8_t> in;
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) return 3;
        in.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    if (in.size() < 32) return 3;
    int32_t h[6];
    uint64_t seed;
    std::memcpy(h, in.data(), 24);
    std::memcpy(&seed, in.data() + 24, 8);
    const int ndocs = h[0];
    if (ndocs < 0 || in.size() < 32 + 4 * (size_t)ndocs) return 3;
    std::vector<int32_t> counts(ndocs);
    if (ndocs) std::memcpy(counts.data(), in.data() + 32, 4 * (size_t)ndocs);
    size_t total = 0;
    for (int32_t c : counts) total += c > 0 ? (size_t)c : 0;
    const uint8_t* desc = in.data() + 32 + 4 * (size_t)ndocs;
    if (in.size() < 32 + 4 * (size_t)ndocs + total * 32) return 3;
    const int repeats = argc > 4 ? std::atoi(argv[4]) : 1;

    ORBVocabulary voc;
    TrainStats st;
    bool ok = false;
    std::printf("SECONDS");
    for (int r = 0; r < (repeats > 0 ? repeats : 1); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        ok = voc.create(desc, counts.data(), ndocs, h[1], h[2], h[3], h[4], seed, &st, h[5]);
        std::printf(" %.9g", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("\n");

    std::vector<uint8_t> out;
    const int32_t ok32 = ok;
    put(out, &ok32, 1);
    if (ok) {
        static_assert(sizeof(TrainStats) == 40, "stats layout");
        put(out, &st, 1);
        const int32_t n = (int32_t)voc.nodes();
        put(out, &n, 1);
        put(out, voc.parents().data(), n);
        put(out, voc.descriptors().data(), (size_t)n * 32);
        put(out, voc.weights().data(), n);
        std::vector<uint8_t> leaf(n);
        for (int32_t id = 0; id < n; ++id) leaf[id] = id > 0 && voc.childPtr()[id + 1] == voc.childPtr()[id];
        put(out, leaf.data(), n);
        if (argc > 3 && std::strcmp(argv[3], "-") != 0 && !voc.saveToBinaryFile(argv[3])) return 4;
    }
    std::ofstream(argv[2], std::ios::binary).write((const char*)out.data(), (std::streamsize)out.size());
    return 0;
}
