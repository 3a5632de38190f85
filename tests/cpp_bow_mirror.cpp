// Batch driver of the host vocabulary include/se2lam_amd/ORBVocabulary.h for tests/test_bow_gpu.py and tools/bow_bench.py
// (host only, no device).  Everything travels as raw little-endian binary, so doubles arrive bit for bit.
//   cpp_bow_mirror transform <voc.bin> <in.bin> <levelsup> <out.bin> [threads [repeats]]
//       in:  int32 nframes, cap, counts[nframes]; uint8 desc[nframes * cap * 32]
//       out: per frame int32 nb, uint32 word[nb], double value[nb], int32 nn, nodes[nn], ptr[nn + 1], idx[ptr[nn]]
//   cpp_bow_mirror score <voc.bin> <vecs.bin> <out.bin> [threads [repeats]]
//       vecs: int32 nq, ndb; then nq + ndb vectors: int32 n, uint32 word[n], double value[n]
//       out:  double score[nq * ndb]  (score(query q, entry e) at q * ndb + e)
// With `threads` the frames / entries are split over that many std::threads; the computation alone is timed `repeats` times
// and printed as "SECONDS <s> <s> ...".
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <thread>
#include <vector>

#include "se2lam_amd/ORBVocabulary.h"

using namespace se2lam_amd;

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize(n > 0 ? (size_t)n : 0);
    if (n > 0 && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear();
    std::fclose(f);
    return v;
}

template <class F>
static std::vector<double> run(int n, int threads, int repeats, F body) {
    std::vector<double> times;
    for (int r = 0; r < repeats; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        if (threads <= 1) {
            for (int i = 0; i < n; ++i) body(i);
        } else {
            std::vector<std::thread> pool;
            for (int t = 0; t < threads; ++t)
                pool.emplace_back([&, t] { for (int i = t; i < n; i += threads) body(i); });
            for (auto& th : pool) th.join();
        }
        times.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    return times;
}

static void print_times(const std::vector<double>& s) {
    std::printf("SECONDS");
    for (double t : s) std::printf(" %.9g", t);
    std::printf("\n");
}

template <class T>
static void put(std::vector<uint8_t>& o, const T* p, size_t n) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
    o.insert(o.end(), b, b + n * sizeof(T));
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string mode = argv[1];
    ORBVocabulary voc;
    if (!voc.loadFromBinaryFile(argv[2])) { std::printf("LOAD failed\n"); return 1; }
    const std::vector<uint8_t> in = slurp(argv[3]);
    if (in.size() < 8) return 3;
    std::vector<uint8_t> out;
    if (mode == "transform") {
        if (argc < 6) return 2;
        const int levelsup = std::atoi(argv[4]);
        const int threads = argc > 6 ? std::atoi(argv[6]) : 1, repeats = argc > 7 ? std::atoi(argv[7]) : 1;
        int32_t nframes, cap;
        std::memcpy(&nframes, in.data(), 4); std::memcpy(&cap, in.data() + 4, 4);
        std::vector<int32_t> counts(nframes);
        std::memcpy(counts.data(), in.data() + 8, 4 * (size_t)nframes);
        const uint8_t* desc = in.data() + 8 + 4 * (size_t)nframes;
        if (in.size() != 8 + 4 * (size_t)nframes + (size_t)nframes * cap * 32) return 3;
        std::vector<BowVector> bow(nframes);
        std::vector<FeatureVectorCSR> fv(nframes);
        const std::vector<double> s = run(nframes, threads, repeats,
                             [&](int f) { voc.transform(desc + (size_t)f * cap * 32, counts[f], bow[f], fv[f], levelsup); });
        print_times(s);
        for (int f = 0; f < nframes; ++f) {
            const int32_t nb = (int32_t)bow[f].size(), nn = (int32_t)fv[f].nodes.size();
            put(out, &nb, 1); put(out, bow[f].word.data(), nb); put(out, bow[f].value.data(), nb);
            put(out, &nn, 1); put(out, fv[f].nodes.data(), nn); put(out, fv[f].ptr.data(), fv[f].ptr.size());
            put(out, fv[f].idx.data(), fv[f].idx.size());
        }
        std::ofstream(argv[5], std::ios::binary).write((const char*)out.data(), (std::streamsize)out.size());
    } else if (mode == "score") {
        const int threads = argc > 5 ? std::atoi(argv[5]) : 1, repeats = argc > 6 ? std::atoi(argv[6]) : 1;
        int32_t nq, ndb;
        std::memcpy(&nq, in.data(), 4); std::memcpy(&ndb, in.data() + 4, 4);
        std::vector<BowVector> v(nq + ndb);
        size_t at = 8;
        for (auto& b : v) {
            int32_t n;
            std::memcpy(&n, in.data() + at, 4); at += 4;
            b.word.resize(n); b.value.resize(n);
            std::memcpy(b.word.data(), in.data() + at, 4 * (size_t)n); at += 4 * (size_t)n;
            std::memcpy(b.value.data(), in.data() + at, 8 * (size_t)n); at += 8 * (size_t)n;
        }
        if (at != in.size()) return 3;
        std::vector<double> sc((size_t)nq * ndb);
        const std::vector<double> s = run(ndb, threads, repeats, [&](int e) {
            for (int q = 0; q < nq; ++q) sc[(size_t)q * ndb + e] = voc.score(v[q], v[nq + e]);
        });
        print_times(s);
        std::ofstream(argv[4], std::ios::binary).write((const char*)sc.data(), (std::streamsize)(sc.size() * 8));
    } else {
        return 2;
    }
    return 0;
}
