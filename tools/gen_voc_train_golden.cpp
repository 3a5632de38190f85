// Generator of tests/golden/voc_train_dbow2.npz (driver: tools/gen_voc_train_golden.py): trains a vocabulary with the
// reference's own DBoW2 (se2lam::ORBVocabulary::create, compiled where the reference lies against oracle/_shim) and records
// every value its rand() stream hands out, so that tests/voc_train_model.py can replay the stream.
//   gen_voc_train_golden <case.bin> <voc_out.bin> <rand_out.bin>
//       case: int32 ndocs, k, L, weighting, scoring, seed; int32 counts[ndocs]; uint8 desc[sum(counts) * 32]
//       rand_out: int32 values, in the order they were drawn
// DBoW2 draws through DUtils::Random, which calls rand(); the definition below takes its place in this program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ORBVocabulary.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"

static std::vector<int32_t> g_drawn;
extern "C" int rand(void) {
    const int v = (int)random();
    g_drawn.push_back(v);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[6];
    if (std::fread(h, 4, 6, f) != 6) return 2;
    std::vector<int32_t> cnt(h[0]);
    if (std::fread(cnt.data(), 4, h[0], f) != (size_t)h[0]) return 2;
    std::vector<std::vector<cv::Mat>> feats(h[0]);
    for (int d = 0; d < h[0]; ++d)
        for (int i = 0; i < cnt[d]; ++i) {
            cv::Mat m(1, 32, CV_8U);
            if (std::fread(m.ptr<unsigned char>(), 1, 32, f) != 32) return 2;
            feats[d].push_back(m);
        }
    std::fclose(f);
    DUtils::Random::SeedRandOnce(h[5]);   // srand(seed): this process is fresh
    se2lam::ORBVocabulary voc;
    voc.create(feats, h[1], h[2], (DBoW2::WeightingType)h[3], (DBoW2::ScoringType)h[4]);
    voc.saveToBinaryFile(argv[2]);
    std::FILE* r = std::fopen(argv[3], "wb");
    if (!r) return 2;
    std::fwrite(g_drawn.data(), 4, g_drawn.size(), r);
    std::fclose(r);
    std::printf("words %u draws %zu\n", voc.size(), g_drawn.size());
    return 0;
}
