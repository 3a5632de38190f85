// include/se2lam_amd/ORBVocabularyDevice.h compiles as plain C++17 and links against libse2gpu (tests/test_bow_capi.py), and
// - given a vocabulary file and a descriptor file on a machine with a device (tests/test_bow_gpu.py) - its call lines give what
// the host class gives, bit for bit:
//   cpp_bow_device_compile [<voc.bin> <desc_a.bin> <desc_b.bin> <levelsup>]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "se2lam_amd/ORBVocabularyDevice.h"

using namespace se2lam_amd;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static bool same(const BowVector& a, const BowVector& b) { return a.word == b.word && a.value == b.value; }
static bool same(const FeatureVectorCSR& a, const FeatureVectorCSR& b) { return a.nodes == b.nodes && a.ptr == b.ptr && a.idx == b.idx; }

int main(int argc, char** argv) {
    ORBVocabularyDevice dev;
    if (se2gpu_device_count() <= 0) {
        se2gpu_voc* v = nullptr;
        const int32_t parent[2] = {0, 0};
        const uint8_t desc[64] = {0}, leaf[2] = {0, 1};
        const double weight[2] = {0.0, 1.0};
        if (se2gpu_voc_create(10, 1, 0, 0, 2, parent, desc, weight, leaf, &v) != SE2GPU_ERR_NO_DEVICE || v) return 10;
        if (dev.loadFromBinaryFile("no such file") || !dev.empty()) return 11;
        std::printf("OK (no device: se2gpu_voc_create says so)\n");
        return 0;
    }
    if (argc < 5) { std::printf("OK (a device is visible; no vocabulary given)\n"); return 0; }
    ORBVocabulary host;
    if (!host.loadFromBinaryFile(argv[1]) || !dev.loadFromBinaryFile(argv[1])) { std::printf("LOAD failed\n"); return 1; }
    if (dev.size() != host.size() || dev.getBranchingFactor() != host.getBranchingFactor() || dev.getDepthLevels() != host.getDepthLevels() ||
        dev.getScoringType() != host.getScoringType() || dev.getWeightingType() != host.getWeightingType()) return 2;
    const int levelsup = std::atoi(argv[4]);
    BowVector hb[2], db[2];
    for (int s = 0; s < 2; ++s) {
        const std::vector<uint8_t> d = slurp(argv[2 + s]);
        struct Row { const uint8_t* data; };
        std::vector<Row> vCurrentDesc;
        for (size_t i = 0; i < d.size() / 32; ++i) vCurrentDesc.push_back(Row{d.data() + 32 * i});
        FeatureVectorCSR hf, df;
        const ORBVocabulary* pHost = &host;
        const ORBVocabularyDevice* _pVoc = &dev;
        pHost->transform(vCurrentDesc, hb[s], hf, levelsup);
        _pVoc->transform(vCurrentDesc, db[s], df, levelsup);    // KeyFrame.cpp:251 with the device class
        if (!same(hb[s], db[s]) || !same(hf, df) || hb[s].empty()) { std::printf("TRANSFORM differs\n"); return 3; }
    }
    if (dev.score(db[0], db[1]) != host.score(hb[0], hb[1]) || dev.score(db[0], db[0]) != host.score(hb[0], hb[0])) {
        std::printf("SCORE differs\n");
        return 4;
    }
    ORBVocabularyDevice second(dev);                            // another thread's context over the same tree
    BowDatabaseDevice kfs(dev);
    kfs.add(3, hb[1]); kfs.add(40, hb[0]); kfs.add(41, hb[1]);
    const std::vector<double> all = kfs.scoreAll(second, hb[0]);
    if (all.size() != 3 || all[0] != host.score(hb[0], hb[1]) || all[1] != host.score(hb[0], hb[0]) || all[2] != all[0]) return 5;
    int bestKF = -1, entry = -1;
    double scoreBest = 0;
    if (!kfs.detectLoop(dev, hb[0], 45, 30, bestKF, scoreBest, &entry) || bestKF != 3 || entry != 0 || scoreBest != all[0]) return 6;
    if (!kfs.detectLoop(dev, hb[0], 100, 30, bestKF, scoreBest, &entry) || bestKF != 40 || entry != 1) return 7;
    kfs.remove(40);
    if (kfs.size() != 2 || !kfs.detectLoop(dev, hb[0], 100, 30, bestKF, scoreBest, &entry) || bestKF != 3 || entry != 0) return 8;
    std::printf("device vocabulary ran: %zu + %zu words, score %.17g\n", hb[0].size(), hb[1].size(), all[0]);
    return 0;
}
