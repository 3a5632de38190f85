// include/se2lam_amd/ORBVocabularyDevice.h: create / saveToBinaryFile compile as plain C++17 with -Wall -Werror and link against
// libse2gpu (tests/test_voc_train.py).  With a device (tests/test_voc_train_gpu.py) the reference's call line - a vector of
// vectors of rows - trains on the device and on the host class, and the two saved files must be equal byte for byte.
//   cpp_voc_train_device <tmp dir>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "se2lam_amd/ORBVocabularyDevice.h"

using namespace se2lam_amd;

struct Row {   // stands for cv::Mat: a `data` member pointing at the 32 descriptor bytes
    uint8_t bytes[32];
    const uint8_t* data;
};

static std::vector<char> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    const std::string tmp = argc > 1 ? argv[1] : ".";
    std::vector<std::vector<Row>> docs(7);
    uint64_t z = 12345;
    for (size_t d = 0; d < docs.size(); ++d) {
        docs[d].resize(d == 3 ? 0 : 90 + 10 * d);   // one document without descriptors
        for (Row& r : docs[d]) {
            const uint64_t proto = voctrain::splitmix64(z++) % 20;
            for (int i = 0; i < 32; ++i) r.bytes[i] = (uint8_t)(voctrain::splitmix64(proto * 64 + i) >> 13);
            const uint64_t flip = voctrain::splitmix64(z++);
            r.bytes[flip % 32] ^= (uint8_t)(1u << ((flip >> 8) % 8));   // one flipped bit
        }
        for (Row& r : docs[d]) r.data = r.bytes;
    }
    ORBVocabulary host;
    TrainStats hs, ds;
    if (!host.create(docs, 5, 3, TF_IDF, L1_NORM, 99, &hs) || host.size() == 0) { std::printf("host create failed\n"); return 1; }
    {   // a negative count is an empty document, on both classes: document 3 with -1 trains the same vocabulary
        std::vector<uint8_t> rows;
        std::vector<int32_t> counts;
        for (const auto& doc : docs) {
            counts.push_back(doc.empty() ? -1 : (int32_t)doc.size());
            for (const Row& r : doc) rows.insert(rows.end(), r.bytes, r.bytes + 32);
        }
        ORBVocabulary neg;
        TrainStats ns;
        if (!neg.create(rows.data(), counts.data(), (int)counts.size(), 5, 3, TF_IDF, L1_NORM, 99, &ns) || std::memcmp(&ns, &hs, sizeof hs) != 0 ||
            neg.descriptors() != host.descriptors() || neg.weights() != host.weights()) { std::printf("host create with a negative count differs\n"); return 1; }
        if (se2gpu_device_count() > 0) {
            ORBVocabularyDevice dneg;
            TrainStats dns;
            if (!dneg.create(rows.data(), counts.data(), (int)counts.size(), 5, 3, TF_IDF, L1_NORM, 99, &dns) || std::memcmp(&dns, &hs, sizeof hs) != 0) {
                std::printf("device create with a negative count differs\n");
                return 1;
            }
        }
    }
    ORBVocabularyDevice dev;
    if (se2gpu_device_count() <= 0) {
        const bool made = dev.create(docs, 5, 3, TF_IDF, L1_NORM, 99, &ds);
        std::printf(made ? "a vocabulary without a device?\n" : "OK (no device: create refused, %u host words)\n", host.size());
        return made ? 1 : 0;
    }
    if (!dev.create(docs, 5, 3, TF_IDF, L1_NORM, 99, &ds)) { std::printf("device create failed: %s\n", se2gpu_last_error()); return 1; }
    if (!host.saveToBinaryFile(tmp + "/host.voc") || !dev.saveToBinaryFile(tmp + "/device.voc")) { std::printf("save failed\n"); return 1; }
    const bool same = slurp(tmp + "/host.voc") == slurp(tmp + "/device.voc") && std::memcmp(&hs, &ds, sizeof hs) == 0 && dev.size() == host.size();
    BowVector a, b;
    FeatureVectorCSR fa, fb;
    host.transform(docs[0], a, fa, 1);
    dev.transform(docs[0], b, fb, 1);
    const bool same_bow = a.word == b.word && a.value == b.value && fa.nodes == fb.nodes && fa.idx == fb.idx;
    std::printf(same && same_bow ? "OK (%u words, device = host)\n" : "MISMATCH (%u words)\n", dev.size());
    return same && same_bow ? 0 : 1;
}
