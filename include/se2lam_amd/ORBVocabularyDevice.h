// ORBVocabulary on the device: the reference's call lines (ORBVocabulary.h gives their places in the reference)
//   create(training_features, k, L, weighting, scoring) [+ seed], saveToBinaryFile(file)
//   loadFromBinaryFile(strVocFile)
//   transform(vCurrentDesc, mBowVec, mFeatVec, 4)
//   score(BowVecCurr, BowVec)
// over the C ABI of libse2gpu (se2gpu.h, "DBoW2 vocabulary"), plus what the ABI adds: BowDatabaseDevice keeps the key
// frames' BowVectors on the device and answers the whole candidate loop of GlobalMapper::DetectLoopClose /
// Localizer::DetectLoopClose with one call (scoreAll / detectLoop).  Every result equals the host class ORBVocabulary bit for
// bit; it reuses that header's BowVector / FeatureVectorCSR.  When to stay on the host class: INTEGRATION.md.
// One ORBVocabularyDevice per calling thread (it owns a stream); copies share the tree on the device.
#pragma once
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../se2gpu.h"
#include "ORBVocabulary.h"

namespace se2lam_amd {

class BowDatabaseDevice;

class ORBVocabularyDevice {
public:
    ORBVocabularyDevice() = default;
    // a second context over the same tree, for another thread (the reference shares one vocabulary between its threads)
    ORBVocabularyDevice(const ORBVocabularyDevice& o) : m_voc(o.m_voc), m_maxFeatures(o.m_maxFeatures) { openContext(); }
    ORBVocabularyDevice& operator=(const ORBVocabularyDevice& o) {
        if (this != &o) { m_ctx.reset(); m_voc = o.m_voc; m_maxFeatures = o.m_maxFeatures; openContext(); }
        return *this;
    }

    bool loadFromBinaryFile(const std::string& filename, int maxFeatures = 4096) {
        m_ctx.reset(); m_voc.reset();
        se2gpu_voc* v = nullptr;
        if (se2gpu_voc_load(filename.c_str(), &v) != SE2GPU_OK) return false;
        m_voc.reset(v, se2gpu_voc_destroy);
        m_maxFeatures = maxFeatures;
        return openContext();
    }

    // create(training_features, k, L, weighting, scoring) on the device (se2gpu_voc_train; the algorithm and the seed that
    // replaces DBoW2's rand() stream: VocabularyTrain.h).  desc: the documents' descriptors concatenated, counts[ndocs] - the
    // arguments of ORBVocabulary::create, whose result this equals bit for bit.  false when the parameters are refused.
    bool create(const uint8_t* desc, const int32_t* counts, int ndocs, int k, int L, int weighting, int scoring, uint64_t seed,
                TrainStats* stats = nullptr, int max_iters = 0, int maxFeatures = 4096) {
        m_ctx.reset(); m_voc.reset();
        if (ndocs < 1 || !counts) return false;
        int cap = 1;
        for (int d = 0; d < ndocs; ++d) cap = counts[d] > cap ? counts[d] : cap;
        std::vector<uint8_t> rows((size_t)ndocs * cap * 32, 0);   // the layout of se2gpu_voc_train: ndocs x cap x 32
        const uint8_t* src = desc;
        for (int d = 0; d < ndocs; ++d) {
            if (counts[d] <= 0) continue;   // a negative count is an empty document, on both classes
            std::memcpy(&rows[(size_t)d * cap * 32], src, (size_t)counts[d] * 32);
            src += (size_t)counts[d] * 32;
        }
        return createPadded(rows.data(), counts, cap, ndocs, false, k, L, weighting, scoring, seed, stats, max_iters, maxFeatures);
    }
    // the same from the layout se2gpu_orb_extract_batch_device writes (ndocs x cap x 32 bytes, counts clamped to 0..cap), in
    // host memory or, with onDevice, where the extractor left it
    bool createPadded(const uint8_t* desc, const int32_t* counts, int cap, int ndocs, bool onDevice, int k, int L, int weighting, int scoring,
                      uint64_t seed, TrainStats* stats = nullptr, int max_iters = 0, int maxFeatures = 4096) {
        m_ctx.reset(); m_voc.reset();
        se2gpu_voc_train_params p = {k, L, scoring, weighting, max_iters, seed};
        se2gpu_voc_train_stats st;
        se2gpu_voc* v = nullptr;
        if (se2gpu_voc_train(&p, desc, counts, cap, ndocs, onDevice ? 1 : 0, &v, &st) != SE2GPU_OK) return false;
        static_assert(sizeof(TrainStats) == sizeof(se2gpu_voc_train_stats), "stats layout");
        if (stats) std::memcpy(static_cast<void*>(stats), &st, sizeof st);
        m_voc.reset(v, se2gpu_voc_destroy);
        m_maxFeatures = maxFeatures;
        return openContext();
    }
    template <class Row>
    bool create(const std::vector<std::vector<Row>>& training_features, int k, int L, int weighting, int scoring, uint64_t seed,
                TrainStats* stats = nullptr, int max_iters = 0) {
        std::vector<uint8_t> rows;
        std::vector<int32_t> counts;
        for (const auto& doc : training_features) {
            counts.push_back((int32_t)doc.size());
            for (const auto& r : doc) rows.insert(rows.end(), r.data, r.data + 32);
        }
        return create(rows.data(), counts.data(), (int)counts.size(), k, L, weighting, scoring, seed, stats, max_iters);
    }

    bool saveToBinaryFile(const std::string& filename) const { return m_voc && se2gpu_voc_save(m_voc.get(), filename.c_str()) == SE2GPU_OK; }

    bool empty() const { return !m_voc || se2gpu_voc_words(m_voc.get()) <= 0; }
    unsigned size() const { return m_voc ? (unsigned)se2gpu_voc_words(m_voc.get()) : 0u; }
    int getBranchingFactor() const { return m_voc ? se2gpu_voc_k(m_voc.get()) : 0; }
    int getDepthLevels() const { return m_voc ? se2gpu_voc_L(m_voc.get()) : 0; }
    WeightingType getWeightingType() const { return (WeightingType)(m_voc ? se2gpu_voc_weighting(m_voc.get()) : 0); }
    ScoringType getScoringType() const { return (ScoringType)(m_voc ? se2gpu_voc_scoring(m_voc.get()) : 0); }

    // descriptors: n x 32 bytes, row-major
    void transform(const uint8_t* descriptors, int n, BowVector& v, FeatureVectorCSR& fv, int levelsup) const {
        v.clear(); fv.clear();
        if (empty() || n <= 0) { fv.ptr.assign(1, 0); return; }
        v.word.resize(n); v.value.resize(n);
        fv.nodes.resize(n); fv.ptr.resize((size_t)n + 1); fv.idx.resize(n);
        int nb = 0, nn = 0;
        check(se2gpu_bow_transform(ctx(), descriptors, n, levelsup, v.word.data(), v.value.data(), &nb, fv.nodes.data(), fv.ptr.data(),
                                   fv.idx.data(), &nn));
        v.word.resize(nb); v.value.resize(nb);
        fv.nodes.resize(nn); fv.ptr.resize((size_t)nn + 1); fv.idx.resize(fv.ptr[nn]);
    }

    // the reference's call line unchanged: any row type with a `data` member pointing at the 32 descriptor bytes (cv::Mat rows)
    template <class Row>
    void transform(const std::vector<Row>& features, BowVector& v, FeatureVectorCSR& fv, int levelsup) const {
        std::vector<uint8_t> rows(features.size() * (size_t)32);
        for (size_t i = 0; i < features.size(); ++i) std::memcpy(&rows[i * 32], features[i].data, 32);
        transform(rows.data(), (int)features.size(), v, fv, levelsup);
    }

    // score(a, b): one pair through a one-entry data base (for many pairs use BowDatabaseDevice)
    double score(const BowVector& a, const BowVector& b) const;

    se2gpu_bow* ctx() const {
        if (!m_ctx) throw std::runtime_error("ORBVocabularyDevice: no vocabulary loaded");
        return m_ctx.get();
    }
    const se2gpu_voc* voc() const { return m_voc.get(); }

    static void check(int rc) {
        if (rc != SE2GPU_OK) throw std::runtime_error(std::string("se2gpu: ") + se2gpu_last_error());
    }

private:
    bool openContext() {
        m_ctx.reset();
        if (!m_voc) return false;
        se2gpu_bow* c = nullptr;
        if (se2gpu_bow_create(m_voc.get(), m_maxFeatures, 1, &c) != SE2GPU_OK) return false;
        m_ctx.reset(c, se2gpu_bow_destroy);
        return true;
    }
    std::shared_ptr<se2gpu_voc> m_voc;
    std::shared_ptr<se2gpu_bow> m_ctx;
    int m_maxFeatures = 4096;
};

// The BowVectors of the map's key frames on the device, in insertion order.
class BowDatabaseDevice {
public:
    explicit BowDatabaseDevice(const ORBVocabularyDevice& voc) {
        se2gpu_bowdb* d = nullptr;
        ORBVocabularyDevice::check(se2gpu_bowdb_create(voc.voc(), &d));
        m_db.reset(d, se2gpu_bowdb_destroy);
    }
    void add(int kfId, const BowVector& v) {
        ORBVocabularyDevice::check(se2gpu_bowdb_add(m_db.get(), kfId, v.word.data(), v.value.data(), (int)v.size()));
    }
    void remove(int kfId) { ORBVocabularyDevice::check(se2gpu_bowdb_remove(m_db.get(), kfId)); }
    size_t size() const { return (size_t)se2gpu_bowdb_size(m_db.get()); }

    // scores[i] = voc.score(query, entry i)
    std::vector<double> scoreAll(const ORBVocabularyDevice& voc, const BowVector& query) const {
        std::vector<double> s(size());
        ORBVocabularyDevice::check(se2gpu_bowdb_query(m_db.get(), voc.ctx(), query.word.data(), query.value.data(), (int)query.size(), 0, 0,
                                                      0, s.data(), nullptr, nullptr, nullptr));
        return s;
    }

    // The loop of GlobalMapper::DetectLoopClose / Localizer::DetectLoopClose: the best-scoring key frame among those at least
    // minKFIdOffset ids away from curKFId.  false when none scores above 0; the comparison with the minimal accepted score
    // (GM_DCL_MIN_SCORE_BEST, 0.05 in the Localizer) stays with the caller, as in the reference.
    bool detectLoop(const ORBVocabularyDevice& voc, const BowVector& query, int curKFId, int minKFIdOffset, int& bestKFId,
                    double& scoreBest, int* bestEntry = nullptr) const {
        int entry = -1;
        ORBVocabularyDevice::check(se2gpu_bowdb_query(m_db.get(), voc.ctx(), query.word.data(), query.value.data(), (int)query.size(), 0,
                                                      curKFId, minKFIdOffset, nullptr, &entry, &bestKFId, &scoreBest));
        if (bestEntry) *bestEntry = entry;
        return entry >= 0;
    }
    se2gpu_bowdb* handle() const { return m_db.get(); }

private:
    std::shared_ptr<se2gpu_bowdb> m_db;
};

inline double ORBVocabularyDevice::score(const BowVector& a, const BowVector& b) const {
    BowDatabaseDevice db(*this);
    db.add(0, b);
    return db.scoreAll(*this, a)[0];
}

}  // namespace se2lam_amd
