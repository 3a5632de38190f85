// ORBVocabulary (/root/reference/include/se2lam/ORBVocabulary.h: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>,
// /root/reference/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) - the three calls se2lam makes:
//   loadFromBinaryFile(strVocFile)                        OdoSLAM.cpp:45          (TemplatedVocabulary.h:1478-1521)
//   transform(vCurrentDesc, mBowVec, mFeatVec, 4)         KeyFrame.cpp:251        (TemplatedVocabulary.h:1150-1216, 1241-1280)
//   score(BowVecCurr, BowVec)                             GlobalMapper.cpp:237, Localizer.cpp:360   (ScoringObject.cpp)
// Host code by design ("SearchByBoW with host DBoW2 transform"): a key frame's 1000 descriptors walk
// a k-ary tree of depth L once per key frame.  What it produces for the device is the FeatureVector in the CSR form that
// se2gpu_search_by_bow / ORBmatcher::SearchByBoW take (FeatureVectorCSR::view()).
//
// The tree lives in flat arrays; nothing of DBoW2, OpenCV or boost is needed.  Restated from the file format and the
// algorithm, not compiled from the reference's sources.  Faithful details:
//   * children keep the order in which their records appear in the file; the nearest child is the FIRST one at the minimal
//     Hamming distance (`d < best_d`, TemplatedVocabulary.h:1263-1272);
//   * a word with weight 0 ("stopped") contributes neither to the BowVector nor to the FeatureVector (:1182, :1203);
//   * TF_IDF / TF add the word's stored weight once per occurrence, IDF / BINARY once per word; L1, L2, chi-square, KL and
//     Bhattacharyya scoring normalise the vector (L1 norm, L2 for L2 scoring), dot-product scoring divides by the number of
//     words instead (:1190-1196) - only for TF_IDF / TF, as in the reference;
//   * the node recorded for a feature is the one `levelsup` levels above the leaves (L - levelsup from the root), the root
//     when that is not positive.
// Deviations (both documented, neither reachable with a well-formed vocabulary):
//   * the reference's loader reads one record past the end of the file (`while (!f.eof())`) and so appends a copy of the
//     last node as an extra child of its parent; being last among equal distances it is never chosen, and it is not
//     created here - size() is the true number of words (the reference reports one more);
//   * if a leaf is reached above level L - levelsup the reference leaves the node id uninitialised; here it is the leaf.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ORBmatcher.h"   // FeatureVectorView
#include "VocabularyTrain.h"
#include "VocabularyTree.h"

namespace se2lam_amd {

typedef uint32_t WordId;
typedef uint32_t NodeId;
typedef double WordValue;

enum WeightingType { TF_IDF = 0, TF = 1, IDF = 2, BINARY = 3 };                                          // BowVector.h:38-44
enum ScoringType { L1_NORM = 0, L2_NORM = 1, CHI_SQUARE = 2, KL = 3, BHATTACHARYYA = 4, DOT_PRODUCT = 5 };  // :47-55

// DBoW2::BowVector (std::map<WordId, WordValue>) as a vector sorted by word id
struct BowVector {
    std::vector<WordId> word;
    std::vector<WordValue> value;
    bool empty() const { return word.empty(); }
    size_t size() const { return word.size(); }
    void clear() { word.clear(); value.clear(); }
};

// DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) as CSR: ascending node ids, ascending feature indices
struct FeatureVectorCSR {
    std::vector<int32_t> nodes, ptr, idx;
    bool empty() const { return nodes.empty(); }
    void clear() { nodes.clear(); ptr.clear(); idx.clear(); }
    FeatureVectorView view(const uint8_t* hasMapPoint = nullptr) const {
        FeatureVectorView v;
        v.nodes = nodes.data(); v.ptr = ptr.data(); v.idx = idx.data();
        v.numNodes = (int)nodes.size();
        v.hasMapPoint = hasMapPoint;
        return v;
    }
};

class ORBVocabulary {
public:
    static const int kDescBytes = 32;   // FORB::L

    bool empty() const { return m_words.empty(); }
    unsigned size() const { return (unsigned)m_words.size(); }   // number of words
    int getBranchingFactor() const { return m_k; }
    int getDepthLevels() const { return m_L; }
    WeightingType getWeightingType() const { return m_weighting; }
    ScoringType getScoringType() const { return m_scoring; }
    unsigned nodes() const { return (unsigned)m_parent.size(); }   // incl. the root (node 0)

    // the file format and every check on it live in VocabularyTree.h, which the device vocabulary (se2gpu_voc_load) shares
    bool loadFromBinaryFile(const std::string& filename) {
        clear();
        VocabularyTree t;
        if (!t.loadFromBinaryFile(filename)) return false;
        adopt(t);
        return true;
    }

    // create(training_features, k, L, weighting, scoring)   (TemplatedVocabulary.h:573-1020) - the algorithm is stated in
    // VocabularyTrain.h; this is its straight depth-first restatement with value semantics, single thread, and what the
    // device path (se2gpu_voc_train) equals bit for bit.  desc: the documents' descriptors concatenated, counts[ndocs] (a
    // negative count is an empty document).
    // false (and empty) when the parameters are refused.  The weights are rounded to float, so the result is what create
    // followed by saveToBinaryFile and loadFromBinaryFile gives.
    bool create(const uint8_t* desc, const int32_t* counts, int ndocs, int k, int L, int weighting, int scoring, uint64_t seed,
                TrainStats* stats = nullptr, int max_iters = 0) {
        clear();
        if (stats) *stats = TrainStats();
        if (!voctrain::paramsOk(k, L, scoring, weighting) || ndocs < 1 || !counts || max_iters < 0) return false;
        int64_t total = 0;
        std::vector<int32_t> cnt(ndocs);   // a negative count is an empty document, as se2gpu_voc_train clamps it
        for (int d = 0; d < ndocs; ++d) {
            cnt[d] = counts[d] > 0 ? counts[d] : 0;
            if (cnt[d] > voctrain::kMaxDocFeatures) return false;
            total += cnt[d];
        }
        if (total == 0 || total > INT32_MAX || !desc) return false;
        Trainer tr;
        tr.feat = desc; tr.k = k; tr.L = L; tr.max_iters = max_iters > 0 ? max_iters : voctrain::kDefaultMaxIters;
        tr.parent.push_back(0);
        tr.desc.assign(kDescBytes, 0);
        std::vector<int32_t> all((size_t)total);
        for (int32_t i = 0; i < (int32_t)total; ++i) all[i] = i;
        tr.step(0, all, 1, voctrain::rootKey(seed));
        const uint32_t N = (uint32_t)tr.parent.size();
        std::vector<uint8_t> leaf(N, 1);
        for (uint32_t id = 1; id < N; ++id) leaf[tr.parent[id]] = 0;
        leaf[0] = 0;
        std::vector<double> w(N, 0.0);
        for (uint32_t id = 1; id < N; ++id) w[id] = leaf[id] ? 1.0 : 0.0;
        VocabularyTree t;
        if (!t.assign(k, L, scoring, weighting, N, tr.parent.data(), tr.desc.data(), w.data(), leaf.data())) return false;
        adopt(t);
        if (weighting == TF_IDF || weighting == IDF) {   // setNodeWeights: a real walk of every training descriptor
            std::vector<int32_t> ni(m_words.size(), 0), last_doc(m_words.size(), -1);
            const uint8_t* f = desc;
            for (int d = 0; d < ndocs; ++d)
                for (int i = 0; i < cnt[d]; ++i, f += kDescBytes) {
                    WordId id; WordValue wv;
                    transform(f, id, wv);
                    if (last_doc[id] != d) { last_doc[id] = d; ++ni[id]; }
                }
            for (size_t wd = 0; wd < m_words.size(); ++wd) m_weight[m_words[wd]] = (double)voctrain::idfWeight(ndocs, ni[wd]);
        }
        tr.stats.nodes = (int32_t)N;
        tr.stats.words = (int32_t)m_words.size();
        for (uint32_t id : m_words) tr.stats.zero_weight_words += !(m_weight[id] > 0);
        if (stats) *stats = tr.stats;
        return true;
    }

    // the reference's call line - create(training_features, k, L, weighting, scoring) with training_features a
    // std::vector<std::vector<cv::Mat>> of 1 x 32 rows - plus the seed that replaces DBoW2's global rand() stream
    template <class Row>
    bool create(const std::vector<std::vector<Row>>& training_features, int k, int L, int weighting, int scoring, uint64_t seed,
                TrainStats* stats = nullptr, int max_iters = 0) {
        std::vector<uint8_t> rows;
        std::vector<int32_t> counts;
        for (const auto& doc : training_features) {
            counts.push_back((int32_t)doc.size());
            for (const auto& r : doc) rows.insert(rows.end(), r.data, r.data + kDescBytes);
        }
        return create(rows.data(), counts.data(), (int)counts.size(), k, L, weighting, scoring, seed, stats, max_iters);
    }

    // the file TemplatedVocabulary::saveToBinaryFile (:1526-1546) writes
    bool saveToBinaryFile(const std::string& filename) const {
        return VocabularyTree::writeBinaryFile(filename, m_k, m_L, (int)m_scoring, (int)m_weighting, nodes(), m_parent.data(), m_desc.data(),
                                               m_weight.data(), m_leaf.data());
    }

    // FORB::distance (FORB.cpp:82-102): bits that differ
    static int distance(const uint8_t* a, const uint8_t* b) {
        int d = 0;
        for (int i = 0; i < kDescBytes; i += 8) {
            uint64_t x, y;
            std::memcpy(&x, a + i, 8); std::memcpy(&y, b + i, 8);
            d += __builtin_popcountll(x ^ y);
        }
        return d;
    }

    // transform(feature, word_id, weight, &nid, levelsup)   (TemplatedVocabulary.h:1241-1280)
    void transform(const uint8_t* feature, WordId& word_id, WordValue& weight, NodeId* nid = nullptr, int levelsup = 0) const {
        const int nid_level = m_L - levelsup;
        bool nid_set = false;
        if (nid_level <= 0 && nid) { *nid = 0; nid_set = true; }
        int32_t final_id = 0, current_level = 0;
        do {
            ++current_level;
            const int32_t c0 = m_child_ptr[final_id], c1 = m_child_ptr[final_id + 1];
            final_id = m_child[c0];
            int best = distance(feature, &m_desc[(size_t)final_id * kDescBytes]);
            for (int32_t c = c0 + 1; c < c1; ++c) {
                const int32_t id = m_child[c];
                const int d = distance(feature, &m_desc[(size_t)id * kDescBytes]);
                if (d < best) { best = d; final_id = id; }
            }
            if (nid && current_level == nid_level) { *nid = (NodeId)final_id; nid_set = true; }
        } while (m_child_ptr[final_id + 1] > m_child_ptr[final_id]);   // Node::isLeaf() = children.empty()
        if (nid && !nid_set) *nid = (NodeId)final_id;
        word_id = (WordId)m_word[final_id];
        weight = m_weight[final_id];
    }

    // transform(features, v, fv, levelsup)   (TemplatedVocabulary.h:1150-1216); descriptors: n x 32 bytes, row-major
    void transform(const uint8_t* descriptors, int n, BowVector& v, FeatureVectorCSR& fv, int levelsup) const {
        v.clear();
        fv.clear();
        if (empty()) return;
        std::vector<WordValue> acc(m_words.size(), 0.0);
        std::vector<uint8_t> seen(m_words.size(), 0);
        std::vector<int32_t> node_of(n, -1);
        const bool once = m_weighting == IDF || m_weighting == BINARY;   // addIfNotExist instead of addWeight
        for (int i = 0; i < n; ++i) {
            WordId id; NodeId nid; WordValue w;
            transform(descriptors + (size_t)i * kDescBytes, id, w, &nid, levelsup);
            if (!(w > 0)) continue;   // stopped
            if (!seen[id]) { seen[id] = 1; acc[id] = w; }
            else if (!once) acc[id] += w;
            node_of[i] = (int32_t)nid;
        }
        for (size_t id = 0; id < acc.size(); ++id)
            if (seen[id]) { v.word.push_back((WordId)id); v.value.push_back(acc[id]); }
        const bool must = m_scoring != DOT_PRODUCT;
        if (!once && !v.empty() && !must) {
            const double nd = (double)v.size();
            for (auto& x : v.value) x /= nd;
        }
        if (must) {   // BowVector::normalize (BowVector.cpp:62-84)
            double norm = 0.0;
            if (m_scoring == L2_NORM) { for (double x : v.value) norm += x * x; norm = std::sqrt(norm); }
            else for (double x : v.value) norm += std::fabs(x);
            if (norm > 0.0) for (auto& x : v.value) x /= norm;
        }
        // FeatureVector: node -> features, both ascending (counting sort over the node ids that occur)
        std::vector<int32_t> cnt(nodes() + 1, 0);
        for (int i = 0; i < n; ++i) if (node_of[i] >= 0) ++cnt[node_of[i] + 1];
        std::vector<int32_t> start(nodes(), -1);
        fv.ptr.push_back(0);
        for (uint32_t node = 0; node < nodes(); ++node)
            if (cnt[node + 1]) {
                start[node] = fv.ptr.back();
                fv.nodes.push_back((int32_t)node);
                fv.ptr.push_back(fv.ptr.back() + cnt[node + 1]);
            }
        fv.idx.assign(fv.ptr.back(), 0);
        for (int i = 0; i < n; ++i) if (node_of[i] >= 0) fv.idx[start[node_of[i]]++] = i;
    }

    // the reference's call line unchanged - `_pVoc->transform(vCurrentDesc, mBowVec, mFeatVec, 4)` (KeyFrame.cpp:248-251) with
    // vCurrentDesc = toDescriptorVector(descriptors), a std::vector<cv::Mat> of 1 x 32 rows: any row type with a `data`
    // member pointing at the 32 descriptor bytes
    template <class Row>
    void transform(const std::vector<Row>& features, BowVector& v, FeatureVectorCSR& fv, int levelsup) const {
        std::vector<uint8_t> rows(features.size() * (size_t)kDescBytes);
        for (size_t i = 0; i < features.size(); ++i) std::memcpy(&rows[i * kDescBytes], features[i].data, kDescBytes);
        transform(rows.data(), (int)features.size(), v, fv, levelsup);
    }

    // score(a, b): the vectors are sorted and normalised as transform() leaves them   (ScoringObject.cpp)
    double score(const BowVector& a, const BowVector& b) const {
        double s = 0.0;
        size_t i = 0, j = 0;
        while (i < a.size() && j < b.size()) {
            if (a.word[i] == b.word[j]) {
                const double vi = a.value[i], wi = b.value[j];
                switch (m_scoring) {
                    case L1_NORM: s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi); break;
                    case L2_NORM: case DOT_PRODUCT: s += vi * wi; break;
                    case CHI_SQUARE: if (vi + wi != 0.0) s += vi * wi / (vi + wi); break;
                    case BHATTACHARYYA: s += std::sqrt(vi * wi); break;
                    case KL: break;   // needs the words only one vector has as well: below
                }
                ++i; ++j;
            } else if (a.word[i] < b.word[j]) ++i;
            else ++j;
        }
        switch (m_scoring) {
            case L1_NORM: return -s / 2.0;                                      // 1 - 0.5 ||v - w||_1, in [0, 1]
            case L2_NORM: return s >= 1.0 ? 1.0 : 1.0 - std::sqrt(1.0 - s);
            case CHI_SQUARE: return 2.0 * s;
            case KL: return scoreKL(a, b);
            default: return s;
        }
    }

    void clear() {
        m_k = 0; m_L = 0; m_scoring = L1_NORM; m_weighting = TF_IDF;
        m_parent.clear(); m_child_ptr.clear(); m_child.clear(); m_desc.clear(); m_weight.clear(); m_word.clear(); m_leaf.clear();
        m_words.clear();
    }

    // flat read access (tests, device upload of the tree in a later round)
    const std::vector<int32_t>& parents() const { return m_parent; }
    const std::vector<int32_t>& childPtr() const { return m_child_ptr; }
    const std::vector<int32_t>& children() const { return m_child; }
    const std::vector<uint8_t>& descriptors() const { return m_desc; }
    const std::vector<WordValue>& weights() const { return m_weight; }
    const std::vector<int32_t>& wordOfNode() const { return m_word; }

private:
    void adopt(VocabularyTree& t) {
        m_k = t.k; m_L = t.L;
        m_scoring = (ScoringType)t.scoring; m_weighting = (WeightingType)t.weighting;
        m_parent.swap(t.parent); m_child_ptr.swap(t.child_ptr); m_child.swap(t.child); m_word.swap(t.word);
        m_desc.swap(t.desc); m_leaf.swap(t.leaf); m_weight.swap(t.weight); m_words.swap(t.words);
    }

    // HKmeansStep and what it calls (VocabularyTrain.h); nodes are appended in DBoW2's depth-first id order
    struct Trainer {
        const uint8_t* feat = nullptr;
        int k = 0, L = 0, max_iters = 0;
        std::vector<int32_t> parent;
        std::vector<uint8_t> desc;
        TrainStats stats;
        typedef std::vector<uint8_t> Centres;   // 32 bytes per cluster

        const uint8_t* f(int32_t i) const { return feat + (size_t)i * kDescBytes; }

        void seed(const std::vector<int32_t>& mem, uint64_t key, Centres& c) const {
            const int n = (int)mem.size();
            uint32_t j = 0;
            const int first = (int)(voctrain::draw(key, j++) * (double)n);
            c.assign(f(mem[first]), f(mem[first]) + kDescBytes);
            std::vector<int> md(n);
            for (int m = 0; m < n; ++m) md[m] = distance(f(mem[m]), c.data());
            while ((int)c.size() < k * kDescBytes) {
                const uint8_t* newest = &c[c.size() - kDescBytes];
                int64_t sum = 0;
                for (int m = 0; m < n; ++m) {
                    if (md[m] > 0) { const int d = distance(f(mem[m]), newest); if (d < md[m]) md[m] = d; }
                    sum += md[m];
                }
                if (sum == 0) break;
                double cut;
                do cut = voctrain::draw(key, j++) * (double)sum; while (cut == 0.0);
                int pick = n - 1;
                int64_t running = 0;
                for (int m = 0; m < n; ++m) {
                    running += md[m];
                    if ((double)running >= cut) { pick = m; break; }
                }
                c.insert(c.end(), f(mem[pick]), f(mem[pick]) + kDescBytes);
            }
        }

        void step(int32_t parent_id, const std::vector<int32_t>& mem, int level, uint64_t key) {
            const int n = (int)mem.size();
            if (n == 0) return;
            Centres c;
            std::vector<int> asg(n);
            int ncl;
            if (n <= k) {
                ++stats.trivial_nodes;
                ncl = n;
                for (int m = 0; m < n; ++m) { c.insert(c.end(), f(mem[m]), f(mem[m]) + kDescBytes); asg[m] = m; }
            } else {
                ++stats.kmeans_nodes;
                seed(mem, key, c);
                ncl = (int)c.size() / kDescBytes;
                if (ncl < k) ++stats.short_seeded_nodes;
                std::vector<int> cur(n);
                int iters = 0;
                for (;;) {
                    if (iters > 0) {   // the means of the previous assignment; a cluster without members keeps its centre
                        std::vector<int> bits((size_t)ncl * 256, 0), cnt(ncl, 0);
                        for (int m = 0; m < n; ++m) {
                            const uint8_t* p = f(mem[m]);
                            int* b = &bits[(size_t)asg[m] * 256];
                            ++cnt[asg[m]];
                            for (int i = 0; i < kDescBytes; ++i)
                                for (int q = 0; q < 8; ++q) b[i * 8 + q] += (p[i] >> q) & 1;
                        }
                        for (int cl = 0; cl < ncl; ++cl) {
                            if (!cnt[cl]) continue;
                            const int need = voctrain::majorityThreshold(cnt[cl]);
                            for (int i = 0; i < kDescBytes; ++i) {
                                uint8_t v = 0;
                                for (int q = 0; q < 8; ++q) v |= (uint8_t)((bits[(size_t)cl * 256 + i * 8 + q] >= need) << q);
                                c[(size_t)cl * kDescBytes + i] = v;
                            }
                        }
                    }
                    for (int m = 0; m < n; ++m) {
                        int best = 0, bd = distance(f(mem[m]), c.data());
                        for (int cl = 1; cl < ncl; ++cl) {
                            const int d = distance(f(mem[m]), &c[(size_t)cl * kDescBytes]);
                            if (d < bd) { bd = d; best = cl; }
                        }
                        cur[m] = best;
                    }
                    ++iters;
                    const bool same = iters > 1 && cur == asg;
                    asg = cur;
                    if (same) break;
                    if (iters >= max_iters) { ++stats.capped_nodes; break; }
                }
                stats.lloyd_iters_total += iters;
                if (iters > stats.lloyd_iters_max) stats.lloyd_iters_max = iters;
            }
            std::vector<std::vector<int32_t>> groups(ncl);
            for (int m = 0; m < n; ++m) groups[asg[m]].push_back(mem[m]);
            std::vector<int32_t> ids(ncl, -1);
            for (int cl = 0; cl < ncl; ++cl) {
                if (groups[cl].empty()) { ++stats.empty_clusters; continue; }
                ids[cl] = (int32_t)parent.size();
                parent.push_back(parent_id);
                desc.insert(desc.end(), &c[(size_t)cl * kDescBytes], &c[(size_t)cl * kDescBytes] + kDescBytes);
            }
            if (level < L)
                for (int cl = 0; cl < ncl; ++cl)
                    if (groups[cl].size() > 1) step(ids[cl], groups[cl], level + 1, voctrain::childKey(key, cl));
        }
    };

    // KLScoring::score (ScoringObject.cpp:175-222): sum over the words of a; a word b lacks counts with log(eps)
    double scoreKL(const BowVector& a, const BowVector& b) const {
        const double log_eps = std::log(2.220446049250313e-16);   // GeneralScoring::LOG_EPS = log(DBL_EPSILON)
        double s = 0.0;
        size_t j = 0;
        for (size_t i = 0; i < a.size(); ++i) {
            while (j < b.size() && b.word[j] < a.word[i]) ++j;
            const double vi = a.value[i];
            if (j < b.size() && b.word[j] == a.word[i]) {
                const double wi = b.value[j];
                if (vi != 0.0 && wi != 0.0) s += vi * std::log(vi / wi);
            } else if (vi != 0.0) {
                s += vi * (std::log(vi) - log_eps);
            }
        }
        return s;
    }

    int m_k = 0, m_L = 0;
    ScoringType m_scoring = L1_NORM;
    WeightingType m_weighting = TF_IDF;
    std::vector<int32_t> m_parent, m_child_ptr, m_child, m_word;
    std::vector<uint8_t> m_desc, m_leaf;
    std::vector<WordValue> m_weight;
    std::vector<uint32_t> m_words;   // word id -> node id
};

}  // namespace se2lam_amd
