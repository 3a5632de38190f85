// The DBoW2 vocabulary tree as flat arrays, and the one place where its records are validated: shared by the host mirror
// (ORBVocabulary.h) and by the device vocabulary of libse2gpu (se2gpu_voc_create / se2gpu_voc_load, csrc/bow.hip), so that
// both refuse exactly the same input - a bad header, a parent that does not precede its child, a childless node that is
// not a leaf, a truncated file.  Plain C++, no device and no other header of the project needed.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace se2lam_amd {

struct VocabularyTree {
    static const int kDescBytes = 32;                    // FORB::L
    static const uint32_t kNodeBytes = 4 + 32 + 4 + 1;   // parent (int32), descriptor, weight (float), is_leaf

    int k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<int32_t> parent, child_ptr, child, word;   // per node (incl. the root, node 0); children in file order (CSR)
    std::vector<uint8_t> desc, leaf;
    std::vector<double> weight;                            // the file's float, widened
    std::vector<uint32_t> words;                           // word id -> node id

    void clear() { *this = VocabularyTree(); }

    static bool headerOk(int64_t nodes, int k_, int L_, int scoring_, int weighting_) {
        return nodes >= 1 && k_ >= 1 && L_ >= 0 && scoring_ >= 0 && scoring_ <= 5 && weighting_ >= 0 && weighting_ <= 3;
    }

    // The records of `nodes` nodes, node 0 being the root (its parent / descriptor / weight / leaf entries are ignored).
    // Weights are rounded to float, which is what the file format stores.  false (and empty) when the records are refused.
    bool assign(int k_, int L_, int scoring_, int weighting_, uint32_t nodes, const int32_t* parent_, const uint8_t* desc_,
                const double* weight_, const uint8_t* leaf_) {
        clear();
        if (!headerOk(nodes, k_, L_, scoring_, weighting_)) return false;
        if (nodes > 1 && !(parent_ && desc_ && weight_ && leaf_)) return false;
        k = k_; L = L_; scoring = scoring_; weighting = weighting_;
        const uint32_t N = nodes;
        parent.assign(N, 0); weight.assign(N, 0.0); word.assign(N, -1); leaf.assign(N, 0);
        desc.assign((size_t)N * kDescBytes, 0);
        std::vector<int32_t> count(N + 1, 0);
        for (uint32_t id = 1; id < N; ++id) {
            const int32_t p = parent_[id];
            if (p < 0 || (uint32_t)p >= id) { clear(); return false; }   // a parent precedes its children in the file
            parent[id] = p;
            std::memcpy(&desc[(size_t)id * kDescBytes], desc_ + (size_t)id * kDescBytes, kDescBytes);
            weight[id] = (double)(float)weight_[id];
            leaf[id] = leaf_[id] ? 1 : 0;
            if (leaf[id]) { word[id] = (int32_t)words.size(); words.push_back(id); }
            ++count[p + 1];
        }
        // children in file order (CSR)
        child_ptr.assign(N + 1, 0);
        for (uint32_t i = 0; i < N; ++i) child_ptr[i + 1] = child_ptr[i] + count[i + 1];
        child.assign(child_ptr[N], 0);
        std::vector<int32_t> fill(child_ptr.begin(), child_ptr.end() - 1);
        for (uint32_t id = 1; id < N; ++id) child[fill[parent[id]]++] = (int32_t)id;
        // a node without children must be a leaf, or a feature that reaches it could not go on
        for (uint32_t id = 0; id < N; ++id)
            if (child_ptr[id + 1] == child_ptr[id] && !(id > 0 && leaf[id]) && N > 1) { clear(); return false; }
        return true;
    }

    // header: nb_nodes (= nodes incl. root), size_node (41), k, L, scoring, weighting; then per node 1 .. nb_nodes-1:
    // parent (int32), descriptor (32 bytes), weight (float), is_leaf (1 byte)   (TemplatedVocabulary.h:1478-1546)
    bool loadFromBinaryFile(const std::string& filename) {
        clear();
        std::FILE* f = std::fopen(filename.c_str(), "rb");
        if (!f) return false;
        uint32_t nb_nodes = 0, size_node = 0;
        int32_t k_ = 0, L_ = 0, scoring_ = 0, weighting_ = 0;
        bool ok = std::fread(&nb_nodes, 4, 1, f) == 1 && std::fread(&size_node, 4, 1, f) == 1 && std::fread(&k_, 4, 1, f) == 1 &&
                  std::fread(&L_, 4, 1, f) == 1 && std::fread(&scoring_, 4, 1, f) == 1 && std::fread(&weighting_, 4, 1, f) == 1;
        ok = ok && size_node == kNodeBytes && headerOk(nb_nodes, k_, L_, scoring_, weighting_);
        if (!ok) { std::fclose(f); return false; }
        std::vector<uint8_t> rec((size_t)size_node * (nb_nodes - 1));
        const size_t got = rec.empty() ? 0 : std::fread(rec.data(), size_node, nb_nodes - 1, f);
        std::fclose(f);
        if (got != nb_nodes - 1) return false;
        const uint32_t N = nb_nodes;
        std::vector<int32_t> p(N, 0);
        std::vector<uint8_t> d((size_t)N * kDescBytes, 0), lf(N, 0);
        std::vector<double> w(N, 0.0);
        for (uint32_t id = 1; id < N; ++id) {
            const uint8_t* r = rec.data() + (size_t)(id - 1) * size_node;
            float wf;
            std::memcpy(&p[id], r, 4);
            std::memcpy(&d[(size_t)id * kDescBytes], r + 4, kDescBytes);
            std::memcpy(&wf, r + 4 + kDescBytes, 4);
            w[id] = (double)wf;
            lf[id] = r[4 + kDescBytes + 4];
        }
        return assign(k_, L_, scoring_, weighting_, N, p.data(), d.data(), w.data(), lf.data());
    }

    // the file TemplatedVocabulary::saveToBinaryFile (:1526-1546) writes, from per-node arrays (root at index 0, not written);
    // the one place that writes the format: this struct and ORBVocabulary::saveToBinaryFile both come here
    static bool writeBinaryFile(const std::string& filename, int k_, int L_, int scoring_, int weighting_, uint32_t nb_nodes,
                                const int32_t* parent_, const uint8_t* desc_, const double* weight_, const uint8_t* leaf_) {
        if (nb_nodes < 1) return false;
        std::FILE* f = std::fopen(filename.c_str(), "wb");
        if (!f) return false;
        const uint32_t size_node = kNodeBytes;
        const int32_t hdr[4] = {k_, L_, scoring_, weighting_};
        bool ok = std::fwrite(&nb_nodes, 4, 1, f) == 1 && std::fwrite(&size_node, 4, 1, f) == 1 && std::fwrite(hdr, 4, 4, f) == 4;
        for (uint32_t id = 1; id < nb_nodes && ok; ++id) {
            const float w = (float)weight_[id];
            ok = std::fwrite(&parent_[id], 4, 1, f) == 1 && std::fwrite(desc_ + (size_t)id * kDescBytes, 1, kDescBytes, f) == (size_t)kDescBytes &&
                 std::fwrite(&w, 4, 1, f) == 1 && std::fwrite(&leaf_[id], 1, 1, f) == 1;
        }
        return (std::fclose(f) == 0) && ok;
    }
    bool saveToBinaryFile(const std::string& filename) const {
        return writeBinaryFile(filename, k, L, scoring, weighting, (uint32_t)parent.size(), parent.data(), desc.data(), weight.data(), leaf.data());
    }
};

}  // namespace se2lam_amd
