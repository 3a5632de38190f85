// Training a DBoW2 vocabulary: hierarchical k-means++ over 256-bit descriptors (TemplatedVocabulary::create,
// Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:573-1020; FORB::meanValue / FORB::distance, FORB.cpp:29-102).  The
// specification, stated once, and the inline functions that the host mirror (ORBVocabulary::create) and the device path
// (csrc/voc_train.hip, se2gpu_voc_train) share.  Plain C++, usable from host code and from a .hip file.
//
// Input       ndocs documents (images), document d holding count[d] descriptors of 32 bytes; the feature list is the
//             documents concatenated in order.  Features are values: nothing ever modifies them ("Vocabulary
//             training", deviation 1: the reference writes cluster means into its own training features).
// Parameters  k, L, scoring, weighting, a 64-bit seed, max_iters (0 = 1000).  Refused: k outside 2..32, L outside 1..10, a
//             scoring / weighting that VocabularyTree::headerOk refuses, no descriptor at all, a document with more than
//             4096 descriptors.
//
// HKmeansStep(node, members in ascending feature index, level)                                        (:657-835)
//   n <= k     one cluster per member, in order; no draws ("trivial node")
//   otherwise  seeding, then the Lloyd loop
//   children are created for the clusters in index order; a child recurses when it has more than one member and level < L.
// Seeding (k-means++, :849-937)
//   first seed: member floor(u * n); the minimal distances start as the distances to it.  Then, until k seeds: update the
//   minimal distances with the newest seed (only where the minimum is still > 0) and sum them; a sum of 0 ends the seeding
//   with fewer than k clusters; cut_d = u * (double)sum, redrawn while it equals 0.0; the new seed is the first member whose
//   inclusive running sum is >= cut_d (the last member if none).
// Lloyd loop (:696-797)
//   iteration 1 assigns every member to the FIRST nearest centre (d < best_d).  Every further iteration first replaces each
//   centre by the mean of its members in the previous assignment and assigns again; the loop stops when the assignment
//   equals the previous one.  The mean is the bit majority: bit b is set when it is set in at least N/2 + N%2 of the N
//   members (the mean of one member is that member).
// Where the reference has no definition (deviation 2: it dereferences a released centre when a cluster loses its members)
//   a cluster without members keeps its previous centre during the loop;
//   a cluster that ends without members creates no node (stat empty_clusters);
//   a node whose number of assignments reaches max_iters without the loop having stopped keeps the assignment and the centres
//   it has (stat capped_nodes).
// Draws (deviation 3: DBoW2's single rand() stream, consumed depth first, cannot be reproduced level by level)
//   key(root) = splitmix64(seed); key(child c) = splitmix64(key(parent) ^ (c + 1)), c the cluster index before empty clusters
//   are dropped; the j-th draw of a node is u = (splitmix64(key + j) >> 11) * 2^-53.  Integer work, one exact conversion and
//   one IEEE multiply: identical on host and device (the .hip is compiled with -ffp-contract=off).
// Node ids     depth first as DBoW2 numbers them: the children of a node get consecutive ids, then the subtree of each child
//              in turn.  Word ids go to the childless nodes in ascending node id.
// Weights (:967-1020)
//   TF, BINARY: 1 for every word.  IDF, TF_IDF: every training descriptor walks the finished tree (first minimum); Ni = the
//   number of documents with at least one feature on the word; weight = log((double)ndocs / (double)Ni) computed on the host,
//   rounded to float as the file format does, 0 when Ni == 0.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SE2_VT_HD __host__ __device__
#else
#define SE2_VT_HD
#endif

namespace se2lam_amd {

// the layout of se2gpu_voc_train_stats (se2gpu.h)
struct TrainStats {
    int32_t nodes = 0;                // incl. the root
    int32_t words = 0;
    int32_t kmeans_nodes = 0;         // nodes split by seeding + Lloyd
    int32_t trivial_nodes = 0;        // nodes with n <= k
    int32_t lloyd_iters_total = 0;    // assignments, summed over the k-means nodes
    int32_t lloyd_iters_max = 0;
    int32_t short_seeded_nodes = 0;   // seeding ended on a zero sum
    int32_t empty_clusters = 0;
    int32_t capped_nodes = 0;
    int32_t zero_weight_words = 0;
};

namespace voctrain {

const int kMaxK = 32, kMaxL = 10, kMaxDocFeatures = 4096, kDefaultMaxIters = 1000;

inline bool paramsOk(int k, int L, int scoring, int weighting) {
    return k >= 2 && k <= kMaxK && L >= 1 && L <= kMaxL && scoring >= 0 && scoring <= 5 && weighting >= 0 && weighting <= 3;
}

SE2_VT_HD inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
SE2_VT_HD inline uint64_t rootKey(uint64_t seed) { return splitmix64(seed); }
SE2_VT_HD inline uint64_t childKey(uint64_t parent_key, int c) { return splitmix64(parent_key ^ (uint64_t)(c + 1)); }
// the j-th draw of the node with this key, in [0, 1)
SE2_VT_HD inline double draw(uint64_t key, uint32_t j) { return (double)(splitmix64(key + j) >> 11) * 0x1.0p-53; }
// a bit of the mean is set when at least this many of the n members have it
SE2_VT_HD inline int majorityThreshold(int n) { return n / 2 + n % 2; }

// the weight of a word that ni of the ndocs documents contain, as the file stores it
inline float idfWeight(int ndocs, int ni) { return ni > 0 ? (float)std::log((double)ndocs / (double)ni) : 0.0f; }

}  // namespace voctrain
}  // namespace se2lam_amd
