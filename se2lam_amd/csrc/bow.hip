// DBoW2 vocabulary on the device: transform(features, BowVector, FeatureVector, levelsup) for batches of frames whose
// descriptors already lie in HBM, and loop-candidate scoring against the BowVectors of every key frame.
//   TemplatedVocabulary::transform   Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1150-1216, 1241-1280
//   BowVector::normalize             Thirdparty/DBoW2/DBoW2/BowVector.cpp:62-84
//   *Scoring::score                  Thirdparty/DBoW2/DBoW2/ScoringObject.cpp
//   DetectLoopClose (best candidate) src/GlobalMapper.cpp:201-254, src/Localizer.cpp:337-391
// Every result equals the host mirror include/se2lam_amd/ORBVocabulary.h bit for bit ("Device vocabulary"):
// the walk is integer arithmetic with the first-minimum rule, a word's value is count * weight (exact: the weight is a float
// widened to double), and every floating-point sum - the norm of a BowVector, the common-word terms of a score - is added
// in ascending word id, the order of the mirror's loops.  Compiled with -ffp-contract=off (build.py).
#include <algorithm>
#include <memory>
#include <new>

#include "../../include/se2lam_amd/VocabularyTree.h"
#include "common.h"
#include "wave_int.h"

using namespace se2gpu;

namespace {

constexpr int kMaxFeat = 4096;      // features per frame the per-frame assembly sorts in LDS
constexpr int kAsmThreads = 1024;
constexpr uint32_t kNoWord = 0xffffffffu;
constexpr int kTagBits = 12;        // query position inside a dense-array tag (kMaxFeat = 1 << kTagBits)
static_assert(kMaxFeat == 1 << kTagBits, "tag layout");

enum { W_TF_IDF = 0, W_TF = 1, W_IDF = 2, W_BINARY = 3 };
enum { S_L1 = 0, S_L2 = 1, S_CHI = 2, S_KL = 3, S_BHAT = 4, S_DOT = 5 };

// ---------------------------------------------------------------------------------------------------------------------
// Tree walk.  Node descriptors are stored in "child slot" order: slot j holds the node children()[j] of the mirror, so the
// children of one node are contiguous (320 bytes for k = 10).  meta[slot] = {first child slot, number of children, node id
// in the file, word id or -1 (no leaf, or a stopped word)}.  A group of G lanes walks one descriptor, one lane per child;
// the minimum over (distance << 32 | child index) is the FIRST child at the minimal distance.
// ---------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ void __launch_bounds__(256) k_bow_walk(const uint4* __restrict__ tree_desc, const int4* __restrict__ meta, int root_children,
                                                  int nid_level, const uint8_t* __restrict__ desc, const int32_t* __restrict__ counts,
                                                  int cap, int nframes, uint32_t* __restrict__ word_out, int32_t* __restrict__ node_out) {
    const long long gid = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    const int f = (int)(gid / cap), i = (int)(gid % cap);
    if (f >= nframes) return;
    const int cnt = min(max(counts[f], 0), cap);
    if (i >= cnt) return;   // slots beyond the frame's count are never read
    const uint4* dp = reinterpret_cast<const uint4*>(desc + ((size_t)f * cap + i) * 32);
    const uint4 a0 = dp[0], a1 = dp[1];
    int cb = 0, cn = root_children, level = 0, nid = nid_level <= 0 ? 0 : -1;
    int4 m = make_int4(0, 0, 0, -1);
    do {
        ++level;
        unsigned long long best = ~0ull;
        for (int c = lane; c < cn; c += G) {
            const uint4 b0 = tree_desc[2 * (size_t)(cb + c)], b1 = tree_desc[2 * (size_t)(cb + c) + 1];
            const int d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                          __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
            const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)c;
            best = key < best ? key : best;
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, G);
            best = o < best ? o : best;
        }
        m = meta[cb + (int)(unsigned)best];
        if (level == nid_level) nid = m.z;
        cb = m.x; cn = m.y;
    } while (cn > 0);   // Node::isLeaf() = children.empty()
    if (lane == 0) {
        word_out[(size_t)f * cap + i] = (uint32_t)m.w;        // kNoWord for a stopped word
        node_out[(size_t)f * cap + i] = nid < 0 ? m.z : nid;  // a leaf above level L - levelsup is recorded itself
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-frame assembly: one workgroup per frame.
// ---------------------------------------------------------------------------------------------------------------------
__device__ void bitonic_sort(unsigned long long* keys, int n_pad) {
    for (int k = 2; k <= n_pad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n_pad; t += blockDim.x) {
                const int p = t ^ j;
                if (p > t) {
                    const unsigned long long a = keys[t], b = keys[p];
                    if ((a > b) == ((t & k) == 0)) { keys[t] = b; keys[p] = a; }
                }
            }
            __syncthreads();
        }
}

// keys (sorted, the invalid ones ~0 at the end) -> start[r] = first position of run r of equal high words, start[runs] = number
// of valid keys; returns the number of runs.  Every thread looks at the 4 consecutive positions it owns.
__device__ int run_starts(const unsigned long long* keys, int n_pad, int* start, int* wave_sums) {
    constexpr int kPer = kMaxFeat / kAsmThreads;
    const int j0 = threadIdx.x * kPer;
    int heads = 0, valid = 0;
    bool is_head[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = j0 + q;
        is_head[q] = false;
        if (j < n_pad && keys[j] != ~0ull) {
            ++valid;
            is_head[q] = j == 0 || (uint32_t)(keys[j - 1] >> 32) != (uint32_t)(keys[j] >> 32);
            heads += is_head[q];
        }
    }
    // block-wide exclusive scan of (heads, valid) packed into one int: both are below 1 << 13
    const int v = (heads << 16) | valid;
    const int inc = wave_scan_incl(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 63) wave_sums[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int x = 0; x < kAsmThreads / 64; ++x) { const int t = wave_sums[x]; wave_sums[x] = s; s += t; }
        wave_sums[kAsmThreads / 64] = s;
    }
    __syncthreads();
    const int total = wave_sums[kAsmThreads / 64];
    int pos = (wave_sums[w] + inc - v) >> 16;
#pragma unroll
    for (int q = 0; q < kPer; ++q)
        if (is_head[q]) start[pos++] = j0 + q;
    if (threadIdx.x == 0) start[total >> 16] = total & 0xffff;
    __syncthreads();
    return total >> 16;
}

__global__ void __launch_bounds__(kAsmThreads) k_bow_assemble(const uint32_t* __restrict__ word_in, const int32_t* __restrict__ node_in,
                                                              const int32_t* __restrict__ counts, int cap, const double* __restrict__ word_weight,
                                                              int scoring, int weighting, uint32_t* __restrict__ bow_word,
                                                              double* __restrict__ bow_value, int32_t* __restrict__ bow_n,
                                                              int32_t* __restrict__ fv_nodes, int32_t* __restrict__ fv_ptr,
                                                              int32_t* __restrict__ fv_idx, int32_t* __restrict__ fv_nn) {
    __shared__ unsigned long long keys[kMaxFeat];
    __shared__ double vals[kMaxFeat];
    __shared__ int start[kMaxFeat + 1];
    __shared__ int wave_sums[kAsmThreads / 64 + 1];
    __shared__ double divisor;
    const int f = blockIdx.x;
    const int cnt = min(max(counts[f], 0), cap);
    word_in += (size_t)f * cap; node_in += (size_t)f * cap;
    bow_word += (size_t)f * cap; bow_value += (size_t)f * cap;
    fv_nodes += (size_t)f * cap; fv_ptr += (size_t)f * (cap + 1); fv_idx += (size_t)f * cap;
    int n_pad = 1;
    while (n_pad < cnt) n_pad <<= 1;

    // ---- BowVector: (word, feature) sorted, one run per word
    for (int i = threadIdx.x; i < n_pad; i += blockDim.x) {
        const uint32_t w = i < cnt ? word_in[i] : kNoWord;
        keys[i] = w == kNoWord ? ~0ull : ((unsigned long long)w << 32) | (unsigned)i;
    }
    __syncthreads();
    bitonic_sort(keys, n_pad);
    const int nw = run_starts(keys, n_pad, start, wave_sums);
    const bool once = weighting == W_IDF || weighting == W_BINARY;   // addIfNotExist instead of addWeight
    for (int p = threadIdx.x; p < nw; p += blockDim.x) {
        const uint32_t w = (uint32_t)(keys[start[p]] >> 32);
        const double wt = word_weight[w];
        vals[p] = once ? wt : (double)(start[p + 1] - start[p]) * wt;   // = the mirror's sum of `count` equal weights, exactly
        bow_word[p] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // the ordered sum of BowVector::normalize: ascending word id, one lane
        double d = 0.0;
        if (scoring == S_DOT) {
            if (!once && nw > 0) d = (double)nw;
        } else {
            double norm = 0.0;
            if (scoring == S_L2) {
                for (int p = 0; p < nw; ++p) norm += vals[p] * vals[p];
                norm = sqrt(norm);
            } else {
                for (int p = 0; p < nw; ++p) norm += fabs(vals[p]);
            }
            if (norm > 0.0) d = norm;
        }
        divisor = d;
        bow_n[f] = nw;
    }
    __syncthreads();
    {
        const double d = divisor;
        for (int p = threadIdx.x; p < nw; p += blockDim.x) bow_value[p] = d != 0.0 ? vals[p] / d : vals[p];
    }
    __syncthreads();

    // ---- FeatureVector: (node, feature) sorted, one run per node; a stopped feature is in neither vector
    for (int i = threadIdx.x; i < n_pad; i += blockDim.x) {
        const bool ok = i < cnt && word_in[i] != kNoWord;
        keys[i] = ok ? ((unsigned long long)(uint32_t)node_in[i] << 32) | (unsigned)i : ~0ull;
    }
    __syncthreads();
    bitonic_sort(keys, n_pad);
    const int nn = run_starts(keys, n_pad, start, wave_sums);
    const int nvalid = start[nn];
    for (int p = threadIdx.x; p < nn; p += blockDim.x) {
        fv_nodes[p] = (int32_t)(keys[start[p]] >> 32);
        fv_ptr[p] = start[p];
    }
    for (int j = threadIdx.x; j < nvalid; j += blockDim.x) fv_idx[j] = (int32_t)(uint32_t)keys[j];
    if (threadIdx.x == 0) { fv_ptr[nn] = nvalid; fv_nn[f] = nn; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Scoring.  The query is scattered into a dense per-word array of tags (epoch << 12 | position in the query; a stale epoch
// means "absent", so the array is never cleared between queries).  One wave per data-base entry walks the entry's words
// 64 at a time; the lanes whose word the query holds compute their term, and the terms are added lane by lane in ascending
// lane order = ascending word id, the order of the mirror's merge loop.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_bow_query_scatter(const uint32_t* __restrict__ q_word, int n, uint32_t words, uint32_t epoch, uint32_t* __restrict__ tag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && q_word[i] < words) tag[q_word[i]] = (epoch << kTagBits) | (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_bow_score(const uint32_t* __restrict__ tag, uint32_t epoch, uint32_t words, const double* __restrict__ q_value,
                                                   int scoring, const int32_t* __restrict__ order, int size, const long long* __restrict__ e_off,
                                                   const int32_t* __restrict__ e_n, const uint32_t* __restrict__ db_word,
                                                   const double* __restrict__ db_value, double* __restrict__ scores) {
    const int pos = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (pos >= size) return;
    const int slot = order[pos];
    const long long off = e_off[slot];
    const int n = e_n[slot];
    double s = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        double term = 0.0;
        bool hit = false;
        if (j < n) {
            const uint32_t w = db_word[off + j];
            const uint32_t t = w < words ? tag[w] : 0u;
            if ((t >> kTagBits) == epoch) {
                const double vi = q_value[t & ((1u << kTagBits) - 1)], wi = db_value[off + j];
                hit = true;
                switch (scoring) {
                    case S_L1: term = fabs(vi - wi) - fabs(vi) - fabs(wi); break;
                    case S_L2: case S_DOT: term = vi * wi; break;
                    case S_CHI: hit = vi + wi != 0.0; if (hit) term = vi * wi / (vi + wi); break;
                    case S_BHAT: term = sqrt(vi * wi); break;
                    default: hit = false; break;
                }
            }
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {   // wave-uniform
            const int l = __ffsll((long long)mask) - 1;
            s += __shfl(term, l, 64);
            mask &= mask - 1;
        }
    }
    if (lane == 0) {
        double r = s;
        switch (scoring) {
            case S_L1: r = -s / 2.0; break;
            case S_L2: r = s >= 1.0 ? 1.0 : 1.0 - sqrt(1.0 - s); break;
            case S_CHI: r = 2.0 * s; break;
            default: break;
        }
        scores[pos] = r;
    }
}

struct BowBest {
    double score;
    int32_t entry, kf_id;
};

// DetectLoopClose's choice: of the entries far enough from the current key frame, the first in insertion order whose score
// exceeds every earlier one's and 0 = the lowest position holding the maximal score, if that is above 0.
__global__ void __launch_bounds__(1024) k_bow_best(const double* __restrict__ scores, const int32_t* __restrict__ order, const int32_t* __restrict__ e_kf,
                                                   int size, int cur_kf, int min_off, BowBest* __restrict__ out) {
    __shared__ double s_score[1024];
    __shared__ int s_pos[1024];
    double best = 0.0;
    int bpos = -1;
    for (int p = threadIdx.x; p < size; p += blockDim.x) {
        const long long d = (long long)e_kf[order[p]] - cur_kf;
        if ((d < 0 ? -d : d) < min_off) continue;
        if (scores[p] > best) { best = scores[p]; bpos = p; }   // positions ascend within a thread: strict > keeps the first
    }
    s_score[threadIdx.x] = best; s_pos[threadIdx.x] = bpos;
    __syncthreads();
    for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const double o = s_score[threadIdx.x + h];
            const int op = s_pos[threadIdx.x + h];
            const double m = s_score[threadIdx.x];
            const int mp = s_pos[threadIdx.x];
            if (op >= 0 && (mp < 0 || o > m || (o == m && op < mp))) { s_score[threadIdx.x] = o; s_pos[threadIdx.x] = op; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->score = s_pos[0] >= 0 ? s_score[0] : 0.0;
        out->entry = s_pos[0];
        out->kf_id = s_pos[0] >= 0 ? e_kf[order[s_pos[0]]] : -1;
    }
}

// one data-base entry filled from device memory: the count stays on the device
__global__ void k_bow_db_put(const uint32_t* __restrict__ src_word, const double* __restrict__ src_value, const int32_t* __restrict__ src_n, int cap,
                             uint32_t* __restrict__ dst_word, double* __restrict__ dst_value, int32_t* __restrict__ dst_n,
                             long long* __restrict__ dst_off, int32_t* __restrict__ dst_kf, long long off, int kf_id) {
    const int n = min(max(*src_n, 0), cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        dst_word[i] = src_word[i];
        dst_value[i] = src_value[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { *dst_n = n; *dst_off = off; *dst_kf = kf_id; }
}

}  // namespace

// =====================================================================================================================
// handles
// =====================================================================================================================
struct se2gpu_voc {
    int k = 0, L = 0, scoring = 0, weighting = 0, nodes = 0, words = 0, root_children = 0, max_children = 0, device = 0;
    DevBuf<uint4> desc;      // 2 per child slot
    DevBuf<int4> meta;       // per child slot
    DevBuf<double> word_weight;
    se2lam_amd::VocabularyTree tree;   // the records on the host: se2gpu_voc_export, se2gpu_voc_save
};

struct se2gpu_bow {
    const se2gpu_voc* voc = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    int max_features = 0, max_batch = 1;
    DevBuf<uint32_t> walk_word;
    DevBuf<int32_t> walk_node;
    // single-frame form: one frame's inputs and outputs
    DevBuf<uint8_t> s_desc;
    DevBuf<int32_t> s_i32;     // count | bow_n | fv_nn | fv_nodes[F] | fv_ptr[F + 1] | fv_idx[F]
    DevBuf<uint32_t> s_word;
    DevBuf<double> s_value;
    // query side
    DevBuf<uint32_t> tag, q_word;
    DevBuf<double> q_value, scores;
    DevBuf<BowBest> best;
    uint32_t epoch = 0;
    ~se2gpu_bow() {
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

struct se2gpu_bowdb {
    const se2gpu_voc* voc = nullptr;
    // a slot is a fixed region of the word / value arrays; `order` lists the live slots in insertion order
    struct Slot { long long off; int cap; int kf_id; };
    std::vector<Slot> slots;
    std::vector<int32_t> order, free_slots;
    long long used = 0, data_cap = 0;
    size_t table_cap = 0;
    uint32_t* d_word = nullptr;
    double* d_value = nullptr;
    long long* d_off = nullptr;
    int32_t *d_n = nullptr, *d_kf = nullptr, *d_order = nullptr;
    bool order_dirty = true;
    hipStream_t last_stream = nullptr;   // the stream the last asynchronous operation on the arrays went to
    bool pending = false;
    ~se2gpu_bowdb() {
        for (void* p : {(void*)d_word, (void*)d_value, (void*)d_off, (void*)d_n, (void*)d_kf, (void*)d_order})
            if (p) (void)hipFree(p);
    }
};

namespace {

int voc_upload(se2lam_amd::VocabularyTree& t, se2gpu_voc** out) {
    std::unique_ptr<se2gpu_voc> v(new (std::nothrow) se2gpu_voc);
    SE2_REQUIRE(v, SE2GPU_ERR_INVALID, "voc: out of memory");
    v->k = t.k; v->L = t.L; v->scoring = t.scoring; v->weighting = t.weighting;
    v->nodes = (int)t.parent.size(); v->words = (int)t.words.size();
    SE2_HIP(hipGetDevice(&v->device));
    const size_t nslots = t.child.size();
    std::vector<uint4> desc(2 * nslots);
    std::vector<int4> meta(nslots);
    for (size_t s = 0; s < nslots; ++s) {
        const int32_t id = t.child[s];
        std::memcpy(&desc[2 * s], &t.desc[(size_t)id * 32], 32);
        const int cn = t.child_ptr[id + 1] - t.child_ptr[id];
        const bool stopped = !(t.weight[id] > 0);
        meta[s] = make_int4(t.child_ptr[id], cn, id, (t.word[id] >= 0 && !stopped) ? t.word[id] : -1);
        v->max_children = std::max(v->max_children, cn);
    }
    v->root_children = v->nodes > 0 ? t.child_ptr[1] - t.child_ptr[0] : 0;
    v->max_children = std::max(v->max_children, v->root_children);
    std::vector<double> ww(t.words.size());
    for (size_t w = 0; w < ww.size(); ++w) ww[w] = t.weight[t.words[w]];
    SE2_CHECK(v->desc.reserve(std::max<size_t>(desc.size(), 2)));
    SE2_CHECK(v->meta.reserve(std::max<size_t>(meta.size(), 1)));
    SE2_CHECK(v->word_weight.reserve(std::max<size_t>(ww.size(), 1)));
    if (nslots) {
        SE2_HIP(hipMemcpy(v->desc.p, desc.data(), desc.size() * sizeof(uint4), hipMemcpyHostToDevice));
        SE2_HIP(hipMemcpy(v->meta.p, meta.data(), meta.size() * sizeof(int4), hipMemcpyHostToDevice));
    }
    if (!ww.empty()) SE2_HIP(hipMemcpy(v->word_weight.p, ww.data(), ww.size() * sizeof(double), hipMemcpyHostToDevice));
    v->tree = std::move(t);
    *out = v.release();
    return SE2GPU_OK;
}

// the arrays of `db` are about to be touched on `s`: whatever another stream still does to them has to finish first
int db_enter(se2gpu_bowdb* db, hipStream_t s) {
    if (db->pending && db->last_stream != s) SE2_HIP(hipStreamSynchronize(db->last_stream));
    db->last_stream = s;
    db->pending = true;
    return SE2GPU_OK;
}

int db_quiesce(se2gpu_bowdb* db) {
    if (db->pending) SE2_HIP(hipStreamSynchronize(db->last_stream));
    db->pending = false;
    return SE2GPU_OK;
}

template <typename T>
int grow(T** p, size_t old_n, size_t new_n) {
    T* q = nullptr;
    SE2_HIP(hipMalloc((void**)&q, new_n * sizeof(T)));
    if (*p) {
        if (old_n) SE2_HIP(hipMemcpy(q, *p, old_n * sizeof(T), hipMemcpyDeviceToDevice));
        (void)hipFree(*p);
    }
    *p = q;
    return SE2GPU_OK;
}

// a slot with room for `cap` words, appended to the order; the device is idle on the arrays when they have to move
int db_new_slot(se2gpu_bowdb* db, int kf_id, int cap, int* slot_out) {
    cap = std::max(cap, 1);
    int slot = -1;
    for (size_t i = 0; i < db->free_slots.size(); ++i)
        if (db->slots[db->free_slots[i]].cap >= cap) {
            slot = db->free_slots[i];
            db->free_slots.erase(db->free_slots.begin() + (ptrdiff_t)i);
            break;
        }
    if (slot < 0) {
        if (db->used + cap > db->data_cap) {
            SE2_CHECK(db_quiesce(db));
            const long long want = std::max<long long>(2 * db->data_cap, std::max<long long>(db->used + cap, 1 << 16));
            SE2_CHECK(grow(&db->d_word, (size_t)db->used, (size_t)want));
            SE2_CHECK(grow(&db->d_value, (size_t)db->used, (size_t)want));
            db->data_cap = want;
        }
        if (db->slots.size() + 1 > db->table_cap) {
            SE2_CHECK(db_quiesce(db));
            const size_t want = std::max<size_t>(2 * db->table_cap, 1024);
            SE2_CHECK(grow(&db->d_off, db->slots.size(), want));
            SE2_CHECK(grow(&db->d_n, db->slots.size(), want));
            SE2_CHECK(grow(&db->d_kf, db->slots.size(), want));
            if (db->d_order) (void)hipFree(db->d_order);
            db->d_order = nullptr;
            SE2_HIP(hipMalloc((void**)&db->d_order, want * sizeof(int32_t)));
            db->table_cap = want;
        }
        slot = (int)db->slots.size();
        db->slots.push_back({db->used, cap, kf_id});
        db->used += cap;
    }
    db->slots[slot].kf_id = kf_id;
    db->order.push_back(slot);
    db->order_dirty = true;
    *slot_out = slot;
    return SE2GPU_OK;
}

template <int G>
void launch_walk(const se2gpu_bow* h, int nid_level, const uint8_t* d_desc, const int32_t* d_counts, int cap, int nframes) {
    const se2gpu_voc* v = h->voc;
    const long long threads = (long long)nframes * cap * G;
    hipLaunchKernelGGL(k_bow_walk<G>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, v->desc.p, v->meta.p, v->root_children,
                       nid_level, d_desc, d_counts, cap, nframes, h->walk_word.p, h->walk_node.p);
}

int transform_launch(se2gpu_bow* h, const uint8_t* d_desc, const int32_t* d_counts, int cap, int nframes, int levelsup, uint32_t* d_bow_word,
                     double* d_bow_value, int32_t* d_bow_n, int32_t* d_fv_nodes, int32_t* d_fv_ptr, int32_t* d_fv_idx, int32_t* d_fv_nn) {
    const se2gpu_voc* v = h->voc;
    if (v->words == 0) {   // an empty vocabulary transforms everything into empty vectors (ORBVocabulary::transform: `if (empty()) return`)
        SE2_HIP(hipMemsetAsync(d_bow_n, 0, sizeof(int32_t) * nframes, h->stream));
        SE2_HIP(hipMemsetAsync(d_fv_nn, 0, sizeof(int32_t) * nframes, h->stream));
        SE2_HIP(hipMemsetAsync(d_fv_ptr, 0, sizeof(int32_t) * (size_t)nframes * (cap + 1), h->stream));
        return SE2GPU_OK;
    }
    const int nid_level = v->L - levelsup;
    const int g = v->max_children;
    if (g <= 4) launch_walk<4>(h, nid_level, d_desc, d_counts, cap, nframes);
    else if (g <= 8) launch_walk<8>(h, nid_level, d_desc, d_counts, cap, nframes);
    else if (g <= 16) launch_walk<16>(h, nid_level, d_desc, d_counts, cap, nframes);
    else if (g <= 32) launch_walk<32>(h, nid_level, d_desc, d_counts, cap, nframes);
    else launch_walk<64>(h, nid_level, d_desc, d_counts, cap, nframes);
    hipLaunchKernelGGL(k_bow_assemble, dim3(nframes), dim3(kAsmThreads), 0, h->stream, h->walk_word.p, h->walk_node.p, d_counts, cap,
                       v->word_weight.p, v->scoring, v->weighting, d_bow_word, d_bow_value, d_bow_n, d_fv_nodes, d_fv_ptr, d_fv_idx, d_fv_nn);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // namespace

extern "C" {

// ---- se2gpu_voc ------------------------------------------------------------------------------------------------------
int se2gpu_voc_create(int k, int L, int scoring, int weighting, int nodes, const int32_t* parent, const uint8_t* desc, const double* weight,
                      const uint8_t* leaf, se2gpu_voc** out) {
    SE2_REQUIRE(out, SE2GPU_ERR_INVALID, "voc_create: out is NULL");
    *out = nullptr;
    SE2_REQUIRE(have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)");
    se2lam_amd::VocabularyTree t;
    SE2_REQUIRE(nodes >= 1 && t.assign(k, L, scoring, weighting, (uint32_t)nodes, parent, desc, weight, leaf), SE2GPU_ERR_INVALID,
                "voc_create: the records are not a vocabulary (header out of range, a parent that does not precede its child, or a "
                "childless node that is not a leaf)");
    return voc_upload(t, out);
}

int se2gpu_voc_load(const char* path, se2gpu_voc** out) {
    SE2_REQUIRE(out && path, SE2GPU_ERR_INVALID, "voc_load: NULL argument");
    *out = nullptr;
    SE2_REQUIRE(have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)");
    se2lam_amd::VocabularyTree t;
    SE2_REQUIRE(t.loadFromBinaryFile(path), SE2GPU_ERR_INVALID, "voc_load: %s is not a vocabulary file (missing, truncated, bad header or bad tree)", path);
    return voc_upload(t, out);
}

void se2gpu_voc_destroy(se2gpu_voc* v) { delete v; }
int se2gpu_voc_words(const se2gpu_voc* v) { return v ? v->words : SE2GPU_ERR_INVALID; }
int se2gpu_voc_nodes(const se2gpu_voc* v) { return v ? v->nodes : SE2GPU_ERR_INVALID; }
int se2gpu_voc_k(const se2gpu_voc* v) { return v ? v->k : SE2GPU_ERR_INVALID; }
int se2gpu_voc_L(const se2gpu_voc* v) { return v ? v->L : SE2GPU_ERR_INVALID; }
int se2gpu_voc_scoring(const se2gpu_voc* v) { return v ? v->scoring : SE2GPU_ERR_INVALID; }
int se2gpu_voc_weighting(const se2gpu_voc* v) { return v ? v->weighting : SE2GPU_ERR_INVALID; }

int se2gpu_voc_export(const se2gpu_voc* v, int cap_nodes, int32_t* parent, uint8_t* desc, double* weight, uint8_t* leaf) {
    SE2_REQUIRE(v && parent && desc && weight && leaf, SE2GPU_ERR_INVALID, "voc_export: NULL argument");
    SE2_REQUIRE(cap_nodes >= v->nodes, SE2GPU_ERR_CAPACITY, "voc_export: the vocabulary has %d nodes, the buffers hold %d", v->nodes, cap_nodes);
    const se2lam_amd::VocabularyTree& t = v->tree;
    std::copy(t.parent.begin(), t.parent.end(), parent);
    std::copy(t.desc.begin(), t.desc.end(), desc);
    std::copy(t.weight.begin(), t.weight.end(), weight);
    std::copy(t.leaf.begin(), t.leaf.end(), leaf);
    return SE2GPU_OK;
}

int se2gpu_voc_save(const se2gpu_voc* v, const char* path) {
    SE2_REQUIRE(v && path, SE2GPU_ERR_INVALID, "voc_save: NULL argument");
    SE2_REQUIRE(v->tree.saveToBinaryFile(path), SE2GPU_ERR_INVALID, "voc_save: %s cannot be written", path);
    return SE2GPU_OK;
}

// ---- se2gpu_bow ------------------------------------------------------------------------------------------------------
int se2gpu_bow_create(const se2gpu_voc* voc, int max_features, int max_batch, se2gpu_bow** out) {
    SE2_REQUIRE(out, SE2GPU_ERR_INVALID, "bow_create: out is NULL");
    *out = nullptr;
    SE2_REQUIRE(have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)");
    SE2_REQUIRE(voc, SE2GPU_ERR_INVALID, "bow_create: voc is NULL");
    SE2_REQUIRE(max_features > 0 && max_features <= kMaxFeat, SE2GPU_ERR_INVALID, "max_features must be in 1..%d", kMaxFeat);
    std::unique_ptr<se2gpu_bow> h(new (std::nothrow) se2gpu_bow);
    SE2_REQUIRE(h, SE2GPU_ERR_INVALID, "bow_create: out of memory");
    h->voc = voc;
    h->max_features = max_features;
    h->max_batch = std::max(1, max_batch);
    SE2_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    const size_t F = (size_t)max_features, n = F * h->max_batch;
    SE2_CHECK(h->walk_word.reserve(n));
    SE2_CHECK(h->walk_node.reserve(n));
    SE2_CHECK(h->s_desc.reserve(F * 32));
    SE2_CHECK(h->s_i32.reserve(3 + 3 * F + 1));
    SE2_CHECK(h->s_word.reserve(F));
    SE2_CHECK(h->s_value.reserve(F));
    SE2_CHECK(h->tag.reserve(std::max(voc->words, 1)));
    SE2_HIP(hipMemsetAsync(h->tag.p, 0, sizeof(uint32_t) * std::max(voc->words, 1), h->stream));
    SE2_CHECK(h->q_word.reserve(F));
    SE2_CHECK(h->q_value.reserve(F));
    SE2_CHECK(h->best.reserve(1));
    SE2_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
    return SE2GPU_OK;
}

void se2gpu_bow_destroy(se2gpu_bow* h) {
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

void* se2gpu_bow_stream(se2gpu_bow* h) { return h ? (void*)h->stream : nullptr; }

int se2gpu_bow_set_stream(se2gpu_bow* h, void* s) {
    SE2_REQUIRE(h, SE2GPU_ERR_INVALID, "bow handle is NULL");
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return SE2GPU_OK;
}

int se2gpu_bow_sync(se2gpu_bow* h) {
    SE2_REQUIRE(h, SE2GPU_ERR_INVALID, "bow handle is NULL");
    SE2_HIP(hipStreamSynchronize(h->stream));
    return SE2GPU_OK;
}

int se2gpu_bow_transform_batch_device(se2gpu_bow* h, const uint8_t* d_desc, const int32_t* d_counts, int cap, int nframes, int levelsup,
                                      uint32_t* d_bow_word, double* d_bow_value, int32_t* d_bow_n, int32_t* d_fv_nodes, int32_t* d_fv_ptr,
                                      int32_t* d_fv_idx, int32_t* d_fv_nn) {
    SE2_REQUIRE(h && d_desc && d_counts && d_bow_word && d_bow_value && d_bow_n && d_fv_nodes && d_fv_ptr && d_fv_idx && d_fv_nn,
                SE2GPU_ERR_INVALID, "bow_transform_batch: NULL argument");
    SE2_REQUIRE(nframes >= 1 && cap >= 1, SE2GPU_ERR_INVALID, "bow_transform_batch: bad sizes");
    SE2_REQUIRE(((uintptr_t)d_desc & 15) == 0, SE2GPU_ERR_INVALID, "bow_transform_batch: d_desc must be 16-byte aligned");
    SE2_REQUIRE(cap <= h->max_features && nframes <= h->max_batch, SE2GPU_ERR_CAPACITY,
                "bow_transform_batch: %d frames of %d features exceed the handle's %d x %d", nframes, cap, h->max_batch, h->max_features);
    return transform_launch(h, d_desc, d_counts, cap, nframes, levelsup, d_bow_word, d_bow_value, d_bow_n, d_fv_nodes, d_fv_ptr, d_fv_idx,
                            d_fv_nn);
}

int se2gpu_bow_transform(se2gpu_bow* h, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word, double* bow_value, int* nb,
                         int32_t* fv_nodes, int32_t* fv_ptr, int32_t* fv_idx, int* nn) {
    SE2_REQUIRE(h && nb && nn && fv_ptr && n >= 0, SE2GPU_ERR_INVALID, "bow_transform: bad argument");
    SE2_REQUIRE(n == 0 || (desc && bow_word && bow_value && fv_nodes && fv_idx), SE2GPU_ERR_INVALID, "bow_transform: NULL buffer");
    SE2_REQUIRE(n <= h->max_features, SE2GPU_ERR_CAPACITY, "bow_transform: %d features exceed the handle's %d", n, h->max_features);
    *nb = 0; *nn = 0; fv_ptr[0] = 0;
    if (n == 0) return SE2GPU_OK;   // an empty frame gives empty vectors
    const int F = n;
    int32_t* d_cnt = h->s_i32.p;
    int32_t *d_bn = d_cnt + 1, *d_nn = d_cnt + 2, *d_fn = d_cnt + 3, *d_fp = d_fn + F, *d_fi = d_fp + F + 1;
    const int32_t cnt = n;
    SE2_HIP(hipMemcpyAsync(h->s_desc.p, desc, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
    SE2_HIP(hipMemcpyAsync(d_cnt, &cnt, sizeof cnt, hipMemcpyHostToDevice, h->stream));
    SE2_CHECK(transform_launch(h, h->s_desc.p, d_cnt, F, 1, levelsup, h->s_word.p, h->s_value.p, d_bn, d_fn, d_fp, d_fi, d_nn));
    std::vector<int32_t> host(3 + 3 * (size_t)F + 1);
    SE2_HIP(hipMemcpyAsync(host.data(), d_cnt, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    SE2_HIP(hipStreamSynchronize(h->stream));
    const int b = host[1], m = host[2];
    SE2_REQUIRE(b >= 0 && b <= n && m >= 0 && m <= n, SE2GPU_ERR_HIP, "bow_transform: the device returned impossible counts");
    if (b) {
        SE2_HIP(hipMemcpyAsync(bow_word, h->s_word.p, sizeof(uint32_t) * b, hipMemcpyDeviceToHost, h->stream));
        SE2_HIP(hipMemcpyAsync(bow_value, h->s_value.p, sizeof(double) * b, hipMemcpyDeviceToHost, h->stream));
        SE2_HIP(hipStreamSynchronize(h->stream));
    }
    const int32_t *fn = host.data() + 3, *fp = fn + F, *fi = fp + F + 1;
    std::copy(fn, fn + m, fv_nodes);
    std::copy(fp, fp + m + 1, fv_ptr);
    std::copy(fi, fi + fp[m], fv_idx);
    *nb = b; *nn = m;
    return SE2GPU_OK;
}

// ---- se2gpu_bowdb ----------------------------------------------------------------------------------------------------
int se2gpu_bowdb_create(const se2gpu_voc* voc, se2gpu_bowdb** out) {
    SE2_REQUIRE(out, SE2GPU_ERR_INVALID, "bowdb_create: out is NULL");
    *out = nullptr;
    SE2_REQUIRE(have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)");
    SE2_REQUIRE(voc, SE2GPU_ERR_INVALID, "bowdb_create: voc is NULL");
    SE2_REQUIRE(voc->scoring != S_KL, SE2GPU_ERR_INVALID,
                "bowdb_create: KL scoring is not implemented on the device (it needs the host's log() bit for bit); use the host vocabulary");
    se2gpu_bowdb* db = new (std::nothrow) se2gpu_bowdb;
    SE2_REQUIRE(db, SE2GPU_ERR_INVALID, "bowdb_create: out of memory");
    db->voc = voc;
    *out = db;
    return SE2GPU_OK;
}

void se2gpu_bowdb_destroy(se2gpu_bowdb* db) {
    if (!db) return;
    (void)db_quiesce(db);
    delete db;
}

int se2gpu_bowdb_size(const se2gpu_bowdb* db) { return db ? (int)db->order.size() : SE2GPU_ERR_INVALID; }

int se2gpu_bowdb_add(se2gpu_bowdb* db, int kf_id, const uint32_t* word, const double* value, int n) {
    SE2_REQUIRE(db && n >= 0 && (n == 0 || (word && value)), SE2GPU_ERR_INVALID, "bowdb_add: bad argument");
    for (int i = 0; i < n; ++i)
        SE2_REQUIRE((i == 0 || word[i - 1] < word[i]) && word[i] < (uint32_t)db->voc->words, SE2GPU_ERR_INVALID,
                    "bowdb_add: word ids must ascend and lie below the vocabulary's %d words", db->voc->words);
    int slot = -1;
    SE2_CHECK(db_new_slot(db, kf_id, n, &slot));
    SE2_CHECK(db_quiesce(db));   // synchronous: the host buffers are the caller's again on return
    const se2gpu_bowdb::Slot& s = db->slots[slot];
    const int32_t n32 = n;
    if (n) {
        SE2_HIP(hipMemcpy(db->d_word + s.off, word, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        SE2_HIP(hipMemcpy(db->d_value + s.off, value, sizeof(double) * n, hipMemcpyHostToDevice));
    }
    SE2_HIP(hipMemcpy(db->d_off + slot, &s.off, sizeof(long long), hipMemcpyHostToDevice));
    SE2_HIP(hipMemcpy(db->d_n + slot, &n32, sizeof n32, hipMemcpyHostToDevice));
    SE2_HIP(hipMemcpy(db->d_kf + slot, &s.kf_id, sizeof(int32_t), hipMemcpyHostToDevice));
    return SE2GPU_OK;
}

int se2gpu_bowdb_add_device(se2gpu_bowdb* db, se2gpu_bow* ctx, int kf_id, const uint32_t* d_word, const double* d_value, const int32_t* d_n,
                            int cap) {
    SE2_REQUIRE(db && ctx && d_word && d_value && d_n && cap >= 1, SE2GPU_ERR_INVALID, "bowdb_add_device: bad argument");
    SE2_REQUIRE(ctx->voc == db->voc, SE2GPU_ERR_INVALID, "bowdb_add_device: the context and the data base belong to different vocabularies");
    SE2_REQUIRE(cap <= kMaxFeat, SE2GPU_ERR_CAPACITY, "bowdb_add_device: cap %d exceeds %d", cap, kMaxFeat);
    int slot = -1;
    SE2_CHECK(db_new_slot(db, kf_id, cap, &slot));
    SE2_CHECK(db_enter(db, ctx->stream));
    const se2gpu_bowdb::Slot& s = db->slots[slot];
    hipLaunchKernelGGL(k_bow_db_put, dim3((cap + 255) / 256), dim3(256), 0, ctx->stream, d_word, d_value, d_n, std::min(cap, s.cap),
                       db->d_word + s.off, db->d_value + s.off, db->d_n + slot, db->d_off + slot, db->d_kf + slot, s.off, s.kf_id);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

int se2gpu_bowdb_remove(se2gpu_bowdb* db, int kf_id) {
    SE2_REQUIRE(db, SE2GPU_ERR_INVALID, "bowdb_remove: db is NULL");
    for (size_t i = 0; i < db->order.size(); ++i)
        if (db->slots[db->order[i]].kf_id == kf_id) {
            db->free_slots.push_back(db->order[i]);
            db->order.erase(db->order.begin() + (ptrdiff_t)i);   // closes the gap, keeps the order
            db->order_dirty = true;
            return SE2GPU_OK;
        }
    set_error("bowdb_remove: key frame %d is not in the data base", kf_id);
    return SE2GPU_ERR_INVALID;
}

int se2gpu_bowdb_query(se2gpu_bowdb* db, se2gpu_bow* ctx, const uint32_t* word, const double* value, int n, int query_on_device,
                       int cur_kf_id, int min_kfid_offset, double* scores_out, int* best_entry, int* best_kf_id, double* best_score) {
    SE2_REQUIRE(db && ctx && n >= 0 && (n == 0 || (word && value)), SE2GPU_ERR_INVALID, "bowdb_query: bad argument");
    SE2_REQUIRE(ctx->voc == db->voc, SE2GPU_ERR_INVALID, "bowdb_query: the context and the data base belong to different vocabularies");
    SE2_REQUIRE(n <= ctx->max_features, SE2GPU_ERR_CAPACITY, "bowdb_query: %d query words exceed the context's %d", n, ctx->max_features);
    if (best_entry) *best_entry = -1;
    if (best_kf_id) *best_kf_id = -1;
    if (best_score) *best_score = 0.0;
    const int size = (int)db->order.size();
    if (size == 0) return SE2GPU_OK;
    const uint32_t words = (uint32_t)db->voc->words;
    hipStream_t s = ctx->stream;
    const uint32_t* qw = word;
    const double* qv = value;
    if (!query_on_device && n) {
        for (int i = 0; i < n; ++i)
            SE2_REQUIRE((i == 0 || word[i - 1] < word[i]) && word[i] < words, SE2GPU_ERR_INVALID,
                        "bowdb_query: word ids must ascend and lie below the vocabulary's %u words", words);
        SE2_HIP(hipMemcpyAsync(ctx->q_word.p, word, sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
        SE2_HIP(hipMemcpyAsync(ctx->q_value.p, value, sizeof(double) * n, hipMemcpyHostToDevice, s));
        qw = ctx->q_word.p; qv = ctx->q_value.p;
    }
    SE2_CHECK(db_enter(db, s));
    if (db->order_dirty) {
        SE2_HIP(hipMemcpyAsync(db->d_order, db->order.data(), sizeof(int32_t) * size, hipMemcpyHostToDevice, s));
        SE2_HIP(hipStreamSynchronize(s));
        db->order_dirty = false;
    }
    if (++ctx->epoch >= (1u << (32 - kTagBits))) {   // the tags of 2^20 queries ago come round again: start over
        SE2_HIP(hipMemsetAsync(ctx->tag.p, 0, sizeof(uint32_t) * std::max<uint32_t>(words, 1), s));
        ctx->epoch = 1;
    }
    SE2_CHECK(ctx->scores.reserve((size_t)size));
    if (n) hipLaunchKernelGGL(k_bow_query_scatter, dim3((n + 255) / 256), dim3(256), 0, s, qw, n, words, ctx->epoch, ctx->tag.p);
    hipLaunchKernelGGL(k_bow_score, dim3((unsigned)(((long long)size * 64 + 255) / 256)), dim3(256), 0, s, ctx->tag.p, ctx->epoch, words, qv,
                       db->voc->scoring, db->d_order, size, db->d_off, db->d_n, db->d_word, db->d_value, ctx->scores.p);
    hipLaunchKernelGGL(k_bow_best, dim3(1), dim3(1024), 0, s, ctx->scores.p, db->d_order, db->d_kf, size, cur_kf_id, min_kfid_offset,
                       ctx->best.p);
    SE2_HIP(hipGetLastError());
    BowBest b;
    SE2_HIP(hipMemcpyAsync(&b, ctx->best.p, sizeof b, hipMemcpyDeviceToHost, s));
    if (scores_out) SE2_HIP(hipMemcpyAsync(scores_out, ctx->scores.p, sizeof(double) * size, hipMemcpyDeviceToHost, s));
    SE2_HIP(hipStreamSynchronize(s));
    db->pending = false;
    if (best_entry) *best_entry = b.entry;
    if (best_kf_id) *best_kf_id = b.kf_id;
    if (best_score) *best_score = b.score;
    return SE2GPU_OK;
}

}  // extern "C"
