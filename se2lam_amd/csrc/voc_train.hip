// Training a DBoW2 vocabulary on the device: hierarchical k-means++ over 256-bit descriptors, level by level.
//   TemplatedVocabulary::create / HKmeansStep / initiateClustersKMpp / setNodeWeights   TemplatedVocabulary.h:573-1020
//   FORB::meanValue, FORB::distance                                                     FORB.cpp:29-102
// The algorithm is specified in include/se2lam_amd/VocabularyTrain.h; the result equals the host mirror
// ORBVocabulary::create bit for bit, statistics included ("Vocabulary training").  Everything is integer work
// except cut_d = u * (double)sum (one exact conversion, one IEEE multiply; compiled with -ffp-contract=off) and the weights,
// which the host computes with libm.
//
// All k-means nodes of one depth are trained together.  order[] is a permutation of the feature indices in which every node
// of the level owns a contiguous range of positions, ascending inside the node - the reference's member order, which a stable
// split preserves.  A node's range is cut into tiles of 256 positions (the last one masked); one workgroup works on one
// tile, so the node's parameters are uniform in the workgroup.  Every kernel ends by itself; the host reads one word per
// Lloyd iteration of a level (how many nodes still move) and the cluster sizes and centres once per level.
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>

#include "../../include/se2lam_amd/VocabularyTrain.h"
#include "../../include/se2lam_amd/VocabularyTree.h"
#include "common.h"
#include "wave_int.h"

using namespace se2gpu;
namespace vt = se2lam_amd::voctrain;

namespace {

constexpr int kTile = 256;
constexpr int kMaxK = vt::kMaxK;
constexpr int kCntStride = 257;   // 256 bit counters and the member count of one (node, cluster)

struct VtNode {
    int32_t start, count;     // the node's positions in order[]
    int32_t tile0, ntiles;
    int32_t nseed;            // clusters seeded so far = the node's number of centres
    int32_t seeding;          // 1 while the seeding goes on
    int32_t done, capped, iters, changed;
    int32_t mt;               // index among the level's nodes of more than one tile, or -1
    uint32_t draws;           // draws consumed
    uint64_t key;
};

__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
           __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ---- the features -----------------------------------------------------------------------------------------------------
// desc (nframes x cap x 32 bytes, counts clamped to 0..cap) -> the feature list (dst_cap == 0: document f from doc_start[f])
// or the same layout with another capacity (dst_cap > 0)
__global__ void __launch_bounds__(256) k_vt_gather(const uint4* __restrict__ src, const int32_t* __restrict__ counts, int cap, int nframes,
                                                   const int32_t* __restrict__ doc_start, uint4* __restrict__ dst, int dst_cap) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = (int)(gid / cap), i = (int)(gid % cap);
    if (f >= nframes) return;
    const int cnt = min(max(counts[f], 0), cap);
    if (i >= cnt) return;
    const size_t d = dst_cap > 0 ? (size_t)f * dst_cap + i : (size_t)doc_start[f] + i;
    dst[2 * d] = src[2 * ((size_t)f * cap + i)];
    dst[2 * d + 1] = src[2 * ((size_t)f * cap + i) + 1];
}

__global__ void k_vt_iota(int32_t* __restrict__ order, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) order[i] = i;
}

// out[j] = the feature at position pos[j]: the descriptors of the children of trivial nodes
__global__ void k_vt_fetch(const uint4* __restrict__ feat, const int32_t* __restrict__ order, const int32_t* __restrict__ pos, int n,
                           uint4* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int f = order[pos[j]];
    out[2 * j] = feat[2 * (size_t)f];
    out[2 * j + 1] = feat[2 * (size_t)f + 1];
}

// ---- seeding ----------------------------------------------------------------------------------------------------------
__global__ void k_vt_seed_first(VtNode* __restrict__ nodes, int nnodes, int k, const int32_t* __restrict__ order, const uint4* __restrict__ feat,
                                uint4* __restrict__ centres) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnodes) return;
    VtNode& nd = nodes[i];
    int idx = (int)(vt::draw(nd.key, 0) * (double)nd.count);
    idx = min(idx, nd.count - 1);
    const int f = order[nd.start + idx];
    centres[2 * (size_t)i * k] = feat[2 * (size_t)f];
    centres[2 * (size_t)i * k + 1] = feat[2 * (size_t)f + 1];
    nd.nseed = 1;
    nd.draws = 1;
    nd.seeding = 1;
}

// the minimal distances against the node's newest seed, and their sum over the tile
__global__ void __launch_bounds__(kTile) k_vt_seed_dist(const VtNode* __restrict__ nodes, const int32_t* __restrict__ tile_node, int k,
                                                        const int32_t* __restrict__ order, const uint4* __restrict__ feat,
                                                        const uint4* __restrict__ centres, int32_t* __restrict__ md,
                                                        long long* __restrict__ tile_sum) {
    __shared__ long long s_w[kTile / 64];
    const int node = tile_node[blockIdx.x];
    const VtNode nd = nodes[node];
    if (!nd.seeding) return;
    const int local = ((int)blockIdx.x - nd.tile0) * kTile + (int)threadIdx.x;
    int v = 0;
    if (local < nd.count) {
        const int pos = nd.start + local;
        const int f = order[pos];
        const size_t c = 2 * ((size_t)node * k + nd.nseed - 1);
        const int d = hamming(feat[2 * (size_t)f], feat[2 * (size_t)f + 1], centres[c], centres[c + 1]);
        int m = d;
        if (nd.nseed > 1) {
            m = md[pos];
            if (m > 0 && d < m) m = d;
        }
        md[pos] = m;
        v = m;
    }
    long long total;
    (void)block_scan_excl<kTile / 64>((long long)v, s_w, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// per node: the sum, the cut, the first member whose inclusive running sum reaches the cut -> the next seed
__global__ void __launch_bounds__(kTile) k_vt_seed_pick(VtNode* __restrict__ nodes, int k, const int32_t* __restrict__ order,
                                                        const uint4* __restrict__ feat, uint4* __restrict__ centres,
                                                        const int32_t* __restrict__ md, const long long* __restrict__ tile_sum) {
    __shared__ long long s_w[kTile / 64];
    __shared__ double s_cut;
    __shared__ int s_first;
    __shared__ long long s_base;
    const int node = blockIdx.x, tid = threadIdx.x;
    const VtNode nd = nodes[node];
    if (!nd.seeding) return;
    long long part = 0, sum;
    for (int t = tid; t < nd.ntiles; t += kTile) part += tile_sum[nd.tile0 + t];
    (void)block_scan_excl<kTile / 64>(part, s_w, sum);
    if (sum == 0) {   // every member coincides with a seed: fewer than k clusters
        if (tid == 0) nodes[node].seeding = 0;
        return;
    }
    if (tid == 0) {
        uint32_t j = nd.draws;
        double cut;
        do cut = vt::draw(nd.key, j++) * (double)sum; while (cut == 0.0);
        s_cut = cut;
        nodes[node].draws = j;
        s_first = INT_MAX;
        s_base = 0;
    }
    __syncthreads();
    const double cut = s_cut;
    // the tile
    long long carry = 0;
    int tile = -1;
    for (int base = 0; base < nd.ntiles; base += kTile) {
        const int t = base + tid;
        const long long v = t < nd.ntiles ? tile_sum[nd.tile0 + t] : 0;
        long long chunk;
        const long long pre = carry + block_scan_excl<kTile / 64>(v, s_w, chunk) + v;   // inclusive
        if (t < nd.ntiles && (double)pre >= cut) atomicMin(&s_first, t);
        __syncthreads();
        tile = s_first;
        if (tile != INT_MAX) {
            if (t == tile) s_base = pre - v;
            break;
        }
        carry += chunk;
    }
    __syncthreads();
    int pick = nd.count - 1;   // "the last member if none"
    if (tile != INT_MAX && tile >= 0) {
        const long long before = s_base;
        __syncthreads();
        if (tid == 0) s_first = INT_MAX;
        __syncthreads();
        const int local = tile * kTile + tid;
        const long long v = local < nd.count ? md[nd.start + local] : 0;
        long long unused;
        const long long pre = before + block_scan_excl<kTile / 64>(v, s_w, unused) + v;
        if (local < nd.count && (double)pre >= cut) atomicMin(&s_first, local);
        __syncthreads();
        if (s_first != INT_MAX) pick = s_first;
    }
    if (tid < 2) {
        const int f = order[nd.start + pick];
        centres[2 * ((size_t)node * k + nd.nseed) + tid] = feat[2 * (size_t)f + tid];
    }
    if (tid == 0) {
        nodes[node].nseed = nd.nseed + 1;
        if (nd.nseed + 1 >= k) nodes[node].seeding = 0;
    }
}

// ---- Lloyd ------------------------------------------------------------------------------------------------------------
// one descriptor against the centres of its node; the first minimum through (distance << 8 | cluster)
__global__ void __launch_bounds__(kTile) k_vt_assign(VtNode* __restrict__ nodes, const int32_t* __restrict__ tile_node, int k,
                                                     const int32_t* __restrict__ order, const uint4* __restrict__ feat,
                                                     const uint4* __restrict__ centres, uint8_t* __restrict__ asg) {
    __shared__ uint4 s_c[2 * kMaxK];
    const int node = tile_node[blockIdx.x];
    const VtNode nd = nodes[node];
    if (nd.done) return;
    const int ncl = nd.nseed;
    if ((int)threadIdx.x < 2 * ncl) s_c[threadIdx.x] = centres[2 * (size_t)node * k + threadIdx.x];
    __syncthreads();
    const int local = ((int)blockIdx.x - nd.tile0) * kTile + (int)threadIdx.x;
    int diff = 0;
    if (local < nd.count) {
        const int pos = nd.start + local;
        const int f = order[pos];
        const uint4 a0 = feat[2 * (size_t)f], a1 = feat[2 * (size_t)f + 1];
        unsigned best = ~0u;
        for (int c = 0; c < ncl; ++c) {
            const unsigned key = ((unsigned)hamming(a0, a1, s_c[2 * c], s_c[2 * c + 1]) << 8) | (unsigned)c;
            best = min(best, key);
        }
        const uint8_t c = (uint8_t)(best & 0xffu);
        diff = asg[pos] != c;
        asg[pos] = c;
    }
    if (__syncthreads_or(diff) && threadIdx.x == 0) atomicOr(&nodes[node].changed, 1);
}

// after an assignment: which nodes stop (the assignment repeated itself, or max_iters reached), how many go on
__global__ void k_vt_ctrl(VtNode* __restrict__ nodes, int nnodes, int max_iters, int32_t* __restrict__ active) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnodes) return;
    VtNode& nd = nodes[i];
    if (nd.done) return;
    nd.iters += 1;
    if (nd.iters > 1 && !nd.changed) nd.done = 1;
    else if (nd.iters >= max_iters) { nd.done = 1; nd.capped = 1; }
    else atomicAdd(active, 1);
    nd.changed = 0;
}

// bit b of the mean of n members is set when at least n / 2 + n % 2 of them have it; the 64 lanes of a wave hold 64
// consecutive bits = two words of the centre
__device__ __forceinline__ void store_majority(uint32_t count_b, int n, uint32_t* centre_words) {
    const unsigned long long mask = __ballot(count_b >= (uint32_t)vt::majorityThreshold(n));
    if ((threadIdx.x & 63) == 0) {
        centre_words[2 * (threadIdx.x >> 6)] = (uint32_t)mask;
        centre_words[2 * (threadIdx.x >> 6) + 1] = (uint32_t)(mask >> 32);
    }
}

// per (node, cluster) 256 bit counters and a member count.  Thread b owns bit b: it walks the tile's members in LDS and adds
// into its own column of the counters (no atomics in LDS, bank = b % 32).  A node of one tile turns the counters into centres
// at once; a node of several tiles flushes the non-zero ones into global counters (integer atomics: the sum has no order).
__global__ void __launch_bounds__(kTile) k_vt_mean(const VtNode* __restrict__ nodes, const int32_t* __restrict__ tile_node, int k,
                                                   const int32_t* __restrict__ order, const uint4* __restrict__ feat,
                                                   const uint8_t* __restrict__ asg, uint4* __restrict__ centres, uint32_t* __restrict__ gcnt) {
    __shared__ uint32_t s_cnt[kMaxK * 256];
    __shared__ uint32_t s_feat[8 * kTile];   // word w of member m at w * 256 + m
    __shared__ uint8_t s_asg[kTile];
    __shared__ uint32_t s_n[kMaxK];
    const int node = tile_node[blockIdx.x], b = threadIdx.x;
    const VtNode nd = nodes[node];
    if (nd.done) return;
    const int ncl = nd.nseed;
    const int local0 = ((int)blockIdx.x - nd.tile0) * kTile;
    const int nm = min(kTile, nd.count - local0);
    for (int c = 0; c < ncl; ++c) s_cnt[c * 256 + b] = 0;
    if (b < kMaxK) s_n[b] = 0;
    __syncthreads();
    if (b < nm) {
        const int pos = nd.start + local0 + b;
        const int f = order[pos];
        const uint4 a0 = feat[2 * (size_t)f], a1 = feat[2 * (size_t)f + 1];
        s_feat[0 * kTile + b] = a0.x; s_feat[1 * kTile + b] = a0.y; s_feat[2 * kTile + b] = a0.z; s_feat[3 * kTile + b] = a0.w;
        s_feat[4 * kTile + b] = a1.x; s_feat[5 * kTile + b] = a1.y; s_feat[6 * kTile + b] = a1.z; s_feat[7 * kTile + b] = a1.w;
        const uint8_t c = asg[pos];
        s_asg[b] = c;
        atomicAdd(&s_n[c], 1u);
    }
    __syncthreads();
    const uint32_t* col = s_feat + (b >> 5) * kTile;
    const int sh = b & 31;
    for (int m = 0; m < nm; ++m) s_cnt[s_asg[m] * 256 + b] += (col[m] >> sh) & 1u;
    __syncthreads();
    if (nd.mt < 0) {
        for (int c = 0; c < ncl; ++c) {
            const int n = (int)s_n[c];
            if (n == 0) continue;   // a cluster without members keeps its centre
            store_majority(s_cnt[c * 256 + b], n, reinterpret_cast<uint32_t*>(centres + 2 * ((size_t)node * k + c)));
        }
    } else {
        uint32_t* g = gcnt + (size_t)nd.mt * k * kCntStride;
        for (int c = 0; c < ncl; ++c) {
            const uint32_t v = s_cnt[c * 256 + b];
            if (v) atomicAdd(&g[c * kCntStride + b], v);
        }
        if (b < ncl && s_n[b]) atomicAdd(&g[b * kCntStride + 256], s_n[b]);
    }
}

__global__ void __launch_bounds__(kTile) k_vt_mean_fin(const VtNode* __restrict__ nodes, const int32_t* __restrict__ mt_node, int k,
                                                       const uint32_t* __restrict__ gcnt, uint4* __restrict__ centres) {
    const int node = mt_node[blockIdx.x], b = threadIdx.x;
    const VtNode nd = nodes[node];
    if (nd.done) return;
    const uint32_t* g = gcnt + (size_t)blockIdx.x * k * kCntStride;
    for (int c = 0; c < nd.nseed; ++c) {
        const int n = (int)g[c * kCntStride + 256];
        if (n == 0) continue;
        store_majority(g[c * kCntStride + b], n, reinterpret_cast<uint32_t*>(centres + 2 * ((size_t)node * k + c)));
    }
}

// ---- the stable split -------------------------------------------------------------------------------------------------
// the rank of this lane among the lanes of its wave with the same cluster and a lower lane id; s_w[wave * 32 + c] = the
// wave's members of cluster c
__device__ __forceinline__ int wave_rank(bool valid, int c, int ncl, int* s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int rank = 0;
    for (int cc = 0; cc < ncl; ++cc) {
        const bool mine = valid && c == cc;
        const unsigned long long mask = __ballot(mine);
        if (lane == 0) s_w[w * kMaxK + cc] = __popcll(mask);
        if (mine) rank = lane_rank(mask);
    }
    return rank;
}

__global__ void __launch_bounds__(kTile) k_vt_split_count(const VtNode* __restrict__ nodes, const int32_t* __restrict__ tile_node,
                                                          const uint8_t* __restrict__ asg, int32_t* __restrict__ tile_cnt) {
    __shared__ int s_w[4 * kMaxK];
    const int node = tile_node[blockIdx.x];
    const VtNode nd = nodes[node];
    const int local = ((int)blockIdx.x - nd.tile0) * kTile + (int)threadIdx.x;
    const bool valid = local < nd.count;
    const int c = valid ? asg[nd.start + local] : 0;
    (void)wave_rank(valid, c, nd.nseed, s_w);
    __syncthreads();
    if ((int)threadIdx.x < kMaxK) {
        const int cc = threadIdx.x;
        tile_cnt[(size_t)blockIdx.x * kMaxK + cc] = cc < nd.nseed ? s_w[cc] + s_w[kMaxK + cc] + s_w[2 * kMaxK + cc] + s_w[3 * kMaxK + cc] : 0;
    }
}

// one wave per node, lane c = cluster c: the exclusive scan in (cluster-major, tile-minor) order.  tile_cnt becomes the
// offset of the tile's members of cluster c inside the cluster; cl_count / cl_base are the cluster's size and first position
__global__ void __launch_bounds__(64) k_vt_split_scan(const VtNode* __restrict__ nodes, int k, int32_t* __restrict__ tile_cnt,
                                                      int32_t* __restrict__ cl_count, int32_t* __restrict__ cl_base) {
    const int node = blockIdx.x, c = threadIdx.x;
    const VtNode nd = nodes[node];
    int run = 0;
    if (c < nd.nseed)
        for (int t = 0; t < nd.ntiles; ++t) {
            int32_t* p = tile_cnt + (size_t)(nd.tile0 + t) * kMaxK + c;
            const int v = *p;
            *p = run;
            run += v;
        }
    const int inc = wave_scan_incl(run);
    if (c < k) {
        cl_count[(size_t)node * k + c] = run;
        cl_base[(size_t)node * k + c] = inc - run;
    }
}

__global__ void __launch_bounds__(kTile) k_vt_split_scatter(const VtNode* __restrict__ nodes, const int32_t* __restrict__ tile_node, int k,
                                                            const uint8_t* __restrict__ asg, const int32_t* __restrict__ tile_off,
                                                            const int32_t* __restrict__ cl_base, const int32_t* __restrict__ order_in,
                                                            int32_t* __restrict__ order_out) {
    __shared__ int s_w[4 * kMaxK];
    const int node = tile_node[blockIdx.x];
    const VtNode nd = nodes[node];
    const int local = ((int)blockIdx.x - nd.tile0) * kTile + (int)threadIdx.x;
    const bool valid = local < nd.count;
    const int c = valid ? asg[nd.start + local] : 0;
    const int rank = wave_rank(valid, c, nd.nseed, s_w);
    __syncthreads();
    if (!valid) return;
    int before = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_w[w * kMaxK + c];
    const int dst = nd.start + cl_base[(size_t)node * k + c] + tile_off[(size_t)blockIdx.x * kMaxK + c] + before + rank;
    order_out[dst] = order_in[nd.start + local];
}

// ---- weights ----------------------------------------------------------------------------------------------------------
// Ni: a document's BowVector holds each of its words once
__global__ void k_vt_doc_hist(const uint32_t* __restrict__ bow_word, const int32_t* __restrict__ bow_n, int cap, int nframes, int words,
                              int32_t* __restrict__ ni) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = (int)(gid / cap), p = (int)(gid % cap);
    if (f >= nframes || p >= min(max(bow_n[f], 0), cap)) return;
    const uint32_t w = bow_word[(size_t)f * cap + p];
    if (w < (uint32_t)words) atomicAdd(&ni[w], 1);
}

// se2gpu_voc_train_profile: the switch, and the table of the training call that ended last.  A call times into a table of its
// own (Trainer::prof) and publishes it under the mutex, so concurrent calls share nothing while they run.
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mutex;
std::vector<LaunchProfile::Slot> g_prof_last;

struct HostNode {   // a k-means node of the current level on the host side
    int32_t hnode, start, count;
    uint64_t key;
};

struct Trainer {
    int k = 0, L = 0, max_iters = 0;
    hipStream_t s = nullptr;
    int N = 0;
    DevBuf<uint4> feat, centres, fetched;
    DevBuf<int32_t> order[2], md, tile_node, tile_cnt, cl_count, cl_base, mt_node, active, fetch_pos;
    DevBuf<long long> tile_sum;
    DevBuf<uint8_t> asg;
    DevBuf<VtNode> nodes;
    DevBuf<uint32_t> gcnt;
    PinBuf<int32_t> h_active;
    // the tree in creation order: a parent precedes its children, siblings are created in cluster order
    std::vector<int32_t> h_parent;
    std::vector<uint8_t> h_desc;
    se2lam_amd::TrainStats st;
    LaunchProfile prof;
    ~Trainer() {
        if (s) (void)hipStreamDestroy(s);
    }

    int32_t new_node(int32_t parent, const uint8_t* d) {
        h_parent.push_back(parent);
        h_desc.insert(h_desc.end(), 32, 0);
        if (d) std::memcpy(&h_desc[h_desc.size() - 32], d, 32);
        return (int32_t)h_parent.size() - 1;
    }

    // a node of `count` members at `level`: trivial (its members become leaves, their descriptors fetched later) or k-means
    void place(int32_t hnode, int32_t start, int32_t count, uint64_t key, std::vector<HostNode>& next, std::vector<int32_t>& fpos,
               std::vector<int32_t>& fnode) {
        if (count <= k) {
            ++st.trivial_nodes;
            for (int m = 0; m < count; ++m) {
                fnode.push_back(new_node(hnode, nullptr));
                fpos.push_back(start + m);
            }
        } else {
            next.push_back({hnode, start, count, key});
        }
    }

    int fetch(int cur, const std::vector<int32_t>& fpos, const std::vector<int32_t>& fnode) {
        const int n = (int)fpos.size();
        if (!n) return SE2GPU_OK;
        SE2_CHECK(fetch_pos.upload(fpos, s));
        SE2_CHECK(fetched.reserve(2 * (size_t)n));
        SE2_LAUNCH(prof, s, "k_vt_fetch", k_vt_fetch, dim3((n + 255) / 256), dim3(256), 0, feat.p, order[cur].p, fetch_pos.p, n, fetched.p);
        std::vector<uint8_t> h((size_t)n * 32);
        SE2_HIP(hipMemcpyAsync(h.data(), fetched.p, h.size(), hipMemcpyDeviceToHost, s));
        SE2_HIP(hipStreamSynchronize(s));
        for (int j = 0; j < n; ++j) std::memcpy(&h_desc[(size_t)fnode[j] * 32], &h[(size_t)j * 32], 32);
        return SE2GPU_OK;
    }

    int level(const std::vector<HostNode>& lv, int lev, int& cur, std::vector<HostNode>& next) {
        const int nn = (int)lv.size();
        std::vector<VtNode> hn(nn);
        std::vector<int32_t> h_tile_node, h_mt;
        for (int i = 0; i < nn; ++i) {
            VtNode& v = hn[i];
            v = VtNode{};
            v.start = lv[i].start; v.count = lv[i].count; v.key = lv[i].key;
            v.tile0 = (int32_t)h_tile_node.size();
            v.ntiles = (v.count + kTile - 1) / kTile;
            v.mt = -1;
            if (v.ntiles > 1) { v.mt = (int32_t)h_mt.size(); h_mt.push_back(i); }
            h_tile_node.insert(h_tile_node.end(), v.ntiles, i);
        }
        const int nt = (int)h_tile_node.size(), nmt = (int)h_mt.size();
        SE2_CHECK(nodes.upload(hn, s));
        SE2_CHECK(tile_node.upload(h_tile_node, s));
        if (nmt) SE2_CHECK(mt_node.upload(h_mt, s));
        SE2_CHECK(tile_sum.reserve(nt));
        SE2_CHECK(tile_cnt.reserve((size_t)nt * kMaxK));
        SE2_CHECK(centres.reserve(2 * (size_t)nn * k));
        SE2_CHECK(cl_count.reserve((size_t)nn * k));
        SE2_CHECK(cl_base.reserve((size_t)nn * k));
        const size_t gbytes = (size_t)nmt * k * kCntStride * sizeof(uint32_t);
        if (nmt) SE2_CHECK(gcnt.reserve((size_t)nmt * k * kCntStride));
        const dim3 per_node((nn + 255) / 256), b256(256);

        SE2_LAUNCH(prof, s, "k_vt_seed_first", k_vt_seed_first, per_node, b256, 0, nodes.p, nn, k, order[cur].p, feat.p, centres.p);
        for (int t = 1; t < k; ++t) {
            SE2_LAUNCH(prof, s, "k_vt_seed_dist", k_vt_seed_dist, dim3(nt), dim3(kTile), 0, nodes.p, tile_node.p, k, order[cur].p, feat.p, centres.p,
                       md.p, tile_sum.p);
            SE2_LAUNCH(prof, s, "k_vt_seed_pick", k_vt_seed_pick, dim3(nn), dim3(kTile), 0, nodes.p, k, order[cur].p, feat.p, centres.p, md.p,
                       tile_sum.p);
        }
        for (;;) {
            SE2_LAUNCH(prof, s, "k_vt_assign", k_vt_assign, dim3(nt), dim3(kTile), 0, nodes.p, tile_node.p, k, order[cur].p, feat.p, centres.p, asg.p);
            SE2_HIP(hipMemsetAsync(active.p, 0, sizeof(int32_t), s));
            SE2_LAUNCH(prof, s, "k_vt_ctrl", k_vt_ctrl, per_node, b256, 0, nodes.p, nn, max_iters, active.p);
            SE2_HIP(hipMemcpyAsync(h_active.p, active.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            SE2_HIP(hipStreamSynchronize(s));
            if (*h_active.p <= 0) break;
            if (nmt) SE2_HIP(hipMemsetAsync(gcnt.p, 0, gbytes, s));
            SE2_LAUNCH(prof, s, "k_vt_mean", k_vt_mean, dim3(nt), dim3(kTile), 0, nodes.p, tile_node.p, k, order[cur].p, feat.p, asg.p, centres.p,
                       gcnt.p);
            if (nmt) SE2_LAUNCH(prof, s, "k_vt_mean_fin", k_vt_mean_fin, dim3(nmt), dim3(kTile), 0, nodes.p, mt_node.p, k, gcnt.p, centres.p);
        }
        SE2_LAUNCH(prof, s, "k_vt_split_count", k_vt_split_count, dim3(nt), dim3(kTile), 0, nodes.p, tile_node.p, asg.p, tile_cnt.p);
        SE2_LAUNCH(prof, s, "k_vt_split_scan", k_vt_split_scan, dim3(nn), dim3(64), 0, nodes.p, k, tile_cnt.p, cl_count.p, cl_base.p);
        SE2_LAUNCH(prof, s, "k_vt_split_scatter", k_vt_split_scatter, dim3(nt), dim3(kTile), 0, nodes.p, tile_node.p, k, asg.p, tile_cnt.p, cl_base.p,
                   order[cur].p, order[cur ^ 1].p);
        SE2_HIP(hipGetLastError());
        std::vector<int32_t> h_cnt((size_t)nn * k), h_base((size_t)nn * k);
        std::vector<uint8_t> h_centres((size_t)nn * k * 32);
        SE2_HIP(hipMemcpyAsync(hn.data(), nodes.p, sizeof(VtNode) * nn, hipMemcpyDeviceToHost, s));
        SE2_HIP(hipMemcpyAsync(h_cnt.data(), cl_count.p, sizeof(int32_t) * h_cnt.size(), hipMemcpyDeviceToHost, s));
        SE2_HIP(hipMemcpyAsync(h_base.data(), cl_base.p, sizeof(int32_t) * h_base.size(), hipMemcpyDeviceToHost, s));
        SE2_HIP(hipMemcpyAsync(h_centres.data(), centres.p, h_centres.size(), hipMemcpyDeviceToHost, s));
        SE2_HIP(hipStreamSynchronize(s));
        cur ^= 1;

        std::vector<int32_t> fpos, fnode;
        for (int i = 0; i < nn; ++i) {
            const VtNode& v = hn[i];
            const int ncl = v.nseed;
            SE2_REQUIRE(ncl >= 1 && ncl <= k && v.done, SE2GPU_ERR_HIP, "voc_train: the device returned an impossible node state");
            ++st.kmeans_nodes;
            st.short_seeded_nodes += ncl < k;
            st.capped_nodes += v.capped;
            st.lloyd_iters_total += v.iters;
            st.lloyd_iters_max = std::max(st.lloyd_iters_max, v.iters);
            int64_t sum = 0;
            for (int c = 0; c < ncl; ++c) {
                const int32_t cnt = h_cnt[(size_t)i * k + c], base = h_base[(size_t)i * k + c];
                SE2_REQUIRE(cnt >= 0 && base == sum, SE2GPU_ERR_HIP, "voc_train: the device returned impossible cluster sizes");
                sum += cnt;
                if (cnt == 0) { ++st.empty_clusters; continue; }
                const int32_t h = new_node(lv[i].hnode, &h_centres[((size_t)i * k + c) * 32]);
                if (cnt > 1 && lev < L) place(h, v.start + base, cnt, vt::childKey(v.key, c), next, fpos, fnode);
            }
            SE2_REQUIRE(sum == v.count, SE2GPU_ERR_HIP, "voc_train: the device returned impossible cluster sizes");
        }
        return fetch(cur, fpos, fnode);
    }
};

}  // namespace

extern "C" {

int se2gpu_voc_train_profile(int enable) {
    g_prof_on.store(enable != 0);
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_last.clear();
    return SE2GPU_OK;
}

int se2gpu_voc_train_profile_get(int idx, const char** name, double* ms, int64_t* launches) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if (idx < 0 || idx >= (int)g_prof_last.size()) return SE2GPU_ERR_INVALID;
    if (name) *name = g_prof_last[idx].name;   // a string literal of this file
    if (ms) *ms = g_prof_last[idx].ms;
    if (launches) *launches = g_prof_last[idx].launches;
    return SE2GPU_OK;
}

int se2gpu_voc_train(const se2gpu_voc_train_params* p, const uint8_t* desc, const int32_t* counts, int cap, int nframes, int on_device,
                     se2gpu_voc** out, se2gpu_voc_train_stats* stats) {
    static_assert(sizeof(se2gpu_voc_train_stats) == sizeof(se2lam_amd::TrainStats), "stats layout");
    SE2_REQUIRE(out, SE2GPU_ERR_INVALID, "voc_train: out is NULL");
    *out = nullptr;
    if (stats) *stats = se2gpu_voc_train_stats{};
    SE2_REQUIRE(have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)");
    SE2_REQUIRE(p && desc && counts && cap >= 1 && nframes >= 1, SE2GPU_ERR_INVALID, "voc_train: bad argument");
    SE2_REQUIRE(vt::paramsOk(p->k, p->L, p->scoring, p->weighting) && p->max_iters >= 0, SE2GPU_ERR_INVALID,
                "voc_train: k must be in 2..%d, L in 1..%d, scoring in 0..5, weighting in 0..3, max_iters >= 0", vt::kMaxK, vt::kMaxL);
    SE2_REQUIRE((long long)nframes * cap <= INT32_MAX, SE2GPU_ERR_CAPACITY, "voc_train: %d x %d descriptor slots exceed 2^31 - 1", nframes, cap);
    SE2_REQUIRE(!on_device || ((uintptr_t)desc & 15) == 0, SE2GPU_ERR_INVALID, "voc_train: a device desc must be 16-byte aligned");

    Trainer T;
    T.prof.enabled = g_prof_on.load();
    T.k = p->k; T.L = p->L; T.max_iters = p->max_iters > 0 ? p->max_iters : vt::kDefaultMaxIters;
    SE2_HIP(hipStreamCreateWithFlags(&T.s, hipStreamNonBlocking));
    hipStream_t s = T.s;

    // the counts decide the feature list: they are needed on the host
    std::vector<int32_t> h_counts(nframes), doc_start(nframes);
    if (on_device) SE2_HIP(hipMemcpy(h_counts.data(), counts, sizeof(int32_t) * nframes, hipMemcpyDeviceToHost));
    else std::copy(counts, counts + nframes, h_counts.begin());
    long long total = 0;
    int max_count = 0;
    for (int f = 0; f < nframes; ++f) {
        h_counts[f] = std::min(std::max(h_counts[f], 0), cap);
        SE2_REQUIRE(h_counts[f] <= vt::kMaxDocFeatures, SE2GPU_ERR_INVALID, "voc_train: document %d holds %d descriptors, more than %d", f, h_counts[f],
                    vt::kMaxDocFeatures);
        doc_start[f] = (int32_t)total;
        total += h_counts[f];
        max_count = std::max(max_count, h_counts[f]);
    }
    SE2_REQUIRE(total > 0, SE2GPU_ERR_INVALID, "voc_train: no descriptor in %d documents", nframes);
    const int N = T.N = (int)total;

    DevBuf<uint8_t> up_desc;
    DevBuf<int32_t> d_counts, d_doc_start;
    const uint8_t* d_desc = desc;
    if (!on_device) {
        SE2_CHECK(up_desc.upload(desc, (size_t)nframes * cap * 32, s));
        d_desc = up_desc.p;
    }
    SE2_CHECK(d_counts.upload(h_counts, s));
    SE2_CHECK(d_doc_start.upload(doc_start, s));
    SE2_CHECK(T.feat.reserve(2 * (size_t)N));
    SE2_CHECK(T.order[0].reserve(N));
    SE2_CHECK(T.order[1].reserve(N));
    SE2_CHECK(T.md.reserve(N));
    SE2_CHECK(T.asg.reserve(N));
    SE2_CHECK(T.active.reserve(1));
    SE2_CHECK(T.h_active.reserve(1));
    const unsigned slot_blocks = (unsigned)(((long long)nframes * cap + 255) / 256);
    SE2_LAUNCH(T.prof, s, "k_vt_gather", k_vt_gather, dim3(slot_blocks), dim3(256), 0, reinterpret_cast<const uint4*>(d_desc), d_counts.p, cap, nframes,
               d_doc_start.p, T.feat.p, 0);
    SE2_LAUNCH(T.prof, s, "k_vt_iota", k_vt_iota, dim3((N + 255) / 256), dim3(256), 0, T.order[0].p, N);
    SE2_HIP(hipGetLastError());

    // ---- the tree, level by level
    T.new_node(0, nullptr);   // the root
    std::vector<HostNode> lv, next;
    int cur = 0;
    {
        std::vector<int32_t> fpos, fnode;
        T.place(0, 0, N, vt::rootKey(p->seed), lv, fpos, fnode);
        SE2_CHECK(T.fetch(cur, fpos, fnode));
    }
    for (int lev = 1; !lv.empty(); ++lev) {
        next.clear();
        SE2_CHECK(T.level(lv, lev, cur, next));
        lv.swap(next);
    }

    // ---- DBoW2's node ids: the children of a node get consecutive ids, then the subtree of each child in turn
    const int32_t M = (int32_t)T.h_parent.size();
    std::vector<int32_t> cptr(M + 1, 0), child(M > 1 ? M - 1 : 0), new_id(M, 0);
    for (int32_t i = 1; i < M; ++i) ++cptr[T.h_parent[i] + 1];
    for (int32_t i = 0; i < M; ++i) cptr[i + 1] += cptr[i];
    {
        std::vector<int32_t> fill(cptr.begin(), cptr.end() - 1);
        for (int32_t i = 1; i < M; ++i) child[fill[T.h_parent[i]]++] = i;
    }
    {
        int32_t next_id = 1;
        std::vector<std::pair<int32_t, int32_t>> stack;   // (node, next child to descend into)
        for (int32_t c = cptr[0]; c < cptr[1]; ++c) new_id[child[c]] = next_id++;
        stack.push_back({0, cptr[0]});
        while (!stack.empty()) {
            auto& top = stack.back();
            if (top.second == cptr[top.first + 1]) { stack.pop_back(); continue; }
            const int32_t h = child[top.second++];
            for (int32_t c = cptr[h]; c < cptr[h + 1]; ++c) new_id[child[c]] = next_id++;
            stack.push_back({h, cptr[h]});
        }
    }
    std::vector<int32_t> parent(M, 0);
    std::vector<uint8_t> ndesc((size_t)M * 32, 0), leaf(M, 0);
    std::vector<double> weight(M, 0.0);
    for (int32_t i = 1; i < M; ++i) {
        const int32_t id = new_id[i];
        parent[id] = new_id[T.h_parent[i]];
        std::memcpy(&ndesc[(size_t)id * 32], &T.h_desc[(size_t)i * 32], 32);
        leaf[id] = cptr[i + 1] == cptr[i];
        weight[id] = leaf[id] ? 1.0 : 0.0;
    }
    std::vector<int32_t> word_node;
    for (int32_t id = 1; id < M; ++id)
        if (leaf[id]) word_node.push_back(id);
    const int words = (int)word_node.size();

    // ---- weights: every training descriptor walks the finished tree (the existing transform); Ni per word
    if (p->weighting == 0 || p->weighting == 2) {
        se2gpu_voc* tmp = nullptr;
        SE2_CHECK(se2gpu_voc_create(p->k, p->L, p->scoring, /*TF: unit weights*/ 1, M, parent.data(), ndesc.data(), weight.data(), leaf.data(), &tmp));
        std::unique_ptr<se2gpu_voc, void (*)(se2gpu_voc*)> tmp_guard(tmp, se2gpu_voc_destroy);
        const int wcap = std::max(max_count, 1), batch = std::min(nframes, 1024);
        se2gpu_bow* bow = nullptr;
        SE2_CHECK(se2gpu_bow_create(tmp, wcap, batch, &bow));
        std::unique_ptr<se2gpu_bow, void (*)(se2gpu_bow*)> bow_guard(bow, se2gpu_bow_destroy);
        SE2_CHECK(se2gpu_bow_set_stream(bow, s));
        const uint8_t* w_desc = d_desc;
        DevBuf<uint4> packed;
        if (cap != wcap) {   // the documents with the capacity the transform's handle was made for
            SE2_CHECK(packed.reserve(2 * (size_t)nframes * wcap));
            SE2_LAUNCH(T.prof, s, "k_vt_gather", k_vt_gather, dim3(slot_blocks), dim3(256), 0, reinterpret_cast<const uint4*>(d_desc), d_counts.p, cap,
                       nframes, d_doc_start.p, packed.p, wcap);
            w_desc = reinterpret_cast<const uint8_t*>(packed.p);
        }
        const size_t slots = (size_t)batch * wcap;
        DevBuf<uint32_t> bw;
        DevBuf<double> bv;
        DevBuf<int32_t> i32, ni;   // bow_n | fv_nn | fv_nodes | fv_idx | fv_ptr
        SE2_CHECK(bw.reserve(slots));
        SE2_CHECK(bv.reserve(slots));
        SE2_CHECK(i32.reserve(2 * (size_t)batch + 2 * slots + (size_t)batch * (wcap + 1)));
        SE2_CHECK(ni.reserve(std::max(words, 1)));
        SE2_HIP(hipMemsetAsync(ni.p, 0, sizeof(int32_t) * std::max(words, 1), s));
        int32_t *bn = i32.p, *fnn = bn + batch, *fn = fnn + batch, *fi = fn + slots, *fp = fi + slots;
        for (int f0 = 0; f0 < nframes; f0 += batch) {
            const int nf = std::min(batch, nframes - f0);
            SE2_CHECK(se2gpu_bow_transform_batch_device(bow, w_desc + (size_t)f0 * wcap * 32, d_counts.p + f0, wcap, nf, 0, bw.p, bv.p, bn, fn, fp, fi, fnn));
            SE2_LAUNCH(T.prof, s, "k_vt_doc_hist", k_vt_doc_hist, dim3((unsigned)(((long long)nf * wcap + 255) / 256)), dim3(256), 0, bw.p, bn, wcap, nf,
                       words, ni.p);
        }
        SE2_HIP(hipGetLastError());
        std::vector<int32_t> h_ni(words);
        SE2_HIP(hipMemcpyAsync(h_ni.data(), ni.p, sizeof(int32_t) * words, hipMemcpyDeviceToHost, s));
        SE2_HIP(hipStreamSynchronize(s));
        for (int w = 0; w < words; ++w) weight[word_node[w]] = (double)vt::idfWeight(nframes, h_ni[w]);
    }
    SE2_HIP(hipStreamSynchronize(s));

    T.st.nodes = M;
    T.st.words = words;
    for (int w = 0; w < words; ++w) T.st.zero_weight_words += !(weight[word_node[w]] > 0);
    SE2_CHECK(se2gpu_voc_create(p->k, p->L, p->scoring, p->weighting, M, parent.data(), ndesc.data(), weight.data(), leaf.data(), out));
    if (stats) std::memcpy(stats, &T.st, sizeof T.st);
    if (T.prof.enabled) {
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        g_prof_last = T.prof.slots;
    }
    return SE2GPU_OK;   // T and the scratch buffers above are released here
}

}  // extern "C"
