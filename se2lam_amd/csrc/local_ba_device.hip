// libse2gpu - local bundle adjustment on the tables where they lie in device memory: se2gpu_local_ba_batch_device.
// se2gpu_local_window_batch_device ends in three lists per job (mLocalGraphKFs, mRefKFs, mLocalGraphMPs in IdLessThan order); this
// call does Map::loadLocalGraph (src/Map.cpp:891-1053 of the reference) on them and on the frame, feature and point tables, and
// runs the one-workgroup-per-window solver (csrc/ba_window.hip) on the graphs, without the host in between:
//   k_local_ba_gather   one workgroup of 1024 threads per job.  The slot -> vertex map over nframes in LDS; the fixed rule, the
//                       poses, the PreSE2 edges (places from a prefix sum over the workgroup); then the points, a wave per point
//                       at a time, twice: a counting pass (edges per point, then a prefix sum over the workgroup gives lm_ptr) and,
//                       once the job's status is known, the pass that writes e_kf, e_uv and e_info.  A frame that stands twice in
//                       a point's list counts once: inside a chunk of 64 entries the lowest lane of a frame wins (readlanes over the chunk),
//                       across chunks a bit row over the vertices in LDS, one per wave (test-and-set, order-free: the lanes that
//                       reach it name different vertices).  No atomic counter anywhere: the same words in every run.
//   k_window_lm_status  csrc/ba_window.hip: window_lm<Se2Model> behind the job's status
//   k_local_ba_finish   one wave per job: poses and landmarks from the buffers BaCtl::sel names, the finite test, d_stats, d_info
// Three launches on the matcher's stream; nothing is allocated, uploaded besides kernel arguments, read back or waited for.
// Every table access goes through obs_table.h (entry rule, segment rule); every slot and point read from a list is range-checked
// before anything is written.  Compiled with -ffp-contract=off (se2lam_amd/build.py).
#include <algorithm>
#include <climits>

#include "ba_window.h"
#include "common.h"
#include "edge_information.h"
#include "wave_int.h"
#include "se2lam_amd/obs_table.h"

using namespace se2gpu;
using se2gpu::badev::BaCtl;
using se2gpu::badev::CamDev;

namespace {

typedef unsigned long long u64;

constexpr int MAX_JOBS = 65535;
constexpr int MAX_FRAMES = SE2GPU_LOCAL_WINDOW_MAX_FRAMES;
constexpr int MAX_FREE = 64;          // 3 * 64 = 192 unknowns: the resident kernel's back-substitution (window_lds_bytes)
constexpr int BLOCK = 1024, WAVES = BLOCK / 64;   // sixteen waves: the points of a window are a chain of dependent loads each, a wave per point
constexpr int VERT_WORDS = MAX_FRAMES / 64;   // a bit per vertex; max_local + max_ref <= MAX_FRAMES is checked

enum { ST_OK = 0, ST_RANGE = 1, ST_FIT = 2, ST_NULL = 3, ST_DEGREE = 4, ST_EMPTY = 5, ST_NONFINITE = 6 };
enum { FLAG_OCTAVE = 1 };             // d_info[6]: an edge was skipped for an octave outside 0..nlevels-1

// d_ws: the regions in this order; a job's slice of a region starts at a multiple of 16 bytes (e_uv is read as double2, desc as int4)
enum {
    WS_CNT, WS_FIXED, WS_POSES, WS_OI, WS_OJ, WS_OMEAS, WS_OINFO, WS_LMPTR, WS_EKF, WS_EUV, WS_EINFO, WS_LMS,   // se2gpu_local_ba_ws_layout
    WS_POSESA, WS_LMSA, WS_POSESB, WS_LMSB, WS_CTL, WS_DESC, WS_AINV, WS_PACK, WS_REGIONS
};
struct WsLayout {
    size_t off[WS_REGIONS], stride[WS_REGIONS];
    size_t bytes;
};

int launch_threads(int max_local, int max_ref, size_t* lds) {
    for (int t : {512, 256, 128}) {
        const size_t b = ba_window_lds_bytes(max_local + max_ref, std::min(max_local, MAX_FREE), t);
        if (b) { if (lds) *lds = b; return t; }
    }
    return 0;
}

bool sizes_positive(int njobs, int max_local, int max_ref, int max_mp, int max_obs) {
    return njobs >= 0 && max_local >= 1 && max_ref >= 1 && max_mp >= 1 && max_obs >= 1;
}
// the product that passes 2^31 - 1, or NULL
const char* product_over(int njobs, int max_local, int max_ref, int max_mp, int max_obs) {
    const long long J = njobs, lim = 2147483647LL;
    if ((long long)max_local + max_ref > MAX_FRAMES) return "max_local + max_ref (at most 4096)";
    if (J * ((long long)max_local + max_ref) * 3 > lim) return "njobs * (max_local + max_ref) * 3";
    if (J * ((long long)max_mp + 1) * 3 > lim) return "njobs * (max_mp + 1) * 3";
    if (J * (long long)max_obs * 3 > lim) return "njobs * max_obs * 3";
    return nullptr;
}
bool ws_args_ok(int njobs, int max_local, int max_ref, int max_mp, int max_obs) {
    return sizes_positive(njobs, max_local, max_ref, max_mp, max_obs) && njobs <= MAX_JOBS &&
           !product_over(njobs, max_local, max_ref, max_mp, max_obs) && launch_threads(max_local, max_ref, nullptr) != 0;
}

WsLayout ws_layout(int njobs, int max_local, int max_ref, int max_mp, int max_obs) {
    const size_t PK = (size_t)max_local + (size_t)max_ref, MO = (size_t)max_local, ML = (size_t)max_mp, ME = (size_t)max_obs;
    const size_t size[WS_REGIONS] = {
        4 * 8, PK, 8 * 3 * PK,                                   // counts, fixed, poses (the start values, kept)
        4 * MO, 4 * MO, 8 * 3 * MO, 8 * 9 * MO,                  // o_i, o_j, o_meas, o_info
        4 * (ML + 1), 4 * ME, 8 * 2 * ME, 8 * 3 * ME, 8 * 3 * ML,   // lm_ptr, e_kf, e_uv, e_info, landmarks (the start values, kept)
        8 * 3 * PK, 8 * 3 * ML, 8 * 3 * PK, 8 * 3 * ML,          // the solver's estimate / trial buffers "a" (starts as a copy) and "b"
        sizeof(BaCtl), 16 * ML + 44 * ME + 16, 8 * 6 * ML,       // BaCtl; desc and ainv as ba_resident_ok sizes them
        sizeof(WindowArgs)
    };
    WsLayout L;
    size_t at = 0;
    for (int i = 0; i < WS_REGIONS; ++i) {
        L.off[i] = at;
        L.stride[i] = (size[i] + 15) & ~(size_t)15;
        if (i == WS_PACK) L.stride[i] = sizeof(WindowArgs);   // the solver indexes the packs as an array
        at += (L.stride[i] * (size_t)njobs + 15) & ~(size_t)15;
    }
    L.bytes = at ? at : 16;
    return L;
}

struct Sigma2 {
    float v[32];
};

struct GatherArgs {
    int njobs, nframes, cap, m, nobs, nlevels, kf_list_cap, mp_list_cap, max_local, max_ref, max_mp, max_obs, iters, mode;
    const int* job_kf;
    const int* win_out;
    const int* local_list;
    const int* ref_list;
    const int* mp_list;
    const int* frame_id;
    const float* frame_Twb;
    const float* frame_Tcw;
    const uint8_t* frame_null;
    const int* odo_to;
    const double* odo_meas;
    const double* odo_cov;
    const se2gpu_keypoint* kps_un;
    const int* counts;
    const float* view_pos;
    const float* pos;
    const int* mp_ptr;
    const int* obs_frame;
    const int* obs_ftr;
    float fx, s_rot, s_z;
    Sigma2 sigma2;
    CamDev cam;
    char* ws;
    WsLayout lay;
    int* status;
};

struct JobArrays {
    int* cnt;
    uint8_t* fixed;
    double* poses;
    int* o_i;
    int* o_j;
    double* o_meas;
    double* o_info;
    int* lm_ptr;
    int* e_kf;
    double* e_uv;
    double* e_info;
    double* lms;
    double* poses_a;   // the solver's copies of poses / lms
    double* lms_a;
};
__device__ __forceinline__ char* ws_at(const GatherArgs& A, int region, int j) { return A.ws + A.lay.off[region] + A.lay.stride[region] * (size_t)j; }

// The points of a job, a wave per point at a time (Map.cpp:980-1051).  EMIT = false counts the edges of every point into lm_ptr[l + 1]
// and returns this thread's share of {edges, entries, largest degree, flags}; EMIT = true writes the edges behind lm_ptr[l].
template <bool EMIT>
__device__ __forceinline__ void point_pass(const GatherArgs& A, const FrameSlots& fs, const ObsCsr& csr, const int* s_vert, u64* bits,
                                           const int* mp_list, int n_mp, const JobArrays& J, long long& edges, long long& entries, int& maxdeg, int& flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int l = wave; l < n_mp; l += WAVES) {                    // uniform in the wave
        const int p = mp_list[l];                                  // in 0..m-1: the caller has checked the list
        int s, n;
        point_segment(csr, p, s, n);
        float lw[3] = {0, 0, 0};
        if (EMIT) {
#pragma unroll
            for (int k = 0; k < 3; ++k) lw[k] = A.pos[3 * (size_t)p + k];
            if (lane < 3) J.lms[3 * (size_t)l + lane] = J.lms_a[3 * (size_t)l + lane] = (double)lw[lane];
        }
        const int e0 = EMIT ? J.lm_ptr[l] : 0;
        int deg = 0;
        for (int base = 0; base < n; base += 64) {
            const bool active = base + lane < n;
            const int i = active ? s + base + lane : s;            // n > 0: s names an entry
            const int f = csr.obs_frame[i], k = csr.obs_ftr[i];
            const bool valid = active && entry_valid(fs, f, k);    // null observers are skipped (:995)
            const int v = valid ? s_vert[f] : -1;                  // a member of either list (:1011-1022)
            bool first = v >= 0;
            const int nq = min(n - base, 64) - 1;                  // uniform: the lanes below the chunk's last entry
            for (int q = 0; q < nq; ++q) {                         // the first entry of a frame inside the chunk
                const int vq = __shfl(v, q);
                if (q < lane && vq == v) first = false;
            }
            if (first) {                                           // ... and in the chunks before it
                const u64 bit = 1ull << (v & 63);
                first = !(atomicOr(&bits[v >> 6], bit) & bit);
            }
            int oct = 0;
            size_t fo = 0;
            if (first) {
                fo = (size_t)f * fs.cap + k;
                oct = A.kps_un[fo].octave;
            }
            const bool okoct = oct >= 0 && oct < A.nlevels;
            if (first && !okoct) flags |= FLAG_OCTAVE;
            const bool edge = first && okoct;
            const u64 mask = __ballot(edge);
            if (EMIT && edge) {
                const size_t at = (size_t)e0 + deg + lane_rank(mask);
                const se2gpu_keypoint kp = A.kps_un[fo];
                J.e_kf[at] = v;
                J.e_uv[2 * at] = (double)kp.x; J.e_uv[2 * at + 1] = (double)kp.y;
                double R[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)A.frame_Tcw[12 * (size_t)f + 4 * r + c];
                const double d0 = (double)lw[0] - (double)A.frame_Twb[3 * (size_t)f], d1 = (double)lw[1] - (double)A.frame_Twb[3 * (size_t)f + 1];
                double xx, xy, yy;
                edge_information((double)A.view_pos[3 * fo], (double)A.view_pos[3 * fo + 1], (double)A.view_pos[3 * fo + 2], R, d0, d1,
                                 (double)lw[2], (double)A.sigma2.v[oct], A.fx, A.s_rot, A.s_z, xx, xy, yy);
                J.e_info[3 * at] = xx; J.e_info[3 * at + 1] = xy; J.e_info[3 * at + 2] = yy;
            }
            deg += __popcll(mask);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        atomicExch(&bits[lane], 0ull);                             // the row is empty again for the wave's next point
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane == 0) {
            if (!EMIT) J.lm_ptr[l + 1] = deg;
            edges += deg; entries += n; maxdeg = max(maxdeg, deg);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_local_ba_gather(const GatherArgs A) {
    __shared__ int s_vert[MAX_FRAMES];
    __shared__ u64 s_bits[WAVES][VERT_WORDS];
    __shared__ int s_w[WAVES], s_red[4][WAVES], s_minid;   // (s_red[1] is unused)
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (j >= A.njobs) return;
    JobArrays J;
    J.cnt = (int*)ws_at(A, WS_CNT, j); J.fixed = (uint8_t*)ws_at(A, WS_FIXED, j); J.poses = (double*)ws_at(A, WS_POSES, j);
    J.o_i = (int*)ws_at(A, WS_OI, j); J.o_j = (int*)ws_at(A, WS_OJ, j); J.o_meas = (double*)ws_at(A, WS_OMEAS, j);
    J.o_info = (double*)ws_at(A, WS_OINFO, j); J.lm_ptr = (int*)ws_at(A, WS_LMPTR, j); J.e_kf = (int*)ws_at(A, WS_EKF, j);
    J.e_uv = (double*)ws_at(A, WS_EUV, j); J.e_info = (double*)ws_at(A, WS_EINFO, j); J.lms = (double*)ws_at(A, WS_LMS, j);
    J.poses_a = (double*)ws_at(A, WS_POSESA, j); J.lms_a = (double*)ws_at(A, WS_LMSA, j);
    const int nframes = A.nframes;
    const int* w = A.win_out + 4 * (size_t)j;
    const int n_local = w[0], n_ref = max(w[1], 0), n_mp = max(w[2], 0);
    // what a job that is not gathered leaves: its status and its counts
    auto leave = [&](int status, int n_pose, int n_free, int n_lm, int n_edge, int n_odo, int skipped, int flags) {
        if (tid == 0) {
            A.status[j] = status;
            J.cnt[0] = n_pose; J.cnt[1] = n_free; J.cnt[2] = n_lm; J.cnt[3] = n_edge; J.cnt[4] = n_odo; J.cnt[5] = skipped; J.cnt[6] = flags;
            J.cnt[7] = 0;
        }
    };
    if ((unsigned)A.job_kf[j] >= (unsigned)nframes || n_local < 0) { leave(ST_RANGE, 0, 0, 0, 0, 0, 0, 0); return; }   // uniform
    if (n_local > min(A.kf_list_cap, A.max_local) || n_ref > min(A.kf_list_cap, A.max_ref) || n_mp > min(A.mp_list_cap, A.max_mp)) {
        leave(ST_FIT, 0, 0, 0, 0, 0, 0, 0);
        return;
    }
    const int* local_list = A.local_list + (size_t)j * A.kf_list_cap;
    const int* ref_list = A.ref_list + (size_t)j * A.kf_list_cap;
    const int* mp_list = A.mp_list + (size_t)j * A.mp_list_cap;
    const int P = n_local + n_ref;
    // the lists name slots and points of the tables, or the job is left as one out of range
    {
        bool bad = false;
        for (int i = tid; i < P; i += BLOCK) bad |= (unsigned)(i < n_local ? local_list[i] : ref_list[i - n_local]) >= (unsigned)nframes;
        for (int i = tid; i < n_mp; i += BLOCK) bad |= (unsigned)mp_list[i] >= (unsigned)A.m;
        if (__syncthreads_or(bad)) { leave(ST_RANGE, 0, 0, 0, 0, 0, 0, 0); return; }
    }
    // slot -> vertex: local key frame i -> i, reference key frame i -> n_local + i (:925, :966)
    for (int f = tid; f < nframes; f += BLOCK) s_vert[f] = -1;
    if (tid < VERT_WORDS) {
#pragma unroll
        for (int v = 0; v < WAVES; ++v) s_bits[v][tid] = 0;
    }
    if (tid == 0) s_minid = INT_MAX;
    __syncthreads();
    for (int i = tid; i < P; i += BLOCK) s_vert[i < n_local ? local_list[i] : ref_list[i - n_local]] = i;
    __syncthreads();
    // the local key frames: null members, the least id (:903-912), the odometry edges that exist (:942-946)
    int has_null = 0, self_loop = 0, minid = INT_MAX;
    for (int i = tid; i < n_local; i += BLOCK) {
        const int slot = local_list[i];
        has_null |= A.frame_null && A.frame_null[slot];
        minid = min(minid, A.frame_id[slot]);
        self_loop |= A.odo_to && A.odo_to[slot] == slot;
    }
    minid = wave_min(minid);
    if (lane == 0) atomicMin(&s_minid, minid);
    has_null = __syncthreads_or(has_null);
    self_loop = __syncthreads_or(self_loop);
    minid = n_ref == 0 ? s_minid : -1;                            // (:899: -1 names no key frame; ids start at 0)
    const bool fix_min = n_ref == 0;
    int n_free = 0;
    for (int i = tid; i < n_local; i += BLOCK) {
        const int id = A.frame_id[local_list[i]];
        n_free += !((fix_min && id == minid) || id == 1);
    }
    FrameSlots fs;
    fs.counts = A.counts; fs.frame_null = A.frame_null; fs.cap = A.cap; fs.nframes = nframes;
    ObsCsr csr;
    csr.mp_ptr = A.mp_ptr; csr.obs_frame = A.obs_frame; csr.obs_ftr = A.obs_ftr; csr.m = A.m; csr.nobs = A.nobs;
    long long edges = 0, entries = 0;
    int maxdeg = 0, flags = 0;
    point_pass<false>(A, fs, csr, s_vert, s_bits[wave], mp_list, n_mp, J, edges, entries, maxdeg, flags);
    // the sums over the workgroup (a job of two billion entries saturates nothing: nobs <= 2^31 - 1 and a point's segment lies inside it,
    // but the sum over the points is taken in 64 bits below)
    n_free = wave_sum(n_free);
    flags = __ballot(flags != 0) != 0ull ? FLAG_OCTAVE : 0;         // (the one flag there is)
    __shared__ long long s_ent[WAVES], s_edges64[WAVES];
    if (lane == 0) {                                               // (lane 0 holds the wave's edges, entries and largest degree)
        s_red[0][wave] = n_free; s_red[2][wave] = maxdeg; s_red[3][wave] = flags;
        s_ent[wave] = entries; s_edges64[wave] = edges;
    }
    __syncthreads();
    long long E64 = 0, ENT = 0;
    n_free = 0; maxdeg = 0; flags = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) {
        n_free += s_red[0][v]; E64 += s_edges64[v]; ENT += s_ent[v];
        maxdeg = max(maxdeg, s_red[2][v]); flags |= s_red[3][v];
    }
    const int skipped = (int)min(ENT - E64, (long long)INT_MAX);
    const int E = (int)min(E64, (long long)INT_MAX);
    // the PreSE2 edges: local key frame i -> the vertex of preOdomFromSelf.first, when that is a local member and not null (:944-946)
    auto odo_target = [&](int i) -> int {
        if (!A.odo_to || i >= n_local) return -1;
        const int t = A.odo_to[local_list[i]];
        if ((unsigned)t >= (unsigned)nframes) return -1;
        const int v = s_vert[t];
        if (v < 0 || v >= n_local) return -1;
        if (A.frame_null && A.frame_null[t]) return -1;
        return v;
    };
    int O = 0;
    for (int i = tid; i < n_local; i += BLOCK) O += odo_target(i) >= 0;
    O = wave_sum(O);
    __syncthreads();
    if (lane == 0) s_w[wave] = O;
    __syncthreads();
    O = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) O += s_w[v];

    int status = ST_OK;
    if (E64 > A.max_obs || n_free > MAX_FREE || self_loop) status = ST_FIT;
    else if (has_null) status = ST_NULL;
    else if (maxdeg > kWindowMaxDegree) status = ST_DEGREE;
    else if (n_free == 0 || E + O == 0) status = ST_EMPTY;
    leave(status, P, n_free, n_mp, E, O, skipped, flags);
    if (status != ST_OK && status != ST_EMPTY) return;            // uniform

    // ---- the graph
    for (int i = tid; i < P; i += BLOCK) {
        const int slot = i < n_local ? local_list[i] : ref_list[i - n_local];
        const int id = A.frame_id[slot];
        J.fixed[i] = i >= n_local || (fix_min && id == minid) || id == 1;                 // :927, :969
        const double x = (double)A.frame_Twb[3 * (size_t)slot], y = (double)A.frame_Twb[3 * (size_t)slot + 1];
        const double th = badev::normalize_theta((double)A.frame_Twb[3 * (size_t)slot + 2]);   // g2o::SE2's constructor (:929)
        J.poses[3 * (size_t)i] = J.poses_a[3 * (size_t)i] = x;
        J.poses[3 * (size_t)i + 1] = J.poses_a[3 * (size_t)i + 1] = y;
        J.poses[3 * (size_t)i + 2] = J.poses_a[3 * (size_t)i + 2] = th;
    }
    for (int i0 = 0, base = 0; i0 < n_local; i0 += BLOCK) {       // uniform
        const int i = i0 + tid;
        const int v = odo_target(i);
        int total;
        const int at = base + block_scan_excl<WAVES>((int)(v >= 0), s_w, total);
        base += total;
        if (v >= 0) {
            const int slot = local_list[i];
            J.o_i[at] = i; J.o_j[at] = v;
#pragma unroll
            for (int k = 0; k < 3; ++k) J.o_meas[3 * (size_t)at + k] = A.odo_meas[3 * (size_t)slot + k];
            const double* c = A.odo_cov + 9 * (size_t)slot;       // info = cov^-1 (Eigen's closed-form 3x3 inverse: cofactors / det), :951-952
            const double Ac = c[4] * c[8] - c[5] * c[7], Bc = -(c[3] * c[8] - c[5] * c[6]), Cc = c[3] * c[7] - c[4] * c[6];
            const double id = 1.0 / (c[0] * Ac + c[1] * Bc + c[2] * Cc);
            double* o = J.o_info + 9 * (size_t)at;
            o[0] = Ac * id; o[1] = -(c[1] * c[8] - c[2] * c[7]) * id; o[2] = (c[1] * c[5] - c[2] * c[4]) * id;
            o[3] = Bc * id; o[4] = (c[0] * c[8] - c[2] * c[6]) * id; o[5] = -(c[0] * c[5] - c[2] * c[3]) * id;
            o[6] = Cc * id; o[7] = -(c[0] * c[7] - c[1] * c[6]) * id; o[8] = (c[0] * c[4] - c[1] * c[3]) * id;
        }
    }
    // lm_ptr: the counts the first pass left in lm_ptr[1..n_mp] become their prefix sums
    __syncthreads();
    for (int l0 = 0, base = 0; l0 < n_mp; l0 += BLOCK) {          // uniform
        const int l = l0 + tid;
        const int c = l < n_mp ? J.lm_ptr[l + 1] : 0;
        int total;
        const int at = base + block_scan_excl<WAVES>(c, s_w, total);
        base += total;
        if (l < n_mp) J.lm_ptr[l + 1] = at + c;
    }
    if (tid == 0) J.lm_ptr[0] = 0;
    __syncthreads();
    point_pass<true>(A, fs, csr, s_vert, s_bits[wave], mp_list, n_mp, J, edges, entries, maxdeg, flags);
    // a zeroed controller block and the window's pack
    {
        double* ctl = (double*)ws_at(A, WS_CTL, j);
        for (int i = tid; i < (int)(sizeof(BaCtl) / 8); i += BLOCK) ctl[i] = 0.0;
    }
    if (tid == 0) {
        WindowArgs a;
        a.P = P; a.L = n_mp; a.E = E; a.O = O; a.iters = A.iters; a.mode = A.mode;
        a.lm_ptr = J.lm_ptr; a.e_kf = J.e_kf; a.e_uv = J.e_uv; a.e_info = J.e_info;
        a.poses_a = J.poses_a; a.poses_b = (double*)ws_at(A, WS_POSESB, j);
        a.lms_a = J.lms_a; a.lms_b = (double*)ws_at(A, WS_LMSB, j);
        a.fixed = J.fixed;
        a.o_i = J.o_i; a.o_j = J.o_j; a.o_meas = J.o_meas; a.o_info = J.o_info;
        a.ctl = (BaCtl*)ws_at(A, WS_CTL, j);
        a.mail = nullptr; a.stop = nullptr; a.stamps = nullptr;
        a.desc = (int4*)ws_at(A, WS_DESC, j);
        a.ainv = (double*)ws_at(A, WS_AINV, j);
        a.cam = A.cam;
        *(WindowArgs*)ws_at(A, WS_PACK, j) = a;
    }
}

struct FinishArgs {
    int njobs, max_pose, max_mp;
    const char* ws;
    WsLayout lay;
    int* status;
    double* kf_out;
    double* mp_out;
    se2gpu_ba_stats* stats;
    int* info;
};

__global__ __launch_bounds__(64) void k_local_ba_finish(const FinishArgs A) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= A.njobs) return;
    auto at = [&](int region) { return A.ws + A.lay.off[region] + A.lay.stride[region] * (size_t)j; };
    int status = A.status[j];
    const int* cnt = (const int*)at(WS_CNT);
    const BaCtl* ctl = (const BaCtl*)at(WS_CTL);
    const bool ran = status == ST_OK;
    if (ran || status == ST_EMPTY) {
        const int P = cnt[0], L = cnt[2];
        const int sel = ran ? ctl->sel : 0;                        // a window that is not run keeps its start values
        const double* poses = (const double*)at(sel ? WS_POSESB : WS_POSESA);
        const double* lms = (const double*)at(sel ? WS_LMSB : WS_LMSA);
        double* kf = A.kf_out + 3 * (size_t)j * A.max_pose;
        double* mp = A.mp_out + 3 * (size_t)j * A.max_mp;
        bool fin = true;
        for (int i = lane; i < 3 * P; i += 64) { const double v = poses[i]; fin = fin && isfinite(v); kf[i] = v; }
        for (int i = lane; i < 3 * L; i += 64) { const double v = lms[i]; fin = fin && isfinite(v); mp[i] = v; }
        if (__ballot(!fin) != 0ull) status = ST_NONFINITE;
    }
    if (A.stats) {
        se2gpu_ba_stats* s = A.stats + j;
        if (lane == 0) {
            s->iterations = ran ? ctl->it : 0;
            s->trials = ran ? ctl->trials : 0;
            s->terminated = ran ? ctl->terminated : 0;
            s->stopped = ran ? ctl->stopped : 0;
            s->chi2_init = ran ? ctl->chi2_init : 0.0;
            s->chi2_final = ran ? ctl->chi2_final : 0.0;
            s->lambda_final = ran ? ctl->lambda : 0.0;
        }
        s->chi2_hist[lane] = ran ? ctl->chi2_hist[lane] : 0.0;
        s->lambda_hist[lane] = ran ? ctl->lambda_hist[lane] : 0.0;
        s->trials_hist[lane] = ran ? ctl->trials_hist[lane] : 0;
    }
    if (lane < 8) A.info[8 * (size_t)j + lane] = lane < 7 ? cnt[lane] : 0;
    if (lane == 0) A.status[j] = status;
}

}  // namespace

extern "C" {

long long se2gpu_local_ba_ws_bytes(int njobs, int max_local, int max_ref, int max_mp, int max_obs) {
    if (!ws_args_ok(njobs, max_local, max_ref, max_mp, max_obs)) return -1;
    return (long long)ws_layout(njobs, max_local, max_ref, max_mp, max_obs).bytes;
}

int se2gpu_local_ba_ws_layout(int njobs, int max_local, int max_ref, int max_mp, int max_obs, long long* offsets, long long* strides, int n) {
    SE2_REQUIRE(ws_args_ok(njobs, max_local, max_ref, max_mp, max_obs), SE2GPU_ERR_INVALID,
                "local_ba_ws_layout: njobs = %d, max_local = %d, max_ref = %d, max_mp = %d, max_obs = %d", njobs, max_local, max_ref, max_mp, max_obs);
    SE2_REQUIRE(offsets && strides && n >= SE2GPU_LOCAL_BA_WS_ARRAYS, SE2GPU_ERR_INVALID, "local_ba_ws_layout: %d offsets and strides are written",
                SE2GPU_LOCAL_BA_WS_ARRAYS);
    const WsLayout L = ws_layout(njobs, max_local, max_ref, max_mp, max_obs);
    for (int i = 0; i < SE2GPU_LOCAL_BA_WS_ARRAYS; ++i) { offsets[i] = (long long)L.off[i]; strides[i] = (long long)L.stride[i]; }
    return SE2GPU_OK;
}

int se2gpu_local_ba_batch_device(se2gpu_matcher* h, const int32_t* d_job_kf, int njobs, const int32_t* d_win_out,
                                 const int32_t* d_local_list, const int32_t* d_ref_list, int kf_list_cap, const int32_t* d_mp_list,
                                 int mp_list_cap, int nframes, const int32_t* d_frame_id, const float* d_frame_Twb,
                                 const float* d_frame_Tcw, const uint8_t* d_frame_null, const int32_t* d_odo_to,
                                 const double* d_odo_meas, const double* d_odo_cov, const se2gpu_keypoint* d_kps_un,
                                 const int32_t* d_counts, int cap, const float* d_view_pos, const float* level_sigma2, int nlevels,
                                 const float* d_pos, int m, const int32_t* d_mp_ptr, const int32_t* d_obs_frame,
                                 const int32_t* d_obs_ftr, int nobs, float fx, float cx, float cy, const double* Tbc12,
                                 double huber_delta, double xrot_info, double z_info, int iters, int mode, int max_local, int max_ref,
                                 int max_mp, int max_obs, void* d_ws, int32_t* d_status, double* d_kf_out, double* d_mp_out,
                                 se2gpu_ba_stats* d_stats, int32_t* d_info) {
    const char* who = "local_ba_batch_device";
    // every refusal comes before the first use of the handle or a device
    SE2_NEED(h);
    SE2_NEED(d_job_kf); SE2_NEED(d_win_out); SE2_NEED(d_local_list); SE2_NEED(d_ref_list); SE2_NEED(d_mp_list);
    SE2_NEED(d_frame_id); SE2_NEED(d_frame_Twb); SE2_NEED(d_frame_Tcw);
    SE2_NEED(d_kps_un); SE2_NEED(d_counts); SE2_NEED(d_view_pos); SE2_NEED(level_sigma2);
    SE2_NEED(d_pos); SE2_NEED(d_mp_ptr); SE2_NEED(d_obs_frame); SE2_NEED(d_obs_ftr); SE2_NEED(Tbc12);
    SE2_NEED(d_ws); SE2_NEED(d_status); SE2_NEED(d_kf_out); SE2_NEED(d_mp_out); SE2_NEED(d_info);
    SE2_REQUIRE(!d_odo_to == !d_odo_meas && !d_odo_to == !d_odo_cov, SE2GPU_ERR_INVALID,
                "%s: d_odo_to, d_odo_meas and d_odo_cov are given together or not at all", who);
    SE2_REQUIRE(((uintptr_t)d_ws & 15) == 0, SE2GPU_ERR_INVALID, "%s: d_ws is not 16-byte aligned", who);
    SE2_REQUIRE(njobs >= 0, SE2GPU_ERR_INVALID, "%s: njobs = %d is negative", who, njobs);
    SE2_REQUIRE(nframes >= 1, SE2GPU_ERR_INVALID, "%s: nframes = %d", who, nframes);
    SE2_REQUIRE(m >= 0, SE2GPU_ERR_INVALID, "%s: m = %d is negative", who, m);
    SE2_REQUIRE(nobs >= 0, SE2GPU_ERR_INVALID, "%s: nobs = %d is negative", who, nobs);
    SE2_REQUIRE(cap >= 1, SE2GPU_ERR_INVALID, "%s: cap = %d", who, cap);
    SE2_REQUIRE(kf_list_cap >= 1, SE2GPU_ERR_INVALID, "%s: kf_list_cap = %d", who, kf_list_cap);
    SE2_REQUIRE(mp_list_cap >= 1, SE2GPU_ERR_INVALID, "%s: mp_list_cap = %d", who, mp_list_cap);
    SE2_REQUIRE(max_local >= 1, SE2GPU_ERR_INVALID, "%s: max_local = %d", who, max_local);
    SE2_REQUIRE(max_ref >= 1, SE2GPU_ERR_INVALID, "%s: max_ref = %d", who, max_ref);
    SE2_REQUIRE(max_mp >= 1, SE2GPU_ERR_INVALID, "%s: max_mp = %d", who, max_mp);
    SE2_REQUIRE(max_obs >= 1, SE2GPU_ERR_INVALID, "%s: max_obs = %d", who, max_obs);
    SE2_REQUIRE(iters >= 1 && iters <= 64, SE2GPU_ERR_INVALID, "%s: iters = %d (1..64, the length of the se2gpu_ba_stats histories)", who, iters);
    SE2_REQUIRE(nlevels >= 1 && nlevels <= 32, SE2GPU_ERR_INVALID, "%s: nlevels = %d (1..32)", who, nlevels);
    SE2_REQUIRE(mode == SE2GPU_BA_LM || mode == SE2GPU_BA_GN, SE2GPU_ERR_INVALID, "%s: mode %d", who, mode);
    SE2_REQUIRE(nframes <= MAX_FRAMES, SE2GPU_ERR_CAPACITY, "%s: nframes = %d exceeds the limit %d", who, nframes, MAX_FRAMES);
    SE2_REQUIRE(njobs <= MAX_JOBS, SE2GPU_ERR_CAPACITY, "%s: njobs = %d exceeds the limit %d", who, njobs, MAX_JOBS);
    SE2_REQUIRE((long long)nframes * cap * 3 <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: nframes * cap * 3 = %lld exceeds 2^31 - 1", who,
                (long long)nframes * cap * 3);
    SE2_REQUIRE((long long)m * 3 <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: m * 3 = %lld exceeds 2^31 - 1", who, (long long)m * 3);
    SE2_REQUIRE((long long)njobs * kf_list_cap <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: njobs * kf_list_cap = %lld exceeds 2^31 - 1", who,
                (long long)njobs * kf_list_cap);
    SE2_REQUIRE((long long)njobs * mp_list_cap <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: njobs * mp_list_cap = %lld exceeds 2^31 - 1", who,
                (long long)njobs * mp_list_cap);
    {
        const char* over = product_over(njobs, max_local, max_ref, max_mp, max_obs);
        SE2_REQUIRE(!over, SE2GPU_ERR_CAPACITY, "%s: %s exceeds its limit", who, over ? over : "");
    }
    size_t lds = 0;
    const int threads = launch_threads(max_local, max_ref, &lds);
    SE2_REQUIRE(threads != 0, SE2GPU_ERR_CAPACITY,
                "%s: a window of max_local + max_ref = %d key frames, min(max_local, 64) = %d of them free, fits no launch width", who,
                max_local + max_ref, std::min(max_local, MAX_FREE));
    if (njobs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();

    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    GatherArgs g;
    g.njobs = njobs; g.nframes = nframes; g.cap = cap; g.m = m; g.nobs = nobs; g.nlevels = nlevels;
    g.kf_list_cap = kf_list_cap; g.mp_list_cap = mp_list_cap;
    g.max_local = max_local; g.max_ref = max_ref; g.max_mp = max_mp; g.max_obs = max_obs; g.iters = iters; g.mode = mode;
    g.job_kf = d_job_kf; g.win_out = d_win_out; g.local_list = d_local_list; g.ref_list = d_ref_list; g.mp_list = d_mp_list;
    g.frame_id = d_frame_id; g.frame_Twb = d_frame_Twb; g.frame_Tcw = d_frame_Tcw; g.frame_null = d_frame_null;
    g.odo_to = d_odo_to; g.odo_meas = d_odo_meas; g.odo_cov = d_odo_cov;
    g.kps_un = d_kps_un; g.counts = d_counts; g.view_pos = d_view_pos; g.pos = d_pos;
    g.mp_ptr = d_mp_ptr; g.obs_frame = d_obs_frame; g.obs_ftr = d_obs_ftr;
    g.fx = fx;
    g.s_rot = (float)(1. / xrot_info);    // float Sigma_rotxy = 1. / Config::PLANEMOTION_XROT_INFO (:1043-1044)
    g.s_z = (float)(1. / z_info);
    for (int i = 0; i < 32; ++i) g.sigma2.v[i] = i < nlevels ? level_sigma2[i] : 0.f;
    // addCamPara and setExtParameter as se2gpu_ba_initialize applies them: Tcb = Tbc^-1
    g.cam.fx = fx; g.cam.cx = cx; g.cam.cy = cy; g.cam.huber = huber_delta;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) g.cam.Rcb[i * 3 + k] = Tbc12[k * 3 + i];
    for (int i = 0; i < 3; ++i)
        g.cam.tcb[i] = -(g.cam.Rcb[i * 3] * Tbc12[9] + g.cam.Rcb[i * 3 + 1] * Tbc12[10] + g.cam.Rcb[i * 3 + 2] * Tbc12[11]);
    g.ws = (char*)d_ws;
    g.lay = ws_layout(njobs, max_local, max_ref, max_mp, max_obs);
    g.status = d_status;
    hipLaunchKernelGGL(k_local_ba_gather, dim3(njobs), dim3(BLOCK), 0, st, g);
    SE2_HIP(hipGetLastError());

    SE2_CHECK(ba_window_launch_status((const WindowArgs*)(g.ws + g.lay.off[WS_PACK]), d_status, njobs, threads, lds, st));

    FinishArgs f;
    f.njobs = njobs; f.max_pose = max_local + max_ref; f.max_mp = max_mp;
    f.ws = g.ws; f.lay = g.lay; f.status = d_status; f.kf_out = d_kf_out; f.mp_out = d_mp_out; f.stats = d_stats; f.info = d_info;
    hipLaunchKernelGGL(k_local_ba_finish, dim3(njobs), dim3(64), 0, st, f);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // extern "C"
