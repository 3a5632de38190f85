// libse2gpu - the localisation mode's pose-only bundle adjustment on the tables where they lie in device memory:
// se2gpu_localizer_ba_batch_device.  Localizer::run (src/Localizer.cpp:32-176 of the reference) does, per frame, MatchLocalMap ->
// DoLocalBA -> UpdateCovisKFCurr -> UpdateLocalMap; this call is the second link for a batch of frames: the observation renewal
// of MatchLocalMap (:220-227), the numMPCurr > 30 gate (:95-98), DoLocalBA (:233-302) with addPlaneMotionSE3Expmap
// (optimizer.cpp:236-314) and KeyFrame::setPose (:298-299), on the frame, feature and point tables.
//   k_localizer_ba   one workgroup of 256 threads per job, ONE launch:
//     renewal   a thread per feature: the match row's point into d_ftr_mp / d_kf_observed; the row's points (or -1) go into
//               the job's work space
//     distinct  a point named by several features keeps the greatest feature index: the row is staged in LDS (4096 entries at
//               a time) and every feature looks for its point among the features behind it (128-bit LDS reads)
//     gather    the edges in ascending feature index: places from ballots and a prefix sum over the workgroup, no atomic
//               counter; e_ftr, xyz, uv, w into the job's slice of the work space
//     prior     a lane of the last wave, beside the renewal: the start pose through a unit quaternion (toSE3Quat) and
//               plane_motion_prior_se3 (se3_math.h) of it
//     solve     pose_ba_run (pose_ba_device.h), the arithmetic of k_pose_ba, on the gathered arrays
//     write-back  thread 0: d_frame_Tcw / d_frame_Twb of the job's frame
// Asynchronous on the matcher's stream; nothing is allocated, uploaded besides kernel arguments, read back or waited for.
// Compiled with -ffp-contract=off (se2lam_amd/build.py): the gathered values and the prior are sums and products rounded one by
// one; pose_ba.hip keeps the default, so the two solvers agree to rounding, not to the bit.
#include <algorithm>

#include "common.h"
#include "pose_ba_device.h"
#include "wave_int.h"

using namespace se2gpu;

namespace {

constexpr int MAX_JOBS = 65535;
constexpr int BLOCK = kPoseBaThreads, WAVES = BLOCK / 64;
constexpr int CHUNK = 4096;           // features of a row staged in LDS at a time (16 KiB)

enum { ST_OK = 0, ST_RANGE = 1, ST_GATE = 5, ST_NONFINITE = 6 };
enum { FLAG_ENTRY = 1, FLAG_OCTAVE = 2 };   // d_info[5]: a d_ftr_mp value outside -1..m-1; an octave outside 0..nlevels-1

// d_ws: the regions in this order; a job's slice of a region starts at a multiple of 16 bytes
enum { WS_CNT, WS_POSE0, WS_PMEAS, WS_PINFO, WS_EFTR, WS_XYZ, WS_UV, WS_W,   // se2gpu_localizer_ba_ws_layout
       WS_PT, WS_STATS, WS_REGIONS };
struct WsLayout {
    size_t off[WS_REGIONS], stride[WS_REGIONS];
    size_t bytes;
};

bool ws_args_ok(int njobs, int cap) {
    return njobs >= 0 && cap >= 1 && njobs <= MAX_JOBS && (long long)njobs * cap * 3 <= 2147483647LL;
}

WsLayout ws_layout(int njobs, int cap) {
    const size_t C = (size_t)cap;
    const size_t size[WS_REGIONS] = {4 * 8, 8 * 12, 8 * 12, 8 * 36, 4 * C, 8 * 3 * C, 8 * 2 * C, 8 * C,
                                     4 * C, sizeof(se2gpu_ba_stats)};   // the row's points; statistics of a job without d_stats
    WsLayout L;
    size_t at = 0;
    for (int i = 0; i < WS_REGIONS; ++i) {
        L.off[i] = at;
        L.stride[i] = (size[i] + 15) & ~(size_t)15;
        at += L.stride[i] * (size_t)njobs;
    }
    L.bytes = at ? at : 16;
    return L;
}

struct InvSigma2 {
    float v[32];
};

struct LocArgs {
    int njobs, nframes, cap, m, nlevels, iters, min_obs;
    const int* job_frame;
    float* frame_Tcw;
    float* frame_Twb;
    const se2gpu_keypoint* kps_un;
    const int* counts;
    int* ftr_mp;
    uint8_t* kf_observed;
    const int* match;
    const float* pos;
    const uint8_t* mp_null;
    const uint8_t* good_prl;
    InvSigma2 isig;
    double f, cx, cy, delta, xrot, yrot, z;
    double Tbc[12], Tcb[12];          // Config::bTc and its inverse (pose12)
    char* ws;
    WsLayout lay;
    int* status;
    double* pose_out;
    se2gpu_ba_stats* stats;
    int* info;
};

__global__ __launch_bounds__(BLOCK) void k_localizer_ba(const LocArgs A) {
    __shared__ __align__(16) int s_pt[CHUNK];                      // read as int4
    __shared__ float s_sig[32];
    __shared__ int s_w[WAVES], s_red[4][WAVES];
    __shared__ PoseParams s_P;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (b >= A.njobs) return;
    auto at = [&](int region) { return A.ws + A.lay.off[region] + A.lay.stride[region] * (size_t)b; };
    int* cnt = (int*)at(WS_CNT);
    se2gpu_ba_stats* stats = A.stats ? A.stats + b : (se2gpu_ba_stats*)at(WS_STATS);
    for (int i = tid; i < (int)(sizeof(se2gpu_ba_stats) / 4); i += BLOCK) ((int*)stats)[i] = 0;
    const int frame = A.job_frame[b];
    if ((unsigned)frame >= (unsigned)A.nframes) {                  // uniform
        if (tid < 8) { cnt[tid] = 0; A.info[8 * (size_t)b + tid] = 0; }
        if (tid == 0) A.status[b] = ST_RANGE;
        return;
    }
    const int cap = A.cap, m = A.m;
    const int n = max(min(A.counts[frame], cap), 0);
    const size_t row = (size_t)frame * cap;
    int* ftr = A.ftr_mp + row;
    int* pt = (int*)at(WS_PT);
    if (tid < 32) s_sig[tid] = A.isig.v[tid];

    // ---- the start pose and its prior, by a lane of the last wave
    if (tid == BLOCK - 64) {
        const float* T = A.frame_Tcw + 12 * (size_t)frame;
        double R[9], q[4], p0[12], meas[12], info[36];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)T[4 * r + c];
            p0[9 + r] = (double)T[4 * r + 3];
        }
        quat_of(R, q);                                             // SE3Quat(R, t): Eigen's quaternion of R, w >= 0, normalised
        mat_of_quat(q, p0);
        plane_motion_prior_se3(p0, A.Tbc, A.xrot, A.yrot, A.z, meas, info);
        double* w0 = (double*)at(WS_POSE0);
        double* w1 = (double*)at(WS_PMEAS);
        double* w2 = (double*)at(WS_PINFO);
#pragma unroll
        for (int i = 0; i < 12; ++i) { w0[i] = p0[i]; w1[i] = meas[i]; }
#pragma unroll
        for (int i = 0; i < 36; ++i) { w2[i] = info[i]; s_P.info[i] = info[i]; }
        s_P.est0 = se3_load(p0);
        s_P.prior = se3_load(meas);
        s_P.f = A.f; s_P.cx = A.cx; s_P.cy = A.cy; s_P.delta = A.delta;
        s_P.iters = A.iters;
    }

    // ---- renewal (:220-227) and the row's points: pt[j] = the point of feature j, or -1
    int renewed = 0, flags = 0;
    for (int j = tid; j < n; j += BLOCK) {
        int v = ftr[j];
        if (A.match) {
            const int q = A.match[(size_t)b * cap + j];
            if ((unsigned)q < (unsigned)m && !(A.mp_null && A.mp_null[q])) {   // addObservation returns on a null point
                v = q;
                ftr[j] = q;
                if (A.kf_observed) A.kf_observed[row + j] = 1;
                ++renewed;
            }
        }
        if ((unsigned)v < (unsigned)m) pt[j] = v;
        else { pt[j] = -1; if (v != -1) flags |= FLAG_ENTRY; }
    }
    __syncthreads();

    // ---- a point named by several features keeps the greatest: pt[j] = -2 where a feature behind j names the same point
    int dups = 0;
    for (int c0 = 0; c0 < n; c0 += CHUNK) {                         // uniform
        const int cn = min(n - c0, CHUNK);
        for (int i = tid; i < cn; i += BLOCK) s_pt[i] = pt[c0 + i];
        __syncthreads();
        for (int j = tid; j < c0 + cn; j += BLOCK) {
            const int p = j >= c0 ? s_pt[j - c0] : pt[j];
            if (p < 0) continue;
            int i = max(j + 1 - c0, 0);
            bool dup = false;
            for (; i < cn && (i & 3); ++i) dup |= s_pt[i] == p;
            for (; i + 4 <= cn; i += 4) {
                const int4 v = *(const int4*)&s_pt[i];
                dup |= (v.x == p) | (v.y == p) | (v.z == p) | (v.w == p);
            }
            for (; i < cn; ++i) dup |= s_pt[i] == p;
            if (dup) { pt[j] = -2; ++dups; }
        }
        __syncthreads();
    }

    // ---- the edges (:261-288) in ascending feature index
    int* e_ftr = (int*)at(WS_EFTR);
    double* xyz = (double*)at(WS_XYZ);
    double* uv = (double*)at(WS_UV);
    double* w = (double*)at(WS_W);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int n_obs = 0, E = 0;
    for (int base = 0; base < n; base += BLOCK) {                   // uniform
        const int j = base + tid;                                   // the thread that wrote pt[j]
        bool edge = false;
        int p = -1, oct = 0;
        se2gpu_keypoint kp;
        if (j < n) {
            p = pt[j];
            if (p >= 0) {
                ++n_obs;                                            // getSizeObsMP(): null and bad-parallax points count
                if (!(A.mp_null && A.mp_null[p]) && !(A.good_prl && !A.good_prl[p])) {
                    kp = A.kps_un[row + j];
                    oct = kp.octave;
                    if ((unsigned)oct < (unsigned)A.nlevels) edge = true;
                    else flags |= FLAG_OCTAVE;
                }
            }
        }
        const unsigned long long mask = __ballot(edge);
        __syncthreads();                                            // (s_w may still be read from the round before)
        if (lane == 0) s_w[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) {
            const int c = s_w[v];
            if (v < wave) before += c;
            total += c;
        }
        if (edge) {
            const size_t e = (size_t)E + before + __popcll(mask & below);
            e_ftr[e] = j;
#pragma unroll
            for (int k = 0; k < 3; ++k) xyz[3 * e + k] = (double)A.pos[3 * (size_t)p + k];
            uv[2 * e] = (double)kp.x; uv[2 * e + 1] = (double)kp.y;
            w[e] = (double)s_sig[oct];
        }
        E += total;
    }
    n_obs = wave_sum(n_obs); renewed = wave_sum(renewed); dups = wave_sum(dups);
    flags = (__ballot(flags & FLAG_ENTRY) ? FLAG_ENTRY : 0) | (__ballot(flags & FLAG_OCTAVE) ? FLAG_OCTAVE : 0);
    if (lane == 0) { s_red[0][wave] = n_obs; s_red[1][wave] = renewed; s_red[2][wave] = dups; s_red[3][wave] = flags; }
    __syncthreads();
    n_obs = renewed = dups = flags = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) { n_obs += s_red[0][v]; renewed += s_red[1][v]; dups += s_red[2][v]; flags |= s_red[3][v]; }
    if (tid < 8) {
        const int word = tid == 0 ? n : tid == 1 ? n_obs : tid == 2 ? E : tid == 3 ? renewed : tid == 4 ? dups : tid == 5 ? flags : 0;
        cnt[tid] = word;
        A.info[8 * (size_t)b + tid] = word;
    }
    double* pose_out = A.pose_out + 12 * (size_t)b;
    if (n_obs <= A.min_obs) {                                       // uniform; the gate of :95-98
        if (tid == 0) {
            se3_store(s_P.est0, pose_out);
            A.status[b] = ST_GATE;
        }
        return;
    }
    if (tid == 0) s_P.n = E;
    __syncthreads();

    pose_ba_run(s_P, xyz, uv, w, pose_out, stats);

    if (tid == 0) {
        double P[12];
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 12; ++i) { P[i] = pose_out[i]; fin = fin && isfinite(P[i]); }
        A.status[b] = fin ? ST_OK : ST_NONFINITE;
        if (fin) {                                                  // KeyFrame::setPose(toCvMat(estimate)) (:298-299)
            float* T = A.frame_Tcw + 12 * (size_t)frame;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)P[3 * r + c];
                T[4 * r + 3] = (float)P[9 + r];
            }
            if (A.frame_Twb) {                                      // Twb = Tcw^-1 * cTb, in FP64
                Se3 Tcw = se3_load(P);
                const Se3 Twc = se3_inv(Tcw), Tcb = se3_load(A.Tcb);
                const Se3 Twb = iso_mul(Twc, Tcb);
                float* o = A.frame_Twb + 3 * (size_t)frame;
                o[0] = (float)Twb.t[0];
                o[1] = (float)Twb.t[1];
                o[2] = (float)atan2(Twb.R[3], Twb.R[0]);
            }
        }
    }
}

}  // namespace

extern "C" {

long long se2gpu_localizer_ba_ws_bytes(int njobs, int cap) {
    if (!ws_args_ok(njobs, cap)) return -1;
    return (long long)ws_layout(njobs, cap).bytes;
}

int se2gpu_localizer_ba_ws_layout(int njobs, int cap, long long* offsets, long long* strides, int n) {
    SE2_REQUIRE(ws_args_ok(njobs, cap), SE2GPU_ERR_INVALID, "localizer_ba_ws_layout: njobs = %d, cap = %d", njobs, cap);
    SE2_REQUIRE(offsets && strides && n >= SE2GPU_LOCALIZER_BA_WS_ARRAYS, SE2GPU_ERR_INVALID,
                "localizer_ba_ws_layout: %d offsets and strides are written", SE2GPU_LOCALIZER_BA_WS_ARRAYS);
    const WsLayout L = ws_layout(njobs, cap);
    for (int i = 0; i < SE2GPU_LOCALIZER_BA_WS_ARRAYS; ++i) { offsets[i] = (long long)L.off[i]; strides[i] = (long long)L.stride[i]; }
    return SE2GPU_OK;
}

int se2gpu_localizer_ba_batch_device(se2gpu_matcher* h, const int32_t* d_job_frame, int njobs, int nframes, float* d_frame_Tcw,
                                     float* d_frame_Twb, const se2gpu_keypoint* d_kps_un, const int32_t* d_counts, int cap,
                                     int32_t* d_ftr_mp, uint8_t* d_kf_observed, const int32_t* d_match_idx_mp, const float* d_pos,
                                     int m, const uint8_t* d_mp_null, const uint8_t* d_good_prl, const float* inv_level_sigma2,
                                     int nlevels, float fx, float cx, float cy, const double* Tbc12, double huber_delta,
                                     double xrot_info, double yrot_info, double z_info, int iters, int min_obs, void* d_ws,
                                     int32_t* d_status, double* d_pose_out, se2gpu_ba_stats* d_stats, int32_t* d_info) {
    const char* who = "localizer_ba_batch_device";
    // every refusal comes before the first use of the handle or a device
    SE2_NEED(h);
    SE2_NEED(d_job_frame); SE2_NEED(d_frame_Tcw); SE2_NEED(d_kps_un); SE2_NEED(d_counts); SE2_NEED(d_ftr_mp); SE2_NEED(d_pos);
    SE2_NEED(inv_level_sigma2); SE2_NEED(Tbc12); SE2_NEED(d_ws); SE2_NEED(d_status); SE2_NEED(d_pose_out); SE2_NEED(d_info);
    SE2_REQUIRE(((uintptr_t)d_ws & 15) == 0, SE2GPU_ERR_INVALID, "%s: d_ws is not 16-byte aligned", who);
    SE2_REQUIRE(njobs >= 0, SE2GPU_ERR_INVALID, "%s: njobs = %d is negative", who, njobs);
    SE2_REQUIRE(m >= 0, SE2GPU_ERR_INVALID, "%s: m = %d is negative", who, m);
    SE2_REQUIRE(nframes >= 1, SE2GPU_ERR_INVALID, "%s: nframes = %d", who, nframes);
    SE2_REQUIRE(cap >= 1, SE2GPU_ERR_INVALID, "%s: cap = %d", who, cap);
    SE2_REQUIRE(iters >= 0 && iters <= 64, SE2GPU_ERR_INVALID, "%s: iters = %d (0..64, the length of the se2gpu_ba_stats histories)", who, iters);
    SE2_REQUIRE(nlevels >= 1 && nlevels <= 32, SE2GPU_ERR_INVALID, "%s: nlevels = %d (1..32)", who, nlevels);
    SE2_REQUIRE(min_obs >= -1, SE2GPU_ERR_INVALID, "%s: min_obs = %d (-1 = run always)", who, min_obs);
    SE2_REQUIRE(njobs <= MAX_JOBS, SE2GPU_ERR_CAPACITY, "%s: njobs = %d exceeds the limit %d", who, njobs, MAX_JOBS);
    SE2_REQUIRE((long long)nframes * cap <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: nframes * cap = %lld exceeds 2^31 - 1", who,
                (long long)nframes * cap);
    SE2_REQUIRE((long long)njobs * cap * 3 <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: njobs * cap * 3 = %lld exceeds 2^31 - 1", who,
                (long long)njobs * cap * 3);
    SE2_REQUIRE((long long)m * 3 <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: m * 3 = %lld exceeds 2^31 - 1", who, (long long)m * 3);
    if (njobs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();

    LocArgs a;
    a.njobs = njobs; a.nframes = nframes; a.cap = cap; a.m = m; a.nlevels = nlevels; a.iters = iters; a.min_obs = min_obs;
    a.job_frame = d_job_frame; a.frame_Tcw = d_frame_Tcw; a.frame_Twb = d_frame_Twb; a.kps_un = d_kps_un; a.counts = d_counts;
    a.ftr_mp = d_ftr_mp; a.kf_observed = d_kf_observed; a.match = d_match_idx_mp; a.pos = d_pos; a.mp_null = d_mp_null;
    a.good_prl = d_good_prl;
    for (int i = 0; i < 32; ++i) a.isig.v[i] = i < nlevels ? inv_level_sigma2[i] : 0.f;
    a.f = fx; a.cx = cx; a.cy = cy; a.delta = huber_delta; a.xrot = xrot_info; a.yrot = yrot_info; a.z = z_info;
    std::memcpy(a.Tbc, Tbc12, sizeof(a.Tbc));
    se3_store(se3_inv(se3_load(Tbc12)), a.Tcb);
    a.ws = (char*)d_ws;
    a.lay = ws_layout(njobs, cap);
    a.status = d_status; a.pose_out = d_pose_out; a.stats = d_stats; a.info = d_info;
    hipLaunchKernelGGL(k_localizer_ba, dim3(njobs), dim3(BLOCK), 0, (hipStream_t)se2gpu_matcher_stream(h), a);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // extern "C"
