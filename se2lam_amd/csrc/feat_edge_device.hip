// libse2gpu - GlobalMapper::CreateFeatEdge on the tables where they lie in device memory: se2gpu_feat_edge_batch_device.
// The covisibility chain (se2gpu_covis_pairs_device's d_common) and the loop chain (se2gpu_track_loop_verify_batch_device's
// d_matches_mp) end in device arrays; this call turns them into the rows k_feat_edge reads, without the host in between:
//   k_feat_gather       one wave per pair: key-frame poses from the frame table (3 x 4 float rows -> rotation, translation in
//                       double), the pair's points compacted in list order at the head of its row (ballot + popcount of the
//                       lower lanes + a running base: no atomics, the same row in every run and at every place in a batch),
//                       the counts, and the constant index arrays k_sparsify wants for the row
//   k_plane_prior_iso3  one thread per key frame: addVertexSE3PlaneMotion's prior (se3_math.h, the text the host function
//                       se2gpu_plane_motion_prior_iso3 runs)
//   k_feat_edge         feat_edge.hip, unchanged in its arithmetic (launch_feat_edge)
//   k_sparsify          sparsify.hip (launch_sparsify)
//   k_feat_finish       one thread per pair: the finite test and the zeroing that se2gpu_feat_edge_batch does on the host
//                       after its download, and d_info8
// Five launches (and one memset with d_stats) on the matcher's stream; nothing is allocated, uploaded besides kernel
// arguments, read back or waited for.  Every index read from an array is range-checked before it is used; the loads of the
// indexed tables are unconditional on clamped indices and the results selected afterwards (profiles/local_window.md).
// Compiled with -ffp-contract=off: the prior's information matrix equals the host function's to the bit.
#include "common.h"
#include "se3_math.h"
#include "wave_int.h"

using namespace se2gpu;

namespace {

constexpr int MAX_PAIRS = 65535;   // se2gpu_feat_edge_batch's limit

// d_ws: the regions in this order, each starting at a multiple of 8 bytes.  P = npairs, NP = npairs * row_cap.
enum {
    WS_META, WS_KF12, WS_PMEAS, WS_PINFO, WS_XYZ0, WS_MZ, WS_MINFO, WS_PA, WS_PB, WS_MPOUT, WS_CHI, WS_SPXYZ, WS_SPINFO, WS_KFBLK,
    WS_SCHUR, WS_INFO4, WS_SPCNT, WS_MPPTR, WS_ORDPTR, WS_MMPTR, WS_MKF, WS_ORD, WS_OUTL, WS_REGIONS
};
struct WsLayout {
    size_t off[WS_REGIONS];
    size_t bytes;
};

bool ws_args_ok(int npairs, int row_cap) {
    return npairs >= 0 && npairs <= MAX_PAIRS && row_cap >= 1 && 2 * (long long)npairs * row_cap <= 2147483647LL;
}

WsLayout ws_layout(int npairs, int row_cap) {
    const size_t P = (size_t)npairs, NP = P * (size_t)row_cap;
    const size_t size[WS_REGIONS] = {
        4 * 4 * P,                                               // {count, raw, dropped, cut} x P
        8 * 24 * P, 8 * 24 * P, 8 * 72 * P,                      // kf12, prior measurement, prior information
        8 * 3 * NP, 8 * 6 * NP, 8 * 18 * NP,                     // the gathered rows: start xyz (kept), m_z, m_info
        8 * 3 * NP, 8 * 3 * NP,                                  // k_feat_edge's estimate / trial (pa starts as a copy of xyz)
        8 * 3 * NP, 8 * 2 * NP,                                  // mp_xyz_out / edge_chi2 when the caller wants none
        8 * 3 * NP, 8 * 18 * NP, 8 * 72 * NP, 8 * 144 * NP,      // the sparsifier's points, informations and scratch
        4 * 4 * P, 4 * P,                                        // k_feat_edge's info4; sp_cnt
        4 * (P + 1), 4 * (P + 1), 4 * (NP + 1), 4 * 2 * NP, 4 * 2 * NP,   // mp_ptr, ord_ptr, mm_ptr, m_kf, ord
        NP                                                       // outlier when the caller wants none
    };
    WsLayout L;
    size_t at = 0;
    for (int i = 0; i < WS_REGIONS; ++i) {
        L.off[i] = at;
        at += (size[i] + 7) & ~(size_t)7;
    }
    L.bytes = at ? at : 8;
    return L;
}

struct GatherArgs {
    int npairs, nframes, m, nobs, cap, row_cap, list_cap;
    const int* pair_a;
    const int* pair_b;
    const float* Twc;        // nframes x 12: rows 0-2 of the 3 x 4 matrix
    const float* pos;        // m x 3
    // covisibility route
    const int* pair_out;     // 4 per pair
    const int* common;       // 3 per entry, list_cap entries per pair
    const float* obs_view;   // nobs x 3
    const float* obs_info;   // nobs x 9
    // match route
    const int* matches;      // npairs x cap
    const int* counts;       // nframes
    const int* ftr_mp;       // nframes x cap
    const float* view_pos;   // nframes x cap x 3
    const float* view_info;  // nframes x cap x 9
    // the rows in d_ws
    double* kf12;
    double* xyz0;
    double* pa;
    double* m_z;
    double* m_info;
    int* meta;
    int* mp_ptr;
    int* ord_ptr;
    int* mm_ptr;
    int* m_kf;
    int* ord;
    uint8_t* outlier;
    double* edge_chi2;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int MODE>
__global__ __launch_bounds__(64) void k_feat_gather(const GatherArgs A) {
    const int p = blockIdx.x;
    if (p >= A.npairs) return;
    const int lane = threadIdx.x;
    const int a = A.pair_a[p], b = A.pair_b[p];
    const bool ok = a >= 0 && a < A.nframes && b >= 0 && b < A.nframes;
    const size_t row0 = (size_t)p * A.row_cap;
    // the two poses: rows of a 3 x 4 float matrix -> rotation (9, row-major), translation (3); float -> double is exact.  A
    // slot out of range gives the identity.
    if (lane < 24) {
        const int k = lane / 12, e = lane % 12, slot = k ? b : a;
        const bool in = slot >= 0 && slot < A.nframes;
        const int src = e < 9 ? 4 * (e / 3) + e % 3 : 4 * (e - 9) + 3;
        const float v = A.Twc[12 * (size_t)clampi(slot, 0, A.nframes - 1) + src];
        A.kf12[24 * (size_t)p + lane] = in ? (double)v : (e == 0 || e == 4 || e == 8 ? 1.0 : 0.0);
    }
    // k_sparsify's index arrays for this row: point g has the measurements 2g (key frame 0) and 2g + 1, listed in that order
    for (int j = lane; j < A.row_cap; j += 64) {
        const int g = (int)row0 + j;
        A.mm_ptr[g] = 2 * g;
        A.m_kf[2 * (size_t)g] = 0; A.m_kf[2 * (size_t)g + 1] = 1;
        A.ord[2 * (size_t)g] = 2 * g; A.ord[2 * (size_t)g + 1] = 2 * g + 1;
    }
    if (lane == 0) {
        A.mp_ptr[p] = (int)row0;
        A.ord_ptr[p] = 2 * (int)row0;
        if (p == A.npairs - 1) {
            const int end = (int)row0 + A.row_cap;
            A.mp_ptr[p + 1] = end; A.ord_ptr[p + 1] = 2 * end; A.mm_ptr[end] = 2 * end;
        }
    }

    int L, nb = 0, n_same = 0;   // entries scanned; match route: the features of b
    if (MODE == SE2GPU_FEAT_EDGE_COVIS) {
        n_same = A.pair_out[4 * (size_t)p];
        L = ok && n_same >= 0 ? min(n_same, min(A.list_cap, A.row_cap)) : 0;
    } else {
        L = ok ? clampi(A.counts[clampi(a, 0, A.nframes - 1)], 0, A.cap) : 0;
        nb = ok ? clampi(A.counts[clampi(b, 0, A.nframes - 1)], 0, A.cap) : 0;
    }
    const bool tables = A.m > 0 && (MODE != SE2GPU_FEAT_EDGE_COVIS || A.nobs > 0);   // an empty table has no element 0 to load
    int raw = 0, npts = 0;
    for (int base = 0; base < L; base += 64) {   // whole-wave steps
        const int i = base + lane;
        const bool active = i < L;
        bool valid = false, israw = false;
        float xyz[3] = {0, 0, 0}, za[3] = {0, 0, 0}, zb[3] = {0, 0, 0}, wa[9], wb[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wa[k] = wb[k] = 0;
        if (MODE == SE2GPU_FEAT_EDGE_COVIS) {
            const int* c = A.common + 3 * ((size_t)p * A.list_cap + min(i, L - 1));
            const int pt = c[0], ea = c[1], eb = c[2];
            israw = active;
            valid = active && pt >= 0 && pt < A.m && ea >= 0 && ea < A.nobs && eb >= 0 && eb < A.nobs;
            if (tables) {
                const size_t ptc = clampi(pt, 0, A.m - 1), eac = clampi(ea, 0, A.nobs - 1), ebc = clampi(eb, 0, A.nobs - 1);
#pragma unroll
                for (int k = 0; k < 3; ++k) { xyz[k] = A.pos[3 * ptc + k]; za[k] = A.obs_view[3 * eac + k]; zb[k] = A.obs_view[3 * ebc + k]; }
#pragma unroll
                for (int k = 0; k < 9; ++k) { wa[k] = A.obs_info[9 * eac + k]; wb[k] = A.obs_info[9 * ebc + k]; }
            }
        } else {
            const int ic = min(i, L - 1);
            const int j = A.matches[(size_t)p * A.cap + ic];
            israw = active && j >= 0 && j < nb;
            const size_t fa_at = (size_t)a * A.cap + ic, fb_at = (size_t)b * A.cap + clampi(j, 0, A.cap - 1);   // ok holds: L > 0
            const int fa = A.ftr_mp[fa_at], fb = A.ftr_mp[fb_at];
            valid = israw && fa >= 0 && fa < A.m && fb >= 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { za[k] = A.view_pos[3 * fa_at + k]; zb[k] = A.view_pos[3 * fb_at + k]; }
#pragma unroll
            for (int k = 0; k < 9; ++k) { wa[k] = A.view_info[9 * fa_at + k]; wb[k] = A.view_info[9 * fb_at + k]; }
            if (tables) {
                const size_t fac = clampi(fa, 0, A.m - 1);
#pragma unroll
                for (int k = 0; k < 3; ++k) xyz[k] = A.pos[3 * fac + k];
            }
        }
        const unsigned long long mask = __ballot(valid);
        raw += __popcll(__ballot(israw));
        const int slot = npts + lane_rank(mask);
        npts += __popcll(mask);
        if (valid && slot < A.row_cap) {
            const size_t r = row0 + slot;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                A.xyz0[3 * r + k] = A.pa[3 * r + k] = (double)xyz[k];
                A.m_z[6 * r + k] = (double)za[k];
                A.m_z[6 * r + 3 + k] = (double)zb[k];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) { A.m_info[18 * r + k] = (double)wa[k]; A.m_info[18 * r + 9 + k] = (double)wb[k]; }
            // what a pair that is not run leaves for its points, as se2gpu_feat_edge_batch's memsets do
            A.outlier[r] = 0;
            A.edge_chi2[2 * r] = 0.0; A.edge_chi2[2 * r + 1] = 0.0;
        }
    }
    if (lane == 0) {
        const int P = A.npairs;
        int cut;
        if (MODE == SE2GPU_FEAT_EDGE_COVIS) {
            cut = ok && n_same > min(A.list_cap, A.row_cap);
            raw = n_same;
            A.meta[2 * P + p] = L - npts;
        } else {
            cut = npts > A.row_cap;
            A.meta[2 * P + p] = raw - npts;
        }
        A.meta[p] = min(npts, A.row_cap);
        A.meta[P + p] = raw;
        A.meta[3 * P + p] = cut;
    }
}

struct Tbc12 {
    double v[12];
};

__global__ __launch_bounds__(64) void k_plane_prior_iso3(int n, const double* __restrict__ kf12, const Tbc12 Tbc, double xrot_info,
                                                         double yrot_info, double z_info, double* __restrict__ meas12,
                                                         double* __restrict__ info36) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    double Twc[12], meas[12], info[36];
#pragma unroll
    for (int i = 0; i < 12; ++i) Twc[i] = kf12[12 * (size_t)k + i];
    plane_motion_prior_iso3(Twc, Tbc.v, xrot_info, yrot_info, z_info, meas, info);
#pragma unroll
    for (int i = 0; i < 12; ++i) meas12[12 * (size_t)k + i] = meas[i];
#pragma unroll
    for (int i = 0; i < 36; ++i) info36[36 * (size_t)k + i] = info[i];
}

// no constraint for a pair that was not run (1) or whose result is not finite (2)
__global__ __launch_bounds__(64) void k_feat_finish(int npairs, const int32_t* __restrict__ info4, const int* __restrict__ meta,
                                                    double* __restrict__ z_out12, double* __restrict__ info_out36,
                                                    int32_t* __restrict__ info8) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= npairs) return;
    double* z = z_out12 + 12 * (size_t)p;
    double* w = info_out36 + 36 * (size_t)p;
    bool fin = true;
    for (int i = 0; i < 12; ++i) fin = fin && isfinite(z[i]);
    for (int i = 0; i < 36; ++i) fin = fin && isfinite(w[i]);
    int status = info4[4 * p], handed = info4[4 * p + 3];
    if (status == 0 && !fin) { status = 2; handed = 0; }
    if (status != 0) {
        for (int i = 0; i < 12; ++i) z[i] = 0.0;
        for (int i = 0; i < 36; ++i) w[i] = 0.0;
    }
    int32_t* o = info8 + 8 * (size_t)p;
    o[0] = status; o[1] = info4[4 * p + 1]; o[2] = info4[4 * p + 2]; o[3] = handed;
    o[4] = meta[npairs + p]; o[5] = meta[2 * npairs + p]; o[6] = meta[3 * npairs + p]; o[7] = 0;
}

}  // namespace

extern "C" {

long long se2gpu_feat_edge_ws_bytes(int npairs, int row_cap) {
    if (!ws_args_ok(npairs, row_cap)) return -1;
    return (long long)ws_layout(npairs, row_cap).bytes;
}

int se2gpu_feat_edge_ws_layout(int npairs, int row_cap, long long* offsets, int n) {
    SE2_REQUIRE(ws_args_ok(npairs, row_cap), SE2GPU_ERR_INVALID, "feat_edge_ws_layout: npairs = %d, row_cap = %d", npairs, row_cap);
    SE2_REQUIRE(offsets && n >= SE2GPU_FEAT_EDGE_WS_ARRAYS, SE2GPU_ERR_INVALID, "feat_edge_ws_layout: %d offsets are written", SE2GPU_FEAT_EDGE_WS_ARRAYS);
    const WsLayout L = ws_layout(npairs, row_cap);
    const int which[SE2GPU_FEAT_EDGE_WS_ARRAYS] = {WS_META, WS_KF12, WS_PMEAS, WS_PINFO, WS_XYZ0, WS_MZ, WS_MINFO};
    for (int i = 0; i < SE2GPU_FEAT_EDGE_WS_ARRAYS; ++i) offsets[i] = (long long)L.off[which[i]];
    return SE2GPU_OK;
}

int se2gpu_feat_edge_batch_device(se2gpu_matcher* h, int mode, int iters, int min_points, double huber_delta, double outlier_chi2,
                                  const double* Tbc12_host, double xrot_info, double yrot_info, double z_info,
                                  const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs, int nframes,
                                  const float* d_frame_Twc, const float* d_pos, int m, int row_cap,
                                  const int32_t* d_pair_out, const int32_t* d_common, int list_cap, const float* d_obs_view,
                                  const float* d_obs_info, int nobs,
                                  const int32_t* d_matches, const int32_t* d_counts, int cap, const int32_t* d_ftr_mp,
                                  const float* d_view_pos, const float* d_view_info,
                                  void* d_ws, int32_t* d_info8, double* d_kf12_out, double* d_z_out12, double* d_info_out36,
                                  double* d_mp_xyz_out, uint8_t* d_outlier, double* d_edge_chi2, se2gpu_ba_stats* d_stats) {
    const char* who = "feat_edge_batch_device";
    // every refusal comes before the first use of the handle or a device
    SE2_NEED(h);
    SE2_REQUIRE(mode == SE2GPU_FEAT_EDGE_COVIS || mode == SE2GPU_FEAT_EDGE_MATCH, SE2GPU_ERR_INVALID, "%s: mode %d", who, mode);
    const bool covis = mode == SE2GPU_FEAT_EDGE_COVIS;
    SE2_REQUIRE(iters >= 1 && iters <= 64, SE2GPU_ERR_INVALID, "%s: %d iterations (1..64, the length of the se2gpu_ba_stats histories)", who, iters);
    SE2_NEED(Tbc12_host); SE2_NEED(d_pair_a); SE2_NEED(d_pair_b); SE2_NEED(d_frame_Twc); SE2_NEED(d_pos);
    SE2_NEED(d_ws); SE2_NEED(d_info8); SE2_NEED(d_kf12_out); SE2_NEED(d_z_out12); SE2_NEED(d_info_out36);
    SE2_REQUIRE(npairs >= 0, SE2GPU_ERR_INVALID, "%s: npairs = %d is negative", who, npairs);
    SE2_REQUIRE(m >= 0, SE2GPU_ERR_INVALID, "%s: m = %d is negative", who, m);
    SE2_REQUIRE(nframes >= 1, SE2GPU_ERR_INVALID, "%s: nframes = %d", who, nframes);
    SE2_REQUIRE(row_cap >= 1, SE2GPU_ERR_INVALID, "%s: row_cap = %d", who, row_cap);
    // the scalars of both routes are checked whatever the mode; the arrays of the mode's route only
    SE2_REQUIRE(nobs >= 0, SE2GPU_ERR_INVALID, "%s: nobs = %d is negative", who, nobs);
    SE2_REQUIRE(list_cap >= 1, SE2GPU_ERR_INVALID, "%s: list_cap = %d", who, list_cap);
    SE2_REQUIRE(cap >= 1, SE2GPU_ERR_INVALID, "%s: cap = %d", who, cap);
    if (covis) {
        SE2_NEED(d_pair_out); SE2_NEED(d_common); SE2_NEED(d_obs_view); SE2_NEED(d_obs_info);
    } else {
        SE2_NEED(d_matches); SE2_NEED(d_counts); SE2_NEED(d_ftr_mp); SE2_NEED(d_view_pos); SE2_NEED(d_view_info);
    }
    SE2_REQUIRE(npairs <= MAX_PAIRS, SE2GPU_ERR_CAPACITY, "%s: %d pairs in one call (at most %d)", who, npairs, MAX_PAIRS);
    SE2_REQUIRE(2 * (long long)npairs * row_cap <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: 2 * npairs * row_cap = %lld exceeds 2^31 - 1",
                who, 2 * (long long)npairs * row_cap);
    SE2_REQUIRE((long long)nframes * cap <= 2147483647LL, SE2GPU_ERR_CAPACITY, "%s: nframes * cap = %lld exceeds 2^31 - 1", who,
                (long long)nframes * cap);
    if (npairs == 0) return SE2GPU_OK;
    SE2_NEED_DEVICE();

    const WsLayout L = ws_layout(npairs, row_cap);
    char* ws = (char*)d_ws;
    auto dbl = [&](int r) { return (double*)(ws + L.off[r]); };
    auto i32 = [&](int r) { return (int*)(ws + L.off[r]); };
    hipStream_t st = (hipStream_t)se2gpu_matcher_stream(h);
    double* mp_out = d_mp_xyz_out ? d_mp_xyz_out : dbl(WS_MPOUT);
    double* chi = d_edge_chi2 ? d_edge_chi2 : dbl(WS_CHI);
    uint8_t* outl = d_outlier ? d_outlier : (uint8_t*)(ws + L.off[WS_OUTL]);

    GatherArgs g;
    g.npairs = npairs; g.nframes = nframes; g.m = m; g.nobs = nobs; g.cap = cap; g.row_cap = row_cap; g.list_cap = list_cap;
    g.pair_a = d_pair_a; g.pair_b = d_pair_b; g.Twc = d_frame_Twc; g.pos = d_pos;
    g.pair_out = d_pair_out; g.common = d_common; g.obs_view = d_obs_view; g.obs_info = d_obs_info;
    g.matches = d_matches; g.counts = d_counts; g.ftr_mp = d_ftr_mp; g.view_pos = d_view_pos; g.view_info = d_view_info;
    g.kf12 = dbl(WS_KF12); g.xyz0 = dbl(WS_XYZ0); g.pa = dbl(WS_PA); g.m_z = dbl(WS_MZ); g.m_info = dbl(WS_MINFO);
    g.meta = i32(WS_META); g.mp_ptr = i32(WS_MPPTR); g.ord_ptr = i32(WS_ORDPTR); g.mm_ptr = i32(WS_MMPTR); g.m_kf = i32(WS_MKF);
    g.ord = i32(WS_ORD); g.outlier = outl; g.edge_chi2 = chi;
    if (covis) hipLaunchKernelGGL(k_feat_gather<SE2GPU_FEAT_EDGE_COVIS>, dim3(npairs), dim3(64), 0, st, g);
    else hipLaunchKernelGGL(k_feat_gather<SE2GPU_FEAT_EDGE_MATCH>, dim3(npairs), dim3(64), 0, st, g);
    SE2_HIP(hipGetLastError());

    // the EdgeSE3Prior of every key frame, from its INPUT pose (addVertexSE3PlaneMotion)
    Tbc12 tbc;
    std::memcpy(tbc.v, Tbc12_host, sizeof tbc.v);
    hipLaunchKernelGGL(k_plane_prior_iso3, dim3((2 * npairs + 63) / 64), dim3(64), 0, st, 2 * npairs, dbl(WS_KF12), tbc, xrot_info,
                       yrot_info, z_info, dbl(WS_PMEAS), dbl(WS_PINFO));
    SE2_HIP(hipGetLastError());

    if (d_stats) SE2_HIP(hipMemsetAsync(d_stats, 0, (size_t)npairs * sizeof(se2gpu_ba_stats), st));
    FeatEdgeArgs a;
    a.npairs = npairs; a.mode = mode; a.iters = iters; a.min_points = min_points;
    a.kf12 = dbl(WS_KF12); a.prior_meas = dbl(WS_PMEAS); a.prior_info = dbl(WS_PINFO); a.mp_ptr = i32(WS_MPPTR);
    a.mp_cnt = i32(WS_META); a.raw_cnt = i32(WS_META) + npairs;
    a.m_z = dbl(WS_MZ); a.m_info = dbl(WS_MINFO); a.huber_delta = huber_delta; a.outlier_chi2 = outlier_chi2;
    a.pa = dbl(WS_PA); a.pb = dbl(WS_PB); a.kf12_out = d_kf12_out; a.mp_out = mp_out; a.outlier = outl; a.edge_chi2 = chi;
    a.info4 = i32(WS_INFO4); a.stats = d_stats; a.sp_xyz = dbl(WS_SPXYZ); a.sp_info = dbl(WS_SPINFO); a.sp_cnt = i32(WS_SPCNT);
    SE2_CHECK(launch_feat_edge(st, a));
    SE2_CHECK(launch_sparsify(st, npairs, d_kf12_out, i32(WS_MPPTR), dbl(WS_SPXYZ), i32(WS_MMPTR), i32(WS_MKF), dbl(WS_SPINFO),
                              i32(WS_ORDPTR), i32(WS_ORD), dbl(WS_KFBLK), dbl(WS_SCHUR), i32(WS_SPCNT), d_z_out12, d_info_out36));
    hipLaunchKernelGGL(k_feat_finish, dim3((npairs + 63) / 64), dim3(64), 0, st, npairs, i32(WS_INFO4), i32(WS_META), d_z_out12,
                       d_info_out36, d_info8);
    SE2_HIP(hipGetLastError());
    return SE2GPU_OK;
}

}  // extern "C"
