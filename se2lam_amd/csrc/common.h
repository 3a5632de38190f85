// Shared host-side utilities of libse2gpu (error channel, device buffers, launch profiling).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/se2gpu.h"

namespace se2gpu {

void set_error(const char* fmt, ...);
bool have_device();
// in-place sum all-reduce of `count` doubles through a native RCCL communicator (comm.hip); 0 on success
int comm_allreduce(se2gpu_comm* c, void* dev_ptr, size_t count, void* hip_stream);
int comm_rank(const se2gpu_comm* c);
int comm_world(const se2gpu_comm* c);
// k_sparsify (sparsify.hip) on device arrays, on `stream`: what se2gpu_sparsify_se3xyz launches after its host preparation
// (measurements grouped by point: d_mm_ptr / d_m_kf / d_m_info; d_ord_ptr / d_ord: the order they were given in; scratch of
// 36 doubles per measurement and 144 per point).  d_mp_cnt, when not NULL, gives the number of points at the head of every
// pair's row that count (rows compacted on the device, feat_edge.hip); the measurements are then listed point by point.
int launch_sparsify(hipStream_t stream, int npairs, const double* d_kf12, const int* d_mp_ptr, const double* d_mp_xyz,
                    const int* d_mm_ptr, const int* d_m_kf, const double* d_m_info, const int* d_ord_ptr, const int* d_ord,
                    double* d_kf_blk, double* d_schur, const int* d_mp_cnt, double* d_z_out, double* d_info_out);
// k_feat_edge (feat_edge.hip) on device arrays, on `stream`: one wave per pair, what se2gpu_feat_edge_batch launches after
// its uploads.  Pair p's points are the rows [mp_ptr[p], mp_ptr[p+1]) of every per-point array.
struct FeatEdgeArgs {
    int npairs, mode, iters, min_points;
    const double* kf12;         // npairs x 2 x 12
    const double* prior_meas;   // npairs x 2 x 12
    const double* prior_info;   // npairs x 2 x 36
    const int* mp_ptr;
    const int* mp_cnt;          // optional: only the first mp_cnt[p] rows of pair p count (rows with slack, feat_edge_device.hip)
    const int* raw_cnt;         // optional: the count min_points is tested against, instead of the number of points
    const double* m_z;          // per point 2 x 3
    const double* m_info;       // per point 2 x 9
    double huber_delta, outlier_chi2;
    double* pa;                 // the points: the start values on entry; pa / pb alternate as estimate and trial
    double* pb;
    double* kf12_out;
    double* mp_out;
    uint8_t* outlier;
    double* edge_chi2;
    int32_t* info4;
    se2gpu_ba_stats* stats;     // optional
    // what k_sparsify reads: a pair's inliers, compacted in input order at the head of its rows
    double* sp_xyz;
    double* sp_info;
    int* sp_cnt;
};
int launch_feat_edge(hipStream_t stream, const FeatEdgeArgs& args);

// The SE2GPU_* environment switches (README) are read through these; an unset variable gives `dflt`.  A flag is on for a
// value that starts with '1', off for one that starts with '0', `dflt` for anything else; env_is compares the whole value.
inline bool env_flag(const char* name, bool dflt) {
    const char* e = std::getenv(name);
    return e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : dflt;
}
inline int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
inline bool env_is(const char* name, const char* value) {
    const char* e = std::getenv(name);
    return e && std::strcmp(e, value) == 0;
}

#define SE2_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            ::se2gpu::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return SE2GPU_ERR_HIP;                                                             \
        }                                                                                      \
    } while (0)

#define SE2_CHECK(expr)                 \
    do {                                \
        int _rc = (expr);               \
        if (_rc != SE2GPU_OK) return _rc; \
    } while (0)

#define SE2_REQUIRE(cond, code, ...)          \
    do {                                      \
        if (!(cond)) {                        \
            ::se2gpu::set_error(__VA_ARGS__); \
            return (code);                    \
        }                                     \
    } while (0)

// A required pointer argument, refused by its name; `who` (a const char* in scope) names the call.  _IF: required when `cond`.
#define SE2_NEED(ptr) SE2_REQUIRE(ptr, SE2GPU_ERR_INVALID, "%s: " #ptr " is NULL", who)
#define SE2_NEED_IF(cond, ptr) SE2_REQUIRE(!(cond) || (ptr), SE2GPU_ERR_INVALID, "%s: " #ptr " is NULL with " #cond, who)
#define SE2_NEED_DEVICE() SE2_REQUIRE(::se2gpu::have_device(), SE2GPU_ERR_NO_DEVICE, "no HIP device visible (libse2gpu has no CPU fallback)")

// Growable device allocation (never shrinks).  Not copyable.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    bool owned = true;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && owned) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        owned = true;
    }
    // view into somebody else's allocation (an arena): never freed here, replaced by the next alias() / reserve()
    void alias(T* q) {
        release();
        p = q;
        owned = false;
    }
    int reserve(size_t n) {
        if (n <= cap) return SE2GPU_OK;
        release();
        if (n == 0) return SE2GPU_OK;
        SE2_HIP(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return SE2GPU_OK;
    }
    int upload(const T* src, size_t n, hipStream_t s) {
        SE2_CHECK(reserve(n));
        if (n) SE2_HIP(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
        return SE2GPU_OK;
    }
    int upload(const std::vector<T>& v, hipStream_t s) { return upload(v.data(), v.size(), s); }
};

// Pinned host staging buffer.
template <typename T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    int reserve(size_t n) {
        if (n <= cap) return SE2GPU_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        SE2_HIP(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault));
        cap = n;
        return SE2GPU_OK;
    }
};

// Optional per-kernel timing with HIP events around every launch (serialises; for bench.py's
// `roofline.achieved`, which must be measured on the stream the kernels are launched on).
struct LaunchProfile {
    struct Slot {
        const char* name;
        double ms = 0;
        int64_t launches = 0;
    };
    bool enabled = false;
    std::vector<Slot> slots;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~LaunchProfile() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int slot(const char* name) {
        for (size_t i = 0; i < slots.size(); ++i)
            if (slots[i].name == name || std::strcmp(slots[i].name, name) == 0) return (int)i;
        slots.push_back(Slot{name});
        return (int)slots.size() - 1;
    }
    void begin(hipStream_t s) {
        if (!enabled) return;
        if (!e0) {
            (void)hipEventCreate(&e0);
            (void)hipEventCreate(&e1);
        }
        (void)hipEventRecord(e0, s);
    }
    void end(hipStream_t s, const char* name) {
        if (!enabled) return;
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        Slot& sl = slots[slot(name)];
        sl.ms += ms;
        sl.launches += 1;
    }
    void reset() {
        for (auto& s : slots) {
            s.ms = 0;
            s.launches = 0;
        }
    }
};

#define SE2_LAUNCH(prof, stream, name, kernel, grid, block, shmem, ...)         \
    do {                                                                        \
        (prof).begin(stream);                                                   \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);    \
        (prof).end(stream, name);                                               \
    } while (0)

}  // namespace se2gpu
