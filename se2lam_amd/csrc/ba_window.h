// One workgroup per local window (the kernel: csrc/ba_window_skeleton.h; its two pose models: csrc/ba_window.hip, SE(2), and
// csrc/ba_window3.hip, SE3-expmap): the argument packs and the launchers.  csrc/ba.hip fills the packs from its handles
// (se2gpu_ba_optimize_batch) - the kernel knows nothing about handles, streams or pools.
#pragma once
#include "ba3_device.h"
#include "ba_device.h"
#include "common.h"

namespace se2gpu {

// what every model's pack holds (the kernel skeleton reads these); sizes that depend on the model are given as SE(2) / SE3-expmap
struct WindowArgsBase {
    int P, L, E, O, iters, mode;
    const int* lm_ptr;        // L + 1: the observation edges are sorted by landmark
    const int* e_kf;          // E: pose index of an edge
    const double* e_uv;       // E x 2
    const double* e_info;     // E x 3 (xx, xy, yy / w: the information is w I)
    double* poses_a;          // P x 3 / P x 12, the two estimate buffers (BaCtl::sel says which one holds the estimate)
    double* poses_b;
    double* lms_a;            // L x 3
    double* lms_b;
    const uint8_t* fixed;     // P
    const int* o_i;           // O: the odometry edges, PreEdgeSE2 (this key frame, next key frame) / EdgeSE3Expmap (i, j)
    const int* o_j;
    const double* o_meas;     // O x 3 / O x 12
    const double* o_info;     // O x 9 / O x 36
    badev::BaCtl* ctl;        // the window's controller block (device)
    double* mail;             // device address of the window's mapped mailbox, or NULL
    const int* stop;          // device address of the mapped force-stop word, or NULL
    int4* desc;               // scratch: the kernel lists the landmarks by their observation counts here (L x 16 B) and copies the
                              // observations into that order behind the list (E x 44 B / E x 28 B)
    double* ainv;             // L x 6 of scratch: the build pass leaves every landmark's factor A here (list order) for the update pass
    long long* stamps;        // debug: 16 phase time stamps (100 MHz wall clock) of the LAST trial, or NULL
};

// the SE(2)-XYZ model's window (csrc/ba_window.hip): poses (x, y, theta), a 2 x 2 information per observation, PreEdgeSE2 odometry
struct WindowArgs : WindowArgsBase {
    badev::CamDev cam;
};

// the SE3-expmap model's window (csrc/ba_window3.hip): poses Tcw as 12 doubles (R row-major, t), isotropic information w I per
// projection edge, a prior per pose (EdgeSE3ExpmapPrior) and EdgeSE3Expmap odometry edges with 6 x 6 information
struct Window3Args : WindowArgsBase {
    badev::Cam3 cam;
    const uint8_t* prior_has; // P: EdgeSE3ExpmapPrior of a pose (measurement P x 12, information P x 36)
    const double* prior_meas;
    const double* prior_info;
};

constexpr int kWindowMaxDegree = 64;     // observations of one landmark the kernel takes (a wave per landmark beyond 16)

// dynamic LDS a window of P poses, nfree of them free, needs with `threads` threads per workgroup (0: does not fit 160 KiB)
size_t ba_window_lds_bytes(int P, int nfree, int threads);
// count workgroups of `threads` (128, 256 or 512) threads, one per pack; asynchronous on st
int ba_window_launch(const WindowArgs* d_args, int count, int threads, size_t lds_bytes, hipStream_t st);
// the same behind a device-side gather (csrc/local_ba_device.hip): workgroup k returns before it reads its pack when d_status[k] != 0.
// Serialises its own raise of the dynamic-LDS limit.
int ba_window_launch_status(const WindowArgs* d_args, const int* d_status, int count, int threads, size_t lds_bytes, hipStream_t st);
// the same for SE3-expmap windows (csrc/ba_window3.hip)
size_t ba_window3_lds_bytes(int P, int nfree, int threads);
int ba_window3_launch(const Window3Args* d_args, int count, int threads, size_t lds_bytes, hipStream_t st);

}  // namespace se2gpu
