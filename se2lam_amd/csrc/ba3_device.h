// Device-side pieces of the SE3-expmap bundle adjustment that more than one translation unit needs (csrc/ba.hip: the multi-launch
// k3_* kernels; csrc/ba_window3.hip: the SE3 model of the one-workgroup-per-window solver, csrc/ba_window_skeleton.h): the camera of EdgeProjectXYZ2UV and its residual with
// the 2x6 pose / 2x3 landmark Jacobians.  [3P g2o 20160424] EdgeProjectXYZ2UV::computeError / linearizeOplus, restated as in
// oracle/ba3_ref.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace se2gpu {
namespace badev {

struct Cam3 { double f, cx, cy, huber; };

}  // namespace badev
}  // namespace se2gpu

namespace {

using se2gpu::badev::Cam3;

__device__ __host__ inline int sym6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }   // r <= c

template <bool JAC>
__device__ inline void proj3(const Cam3& cam, const double* __restrict__ T, double X0, double X1, double X2, double u, double v,
                             double& e0, double& e1, double* Jp, double* Jl) {
    const double x = T[0] * X0 + T[1] * X1 + T[2] * X2 + T[9];
    const double y = T[3] * X0 + T[4] * X1 + T[5] * X2 + T[10];
    const double z = T[6] * X0 + T[7] * X1 + T[8] * X2 + T[11];
    const double zi = 1.0 / z;
    e0 = u - (x * zi * cam.f + cam.cx);
    e1 = v - (y * zi * cam.f + cam.cy);
    if (JAC) {
        const double f = cam.f, zi2 = zi * zi;
        const double t02 = -x * zi * f, t12 = -y * zi * f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Jl[c] = -zi * (f * T[c] + t02 * T[6 + c]);
            Jl[3 + c] = -zi * (f * T[3 + c] + t12 * T[6 + c]);
        }
        Jp[0] = x * y * zi2 * f; Jp[1] = -(1 + (x * x * zi2)) * f; Jp[2] = y * zi * f; Jp[3] = -zi * f; Jp[4] = 0; Jp[5] = x * zi2 * f;
        Jp[6] = (1 + y * y * zi2) * f; Jp[7] = -x * y * zi2 * f; Jp[8] = -x * zi * f; Jp[9] = 0; Jp[10] = -zi * f; Jp[11] = y * zi2 * f;
    }
}

}  // namespace
