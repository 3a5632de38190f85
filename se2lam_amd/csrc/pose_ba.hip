// Localizer::DoLocalBA (/root/reference/src/Localizer.cpp:233-302) - SURVEY.md 8(f).2: pose-only bundle adjustment of
// the current key frame against the FIXED map points it observes.
//   graph   one VertexSE3Expmap (Tcw), one EdgeProjectXYZ2UV per observation (information invSigma2 * I, Huber with
//           delta = Config::TH_HUBER), one EdgeSE3ExpmapPrior built by addPlaneMotionSE3Expmap
//           (/root/reference/src/optimizer.cpp:236-314, 159-197); Levenberg-Marquardt, optimize(30)
//   [3P g2o 20160424]  EdgeProjectXYZ2UV::computeError / linearizeOplus and VertexSE3Expmap::oplusImpl
//           (types_six_dof_expmap), SE3Quat::exp / log / adj (se3quat.h), OptimizationAlgorithmLevenberg - the same
//           policy as the SE(2) bundle adjustment in ba.hip
// The system has six unknowns, so the whole optimize(30) is ONE launch of one workgroup: the threads share the edges
// (normal equations and robust chi2 by wave shuffles + LDS), thread 0 adds the prior, solves the damped 6x6 system
// (LL^T), applies exp(update) * estimate and runs the accept / reject logic; the key frame's pose and the statistics
// come back in one download.  Rotations are matrices, passed through a unit quaternion after every product and
// exponential the way SE3Quat renormalises its rotation.
#include "track_ws.h"
#include "pose_ba_device.h"

#include <cmath>
#include <limits>

namespace se2gpu {
namespace {

__global__ __launch_bounds__(256) void k_pose_ba(PoseParams P, const double* __restrict__ xyz, const double* __restrict__ uv,
                                                  const double* __restrict__ w, double* __restrict__ pose_out,
                                                  se2gpu_ba_stats* __restrict__ stats) {
    pose_ba_run(P, xyz, uv, w, pose_out, stats);
}

Se3 se3_from(const double* p) {
    Se3 T;
    std::memcpy(T.R, p, 9 * sizeof(double));
    std::memcpy(T.t, p + 9, 3 * sizeof(double));
    return T;
}

}  // namespace
}  // namespace se2gpu

using namespace se2gpu;

// addPlaneMotionSE3Expmap (optimizer.cpp:236-314, the branch that is compiled): graph construction on the host, by the text
// the device runs in k_localizer_ba (se3_math.h).
extern "C" int se2gpu_plane_motion_prior(const double* Tcw12, const double* Tbc12, double xrot_info, double yrot_info,
                                         double z_info, double* meas12, double* info36) {
    SE2_REQUIRE(Tcw12 && Tbc12 && meas12 && info36, SE2GPU_ERR_INVALID, "plane_motion_prior: NULL argument");
    plane_motion_prior_se3(Tcw12, Tbc12, xrot_info, yrot_info, z_info, meas12, info36);
    return SE2GPU_OK;
}

extern "C" int se2gpu_track_pose_ba(se2gpu_track* h, const double* Tcw12, const double* prior_meas12,
                                    const double* prior_info36, int n, const double* xyz, const double* uv,
                                    const double* inv_sigma2, double f, double cx, double cy, double huber_delta, int iters,
                                    double* Tcw_out12, se2gpu_ba_stats* stats) {
    SE2_REQUIRE(h && Tcw12 && prior_meas12 && prior_info36 && Tcw_out12, SE2GPU_ERR_INVALID, "pose_ba: NULL argument");
    SE2_REQUIRE(n >= 0 && iters >= 0, SE2GPU_ERR_INVALID, "pose_ba: negative size");
    SE2_REQUIRE(n == 0 || (xyz && uv && inv_sigma2), SE2GPU_ERR_INVALID, "pose_ba: NULL buffer");
    PoseParams P;
    P.est0 = se3_from(Tcw12);
    P.prior = se3_from(prior_meas12);
    std::memcpy(P.info, prior_info36, sizeof(P.info));
    P.f = f; P.cx = cx; P.cy = cy; P.delta = huber_delta;
    P.n = n; P.iters = iters;
    // one upload [xyz | uv | w], one download [pose (12) | stats]
    const size_t nn = (size_t)std::max(n, 1);
    const size_t in_b = nn * 6 * sizeof(double);
    const size_t out_b = 12 * sizeof(double) + sizeof(se2gpu_ba_stats);
    SE2_CHECK(h->h_in.reserve(in_b));
    SE2_CHECK(h->d_in.reserve(in_b));
    SE2_CHECK(h->h_out.reserve(out_b));
    SE2_CHECK(h->d_out.reserve(out_b));
    double* hi = (double*)h->h_in.p;
    if (n) {
        std::memcpy(hi, xyz, (size_t)n * 3 * sizeof(double));
        std::memcpy(hi + 3 * nn, uv, (size_t)n * 2 * sizeof(double));
        std::memcpy(hi + 5 * nn, inv_sigma2, (size_t)n * sizeof(double));
    }
    hipStream_t st = h->stream;
    SE2_HIP(hipMemcpyAsync(h->d_in.p, h->h_in.p, in_b, hipMemcpyHostToDevice, st));
    SE2_HIP(hipMemsetAsync(h->d_out.p, 0, out_b, st));
    const double* di = (const double*)h->d_in.p;
    hipLaunchKernelGGL(k_pose_ba, dim3(1), dim3(256), 0, st, P, di, di + 3 * nn, di + 5 * nn, (double*)h->d_out.p,
                       (se2gpu_ba_stats*)(h->d_out.p + 12 * sizeof(double)));
    SE2_HIP(hipGetLastError());
    SE2_HIP(hipMemcpyAsync(h->h_out.p, h->d_out.p, out_b, hipMemcpyDeviceToHost, st));
    SE2_HIP(hipStreamSynchronize(st));
    std::memcpy(Tcw_out12, h->h_out.p, 12 * sizeof(double));
    if (stats) std::memcpy(stats, h->h_out.p + 12 * sizeof(double), sizeof(se2gpu_ba_stats));
    return SE2GPU_OK;
}
