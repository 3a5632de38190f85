// Test introspection of se3_math.h: one function of the header per thread, on the device, compiled with the flags ba.hip and
// ba_window3.hip are compiled with (build.py: no per-file entry), so that what a test reads here is the arithmetic those
// translation units inline.
#include "common.h"
#include "se3_math.h"

namespace se2gpu {
namespace {

constexpr int kIn = 24, kOut = 36;   // doubles per item, whatever the op: the pose12 pairs and the 6x6 results fit

__global__ void k_debug_se3(int op, int n, const double* __restrict__ in, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* x = in + (size_t)kIn * i;
    double* y = out + (size_t)kOut * i;
    for (int k = 0; k < kOut; ++k) y[k] = 0;
    switch (op) {
    case SE2GPU_SE3_EXP: se3_store(se3_exp(x), y); break;
    case SE2GPU_SE3_LOG: se3_log(se3_load(x), y); break;
    case SE2GPU_SE3_MUL: se3_store(se3_mul(se3_load(x), se3_load(x + 12)), y); break;
    case SE2GPU_SE3_NORMALIZE: {
        double R[9];
        for (int k = 0; k < 9; ++k) R[k] = x[k];
        normalize_rotation(R);
        for (int k = 0; k < 9; ++k) y[k] = R[k];
        break;
    }
    case SE2GPU_SE3_QUAT_OF: quat_of(x, y); break;
    case SE2GPU_SE3_TO_MQT: to_mqt(se3_load(x), y); break;
    case SE2GPU_SE3_FROM_MQT: se3_store(from_mqt(x), y); break;
    case SE2GPU_SE3_ADJ: se3_adj(se3_load(x), y); break;
    case SE2GPU_SE3_JAC_RIGHT: mqt_jac_right(se3_load(x), y); break;
    case SE2GPU_SE3_JAC_LEFT_INV: mqt_jac_left_inv(se3_load(x), se3_load(x + 12), y); break;
    case SE2GPU_SE3_LOG_EXP: se3_log(se3_exp(x), y); break;
    default: break;
    }
}

}  // namespace
}  // namespace se2gpu

extern "C" int se2gpu_debug_se3(int op, int n, const double* in, double* out) {
    using namespace se2gpu;
    const char* who = "se2gpu_debug_se3";
    SE2_REQUIRE(op >= 0 && op < SE2GPU_SE3_OPS, SE2GPU_ERR_INVALID, "%s: op %d is none of the %d", who, op, (int)SE2GPU_SE3_OPS);
    SE2_REQUIRE(n >= 0 && n <= (1 << 20), SE2GPU_ERR_INVALID, "%s: n = %d outside [0, 2^20]", who, n);
    if (n == 0) return SE2GPU_OK;
    SE2_NEED(in);
    SE2_NEED(out);
    SE2_NEED_DEVICE();
    DevBuf<double> d_in, d_out;
    SE2_CHECK(d_in.reserve((size_t)kIn * n));
    SE2_CHECK(d_out.reserve((size_t)kOut * n));
    SE2_HIP(hipMemcpy(d_in.p, in, sizeof(double) * kIn * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_se3, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, d_in.p, d_out.p);
    SE2_HIP(hipGetLastError());
    SE2_HIP(hipMemcpy(out, d_out.p, sizeof(double) * kOut * n, hipMemcpyDeviceToHost));
    return SE2GPU_OK;
}
