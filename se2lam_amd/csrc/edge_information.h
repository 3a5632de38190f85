// Map::loadLocalGraph's per-observation information (src/Map.cpp:1024-1049 of the reference), the arithmetic of one edge:
// shared by k_edge_information (csrc/ba.hip, the host-loaded graph) and k_local_ba_gather (csrc/local_ba_device.hip, the graph
// gathered from the tables in device memory), so the rule has one text.  The two files are compiled with different
// -ffp-contract settings (se2lam_amd/build.py): their results agree to rounding, not to the bit.
#pragma once
#include <hip/hip_runtime.h>

namespace se2gpu {

// lc = mViewMPs[ftrIdx], R = the rotation block of KeyFrame::Tcw (row-major), d = lw - (Twb.x, Twb.y, 0), s2 = mvLevelSigma2[octave],
// s_rot = 1 / PLANEMOTION_XROT_INFO and s_z = 1 / PLANEMOTION_Z_INFO as floats (:1043-1044).  Returns Sigma_all^-1 as (xx, xy, yy).
__device__ __forceinline__ void edge_information(double lc0, double lc1, double lc2, const double (&R)[9], double d0, double d1, double d2,
                                                 double s2, float fx, float s_rot, float s_z, double& xx, double& xy, double& yy) {
    const double zi = 1. / lc2, zi2 = zi * zi;
    const double j00 = fx * zi, j02 = -fx * lc0 * zi2, j12 = -fx * lc1 * zi2;
    double A[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A[c] = j00 * R[c] + j02 * R[6 + c];
        A[3 + c] = j00 * R[3 + c] + j12 * R[6 + c];
    }
    // (A * skew(d))[:, 0] = A[:,1]*d2 - A[:,2]*d1 ; [:, 1] = -A[:,0]*d2 + A[:,2]*d0
    const double r00 = A[1] * d2 - A[2] * d1, r01 = -A[0] * d2 + A[2] * d0;
    const double r10 = A[4] * d2 - A[5] * d1, r11 = -A[3] * d2 + A[5] * d0;
    const double z0 = -A[2], z1 = -A[5];
    const double S00 = s_rot * (r00 * r00 + r01 * r01) + s_z * z0 * z0 + s2;
    const double S01 = s_rot * (r00 * r10 + r01 * r11) + s_z * z0 * z1;
    const double S11 = s_rot * (r10 * r10 + r11 * r11) + s_z * z1 * z1 + s2;
    const double id = 1.0 / (S00 * S11 - S01 * S01);
    xx = S11 * id; xy = -S01 * id; yy = S00 * id;
}

}  // namespace se2gpu
