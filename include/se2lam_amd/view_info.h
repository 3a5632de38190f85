// The arithmetic a new observation needs, shared by triangulate.hip and new_kf.hip (through csrc/view_info.h) and the host
// mirror FindCorrespd.h: the same text compiles for the device and for the host.  Self-contained: <cfloat> and <cmath> only.
//   smallest_right_singular_vector / triangulate_dlt   cvu::triangulate        src/cvutil.cpp:46-59
//   se3map                                              cvu::se3map             src/cvutil.cpp:100-105
//   check_parallax                                      cvu::checkParallax      src/cvutil.cpp:92-98
//   se3_to_xyz_info                                     Track::calcSE3toXYZInfo src/Track.cpp:259-306
//   accept_new_observe                                  MapPoint::acceptNewObserve src/MapPoint.cpp:202-209
// Number formats follow the reference operation by operation: Point3f / Matx33f products, cross and dot are float arithmetic
// in index order; cv::norm(Point3f) and cv::norm(scalar) are double and narrowed where the reference assigns to float;
// std::asin(float) is asinf; cv::Rodrigues computes in double and narrows (oracle/_shim/cv_shim.cpp:388-415); a cv::Mat
// product of float matrices sums each element in a double accumulator and stores a float (OpenCV's gemm for CV_32F and the
// shim's, cv_shim.cpp:131-142), so R.t() * info * R is two float matrices, each rounded once per element.
// Translation units that include this are compiled with -ffp-contract=off: a fused multiply-add would round differently.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define SE2_VI_FN __host__ __device__ inline
#else
#define SE2_VI_FN inline
#endif

namespace se2gpu {

// smallest right singular vector of the 4x4 matrix a (row-major); v4 = that vector (unnormalised sign)
SE2_VI_FN void smallest_right_singular_vector(const double a_in[16], double v4[4]) {
    double At[4][4], Vt[4][4], W[4];   // At: rows = columns of A (one-sided Jacobi works on A^T), Vt: accumulates V^T
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) {
            At[i][k] = a_in[k * 4 + i];
            Vt[i][k] = i == k ? 1.0 : 0.0;
        }
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
        for (int k = 0; k < 4; ++k) sd += At[i][k] * At[i][k];
        W[i] = sd;
    }
    const double eps = 2.220446049250313e-16 * 10;
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 4; ++j) {
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < 4; ++k) p += At[i][k] * At[j][k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = 0;
                b = 0;
                for (int k = 0; k < 4; ++k) {
                    const double t0 = c * At[i][k] + s * At[j][k];
                    const double t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0;
                    At[j][k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                for (int k = 0; k < 4; ++k) {
                    const double t0 = c * Vt[i][k] + s * Vt[j][k];
                    const double t1 = -s * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0;
                    Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
    int m = 0;
    for (int i = 1; i < 4; ++i)
        if (W[i] < W[m]) m = i;   // first minimum
    for (int k = 0; k < 4; ++k) v4[k] = Vt[m][k];
}

// cvu::triangulate(pt1, pt2, P1, P2): P1 / P2 are 3x4 row-major.  Rows in float as cv::Mat arithmetic forms them, then
// widened; one-sided Jacobi in FP64; the point dehomogenised in float.
SE2_VI_FN void triangulate_dlt(const float pt1[2], const float pt2[2], const float* P1, const float* P2, float x3d[3]) {
    const float x1 = pt1[0], y1 = pt1[1], x2 = pt2[0], y2 = pt2[1];
    double A[16];
    for (int c = 0; c < 4; ++c) {
        A[0 + c] = (double)(x1 * P1[8 + c] - P1[0 + c]);
        A[4 + c] = (double)(y1 * P1[8 + c] - P1[4 + c]);
        A[8 + c] = (double)(x2 * P2[8 + c] - P2[0 + c]);
        A[12 + c] = (double)(y2 * P2[8 + c] - P2[4 + c]);
    }
    double v[4];
    smallest_right_singular_vector(A, v);
    const float w = (float)v[3];
    x3d[0] = (float)v[0] / w;
    x3d[1] = (float)v[1] / w;
    x3d[2] = (float)v[2] / w;
}

// cvu::se3map: Matx33f * Point3f + Point3f on rows 0-2 of T (3x4 row-major)
SE2_VI_FN void se3map(const float* T, const float p[3], float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = (T[4 * i] * p[0] + T[4 * i + 1] * p[1] + T[4 * i + 2] * p[2]) + T[4 * i + 3];
}

SE2_VI_FN double norm3(const float v[3]) {   // cv::norm(Point3f)
    return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
}

SE2_VI_FN void cross3(const float a[3], const float b[3], float out[3]) {   // Point3f::cross
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

SE2_VI_FN float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }   // Point3f::dot

// cosParallax of cvu::checkParallax(o1, o2, pt3, .): the caller compares it with minCos[minDegree - 1]
SE2_VI_FN float cos_parallax(const float o1[3], const float o2[3], const float pt3[3]) {
    const float p1[3] = {pt3[0] - o1[0], pt3[1] - o1[1], pt3[2] - o1[2]};
    const float p2[3] = {pt3[0] - o2[0], pt3[1] - o2[1], pt3[2] - o2[2]};
    return (float)(fabs((double)dot3(p1, p2)) / (norm3(p1) * norm3(p2)));
}

// cv::Mat product of two 3x3 float matrices (row-major); out must not alias a or b
SE2_VI_FN void mat3_mul(const float a[9], const float b[9], float out[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += (double)a[3 * r + k] * (double)b[3 * k + c];
            out[3 * r + c] = (float)s;
        }
}

SE2_VI_FN void mat3_t(const float a[9], float out[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = a[3 * c + r];
}

// A^T * M * A as the reference writes it: (A.t() * M) * A
SE2_VI_FN void mat3_at_m_a(const float A[9], const float M[9], float out[9]) {
    float At[9], t[9];
    mat3_t(A, At);
    mat3_mul(At, M, t);
    mat3_mul(t, A, out);
}

// A * M * A^T: (A * M) * A.t()
SE2_VI_FN void mat3_a_m_at(const float A[9], const float M[9], float out[9]) {
    float At[9], t[9];
    mat3_t(A, At);
    mat3_mul(A, M, t);
    mat3_mul(t, At, out);
}

// rows 0-2, columns 0-2 of a 3x4 row-major pose
SE2_VI_FN void rot_of(const float* T, float R[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * r + c];
}

// cv::Rodrigues, rotation vector -> matrix, of a CV_32F vector
SE2_VI_FN void rodrigues(const float k[3], float R[9]) {
    const double r0 = (double)k[0], r1 = (double)k[1], r2 = (double)k[2];
    const double theta = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    double Rd[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!(theta < DBL_EPSILON)) {
        const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
        const double x = r0 * itheta, y = r1 * itheta, z = r2 * itheta;
        const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
        const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int i = 0; i < 9; ++i) Rd[i] = c * I[i] + c1 * rrt[i] + s * rx[i];
    }
    for (int i = 0; i < 9; ++i) R[i] = (float)Rd[i];
}

// The information of one view: R.t() * diag(1/dxy^2, 1/dxy^2, 1/dz^2) * R, R turning the ray xyz onto the z axis
// (Track.cpp:276-304 for one of the two views).  A point exactly on the optical axis has k = 0 * (0 / 0) = NaN in the
// reference and here.
SE2_VI_FN void view_info(const float xyz[3], float length, float dxy, float dz, float info[9]) {
    const float ixy = 1.f / (dxy * dxy), iz = 1.f / (dz * dz);
    const float D[9] = {ixy, 0.f, 0.f, 0.f, ixy, 0.f, 0.f, 0.f, iz};
    const float z[3] = {0.f, 0.f, length};
    float k[3];
    cross3(xyz, z, k);
    const float normk = (float)norm3(k);
    const float sn = (float)((double)normk / (norm3(z) * norm3(xyz)));
    const float f = asinf(sn) / normk;
    k[0] = k[0] * f;
    k[1] = k[1] * f;
    k[2] = k[2] * f;
    float R[9];
    rodrigues(k, R);
    mat3_at_m_a(R, D, info);
}

// Track::calcSE3toXYZInfo(xyz1, Tcw1, Tcw2, info1, info2) with the inverse poses supplied: Twc1 = cvu::inv(Tcw1),
// Twc2 = cvu::inv(Tcw2), all 3x4 row-major; the camera centres are column 3 of Twc.  info1 / info2: 3x3 row-major floats
// (the reference widens them to Eigen::Matrix3d).  xyz2: the point in the second camera (may be NULL).
SE2_VI_FN void se3_to_xyz_info(const float xyz1[3], const float* Twc1, const float* Tcw2, const float* Twc2, float fx,
                               float info1[9], float info2[9], float* xyz2_out) {
    const float O1[3] = {Twc1[3], Twc1[7], Twc1[11]}, O2[3] = {Twc2[3], Twc2[7], Twc2[11]};
    float xyz[3];
    se3map(Twc1, xyz1, xyz);
    const float vO1[3] = {xyz[0] - O1[0], xyz[1] - O1[1], xyz[2] - O1[2]};
    const float vO2[3] = {xyz[0] - O2[0], xyz[1] - O2[1], xyz[2] - O2[2]};
    float cr[3];
    cross3(vO1, vO2, cr);
    const float sinParallax = (float)(norm3(cr) / (norm3(vO1) * norm3(vO2)));
    float xyz2[3];
    se3map(Tcw2, xyz, xyz2);
    const float length1 = (float)norm3(xyz1), length2 = (float)norm3(xyz2);
    const float dxy1 = 2.f * length1 / fx, dxy2 = 2.f * length2 / fx;
    const float dz1 = dxy2 / sinParallax, dz2 = dxy1 / sinParallax;
    view_info(xyz1, length1, dxy1, dz1, info1);
    view_info(xyz2, length2, dxy2, dz2, info2);
    if (xyz2_out) {
        xyz2_out[0] = xyz2[0];
        xyz2_out[1] = xyz2[1];
        xyz2_out[2] = xyz2[2];
    }
}

// MapPoint::acceptNewObserve(posKF, kp): normal = mNormalVector, main_octave = the main observation's octave
SE2_VI_FN bool accept_new_observe(const float posKF[3], const float normal[3], int main_octave, int kp_octave,
                                  float min_dist, float max_dist) {
    const float dist = (float)norm3(posKF);
    const float cosAngle = (float)(fabs((double)dot3(posKF, normal)) / ((double)dist * norm3(normal)));
    const long long d = (long long)main_octave - (long long)kp_octave;
    const bool c1 = (d < 0 ? -d : d) <= 2;
    const bool c2 = cosAngle >= 0.866f;
    const bool c3 = dist >= min_dist && dist <= max_dist;
    return c1 && c2 && c3;
}

}  // namespace se2gpu
