// MapPoint::mNormalVector under addObservation and eraseObservation, shared by map_apply.hip and the host mirror MapUpdate.h:
// the same text compiles for the device and for the host.  Self-contained: <cmath> only.
//   normal_add     MapPoint::addObservation     src/MapPoint.cpp:115-117
//   normal_erase   MapPoint::eraseObservation   src/MapPoint.cpp:89-90, :98-99
// Number formats follow the reference operation by operation: cv::norm(Point3f) is a double (the squares widened before they
// are multiplied), 1.f / norm is a double, Point3f * double multiplies in double and narrows each component; Point3f * float,
// the sum and the difference are float; 1.f / (float)size is one float division.
// Translation units that include this are compiled with -ffp-contract=off: a fused multiply-add would round differently.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SE2_MN_FN __host__ __device__ inline
#else
#define SE2_MN_FN inline
#endif

namespace se2gpu {

// Point3f normPos = viewPos * (1.f / cv::norm(viewPos))
SE2_MN_FN void unit_view(const float v[3], float u[3]) {
    const double x = v[0], y = v[1], z = v[2];
    const double s = 1.0 / sqrt(x * x + y * y + z * z);
    u[0] = (float)(x * s);
    u[1] = (float)(y * s);
    u[2] = (float)(z * s);
}

// mNormalVector = (mNormalVector * (float)oldObsSize + newNorm) * (1.f / (float)(oldObsSize + 1))
SE2_MN_FN void normal_add(float nv[3], const float view[3], int oldObsSize) {
    float u[3];
    unit_view(view, u);
    const float a = (float)oldObsSize, k = 1.f / (float)(oldObsSize + 1);
    for (int i = 0; i < 3; ++i) {
        const float scaled = nv[i] * a;
        const float sum = scaled + u[i];
        nv[i] = sum * k;
    }
}

// mNormalVector = (mNormalVector * (float)(size + 1) - normPos) * (1.f / (float)size), size = the list's length after the erase
SE2_MN_FN void normal_erase(float nv[3], const float view[3], int size) {
    float u[3];
    unit_view(view, u);
    const float a = (float)(size + 1), k = 1.f / (float)size;
    for (int i = 0; i < 3; ++i) {
        const float scaled = nv[i] * a;
        const float diff = scaled - u[i];
        nv[i] = diff * k;
    }
}

}  // namespace se2gpu
