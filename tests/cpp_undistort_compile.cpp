// include/se2lam_amd/Frame.h and ORBextractor::setCamera compile as plain C++17 and link against libse2gpu
// (tests/test_undistort.py).  Without a device the host functions run (undistortPoints, computeBoundUn) and the extractor
// says there is no device; with one, an extractor that carries the identity camera gives what one without a camera gives,
// and a distorting camera gives something else.  Prints the bounds for the Python side to compare with its model:
//   BOUNDS <minXUn> <minYUn> <maxXUn> <maxYUn>      (%.9g: round-trips a float)
#include <cstdio>
#include <cstring>
#include <vector>

#include "se2lam_amd/Frame.h"
#include "se2lam_amd/ORBextractor.h"

using namespace se2lam_amd;

static bool same(const std::vector<KeyPoint>& a, const std::vector<KeyPoint>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(KeyPoint)) == 0);
}

int main() {
    const int rows = 480, cols = 640;
    MatF K = MatF::eye(3);
    K.at<float>(0, 0) = 524.8f; K.at<float>(1, 1) = 531.2f; K.at<float>(0, 2) = 321.7f; K.at<float>(1, 2) = 237.7f;
    MatF D(5, 1), D0(4, 1), Dk2(1, 4);
    const float d5[5] = {-0.30f, 0.10f, 5e-4f, -4e-4f, -0.015f};
    for (int i = 0; i < 5; ++i) D.at<float>(i, 0) = d5[i];
    Dk2.at<float>(0, 1) = 0.07f;                               // k1 == 0, k2 != 0

    // Frame::computeBoundUn (Frame.cpp:183-200) and the cv::undistortPoints line inside it
    const FrameBoundsUn b = computeBoundUn(K, D, rows, cols);
    std::vector<Point2f> mat(4);
    mat[1].x = (float)cols; mat[2].y = (float)rows; mat[3].x = (float)cols; mat[3].y = (float)rows;
    undistortPoints(mat, mat, K, D);
    if (b.minXUn != std::min(mat[0].x, mat[2].x) || b.minYUn != std::min(mat[0].y, mat[1].y) ||
        b.maxXUn != std::max(mat[1].x, mat[3].x) || b.maxYUn != std::max(mat[2].y, mat[3].y)) return 2;
    if (!(b.minXUn < 0 && b.minYUn < 0 && b.maxXUn > cols && b.maxYUn > rows)) return 3;   // barrel distortion: the corners move out
    std::printf("BOUNDS %.9g %.9g %.9g %.9g\n", b.minXUn, b.minYUn, b.maxXUn, b.maxYUn);
    FrameView fv;
    computeBoundUn(fv, K, Dk2, rows, cols);                    // decided by k1 alone
    if (fv.minXUn != 0.f || fv.minYUn != 0.f || fv.maxXUn != (float)cols || fv.maxYUn != (float)rows) return 4;
    computeBoundUn(fv, K, D0, rows, cols);
    if (fv.minXUn != 0.f || fv.maxYUn != (float)rows) return 5;
    try {
        (void)toCamera(K, MatF(6, 1));
        return 6;
    } catch (const std::invalid_argument&) {
    }

    if (se2gpu_device_count() <= 0) {
        try {
            ORBextractor none;
            return 7;
        } catch (const std::runtime_error&) {
        }
        std::printf("OK (no device: the host functions ran)\n");
        return 0;
    }

    // a raw image with corners: a checker of 24 px squares under a gradient
    std::vector<uint8_t> px((size_t)rows * cols);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) px[(size_t)y * cols + x] = (uint8_t)((((x / 24) + (y / 24)) & 1 ? 150 : 40) + (x + y) / 16);
    Mat8U im;
    im.rows = rows; im.cols = cols; im.step = (size_t)cols; im.data = px.data();
    ORBextractor plain, withCam;
    std::vector<KeyPoint> k0, k1, k2, k3;
    Mat8U d0, d1, d2, d3;
    plain(im, Mat8U(), k0, d0);
    withCam.setCamera(K, D0);                                  // the kernel runs over the identity map
    withCam(im, Mat8U(), k1, d1);
    if (k0.empty() || !same(k0, k1) || d0.owned != d1.owned) return 8;
    withCam.setCamera(K, D);                                   // Frame::Frame: undistort(im, img, Kcam, Dcam); (*extractor)(img, ...)
    withCam(im, Mat8U(), k2, d2);
    if (k2.empty() || same(k0, k2)) return 9;
    withCam.clearCamera();
    withCam(im, Mat8U(), k3, d3);
    if (!same(k0, k3) || d0.owned != d3.owned) return 10;
    std::printf("OK (device: %zu key points, %zu through the camera)\n", k0.size(), k2.size());
    return 0;
}
