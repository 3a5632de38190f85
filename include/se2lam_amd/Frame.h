// The camera side of se2lam::Frame (the reference's include/se2lam/Frame.h, src/Frame.cpp) over libse2gpu's host functions.
//   void Frame::computeBoundUn(const Mat& K, const Mat& D)      (Frame.cpp:183-200) -> minXUn, minYUn, maxXUn, maxYUn
//   cv::undistortPoints(mat, mat, K, D, Mat(), K)               (its only third-party call, Frame.cpp:195)
// Frame itself is a pointer-graph class of the reference's data model (out of scope); what the matchers read from it is
// ORBmatcher.h's FrameView, and computeBoundUn below fills that view's bounds.  Frame::undistortKeyPoints is commented out
// in the reference (Frame.cpp:34) and has no mirror.  Host code: no device is needed.
#pragma once
#include "ORBmatcher.h"
#include "types.h"

namespace se2lam_amd {

// cv::undistortPoints(src, dst, K, D, cv::Mat(), K) on pixel coordinates (dst may be src)
inline void undistortPoints(const std::vector<Point2f>& src, std::vector<Point2f>& dst, const MatF& K, const MatF& D) {
    const se2gpu_camera c = toCamera(K, D);
    std::vector<Point2f> out(src.size());
    static_assert(sizeof(Point2f) == 2 * sizeof(float), "cv::Point2f layout");
    check(se2gpu_undistort_points(&c, src.empty() ? nullptr : &src[0].x, (int)src.size(), out.empty() ? nullptr : &out[0].x),
          "undistortPoints");
    dst.swap(out);
}

struct FrameBoundsUn {
    float minXUn = 0, minYUn = 0, maxXUn = 0, maxYUn = 0;
};

// Frame::computeBoundUn for an img of rows x cols: the image rectangle when D.at<float>(0) == 0, else the bounds of the
// four undistorted corners
inline FrameBoundsUn computeBoundUn(const MatF& K, const MatF& D, int rows, int cols) {
    const se2gpu_camera c = toCamera(K, D);
    se2gpu_frame_bounds b{};
    check(se2gpu_frame_bounds_un(&c, rows, cols, &b), "computeBoundUn");
    return FrameBoundsUn{b.min_x, b.min_y, b.max_x, b.max_y};
}

// ... straight into the view the matchers take
inline void computeBoundUn(FrameView& frame, const MatF& K, const MatF& D, int rows, int cols) {
    const FrameBoundsUn b = computeBoundUn(K, D, rows, cols);
    frame.minXUn = b.minXUn; frame.minYUn = b.minYUn; frame.maxXUn = b.maxXUn; frame.maxYUn = b.maxYUn;
}

}  // namespace se2lam_amd
