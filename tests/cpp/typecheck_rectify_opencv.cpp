// Type-check of adf::initUndistortRectifyMap / adf::remap / adf::rectifyViews in the cv::Mat branch of
// include/adf_ximgproc.hpp against the declaration stubs in opencv_stub_rectify/ (cv::Scalar, CV_32FC1) over
// opencv_stub_calib3d/, opencv_stub_imgproc/ and opencv_stub/ (g++ -fsyntax-only; never linked): the step a stereo
// pipeline takes first, from the camera's frames to rectified views.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

static_assert(adf::M32FC1 == CV_32FC1, "the adaptor's code of the one map type that is built");

void frames_to_rectified_views(const cv::Mat& left, const cv::Mat& right, cv::Mat& left_rect, cv::Mat& right_rect)
{
    cv::Mat K1(3, 3, CV_64F), D1(1, 5, CV_64F), R1(3, 3, CV_64F), P1(3, 4, CV_64F);   // the caller's stereoRectify made R1, P1
    cv::Mat K2(3, 3, CV_64F), D2(1, 5, CV_64F), R2(3, 3, CV_64F), P2(3, 4, CV_64F);
    cv::Mat map1, map2;
    adf::initUndistortRectifyMap(K1, D1, R1, P1, cv::Size(1242, 375), CV_32FC1, map1, map2);   // cv's two calls ...
    adf::remap(left, left_rect, map1, map2);
    adf::remap(left, left_rect, map1, map2, adf::INTER_LINEAR, adf::BORDER_CONSTANT, cv::Scalar(7, 200, 99));
    adf::rectifyViews(right, right_rect, K2, D2, R2, P2, cv::Size());                          // ... or one, per frame
    adf::rectifyViews(right, right_rect, K2, cv::Mat(), cv::Mat(), cv::Mat(), cv::Size(1242, 375), cv::Scalar(0));
}
