// Type-check of adf::weightedMedianFilter in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration stubs in
// opencv_stub/ (g++ -fsyntax-only; never linked): the hole-filling step between the matcher's own checks and reprojection.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void fill_and_denoise(const cv::Mat& left_view, cv::Mat& disp, const cv::Mat& cost, const cv::Mat& mask, int min_disparity,
                      int num_disparities)
{
    adf::validateDisparity(disp, cost, min_disparity, num_disparities);
    cv::Mat filled, median, masked;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::weightedMedianFilter(left_view, disp, median, 3);                                    // cv's defaults: sigma 25.5, WMF_EXP, no mask
    adf::weightedMedianFilter(left_view, disp, masked, 3, 25.5, adf::WMF_OFF, mask);
    adf::weightedMedianFilter(left_view, disp, disp, 3);                                      // in place, as cv allows
}
