// Type-check of adf::jointBilateralFilter in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration stubs
// in opencv_stub/ (g++ -fsyntax-only; never linked): the refinement step after the hole filling, and a float map refined
// through the left view.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void refine(const cv::Mat& left_view, cv::Mat& disp, const cv::Mat& learned, int min_disparity)
{
    cv::Mat filled, smooth, refined;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::jointBilateralFilter(left_view, filled, smooth, 9, 25.0, 3.0);                       // BORDER_DEFAULT
    adf::jointBilateralFilter(left_view, filled, smooth, -1, 25.0, 8.0, adf::BORDER_REPLICATE);
    adf::jointBilateralFilter(left_view, disp, disp, 5, 40.0, 2.0, adf::BORDER_REFLECT);      // in place, as cv allows
    adf::jointBilateralFilter(left_view, learned, refined, 9, 25.0, 3.0, adf::BORDER_REFLECT_101);
}
