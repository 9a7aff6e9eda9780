// Type-check of adf::dtFilter / adf::createDTFilter / adf::DTFilter in the cv::Mat branch of include/adf_ximgproc.hpp
// against the declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked): the refinement step after the hole
// filling, and a float map refined through the left view.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void refine(const cv::Mat& left_view, cv::Mat& disp, const cv::Mat& learned, int min_disparity)
{
    cv::Mat filled, smooth, refined;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::dtFilter(left_view, filled, smooth, 10.0, 30.0);                                     // DTF_RF, three iterations
    adf::dtFilter(left_view, filled, smooth, 10.0, 30.0, adf::DTF_RF, 2);
    adf::dtFilter(left_view, disp, disp, 40.0, 10.0);                                         // in place, as cv allows
    cv::Ptr<adf::DTFilter> f = adf::createDTFilter(left_view, 10.0, 30.0, adf::DTF_RF, 3);
    f->filter(learned, refined);
    f->filter(learned, refined, CV_16S);
}
