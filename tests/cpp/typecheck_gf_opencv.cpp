// Type-check of adf::guidedFilter / adf::createGuidedFilter / adf::GuidedFilter in the cv::Mat branch of
// include/adf_ximgproc.hpp against the declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked): the smoothing
// step after the hole filling, and a float map refined through the left view.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void refine(const cv::Mat& left_view, cv::Mat& disp, const cv::Mat& learned, int min_disparity)
{
    cv::Mat filled, smooth, as_float, refined;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::guidedFilter(left_view, filled, smooth, 8, 100.0);                                   // cv's default dDepth: src's
    adf::guidedFilter(left_view, filled, as_float, 8, 100.0, CV_32F);
    adf::guidedFilter(left_view, disp, disp, 4, 1.0);                                         // in place, as cv allows
    cv::Ptr<adf::GuidedFilter> gf = adf::createGuidedFilter(left_view, 4, 6502.5);
    gf->filter(learned, refined);
    gf->filter(learned, refined, CV_16S);
}
