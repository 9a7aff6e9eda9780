// Type-check of adf::dtWindowFilter / adf::createDTWindowFilter / adf::DTWindowFilter in the cv::Mat branch of
// include/adf_ximgproc.hpp against the declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked): a reference
// call ported without naming a mode, and how a binding routes the mode it is handed.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void refine(const cv::Mat& left_view, cv::Mat& disp, const cv::Mat& learned, int min_disparity)
{
    cv::Mat filled, smooth, refined;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::dtWindowFilter(left_view, filled, smooth, 10.0, 30.0);                               // DTF_NC, three iterations
    adf::dtWindowFilter(left_view, filled, smooth, 80.0, 50.0, adf::DTF_NC, 3);
    adf::dtWindowFilter(left_view, disp, disp, 40.0, 10.0);                                   // in place, as cv allows
    cv::Ptr<adf::DTWindowFilter> f = adf::createDTWindowFilter(left_view, 10.0, 30.0, adf::DTF_NC, 3);
    f->filter(learned, refined);
    f->filter(learned, refined, CV_16S);
}

void routed(const cv::Mat& guide, const cv::Mat& src, cv::Mat& dst, double sigmaSpatial, double sigmaColor, int mode, int numIters)
{
    if (mode == adf::DTF_NC) adf::dtWindowFilter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters);
    else adf::dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters);            // DTF_RF; DTF_IC is refused there
}
