// Type-check of adf::rollingGuidanceFilter in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration
// stubs in opencv_stub/ (g++ -fsyntax-only; never linked): the smoothing step after the hole filling, with the reference's
// defaults and with every argument given.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void smooth(const cv::Mat& left_view, cv::Mat& disp, const cv::Mat& learned, int min_disparity)
{
    cv::Mat filled, rolled, refined;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::rollingGuidanceFilter(filled, rolled);                                               // d = -1, 25, 3, 4, BORDER_DEFAULT
    adf::rollingGuidanceFilter(filled, rolled, 9, 40.0, 4.0, 3, adf::BORDER_REPLICATE);
    adf::rollingGuidanceFilter(disp, disp, -1, 25.0, 3.0, 2, adf::BORDER_REFLECT);            // in place, as cv allows
    adf::rollingGuidanceFilter(learned, refined, 5, 0.5, 2.0);
}
