// Type-check of DisparityWLSFilter::filterToFloat in the cv::Mat branch of include/adf_ximgproc.hpp against the
// declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked).
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

using namespace adf::ximgproc;

void depth_pipeline(const cv::Mat& left, const cv::Mat& dl, const cv::Mat& dr, cv::Mat& filtered_f32)
{
    cv::Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(true);
    wls->filterToFloat(dl, left, filtered_f32, dr);
    wls->filterToFloat(dl, left, filtered_f32, dr, cv::Rect(160, 0, 1760, 1080));
    cv::Ptr<DisparityWLSFilter> plain = createDisparityWLSFilterGeneric(false);
    plain->filterToFloat(dl, left, filtered_f32);
}
