// Type-check of DisparityWLSFilter::filter / filterToFloat on CV_32FC1 disparity maps in the cv::Mat branch of
// include/adf_ximgproc.hpp against the declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked).
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

using namespace adf::ximgproc;

void refine_pipeline(const cv::Mat& left, const cv::Mat& dl_f32, const cv::Mat& dr_f32, cv::Mat& filtered_i16, cv::Mat& filtered_f32)
{
    cv::Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(true);
    wls->filter(dl_f32, left, filtered_i16, dr_f32);
    wls->filterToFloat(dl_f32, left, filtered_f32, dr_f32, cv::Rect(160, 0, 1760, 1080));
    wls->filterToFloat(filtered_f32, left, filtered_f32, dr_f32);      // (refused at run time: the maps may not be the output)
    cv::Ptr<DisparityWLSFilter> plain = createDisparityWLSFilterGeneric(false);
    plain->filterToFloat(dl_f32, left, filtered_f32);
}
