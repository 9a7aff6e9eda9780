// Type-check of adf::censusTransform in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration stubs in
// opencv_stub/ (g++ -fsyntax-only; never linked): the call cv::stereo's matchers make on each view
// (modules/stereo/src/descriptor.cpp:77-98).
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void describe_view(const cv::Mat& view, cv::Mat& descriptors)
{
    adf::censusTransform(view, 9, descriptors, ADF_SGBM_COST_CENSUS_SPARSE);
}
