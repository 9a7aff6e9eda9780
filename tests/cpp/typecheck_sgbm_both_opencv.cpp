// Type-check of StereoSGBM::computeBoth in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration stubs
// in opencv_stub/ (g++ -fsyntax-only; never linked): the sample's two compute calls (samples/disparity_filtering.cpp:
// 185-186) as one.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void both_views(const cv::Mat& left, const cv::Mat& right, cv::Mat& left_disp, cv::Mat& right_disp)
{
    adf::Ptr<adf::ximgproc::StereoSGBM> m = adf::ximgproc::StereoSGBM::create(0, 64, 3);
    m->computeBoth(left, right, left_disp, right_disp);
    m->computeBoth(left, right, left_disp, right_disp, ADF_SGBM_RIGHT_FROM_VOLUME);
}
