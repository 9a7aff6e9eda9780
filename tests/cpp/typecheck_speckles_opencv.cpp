// Type-check of adf::filterSpeckles in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration stubs in
// opencv_stub/ (g++ -fsyntax-only; never linked): the call a calib3d pipeline makes after StereoBM / StereoSGBM.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void remove_speckles_after_matching(cv::Mat& disp, int min_disparity, int speckle_window, int speckle_range)
{
    // the in-tree call convention, modules/stereo/src/stereo_binary_sgbm.cpp:716-718
    adf::filterSpeckles(disp, (min_disparity - 1) * 16, speckle_window, 16 * speckle_range);
}
