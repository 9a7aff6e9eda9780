// Type-check of adf::validateDisparity in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration stubs in
// opencv_stub/ (g++ -fsyntax-only; never linked): the left-right check and the speckle filter a calib3d pipeline runs on
// StereoBM's map and cost.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void check_then_remove_speckles(cv::Mat& disp, const cv::Mat& cost, int min_disparity, int num_disparities, int disp12_max_diff,
                                int speckle_window, int speckle_range)
{
    if (disp12_max_diff >= 0) adf::validateDisparity(disp, cost, min_disparity, num_disparities, disp12_max_diff);
    adf::validateDisparity(disp, cost, min_disparity, num_disparities);                       // disp12MaxDiff = 1
    // the block matcher's call convention, modules/stereo/src/stereo_binary_bm.cpp:416-417: the range unscaled
    if (speckle_window > 0) adf::filterSpeckles(disp, (min_disparity - 1) * 16, speckle_window, speckle_range);
}
