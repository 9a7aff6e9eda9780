// Type-check of adf::reprojectImageTo3D / adf::pointCloud in the cv::Mat branch of include/adf_ximgproc.hpp against the
// declaration stubs in opencv_stub_calib3d/ (CV_64F) over opencv_stub_imgproc/ and opencv_stub/ (g++ -fsyntax-only; never
// linked): the step a stereo pipeline takes after filtering, from the filtered map to metres.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

static_assert(adf::D64F == CV_64F, "the adaptor's depth code of Q");

size_t filtered_map_to_points(const cv::Mat& filtered_disp, const cv::Mat& filtered_f32, const cv::Mat& left, cv::Mat& xyz,
                              cv::Mat& depth, std::vector<float>& points, std::vector<uint8_t>& colours)
{
    cv::Mat Q(4, 4, CV_64F);
    adf::reprojectImageTo3D(filtered_disp, xyz, Q);                        // cv's call, cv's defaults
    adf::reprojectImageTo3D(filtered_disp, xyz, Q, true, CV_32F);
    const double fill = -16.0;
    adf::reprojectImageTo3D(filtered_f32, depth, Q, false, -1, 1.0 / 16, &fill, true);
    std::vector<int32_t> index;
    adf::pointCloud(filtered_disp, Q, points);
    return adf::pointCloud(filtered_f32, Q, points, &colours, left, cv::Rect(16, 0, 100, 50), 0.5, 80.0, false, 1.0 / 16, &fill, &index);
}
