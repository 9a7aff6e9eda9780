// Type-check of adf::resize / adf::cvtColor in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration
// stubs in opencv_stub_imgproc/ (cv::Size) over opencv_stub/ (g++ -fsyntax-only; never linked): the lines of the sample's
// default pipeline that prepare the matcher's views (samples/disparity_filtering.cpp:130-141, 155-156).
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void views_for_the_matcher(const cv::Mat& left, const cv::Mat& right, cv::Mat& left_for_matcher, cv::Mat& right_for_matcher)
{
    adf::resize(left, left_for_matcher, cv::Size(), 0.5, 0.5);
    adf::resize(right, right_for_matcher, cv::Size(), 0.5, 0.5);
    adf::cvtColor(left_for_matcher, left_for_matcher, adf::COLOR_BGR2GRAY);
    adf::cvtColor(right_for_matcher, right_for_matcher, adf::COLOR_BGR2GRAY);
    cv::Mat again;
    adf::resize(left, again, cv::Size(adf::halfSize(left.cols), adf::halfSize(left.rows)), 0, 0, adf::INTER_LINEAR);
}
