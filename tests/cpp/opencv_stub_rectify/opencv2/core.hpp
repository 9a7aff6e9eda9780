// COMPILE-ONLY declaration stub, layered over opencv_stub_calib3d/opencv2/core.hpp (see the notes there and in
// opencv_stub/): adds cv::Scalar and CV_32FC1, the two further cv:: names a caller of adf::remap / adf::rectifyViews /
// adf::initUndistortRectifyMap of include/adf_ximgproc.hpp writes (borderValue, m1type).  Put this directory in front of
// the other three on the include path (tests/test_cpp_rectify.py); declarations only, never linked or run.  Signatures
// and the value follow the public OpenCV API as documented (opencv2/core/types.hpp, opencv2/core/hal/interface.h).
#pragma once
#include "../../opencv_stub_calib3d/opencv2/core.hpp"

#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)

namespace cv {

template <class T> class Scalar_ {
public:
    Scalar_();
    Scalar_(T v0, T v1 = 0, T v2 = 0, T v3 = 0);
    const T& operator[](int i) const;
};
typedef Scalar_<double> Scalar;

} // namespace cv
