// COMPILE-ONLY declaration stub, layered over opencv_stub_imgproc/opencv2/core.hpp (see the notes there and in
// opencv_stub/): adds CV_64F, the depth of the matrix Q that adf::reprojectImageTo3D / adf::pointCloud of
// include/adf_ximgproc.hpp accept besides CV_32F.  Put this directory in front of the other two on the include path
// (tests/test_cpp_reproject.py); declarations only, never linked or run.  Value as in the public OpenCV API
// (opencv2/core/hal/interface.h).
#pragma once
#include "../../opencv_stub_imgproc/opencv2/core.hpp"

#define CV_64F 6
