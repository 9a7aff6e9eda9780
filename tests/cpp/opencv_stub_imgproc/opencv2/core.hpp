// COMPILE-ONLY declaration stub, layered over opencv_stub/opencv2/core.hpp (see the note there): adds cv::Size, the one
// further cv:: name that adf::resize of include/adf_ximgproc.hpp touches in its OpenCV branch.  Put this directory in
// front of opencv_stub on the include path (tests/test_cpp_view_prep.py); declarations only, never linked or run.
// Signature follows the public OpenCV API as documented (opencv2/core/types.hpp).
#pragma once
#include "../../opencv_stub/opencv2/core.hpp"

namespace cv {

template <class T> class Size_ {
public:
    Size_();
    Size_(T width, T height);
    T width, height;
};
typedef Size_<int> Size;

} // namespace cv
