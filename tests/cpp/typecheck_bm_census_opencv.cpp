// Type-check of the block matcher's census cost in the cv::Mat branch of include/adf_ximgproc.hpp against the declaration
// stubs in opencv_stub/ (g++ -fsyntax-only; never linked): the sample's fast pipeline (samples/disparity_filtering.cpp:
// 151-189) with the cost of cv::stereo::StereoBinaryBM (modules/stereo/src/stereo_binary_bm.cpp:367-408).
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

using namespace adf::ximgproc;

void census_pipeline(const cv::Mat& left, const cv::Mat& right, cv::Mat& filtered)
{
    adf::Ptr<StereoBM> bm = StereoBM::create(64, 9);
    bm->setCostType(ADF_BM_COST_CENSUS_SPARSE);
    bm->setCensusSize(9);
    adf::Ptr<DisparityWLSFilter> wls = createDisparityWLSFilter(bm);
    adf::Ptr<StereoBM> rbm = createRightMatcher(bm);
    const int cost = rbm->getCostType(), size = rbm->getCensusSize();
    (void)cost; (void)size;
    cv::Mat dl, dr;
    bm->compute(left, right, dl);
    rbm->compute(right, left, dr);
    wls->filter(dl, left, filtered, dr);
}
