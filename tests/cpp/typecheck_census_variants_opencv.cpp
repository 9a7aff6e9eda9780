// Type-check of the modified and the centre-symmetric census in the cv::Mat branch of include/adf_ximgproc.hpp against the
// declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked): the transform on a view, and a block matcher
// that is given one of the new costs.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

static_assert(ADF_BM_COST_MCT_DENSE == ADF_SGBM_COST_MCT_DENSE && ADF_BM_COST_MCT_SPARSE == ADF_SGBM_COST_MCT_SPARSE &&
              ADF_BM_COST_CENSUS_CS == ADF_SGBM_COST_CENSUS_CS, "the two matchers share the census constants");

void describe_view(const cv::Mat& view, cv::Mat& descriptors)
{
    adf::censusTransform(view, 5, descriptors, ADF_SGBM_COST_CENSUS_CS);
}

void match_views(const cv::Mat& left, const cv::Mat& right, cv::Mat& disparity)
{
    adf::Ptr<adf::ximgproc::StereoBM> bm = adf::ximgproc::StereoBM::create(16, 9);
    bm->setCostType(ADF_BM_COST_MCT_DENSE); bm->setCensusSize(3);
    bm->compute(left, right, disparity);
}
