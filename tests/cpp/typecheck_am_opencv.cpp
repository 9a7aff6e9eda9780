// Type-check of adf::amFilter / adf::createAMFilter / adf::AdaptiveManifoldFilter in the cv::Mat branch of
// include/adf_ximgproc.hpp against the declaration stubs in opencv_stub/ (g++ -fsyntax-only; never linked): the reference's
// calls ported by changing the namespace alone, apart from UseRNG.
#include "adf_ximgproc.hpp"

#if !defined(ADF_HAVE_OPENCV)
#error "the OpenCV branch was not selected: check the include path of the stub"
#endif

void refine(const cv::Mat& left_view, cv::Mat& disp, int min_disparity)
{
    cv::Mat filled, smooth;
    adf::weightedMedianFilter(left_view, disp, filled, 7, 10.0, adf::WMF_EXP, cv::Mat(), (min_disparity - 1) * 16.0);
    adf::amFilter(left_view, filled, smooth, 16.0, 0.2);
    adf::amFilter(left_view, filled, smooth, 40.0, 0.1, true);
    adf::amFilter(left_view, disp, disp, 16.0, 0.2);                                          // in place, as cv allows
    cv::Ptr<adf::AdaptiveManifoldFilter> f = adf::createAMFilter(16.0, 0.2, true);
    f->filter(filled, smooth, left_view);
    cv::Ptr<adf::AdaptiveManifoldFilter> g = adf::AdaptiveManifoldFilter::create();
    g->setSigmaS(32.0);
    g->setSigmaR(0.15);
    g->setTreeHeight(4);
    g->setPCAIterations(2);
    g->setAdjustOutliers(!g->getAdjustOutliers());
    g->setUseRNG(false);                                                                      // true is refused: not built
    g->filter(filled, smooth, left_view);
    g->collectGarbage();
    const double product = g->getSigmaS() * g->getSigmaR() * g->getTreeHeight() * g->getPCAIterations();
    (void)product;
    (void)g->getUseRNG();
}
