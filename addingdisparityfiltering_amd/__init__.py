"""MI355X-native DisparityWLSFilter / FastGlobalSmootherFilter.

The package mirrors cv::ximgproc's interface for this one path and calls hand-written HIP kernels
through the C-ABI of include/adf_wls.h.  Importing the API does not load the library; the first
filter construction does, and fails loudly if libadf_wls.so has not been built.
"""
from .ximgproc import (  # noqa: F401
    AdfError,
    COLOR_BGR2GRAY,
    CV_32F,
    DisparityFilter,
    DisparityWLSFilter,
    FastGlobalSmootherFilter,
    INTER_LINEAR,
    PATH_CONF_BAND,
    PATH_FUSED_FIRST_PASS,
    PATH_MERGED_PREP,
    PATH_ROW_WEIGHTS_GUIDE,
    PATH_SCALED_FUSED,
    PATH_SCALED_HALF,
    SGBM_COST_BT,
    SGBM_COST_CENSUS_DENSE,
    SGBM_COST_CENSUS_SPARSE,
    SOLVER_EXACT,
    SOLVER_WAVE,
    StereoBM,
    StereoMatcher,
    StereoSGBM,
    UNKNOWN_DISPARITY,
    censusTransform,
    computeBadPixelPercent,
    computeMSE,
    createDisparityWLSFilter,
    createDisparityWLSFilterGeneric,
    createFastGlobalSmootherFilter,
    createRightMatcher,
    cvtColor,
    fastGlobalSmootherFilter,
    filterSpeckles,
    releaseCachedMemory,
    getDisparityVis,
    halfSize,
    matcherViews,
    pointCloud,
    pointCloudWorkspaceBytes,
    readGT,
    reprojectImageTo3D,
    reprojectWorkspaceBytes,
    resize,
    speckleWorkspaceBytes,
)

__version__ = "0.1.0"
