// adf_ximgproc.hpp -- header-only C++ adaptor: the reference's operator interface over the C-ABI.
//
// Mirrors cv::ximgproc for the disparity-filter path -- same class and function names, argument
// order and meaning, defaults and error behaviour (exceptions) as
//   modules/ximgproc/include/opencv2/ximgproc/disparity_filter.hpp  (DF.hpp:52-149)
//   modules/ximgproc/include/opencv2/ximgproc/edge_filter.hpp       (EF.hpp:361-413)
// so that a stereo pipeline switches by changing a namespace.  All compute happens in
// libadf_wls.so (HIP kernels); this header only marshals cv::Mat-like images into adf_wls.h calls.
//
// With OpenCV available (opencv2/core.hpp on the include path) the types are cv::Mat / cv::Rect /
// cv::Ptr and the matcher factories take cv::StereoMatcher.  Without it (this repo's CI image has no
// OpenCV) a minimal Mat / Rect stands in and the matcher factories take the three numbers they read.
#pragma once

#include "adf_wls.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#if !defined(ADF_NO_OPENCV) && defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define ADF_HAVE_OPENCV 1
#if __has_include(<opencv2/calib3d.hpp>)
#include <opencv2/calib3d.hpp>
#define ADF_HAVE_CALIB3D 1
#endif
#endif
#endif

namespace adf {

// cv::Exception counterpart: CV_Assert / CV_Error sites of DF.cpp:221-222,262-264, FGS.cpp:143-144,184-189.
struct Exception : std::runtime_error {
    int code;
    Exception(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) { if (rc != ADF_OK) throw Exception(rc, adf_last_error()); }

#ifdef ADF_HAVE_OPENCV
using Mat = cv::Mat;
using Rect = cv::Rect;
template <class T> using Ptr = cv::Ptr<T>;
enum { D8U = CV_8U, D16S = CV_16S, D32S = 4 /* CV_32S */, D32F = CV_32F, D64F = 6 /* CV_64F */ };
inline int mat_depth(const Mat& m) { return m.depth(); }
inline int mat_channels(const Mat& m) { return m.channels(); }
inline ptrdiff_t mat_step(const Mat& m) { return (ptrdiff_t)m.step; }
inline void mat_create(Mat& m, int rows, int cols, int depth, int cn) { m.create(rows, cols, CV_MAKETYPE(depth, cn)); }
#else
struct Rect {
    int x = 0, y = 0, width = 0, height = 0;
    Rect() {}
    Rect(int x_, int y_, int w_, int h_) : x(x_), y(y_), width(w_), height(h_) {}
    int area() const { return width * height; }
};
enum { D8U = 0, D16S = 3, D32S = 4, D32F = 5, D64F = 6 }; // cv depth codes
// Minimal dense image: shared buffer, header copies share data (like cv::Mat).
struct Mat {
    int rows = 0, cols = 0, depth_ = D8U, cn = 1;
    size_t step = 0;
    unsigned char* data = nullptr;
    std::shared_ptr<std::vector<unsigned char>> buf;
    Mat() {}
    Mat(int r, int c, int depth, int channels = 1) { create(r, c, depth, channels); }
    static size_t esz(int depth) { return depth == D8U ? 1 : depth == D16S ? 2 : depth == D64F ? 8 : 4; }
    void create(int r, int c, int depth, int channels = 1)
    {
        if (r == rows && c == cols && depth == depth_ && channels == cn && data) return;
        rows = r; cols = c; depth_ = depth; cn = channels;
        step = (size_t)c * channels * esz(depth);
        buf = std::make_shared<std::vector<unsigned char>>(step * (size_t)r);
        data = buf->data();
    }
    bool empty() const { return !data || rows == 0 || cols == 0; }
    template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data + step * (size_t)r); }
    template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data + step * (size_t)r); }
};
template <class T> using Ptr = std::shared_ptr<T>;
inline int mat_depth(const Mat& m) { return m.depth_; }
inline int mat_channels(const Mat& m) { return m.cn; }
inline ptrdiff_t mat_step(const Mat& m) { return (ptrdiff_t)m.step; }
inline void mat_create(Mat& m, int rows, int cols, int depth, int cn) { m.create(rows, cols, depth, cn); }
#endif

// cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) of calib3d (outside the reference tree; parity unpinned, see
// adf_filter_speckles_* in adf_wls.h) on a CV_16SC1 host Mat, in place, through the library's host entry.  newVal and
// maxDiff are rounded half-to-even (cvRound) before they reach the C-ABI; CV_8UC1 is not supported.
inline void filterSpeckles(Mat& img, double newVal, int maxSpeckleSize, double maxDiff)
{
    if (img.empty() || mat_depth(img) != D16S || mat_channels(img) != 1)
        throw Exception(ADF_EBADARG, "filterSpeckles: img must be a non-empty CV_16SC1 image (CV_8UC1 is not supported)");
    if (!(newVal >= -32768.5 && newVal <= 32767.5))                           // (NaN fails too)
        throw Exception(ADF_EBADARG, "filterSpeckles: newVal is outside the CV_16S range");
    const double nv = std::nearbyint(newVal);                                 // default rounding mode: half to even
    if (nv < -32768.0 || nv > 32767.0) throw Exception(ADF_EBADARG, "filterSpeckles: newVal is outside the CV_16S range");
    if (std::isnan(maxDiff)) throw Exception(ADF_EBADARG, "filterSpeckles: maxDiff is NaN");
    const double md = std::fmin(std::fmax(std::nearbyint(maxDiff), -2147483647.0), 2147483647.0);
    check(adf_filter_speckles_host(1, reinterpret_cast<int16_t*>(img.data), mat_step(img), 0, img.cols, img.rows,
                                   (int)nv, maxSpeckleSize, (int)md));
}

// calib3d's validateDisparity(disparity, cost, minDisparity, numberOfDisparities, disp12MaxDiff) (outside the reference
// tree; parity unpinned, see adf_validate_disparity_* in adf_wls.h), the block matcher's own left-right check: a CV_16SC1
// host Mat, in place, and the CV_16SC1 or CV_32SC1 cost of each winning disparity (StereoBM::computeWithCost below),
// through the library's host entry.  A negative disp12MaxDiff is refused: "off" is the matcher's business.
inline void validateDisparity(Mat& disparity, const Mat& cost, int minDisparity, int numberOfDisparities, int disp12MaxDiff = 1)
{
    if (disparity.empty() || mat_depth(disparity) != D16S || mat_channels(disparity) != 1)
        throw Exception(ADF_EBADARG, "validateDisparity: disparity must be a non-empty CV_16SC1 image");
    if (cost.empty() || (mat_depth(cost) != D16S && mat_depth(cost) != D32S) || mat_channels(cost) != 1)
        throw Exception(ADF_EBADARG, "validateDisparity: cost must be a non-empty CV_16SC1 or CV_32SC1 image");
    if (cost.rows != disparity.rows || cost.cols != disparity.cols)
        throw Exception(ADF_ESIZE, "validateDisparity: cost must have the disparity map's size");
    check(adf_validate_disparity_host(1, reinterpret_cast<int16_t*>(disparity.data), mat_step(disparity), 0, cost.data, mat_step(cost), 0,
                                      mat_depth(cost) == D16S ? ADF_16S : ADF_32S, disparity.cols, disparity.rows,
                                      minDisparity, numberOfDisparities, disp12MaxDiff));
}

// cv::ximgproc::weightedMedianFilter(joint, src, dst, r, sigma, weightType, mask) (weighted_median_filter.hpp:64-90) on host
// Mats through the library's host entry, in the library's own integer definition (adf_weighted_median_filter_* in
// adf_wls.h: fixed-point weights, the exact colour distance of a 3-channel joint, no quantisation of CV_16S / CV_32F
// sources).  joint: CV_8UC1 or CV_8UC3; src: CV_8UC1, CV_16SC1 or CV_32FC1 of its size (multi-channel sources are not built:
// split them); mask: empty or CV_8UC1, 0 = ignored.  WMF_EXP and WMF_OFF are built; WMF_IV1, WMF_IV2, WMF_COS and WMF_JAC
// are refused.  The overload with ignoreValue (extension) also ignores -- and so fills from their neighbours -- the pixels
// that hold it: (minDisparity - 1) * 16 for a matcher's map after validateDisparity / filterSpeckles.
enum WMFWeightType { WMF_EXP, WMF_IV1, WMF_IV2, WMF_COS, WMF_JAC, WMF_OFF }; // cv's values
// What the five edge-aware filters below ask of their Mats, said once; `who` is the function's name in the texts.
inline void filter_src(const std::string& who, const Mat& src)
{
    if (src.empty() || mat_channels(src) != 1 || (mat_depth(src) != D8U && mat_depth(src) != D16S && mat_depth(src) != D32F))
        throw Exception(ADF_EBADARG, who + ": src must be a non-empty CV_8UC1, CV_16SC1 or CV_32FC1 image");
}
inline void filter_guide(const std::string& who, const std::string& role, const Mat& guide, const Mat& src)   // role: "guide" or "joint"
{
    if (guide.empty() || mat_depth(guide) != D8U) throw Exception(ADF_EBADARG, who + ": " + role + " must be a non-empty CV_8UC1 or CV_8UC3 image");
    if (guide.rows != src.rows || guide.cols != src.cols) throw Exception(ADF_ESIZE, who + ": " + role + " must have src's size");
}
inline int filter_ddepth(const std::string& who, const Mat& src, int dDepth)   // the depth dDepth asks for: -1 is src's
{
    const int ddepth = dDepth == -1 ? mat_depth(src) : dDepth;
    if (ddepth != D8U && ddepth != D16S && ddepth != D32F) throw Exception(ADF_EBADARG, who + ": dDepth must be -1, CV_8U, CV_16S or CV_32F");
    return ddepth;
}
inline int depth_code(int depth) { return depth == D8U ? ADF_8U : depth == D16S ? ADF_16S : ADF_32F; }   // cv's depth as the C-ABI's
inline Mat filter_out(const Mat& src, int depth) { Mat out; mat_create(out, src.rows, src.cols, depth, 1); return out; }   // a new Mat: dst may be src
inline Mat guide_copy(const std::string& who, const Mat& guide)   // a filter object's own dense copy of the guide it accepts
{
    if (guide.empty() || mat_depth(guide) != D8U || (mat_channels(guide) != 1 && mat_channels(guide) != 3))
        throw Exception(ADF_EBADARG, who + ": guide must be a non-empty CV_8UC1 or CV_8UC3 image");
    Mat own;
    mat_create(own, guide.rows, guide.cols, D8U, mat_channels(guide));
    for (int y = 0; y < guide.rows; y++)
        std::memcpy(own.data + (size_t)mat_step(own) * y, guide.data + (size_t)mat_step(guide) * y, (size_t)guide.cols * mat_channels(guide));
    return own;
}

inline void weighted_median(const Mat& joint, const Mat& src, Mat& dst, int r, double sigma, int weightType, const Mat& mask,
                            const double* ignoreValue)
{
    filter_src("weightedMedianFilter", src);
    filter_guide("weightedMedianFilter", "joint", joint, src);
    if (!mask.empty() && (mat_depth(mask) != D8U || mat_channels(mask) != 1))
        throw Exception(ADF_EBADARG, "weightedMedianFilter: mask must be empty or a CV_8UC1 image");
    if (!mask.empty() && (mask.rows != src.rows || mask.cols != src.cols)) throw Exception(ADF_ESIZE, "weightedMedianFilter: mask must have src's size");
    Mat out = filter_out(src, mat_depth(src));
    check(adf_weighted_median_filter_host(1, joint.data, mat_step(joint), 0, mat_channels(joint), src.data, mat_step(src), 0, depth_code(mat_depth(src)),
                                          out.data, mat_step(out), 0, src.cols, src.rows, r, sigma, weightType,
                                          mask.empty() ? nullptr : mask.data, mask.empty() ? 0 : mat_step(mask), 0,
                                          ignoreValue ? 1 : 0, ignoreValue ? *ignoreValue : 0.0));
    dst = out;
}
inline void weightedMedianFilter(const Mat& joint, const Mat& src, Mat& dst, int r, double sigma = 25.5, int weightType = WMF_EXP,
                                 const Mat& mask = Mat())
{
    weighted_median(joint, src, dst, r, sigma, weightType, mask, nullptr);
}
inline void weightedMedianFilter(const Mat& joint, const Mat& src, Mat& dst, int r, double sigma, int weightType, const Mat& mask,
                                 double ignoreValue)
{
    weighted_median(joint, src, dst, r, sigma, weightType, mask, &ignoreValue);
}

// cv::ximgproc::guidedFilter(guide, src, dst, radius, eps, dDepth) (EF.hpp:180), createGuidedFilter(guide, radius, eps)
// (EF.hpp:158) and GuidedFilter::filter(src, dst, dDepth) (EF.hpp:143) on host Mats through the library's host entry, in
// the library's own definition (adf_guided_filter_* in adf_wls.h: exact integer statistics, one stated operation order,
// BORDER_REFLECT).  guide: CV_8UC1 or CV_8UC3; src: CV_8UC1, CV_16SC1 or CV_32FC1 of its size (multi-channel sources are
// not built: split them); dDepth: -1 (src's depth), CV_8U, CV_16S or CV_32F; 0 <= radius <= ADF_GF_MAX_RADIUS; eps > 0 in
// squared grey levels of the 0..255 guide.  dst may be src.  The filter is not blind to a matcher's invalid value: run
// weightedMedianFilter with ignoreValue first.
inline void guidedFilter(const Mat& guide, const Mat& src, Mat& dst, int radius, double eps, int dDepth = -1)
{
    filter_src("guidedFilter", src);
    filter_guide("guidedFilter", "guide", guide, src);
    const int ddepth = filter_ddepth("guidedFilter", src, dDepth);
    Mat out = filter_out(src, ddepth);
    check(adf_guided_filter_host(1, guide.data, mat_step(guide), 0, mat_channels(guide), src.data, mat_step(src), 0, depth_code(mat_depth(src)),
                                 out.data, mat_step(out), 0, depth_code(ddepth), src.cols, src.rows, radius, eps));
    dst = out;
}

class GuidedFilter {
public:
    virtual ~GuidedFilter() {}
    virtual void filter(const Mat& src, Mat& dst, int dDepth = -1) = 0;
};

// Holds its own copy of the guide (made first: the caller's Mat may change or go away, as with cv's) and the parameters; the guide's
// statistics are recomputed per call -- they ride along in the coefficient kernel -- so the object saves no work.
class GuidedFilterImpl : public GuidedFilter {
    Mat guide_;
    int radius_;
    double eps_;
public:
    GuidedFilterImpl(const Mat& guide, int radius, double eps) : guide_(guide_copy("createGuidedFilter", guide)), radius_(radius), eps_(eps)
    {
        if (radius < 0 || radius > ADF_GF_MAX_RADIUS) throw Exception(ADF_EBADARG, "createGuidedFilter: radius must lie in [0, 31]");
        if (!std::isfinite(eps) || !(eps > 0.0)) throw Exception(ADF_EBADARG, "createGuidedFilter: eps must be finite and > 0");
    }
    void filter(const Mat& src, Mat& dst, int dDepth = -1) override { guidedFilter(guide_, src, dst, radius_, eps_, dDepth); }
};

inline Ptr<GuidedFilter> createGuidedFilter(const Mat& guide, int radius, double eps)
{
    return Ptr<GuidedFilter>(new GuidedFilterImpl(guide, radius, eps));
}

// cv::ximgproc::dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters) (EF.hpp:121), createDTFilter(guide,
// sigmaSpatial, sigmaColor, mode, numIters) (EF.hpp:102) and DTFilter::filter(src, dst, dDepth) (EF.hpp:79) on host Mats
// through the library's host entry, in mode DTF_RF and the library's own definition (adf_dt_filter_* in adf_wls.h: the
// recurrence in the reference's order, a feedback table with one rounding per entry).  guide: CV_8UC1 or CV_8UC3; src:
// CV_8UC1, CV_16SC1 or CV_32FC1 of its size (multi-channel sources are not built: split them); dDepth: -1 (src's depth),
// CV_8U, CV_16S or CV_32F.  DTF_NC and DTF_IC are refused here as not built -- so the default mode HERE is DTF_RF, not the
// reference's DTF_NC, which is dtWindowFilter / createDTWindowFilter below.  dst may be src.  The filter is not blind to a matcher's invalid value: run weightedMedianFilter
// with ignoreValue first.
enum EdgeAwareFiltersList { DTF_NC, DTF_IC, DTF_RF }; // cv's values
inline void dt_filter(const Mat& guide, const Mat& src, Mat& dst, double sigmaSpatial, double sigmaColor, int mode, int numIters, int dDepth)
{
    filter_src("dtFilter", src);
    filter_guide("dtFilter", "guide", guide, src);
    const int ddepth = filter_ddepth("dtFilter", src, dDepth);
    Mat out = filter_out(src, ddepth);
    check(adf_dt_filter_host(1, guide.data, mat_step(guide), 0, mat_channels(guide), src.data, mat_step(src), 0, depth_code(mat_depth(src)),
                             out.data, mat_step(out), 0, depth_code(ddepth), src.cols, src.rows, sigmaSpatial, sigmaColor, mode, numIters));
    dst = out;
}
inline void dtFilter(const Mat& guide, const Mat& src, Mat& dst, double sigmaSpatial, double sigmaColor, int mode = DTF_RF, int numIters = 3)
{
    dt_filter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters, -1);
}

class DTFilter {
public:
    virtual ~DTFilter() {}
    virtual void filter(const Mat& src, Mat& dst, int dDepth = -1) = 0;
};

// Holds its own copy of the guide (the caller's Mat may change or go away, as with cv's) and the parameters.  There is no
// init stage: the weights are one table read per step, recomputed from the guide in every sweep.
class DTFilterImpl : public DTFilter {
    Mat guide_;
    double sigmaSpatial_, sigmaColor_;
    int mode_, numIters_;
public:
    DTFilterImpl(const Mat& guide, double sigmaSpatial, double sigmaColor, int mode, int numIters)
        : guide_(guide_copy("createDTFilter", guide)), sigmaSpatial_(sigmaSpatial), sigmaColor_(sigmaColor), mode_(mode), numIters_(numIters)
    {
        if (mode != DTF_RF) throw Exception(ADF_EBADARG, "createDTFilter: mode must be DTF_RF (DTF_NC and DTF_IC are not built)");
        if (!std::isfinite(sigmaSpatial) || !std::isfinite(sigmaColor)) throw Exception(ADF_EBADARG, "createDTFilter: the sigmas must be finite");
        if (numIters > ADF_DT_MAX_ITERS) throw Exception(ADF_EBADARG, "createDTFilter: numIters must not exceed 8");
    }
    void filter(const Mat& src, Mat& dst, int dDepth = -1) override
    {
        dt_filter(guide_, src, dst, sigmaSpatial_, sigmaColor_, mode_, numIters_, dDepth);
    }
};

inline Ptr<DTFilter> createDTFilter(const Mat& guide, double sigmaSpatial, double sigmaColor, int mode = DTF_RF, int numIters = 3)
{
    return Ptr<DTFilter>(new DTFilterImpl(guide, sigmaSpatial, sigmaColor, mode, numIters));
}

// cv::ximgproc::dtFilter / createDTFilter / DTFilter::filter in mode DTF_NC -- the reference's default -- on host Mats
// through the library's host entry, under names of their own (dtFilter above keeps refusing DTF_NC), in the library's own
// definition (adf_dt_window_filter_* in adf_wls.h: a local distance with one rounding, every window summed directly).
// guide, src, dDepth and dst are dtFilter's.  The default mode is DTF_NC, as the reference's; DTF_RF is dtFilter's and
// DTF_IC is not built: both are refused, and so is a sigmaSpatial whose first radius exceeds ADF_DT_NC_MAX_RADIUS pixels
// (84 at 3 iterations still passes).  A binding of the reference routes mode == DTF_NC here and mode == DTF_RF to dtFilter.
inline void dt_window_filter(const Mat& guide, const Mat& src, Mat& dst, double sigmaSpatial, double sigmaColor, int mode, int numIters, int dDepth)
{
    filter_src("dtWindowFilter", src);
    filter_guide("dtWindowFilter", "guide", guide, src);
    const int ddepth = filter_ddepth("dtWindowFilter", src, dDepth);
    Mat out = filter_out(src, ddepth);
    check(adf_dt_window_filter_host(1, guide.data, mat_step(guide), 0, mat_channels(guide), src.data, mat_step(src), 0, depth_code(mat_depth(src)),
                                    out.data, mat_step(out), 0, depth_code(ddepth), src.cols, src.rows, sigmaSpatial, sigmaColor, mode, numIters));
    dst = out;
}
inline void dtWindowFilter(const Mat& guide, const Mat& src, Mat& dst, double sigmaSpatial, double sigmaColor, int mode = DTF_NC, int numIters = 3)
{
    dt_window_filter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters, -1);
}

class DTWindowFilter {
public:
    virtual ~DTWindowFilter() {}
    virtual void filter(const Mat& src, Mat& dst, int dDepth = -1) = 0;
};

// Holds its own copy of the guide (the caller's Mat may change or go away, as with cv's) and the parameters.  There is no
// init stage: the distances are summed from the guide in every pass.
class DTWindowFilterImpl : public DTWindowFilter {
    Mat guide_;
    double sigmaSpatial_, sigmaColor_;
    int mode_, numIters_;
public:
    DTWindowFilterImpl(const Mat& guide, double sigmaSpatial, double sigmaColor, int mode, int numIters)
        : guide_(guide_copy("createDTWindowFilter", guide)), sigmaSpatial_(sigmaSpatial), sigmaColor_(sigmaColor), mode_(mode), numIters_(numIters)
    {
        if (mode != DTF_NC) throw Exception(ADF_EBADARG, "createDTWindowFilter: mode must be DTF_NC (DTF_RF is createDTFilter's, DTF_IC is not built)");
        if (!std::isfinite(sigmaSpatial) || !std::isfinite(sigmaColor)) throw Exception(ADF_EBADARG, "createDTWindowFilter: the sigmas must be finite");
        if (numIters > ADF_DT_MAX_ITERS) throw Exception(ADF_EBADARG, "createDTWindowFilter: numIters must not exceed 8");
        float radii[ADF_DT_MAX_ITERS];
        check(adf_dt_nc_radii_host(sigmaSpatial, numIters, radii));
        if (!(radii[0] < (float)(ADF_DT_NC_MAX_RADIUS + 1))) throw Exception(ADF_EBADARG, "createDTWindowFilter: the first iteration's radius exceeds 127 pixels");
    }
    void filter(const Mat& src, Mat& dst, int dDepth = -1) override
    {
        dt_window_filter(guide_, src, dst, sigmaSpatial_, sigmaColor_, mode_, numIters_, dDepth);
    }
};

inline Ptr<DTWindowFilter> createDTWindowFilter(const Mat& guide, double sigmaSpatial, double sigmaColor, int mode = DTF_NC, int numIters = 3)
{
    return Ptr<DTWindowFilter>(new DTWindowFilterImpl(guide, sigmaSpatial, sigmaColor, mode, numIters));
}

// cv::ximgproc::amFilter(joint, src, dst, sigma_s, sigma_r, adjust_outliers) (EF.hpp:280), createAMFilter(sigma_s, sigma_r,
// adjust_outliers) (EF.hpp:259) and AdaptiveManifoldFilter (EF.hpp:203-245) on host Mats through the library's host entry,
// in the library's own definition (adf_am_filter_* in adf_wls.h: a complete tree of manifolds, its own exp, every operation
// in a stated order).  joint: CV_8UC1 or CV_8UC3, never empty (the reference then filters src by itself: not built); src:
// CV_8UC1, CV_16SC1 or CV_32FC1 of its size; dst gets src's depth and may be src.  sigma_s >= 1; 0 < sigma_r <= 1, the
// joint taken as 0 .. 1.  Where this departs from the reference: UseRNG is false and setUseRNG(true) is refused (the
// reference's default is true); PCAIterations is stored, clamped to >= 1, and does not change the result.
inline void am_filter(const Mat& joint, const Mat& src, Mat& dst, double sigma_s, double sigma_r, int tree_height, bool adjust_outliers)
{
    filter_src("amFilter", src);
    if (joint.empty()) throw Exception(ADF_EBADARG, "amFilter: joint must not be empty (filtering src by itself is not built)");
    filter_guide("amFilter", "joint", joint, src);
    Mat out = filter_out(src, mat_depth(src));
    check(adf_am_filter_host(1, joint.data, mat_step(joint), 0, mat_channels(joint), src.data, mat_step(src), 0, depth_code(mat_depth(src)),
                             out.data, mat_step(out), 0, depth_code(mat_depth(src)), src.cols, src.rows, sigma_s, sigma_r, tree_height,
                             adjust_outliers ? 1 : 0));
    dst = out;
}
inline void amFilter(const Mat& joint, const Mat& src, Mat& dst, double sigma_s, double sigma_r, bool adjust_outliers = false)
{
    am_filter(joint, src, dst, sigma_s, sigma_r, -1, adjust_outliers);
}

class AdaptiveManifoldFilter {
public:
    virtual ~AdaptiveManifoldFilter() {}
    virtual void filter(const Mat& src, Mat& dst, const Mat& joint = Mat()) = 0;
    virtual void collectGarbage() = 0;
    static Ptr<AdaptiveManifoldFilter> create();
    virtual double getSigmaS() const = 0;
    virtual void setSigmaS(double val) = 0;
    virtual double getSigmaR() const = 0;
    virtual void setSigmaR(double val) = 0;
    virtual int getTreeHeight() const = 0;
    virtual void setTreeHeight(int val) = 0;
    virtual int getPCAIterations() const = 0;
    virtual void setPCAIterations(int val) = 0;
    virtual bool getAdjustOutliers() const = 0;
    virtual void setAdjustOutliers(bool val) = 0;
    virtual bool getUseRNG() const = 0;
    virtual void setUseRNG(bool val) = 0;
};

// Holds the parameters alone: the tree is rebuilt from the joint in every call.
class AdaptiveManifoldFilterImpl : public AdaptiveManifoldFilter {
    double sigma_s_ = 16.0, sigma_r_ = 0.2;
    int tree_height_ = -1, pca_iterations_ = 1;
    bool adjust_outliers_ = false;
public:
    void filter(const Mat& src, Mat& dst, const Mat& joint = Mat()) override
    {
        am_filter(joint, src, dst, sigma_s_, sigma_r_, tree_height_, adjust_outliers_);
    }
    void collectGarbage() override {}
    double getSigmaS() const override { return sigma_s_; }
    void setSigmaS(double val) override { sigma_s_ = val; }
    double getSigmaR() const override { return sigma_r_; }
    void setSigmaR(double val) override { sigma_r_ = val; }
    int getTreeHeight() const override { return tree_height_; }
    void setTreeHeight(int val) override { tree_height_ = val; }
    int getPCAIterations() const override { return pca_iterations_; }
    void setPCAIterations(int val) override { pca_iterations_ = val < 1 ? 1 : val; }
    bool getAdjustOutliers() const override { return adjust_outliers_; }
    void setAdjustOutliers(bool val) override { adjust_outliers_ = val; }
    bool getUseRNG() const override { return false; }
    void setUseRNG(bool val) override
    {
        if (val) throw Exception(ADF_EBADARG, "amFilter: UseRNG is not built; the start vector is (0.5, -0.5, 0.5)");
    }
};

inline Ptr<AdaptiveManifoldFilter> AdaptiveManifoldFilter::create() { return Ptr<AdaptiveManifoldFilter>(new AdaptiveManifoldFilterImpl()); }

inline Ptr<AdaptiveManifoldFilter> createAMFilter(double sigma_s, double sigma_r, bool adjust_outliers = false)
{
    Ptr<AdaptiveManifoldFilter> f = AdaptiveManifoldFilter::create();
    f->setSigmaS(sigma_s);
    f->setSigmaR(sigma_r);
    f->setAdjustOutliers(adjust_outliers);
    return f;
}

// cv::ximgproc::jointBilateralFilter(joint, src, dst, d, sigmaColor, sigmaSpace, borderType) (EF.hpp:317) on host Mats
// through the library's host entry, in the library's own definition (adf_joint_bilateral_filter_* in adf_wls.h: the
// reference's `_8u` arithmetic in its order of evaluation, widened to CV_16S and CV_32F sources).  joint: CV_8UC1 or
// CV_8UC3 (CV_32F joints are not built); src: CV_8UC1, CV_16SC1 or CV_32FC1 of its size (multi-channel sources are not
// built: split them); dst gets src's depth and may be src.  d > 0: radius d / 2; d <= 0: cvRound(1.5 sigmaSpace); at most
// ADF_JBF_MAX_RADIUS.  borderType: BORDER_REPLICATE, BORDER_REFLECT or BORDER_REFLECT_101 (= BORDER_DEFAULT, cv's and the
// default here); BORDER_CONSTANT and BORDER_WRAP are not built and refused.  An empty joint or joint == src, which the
// reference hands to cv::bilateralFilter, is refused.  The filter is not blind to a matcher's invalid value: run
// weightedMedianFilter with ignoreValue first.  (BORDER_CONSTANT is declared with remap below.)
enum BorderTypes { BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 }; // cv's values
inline void jointBilateralFilter(const Mat& joint, const Mat& src, Mat& dst, int d, double sigmaColor, double sigmaSpace,
                                 int borderType = BORDER_DEFAULT)
{
    filter_src("jointBilateralFilter", src);
    if (joint.empty() || mat_depth(joint) != D8U)              // (its own: joint == src is said between the two of filter_guide)
        throw Exception(ADF_EBADARG, "jointBilateralFilter: joint must be a non-empty CV_8UC1 or CV_8UC3 image (an empty or CV_32F joint is not built)");
    if (joint.data == src.data)
        throw Exception(ADF_EBADARG, "jointBilateralFilter: joint == src is cv::bilateralFilter, which is not built");
    if (joint.rows != src.rows || joint.cols != src.cols) throw Exception(ADF_ESIZE, "jointBilateralFilter: joint must have src's size");
    const int depth = depth_code(mat_depth(src));
    Mat out = filter_out(src, mat_depth(src));                           // (dst may be joint too)
    check(adf_joint_bilateral_filter_host(1, joint.data, mat_step(joint), 0, mat_channels(joint), src.data, mat_step(src), 0, depth,
                                          out.data, mat_step(out), 0, depth, src.cols, src.rows, d, sigmaColor, sigmaSpace, borderType));
    dst = out;
}

// cv::ximgproc::rollingGuidanceFilter(src, dst, d, sigmaColor, sigmaSpace, numOfIter, borderType) (EF.hpp:350) on host Mats
// through the library's host entry, in the library's own definition (adf_rolling_guidance_filter_* in adf_wls.h): numOfIter
// joint bilateral filters of src, each with the previous result -- kept in src's depth -- as the joint, the first with src
// itself.  src: CV_8UC1, CV_16SC1 or CV_32FC1 (multi-channel sources are not built: split them); dst gets src's type and
// may be src (the result lands in a new Mat).  d, sigmaSpace and borderType as for jointBilateralFilter above; sigmaColor
// is in the map's own units; numOfIter 0 .. ADF_RGF_MAX_ITERS, 0 copies src.  CV_32F maps interpolate a constant grid laid
// over 16 sigmaColor, not over the joint's min-max range as the reference does, and take no Gaussian shortcut when
// uniform.  The filter is not blind to a matcher's invalid value: run weightedMedianFilter with ignoreValue first.
inline void rollingGuidanceFilter(const Mat& src, Mat& dst, int d = -1, double sigmaColor = 25, double sigmaSpace = 3, int numOfIter = 4,
                                  int borderType = BORDER_DEFAULT)
{
    filter_src("rollingGuidanceFilter", src);
    Mat out = filter_out(src, mat_depth(src));
    check(adf_rolling_guidance_filter_host(1, src.data, mat_step(src), 0, out.data, mat_step(out), 0, depth_code(mat_depth(src)), src.cols, src.rows, d,
                                           sigmaColor, sigmaSpace, numOfIter, borderType));
    dst = out;
}

// cv::stereo::censusTransform(image, kernelSize, dist, type) (modules/stereo descriptor.hpp:428, descriptor.cpp:77-98) on a
// CV_8UC1 host Mat, through the library's host entry: the census descriptor of every pixel, type
// ADF_SGBM_COST_CENSUS_DENSE (kernelSize 3, 5, 7), ADF_SGBM_COST_CENSUS_SPARSE (5, 7, 9, 11), the modified census
// ADF_SGBM_COST_MCT_DENSE (3, 5, 7) / ADF_SGBM_COST_MCT_SPARSE (5, 7, 9, 11) or the centre-symmetric
// ADF_SGBM_COST_CENSUS_CS (3, 5, 7, 9); definition, bit order
// and why it is not bit parity with the in-tree code: adf_census_transform_* in adf_wls.h.  A descriptor has up to 48
// bits, and cv::Mat has no 64-bit integer depth, so dist is CV_32SC2: one uint64 per pixel in the machine's byte order
// (channel 0 the low half), read with dist.ptr<uint64_t>(y)[x].
inline void censusTransform(const Mat& image, int kernelSize, Mat& dist, int type)
{
    if (image.empty() || mat_depth(image) != D8U || mat_channels(image) != 1)                 // descriptor.cpp:81
        throw Exception(ADF_EBADARG, "censusTransform: image must be a non-empty CV_8UC1 image");
    Mat out;
    mat_create(out, image.rows, image.cols, D32S, 2);
    check(adf_census_transform_host(1, image.data, mat_step(image), 0, image.cols, image.rows, type, kernelSize,
                                    reinterpret_cast<uint64_t*>(out.data), mat_step(out), 0));
    dist = out;
}

// The two imgproc calls in front of the matcher in the sample's default pipeline (samples/disparity_filtering.cpp:130-141;
// adf_prepare_views_* in adf_wls.h) on host Mats, through the library's host entry.  Same limits as the C-ABI:
//   resize    CV_8UC1 / CV_8UC3, INTER_LINEAR, fx == fy == 0.5 or the dsize that scale gives (halfSize of both axes):
//             the 2x2 mean (a + b + c + d + 2) >> 2; odd sizes: adf_wls.h (parity unpinned)
//   cvtColor  COLOR_BGR2GRAY on CV_8UC3: (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14
// src and dst may be the same Mat, as in the sample.
// dsize is cv::Size with OpenCV (a template parameter, so that this header asks nothing of opencv2/core.hpp that the
// rest of it does not use) and the stand-in below without.
#ifndef ADF_HAVE_OPENCV
struct Size {
    int width = 0, height = 0;
    Size() {}
    Size(int w, int h) : width(w), height(h) {}
};
#endif
enum { INTER_LINEAR = 1, COLOR_BGR2GRAY = 6 }; // cv's values

inline int halfSize(int n) { int h = 0; check(adf_half_size(n, &h)); return h; } // cvRound(n * 0.5)

template <class SizeT>
inline void resize(const Mat& src, Mat& dst, SizeT dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR)
{
    if (src.empty() || mat_depth(src) != D8U || (mat_channels(src) != 1 && mat_channels(src) != 3))
        throw Exception(ADF_EBADARG, "resize: src must be a non-empty CV_8UC1 or CV_8UC3 image");
    if (interpolation != INTER_LINEAR) throw Exception(ADF_EBADARG, "resize: INTER_LINEAR at a scale of exactly 0.5 only");
    const int w = halfSize(src.cols), h = halfSize(src.rows);
    if (dsize.width != 0 || dsize.height != 0) {
        if (dsize.width != w || dsize.height != h) throw Exception(ADF_EBADARG, "resize: half size only (dsize must be halfSize of both axes)");
    } else if (!(fx == 0.5 && fy == 0.5)) {
        throw Exception(ADF_EBADARG, "resize: fx == fy == 0.5 only");
    }
    if (w < 1 || h < 1) throw Exception(ADF_EBADARG, "resize: the half-size image is empty");
    Mat out;
    mat_create(out, h, w, D8U, mat_channels(src));
    check(adf_prepare_views_host(1, src.data, mat_step(src), 0, src.cols, src.rows, mat_channels(src),
                                 out.data, mat_step(out), 0, w, h, mat_channels(src)));
    dst = out;
}

inline void cvtColor(const Mat& src, Mat& dst, int code, int dstCn = 0)
{
    if (code != COLOR_BGR2GRAY || (dstCn != 0 && dstCn != 1)) throw Exception(ADF_EBADARG, "cvtColor: COLOR_BGR2GRAY only");
    if (src.empty() || mat_depth(src) != D8U || mat_channels(src) != 3)
        throw Exception(ADF_EBADARG, "cvtColor: src must be a non-empty CV_8UC3 image");
    Mat out;
    mat_create(out, src.rows, src.cols, D8U, 1);
    check(adf_prepare_views_host(1, src.data, mat_step(src), 0, src.cols, src.rows, 3, out.data, mat_step(out), 0,
                                 src.cols, src.rows, 1));
    dst = out;
}

// cv::reprojectImageTo3D(disparity, _3dImage, Q, handleMissingValues, ddepth) of calib3d (outside the reference tree;
// parity unpinned) and the point list, on host Mats through the library's host entries: definition, missing values and
// what "valid" means are adf_reproject_* / adf_point_cloud_* in adf_wls.h.  disparity: CV_16SC1 or CV_32FC1; Q: 4x4, CV_32F
// or CV_64F; ddepth: -1 or CV_32F.  Extensions after cv's arguments: dispScale multiplies the raw value first (1/16 for the
// filters' fixed-point units), missingValue names the missing value instead of the map's minimum (-16 for filterToFloat
// output), zOnly gives the CV_32FC1 Z plane alone.
inline adf_reproject_params reproject_params(const char* who, const Mat& Q, bool handleMissingValues, double dispScale,
                                             const double* missingValue)
{
    if (Q.empty() || Q.rows != 4 || Q.cols != 4 || mat_channels(Q) != 1 || (mat_depth(Q) != D32F && mat_depth(Q) != D64F))
        throw Exception(ADF_EBADARG, std::string(who) + ": Q must be a 4x4 CV_32F or CV_64F matrix");
    adf_reproject_params p;
    for (int r = 0; r < 4; r++) {
        const unsigned char* row = Q.data + (size_t)mat_step(Q) * r;
        for (int c = 0; c < 4; c++)
            p.Q[4 * r + c] = mat_depth(Q) == D64F ? reinterpret_cast<const double*>(row)[c] : (double)reinterpret_cast<const float*>(row)[c];
    }
    p.disp_scale = dispScale;
    p.missing_mode = missingValue ? ADF_MISSING_VALUE : handleMissingValues ? ADF_MISSING_MIN : ADF_MISSING_NONE;
    p.missing_value = missingValue ? *missingValue : 0.0;
    return p;
}

inline int reproject_depth(const char* who, const Mat& disparity)
{
    if (disparity.empty() || mat_channels(disparity) != 1 || (mat_depth(disparity) != D16S && mat_depth(disparity) != D32F))
        throw Exception(ADF_EBADARG, std::string(who) + ": disparity must be a non-empty CV_16SC1 or CV_32FC1 image");
    return mat_depth(disparity) == D16S ? ADF_16S : ADF_32F;
}

inline void reprojectImageTo3D(const Mat& disparity, Mat& _3dImage, const Mat& Q, bool handleMissingValues = false, int ddepth = -1,
                               double dispScale = 1.0, const double* missingValue = nullptr, bool zOnly = false)
{
    const int depth = reproject_depth("reprojectImageTo3D", disparity);
    if (ddepth != -1 && ddepth != D32F)
        throw Exception(ADF_EBADARG, "reprojectImageTo3D: ddepth must be -1 or CV_32F (CV_16SC3 and CV_32SC3 are not built)");
    const adf_reproject_params p = reproject_params("reprojectImageTo3D", Q, handleMissingValues, dispScale, missingValue);
    Mat out;
    mat_create(out, disparity.rows, disparity.cols, D32F, zOnly ? 1 : 3);
    check(adf_reproject_to_3d_host(1, disparity.data, depth, mat_step(disparity), 0, disparity.cols, disparity.rows, &p,
                                   reinterpret_cast<float*>(out.data), mat_step(out), 0, zOnly ? 1 : 3));
    _3dImage = out;
}

// The valid points of the map in raster order, three floats each, into `points`; optionally their `view` pixels
// (CV_8UC1 / CV_8UC3, the map's size) into `colours` and y * cols + x into `index`.  ROI with zero area = the whole map;
// zMin / zMax = -+infinity switch the range off.  Returns the number of points.
inline size_t pointCloud(const Mat& disparity, const Mat& Q, std::vector<float>& points, std::vector<uint8_t>* colours = nullptr,
                         const Mat& view = Mat(), Rect ROI = Rect(), double zMin = -HUGE_VAL, double zMax = HUGE_VAL,
                         bool handleMissingValues = false, double dispScale = 1.0, const double* missingValue = nullptr,
                         std::vector<int32_t>* index = nullptr)
{
    const int depth = reproject_depth("pointCloud", disparity);
    const adf_reproject_params p = reproject_params("pointCloud", Q, handleMissingValues, dispScale, missingValue);
    int vch = 0;
    if (colours) {
        if (view.empty() || mat_depth(view) != D8U || view.rows != disparity.rows || view.cols != disparity.cols)
            throw Exception(ADF_ESIZE, "pointCloud: colours need a CV_8U view of the disparity map's size");
        vch = mat_channels(view);
    }
    adf_rect roi{ROI.x, ROI.y, ROI.width, ROI.height};
    const bool whole = ROI.area() == 0;
    const size_t area = whole ? (size_t)disparity.rows * (size_t)disparity.cols : (size_t)ROI.width * (size_t)ROI.height;
    if (area > 2147483647u) throw Exception(ADF_ESIZE, "pointCloud: W*H must be below 2^31");
    points.resize(std::max<size_t>(area, 1) * 3);
    if (colours) colours->resize(std::max<size_t>(area, 1) * (size_t)std::max(vch, 1));
    if (index) index->resize(std::max<size_t>(area, 1));
    uint32_t count = 0;
    check(adf_point_cloud_host(1, disparity.data, depth, mat_step(disparity), 0, disparity.cols, disparity.rows, &p,
                               whole ? nullptr : &roi, zMin, zMax, colours ? view.data : nullptr, colours ? mat_step(view) : 0, 0, vch,
                               points.data(), 0, colours ? colours->data() : nullptr, 0, index ? index->data() : nullptr, 0,
                               (int)area, &count));
    points.resize((size_t)count * 3);
    if (colours) colours->resize((size_t)count * (size_t)vch);
    if (index) index->resize(count);
    return count;
}

// cv::initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type, map1, map2) of calib3d and
// cv::remap(src, dst, map1, map2, interpolation, borderMode, borderValue) of imgproc (outside the reference tree; parity
// unpinned) on host Mats through the library's host entries, and rectifyViews, both in one launch without the maps:
// definition and limits are adf_rectify_params_init / adf_init_undistort_rectify_map_* / adf_remap_* /
// adf_rectify_views_* in adf_wls.h.  cameraMatrix, R, newCameraMatrix: CV_64F, 3x3 (newCameraMatrix also 3x4: P1 / P2 of
// stereoRectify); R and newCameraMatrix may be empty (identity / cameraMatrix).  distCoeffs: empty or a CV_64F vector of 4, 5
// or 8.  m1type: CV_32FC1 only.  Images: CV_8UC1 / CV_8UC3; INTER_LINEAR with BORDER_CONSTANT only.  borderValue is
// templated like dsize above (cv::Scalar, or the stand-in below): its first three entries are the channels' fill.
#ifndef ADF_HAVE_OPENCV
struct Scalar {
    double val[4] = {0, 0, 0, 0};
    Scalar() {}
    Scalar(double v0, double v1 = 0, double v2 = 0, double v3 = 0) { val[0] = v0; val[1] = v1; val[2] = v2; val[3] = v3; }
    double operator[](int i) const { return val[i]; }
};
#endif
enum { BORDER_CONSTANT = 0, M32FC1 = 5 /* CV_32FC1 */ }; // cv's values

inline const double* rectify_matrix(const char* who, const char* name, const Mat& m, bool may_be_empty, bool or_3x4, double* copy)
{
    if (m.empty() && may_be_empty) return nullptr;
    if (m.empty() || mat_depth(m) != D64F || mat_channels(m) != 1 || m.rows != 3 || !(m.cols == 3 || (or_3x4 && m.cols == 4)))
        throw Exception(ADF_EBADARG, std::string(who) + ": " + name + " must be a CV_64F 3x3" + (or_3x4 ? " or 3x4" : "") + " matrix");
    for (int r = 0; r < 3; r++) std::memcpy(copy + r * m.cols, m.data + (size_t)mat_step(m) * r, sizeof(double) * m.cols);
    return copy;
}

inline adf_rectify_params rectify_params(const char* who, const Mat& cameraMatrix, const Mat& distCoeffs, const Mat& R, const Mat& newCameraMatrix)
{
    double K[9], Rm[9], P[12], dist[14];
    rectify_matrix(who, "cameraMatrix", cameraMatrix, false, false, K);
    const double* r = rectify_matrix(who, "R", R, true, false, Rm);
    const double* p = rectify_matrix(who, "newCameraMatrix", newCameraMatrix, true, true, P);
    int n_dist = 0;
    if (!distCoeffs.empty()) {
        if (mat_depth(distCoeffs) != D64F || mat_channels(distCoeffs) != 1 || (distCoeffs.rows != 1 && distCoeffs.cols != 1) ||
            distCoeffs.rows * distCoeffs.cols > 14)
            throw Exception(ADF_EBADARG, std::string(who) + ": distCoeffs must be a CV_64F vector of 4, 5 or 8 coefficients");
        n_dist = distCoeffs.rows * distCoeffs.cols;
        for (int i = 0; i < n_dist; i++)
            dist[i] = distCoeffs.rows == 1 ? reinterpret_cast<const double*>(distCoeffs.data)[i]
                                           : *reinterpret_cast<const double*>(distCoeffs.data + (size_t)mat_step(distCoeffs) * i);
    }
    adf_rectify_params prm;
    check(adf_rectify_params_init(K, dist, n_dist, r, p ? p : K, p ? newCameraMatrix.cols : 3, &prm));
    return prm;
}

template <class SizeT>
inline void initUndistortRectifyMap(const Mat& cameraMatrix, const Mat& distCoeffs, const Mat& R, const Mat& newCameraMatrix,
                                    SizeT size, int m1type, Mat& map1, Mat& map2)
{
    if (m1type != M32FC1) throw Exception(ADF_EBADARG, "initUndistortRectifyMap: m1type must be CV_32FC1 (the CV_16SC2 pair is not built)");
    if (size.width < 1 || size.height < 1) throw Exception(ADF_EBADARG, "initUndistortRectifyMap: the size is empty");
    const adf_rectify_params prm = rectify_params("initUndistortRectifyMap", cameraMatrix, distCoeffs, R, newCameraMatrix);
    Mat mx, my;
    mat_create(mx, size.height, size.width, D32F, 1);
    mat_create(my, size.height, size.width, D32F, 1);
    check(adf_init_undistort_rectify_map_host(&prm, size.width, size.height, reinterpret_cast<float*>(mx.data), mat_step(mx),
                                              reinterpret_cast<float*>(my.data), mat_step(my)));
    map1 = mx;
    map2 = my;
}

template <class ScalarT> inline void border_bytes(const char* who, const ScalarT& v, uint8_t* b)
{
    for (int c = 0; c < 3; c++) {
        const double d = v[c];
        if (!(d >= 0.0 && d <= 255.0) || d != std::floor(d)) throw Exception(ADF_EBADARG, std::string(who) + ": borderValue must hold integers in [0, 255]");
        b[c] = (uint8_t)d;
    }
}

inline void rectify_source(const char* who, const Mat& src)
{
    if (src.empty() || mat_depth(src) != D8U || (mat_channels(src) != 1 && mat_channels(src) != 3))
        throw Exception(ADF_EBADARG, std::string(who) + ": src must be a non-empty CV_8UC1 or CV_8UC3 image");
}

template <class ScalarT>
inline void remap(const Mat& src, Mat& dst, const Mat& map1, const Mat& map2, int interpolation, int borderMode, const ScalarT& borderValue)
{
    rectify_source("remap", src);
    if (map1.empty() || map2.empty() || mat_depth(map1) != D32F || mat_depth(map2) != D32F || mat_channels(map1) != 1 ||
        mat_channels(map2) != 1 || map1.rows != map2.rows || map1.cols != map2.cols)
        throw Exception(ADF_EBADARG, "remap: map1 and map2 must be two CV_32FC1 planes of one size");
    uint8_t b[3];
    border_bytes("remap", borderValue, b);
    Mat out;
    mat_create(out, map1.rows, map1.cols, D8U, mat_channels(src));
    check(adf_remap_host(1, src.data, mat_step(src), 0, src.cols, src.rows, mat_channels(src), reinterpret_cast<const float*>(map1.data),
                         mat_step(map1), reinterpret_cast<const float*>(map2.data), mat_step(map2), out.data, mat_step(out), 0,
                         map1.cols, map1.rows, interpolation, borderMode, b));
    dst = out;
}

inline void remap(const Mat& src, Mat& dst, const Mat& map1, const Mat& map2, int interpolation = INTER_LINEAR, int borderMode = BORDER_CONSTANT)
{
    const double zero[3] = {0, 0, 0};
    remap(src, dst, map1, map2, interpolation, borderMode, zero);
}

// Extension: remap(src, dst, <the maps of initUndistortRectifyMap(...)>) in one launch, bit for bit, without the maps.
// size with zero area = the source's size.
template <class SizeT, class ScalarT>
inline void rectifyViews(const Mat& src, Mat& dst, const Mat& cameraMatrix, const Mat& distCoeffs, const Mat& R, const Mat& newCameraMatrix,
                         SizeT size, const ScalarT& borderValue)
{
    rectify_source("rectifyViews", src);
    const int W = size.width == 0 && size.height == 0 ? src.cols : size.width, H = size.width == 0 && size.height == 0 ? src.rows : size.height;
    if (W < 1 || H < 1) throw Exception(ADF_EBADARG, "rectifyViews: the size is empty");
    const adf_rectify_params prm = rectify_params("rectifyViews", cameraMatrix, distCoeffs, R, newCameraMatrix);
    uint8_t b[3];
    border_bytes("rectifyViews", borderValue, b);
    Mat out;
    mat_create(out, H, W, D8U, mat_channels(src));
    check(adf_rectify_views_host(1, src.data, mat_step(src), 0, src.cols, src.rows, mat_channels(src), &prm, out.data, mat_step(out), 0,
                                 W, H, ADF_INTER_LINEAR, ADF_BORDER_CONSTANT, b));
    dst = out;
}

template <class SizeT>
inline void rectifyViews(const Mat& src, Mat& dst, const Mat& cameraMatrix, const Mat& distCoeffs, const Mat& R, const Mat& newCameraMatrix,
                         SizeT size)
{
    const double zero[3] = {0, 0, 0};
    rectifyViews(src, dst, cameraMatrix, distCoeffs, R, newCameraMatrix, size, zero);
}

namespace ximgproc {

// DF.hpp:52-76
class DisparityFilter {
public:
    virtual ~DisparityFilter() {}
    virtual void filter(const Mat& disparity_map_left, const Mat& left_view, Mat& filtered_disparity_map,
                        const Mat& disparity_map_right = Mat(), Rect ROI = Rect(), const Mat& right_view = Mat()) = 0;
};

// DF.hpp:82-122
class DisparityWLSFilter : public DisparityFilter {
public:
    virtual double getLambda() = 0;
    virtual void setLambda(double _lambda) = 0;
    virtual double getSigmaColor() = 0;
    virtual void setSigmaColor(double _sigma_color) = 0;
    virtual int getLRCthresh() = 0;
    virtual void setLRCthresh(int _LRC_thresh) = 0;
    virtual int getDepthDiscontinuityRadius() = 0;
    virtual void setDepthDiscontinuityRadius(int _disc_radius) = 0;
    virtual Mat getConfidenceMap() = 0;
    virtual Rect getROI() = 0;
    // extension: ADF_SOLVER_EXACT (bit-exact scalar order) or ADF_SOLVER_WAVE (on-chip, <= 1 LSB)
    virtual void setSolver(int solver) = 0;
    // extension (adf_wls_filter*_f32_* in adf_wls.h): filter() with a CV_32FC1 filtered map, view-sized, that keeps what
    // the rounding to 1/16 pixel throws away -- the int16 map's units (disparity * 16), -16.0f outside the ROI, never
    // NaN or inf, and saturate_cast<short> of it is filter()'s map bit for bit.  Same rules as filter(), the
    // lower-resolution maps included.
    virtual void filterToFloat(const Mat& disparity_map_left, const Mat& left_view, Mat& filtered_disparity_map,
                               const Mat& disparity_map_right = Mat(), Rect ROI = Rect()) = 0;
};

class DisparityWLSFilterImpl : public DisparityWLSFilter {
    adf_wls_t* h_ = nullptr;
    bool use_confidence_;
    int last_rows_ = 0, last_cols_ = 0;
public:
    DisparityWLSFilterImpl(bool use_confidence, int l, int r, int t, int b, int min_disp) : use_confidence_(use_confidence)
    {
        check(adf_wls_create(&h_, use_confidence ? 1 : 0, l, r, t, b, min_disp));
    }
    ~DisparityWLSFilterImpl() override { adf_wls_destroy(h_); }
    DisparityWLSFilterImpl(const DisparityWLSFilterImpl&) = delete;
    DisparityWLSFilterImpl& operator=(const DisparityWLSFilterImpl&) = delete;

    void filter(const Mat& dl, const Mat& view, Mat& out, const Mat& dr, Rect ROI, const Mat&) override
    {
        run(dl, view, out, dr, ROI, false);
    }
    void filterToFloat(const Mat& dl, const Mat& view, Mat& out, const Mat& dr, Rect ROI) override
    {
        run(dl, view, out, dr, ROI, true);
    }
private:
    // filter() and filterToFloat(): one set of checks, the output's depth and the entry point differ
    void run(const Mat& dl, const Mat& view, Mat& out, const Mat& dr, Rect ROI, bool f32)
    {
        // CV_16SC1 (DF.cpp:221) or, an extension, CV_32FC1 maps in the same units (adf_wls_filter_typed_* in adf_wls.h:
        // the solve takes the floats as they are, the confidence map their rounding); the left map's depth is the pair's
        const bool fin = !dl.empty() && mat_depth(dl) == D32F;
        if (dl.empty() || (mat_depth(dl) != D16S && !fin) || mat_channels(dl) != 1)
            throw Exception(ADF_EBADARG, "disparity_map_left must be a non-empty CV_16SC1 or CV_32FC1 image");
        if (view.empty() || mat_depth(view) != D8U || (mat_channels(view) != 1 && mat_channels(view) != 3)) // :222
            throw Exception(ADF_EBADARG, "left_view must be CV_8UC1 or CV_8UC3");
        const bool have_r = !dr.empty();
        if (use_confidence_) {                                                 // DF.cpp:262-264
            if (!have_r || mat_depth(dr) != mat_depth(dl) || mat_channels(dr) != 1)
                throw Exception(ADF_EBADARG, fin ? "disparity_map_right must be a non-empty CV_32FC1 image, as the left map is"
                                                 : "disparity_map_right must be a non-empty CV_16SC1 image");
            if (dr.rows != dl.rows || dr.cols != dl.cols)
                throw Exception(ADF_ESIZE, "left and right disparity maps differ in size");
        }
        mat_create(out, view.rows, view.cols, f32 ? D32F : D16S, 1);           // DF.cpp:252,282 (view-sized)
        adf_rect roi{ROI.x, ROI.y, ROI.width, ROI.height};
        const int16_t* l = reinterpret_cast<const int16_t*>(dl.data);
        const int16_t* r = have_r ? reinterpret_cast<const int16_t*>(dr.data) : nullptr;
        const ptrdiff_t rs = have_r ? mat_step(dr) : 0;
        const adf_rect* rp = ROI.area() != 0 ? &roi : nullptr;
        // a lower-resolution disparity map is resized to the view inside the call (DF.cpp:239-247,268-277)
        if (fin)
            check(adf_wls_filter_typed_host(h_, 1, dl.data, mat_step(dl), 0, ADF_32F, dl.cols, dl.rows, view.data, mat_step(view), 0,
                                            mat_channels(view), view.cols, view.rows, out.data, mat_step(out), 0,
                                            f32 ? ADF_32F : ADF_16S, (have_r && use_confidence_) ? dr.data : nullptr, rs, 0, rp));   // (no confidence: no use for a right map)
        else if (f32)
            check(adf_wls_filter_scaled_f32_host(h_, 1, l, mat_step(dl), 0, dl.cols, dl.rows, view.data, mat_step(view), 0,
                                                 mat_channels(view), view.cols, view.rows,
                                                 reinterpret_cast<float*>(out.data), mat_step(out), 0, r, rs, 0, rp));
        else
            check(adf_wls_filter_scaled_host(h_, 1, l, mat_step(dl), 0, dl.cols, dl.rows, view.data, mat_step(view), 0,
                                             mat_channels(view), view.cols, view.rows,
                                             reinterpret_cast<int16_t*>(out.data), mat_step(out), 0, r, rs, 0, rp));
        last_rows_ = view.rows; last_cols_ = view.cols;
    }
public:
    double getLambda() override { double v; check(adf_wls_get_lambda(h_, &v)); return v; }
    void setLambda(double v) override { check(adf_wls_set_lambda(h_, v)); }
    double getSigmaColor() override { double v; check(adf_wls_get_sigma_color(h_, &v)); return v; }
    void setSigmaColor(double v) override { check(adf_wls_set_sigma_color(h_, v)); }
    int getLRCthresh() override { int v; check(adf_wls_get_lrc_thresh(h_, &v)); return v; }
    void setLRCthresh(int v) override { check(adf_wls_set_lrc_thresh(h_, v)); }
    int getDepthDiscontinuityRadius() override { int v; check(adf_wls_get_depth_discontinuity_radius(h_, &v)); return v; }
    void setDepthDiscontinuityRadius(int v) override { check(adf_wls_set_depth_discontinuity_radius(h_, v)); }
    Mat getConfidenceMap() override
    {
        Mat m;                                                                 // empty Mat before the first call (DF.cpp:153)
        if (!use_confidence_ || last_rows_ == 0) return m;
        mat_create(m, last_rows_, last_cols_, D32F, 1);
        check(adf_wls_get_confidence_host(h_, 0, reinterpret_cast<float*>(m.data), mat_step(m)));
        return m;
    }
    Rect getROI() override { adf_rect r; check(adf_wls_get_roi(h_, &r)); return Rect(r.x, r.y, r.width, r.height); }
    void setSolver(int solver) override { check(adf_wls_set_solver(h_, solver)); }
};

// DF.hpp:149, DF.cpp:452-455
inline Ptr<DisparityWLSFilter> createDisparityWLSFilterGeneric(bool use_confidence)
{
    return Ptr<DisparityWLSFilter>(new DisparityWLSFilterImpl(use_confidence, 0, 0, 0, 0, 0));
}

// The arithmetic of createDisparityWLSFilter (DF.cpp:392-409) on the three matcher parameters it reads.
inline Ptr<DisparityWLSFilter> createDisparityWLSFilter(bool is_sgbm, int min_disp, int num_disp, int wsize)
{
    const int wsize2 = wsize / 2;
    Ptr<DisparityWLSFilter> wls;
    if (!is_sgbm) {                                                            // StereoBM, DF.cpp:397-403
        wls = Ptr<DisparityWLSFilter>(new DisparityWLSFilterImpl(true, std::max(0, min_disp + num_disp) + wsize2,
                                                                 std::max(0, -min_disp) + wsize2, wsize2, wsize2, min_disp));
        wls->setDepthDiscontinuityRadius((int)std::ceil(0.33 * wsize));
    } else {                                                                   // StereoSGBM, DF.cpp:404-409
        wls = Ptr<DisparityWLSFilter>(new DisparityWLSFilterImpl(true, std::max(0, min_disp + num_disp),
                                                                 std::max(0, -min_disp), 0, 0, min_disp));
        wls->setDepthDiscontinuityRadius((int)std::ceil(0.5 * wsize));
    }
    return wls;
}

#ifdef ADF_HAVE_CALIB3D
// DF.hpp:131, DF.cpp:386-414 (mutates the matcher exactly like the reference)
inline Ptr<DisparityWLSFilter> createDisparityWLSFilter(cv::Ptr<cv::StereoMatcher> matcher_left)
{
    matcher_left->setDisp12MaxDiff(1000000);
    matcher_left->setSpeckleWindowSize(0);
    const int min_disp = matcher_left->getMinDisparity(), num_disp = matcher_left->getNumDisparities();
    const int wsize = matcher_left->getBlockSize();
    if (cv::Ptr<cv::StereoBM> bm = matcher_left.dynamicCast<cv::StereoBM>()) {
        bm->setTextureThreshold(0);
        bm->setUniquenessRatio(0);
        return createDisparityWLSFilter(false, min_disp, num_disp, wsize);
    }
    if (cv::Ptr<cv::StereoSGBM> sgbm = matcher_left.dynamicCast<cv::StereoSGBM>()) {
        sgbm->setUniquenessRatio(0);
        return createDisparityWLSFilter(true, min_disp, num_disp, wsize);
    }
    throw Exception(ADF_EBADARG, "DisparityWLSFilter natively supports only StereoBM and StereoSGBM");
}

// DF.hpp:139, DF.cpp:417-449
inline cv::Ptr<cv::StereoMatcher> createRightMatcher(cv::Ptr<cv::StereoMatcher> matcher_left)
{
    const int min_disp = matcher_left->getMinDisparity(), num_disp = matcher_left->getNumDisparities();
    const int wsize = matcher_left->getBlockSize();
    if (cv::Ptr<cv::StereoBM> bm = matcher_left.dynamicCast<cv::StereoBM>()) {
        cv::Ptr<cv::StereoBM> right_bm = cv::StereoBM::create(num_disp, wsize);
        right_bm->setMinDisparity(-(min_disp + num_disp) + 1);
        right_bm->setTextureThreshold(0);
        right_bm->setUniquenessRatio(0);
        right_bm->setDisp12MaxDiff(1000000);
        right_bm->setSpeckleWindowSize(0);
        // (cv::StereoBM has one matching cost: the census costs exist on adf::ximgproc::StereoBM below, whose
        // createRightMatcher carries them over)
        return right_bm;
    }
    if (cv::Ptr<cv::StereoSGBM> sgbm = matcher_left.dynamicCast<cv::StereoSGBM>()) {
        cv::Ptr<cv::StereoSGBM> right_sgbm = cv::StereoSGBM::create(-(min_disp + num_disp) + 1, num_disp, wsize);
        right_sgbm->setUniquenessRatio(0);
        right_sgbm->setP1(sgbm->getP1());
        right_sgbm->setP2(sgbm->getP2());
        right_sgbm->setMode(sgbm->getMode());
        right_sgbm->setPreFilterCap(sgbm->getPreFilterCap());
        // (cv::StereoSGBM has one matching cost: the census costs exist on adf::ximgproc::StereoSGBM below, whose
        // createRightMatcher carries them over)
        right_sgbm->setDisp12MaxDiff(1000000);
        right_sgbm->setSpeckleWindowSize(0);
        return right_sgbm;
    }
    throw Exception(ADF_EBADARG, "createRightMatcher supports only StereoBM and StereoSGBM");
}
#endif

// ---------------------------------------------------------------------------------------------------------
// Block matcher feeding the filter.  cv::StereoBM is a class of OpenCV's calib3d, outside the
// reference tree (parity unpinned there); this class carries its accessor names over adf_bm_* so that the
// sample's pipeline (samples/disparity_filtering.cpp:151-189) reads the same.  Host images in, host image out;
// device-resident pipelines call adf_bm_compute_device directly.
// ---------------------------------------------------------------------------------------------------------
class StereoBM {
    adf_bm_t* h_ = nullptr;
    int min_disp_ = 0, num_disp_, block_, cap_ = 31, texture_ = 10, uniq_ = 15;   // cv::StereoBM's defaults
    int disp12_ = -1, speckle_window_ = 0;
    int cost_ = ADF_BM_COST_SAD, census_size_ = 7;                                // a new adf_bm handle's
public:
    StereoBM(int numDisparities, int blockSize) : num_disp_(numDisparities > 0 ? numDisparities : 64), block_(blockSize)
    {
        check(adf_bm_create(&h_, num_disp_, block_));
    }
    ~StereoBM() { adf_bm_destroy(h_); }
    StereoBM(const StereoBM&) = delete;
    StereoBM& operator=(const StereoBM&) = delete;
    static Ptr<StereoBM> create(int numDisparities = 0, int blockSize = 21) { return Ptr<StereoBM>(new StereoBM(numDisparities, blockSize)); }
    int getMinDisparity() const { return min_disp_; }        void setMinDisparity(int v) { min_disp_ = v; }
    int getNumDisparities() const { return num_disp_; }      void setNumDisparities(int v) { num_disp_ = v; }
    int getBlockSize() const { return block_; }              void setBlockSize(int v) { block_ = v; }
    int getPreFilterCap() const { return cap_; }             void setPreFilterCap(int v) { cap_ = v; }
    int getTextureThreshold() const { return texture_; }     void setTextureThreshold(int v) { texture_ = v; }
    int getUniquenessRatio() const { return uniq_; }         void setUniquenessRatio(int v) { uniq_ = v; }
    int getDisp12MaxDiff() const { return disp12_; }         void setDisp12MaxDiff(int v) { disp12_ = v; }
    int getSpeckleWindowSize() const { return speckle_window_; } void setSpeckleWindowSize(int v) { speckle_window_ = v; }
    // extension (adf_bm_set_cost in adf_wls.h): ADF_BM_COST_SAD, or a census descriptor + Hamming distance, the cost of
    // the reference's own cv::stereo::StereoBinaryBM; preFilterCap and textureThreshold are validated and not used with
    // it (there is no prefiltered image).  The library checks the pair (type, size) when compute() pushes it.
    // Descriptors: ADF_BM_COST_CENSUS_DENSE / _CENSUS_SPARSE / _MCT_DENSE / _MCT_SPARSE / _CENSUS_CS (sizes: adf_wls.h).
    int getCostType() const { return cost_; }                void setCostType(int v) { cost_ = v; }
    int getCensusSize() const { return census_size_; }       void setCensusSize(int v) { census_size_ = v; }
    // StereoMatcher::compute: CV_8UC1 views -> CV_16SC1 disparity * 16, rejected pixels (minDisparity - 1) * 16
    void compute(const Mat& left, const Mat& right, Mat& disparity)
    {
        check_views(left, right);
        if ((disp12_ >= 0 && disp12_ < 1000000) || speckle_window_ > 0)          // the filter factory switches both off (DF.cpp:389-390)
            throw Exception(ADF_EBADARG, "the matcher's own left-right check and speckle filter are not implemented");
        match(left, right, disparity, nullptr);
    }
    // extension (adf_bm_compute_cost_host in adf_wls.h): compute()'s map and the CV_16SC1 aggregated cost of each winning
    // disparity (0 where the map holds (minDisparity - 1) * 16), the pair adf::validateDisparity takes.  The match alone:
    // disp12MaxDiff and speckleWindowSize are not applied, so the caller runs validateDisparity / filterSpeckles itself.
    void computeWithCost(const Mat& left, const Mat& right, Mat& disparity, Mat& cost)
    {
        check_views(left, right);
        match(left, right, disparity, &cost);
    }
private:
    // checked views -> the map and, with `cost`, the winners' cost plane, through the host entry that returns them
    void match(const Mat& left, const Mat& right, Mat& disparity, Mat* cost)
    {
        push_params();
        Mat out, c;
        mat_create(out, left.rows, left.cols, D16S, 1);
        int16_t* const d = reinterpret_cast<int16_t*>(out.data);
        if (cost) {
            mat_create(c, left.rows, left.cols, D16S, 1);
            check(adf_bm_compute_cost_host(h_, 1, left.data, mat_step(left), 0, right.data, mat_step(right), 0, left.cols, left.rows,
                                           d, mat_step(out), 0, reinterpret_cast<int16_t*>(c.data), mat_step(c), 0));
            *cost = c;
        } else
            check(adf_bm_compute_host(h_, 1, left.data, mat_step(left), 0, right.data, mat_step(right), 0, left.cols, left.rows,
                                      d, mat_step(out), 0));
        disparity = out;
    }
    static void check_views(const Mat& left, const Mat& right)
    {
        if (left.empty() || right.empty() || mat_depth(left) != D8U || mat_depth(right) != D8U ||
            mat_channels(left) != 1 || mat_channels(right) != 1)
            throw Exception(ADF_EBADARG, "Both input images must have CV_8UC1");
        if (left.rows != right.rows || left.cols != right.cols)
            throw Exception(ADF_ESIZE, "All the images must have the same size");
    }
    void push_params()
    {
        check(adf_bm_set_params(h_, min_disp_, num_disp_, block_, cap_, texture_, uniq_));
        check(adf_bm_set_cost(h_, cost_, census_size_));
    }
};

// DF.cpp:386-403 (StereoBM branch): mutates the matcher exactly like the reference, derives ROI offsets and radius
inline Ptr<DisparityWLSFilter> createDisparityWLSFilter(const Ptr<StereoBM>& matcher_left)
{
    matcher_left->setDisp12MaxDiff(1000000);
    matcher_left->setSpeckleWindowSize(0);
    matcher_left->setTextureThreshold(0);
    matcher_left->setUniquenessRatio(0);
    return createDisparityWLSFilter(false, matcher_left->getMinDisparity(), matcher_left->getNumDisparities(),
                                    matcher_left->getBlockSize());
}

// DF.cpp:417-431
inline Ptr<StereoBM> createRightMatcher(const Ptr<StereoBM>& matcher_left)
{
    const int min_disp = matcher_left->getMinDisparity(), num_disp = matcher_left->getNumDisparities();
    Ptr<StereoBM> right_bm = StereoBM::create(num_disp, matcher_left->getBlockSize());
    right_bm->setMinDisparity(-(min_disp + num_disp) + 1);
    right_bm->setTextureThreshold(0);
    right_bm->setUniquenessRatio(0);
    right_bm->setDisp12MaxDiff(1000000);
    right_bm->setSpeckleWindowSize(0);
    // (the reference's BM branch does not copy preFilterCap: the right matcher keeps cv::StereoBM's default 31)
    right_bm->setCostType(matcher_left->getCostType());         // (a different cost on the right view would wreck the LRC confidence)
    right_bm->setCensusSize(matcher_left->getCensusSize());
    return right_bm;
}

// ---------------------------------------------------------------------------------------------------------
// Semi-global matcher feeding the filter: cv::StereoSGBM's accessor names over adf_sgbm_*, the
// sample's other producer (samples/disparity_filtering.cpp:166-176).  MODE_SGBM_3WAY (the sample's), MODE_SGBM, MODE_HH.
// ---------------------------------------------------------------------------------------------------------
class StereoSGBM {
    adf_sgbm_t* h_ = nullptr;
    int min_disp_, num_disp_, block_, P1_ = 0, P2_ = 0, cap_ = 0, uniq_ = 0, mode_ = MODE_SGBM;    // cv::StereoSGBM::create's defaults
    int disp12_ = 0, speckle_window_ = 0;
    int cost_ = ADF_SGBM_COST_BT, census_size_ = 7;                                                  // a new adf_sgbm handle's
public:
    enum { MODE_SGBM = ADF_SGBM_MODE_SGBM, MODE_HH = ADF_SGBM_MODE_HH, MODE_SGBM_3WAY = ADF_SGBM_MODE_3WAY };
    StereoSGBM(int minDisparity, int numDisparities, int blockSize) : min_disp_(minDisparity), num_disp_(numDisparities), block_(blockSize)
    {
        check(adf_sgbm_create(&h_, min_disp_, num_disp_, block_));
    }
    ~StereoSGBM() { adf_sgbm_destroy(h_); }
    StereoSGBM(const StereoSGBM&) = delete;
    StereoSGBM& operator=(const StereoSGBM&) = delete;
    static Ptr<StereoSGBM> create(int minDisparity = 0, int numDisparities = 16, int blockSize = 3)
    {
        return Ptr<StereoSGBM>(new StereoSGBM(minDisparity, numDisparities, blockSize));
    }
    int getMinDisparity() const { return min_disp_; }        void setMinDisparity(int v) { min_disp_ = v; }
    int getNumDisparities() const { return num_disp_; }      void setNumDisparities(int v) { num_disp_ = v; }
    int getBlockSize() const { return block_; }              void setBlockSize(int v) { block_ = v; }
    int getP1() const { return P1_; }                        void setP1(int v) { P1_ = v; }
    int getP2() const { return P2_; }                        void setP2(int v) { P2_ = v; }
    int getPreFilterCap() const { return cap_; }             void setPreFilterCap(int v) { cap_ = v; }
    int getUniquenessRatio() const { return uniq_; }         void setUniquenessRatio(int v) { uniq_ = v; }
    int getMode() const { return mode_; }                    void setMode(int v) { mode_ = v; }
    int getDisp12MaxDiff() const { return disp12_; }         void setDisp12MaxDiff(int v) { disp12_ = v; }
    int getSpeckleWindowSize() const { return speckle_window_; } void setSpeckleWindowSize(int v) { speckle_window_ = v; }
    // extension (adf_sgbm_set_cost in adf_wls.h): ADF_SGBM_COST_BT, or a census descriptor + Hamming distance, the cost of
    // cv::stereo::StereoBinarySGBM (its setBinaryKernelType / kernelSize); the pair is checked when compute() pushes it.
    // Descriptors: ADF_SGBM_COST_CENSUS_DENSE / _CENSUS_SPARSE / _MCT_DENSE / _MCT_SPARSE / _CENSUS_CS (sizes: adf_wls.h).
    int getCostType() const { return cost_; }                void setCostType(int v) { cost_ = v; }
    int getCensusSize() const { return census_size_; }       void setCensusSize(int v) { census_size_ = v; }
    // StereoMatcher::compute: CV_8UC1 / CV_8UC3 views -> CV_16SC1 disparity * 16, invalid pixels (minDisparity - 1) * 16
    void compute(const Mat& left, const Mat& right, Mat& disparity)
    {
        prepare(left, right);
        Mat out;
        mat_create(out, left.rows, left.cols, D16S, 1);
        check(adf_sgbm_compute_host(h_, 1, left.data, mat_step(left), 0, right.data, mat_step(right), 0, mat_channels(left),
                                    left.cols, left.rows, reinterpret_cast<int16_t*>(out.data), mat_step(out), 0));
        disparity = out;
    }
    // extension (adf_sgbm_compute_both_host in adf_wls.h): compute()'s map and a right-view map from one call, the pair
    // DisparityWLSFilter::filter takes.  ADF_SGBM_RIGHT_MATCHER (default): the map of createRightMatcher(this)->compute(right,
    // left), identical to the two separate computes and as expensive.  ADF_SGBM_RIGHT_FROM_VOLUME: a speed-for-fidelity
    // option -- the right map is read from this view's aggregated volume inside the winner pass; it is NOT the right matcher's
    // map and has its own definition in adf_wls.h.
    void computeBoth(const Mat& left, const Mat& right, Mat& disparity_left, Mat& disparity_right, int rightSource = ADF_SGBM_RIGHT_MATCHER)
    {
        prepare(left, right);
        Mat outl, outr;
        mat_create(outl, left.rows, left.cols, D16S, 1);
        mat_create(outr, left.rows, left.cols, D16S, 1);
        check(adf_sgbm_compute_both_host(h_, 1, left.data, mat_step(left), 0, right.data, mat_step(right), 0, mat_channels(left),
                                         left.cols, left.rows, reinterpret_cast<int16_t*>(outl.data), mat_step(outl), 0,
                                         reinterpret_cast<int16_t*>(outr.data), mat_step(outr), 0, rightSource));
        disparity_left = outl;
        disparity_right = outr;
    }
private:
    // the views checked, the speckle setting refused, the parameters pushed
    void prepare(const Mat& left, const Mat& right)
    {
        if (left.empty() || right.empty() || mat_depth(left) != D8U || mat_depth(right) != D8U ||
            (mat_channels(left) != 1 && mat_channels(left) != 3) || mat_channels(left) != mat_channels(right))
            throw Exception(ADF_EBADARG, "Both input images must have CV_8UC1 or CV_8UC3");
        if (left.rows != right.rows || left.cols != right.cols)
            throw Exception(ADF_ESIZE, "All the images must have the same size");
        if (speckle_window_ > 0)                                                 // the filter factory switches it off (DF.cpp:390)
            throw Exception(ADF_EBADARG, "the matcher's speckle filter is not implemented");
        check(adf_sgbm_set_params(h_, min_disp_, num_disp_, block_, P1_, P2_, cap_, uniq_, mode_));
        check(adf_sgbm_set_disp12_max_diff(h_, disp12_));
        check(adf_sgbm_set_cost(h_, cost_, census_size_));
    }
};

// DF.cpp:386-391, 404-409 (StereoSGBM branch)
inline Ptr<DisparityWLSFilter> createDisparityWLSFilter(const Ptr<StereoSGBM>& matcher_left)
{
    matcher_left->setDisp12MaxDiff(1000000);
    matcher_left->setSpeckleWindowSize(0);
    matcher_left->setUniquenessRatio(0);
    return createDisparityWLSFilter(true, matcher_left->getMinDisparity(), matcher_left->getNumDisparities(),
                                    matcher_left->getBlockSize());
}

// DF.cpp:432-445
inline Ptr<StereoSGBM> createRightMatcher(const Ptr<StereoSGBM>& matcher_left)
{
    const int min_disp = matcher_left->getMinDisparity(), num_disp = matcher_left->getNumDisparities();
    Ptr<StereoSGBM> right_sgbm = StereoSGBM::create(-(min_disp + num_disp) + 1, num_disp, matcher_left->getBlockSize());
    right_sgbm->setUniquenessRatio(0);
    right_sgbm->setP1(matcher_left->getP1());
    right_sgbm->setP2(matcher_left->getP2());
    right_sgbm->setMode(matcher_left->getMode());
    right_sgbm->setPreFilterCap(matcher_left->getPreFilterCap());
    right_sgbm->setCostType(matcher_left->getCostType());       // (a different cost on the right view would wreck the LRC confidence)
    right_sgbm->setCensusSize(matcher_left->getCensusSize());
    right_sgbm->setDisp12MaxDiff(1000000);
    right_sgbm->setSpeckleWindowSize(0);
    return right_sgbm;
}

// EF.hpp:361-371
class FastGlobalSmootherFilter {
    adf_fgs_t* h_ = nullptr;
    int rows_, cols_;
public:
    FastGlobalSmootherFilter(const Mat& guide, double lambda, double sigma_color, double lambda_attenuation, int num_iter,
                             int solver = ADF_SOLVER_WAVE)
        : rows_(guide.rows), cols_(guide.cols)
    {
        if (guide.empty() || mat_depth(guide) != D8U)                          // FGS.cpp:143-144
            throw Exception(ADF_EBADARG, "guide must be a non-empty CV_8UC1 / CV_8UC3 image");
        check(adf_fgs_create(&h_, guide.data, mat_step(guide), mat_channels(guide), guide.cols, guide.rows, lambda,
                             sigma_color, lambda_attenuation, num_iter, solver));
    }
    ~FastGlobalSmootherFilter() { adf_fgs_destroy(h_); }
    FastGlobalSmootherFilter(const FastGlobalSmootherFilter&) = delete;
    FastGlobalSmootherFilter& operator=(const FastGlobalSmootherFilter&) = delete;
    void filter(const Mat& src, Mat& dst)                                      // EF.hpp:370, FGS.cpp:182-233
    {
        if (src.empty()) throw Exception(ADF_EBADARG, "src is empty");
        if (src.rows != rows_ || src.cols != cols_)                            // FGS.cpp:185-189
            throw Exception(ADF_ESIZE, "Size of the filtered image must be equal to the size of the guide image");
        Mat out;
        mat_create(out, src.rows, src.cols, mat_depth(src), mat_channels(src));
        check(adf_fgs_filter_host(h_, src.data, mat_step(src), out.data, mat_step(out), mat_depth(src), mat_channels(src)));
        dst = out;
    }
};

// EF.hpp:393
inline Ptr<FastGlobalSmootherFilter> createFastGlobalSmootherFilter(const Mat& guide, double lambda, double sigma_color,
                                                                    double lambda_attenuation = 0.25, int num_iter = 3)
{
    return Ptr<FastGlobalSmootherFilter>(new FastGlobalSmootherFilter(guide, lambda, sigma_color, lambda_attenuation, num_iter));
}

// EF.hpp:413
inline void fastGlobalSmootherFilter(const Mat& guide, const Mat& src, Mat& dst, double lambda, double sigma_color,
                                     double lambda_attenuation = 0.25, int num_iter = 3)
{
    createFastGlobalSmootherFilter(guide, lambda, sigma_color, lambda_attenuation, num_iter)->filter(src, dst);
}

} // namespace ximgproc
} // namespace adf
