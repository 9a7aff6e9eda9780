/*
 * adf_wls.h -- C-ABI of the MI355X-native DisparityWLSFilter / FastGlobalSmoother path.
 *
 * This is the drop-in boundary: plain pointers, sizes and strides, no C++ and no
 * torch types.  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree):
 *   DF.hpp  = modules/ximgproc/include/opencv2/ximgproc/disparity_filter.hpp
 *   DF.cpp  = modules/ximgproc/src/disparity_filters.cpp
 *   EF.hpp  = modules/ximgproc/include/opencv2/ximgproc/edge_filter.hpp
 *   FGS.cpp = modules/ximgproc/src/fgs_filter.cpp
 *
 * Conventions
 *   - all strides are in BYTES; images are row-major, channels interleaved;
 *   - "_device" entry points take HIP device pointers and run asynchronously on
 *     `stream` (a hipStream_t passed as void*, NULL = default stream);
 *     "_host" entry points take host pointers, copy, run and synchronise;
 *   - a handle owns a device workspace that is sized on first use and reused; a
 *     handle serves one caller at a time (the reference objects are not
 *     re-entrant either: DF.cpp:224-233, FGS.cpp:202-223);
 *   - a handle is bound to the HIP device that was current when it was created
 *     (adf_*_get_device) and to ONE stream at a time: every call on a handle
 *     stages through the same workspace, so two calls on different streams must
 *     be ordered by the caller (an event, or adf_wls_sync) -- nothing inside the
 *     library serialises them.  Device pointers must belong to the handle's
 *     device.  Concurrency = several handles, each on its own stream;
 *   - every function returns ADF_OK or an error code; adf_last_error() gives the
 *     message of the calling thread's last failure (the reference throws
 *     cv::Exception from CV_Assert / CV_Error: DF.cpp:221-222,262-264,
 *     FGS.cpp:143-144,184-189 -- a C++ adaptor turns codes back into exceptions).
 */
#ifndef ADF_WLS_H
#define ADF_WLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADF_VERSION 100

enum adf_status {
    ADF_OK = 0,
    ADF_EBADARG = 1, /* CV_Assert on types / emptiness            DF.cpp:221-222,262 */
    ADF_ESIZE = 2,   /* size mismatch (Error::StsBadSize)         DF.cpp:263-264, FGS.cpp:185-189 */
    ADF_EHIP = 3,    /* a HIP runtime call failed                                       */
    ADF_ENOMEM = 4,  /* workspace allocation failed                                     */
    ADF_ENODEV = 5   /* no usable gfx950 device                                         */
};

/* Thomas-solve strategy (no counterpart in the reference, which picks its own
 * floating-point order per stripe: FGS.cpp:466-476).
 *   ADF_SOLVER_EXACT : one lane per scanline, canonical scalar order of
 *                      process_row (FGS.cpp:439-464); bit-identical to the CPU
 *                      restatement in oracle/.
 *   ADF_SOLVER_WAVE  : one wavefront per scanline, partitioned solve held in
 *                      registers/LDS; re-associated arithmetic, within the
 *                      reference's own reproducibility tolerance (<=1 LSB of the
 *                      CV_16S output, test_disparity_wls_filter.cpp:104-105).
 * A new handle uses ADF_SOLVER_WAVE (13x lower latency on a single 1920x1080 pair, 1.8x the
 * throughput on 4K batches); the confidence map is bit-exact with either.  Select
 * ADF_SOLVER_EXACT when the filtered map has to reproduce the scalar evaluation order bit for bit. */
enum adf_solver { ADF_SOLVER_EXACT = 0, ADF_SOLVER_WAVE = 1 };

/* cv::Mat depth codes for adf_fgs_filter_* (FGS.cpp:184); ADF_32S (CV_32S) is a cost plane of adf_validate_disparity_* only. */
enum adf_depth { ADF_8U = 0, ADF_16S = 3, ADF_32S = 4, ADF_32F = 5 };

typedef struct adf_wls adf_wls_t; /* cv::Ptr<DisparityWLSFilter>        */
typedef struct adf_fgs adf_fgs_t; /* cv::Ptr<FastGlobalSmootherFilter>  */

typedef struct adf_rect { int x, y, width, height; } adf_rect; /* cv::Rect */

int adf_version(void);
const char* adf_last_error(void);
/* Number of visible HIP devices (0 when none); never fails. */
int adf_device_count(void);
/* PCI bus id ("0000:c1:00.0") of HIP device `device` into buf (at least 16 bytes): lets a multi-process harness show
 * that its ranks sit on distinct devices.  No counterpart in the reference (it has no device layer). */
int adf_device_pci_bus_id(int device, char* buf, int len);

/* ---------------- DisparityWLSFilter ---------------- */

/* DisparityWLSFilterImpl::create + init (DF.cpp:142-159, 212-217), reached through
 * createDisparityWLSFilterGeneric(use_confidence) (DF.hpp:149, DF.cpp:452-455; all
 * offsets 0) or createDisparityWLSFilter(matcher) (DF.hpp:131, DF.cpp:386-414; the
 * caller derives the offsets from the matcher).
 * Defaults as the reference: lambda 8000, sigma_color 1.0, LRC_thresh 24,
 * depth_discontinuity_radius 5; min_disp is accepted and ignored (DF.cpp:146,149). */
int adf_wls_create(adf_wls_t** out, int use_confidence, int left_offset, int right_offset,
                   int top_offset, int bottom_offset, int min_disp);
void adf_wls_destroy(adf_wls_t* h);

/* DisparityWLSFilter get/set (DF.hpp:90-122, DF.cpp:126-136). */
int adf_wls_set_lambda(adf_wls_t* h, double lambda);
int adf_wls_get_lambda(const adf_wls_t* h, double* lambda);
/* (every sigma_color a handle has seen keeps its own immutable weight table on the device, up to eight: coming back to
 * one is free and capturable; a NEW value builds its table on the host inside the next filter call and uploads it with
 * one synchronous copy -- use each sigma once BEFORE capturing filter calls that switch between them into a hipGraph) */
int adf_wls_set_sigma_color(adf_wls_t* h, double sigma_color);
int adf_wls_get_sigma_color(const adf_wls_t* h, double* sigma_color);
int adf_wls_set_lrc_thresh(adf_wls_t* h, int lrc_thresh);
int adf_wls_get_lrc_thresh(const adf_wls_t* h, int* lrc_thresh);
int adf_wls_set_depth_discontinuity_radius(adf_wls_t* h, int radius);
int adf_wls_get_depth_discontinuity_radius(const adf_wls_t* h, int* radius);

/* The inner smoother's parameters, fixed to (0.25, 3) by the reference call site
 * createFastGlobalSmootherFilter(src, lambda, sigma_color) (DF.cpp:292, EF.hpp:393);
 * exposed because BASELINE config 5 names num_iter explicitly. */
int adf_wls_set_fgs_params(adf_wls_t* h, double lambda_attenuation, int num_iter);
int adf_wls_set_solver(adf_wls_t* h, int solver);
int adf_wls_get_solver(const adf_wls_t* h, int* solver);
/* Solver the last filter call actually ran: ADF_SOLVER_WAVE covers ROIs up to 8192 x 4352 (an 8K frame: beyond 4096
 * columns two wavefronts share a row, beyond 2176 rows a column is cut into 128 chunks); larger ones fall back to
 * ADF_SOLVER_EXACT. */
int adf_wls_get_last_solver(const adf_wls_t* h, int* solver);
/* Which kernels the confidence stage of the last filter call took (introspection for tests and benchmarks; the
 * results do not depend on it): ADF_PATH_CONF_BAND = computeConfidenceMap (DF.cpp:197-210) ran as the one-sweep band
 * kernel (depth-discontinuity radius 1..8), ADF_PATH_FUSED_FIRST_PASS = the first row pass formed conf*disp itself
 * (DF.cpp:288-290) instead of reading planes a prologue kernel wrote, ADF_PATH_MERGED_PREP = the edge weights, the
 * confidence map and the fill outside the ROI were one launch (calls of at most 2.5 Mpixels of ROI). */
#define ADF_PATH_CONF_BAND 1
#define ADF_PATH_FUSED_FIRST_PASS 2
#define ADF_PATH_MERGED_PREP 4       /* weights + confidence + fill ran as ONE launch (small calls) */
#define ADF_PATH_SCALED_FUSED 8      /* down-scaled call: the first row pass interpolated the low-resolution maps itself
                                        (no resize launch); the view-sized confidence map is produced on demand by
                                        adf_wls_get_confidence_* */
#define ADF_PATH_SCALED_HALF 16      /* ... in its form for maps of exactly half the view's width on a ROI starting on an even
                                        column >= 2 (the sample's default): four output columns share four source elements */
int adf_wls_get_last_path(const adf_wls_t* h, int* path_flags);
/* ... and which the solve passes took -- a word of its own: callers compare the word above as a whole. */
#define ADF_PATH_ROW_WEIGHTS_GUIDE 32 /* wave solver, full-resolution call: the row passes formed their edge weights from the
                                        guide rows themselves (FGS.cpp:607-614 inside the pass); the weight kernel wrote the
                                        vertical weights only and the horizontal plane was neither written nor read */
int adf_wls_get_last_solver_path(const adf_wls_t* h, int* path_flags);
/* ... and how the last row pass of the last filter call handed its solutions to the last column pass (a getter of its
 * own; the results do not depend on it): through the pair plane every other pass uses, or as the column pass's
 * register image -- wave solver, confidence mode, at least two iterations, ROIs of up to 4096 columns and 2176 rows,
 * chunks of at least twelve 4K pairs' worth of ROI pixels (92.9 Mpx).  ADF_LAST_HANDOFF_IMAGE=0 at handle creation forces the pair plane. */
#define ADF_HANDOFF_PAIR_PLANE 0
#define ADF_HANDOFF_IMAGE 1
#define ADF_HANDOFF_IMAGE_PAIR_TAIL 2 /* the full chunks the image, the shorter last chunk (below the size threshold) the pair plane */
int adf_wls_get_last_handoff(const adf_wls_t* h, int* form);
/* ... and how many of the INNER row -> column hand-offs (those of iterations before the last: num_iter - 1 of them)
 * took the register image in the last call's full chunks and in its shorter last chunk (equal to `full` where the call
 * has none).  An inner hand-off takes the image under the last one's conditions; the first one only where the first row
 * pass forms its right-hand sides from view-resolution int16 maps (float maps and the down-scaled path's interpolating
 * first pass keep the pair plane there).  A one-iteration call has no inner hand-off.  ADF_INNER_HANDOFF_IMAGE=0 at
 * handle creation keeps the inner hand-offs on the pair plane and leaves the last one alone; ADF_LAST_HANDOFF_IMAGE=0
 * keeps every hand-off there.  The results do not depend on either. */
int adf_wls_get_inner_handoffs(const adf_wls_t* h, int* full, int* tail);

/* DisparityFilter::filter (DF.hpp:75, DF.cpp:219-298) on a batch of n_pairs
 * independent, equally sized stereo pairs laid out `*_pair_stride` bytes apart
 * (n_pairs = 1 is the reference call).  disparity maps: CV_16SC1 (disparity*16; CV_32FC1 maps go through
 * adf_wls_filter_typed_* below), W x H; left_view: CV_8UC1 / CV_8UC3 (view_channels), same size; out: CV_16SC1,
 * W x H, filled with -16 outside the ROI (DF.cpp:254,284).  disp_right may be
 * NULL only for a filter created with use_confidence = 0.  roi: NULL or zero
 * area = derive from the offsets given at creation (DF.cpp:228-233). */
int adf_wls_filter_device(adf_wls_t* h, int n_pairs,
                          const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                          const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                          int view_channels, int W, int H,
                          int16_t* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                          const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                          const adf_rect* roi, void* stream);

int adf_wls_filter_host(adf_wls_t* h, int n_pairs,
                        const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                        const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                        int view_channels, int W, int H,
                        int16_t* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                        const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                        const adf_rect* roi);

/* The same call with disparity maps of a LOWER resolution than the view (DF.hpp:59-61: "Disparity map can
 * have any resolution, it will be automatically resized to fit left_view resolution"; DF.cpp:224-227,
 * 239-247, 268-277): maps are disp_W x disp_H, view and output W x H; the confidence map is computed at
 * the maps' resolution with LRC_thresh and the roll-off scaled by resize_factor = disp_W/W, then both are
 * resized (bilinear) and the disparity multiplied by W/disp_W.  roi is in disparity-map coordinates.
 * With disp_W == W and disp_H == H this is adf_wls_filter_*. */
int adf_wls_filter_scaled_device(adf_wls_t* h, int n_pairs,
                                 const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                 int disp_W, int disp_H,
                                 const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                                 int view_channels, int W, int H,
                                 int16_t* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                                 const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                 const adf_rect* roi, void* stream);
int adf_wls_filter_scaled_host(adf_wls_t* h, int n_pairs,
                               const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                               int disp_W, int disp_H,
                               const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                               int view_channels, int W, int H,
                               int16_t* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                               const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                               const adf_rect* roi);

/* Extension (no counterpart in the reference, which ends in disp_mul_conf.convertTo(dst, CV_16S), DF.cpp:296): the same
 * four calls with a CV_32FC1 filtered map that keeps what the rounding to 1/16 pixel throws away -- for callers that go
 * on to depth (f*B/d) or point clouds, where the 1/16-pixel staircase is the dominant error on small disparities.  Every
 * argument means what it means above; `out` is float*, W x H, strides in bytes.
 *   - Units: those of the int16 map, disparity * 16.  The value stored is exactly the float the int16 epilogue rounds:
 *     u0 * (1 / (u1 + EPS)) of the two filtered planes in confidence mode (DF.cpp:295; EPS = 1e-43f, DF.cpp:47), u0
 *     without confidence (DF.cpp:257-258).
 *   - Outside the ROI every pixel is -16.0f: the int16 map's fill, 16 * (min_disp - 1) with min_disp ignored
 *     (DF.cpp:146,149,254,284).
 *   - Where the int16 map saturates to -32768 because the value is not finite or |x| >= 2^31 (u1 == 0 exactly: a ROI
 *     without a single confident pixel gives 0 * inf), the float map holds -32768.0f.  It never holds NaN or inf.
 *     Finite values beyond the int16 range are stored as they are.
 *   - Rounding relation: for the same handle, inputs, parameters and solver, saturate_cast<short>(out_f32) -- cvRound,
 *     half to even, clamped to [-32768, 32767] -- equals the map adf_wls_filter* writes, bit for bit, inside and
 *     outside the ROI.
 *   - adf_wls_get_confidence_*, adf_wls_get_roi, adf_wls_get_last_solver, adf_wls_get_last_path, profiling (the float
 *     map counts 4 bytes per pixel), stream capture, the fallback to ADF_SOLVER_EXACT beyond 8192 x 4352 and the chunked
 *     workspace behave as for the int16 call.
 *   - Alignment: `out`, out_stride and out_pair_stride must be multiples of 4 bytes (ADF_EBADARG otherwise).  A base or
 *     strides that are not multiples of 8, or an odd ROI x, give the same bits through a slower store path. */
int adf_wls_filter_f32_device(adf_wls_t* h, int n_pairs,
                              const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                              const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                              int view_channels, int W, int H,
                              float* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                              const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                              const adf_rect* roi, void* stream);
int adf_wls_filter_f32_host(adf_wls_t* h, int n_pairs,
                            const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                            const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                            int view_channels, int W, int H,
                            float* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                            const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                            const adf_rect* roi);
int adf_wls_filter_scaled_f32_device(adf_wls_t* h, int n_pairs,
                                     const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                     int disp_W, int disp_H,
                                     const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                                     int view_channels, int W, int H,
                                     float* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                                     const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                     const adf_rect* roi, void* stream);
int adf_wls_filter_scaled_f32_host(adf_wls_t* h, int n_pairs,
                                   const int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                   int disp_W, int disp_H,
                                   const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                                   int view_channels, int W, int H,
                                   float* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride,
                                   const int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                   const adf_rect* roi);

/* Extension: float32 (CV_32FC1) disparity MAPS, through one typed pair of entries.  The reference asserts CV_16S maps
 * (DF.cpp:221,262); upstream OpenCV widened DisparityWLSFilter::filter to CV_32F later, so the definition is this library's
 * own, as with the float filtered map above.  For callers whose disparities are float already -- a learned matcher or a
 * cost-volume refinement on the same device, adf_wls_filter_f32_*'s own output -- and who would otherwise round them to
 * 1/16 pixel, the very information the float filtered map keeps.
 * adf_wls_filter_typed_*: the arguments of adf_wls_filter_scaled_* with the maps and `out` as void*, `disp_depth` (the
 * depth of BOTH maps) behind the left map's strides and `out_depth` behind the output's strides, each ADF_16S or ADF_32F
 * (ADF_EBADARG otherwise).  disp_W == W && disp_H == H is the plain call.  With disp_depth == ADF_16S the call is byte
 * for byte adf_wls_filter[_scaled][_f32]_*; the eight entries above keep their signatures and behaviour.
 * Float maps (disp_depth == ADF_32F):
 *   - Units: those of the int16 map, disparity * 16.  CV_32FC1, base and strides multiples of 4 bytes (ADF_EBADARG
 *     otherwise); left and right map have the same depth.  `out` must not overlap the maps (ADF_EBADARG).
 *   - For every element d two values are derived where it is loaded:
 *       v = isfinite(d) ? min(max(d, -32768.0f), 32767.0f) : -32768.0f     the value the solve uses;
 *       q = (int16_t)rintf(v), half to even                                the value the confidence map uses.
 *   - Confidence: the discontinuity maps (DF.cpp:161-210, 349-373), the discontinuity-aware left-right check
 *     (DF.cpp:306-341, including ridx = j - (q >> 4) and abs(q + qr) < thresh) and the low-resolution confidence of a
 *     scaled call are computed on q: adf_wls_get_confidence_* after a float call is bit for bit the map of the int16 call
 *     on the q maps.  (That arithmetic is integer sums and thresholds of 1.5 px; it gains nothing from sub-LSB input.)
 *   - Data term: u0 = c * v with confidence -- ONE float multiply where the int16 call has c * (float)d (DF.cpp:288-290)
 *     -- and u0 = v without (DF.cpp:250,257).  Weights, passes, epilogues, fill, ROI, chunking, solver fallback,
 *     profiling and stream capture are those of the int16 call.
 *   - Scaled calls (maps smaller than the view): the v map is resized with the float taps the confidence map goes
 *     through, then multiplied once, in float, by x_ratio = W / (float)disp_W (DF.cpp:241-244, 270-273): no rounding, no
 *     saturation.  The low-resolution confidence is computed on q with resize_factor, then resized, as for int16 maps.
 *     Such a call never reports ADF_PATH_SCALED_FUSED (it runs the resize kernels).
 *   - Relation R1, full-resolution calls: when every element of both maps is an integer in [-32768, 32767], the int16
 *     output and the float output are bit for bit those of the int16 call on the (int16_t) maps, with either solver, on
 *     every path, and adf_wls_get_last_path reports the same word.  It does NOT hold for scaled calls: the int16 call
 *     rounds (and saturates) the interpolated map, the float call does not.
 *   - Never NaN: for any input bits (NaN, +-inf, 1e30) the guarantees of the float filtered map above carry over -- no NaN
 *     or inf in the output, -16.0f outside the ROI, saturate_cast<short>(out_f32) == out_i16.
 *   - Workspace: a confidence-mode call keeps the two maps' q as int16 planes (one extra launch, 12 bytes per pixel of
 *     traffic, 4 bytes per pixel and pair of adf_wls_workspace_bytes); calls on int16 maps neither run it nor pay for it. */
int adf_wls_filter_typed_device(adf_wls_t* h, int n_pairs,
                                const void* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride, int disp_depth,
                                int disp_W, int disp_H,
                                const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                                int view_channels, int W, int H,
                                void* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride, int out_depth,
                                const void* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                const adf_rect* roi, void* stream);
int adf_wls_filter_typed_host(adf_wls_t* h, int n_pairs,
                              const void* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride, int disp_depth,
                              int disp_W, int disp_H,
                              const uint8_t* left_view, ptrdiff_t view_stride, ptrdiff_t view_pair_stride,
                              int view_channels, int W, int H,
                              void* out, ptrdiff_t out_stride, ptrdiff_t out_pair_stride, int out_depth,
                              const void* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                              const adf_rect* roi);

/* getConfidenceMap() (DF.hpp:117, DF.cpp:138): CV_32FC1, W x H, values in [0,255],
 * zero outside the ROI, of pair `pair` of the last filter call.  Valid until the
 * next filter call on the handle. */
int adf_wls_get_confidence_device(adf_wls_t* h, int pair, float* dst, ptrdiff_t dst_stride, void* stream);
int adf_wls_get_confidence_host(adf_wls_t* h, int pair, float* dst, ptrdiff_t dst_stride);
/* The HIP device the handle's workspace lives on (the device current at adf_wls_create); device
 * pointers and streams passed to the handle must belong to it. */
int adf_wls_get_device(const adf_wls_t* h, int* device);
/* getROI() (DF.hpp:120, DF.cpp:139): ROI used by the last filter call. */
int adf_wls_get_roi(const adf_wls_t* h, adf_rect* roi);
/* Block until everything the handle queued on `stream` has finished. */
int adf_wls_sync(adf_wls_t* h, void* stream);
/* Bytes of device workspace currently owned by the handle. */
size_t adf_wls_workspace_bytes(const adf_wls_t* h);

/* Measurement hook (no counterpart in the reference, which times filter() from outside with
 * getTickCount: samples/disparity_filtering.cpp:186-191).  While enabled, every kernel launch of
 * adf_wls_filter_device is bracketed by HIP events recorded on the caller's stream;
 * adf_wls_profile_read waits for them and returns per-kernel-class launch counts, summed durations
 * and the algorithmic bytes those launches moved (SURVEY.md 8d figures). */
typedef struct adf_kernel_time {
    char name[48];      /* kernel class, e.g. "pass_h", "pass_v", "weights"            */
    int launches;
    double total_ms;    /* sum of event-to-event durations                               */
    double alg_bytes;   /* algorithmic bytes summed over the launches                    */
    double moved_bytes; /* bytes this implementation reads+writes, by construction       */
} adf_kernel_time;
int adf_wls_profile_enable(adf_wls_t* h, int on); /* also clears what was collected */
int adf_wls_profile_read(adf_wls_t* h, adf_kernel_time* out, int capacity, int* count);

/* ---------------- FastGlobalSmootherFilter ---------------- */

/* createFastGlobalSmootherFilter(guide, lambda, sigma_color, lambda_attenuation,
 * num_iter) (EF.hpp:393, FGS.cpp:141-180, 681-684).  guide: CV_8UC1 / CV_8UC3,
 * w x h, HOST pointer (copied).  The weights are built once and reused by every
 * filter call, as in the reference. */
int adf_fgs_create(adf_fgs_t** out, const uint8_t* guide, ptrdiff_t guide_stride, int guide_channels,
                   int w, int h, double lambda, double sigma_color, double lambda_attenuation,
                   int num_iter, int solver);
/* The same with the guide already resident in HBM (a DEVICE pointer): the guide never crosses PCIe -- its copy into
 * the handle and the weight kernel are queued on `stream`, which is also the stream the handle's filter calls are
 * expected on.  (Creation still uploads the 768 KB weight table built on the host with libm, FGS.cpp:663-675, and
 * synchronises `stream` once for it.)  For device pipelines such as the second in-tree caller, which
 * smooths flow fields against an image it already holds (sparse_match_interpolators.cpp:202-203:
 * fastGlobalSmootherFilter(prevImage, flow, ...)). */
int adf_fgs_create_device(adf_fgs_t** out, const uint8_t* guide, ptrdiff_t guide_stride, int guide_channels,
                          int w, int h, double lambda, double sigma_color, double lambda_attenuation,
                          int num_iter, int solver, void* stream);
void adf_fgs_destroy(adf_fgs_t* h);
/* Filters made and destroyed per call -- the one-shot fastGlobalSmootherFilter (EF.hpp:413, FGS.cpp:687-691), the
 * reference's own perf test (perf/perf_fgs_filter.cpp:70-76) -- would pay hipMalloc + hipFree (which waits for the whole
 * device) and 3*256*256 libm calls for the weight table on every call.  The library therefore keeps a destroyed
 * filter's device block (at most 8 blocks / 3 GB per process, handed to the next filter behind the event of its last
 * user: no host synchronisation) and the weight tables by (device, sigma) (16 of them; the weighted median filter's
 * tables by (device, sigma, weight type), 16 more).  This returns all of it to the
 * driver; it waits for the blocks' last users.  (The library does the same on its own whenever one of its device
 * allocations -- a filter's workspace, a matcher's -- is refused for want of memory, and tries again; allocations the
 * CALLER makes in the same process do not see the cache: call this before a large one.) */
void adf_release_cached_memory(void);
/* The weight table of a sigma_color exactly as the filters build it (FGS.cpp:150-154, 663-675: 3*256*256 entries
 * -exp(-sqrt(i)/sigma) through the host's libm; built by several threads, the underflowed tail stored as -0.0f without
 * calling libm).  Host only -- no device is touched: the CPU test suite compares it bit for bit with the oracle's table. */
#define ADF_WEIGHT_TABLE_LEVELS (3 * 256 * 256)
int adf_weight_table_host(float sigma_color, float* table, int levels);
int adf_fgs_get_device(const adf_fgs_t* h, int* device);
/* Solver the handle actually runs: the one asked for at creation, except that ADF_SOLVER_WAVE covers guides up to
 * 8192 x 4352 (and at least 2 x 2) -- a larger or degenerate guide runs ADF_SOLVER_EXACT. */
int adf_fgs_get_solver(const adf_fgs_t* h, int* solver);

/* FastGlobalSmootherFilter::filter(src, dst) (EF.hpp:370, FGS.cpp:182-233).
 * src/dst: HOST pointers, same size as the guide, depth ADF_8U / ADF_16S / ADF_32F,
 * 1..4 interleaved channels; dst may alias src. */
int adf_fgs_filter_host(adf_fgs_t* h, const void* src, ptrdiff_t src_stride, void* dst,
                        ptrdiff_t dst_stride, int depth, int channels);
/* The same with DEVICE pointers, asynchronous on `stream` (a hipStream_t; NULL = the null
 * stream): for callers whose images already live in HBM (EdgeAwareInterpolator-style flow
 * post-filtering, sparse_match_interpolators.cpp:202-203).  dst may alias src.
 * Stream capture: the call may be captured into a hipGraph.  Calls on different streams are ordered by an event the
 * handle keeps; a call that is being captured neither waits for nor records it, so a handle whose calls are captured
 * must be used on ONE stream (captured and ordinary calls alike), and destroyed outside any capture once its graphs'
 * replays have finished (adf_fgs_destroy then synchronises the device instead of caching the handle's block). */
int adf_fgs_filter_device(adf_fgs_t* h, const void* src, ptrdiff_t src_stride, void* dst,
                          ptrdiff_t dst_stride, int depth, int channels, void* stream);

/* ---------------- evaluation utilities (DF.hpp:163-204) ---------------- */

#define ADF_UNKNOWN_DISPARITY 16320 /* DF.cpp:460 */

/* computeMSE(GT, src, ROI) (DF.hpp:176, DF.cpp:497-517): mean of (GT-src)^2 over ROI pixels whose
 * ground truth is known (!= 16320), divided by 256 (disparities are scaled by 16).  CV_16SC1 maps of
 * equal size W x H; `*_device` takes device pointers and synchronises `stream` to return the value. */
int adf_compute_mse_host(const int16_t* gt, ptrdiff_t gt_stride, const int16_t* src, ptrdiff_t src_stride,
                         int W, int H, const adf_rect* roi, double* mse);
int adf_compute_mse_device(const int16_t* gt, ptrdiff_t gt_stride, const int16_t* src, ptrdiff_t src_stride,
                           int W, int H, const adf_rect* roi, double* mse, void* stream);
/* computeBadPixelPercent(GT, src, ROI, thresh = 24) (DF.hpp:190, DF.cpp:519-539): percentage of known
 * ROI pixels with |GT-src| >= thresh. */
int adf_compute_bad_pixel_percent_host(const int16_t* gt, ptrdiff_t gt_stride, const int16_t* src, ptrdiff_t src_stride,
                                       int W, int H, const adf_rect* roi, int thresh, double* percent);
int adf_compute_bad_pixel_percent_device(const int16_t* gt, ptrdiff_t gt_stride, const int16_t* src, ptrdiff_t src_stride,
                                         int W, int H, const adf_rect* roi, int thresh, double* percent, void* stream);
/* getDisparityVis(src, dst, scale = 1.0) (DF.hpp:202, DF.cpp:541-556): CV_8U visualisation,
 * saturate_cast<uchar>(scale*src/16.0), unknown disparities -> 0. */
int adf_get_disparity_vis_host(const int16_t* src, ptrdiff_t src_stride, uint8_t* dst, ptrdiff_t dst_stride,
                               int W, int H, double scale);
int adf_get_disparity_vis_device(const int16_t* src, ptrdiff_t src_stride, uint8_t* dst, ptrdiff_t dst_stride,
                                 int W, int H, double scale, void* stream);

/* ---------------- block matcher feeding the filter ----------------
 * The reference's filter takes its maps from cv::StereoBM / cv::StereoSGBM (disparity_filters.cpp:386-449,
 * samples/disparity_filtering.cpp:151,214), classes of OpenCV's calib3d module that are not part of the
 * reference tree (parity unpinned there).  adf_bm_* is the published StereoBM algorithm on the device --
 * x-Sobel prefilter, SAD block matching, sub-pixel fit, CV_16SC1 output with 4 fractional bits, rejected
 * pixels = (minDisparity-1)*16 -- so a pair can go from views to filtered disparity without leaving HBM.
 * Bit-exact against oracle/adf_oracle_bm.c; pinned by the reference's own block-matching test data and
 * accuracy bar (modules/stereo/test/test_block_matching.cpp:61-82,148).  Limits: blockSize 5..21. */
typedef struct adf_bm adf_bm_t; /* cv::Ptr<StereoBM> */
/* StereoBM::create(numDisparities, blockSize); other parameters start at cv::StereoBM's defaults
 * (minDisparity 0, preFilterCap 31, textureThreshold 10, uniquenessRatio 15). */
int adf_bm_create(adf_bm_t** out, int num_disparities, int block_size);
void adf_bm_destroy(adf_bm_t* h);
/* The StereoMatcher / StereoBM setters in one call (the filter factory forces textureThreshold = 0 and
 * uniquenessRatio = 0, disparity_filters.cpp:399-400; the right-view matcher uses
 * minDisparity = -(min_disp+num_disp)+1, :424).  Values are checked at compute time like cv::StereoBM. */
int adf_bm_set_params(adf_bm_t* h, int min_disparity, int num_disparities, int block_size,
                      int prefilter_cap, int texture_threshold, int uniqueness_ratio);
int adf_bm_get_device(const adf_bm_t* h, int* device);
int adf_bm_get_params(const adf_bm_t* h, int* min_disparity, int* num_disparities, int* block_size,
                      int* prefilter_cap, int* texture_threshold, int* uniqueness_ratio);
/* The matching cost.  The reference's own block matcher, cv::stereo::StereoBinaryBM, matches census descriptors with a
 * Hamming distance (modules/stereo/src/stereo_binary_bm.cpp:367-408; setBinaryKernelType, kernelSize).  With a census cost
 *   cL, cR      = adf_census_transform_* (below) of the left and the right CV_8UC1 view at (cost_type, census_size):
 *                 dense 3 / 5 / 7, sparse 5 / 7 / 9 / 11, modified census (ADF_BM_COST_MCT_DENSE 3 / 5 / 7, _MCT_SPARSE
 *                 5 / 7 / 9 / 11: k * k * neighbour > window sum), centre-symmetric (ADF_BM_COST_CENSUS_CS 3 / 5 / 7 / 9:
 *                 neighbour > mirrored neighbour, 4 / 12 / 24 / 40 bits); neighbour coordinates clamped, so every
 *                 pixel has a descriptor; the matcher's time follows the byte planes, ceil(bits / 8);
 *   pixel cost  = popcount(cL(y, x) ^ cR(y, x - d));
 *   block cost  = S[k][x], the sum of the pixel cost over the full blockSize x blockSize window, d = minDisparity + k
 *                 (at most 21 * 21 * 48 = 21168);
 * and everything else is the SAD matcher's: the valid rectangle x in [max(maxD,0) + w/2, W + min(minD,0) - w/2),
 * y in [w/2, H - w/2), (minDisparity-1)*16 outside it, ties to the largest disparity (with a Hamming cost ties are the
 * rule: a flat image ties everywhere), the uniqueness test, the sub-pixel formula and the +15 >> 4 rounding.
 * preFilterCap and textureThreshold are validated as with SAD and NOT USED with a census cost: there is no prefiltered
 * image, hence no texture that could be summed (the filter factory sets textureThreshold to 0 anyway,
 * disparity_filters.cpp:399-400).  The definition is this library's own -- bit-exact against the direct statement
 * tests/bm_census_ref.py, NOT against the in-tree StereoBinaryBM, whose descriptors are no usable bit-level oracle (see
 * adf_census_transform_*) and whose median filters and 8-bit output are not built.
 * ADF_BM_COST_CENSUS_* / _MCT_* equal ADF_SGBM_COST_CENSUS_* / _MCT_*, which are accepted too.  An unknown (cost_type, census_size) pair is
 * ADF_EBADARG and the handle keeps its cost; census_size is ignored, and left as it was, with ADF_BM_COST_SAD.  A handle
 * may change cost between calls; adf_bm_compute_both_device shares the descriptor planes between the two views. */
#define ADF_BM_COST_SAD 0            /* cv::StereoBM's SAD on the x-Sobel prefiltered views (default) */
#define ADF_BM_COST_CENSUS_DENSE 1   /* cv::stereo CV_DENSE_CENSUS, census_size 3, 5, 7 */
#define ADF_BM_COST_CENSUS_SPARSE 2  /* cv::stereo CV_SPARSE_CENSUS, census_size 5, 7, 9, 11 */
/* (3 and 7 stay unassigned, as with ADF_SGBM_COST_*: callers rely on their being refused) */
#define ADF_BM_COST_MCT_DENSE 4      /* modified census (window mean), dense grid, census_size 3, 5, 7 */
#define ADF_BM_COST_MCT_SPARSE 5     /* modified census (window mean), sparse grid, census_size 5, 7, 9, 11 */
#define ADF_BM_COST_CENSUS_CS 6      /* cv::stereo CV_CS_CENSUS, centre-symmetric, census_size 3, 5, 7, 9 */
int adf_bm_set_cost(adf_bm_t* h, int cost_type, int census_size);
int adf_bm_get_cost(const adf_bm_t* h, int* cost_type, int* census_size); /* a new handle: ADF_BM_COST_SAD, 7 */
/* StereoMatcher::compute(left, right, disparity) on a batch of n_pairs equally sized CV_8UC1 pairs laid out
 * `*_pair_stride` bytes apart; disparity: CV_16SC1, W x H (strides in bytes).  Asynchronous on `stream`. */
int adf_bm_compute_device(adf_bm_t* h, int n_pairs,
                          const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                          const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                          int W, int H,
                          int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                          void* stream);
/* Extension (not a cv:: call): the left-view map of adf_bm_compute_device AND the map of the right-view matcher of
 * createRightMatcher (disparity_filters.cpp:417-431: views swapped, minDisparity = -(min_disp+num_disp)+1, texture
 * and uniqueness tests off) from one launch -- the two images are prefiltered once and both searches share a grid,
 * which matters for a single pair per call (1920x1080: 0.36 ms for two calls).  Results are identical to the two
 * separate computes. */
int adf_bm_compute_both_device(adf_bm_t* h, int n_pairs,
                               const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                               const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                               int W, int H,
                               int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                               int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                               void* stream);
int adf_bm_compute_host(adf_bm_t* h, int n_pairs,
                        const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                        const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                        int W, int H,
                        int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride);
/* The winning-cost map.  adf_bm_compute_cost_* are adf_bm_compute_* plus a CV_16SC1 cost plane (W x H, rows `cost_stride`,
 * pairs `cost_pair_stride` bytes apart, 2-byte aligned, non-NULL), what calib3d's StereoBM keeps for its own left-right
 * check (validateDisparity, below).  The disparity map is byte for byte the one adf_bm_compute_* writes, and
 *   - where the map holds a disparity other than (minDisparity-1)*16, the plane holds (int16_t)S[kb][x]: the aggregated
 *     cost (SAD or Hamming, every ADF_BM_COST_*) of the winning INTEGER disparity kb, before the sub-pixel fit;
 *   - where the map holds (minDisparity-1)*16 -- texture test, uniqueness test, rows and columns without a full window
 *     or search range -- the plane holds 0 (calib3d leaves those entries unwritten; 0 makes the plane deterministic).
 * The conversion is a plain truncation to 16 bits, because calib3d's cost map is CV_16S.  It changes a value only where a
 * cost can exceed 32767: a SAD is at most 2 * preFilterCap * blockSize^2, which passes 32767 only with blockSize 21 and
 * preFilterCap above 37, blockSize 19 and preFilterCap above 45, or blockSize 17 and preFilterCap above 56 -- never with
 * blockSize 15 or less; a census cost is at most 48 * 441 = 21168 and never truncates.  Parity with calib3d is UNPINNED
 * here as for the rest of the matcher (the class is outside the reference tree); the plane is bit-exact against the direct
 * statement tests/validate_ref.py.
 * adf_bm_compute_both_cost_device: both maps of adf_bm_compute_both_device and both planes; the right view's plane is the
 * cost of the createRightMatcher search, equal to what a separate adf_bm_compute_cost_device of that matcher writes. */
int adf_bm_compute_cost_device(adf_bm_t* h, int n_pairs,
                               const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                               const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                               int W, int H,
                               int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                               int16_t* cost, ptrdiff_t cost_stride, ptrdiff_t cost_pair_stride,
                               void* stream);
int adf_bm_compute_cost_host(adf_bm_t* h, int n_pairs,
                             const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                             const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                             int W, int H,
                             int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                             int16_t* cost, ptrdiff_t cost_stride, ptrdiff_t cost_pair_stride);
int adf_bm_compute_both_cost_device(adf_bm_t* h, int n_pairs,
                                    const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                    const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                    int W, int H,
                                    int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                    int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                    int16_t* cost_left, ptrdiff_t cost_left_stride, ptrdiff_t cost_left_pair_stride,
                                    int16_t* cost_right, ptrdiff_t cost_right_stride, ptrdiff_t cost_right_pair_stride,
                                    void* stream);

/* ---------------- semi-global matcher feeding the filter ----------------
 * cv::StereoSGBM as the reference's sample configures it (samples/disparity_filtering.cpp:166-176, 229-235:
 * P1 = 24*w*w, P2 = 96*w*w, preFilterCap 63, MODE_SGBM_3WAY) and as its factories expect it
 * (disparity_filters.cpp:404-409, 432-445): the published semi-global algorithm (Hirschmueller 2008) with the
 * Birchfield-Tomasi block cost and three paths (MODE_SGBM_3WAY: left, top, right; MODE_SGBM: five, MODE_HH: eight --
 * modules/stereo/src/stereo_binary_sgbm.cpp:173-186, 286-301 is the in-tree statement of the path sets), sub-pixel fit,
 * 3x3 median of the result;
 * CV_16SC1 with 4 fractional bits, invalid pixels (minDisparity-1)*16, matchable columns
 * [max(minDisparity+numDisparities,0), W+min(minDisparity,0)).  The class itself lives in OpenCV's calib3d (outside
 * the reference tree: parity unpinned); results are bit-exact against oracle/adf_oracle_sgbm.c and anchored on the
 * reference's own semi-global test (modules/stereo/test/test_block_matching.cpp:157-238).  The matchers' own speckle
 * filter (speckleWindowSize > 0) is not run by compute(), and the filter's factories switch it off anyway; the same
 * step exists as the separate call adf_filter_speckles_* below.  Limits: numDisparities <= 512, blockSize odd <= 11. */
#define ADF_SGBM_MODE_SGBM 0
#define ADF_SGBM_MODE_HH 1
#define ADF_SGBM_MODE_3WAY 2 /* StereoSGBM::MODE_SGBM_3WAY */
typedef struct adf_sgbm adf_sgbm_t; /* cv::Ptr<StereoSGBM> */
/* StereoSGBM::create(minDisparity, numDisparities, blockSize); the other parameters start at its defaults
 * (P1 = P2 = 0, preFilterCap 0, uniquenessRatio 0, disp12MaxDiff 0, mode MODE_SGBM). */
int adf_sgbm_create(adf_sgbm_t** out, int min_disparity, int num_disparities, int block_size);
void adf_sgbm_destroy(adf_sgbm_t* h);
int adf_sgbm_get_device(const adf_sgbm_t* h, int* device);
int adf_sgbm_set_params(adf_sgbm_t* h, int min_disparity, int num_disparities, int block_size, int P1, int P2,
                        int prefilter_cap, int uniqueness_ratio, int mode);
/* StereoSGBM::setDisp12MaxDiff: the matcher's own left-right check (stereo_binary_sgbm.cpp:548-556, 598-613 is the in-tree
 * statement).  cv::StereoSGBM::create's default 0 is read as 1 by the algorithm (check ON, :141); the filter factory sets
 * 1000000 (disparity_filters.cpp:389, 444), which switches it off. */
int adf_sgbm_set_disp12_max_diff(adf_sgbm_t* h, int disp12_max_diff);
int adf_sgbm_get_disp12_max_diff(const adf_sgbm_t* h, int* disp12_max_diff);
int adf_sgbm_get_params(const adf_sgbm_t* h, int* min_disparity, int* num_disparities, int* block_size, int* P1, int* P2,
                        int* prefilter_cap, int* uniqueness_ratio, int* mode);
/* The matching cost.  The reference's own semi-global matcher, cv::stereo::StereoBinarySGBM, matches on census
 * descriptors with a Hamming distance (modules/stereo/src/stereo_binary_sgbm.cpp; setBinaryKernelType, stereo.hpp:227-228;
 * descriptor.cpp:54-75), and its test is this library's anchor (test_block_matching.cpp:157-238).  With a census cost
 *   pixel cost  = popcount(census(left)(y, x) ^ census(right)(y, x - d)), the descriptors of adf_census_transform_*
 *                 below at (cost_type, census_size): census dense 3 / 5 / 7 and sparse 5 / 7 / 9 / 11, modified census
 *                 (ADF_SGBM_COST_MCT_DENSE 3 / 5 / 7, _MCT_SPARSE 5 / 7 / 9 / 11), centre-symmetric census
 *                 (ADF_SGBM_COST_CENSUS_CS 3 / 5 / 7 / 9);
 *   block cost  = the sum of pixel costs over the blockSize x blockSize window, window coordinates clamped to the rows
 *                 [0, H) and to the matchable columns -- the rule of the Birchfield-Tomasi path, at most 11*11*48;
 * and everything from the cost volume on (paths, winner, uniqueness, sub-pixel fit, left-right check, median) is the
 * same code.  preFilterCap is ignored; views must be CV_8UC1 (descriptor.cpp:58), 3 channels are ADF_EBADARG at compute
 * time.  Path costs are bounded by the block cost, so P1 / P2 want the scale of blockSize^2 * bits, not of
 * Birchfield-Tomasi costs.  The definition is this library's own (see adf_census_transform_*): bit-exact against the
 * direct statement tests/census_ref.py, NOT against the in-tree code.
 * census_size is validated here (ADF_EBADARG; the handle keeps its cost) and ignored, and left as it was, with ADF_SGBM_COST_BT.
 * A handle may change cost between calls. */
#define ADF_SGBM_COST_BT 0            /* cv::StereoSGBM's Birchfield-Tomasi block cost (default) */
#define ADF_SGBM_COST_CENSUS_DENSE 1  /* cv::stereo CV_DENSE_CENSUS (descriptor.hpp:58, descriptor.cpp:65-69), census_size 3, 5, 7 */
#define ADF_SGBM_COST_CENSUS_SPARSE 2 /* cv::stereo CV_SPARSE_CENSUS (descriptor.cpp:70-74), census_size 5, 7, 9, 11 */
/* 3 and 7 stay unassigned: callers (and this library's tests) rely on (3, 5) and (7, 5) being refused as unknown types, so
 * the newer descriptors start at 4. */
#define ADF_SGBM_COST_MCT_DENSE 4     /* modified census transform (Froeba & Ernst 2004; cv::stereo CV_MODIFIED_CENSUS_TRANSFORM's
                                         rule): neighbours against the window mean, dense grid, census_size 3, 5, 7 */
#define ADF_SGBM_COST_MCT_SPARSE 5    /* the same rule on the sparse grid, census_size 5, 7, 9, 11 */
#define ADF_SGBM_COST_CENSUS_CS 6     /* centre-symmetric census (Spangenberg et al. 2013; cv::stereo CV_CS_CENSUS,
                                         descriptor.hpp:59): neighbours against their mirror image, census_size 3, 5, 7, 9 */
int adf_sgbm_set_cost(adf_sgbm_t* h, int cost_type, int census_size);
int adf_sgbm_get_cost(const adf_sgbm_t* h, int* cost_type, int* census_size); /* a new handle: ADF_SGBM_COST_BT, 7 */
/* StereoMatcher::compute(left, right, disparity) on n_pairs equally sized CV_8UC1 / CV_8UC3 pairs (`channels`);
 * disparity: CV_16SC1, W x H (strides in bytes).  Asynchronous on `stream`. */
int adf_sgbm_compute_device(adf_sgbm_t* h, int n_pairs,
                            const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                            const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                            int channels, int W, int H,
                            int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                            void* stream);
int adf_sgbm_compute_host(adf_sgbm_t* h, int n_pairs,
                          const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                          const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                          int channels, int W, int H,
                          int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride);
/* Extension (not a cv:: call): both views' maps from one call, what DisparityWLSFilter::filter(dispL, view, out, dispR)
 * takes.  disp_left is adf_sgbm_compute_*'s map with the handle's settings, byte for byte (uniquenessRatio and the
 * matcher's own left-right check included).  disp_right (CV_16SC1, W x H, non-NULL, 2-byte aligned, not overlapping
 * disp_left) comes from `right_source`; any other value is ADF_EBADARG:
 *
 * ADF_SGBM_RIGHT_MATCHER (0): the map of createRightMatcher's matcher (disparity_filters.cpp:432-445) -- views swapped,
 *   minDisparity = 1 - minDisparity - numDisparities, uniquenessRatio 0, disp12MaxDiff 1000000; P1, P2, mode,
 *   preFilterCap, cost type and census size are the handle's -- as a second run through the same workspace inside the
 *   call.  Identical to the two separate computes, and as expensive.
 *
 * ADF_SGBM_RIGHT_FROM_VOLUME (1): a speed-for-fidelity option.  The right view's map is read from the LEFT view's
 *   aggregated volume along its diagonals (Hirschmueller 2008 derives the match image's map "from the same costs, by
 *   traversing the epipolar line"), inside the winner pass: no second cost volume, no second set of path passes.  It is
 *   NOT the right matcher's map, because the paths were aggregated along the left image.  The definition, with
 *   md = minDisparity, nd = numDisparities, matched left columns [minX1, maxX1) = [max(md+nd, 0), W + min(md, 0)),
 *   w1 = maxX1 - minX1, and S[y][x1][k] (x1 in [0, w1), k in [0, nd)) the final summed path cost, the very value the left
 *   winner reads, bit for bit.  For row y and right-view column xr in [0, W):
 *     1. Candidates K = { k in [0, nd) : minX1 <= xr + md + k < maxX1 }, s(k) = S[y][xr + md + k - minX1][k].  Partial
 *        ranges count: every xr with at least one candidate gets a winner (md = 0: columns 1 ... W-1).
 *     2. invalid_R = -(md + nd) * 16, the (minDisparity_R - 1) * 16 of the right matcher.  If K is empty, or
 *        m = min s(k) >= SHRT_MAX, the raw value is invalid_R.
 *     3. The winner k* is the LARGEST k with s(k) = m: the right matcher's own "first minimum" in its own index
 *        d' = nd - 1 - k.
 *     4. Sub-pixel fit only if 0 < k* < nd-1 and both k*-1 and k*+1 are in K: den = max(s(k*+1) + s(k*-1) - 2m, 1),
 *        d'16 = d' * 16 + trunc(((s(k*+1) - s(k*-1)) * 16 + den) / (2 * den)), C truncation toward zero
 *        (stereo_binary_sgbm.cpp:584-591 in the right matcher's index); otherwise d'16 = d' * 16.
 *     5. Raw value d'16 + (1 - md - nd) * 16: k* = 0 gives -md * 16, every value is <= -md * 16, as the right matcher's.
 *     6. No uniqueness test and no left-right check on this map; then the 3x3 median of every map of this matcher, over
 *        a raw plane pre-filled with invalid_R.
 *   When w1 <= 0 both maps are entirely invalid.  Bit-exact against the direct statement tests/sgbm_both_ref.py.
 *   Agreement with the right matcher's map, MEASURED ON THE CPU with that statement on ONE fixture (Tsukuba, 384 x 288,
 *   16 disparities; share of columns 1 ... W-nd-1 within 1 px): Birchfield-Tomasi, block 3 or 5, 3-way, the sample's
 *   P1 / P2, cap 63: 95.8 %; census dense 5, block 3, 3-way, P1 72 / P2 288: 92.6 %; census dense 7, block 5, MODE_SGBM,
 *   P1 200 / P2 800: 92.8 %.  The filtered map against ground truth (oracle.wls_filter; block 3: MSE 1.451, bad 5.20 %
 *   with this map; 1.392, 4.94 % with the right matcher's; 1.597, 6.15 % unfiltered; block 5: 1.598, 5.28 % / 1.551,
 *   4.91 % / 1.709, 6.51 %): the filter still improves the raw map, by a little less than with the genuine right map.
 *   Limits: the winner pass keeps a row of each map and a ring of numDisparities live right columns in LDS (16 W bytes
 *   + at most 16 KiB; 32 W with the matcher's own left-right check) within 150 KiB: images up to 8576 columns, 4288 with
 *   disp12MaxDiff below 100000 -- wider calls are ADF_ESIZE and launch nothing.  Workspace per image in flight:
 *   adf_sgbm_compute_*'s (two signal or descriptor planes, three H x w1 x nd int16 volumes, one W x H int16 raw map)
 *   plus a second W x H int16 raw map; ADF_SGBM_RIGHT_MATCHER takes exactly adf_sgbm_compute_*'s. */
#define ADF_SGBM_RIGHT_MATCHER 0
#define ADF_SGBM_RIGHT_FROM_VOLUME 1
int adf_sgbm_compute_both_device(adf_sgbm_t* h, int n_pairs,
                                 const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                 const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                 int channels, int W, int H,
                                 int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                 int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                 int right_source, void* stream);
int adf_sgbm_compute_both_host(adf_sgbm_t* h, int n_pairs,
                               const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                               const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                               int channels, int W, int H,
                               int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                               int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                               int right_source);

/* ---------------- census transform (cv::stereo::censusTransform) ----------------
 * cv::stereo::censusTransform(image, kernelSize, dist, type) (descriptor.hpp:428, descriptor.cpp:77-98) on n_images
 * equally sized CV_8UC1 images, rows `src_stride` and images `src_image_stride` bytes apart: the published transform
 * (Zabih & Woodfill 1994), one uint64 descriptor per pixel, rows `dst_stride` and images `dst_image_stride` bytes apart.
 * census_type is one of ADF_SGBM_COST_CENSUS_DENSE, _CENSUS_SPARSE, _MCT_DENSE, _MCT_SPARSE, _CENSUS_CS (or its
 * ADF_BM_COST_* twin), census_size the odd window size k, n2 = k / 2:
 *   - dense (descriptor.cpp:65-69): offsets -n2 .. n2 in both directions, k in {3, 5, 7}: 8 / 24 / 48 bits;
 *   - sparse (every second pixel, descriptor.cpp:70-74): offsets -n2, -n2 + 2, ... <= n2, k in {5, 7, 9, 11}:
 *     8 / 16 / 24 / 36 bits;
 *   - the offset (0, 0) is skipped where it occurs; a bit is 1 when neighbour > centre (descriptor.hpp:182-194);
 *   - neighbour coordinates are clamped to the image (replicated edge): every pixel has a descriptor, also in an image
 *     smaller than the window;
 *   - bit order: rows top to bottom, left to right within a row; the first comparison is the most significant of the
 *     bits used, the upper bits are zero.
 * Two more comparison rules run on the same clamped window, in the same raster order, with the same bit order and the
 * same strict `>` (stated directly in tests/census_variants_ref.py; the device is bit-exact against it):
 *   - ADF_SGBM_COST_MCT_DENSE, k in {3, 5, 7}, and ADF_SGBM_COST_MCT_SPARSE, k in {5, 7, 9, 11}: the modified census
 *     transform (Froeba & Ernst 2004; the rule of cv::stereo's CV_MODIFIED_CENSUS_TRANSFORM).  The offsets, hence the bit
 *     counts (8 / 24 / 48; 8 / 16 / 24 / 36), are the dense / sparse ones above, (0, 0) skipped.  S is the sum of all
 *     k * k pixels of the clamped k x k window around the pixel, centre included (the sparse grids use the full window
 *     too); a bit is 1 when k * k * p(y+dy, x+dx) > S: integers, no division, no rounding rule, at most 121 * 255.
 *   - ADF_SGBM_COST_CENSUS_CS, k in {3, 5, 7, 9}: the centre-symmetric census (Spangenberg et al. 2013; cv::stereo's
 *     CV_CS_CENSUS).  The offsets are the first half of the window in raster order: every dx in [-n2, n2] for dy in
 *     [-n2, -1], then dx in [-n2, -1] for dy = 0; a bit is 1 when p(y+dy, x+dx) > p(y-dy, x-dx), both coordinates
 *     clamped: 4 / 12 / 24 / 40 bits.  k = 11 would take 60 bits and is refused (at most 48).
 *   Not built: cv::stereo's CV_MODIFIED_CS_CENSUS, CV_MEAN_VARIATION and CV_STAR_KERNEL, and the modified census's threshold.
 * This is the library's OWN definition, not bit parity with the in-tree code, which is no usable bit-level oracle: its
 * row ranges read one row past Range::end (descriptor.hpp:219), it compares a row offset with a row index where it
 * means to skip the centre (`ii != i`, descriptor.hpp:234), and it leaves the border pixels unwritten (:222); it keeps
 * 32 bits (dense up to 5 only, descriptor.cpp:83).  Every other (type, size) is ADF_EBADARG; dst and its strides must
 * be 8-byte aligned (ADF_EBADARG).  src and dst must not overlap.
 * _device: device pointers on the current HIP device, asynchronous on `stream`; no allocation, no synchronisation, so
 * the call may be captured into a hipGraph.  _host: host pointers; copies, runs and synchronises. */
int adf_census_transform_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                                int W, int H, int census_type, int census_size,
                                uint64_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride, void* stream);
int adf_census_transform_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                              int W, int H, int census_type, int census_size,
                              uint64_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride);

/* ---------------- speckle filter (cv::filterSpeckles) ----------------
 * cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, buf) of OpenCV's calib3d, the step a StereoBM / StereoSGBM
 * pipeline runs on the matcher's output; the in-tree call site is modules/stereo/src/stereo_binary_sgbm.cpp:716-718:
 * filterSpeckles(disp, (minDisparity-1)*16, speckleWindowSize, 16*speckleRange, buffer).  Semantics:
 *   - pixels equal to new_val belong to no component;
 *   - 4-neighbours p, q are in one component when both differ from new_val and |d(p) - d(q)| <= max_diff (int32);
 *   - every component of AT MOST max_speckle_size pixels is set to new_val; every other pixel keeps its value;
 *   - max_speckle_size <= 0 changes nothing; a negative max_diff makes every pixel its own component.
 * The result does not depend on how components are labelled: bit-exact against a sequential restatement and
 * identical from run to run.  calib3d is outside the reference tree, so parity with it is UNPINNED; what OpenCV does
 * when built with IPP is not known here.  cv's newVal and maxDiff are doubles: the C++ and Python layers round them
 * half-to-even (cvRound) before they reach these ints.
 * CV_16SC1 maps only (what both matchers produce; CV_8UC1 is not supported), n_maps equally sized maps `map_stride`
 * bytes apart, modified IN PLACE.  new_val must lie in [-32768, 32767] (ADF_EBADARG); W*H must be below 2^31
 * (int32 labels, ADF_ESIZE).
 * workspace (cv's buf): device memory of at least adf_filter_speckles_workspace_bytes(n_maps, W, H) bytes (int32
 * label + int32 count per pixel, 8 B/px), 4-byte aligned; with it the call allocates nothing and never synchronises,
 * so it may be captured into a hipGraph.  NULL = scratch from the library's cache of device blocks, ordered on
 * `stream` behind its previous user (no host synchronisation; the first call of a size allocates it; not capturable).
 * _device: device pointers, asynchronous on `stream`, on the current HIP device.  _host: host pointers, copies,
 * runs and synchronises. */
size_t adf_filter_speckles_workspace_bytes(int n_maps, int W, int H);
int adf_filter_speckles_device(int n_maps, int16_t* img, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                               int new_val, int max_speckle_size, int max_diff,
                               void* workspace, size_t workspace_bytes, void* stream);
int adf_filter_speckles_host(int n_maps, int16_t* img, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                             int new_val, int max_speckle_size, int max_diff);

/* ---------------- validateDisparity (the block matcher's own left-right check) ----------------
 * calib3d's validateDisparity(disp, cost, minDisparity, numberOfDisparities, disp12MaxDiff), the step
 * cv::StereoBM::compute runs on its map and on the aggregated cost of each winning disparity (adf_bm_compute_cost_*)
 * when 0 <= disp12MaxDiff.  The chain of the canonical stereo sample is three calls:
 *     adf_bm_compute_cost_device -> adf_validate_disparity_device -> adf_filter_speckles_device.
 * n_maps equally sized CV_16SC1 maps `map_stride` bytes apart, modified IN PLACE; cost: a plane of cost_type ADF_16S or
 * ADF_32S (calib3d accepts CV_16S and CV_32S) per map, read only.  Every row of every map is independent, all
 * arithmetic is int32:
 *     minD = min_disparity, maxD = minD + num_disparities, INV = (minD-1)*16, X0 = max(maxD, 0), X1 = W + min(minD, 0)
 *   1. disp2[x2] = INV and cost2[x2] = INT_MAX for every x2 in [0, W);
 *   2. x ascending in [X0, X1) with d = disp[x] != INV, c = cost[x]: x2 = x - ((d + 8) >> 4); if cost2[x2] > c then
 *      (cost2, disp2)[x2] = (c, d).  The comparison is strict: among equal costs the smallest x wins, and a CV_32S cost
 *      of INT_MAX never wins;
 *   3. x in [X0, X1) with d = disp[x] != INV, d0 = d >> 4, d1 = (d + 15) >> 4: disp[x] = INV only if for d0 AND for d1
 *      0 <= x-dk < W, disp2[x-dk] > INV and |disp2[x-dk] - d| > 16 * disp12_max_diff.  A candidate outside the row or on
 *      an empty disp2 keeps the pixel.
 * Deviation: a pixel whose x2 of step 2 falls outside [0, W) does not vote; calib3d indexes out of bounds there.  Maps of
 * this library's matcher never produce that case (d lies in [minD*16, (maxD-1)*16]: the sub-pixel term is 0 at both ends
 * of the search).  calib3d is outside the reference tree, so parity with it is UNPINNED; the device is bit-exact against
 * the sequential statement tests/validate_ref.py and identical from run to run (csrc/validate_kernels.hip).
 * Refused: disp12_max_diff < 0 ("off" is the matcher's business, not this function's) or above 2^26, num_disparities <= 0,
 * INV outside CV_16S, an unknown cost_type, NULL pointers, misaligned images (all ADF_EBADARG); W above
 * ADF_VALIDATE_MAX_WIDTH -- a row is held on chip -- and strides smaller than a row (ADF_ESIZE).
 * Stateless: no workspace, no allocation, no synchronisation on the device path, so the call may be captured into a
 * hipGraph.  _device: device pointers, asynchronous on `stream`, on the current HIP device.  _host: host pointers,
 * copies, runs and synchronises. */
#define ADF_VALIDATE_MAX_WIDTH 15360
int adf_validate_disparity_device(int n_maps, int16_t* disp, ptrdiff_t stride, ptrdiff_t map_stride,
                                  const void* cost, ptrdiff_t cost_stride, ptrdiff_t cost_map_stride, int cost_type,
                                  int W, int H, int min_disparity, int num_disparities, int disp12_max_diff, void* stream);
int adf_validate_disparity_host(int n_maps, int16_t* disp, ptrdiff_t stride, ptrdiff_t map_stride,
                                const void* cost, ptrdiff_t cost_stride, ptrdiff_t cost_map_stride, int cost_type,
                                int W, int H, int min_disparity, int num_disparities, int disp12_max_diff);

/* ---------------- the matcher's views (cv::resize to half size, cv::cvtColor BGR2GRAY) ----------------
 * The two imgproc calls the sample's default pipeline makes before matching (samples/disparity_filtering.cpp:130-141):
 *     resize(left, left_for_matcher, Size(), 0.5, 0.5);              both views, colour
 *     cvtColor(left_for_matcher, left_for_matcher, COLOR_BGR2GRAY);  StereoBM only
 * on n_images equally sized 8-bit images, rows `stride` bytes apart, images `image_stride` bytes apart (all left views
 * then all right views, or interleaved pairs: both are a batch of images).  Four cases:
 *     src_channels 3 -> dst_channels 3, half size     resize(.., 0.5, 0.5) on CV_8UC3
 *     src_channels 1 -> dst_channels 1, half size     the same on CV_8UC1
 *     src_channels 3 -> dst_channels 1, same size     cvtColor(COLOR_BGR2GRAY)
 *     src_channels 3 -> dst_channels 1, half size     both in one sweep (the half-size colour image is never written)
 * (dst_W, dst_H) must be (W, H) or (adf_half_size(W), adf_half_size(H)).  Every other scale, 1 -> 3 channels, 4 channels
 * and a same-size call that would change nothing are ADF_EBADARG; general INTER_LINEAR is not built.
 * Arithmetic, all integer, so every case is bit-exact and the fused case equals the two-step case:
 *   - half size: the destination is cvRound(W * 0.5) x cvRound(H * 0.5), half to even (1242 x 375 -> 621 x 188); cv::resize
 *     with INTER_LINEAR at a scale of exactly 2 in both directions is the 2x2 mean, (a + b + c + d + 2) >> 2 per channel;
 *   - where the last destination column or row has a single source column / row (W or H = 3 mod 4), the sample is the
 *     mean over the source pixels that exist, cvRound((float)sum / count), half to even;
 *   - gray: (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 on the 8-bit channels (in the fused case: the rounded ones),
 *     channel order B, G, R.
 * imgproc is outside the reference tree.  The even-size case is what the replay of the tutorial's pair against its
 * published result images rests on; for odd sizes (the single-column / single-row tail) parity with OpenCV is UNPINNED:
 * the rule above is this library's definition.
 * src and dst must not overlap.  Destination images of a batch must not overlap each other (they follow one another,
 * or interleave row by row).  Images whose source base and strides are 16-byte aligned and whose destination base and
 * strides are 16-byte aligned (8 is enough at half size) take the vector path; anything else is computed byte by byte
 * (same results, slower).
 * _device: device pointers on the current HIP device, asynchronous on `stream`; no allocation, no synchronisation, so
 * the call may be captured into a hipGraph.  _host: host pointers; copies, runs and synchronises. */
int adf_half_size(int n, int* half); /* cvRound(n * 0.5), half to even: every layer computes dsize with it */
int adf_prepare_views_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                             int W, int H, int src_channels,
                             uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride,
                             int dst_W, int dst_H, int dst_channels, void* stream);
int adf_prepare_views_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                           int W, int H, int src_channels,
                           uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride,
                           int dst_W, int dst_H, int dst_channels);

/* ---------------- reprojection to 3-D (cv::reprojectImageTo3D) and the point list ----------------
 * cv::reprojectImageTo3D(disparity, _3dImage, Q, handleMissingValues, ddepth) of OpenCV's calib3d, the call a stereo
 * pipeline makes after filtering: from a disparity map and the 4x4 matrix Q of stereoRectify to an XYZ image, and --
 * an extension -- to a compact list of the valid points.  n_maps equally sized maps `map_stride` bytes apart, CV_16SC1
 * (ADF_16S) or CV_32FC1 (ADF_32F); CV_8U / CV_32S maps are not supported.
 *
 * Reprojection.  Map pixel (x, y) with raw source value s, Q row-major doubles:
 *     d   = (double)s * disp_scale                 (disp_scale = 1.0 is cv's behaviour: no division by 16 for CV_16S)
 *     r_i = ((Q[i][0]*x + Q[i][1]*y) + Q[i][3]) + Q[i][2]*d          i = 0..3
 *     iw  = 1.0 / r_3
 *     X = r_0*iw, Y = r_1*iw, Z = r_2*iw           stored as (float)X, (float)Y, (float)Z (round to nearest)
 *   - every product, sum and the division is ONE IEEE binary64 operation, in exactly this order; no fused multiply-add;
 *   - nothing is sanitised: r_3 == 0 gives +-inf or NaN as the arithmetic gives them, as in cv.  The sign and payload of
 *     a NaN are not part of the contract.
 * calib3d is outside the reference tree, so parity with it is UNPINNED: this is the library's own definition, bit-exact
 * against the direct NumPy statement tests/reproject_ref.py.  One known difference: cv accumulates Q[i][0] column by
 * column in double (x additions) instead of multiplying by x, which differs in the last bits of a double before the
 * rounding to float.
 *
 * Missing values (missing_mode):
 *     ADF_MISSING_NONE  0  no pixel is missing
 *     ADF_MISSING_MIN   1  cv's handleMissingValues = true: m = the minimum raw source value of THAT map -- each map of a
 *                          batch has its own, taken over the whole map (not a ROI), NaN in a float map ignored (a map of
 *                          NaN only has m = NaN: nothing is missing)
 *     ADF_MISSING_VALUE 2  extension: m = missing_value, no reduction launch.  Suits this library's own fills: -16 outside
 *                          the filter's ROI, (minDisparity - 1) * 16 from the matchers
 *   missing(s) <=> fabs((double)s - m) <= FLT_EPSILON, tested on RAW values (before disp_scale).  A missing pixel gets
 *   Z = 10000.0f (cv's bigZ); its X and Y stay as computed.
 *
 * Outputs.  out_channels = 3: CV_32FC3, interleaved XYZ.  out_channels = 1 (extension): the Z plane only, a CV_32FC1 depth
 * map.  cv's ddepth CV_16SC3 / CV_32SC3 are not built.  `out`, out_stride and out_map_stride must be multiples of 4 bytes;
 * a source whose base and strides are multiples of 8 (CV_16S) or 16 bytes (CV_32F) is read with one load per four pixels,
 * an output whose base and strides are multiples of 16 bytes is written with 16-byte stores; anything else gives the same
 * bits element by element (slower).
 *
 * Point list.  valid(p) <=> p lies inside `roi` (NULL = whole map) and not missing(s) and Xf, Yf, Zf are all finite and
 * z_min <= Zf <= z_max (doubles; -infinity / +infinity switch the range off; NaN is refused).  Per map, the k-th valid
 * pixel in raster order (y major, x minor) gives points[k] = (Xf, Yf, Zf) -- the bits of the reprojection above --,
 * optionally colours[k] = the `view` pixel (view_channels = 1 or 3 bytes, as the view has) and index[k] = y*W + x
 * (int32).  counts[map] = the number of valid pixels, even when it exceeds `capacity`; entries k >= capacity are not
 * written and nothing beyond min(count, capacity) is touched.  Lists of map k start k * *_map_stride BYTES after the first.
 * The result is identical from run to run.  `points` and points_map_stride (and index) must be multiples of 4 bytes.
 *
 * W*H must be below 2^31 (ADF_ESIZE), for the image too.
 *
 * Conventions (as adf_filter_speckles_* and adf_census_transform_*): calls run on the current HIP device; `prm` is a HOST
 * pointer in both forms -- Q travels in the kernel arguments, there is no upload.  Workspace: adf_reproject_workspace_bytes
 * (4 bytes per map, read and written with ADF_MISSING_MIN only; the other modes use none and ignore the argument) /
 * adf_point_cloud_workspace_bytes (the minimum slots and one uint32 per tile of 1024 pixels), 4-byte aligned device
 * memory.  With a caller workspace the _device calls allocate nothing, never synchronise and may be captured into a
 * hipGraph; with workspace = NULL they take scratch from the library's cache of device blocks (not capturable).  In the
 * _device form `counts` is a device pointer too.  _host: host pointers (counts on the host); copies, runs, synchronises. */
#define ADF_MISSING_NONE 0
#define ADF_MISSING_MIN 1
#define ADF_MISSING_VALUE 2
typedef struct adf_reproject_params { double Q[16]; double disp_scale; int missing_mode; double missing_value; } adf_reproject_params;
size_t adf_reproject_workspace_bytes(int n_maps);
int adf_reproject_to_3d_device(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride,
                               int W, int H, const adf_reproject_params* prm, float* out, ptrdiff_t out_stride,
                               ptrdiff_t out_map_stride, int out_channels, void* workspace, size_t workspace_bytes, void* stream);
int adf_reproject_to_3d_host(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride,
                             int W, int H, const adf_reproject_params* prm, float* out, ptrdiff_t out_stride,
                             ptrdiff_t out_map_stride, int out_channels);
size_t adf_point_cloud_workspace_bytes(int n_maps, int W, int H);
int adf_point_cloud_device(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                           const adf_reproject_params* prm, const adf_rect* roi, double z_min, double z_max,
                           const uint8_t* view, ptrdiff_t view_stride, ptrdiff_t view_map_stride, int view_channels,
                           float* points, ptrdiff_t points_map_stride, uint8_t* colours, ptrdiff_t colours_map_stride,
                           int32_t* index, ptrdiff_t index_map_stride, int capacity, uint32_t* counts,
                           void* workspace, size_t workspace_bytes, void* stream);
int adf_point_cloud_host(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                         const adf_reproject_params* prm, const adf_rect* roi, double z_min, double z_max,
                         const uint8_t* view, ptrdiff_t view_stride, ptrdiff_t view_map_stride, int view_channels,
                         float* points, ptrdiff_t points_map_stride, uint8_t* colours, ptrdiff_t colours_map_stride,
                         int32_t* index, ptrdiff_t index_map_stride, int capacity, uint32_t* counts);

/* ---------------- rectification (cv::initUndistortRectifyMap, cv::remap) ----------------
 * The two calls a stereo pipeline makes in front of everything above: cv::initUndistortRectifyMap(K, dist, R, P, size,
 * CV_32FC1, map1, map2) once per camera and cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, borderValue) per
 * frame, with K, dist of the calibration and R1/P1 (R2/P2) of the caller's stereoRectify -- the same stereoRectify whose Q
 * adf_reproject_* takes.  adf_rectify_views_* (extension) is both in one launch: the maps never exist in memory.
 * calib3d and imgproc are outside the reference tree, so parity with OpenCV is UNPINNED: what follows is the library's own
 * definition, bit-exact against the direct NumPy statement tests/rectify_ref.py.
 *
 * Parameters (host only).  adf_rectify_params_init(K, dist, n_dist, R, P, p_cols, out): K, dist, R, P are cv's cameraMatrix,
 * distCoeffs, R and newCameraMatrix, row-major doubles.
 *   - fx, fy, cx, cy = K[0], K[4], K[2], K[5]; the skew K[1] is ignored, as in cv;
 *   - dist in cv's order k1 k2 p1 p2 k3 k4 k5 k6; n_dist 0, 4, 5 or 8 (missing entries are 0; dist may be NULL with 0).  n_dist
 *     12 or 14 (thin prism, tilt) and every other count are ADF_EBADARG: those models are not built;
 *   - R: 9 doubles, NULL = identity; P: 3 x p_cols with p_cols 3 or 4 (ADF_EBADARG otherwise), only P[:, :3] is read;
 *   - ir = the inverse of A = P[:, :3] * R (A = P[:, :3] itself when R is NULL), in binary64, in this order:
 *         A[i][j] = (P[i][0]*R[0][j] + P[i][1]*R[1][j]) + P[i][2]*R[2][j]
 *         the signed cofactors, two products and one difference each:
 *           c00 = a11*a22 - a12*a21   c01 = a12*a20 - a10*a22   c02 = a10*a21 - a11*a20
 *           c10 = a02*a21 - a01*a22   c11 = a00*a22 - a02*a20   c12 = a01*a20 - a00*a21
 *           c20 = a01*a12 - a02*a11   c21 = a02*a10 - a00*a12   c22 = a00*a11 - a01*a10
 *         the determinant by the first row: det = (a00*c00 + a01*c01) + a02*c02
 *         one division per entry: ir[3*i + j] = c_ji / det      (the adjugate is the transposed cofactor matrix)
 *     det == 0 or a non-finite det is ADF_EBADARG.  Every layer (Python, C++) calls this function: one inverse.
 *
 * Maps.  adf_init_undistort_rectify_map_* writes two CV_32FC1 planes of W x H; for destination pixel (u, v), with
 * k1..k6, p1, p2 from dist, every operator below ONE IEEE binary64 operation in exactly this order, no fused multiply-add:
 *     X = (ir0*u + ir1*v) + ir2      Y = (ir3*u + ir4*v) + ir5      D = (ir6*u + ir7*v) + ir8
 *     w = 1.0 / D        x = X*w        y = Y*w
 *     x2 = x*x    y2 = y*y    r2 = x2 + y2    xy2 = (2.0*x)*y
 *     kr = (1.0 + ((k3*r2 + k2)*r2 + k1)*r2) / (1.0 + ((k6*r2 + k5)*r2 + k4)*r2)
 *     xd = (x*kr + p1*xy2) + p2*(r2 + 2.0*x2)
 *     yd = (y*kr + p1*(r2 + 2.0*y2)) + p2*xy2
 *     mapx = (float)(fx*xd + cx)     mapy = (float)(fy*yd + cy)         (round to nearest)
 *   Nothing is sanitised: D == 0 gives inf or NaN as the arithmetic gives them; the sign and payload of a NaN are not part
 *   of the contract.  Known differences from cv: cv accumulates ir0, ir3, ir6 along u (u additions) instead of multiplying by
 *   u, and cv's SIMD builds fuse multiply-adds; both differ in the last bits of a double before the rounding to float.
 *   Only the CV_32FC1 pair is built: cv's CV_16SC2 + CV_16UC1 fixed-point pair and convertMaps are not.  The maps and their
 *   strides must be multiples of 4 bytes (ADF_EBADARG); multiples of 16 are written with 16-byte stores.  W*H < 2^31.
 *
 * Sampling.  adf_remap_*: n_images equally sized 8-bit images of 1 or 3 channels (srcW x srcH, rows src_stride bytes
 * apart, images src_image_stride bytes apart) through ONE map pair of W x H into n_images destinations of W x H.  Only
 * ADF_INTER_LINEAR with ADF_BORDER_CONSTANT is accepted; everything else is ADF_EBADARG.  border_value: 3 bytes (a 1-channel
 * image reads the first; NULL = 0).  Per destination pixel, float and integer arithmetic, 5 fractional bits as cv's
 * INTER_TAB_SIZE = 32:
 *     tx = mapx*32.0f   ty = mapy*32.0f
 *     ok = tx >= -1048576.0f && tx <= 1048575.0f && ty >= -1048576.0f && ty <= 1048575.0f       (false for NaN)
 *     not ok: every channel = border_value[c]
 *     sx = (int)rintf(tx) (half to even)   ix = sx >> 5   ax = sx & 31          (the same for y)
 *     tap(i, j) = 0 <= i < srcW && 0 <= j < srcH ? src[j][i][c] : border_value[c]
 *     out = (tap(ix,iy)*(32-ax)*(32-ay) + tap(ix+1,iy)*ax*(32-ay) + tap(ix,iy+1)*(32-ax)*ay + tap(ix+1,iy+1)*ax*ay + 512) >> 10
 *   This equals cv's 15-bit table form (its weights are these times 32, its rounding +16384 >> 15).  A tap outside the source
 *   is never loaded.  Limits: srcW, srcH <= 32767 and W*H < 2^31 (ADF_ESIZE).  src and dst must not overlap; destination
 *   images of a batch must not overlap each other (they follow one another, or interleave row by row).  A destination whose
 *   base and strides are multiples of 4 bytes is written with whole 4- / 12-byte stores, maps whose bases and strides are
 *   multiples of 16 are read with 16-byte loads; anything else gives the same bits byte by byte (slower).
 *
 * adf_rectify_views_* takes the arguments of adf_remap_* with the parameters in place of the maps, evaluates the
 * coordinates and samples in one launch, and gives the bits of the two-step form: it is the per-frame call, its bytes one
 * read of the source plus one write of the destination.
 *
 * Conventions (as adf_reproject_* and adf_prepare_views_*): _device runs on the current HIP device, asynchronously on
 * `stream`, allocates nothing and never synchronises, so it may be captured into a hipGraph; `prm` and border_value are HOST
 * pointers in both forms -- they travel in the kernel arguments, there is no upload.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_INTER_LINEAR 1    /* cv::INTER_LINEAR */
#define ADF_BORDER_CONSTANT 0 /* cv::BORDER_CONSTANT */
typedef struct adf_rectify_params { double fx, fy, cx, cy; double dist[8]; double ir[9]; } adf_rectify_params;
int adf_rectify_params_init(const double K[9], const double* dist, int n_dist, const double* R /* 9, NULL = I */,
                            const double* P /* 9 or 12 */, int p_cols /* 3 or 4 */, adf_rectify_params* out);
int adf_init_undistort_rectify_map_device(const adf_rectify_params* prm, int W, int H, float* mapx, ptrdiff_t mapx_stride,
                                          float* mapy, ptrdiff_t mapy_stride, void* stream);
int adf_init_undistort_rectify_map_host(const adf_rectify_params* prm, int W, int H, float* mapx, ptrdiff_t mapx_stride,
                                        float* mapy, ptrdiff_t mapy_stride);
int adf_remap_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW, int srcH,
                     int channels, const float* mapx, ptrdiff_t mapx_stride, const float* mapy, ptrdiff_t mapy_stride,
                     uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride, int W, int H, int interpolation,
                     int border_mode, const uint8_t* border_value /* 3 */, void* stream);
int adf_remap_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW, int srcH,
                   int channels, const float* mapx, ptrdiff_t mapx_stride, const float* mapy, ptrdiff_t mapy_stride,
                   uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride, int W, int H, int interpolation,
                   int border_mode, const uint8_t* border_value /* 3 */);
int adf_rectify_views_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW,
                             int srcH, int channels, const adf_rectify_params* prm, uint8_t* dst, ptrdiff_t dst_stride,
                             ptrdiff_t dst_image_stride, int W, int H, int interpolation, int border_mode,
                             const uint8_t* border_value /* 3 */, void* stream);
int adf_rectify_views_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW,
                           int srcH, int channels, const adf_rectify_params* prm, uint8_t* dst, ptrdiff_t dst_stride,
                           ptrdiff_t dst_image_stride, int W, int H, int interpolation, int border_mode,
                           const uint8_t* border_value /* 3 */);

/* ---------------- weighted median filter (cv::ximgproc::weightedMedianFilter) ----------------
 * cv::ximgproc::weightedMedianFilter(joint, src, dst, r, sigma, weightType, mask) (weighted_median_filter.hpp:64-90,
 * weighted_median_filter.cpp; Zhang et al., "100+ Times Faster Weighted Median Filter"): the operator that fills and
 * de-noises a disparity map from the map's own values -- edge-aware through a joint image, blind to masked pixels (which
 * is what fills holes), and returning only values that occur in the window, so it never blends foreground and background.
 * In the chain: matcher -> adf_validate_disparity_* / adf_filter_speckles_* -> this, with ignore_value =
 * (minDisparity-1)*16 -> adf_reproject_*; or in front of the WLS filter.
 *
 * This is the library's OWN definition: the reference cannot be matched bit for bit (below).  The rule it converges to
 * (weighted_median_filter.cpp:493-543: the smallest cut with non-negative balance) is kept.
 *
 * Inputs.  n_maps equally sized maps of W x H, `*_map_stride` bytes apart, rows `*_stride` bytes apart.
 *   - src, dst: ONE channel, depth ADF_8U, ADF_16S or ADF_32F, dst of the same depth.  Multi-channel sources are not
 *     built: callers split them.
 *   - joint: 8-bit, joint_channels 1 or 3 (interleaved), the size of src.
 *   - mask (optional): an 8-bit plane of that size, 0 = ignored; NULL = no mask.
 *   - use_ignore != 0 with ignore_value (optional; ignore_value is not looked at otherwise).
 * Whether a tap is used.  Pixel q is used when mask(q) != 0 and, with use_ignore, src(q) != ignore_value (compared as
 * doubles).  In a float map a NaN is never used; +-inf are ordinary ordered values; float values are ordered as IEEE
 * totals, -0.0 below +0.0, and the output is the BITS of a tap.  For ADF_8U and ADF_16S ignore_value must be an integer
 * inside the depth's range (ADF_EBADARG otherwise).
 * Window.  For pixel p every q with |qx - px| <= r and |qy - py| <= r inside the image: clipped at the border, nothing is
 * replicated (as weighted_median_filter.cpp:437-441, 549-550).
 * Weights, all integers.  w(p, q) = T[ sum_c (joint_c(p) - joint_c(q))^2 ], the index 0 .. 3*255^2:
 *   - ADF_WMF_EXP: T[i] = (uint32_t)lrint(exp(-(double)i / (2.0 * sigma * sigma)) * 65536.0), built on the host with libm
 *     like the filters' table (adf_weight_table_host).  For a 1-channel joint this is weighted_median_filter.cpp:252-263
 *     in fixed point; for 3 channels it is the EXACT colour distance where the reference has its cluster centres;
 *   - ADF_WMF_OFF: T[i] = 65536, the plain median of the used pixels;
 *   - cv's WMF_IV1, WMF_IV2, WMF_COS and WMF_JAC are not built: every other weight_type is ADF_EBADARG.
 * Result.  Tot = sum of w over the used taps, L(v) = sum of w over the used taps with src(q) <= v: dst(p) is the smallest
 * tap value v with 2 * L(v) >= Tot.  Tot == 0 -- no tap used, or every used tap of weight 0 -- gives dst(p) = src(p)
 * unchanged.  A pixel that is itself unused still gets its result from its neighbours: that is the hole filling.
 * Radius.  1 <= r <= ADF_WMF_MAX_RADIUS = 31; the bound is arithmetic: 63^2 * 65536 < 2^28, so Tot and 2 * L fit unsigned
 * 32-bit.  Every sum is an integer sum: the result does not depend on summation order, is bit-exact against the direct
 * NumPy statement tests/wmf_ref.py and identical from run to run (csrc/wmf_kernels.hip).
 * Deviations from the reference, all deliberate:
 *   - fixed-point integer weights where it accumulates floats in a history-dependent order (:55-131, 277-347, 475-543);
 *   - the exact colour distance of a 3-channel joint where it k-means-clusters the joint to 256 indices;
 *   - ADF_16S and ADF_32F sources are NOT quantised to 256 levels: the result is one of the source's own values;
 *   - four weight types (IV1, IV2, COS, JAC) and multi-channel sources are not built.
 * Refused: sigma not finite or not > 0, r outside [1, 31], an unknown depth, weight_type or joint_channels, NULL joint /
 * src / dst, bases or strides not aligned to the depth (2 bytes for ADF_16S, 4 for ADF_32F), dst overlapping (by the byte
 * ranges they span) src, joint or mask (all ADF_EBADARG); W*H at or above 2^31, strides smaller than a row, destination
 * maps of a batch that overlap each other (ADF_ESIZE).  All of this is checked before a device is touched.
 *
 * adf_wmf_weight_table_host: T exactly as the calls build it, ADF_WMF_TABLE_LEVELS entries.  Host only -- no device is
 * touched.
 * (the device copy of T lives in a process-wide cache by (device, sigma, weight type), 16 of them, which
 * adf_release_cached_memory frees: coming back to a sigma is free and capturable; a NEW value builds its table on the
 * host inside the call and uploads it with one synchronous copy -- use each sigma once BEFORE capturing calls with it into
 * a hipGraph.  Every later call with that sigma allocates nothing and never synchronises.)
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_WMF_EXP 0 /* cv::ximgproc::WMF_EXP */
#define ADF_WMF_OFF 5 /* cv::ximgproc::WMF_OFF */
#define ADF_WMF_WEIGHT_ONE 65536
#define ADF_WMF_TABLE_LEVELS (3 * 256 * 256)
#define ADF_WMF_MAX_RADIUS 31
int adf_wmf_weight_table_host(double sigma, int weight_type, uint32_t* table, int levels);
int adf_weighted_median_filter_device(int n_maps,
                                      const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                      const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int depth,
                                      void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                      int W, int H, int r, double sigma, int weight_type,
                                      const uint8_t* mask, ptrdiff_t mask_stride, ptrdiff_t mask_map_stride,
                                      int use_ignore, double ignore_value, void* stream);
int adf_weighted_median_filter_host(int n_maps,
                                    const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                    const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int depth,
                                    void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                    int W, int H, int r, double sigma, int weight_type,
                                    const uint8_t* mask, ptrdiff_t mask_stride, ptrdiff_t mask_map_stride,
                                    int use_ignore, double ignore_value);

/* ---------------- guided filter (cv::ximgproc::guidedFilter / GuidedFilter) ----------------
 * createGuidedFilter(guide, radius, eps) (EF.hpp:158), GuidedFilter::filter(src, dst, dDepth) (EF.hpp:143) and
 * guidedFilter(guide, src, dst, radius, eps, dDepth) (EF.hpp:180; modules/ximgproc/src/guided_filter.cpp = GF.cpp; He et
 * al., "Guided Image Filtering"): per window a linear model q = a . I + b of the source in the guide, the models of all
 * windows that cover a pixel averaged.  No recursion along a scanline: two streaming launches per call.  In the chain:
 * matcher -> adf_validate_disparity_* / adf_filter_speckles_* -> adf_weighted_median_filter_* (which fills the holes: this
 * filter is NOT blind to (minDisparity-1)*16, it blends it in) -> this -> adf_reproject_*; or on the float map of a
 * learned matcher.
 *
 * This is the library's OWN definition.  It keeps GF.cpp's window, border, meaning of eps and linear model; it has exact
 * integer statistics and one stated operation order, so the result is bit-exact against the direct NumPy statement
 * tests/gf_ref.py and identical from run to run.
 *
 * Inputs.  n_maps equally sized maps of W x H, `*_map_stride` bytes apart, rows `*_stride` bytes apart.
 *   - guide: 8-bit, guide_channels 1 or 3 (interleaved), the size of src.
 *   - src: ONE channel, depth ADF_8U, ADF_16S or ADF_32F.
 *   - dst: one channel, depth dst_depth, any of the three, independent of src's (cv's dDepth).
 *   - 0 <= r <= ADF_GF_MAX_RADIUS = 31.
 *   - eps finite and > 0, in squared grey levels of the 0..255 guide (GF.cpp:333, 354: the guide is not scaled to [0, 1]).
 * Window and border.  The (2r+1)^2 square, N = (2r+1)^2, at every depth with BORDER_REFLECT (GF.cpp:160-163): index i of
 * an axis of length n reads m = i mod 2n (non-negative), then m < n ? m : 2n-1-m.  The radius may exceed the image
 * (numpy.pad(mode="symmetric")).
 * Stage 1, the coefficients of every pixel's window (I_c the guide's channels, p the source):
 *   - integer sources: S_c = sum I_c, S_cd = sum I_c I_d, S_p = sum p, S_cp = sum I_c p are integers;
 *     V_cd = N S_cd - S_c S_d and n_c = N S_cp - S_c S_p in int64 (every term is below 3969^2 * 255 * 32768 < 2^53, so their
 *     conversion to double is exact);
 *   - E = eps * (double)N * (double)N, evaluated left to right;
 *   - ADF_32F sources: S_p and S_cp are double sums of (double)p and (double)I_c * (double)p in the fixed order of stage 2
 *     (column first, then row); n_c = (double)N * S_cp - (double)S_c * S_p.  Integer-valued float maps therefore give the
 *     int16 call's bits; non-finite source values give what IEEE arithmetic gives in that order;
 *   - 1 channel: a_0 = (float)(n_0 / (V_00 + E));
 *   - 3 channels, in double, no contraction, exactly these expressions:
 *       s00 = V_00 + E, s11 = V_11 + E, s22 = V_22 + E, s01 = V_01, s02 = V_02, s12 = V_12;
 *       c00 = s11*s22 - s12*s12, c01 = s02*s12 - s01*s22, c02 = s01*s12 - s02*s11;
 *       c11 = s00*s22 - s02*s02, c12 = s01*s02 - s00*s12, c22 = s00*s11 - s01*s01;
 *       det = (s00*c00 + s01*c01) + s02*c02;
 *       a_0 = (float)(((c00*n_0 + c01*n_1) + c02*n_2) / det);
 *       a_1 = (float)(((c01*n_0 + c11*n_1) + c12*n_2) / det);
 *       a_2 = (float)(((c02*n_0 + c12*n_1) + c22*n_2) / det);
 *     det not finite or not > 0: every a_c is 0;
 *   - b = (float)((((double)S_p - (double)a_0 * S_0) - (double)a_1 * S_1 - (double)a_2 * S_2) / (double)N), the
 *     subtractions left to right.
 * Stage 2, the output.  SA_c and SB are the float32 window sums of a_c and b in ONE fixed order:
 *   - the column sum C(y, x) = ((v(y-r, x) + v(y-r+1, x)) + ...) + v(y+r, x), top to bottom, reflected indices, every
 *     partial sum rounded to float32;
 *   - then the row sum S(y, x) = ((C(y, x-r) + C(y, x-r+1)) + ...) + C(y, x+r), left to right;
 *   - q = (((double)SB + (double)SA_0 * I_0) + (double)SA_1 * I_1 + (double)SA_2 * I_2) / (double)N, left to right;
 *   - dst = (float)q for ADF_32F; rint(q) (half to even, cv's saturate_cast) saturated to the depth for ADF_8U / ADF_16S
 *     (a NaN gives the depth's minimum, as cv's saturate_cast does).
 * Deviations from the reference, all deliberate:
 *   - exact covariances where it forms mean(I p) - mean(I) mean(p) in float32 (GF.cpp:487-510, 330-358): on CV_16S
 *     disparities mean(I p) reaches 10^6..10^7, where a float32 ulp is 0.5..1, so its covariance is wrong by about its own
 *     size wherever the guide is flat;
 *   - CV_16S sources (it takes CV_8U and CV_32F only, GF.cpp:707);
 *   - one-channel sources only (callers split them, as with the weighted median);
 *   - guides of 1 or 3 channels of 8 bits;
 *   - the guide's statistics are recomputed per call: there is no init stage (they ride along in the same kernel);
 *   - its box means are cv::boxFilter(..., BORDER_REFLECT) of un-vendored OpenCV: bit parity is unpinnable.
 * Refused: eps not finite or not > 0, r outside [0, 31], an unknown depth or guide_channels, NULL guide / src / dst, bases
 * or strides not aligned to the depth (2 bytes for ADF_16S, 4 for ADF_32F), dst overlapping (by the byte ranges they span)
 * guide or src (all ADF_EBADARG); W*H at or above 2^31, strides smaller than a row, destination maps of a batch that
 * overlap each other (ADF_ESIZE).  All of this is checked before a device is touched.
 * Workspace: the coefficient planes between the two launches, (guide_channels + 1) float planes per map --
 * adf_guided_filter_workspace_bytes(n_maps, W, H, guide_channels) bytes of 4-byte aligned device memory (0 for arguments
 * the calls refuse).  workspace == NULL takes library scratch from the process-wide cache (no allocation once it is
 * warm); a caller-supplied workspace makes the call capturable into a hipGraph.
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_GF_MAX_RADIUS 31
size_t adf_guided_filter_workspace_bytes(int n_maps, int W, int H, int guide_channels);
int adf_guided_filter_device(int n_maps,
                             const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                             const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                             void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                             int W, int H, int r, double eps,
                             void* workspace, size_t workspace_bytes, void* stream);
int adf_guided_filter_host(int n_maps,
                           const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                           const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                           void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                           int W, int H, int r, double eps);

/* ---------------- domain transform filter (cv::ximgproc::dtFilter / DTFilter), recursive mode ----------------
 * createDTFilter(guide, sigmaSpatial, sigmaColor, mode, numIters) (EF.hpp:100), DTFilter::filter(src, dst, dDepth)
 * (EF.hpp:80) and dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters) (EF.hpp:120;
 * modules/ximgproc/src/dtfilter_cpu.hpp = DT.hpp, dtfilter_cpu.inl.hpp = DT.inl; Gastal and Oliveira, "Domain Transform
 * for Edge-Aware Image and Video Processing"): in mode DTF_RF one iteration is four first-order recursive sweeps over the
 * map -- along every row there and back, then along every column -- whose feedback falls with the guide's difference
 * between the two pixels of a step.  No window and no tridiagonal solve: the cheapest edge-aware refinement of a
 * disparity map.  In the chain it stands where the guided filter does.
 *
 * This is the library's OWN definition.  It keeps DT's distance, its sigma schedule and its recurrence in DT's order of
 * evaluation, which IS the definition; it builds the feedback table with one rounding per entry.  The result is bit-exact
 * against the direct NumPy statement tests/dt_ref.py fed with adf_dt_rf_table_host, and identical from run to run.
 *
 * Inputs.  n_maps equally sized maps of W x H, `*_map_stride` bytes apart, rows `*_stride` bytes apart.
 *   - guide: 8-bit, guide_channels 1 or 3 (interleaved), the size of src.
 *   - src: ONE channel, depth ADF_8U, ADF_16S or ADF_32F.
 *   - dst: one channel, depth dst_depth, any of the three, independent of src's (cv's dDepth).
 *   - mode: ADF_DTF_RF.  These entry points refuse ADF_DTF_NC and ADF_DTF_IC (windows of variable width in the transformed
 *     domain) as not built: ADF_DTF_NC lives under its own names, adf_dt_window_filter_* (the next section); ADF_DTF_IC is
 *     NOT built.
 * Parameters, as DT.inl:79-83 clamps them: ss = max(1.0f, (float)sigmaSpatial), sr = max(0.01f, (float)sigmaColor),
 * N = max(1, numIters).
 * Distance (DT.hpp:115-118).  k = ss / sr in float32.  For the L1 difference L of two guide pixels (the sum over the
 * channels of |difference|: 0..255 for 1 channel, 0..765 for 3) d_L = 1.0f + k * (float)L, the product and the sum each
 * rounded to float32.
 * Feedback table, one row per iteration i = 1..N, 255 * guide_channels + 1 entries each:
 *   - sigmaH_i = ss * 2^(N-i) / sqrt(4^N - 1) in double, left to right (DT.hpp:120-123);
 *   - A_i[L] = (float)exp((-sqrt(2/3) / sigmaH_i) * (double)d_L), in double, libm's exp on the host.
 *   adf_dt_rf_table_host writes the N rows, row i - 1 first, exactly as the calls build them.  Host only -- no device is
 *   touched.  (The calls hand a row to their kernels with the launch: there is no device table to build or cache.)
 * Recurrence (DT.inl:407-415, 438-466), on x = (float)src, for i = 1..N:
 *   - every row, left to right, j = 1..W-1:   x[j] = x[j] + A_i[L(j-1, j)] * (x[j-1] - x[j]);
 *   - then right to left, j = W-2..0:         x[j] = x[j] + A_i[L(j, j+1)] * (x[j+1] - x[j]);
 *   - then the same down (1..H-1) and up (H-2..0) every column, L between the two rows.
 *   Subtraction, product and sum are each rounded to float32 (no FMA).  W == 1 leaves the rows as they are, H == 1 the
 *   columns.  Every step is a convex combination of two values of the map: a constant map comes back exactly.
 * Output.  dst = x for ADF_32F; rint(x) (half to even, cv's saturate_cast) saturated to the depth for ADF_8U / ADF_16S
 * (a NaN gives the depth's minimum).
 * Deviations from the reference, all deliberate:
 *   - DT rounds alpha = exp(-sqrt(2/3) / sigmaH_1) and log(alpha) to float, runs cv::exp once over a float plane of
 *     d * log(alpha), and squares that plane in place for each later iteration (DT.inl:401-405, 539-561): its weights
 *     of iteration i carry 2^(i-1) accumulated roundings.  Ours carry one; the cost is measured in tests/test_dt_ref.py;
 *   - the weights are not a plane: they are one table read per step, recomputed from the guide in every sweep, so there
 *     is no init stage (DTFilter keeps the guide and the parameters);
 *   - one-channel sources only (callers split them); guides of 1 or 3 channels of 8 bits;
 *   - DTF_NC and DTF_IC are refused here (DTF_NC is adf_dt_window_filter_*).
 * Refused: mode ADF_DTF_NC or ADF_DTF_IC (not built) and any other mode but ADF_DTF_RF, sigmas that are not finite (as
 * double or as float32), numIters above ADF_DT_MAX_ITERS = 8, an unknown depth or guide_channels, NULL guide / src / dst,
 * n_maps, W or H below 1, bases or strides not aligned to the depth (2 bytes for ADF_16S, 4 for ADF_32F), dst
 * overlapping (by the byte ranges they span) guide or src (all ADF_EBADARG); W*H at or above 2^31, strides smaller than
 * a row, destination maps of a batch that overlap each other, a workspace that is too small (ADF_ESIZE).  All of this is
 * checked before a device is touched.
 * Workspace: the map between the passes, one float plane per map -- adf_dt_filter_workspace_bytes(n_maps, W, H) bytes of
 * 4-byte aligned device memory (0 for arguments the calls refuse).  workspace == NULL takes library scratch from the
 * process-wide cache (no allocation once it is warm); a caller-supplied workspace makes the call capturable into a
 * hipGraph.
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_DTF_NC 0 /* cv::ximgproc::DTF_NC: adf_dt_window_filter_* (adf_dt_filter_* refuses it as not built) */
#define ADF_DTF_IC 1 /* cv::ximgproc::DTF_IC: not built */
#define ADF_DTF_RF 2 /* cv::ximgproc::DTF_RF */
#define ADF_DT_MAX_ITERS 8
size_t adf_dt_filter_workspace_bytes(int n_maps, int W, int H);
int adf_dt_rf_table_host(double sigma_spatial, double sigma_color, int num_iters, int guide_channels, float* table);
int adf_dt_filter_device(int n_maps,
                         const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                         const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                         void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                         int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters,
                         void* workspace, size_t workspace_bytes, void* stream);
int adf_dt_filter_host(int n_maps,
                       const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                       const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                       void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                       int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters);

/* ---------------- domain transform filter, normalized convolution (cv::ximgproc::dtFilter, mode DTF_NC) ----------------
 * The reference's DEFAULT mode (dtFilter(..., int mode = DTF_NC, ...), createDTFilter likewise; EF.hpp:100-120, DT.hpp,
 * DT.inl): per iteration every pixel becomes the plain mean of the map over a window along its row, then along its
 * column, the window being the pixels within a radius of it in the transformed domain -- the pixel distance plus the
 * guide's differences walked over.  No sequential chain along a scanline: every pixel finds its own window.  It arrives
 * under names of its own because adf_dt_filter_* is pinned to refuse ADF_DTF_NC; a binding of the reference routes
 * mode == DTF_NC to adf_dt_window_filter_* and mode == DTF_RF to adf_dt_filter_* (INTEGRATION.md, section 2.13).
 *
 * This is the library's OWN definition.  The result is bit-exact against the direct NumPy statement
 * tests/dt_window_ref.py fed with adf_dt_nc_radii_host, and identical from run to run.
 *
 * Inputs: those of adf_dt_filter_* -- n_maps maps of W x H; guide 8-bit with 1 or 3 interleaved channels; src ONE channel
 * of depth ADF_8U, ADF_16S or ADF_32F; dst one channel of depth dst_depth, independent of src's.  mode: ADF_DTF_NC.
 * Parameters, clamped as DT.inl:79-83 does and as adf_dt_filter_* does: ss = max(1.0f, (float)sigmaSpatial),
 * sr = max(0.01f, (float)sigmaColor), N = max(1, numIters), N <= ADF_DT_MAX_ITERS.  k = ss / sr in float32.
 * Radii (DT.hpp:120-128).  sigmaH_i = ss * 2^(N-i) / sqrt(4^N - 1) in double, r_i = (float)(3.0 * sigmaH_i), i = 1..N;
 *   R_i = floor(r_i).  adf_dt_nc_radii_host writes r_1 .. r_N exactly as the calls form them.  Host only -- no device is
 *   touched.
 * Distance, local and with one rounding.  For pixels a <= b of one scanline S(a, b) is the exact integer sum of the
 *   guide's L1 differences (the sum over the channels of |difference|: 0..255 per step for 1 channel, 0..765 for 3) over the
 *   steps between them, and D(a, b) = (float)(b - a) + k * (float)S(a, b): the two conversions, the product and the sum
 *   each rounded to float32 (no FMA).  D is non-decreasing in b - a, and D >= b - a.
 * Window of pixel j in a scanline of n pixels (the asymmetry is the reference's: getLeftBound uses >=, getRightBound <,
 *   DT.hpp:248-260):
 *   - lb is the smallest a in [0, j] with D(a, j) <= r_i;
 *   - rb is the largest b in [j, n-1] with b == j or D(j, b) < r_i.
 *   The window is contiguous, has at most 2 R_i + 1 pixels and is clipped by the ends of the scanline.
 * Pass.  y[j] = (x[lb] + x[lb+1] + ... + x[rb]) / (float)(rb - lb + 1): the sum runs left to right in float32, starting
 *   from x[lb], and is followed by one IEEE float32 division.  A pass reads one plane and writes another.
 * Call.  x = (float)src; for i = 1..N: every row with r_i, then every column with r_i (DT.inl:157-163).
 * Output, as in DTF_RF.  dst = x for ADF_32F; rint(x) (half to even) saturated to the depth for ADF_8U / ADF_16S (a NaN
 *   gives the depth's minimum).
 * Limit.  R_1 <= ADF_DT_NC_MAX_RADIUS = 127, else ADF_EBADARG.  It admits the reference's own perf configuration
 *   (sigmaSpatial = 80 at 3 iterations: r_1 = 120.9), bounds the halo a tile carries, and keeps every partial sum of the
 *   first pass over an ADF_16S map an integer below 2^24: that pass is exact, and an integer-valued constant map comes
 *   back exactly.
 * Deviations from the reference, all deliberate:
 *   - the reference compares float32 running sums of the distance along the whole scanline (idist[], DT.inl:484-491),
 *     which carry up to W accumulated roundings; ours is local, has one rounding and is translation-invariant;
 *   - the reference differences a float32 running integral of the row (integrateRow, DT.inl:211-221), which on a 4K row
 *     of 16-bit disparities passes 2^24 and loses integer bits; ours sums the window directly;
 *   - one-channel sources only (callers split them); guides of 1 or 3 channels of 8 bits;
 *   - DTF_IC stays unbuilt.
 *   Measured against the reference's arithmetic restated in NumPy (tests/test_dt_window_ref.py): DESIGN.md, section 26.
 * Refused: mode ADF_DTF_IC (not built), ADF_DTF_RF (it is adf_dt_filter_*'s) and any other mode but ADF_DTF_NC; R_1 above
 * ADF_DT_NC_MAX_RADIUS; and everything adf_dt_filter_* refuses, with the same status -- sigmas that are not finite (as
 * double or as float32), numIters above ADF_DT_MAX_ITERS, an unknown depth or guide_channels, NULL guide / src / dst,
 * n_maps, W or H below 1, bases or strides not aligned to the depth, dst overlapping guide or src (all ADF_EBADARG); W*H at
 * or above 2^31, strides smaller than a row, destination maps of a batch that overlap each other, a workspace that is too
 * small (ADF_ESIZE).  All of this is checked before a device is touched.
 * Workspace: the map between the passes, TWO float planes per map -- adf_dt_window_filter_workspace_bytes(n_maps, W, H)
 * bytes of 4-byte aligned device memory (0 for arguments the calls refuse).  The rules are adf_dt_filter_*'s: NULL takes
 * library scratch from the process-wide cache; a caller-supplied workspace makes the call capturable into a hipGraph (2 N
 * launches in one chain, no device table).
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_DT_NC_MAX_RADIUS 127
size_t adf_dt_window_filter_workspace_bytes(int n_maps, int W, int H);
int adf_dt_nc_radii_host(double sigma_spatial, int num_iters, float* radii);
int adf_dt_window_filter_device(int n_maps,
                                const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters,
                                void* workspace, size_t workspace_bytes, void* stream);
int adf_dt_window_filter_host(int n_maps,
                              const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                              const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                              void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                              int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters);

/* ---------------- joint bilateral filter (cv::ximgproc::jointBilateralFilter) ----------------
 * jointBilateralFilter(joint, src, dst, d, sigmaColor, sigmaSpace, borderType) (EF.hpp:317;
 * modules/ximgproc/src/joint_bilateral_filter.cpp = JBF.cpp): every pixel becomes the weighted mean of the source over a
 * disc around it, a tap's weight falling with its distance and with the difference between the JOINT image's pixels
 * there and at the centre -- the textbook refinement of a disparity map through the colour view, and the building block
 * of rollingGuidanceFilter.  One streaming launch per call.  In the chain it stands where the guided filter does:
 * matcher -> adf_validate_disparity_* / adf_filter_speckles_* -> adf_weighted_median_filter_* (which fills the holes: this
 * filter is NOT blind to (minDisparity-1)*16, it blends it in) -> this -> adf_reproject_*.
 *
 * This is the library's OWN definition.  It keeps JBF.cpp's `_8u` path (JBF.cpp:231-337) operation for operation and
 * widens the source depths.  The result is bit-exact against the direct NumPy statement tests/jbf_ref.py fed with
 * adf_jbf_tables_host, and identical from run to run.
 *
 * Inputs.  n_maps equally sized maps of W x H, `*_map_stride` bytes apart, rows `*_stride` bytes apart.
 *   - joint: 8-bit, joint_channels 1 or 3 (interleaved), the size of src.
 *   - src: ONE channel, depth ADF_8U, ADF_16S or ADF_32F (the reference demands src.depth() == joint.depth(); a 16-bit
 *     or float disparity map through an 8-bit view is the case this library exists for).
 *   - dst: one channel, depth dst_depth, any of the three, independent of src's (cv's dDepth; the reference's is
 *     src.type()).
 * Parameters, as JBF.cpp:361-371 clamps them: sigma_color <= 0 -> 1, sigma_space <= 0 -> 1;
 * r = d <= 0 ? cvRound(sigma_space * 1.5) : d / 2, then max(r, 1); cvRound rounds half to even (1.5 -> 2, 4.5 -> 4).
 * r above ADF_JBF_MAX_RADIUS = 31 is refused.
 * Tables, built on the host in double with libm's exp, one rounding per entry:
 *   - colour: C[a] = (float)exp((double)(a * a) * (-0.5 / (sigma_color * sigma_color))), a = 1 .. 255 * joint_channels;
 *   - space:  S[q] = (float)exp((double)q * (-0.5 / (sigma_space * sigma_space))), q = 1 .. r * r, indexed by the squared
 *     distance q = i*i + j*j (JBF.cpp:307's value for every tap at that distance);
 *   - C[0] = S[0] = 1.0f.
 *   adf_jbf_tables_host writes C (255 * joint_channels + 1 entries), S (r * r + 1 entries, r the returned radius) and r
 *   exactly as the calls use them; colour and space may both be NULL, which gives the radius alone (what sizes S).  Host
 *   only -- no device is touched.
 * Window.  The taps (i, j), -r <= i, j <= r, with i*i + j*j <= r*r, in row-major order: i (rows) outer, j inner.  This
 * order IS the definition.  A tap outside the image is taken, for joint and src alike (the reference's copyMakeBorder of
 * both), from the coordinate cv::borderInterpolate gives on each axis of length n:
 *   - ADF_BORDER_REPLICATE (1):   min(max(p, 0), n - 1);
 *   - ADF_BORDER_REFLECT (2):     m = p mod 2n (non-negative), then m < n ? m : 2n - 1 - m;
 *   - ADF_BORDER_REFLECT_101 (4, cv's BORDER_DEFAULT): n == 1 ? 0 : m = p mod (2n - 2), then m < n ? m : 2n - 2 - m.
 *   Reflection so repeats until the coordinate is inside, and an axis of length 1 gives 0: a 3 x 2 image takes r = 31.
 *   BORDER_CONSTANT (0), BORDER_WRAP (3) and anything else are NOT built.
 * Per pixel p, with x = (float)src, sum = 0.0f, wsum = 0.0f, for the taps q in order:
 *   L = the L1 difference of joint(p) and joint(q) over the channels (0 .. 255 * joint_channels);
 *   w = S[i*i + j*j] * C[L];  sum = sum + w * x(q);  wsum = wsum + w;
 * every product and sum rounded to float32, no FMA.  Then y = sum / wsum, the correctly rounded IEEE quotient.  The centre
 * tap has weight exactly 1, so wsum >= 1: there is no zero divide and no special case.  Denormal table entries and
 * products stay denormal (nothing is flushed).  Non-finite float sources propagate as the arithmetic gives; the payload
 * bits of a resulting NaN are not specified.
 * Output.  dst = y for ADF_32F; rint(y) (half to even, cv's saturate_cast) saturated to the depth for ADF_8U / ADF_16S
 * (a NaN gives the depth's minimum).
 * Deviations from the reference, all deliberate:
 *   - 8-bit joints only: the `_32f` path with its interpolated 4096-bin table is not built;
 *   - one-channel sources only (callers split them); CV_16S sources; any output depth;
 *   - an empty joint or joint == src (the reference falls back to cv::bilateralFilter) is refused;
 *   - the uniform-joint Gaussian shortcut exists only in the `_32f` path and is not taken;
 *   - no ignore value: run adf_weighted_median_filter_* first, as the sections above say.
 *   For an 8-bit source and the three border types this is the reference's `_8u` arithmetic itself.
 * Refused: sigmas that are not finite (as double or as float32), a radius above ADF_JBF_MAX_RADIUS, a border type that is
 * not built, an unknown depth or joint_channels, NULL joint / src / dst, n_maps, W or H below 1, bases or strides not
 * aligned to the depth (2 bytes for ADF_16S, 4 for ADF_32F), dst overlapping (by the byte ranges they span) joint or src
 * (all ADF_EBADARG); W*H at or above 2^31, strides smaller than a row, destination maps of a batch that overlap each
 * other (ADF_ESIZE).  All of this is checked before a device is touched.
 * Workspace: none.  The two tables are one immutable device table per (device, sigma_color, sigma_space, r,
 * joint_channels) in the process-wide store (adf_release_cached_memory drops them); after its first use a key is a
 * look-up, the call launches one kernel and allocates nothing, and is capturable into a hipGraph.
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_JBF_MAX_RADIUS 31
#define ADF_BORDER_REPLICATE 1   /* cv::BORDER_REPLICATE */
#define ADF_BORDER_REFLECT 2     /* cv::BORDER_REFLECT */
#define ADF_BORDER_REFLECT_101 4 /* cv::BORDER_REFLECT_101 = cv::BORDER_DEFAULT */
int adf_jbf_tables_host(int d, double sigma_color, double sigma_space, int joint_channels, float* colour, float* space, int* radius);
int adf_joint_bilateral_filter_device(int n_maps,
                                      const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                      const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                      void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                      int W, int H, int d, double sigma_color, double sigma_space, int border_type,
                                      void* stream);
int adf_joint_bilateral_filter_host(int n_maps,
                                    const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                    const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                    void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                    int W, int H, int d, double sigma_color, double sigma_space, int border_type);

/* ---------------- rolling guidance filter (cv::ximgproc::rollingGuidanceFilter) ----------------
 * rollingGuidanceFilter(src, dst, d, sigmaColor, sigmaSpace, numOfIter, borderType) (EF.hpp:350;
 * modules/ximgproc/src/rolling_guidance_filter.cpp = RGF.cpp:45-82): guidance = src; numOfIter times
 * jointBilateralFilter(guidance, src, guidance, ...); dst = guidance.  The scale-aware smoother of the family: structures
 * smaller than the spatial scale (matcher noise, speckle remnants) vanish in the first iteration, the later ones put the
 * large depth edges back where they were -- and it needs no colour view at all.  num_iter launches per call.  In the
 * chain it stands where the joint bilateral filter does, after the holes are filled (adf_weighted_median_filter_*).
 *
 * This is the library's OWN definition, bit-exact against the direct NumPy statement tests/rgf_ref.py fed with
 * adf_rgf_tables_host, and identical from run to run.
 *
 * Inputs.  n_maps equally sized maps of W x H, `*_map_stride` bytes apart, rows `*_stride` bytes apart.
 *   - src: ONE channel, depth ADF_8U, ADF_16S or ADF_32F.
 *   - dst: one channel, THE SOURCE'S depth (the reference's dst has src.type(); there is no dDepth here).  dst overlaps
 *     neither src nor, across a batch, another map's dst.
 * Parameters.  sigma_color <= 0 -> 1, sigma_space <= 0 -> 1 (RGF.cpp:56-59); the radius as the joint bilateral filter's:
 * r = d <= 0 ? cvRound(sigma_space * 1.5) : d / 2, then max(r, 1); r above ADF_JBF_MAX_RADIUS is refused.  border_type:
 * ADF_BORDER_REPLICATE, ADF_BORDER_REFLECT or ADF_BORDER_REFLECT_101 (cv's default), cv::borderInterpolate on each axis
 * exactly as the joint bilateral section states it.  num_iter: 0 copies src to dst (the reference's `while (numOfIter--)`
 * does the same); negative (the reference would loop until the counter wraps) and above ADF_RGF_MAX_ITERS = 16 (a
 * decision, not a measurement: the filter has converged long before) are refused.
 * Iteration.  J_0 = src.  For k = 0 .. num_iter - 1, J_{k+1} is the joint bilateral filter of src with joint J_k, STORED
 * IN THE SOURCE'S DEPTH: rint (half to even), saturated, for the integer depths (a NaN gives the depth's minimum); as it
 * is for ADF_32F.  dst = J_num_iter.  The border rule applies to src and to J_k alike.
 * Per pixel p.  The taps q = p + (i, j) with i*i + j*j <= r*r, rows outer, columns inner: this order IS the definition.
 * With x = (float)src, sum = 0.0f, wsum = 0.0f, per tap:
 *   w = S[i*i + j*j] * Wc(p, q);  sum = sum + w * x(q);  wsum = wsum + w;
 * every product and sum rounded to float32, no FMA; y = sum / wsum is the correctly rounded IEEE quotient.  S is the joint
 * bilateral filter's space table, unchanged (S[0] = 1).
 * Range weight Wc, integer depths.  L = |J_k(p) - J_k(q)| as an integer (0 .. 255 or 0 .. 65535); Wc = C[min(L, T - 1)].
 *   C[0] = 1.0f, C[L] = (float)exp((double)L * (double)L * (-0.5 / (sigma_color * sigma_color))), built on the host in
 *   double with libm's exp, one rounding per entry (the square is formed in double: L * L in int overflows from 46341
 *   on).  T is the number of entries up to and including the first that rounds to 0.0f, at most 256 or 65536 (16 at
 *   sigma_color 1, 362 at 25, 14422 at 1000, all 65536 from 4545 up).  C falls monotonically, so the clamp returns exactly
 *   what the full table would.  For ADF_8U this is the joint bilateral filter's C for one channel and the arithmetic is
 *   the reference's `_8u` path operation for operation: one iteration equals adf_joint_bilateral_filter_* with a
 *   one-channel 8-bit joint and dst_depth = ADF_8U, bit for bit.
 * Range weight Wc, ADF_32F.  The reference's `_32f` path (JBF.cpp:98-108) interpolates a 4096-bin table laid over the
 *   joint's min-max range, which it finds anew with minMaxLoc on every call, and switches to a square-window GaussianBlur
 *   when the joint is uniform.  Ours keeps the interpolation and puts the grid on sigma_color instead: no reduction, no
 *   data-dependent table, no second algorithm.
 *     G[i] = (float)exp(-0.5 * (i / 256.0) * (i / 256.0)), i = 0 .. 4097: a constant table, independent of every
 *            parameter, zero from i = 3692 on -- a difference beyond 16 sigma weighs exactly 0;
 *     scale = (float)(256.0 / sigma_color); a call whose scale is not finite is refused;
 *     L = fabsf(J(p) - J(q));  a = L * scale;  if (!(a < 4096.0f)) a = 4096.0f   (NaN and infinity go to the zero end);
 *     idx = (int)a;  f = a - (float)idx;  Wc = G[idx] + f * (G[idx + 1] - G[idx]), each operation rounded separately.
 *   The centre tap has L = 0 and weight exactly 1 for finite data, so wsum >= 1.  Non-finite sources propagate as this
 *   arithmetic gives; the payload bits of a NaN are not specified.
 * adf_rgf_tables_host writes the range table (`colour`: C, T entries, or G, 4098 entries) and S (`space`, r * r + 1
 * entries) exactly as the calls use them, and returns the radius, the range table's entry count and scale (1.0f for the
 * integer depths) through the pointers that are not NULL; colour == space == NULL gives the sizes alone.  Host only.
 * Deviations from the reference, all deliberate:
 *   - CV_16S sources;
 *   - the float grid as above, and no Gaussian shortcut for a uniform joint;
 *   - one-channel sources only (callers split them);
 *   - no in-place call (dst must not overlap src);
 *   - no ignore value: the matcher's invalid value is blended in, as with the joint bilateral filter.  The range weight
 *     on the map itself makes it a weak tap, not an absent one; hole filling still comes first
 *     (adf_weighted_median_filter_*).
 * Refused, all before a device is touched: what the joint bilateral section lists (sigmas that are not finite, the
 * radius, the border type, an unknown depth, NULL src / dst, n_maps, W or H below 1, alignment, dst overlapping src: all
 * ADF_EBADARG; W*H at or above 2^31, strides smaller than a row, overlapping destination maps: ADF_ESIZE), num_iter
 * outside 0 .. ADF_RGF_MAX_ITERS, a scale that is not finite, a workspace that overlaps src or dst (ADF_EBADARG), a
 * workspace that is too small (ADF_ESIZE).
 * Workspace.  The iterations write alternately into one dense plane of the source's depth per map and into dst, arranged
 * so that the last one writes dst; src is read by every iteration and never written.  Hence
 * adf_rolling_guidance_workspace_bytes = n_maps * W * H * the depth's size for num_iter >= 2, and 0 for num_iter <= 1 and
 * for arguments the calls refuse.  The rules are adf_dt_filter_*'s: NULL takes library scratch from the process-wide
 * cache; with a caller's workspace the call allocates nothing and is capturable into a hipGraph once the tables are
 * warm.  The device tables (the range table, then S) are one immutable table per (device, depth, sigma_color,
 * sigma_space, r) in the process-wide store next to the joint bilateral filter's, dropped by adf_release_cached_memory.
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_RGF_MAX_ITERS 16
size_t adf_rolling_guidance_workspace_bytes(int n_maps, int W, int H, int depth, int num_iter);
int adf_rgf_tables_host(int depth, int d, double sigma_color, double sigma_space, float* colour, float* space,
                        int* radius, int* colour_entries, float* scale);
int adf_rolling_guidance_filter_device(int n_maps,
                                       const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride,
                                       void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                       int depth, int W, int H, int d, double sigma_color, double sigma_space, int num_iter,
                                       int border_type, void* workspace, size_t workspace_bytes, void* stream);
int adf_rolling_guidance_filter_host(int n_maps,
                                     const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride,
                                     void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                     int depth, int W, int H, int d, double sigma_color, double sigma_space, int num_iter,
                                     int border_type);

/* ---------------- adaptive manifold filter (cv::ximgproc::amFilter / AdaptiveManifoldFilter) ----------------
 * amFilter(joint, src, dst, sigma_s, sigma_r, adjust_outliers) (EF.hpp:203-280;
 * modules/ximgproc/src/adaptive_manifold_filter_n.cpp = AMF.cpp): Gastal & Oliveira's adaptive manifolds, an approximation
 * of a high-dimensional bilateral filter of a map through a gray or BGR view with large kernels (sigma_s 16 .. 64, where
 * the joint bilateral filter stops at radius 31).  A complete binary tree of 2^height - 1 manifolds; every manifold
 * weighs the pixels by their distance to it, blurs the weighted map at 1/df of its size and hands its share back.
 *
 * This is the library's OWN definition.  The result is bit-exact against the direct NumPy statement tests/am_ref.py fed
 * with adf_am_plan_host, and identical from run to run.
 *
 * Images: n_maps maps of W x H; joint 8-bit with 1 or 3 interleaved channels; src ONE channel of depth ADF_8U, ADF_16S
 * or ADF_32F; dst one channel of depth dst_depth, independent of src's (the reference gives src's).  dst must not
 * overlap src or joint.
 * Plan (host, double arithmetic; AMF.cpp:70-75, 172-184).  df = max(1, 2^floor(log2(min(sigma_s / 4, 256 sigma_r))));
 *   height = tree_height > 0 ? tree_height : max(2, ceil((floor(log2 sigma_s) - 1) (1 - sigma_r))); the small size
 *   (sh, sw) = (cvRound(H (1 / df)), cvRound(W (1 / df))), ties to even.  The tree is always complete: nothing on the
 *   host depends on the data.  Float32 scalars, each rounded once: a(sigma) = (float)exp(-sqrt(2) / sigma) for
 *   sigma = sigma_s (a_root) and sigma_s / df (a_child); sr2 = (float)(sigma_r / sqrt(2)); arg_w = -0.5f / (sr2 * sr2);
 *   ss = (float)(sigma_s / df); ratio = (ss / sr2)^2 in float32; ln_a = (float)(-sqrt(2) / ss);
 *   arg_out = (float)(-0.5 / sigma_r^2); Jtab[v] = (float)(v / 255.0).  adf_am_plan_host returns all of them (jtab: 256
 *   floats, may be NULL).  Host only -- no device is touched.
 * Arithmetic.  Every + - * / sqrt is one IEEE float32 operation, rounded once, never contracted; quotient and root are
 *   correctly rounded; denormals are kept; x / 0 = 0 everywhere (cv::divide's rule).
 * am_exp(x), x <= 0, from float32 operations alone: t = x * (float)log2(e), n = floor(t + 0.5f), f = t - n, p the Horner
 *   form of degree 7 in f with c_k = (float)(ln2^k / k!) (multiply, then add), the result p * 2^n with 2^n built from
 *   bits; 0 where n < -126 (or x is a NaN); am_exp(0) == 1.  At most 1.6 ulp on [-1, 0], relative error 3.9e-6 at
 *   x = -86 (the argument's rounding).  adf_am_exp_host(x, y, n) evaluates it on the host.
 * down(P), full -> small: cv::resize INTER_LINEAR by the tap rule of the WLS filter's down-scaled path
 *   (fx = (float)((dx + 0.5) scale - 0.5), sx = floor(fx), fx -= sx; along a row a tap that would leave it has the
 *   weights (1, 0); along a column the rows are clamped and the weights stay; row blend S[sx] (1 - fx) + S[sx+1] fx
 *   first, then the column blend) with scale = df on both axes: for df >= 2 the 2 x 2 pixels at the centre of each cell.
 *   up(P), small -> full: the same rule with scale_x = sw / W, scale_y = sh / H in double.
 * sweep(P, ah, av), in place: every row left to right x[j] = x[j] + ah[j-1] (x[j-1] - x[j]), then right to left
 *   x[j] = x[j] + ah[j] (x[j+1] - x[j]); then every column down and up with av (AMF.cpp's RF pass, one iteration).
 *   h_filter(P, sigma) = sweep with the constant a(sigma).
 * Tree.  Root: eta_c = h_filter(J_c, sigma_s) at full size, J_c = Jtab[joint channel c], cluster = every pixel.  Nodes
 *   in pre-order, the minus child before the plus child; each adds to num and den in that order.  A node at level l:
 *   1. etaF = eta and eta = down(eta) at the root; etaF = up(eta) below it.
 *   2. d2 = sum over c, in order, of (etaF_c - J_c)^2; w = am_exp(d2 * arg_w); with adjust_outliers mind = d2 at l = 1,
 *      else min(mind, d2).
 *   3. psi = down(f * w), psi0 = down(w), f = (float)src.
 *   4. ah = am_exp(sqrt((sum over c of (eta_c[j] - eta_c[j+1])^2) * ratio + 1) * ln_a), av likewise between rows;
 *      sweep(psi, ah, av), sweep(psi0, ah, av).
 *   5. num = num + up(psi) * w, den = den + up(psi0) * w.
 *   6. If l < height: X_c = J_c - etaF_c.  One joint channel: o = X_0.  Three: m = 0.5 X_0 + (-0.5) X_1 + 0.5 X_2 in
 *      that order (the reference's start vector without its random generator), 0 outside the cluster;
 *      s_c = sum over the pixels of rint((m * X_c) * 2^30) as 64-bit integers (exact, so any order gives it), times
 *      2^-30 in double; vec = (float)(s / sqrt(s_0^2 + s_1^2 + s_2^2)) in double, 0 if the norm is 0;
 *      o = vec_0 X_0 + vec_1 X_1 + vec_2 X_2 in that order.  minus = cluster and o < 0, plus = cluster and o >= 0.  Per
 *      child: tm = 1 - w inside its cluster, 0 outside; tb = h_filter(down(tm), ss);
 *      eta_c = h_filter(down(tm * J_c), ss) / tb.
 *   g = num / den; with adjust_outliers alpha = am_exp(mind * arg_out), g = alpha * (g - f) + f.  dst = g for ADF_32F;
 *   rint(g) (half to even) saturated to the depth for ADF_8U / ADF_16S.
 * Deviations from the reference, all deliberate: cv::exp is replaced by am_exp; the joint is normalised through Jtab;
 *   useRNG is false (the reference seeds cv::RNG from the centre pixel; that generator is not part of this library, so
 *   setUseRNG(true) is refused as not built -- the reference's default is true); num_pca_iterations does not change the
 *   result (AMF.cpp:759-800 multiplies with the START vector in every iteration, so n iterations give n times one pass
 *   before normalisation): this definition takes one pass; one-channel sources only; a NULL joint (the reference then
 *   filters src by itself) is not built.
 * Refused (ADF_EBADARG, before a device is touched): sigma_s below 1 or not finite; sigma_r outside (0, 1] or not finite
 *   (the reference's own assert); tree_height 0, below -1 or above ADF_AM_MAX_TREE_HEIGHT, and an automatic height above
 *   it; sh or sw below 1; a NULL joint, src or dst; joint_channels other than 1 or 3; unknown depths; n_maps, W or H below
 *   1; and what the other edge-aware filters' shared check refuses, with the same status (alignment, overlap: ADF_EBADARG;
 *   W*H at or above 2^31, strides, overlapping destination maps, a workspace that is too small: ADF_ESIZE).
 * Workspace: adf_am_filter_workspace_bytes(n_maps, W, H, joint_channels, sigma_s, sigma_r, tree_height) bytes of 4-byte
 *   aligned device memory (0 for arguments the calls refuse): per map num, den, mind and the root manifold at full size,
 *   a byte of cluster bits per pixel, and 4 + 2 height (1 + channels) small planes.  NULL takes library scratch; a
 *   caller-supplied workspace makes the call capturable into a hipGraph (one chain of launches and at most one memset).
 * _device: device pointers on the current HIP device, asynchronous on `stream`.  _host: host pointers; copies, runs and
 * synchronises. */
#define ADF_AM_MAX_TREE_HEIGHT 8 /* 255 manifolds */
typedef struct adf_am_plan {
    int df, height, sh, sw, manifolds;
    float a_root, a_child, sr2, arg_w, ss, ratio, ln_a, arg_out;
} adf_am_plan;
int adf_am_plan_host(double sigma_s, double sigma_r, int tree_height, int W, int H, adf_am_plan* plan, float* jtab);
int adf_am_exp_host(const float* x, float* y, size_t n);
size_t adf_am_filter_workspace_bytes(int n_maps, int W, int H, int joint_channels, double sigma_s, double sigma_r, int tree_height);
int adf_am_filter_device(int n_maps,
                         const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                         const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                         void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                         int W, int H, double sigma_s, double sigma_r, int tree_height, int adjust_outliers,
                         void* workspace, size_t workspace_bytes, void* stream);
int adf_am_filter_host(int n_maps,
                       const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                       const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                       void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                       int W, int H, double sigma_s, double sigma_r, int tree_height, int adjust_outliers);

#ifdef __cplusplus
}
#endif
#endif
