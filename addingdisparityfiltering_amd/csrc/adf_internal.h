// adf_internal.h -- shared declarations between the HIP kernels and the C-ABI host code (whose own toolkit is adf_host.h).
// Not installed; the public boundary is include/adf_wls.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/adf_wls.h" /* the public enums (adf_depth) are the kernels' codes too */

#define ADF_LUT_LEVELS (3 * 256 * 256) /* FGS.cpp:150 */
#define ADF_EPS 1e-43f                 /* DF.cpp:47  */

namespace adf {

// Geometry of one filter call.  ROI planes are kept in two orientations:
//   N ("natural")    [rh][pw] : column index fastest -> lane-per-column (vertical) sweeps coalesce
//   T ("transposed") [rw][ph] : row index fastest    -> lane-per-row (horizontal) sweeps coalesce
// pw / ph are rw / rh rounded up to 64 floats so every sweep step is one aligned 256-byte row.
struct Geom {
    int W, H;           // full frame
    int rx, ry, rw, rh; // ROI (DF.cpp:228-233)
    int pw, ph;         // padded pitches (floats)
    size_t plane;       // floats per pair per ROI plane = max(rh*pw, rw*ph)
    size_t frame;       // floats per pair per full-frame plane = W*H
    // The confidence plane (library-owned; getConfidenceMap copies it out) has a layout of its own: frame pixel (i, j)
    // at cframe*pair + i*cpitch + cx0 + j, with cx0 chosen so that ROI column 0 is 16-byte aligned for ANY ROI x,
    // cpitch a multiple of 4 floats that leaves at least 3 zero floats behind frame column W-1 (the fused first row
    // pass reads whole float4s: what it over-reads is zero), zeros everywhere outside the ROI.
    int cpitch, cx0;
    size_t cframe;      // floats per pair of the confidence plane = cpitch*H
};

// Destination layout of a plane-writing kernel.
//   ORIENT_PAIR   (wave solver, two right-hand sides) ONE plane of 2*plane floats per image holding
//                 both, tiled [row pair][16-column strip][row parity][U0 x16 | U1 x16]: a strip row of the
//                 column pass is one 128-byte line and two consecutive rows of a strip are 256 contiguous
//                 bytes, while an image row is still 128-byte pieces at a fixed 256-byte stride for the row
//                 pass; the U1 pointer is unused
//   ORIENT_STRIP  (wave solver, Cvert) strip-major [pw/16][rh][16]
enum Orient { ORIENT_N = 0, ORIENT_T = 1, ORIENT_PAIR = 2, ORIENT_STRIP = 3 };
#define ADF_STRIP 16
// Rows per tile of the pair plane: [rh/TR][pw/16][TR rows][U0 x16 | U1 x16] -- a strip visit of the column pass is
// TR*128 contiguous bytes, a row of the row pass is 128-byte pieces at a TR*128-byte stride (power of two).
constexpr int TILE_ROWS = 2;

// What the last sweep of a solve writes (fused epilogues).
enum Epilogue {
    EPI_PLANES = 0,   // float planes in the opposite orientation (feeds the next pass)
    EPI_WLS_CONF = 1, // int16 = sat(u0 * (1/(u1+EPS)))   DF.cpp:295-296
    EPI_I16 = 2,      // int16 = sat(u0)                  FGS.cpp:216 (no-confidence path, DF.cpp:257-258)
    EPI_F32 = 3,      // float natural layout             FGS.cpp:218
    EPI_U8 = 4,       // uint8 = sat(u0)                  FGS.cpp:216
    EPI_WLS_CONF_F32 = 5 // float = the value EPI_WLS_CONF rounds, single channel (adf_wls_filter_f32_*)
};
constexpr int N_EPILOGUES = EPI_WLS_CONF_F32 + 1;

// Both views of a pair in one launch: index 0 = left, 1 = right (mirrored ROI x, DF.cpp:202-203).
struct DiscArgs {
    const int16_t* disp[2]; ptrdiff_t stride[2], pair_stride[2]; // bytes
    int rx[2]; int ry, rw, rh;
    int radius; float roll_off;
    float* dst[2]; int W; size_t frame; // full-frame float planes, W pitch
    int only_view;                      // -1 = both views, else the one view to compute
};

// Left view: discontinuity map + LRC + x255 in one sweep (no cL round trip through HBM); needs the
// right view's discontinuity map cR complete.  Optionally also writes the two right-hand sides.
struct ConfLeftArgs {
    const int16_t* dL; ptrdiff_t sL, psL; // bytes
    const int16_t* dR; ptrdiff_t sR, psR;
    const float* cR;                      // full-frame, W pitch
    float* conf;                          // confidence plane (x255; Geom::cpitch layout); only ROI pixels are written
    float* U0; float* U1;                 // ORIENT_PAIR plane at U0 (may be null: first pass reads conf/dL itself); U1 unused
    Geom g; int rrx; int thresh;
    int radius; float roll_off;
};

// Both views' discontinuity maps + LRC + x255 in ONE sweep over row bands (conf_band_kernel): the right view's
// map of a row lives in LDS only, so nothing but dL, dR (read) and the confidence map (written) touches HBM.
struct ConfBandArgs {
    const int16_t* dL; ptrdiff_t sL, psL; // bytes
    const int16_t* dR; ptrdiff_t sR, psR;
    float* conf;                          // confidence plane (x255; Geom::cpitch layout); only ROI pixels are written
    Geom g; int rrx; int thresh;
    int radius; float roll_off;
    int rows_per_band;
};

// Non-ROI pixels: filtered map = fill (DF.cpp:284), confidence = 0 (DF.cpp:187-190); either may be null.  The map is
// CV_16SC1, or CV_32FC1 holding float(fill) when out_f32 is set (adf_wls_filter_f32_*).
struct OutsideArgs {
    void* out; ptrdiff_t stride, pair_stride; int16_t fill; int out_f32;
    float* conf;
    Geom g;
};

struct LrcArgs {
    const int16_t* dL; ptrdiff_t sL, psL; // bytes
    const int16_t* dR; ptrdiff_t sR, psR;
    const float* cL; const float* cR; // full-frame discontinuity maps
    float* conf;                      // confidence plane (x255; Geom::cpitch layout), zero outside ROI
    void* out; ptrdiff_t sO, psO; int16_t fill; int out_f32; // filtered map (int16, or float when out_f32): `fill` outside the ROI (DF.cpp:284); may be null
    float* U0; float* U1;             // ROI planes: conf*disp, conf
    Geom g; int rrx;                  // right ROI x (DF.cpp:202)
    int thresh; int orient;           // orientation of U0/U1
    // float maps (adf_wls_filter_typed_*): dL is the caller's CV_32FC1 left map -- the kernel forms v and q of its own
    // pixel itself, U0 = conf * v -- while dR stays the int16 plane q of the right map (a gather)
    int dl_f32 = 0;
};

// Source plane -> float right-hand side on the ROI: the no-confidence path's float(disp)
// (DF.cpp:250,257) and FastGlobalSmootherFilter::filter's split + convertTo (FGS.cpp:191-205).
struct PlainPrologueArgs {
    const void* src; ptrdiff_t stride, pair_stride; // bytes
    int depth, cn, c;                               // adf_depth code, channel count, channel index
    float* U0; Geom g; int orient;
    // optional confidence weighting (down-scaled path, DF.cpp:286-290 on the resized maps):
    // U0 = conf*float(src), U1 = conf, conf read from a confidence plane (Geom::cpitch layout)
    const float* conf; float* U1;
    // or a second source channel as the second right-hand side (generic FGS on the wave solver: channel
    // pairs share one factorisation): U1 = float(src channel c2) when pair2 is set (conf must be null)
    int pair2, c2;
};

// A float disparity map of a WLS filter call as a right-hand side source (adf_wls_filter_typed_*): ADF_32F whose
// elements go through wls_input_value -- the generic smoother's ADF_32F sources are taken as they are.
constexpr int DEPTH_WLS_F32 = 0x100 | ADF_32F;

// The float disparity maps of a chunk of pairs (adf_wls_filter_typed_*) -> what the confidence kernels read: per map m
// (0 = left, 1 = right; src[1] may be null) the plane q[m] of q = (int16_t)rintf(v), v = wls_input_value(element), and,
// where v is set, the left map's v as a float plane (the down-scaled path resizes it).  Planes are `pitch` elements
// wide (a multiple of 8: 16-byte rows; columns past W hold 0), images `frame` elements apart.
struct QuantArgs {
    const void* src[2]; ptrdiff_t stride[2], pair_stride[2];   // bytes
    int16_t* q[2]; float* v;
    int W, H, pitch; size_t frame;
    int n_pairs;
};

// cv::resize(INTER_LINEAR) of CV_16SC1 (is16, optional saturating post-scale) or CV_32FC1 images (post-scale: one
// float multiply, no saturation).
struct ResizeArgs {
    const void* src; ptrdiff_t sstride, spair; int sw, sh; // bytes
    void* dst; ptrdiff_t dstride, dpair; int dw, dh;
    double scale_x, scale_y;                               // sw/dw, sh/dh
    float post_scale; int is16;
    int zero_outside = 0, vx0 = 0, vy0 = 0, vx1 = 0, vy1 = 0; // source elements outside [vx0,vx1) x [vy0,vy1) read as zero
};

struct WeightArgs {
    const uint8_t* guide; ptrdiff_t stride, pair_stride; int ch; // bytes
    const float* lut;
    float* chor; float* cvert; int chor_orient, cvert_orient;
    Geom g;
    // exact solver (chor_orient == ORIENT_T): a free plane the streaming kernel can write Chor row-major
    // into before it is transposed; null = the generic tile kernel writes the transposed plane itself
    float* scratch;
};

// One solve pass (forward elimination + back substitution along every scanline).
// Input planes have the scanline index fastest: element (step t, scanline s) at t*pitch_in + s.
struct PassArgs {
    const float* C; const float* U0; const float* U1;
    float* D; float* F0; float* F1; // forward intermediates, same layout as the inputs
    float* O0; float* O1;           // EPI_PLANES: [nscan][pitch_out], step index fastest
    void* out; ptrdiff_t out_stride, out_pair_stride; // other epilogues: natural image, bytes
    int out_x0, out_y0, out_cn, out_c;                // ROI origin, channel count / index of `out`
    int nscan, len, pitch_in, pitch_out;
    size_t plane;
    float lambda;
};

// Inputs of a fused first horizontal pass of the wave solver (WavePassArgs::fuse; all zero = not fused).
struct FusedInputs {
    // fused prologue of the first horizontal pass (DF.cpp:288-290): when conf_in is set the right-hand
    // sides are read as U1 = conf, U0 = conf * float(dL) from the confidence plane and the disparity map
    const float* conf_in; size_t conf_frame; int conf_pitch, conf_x0, conf_y0;
    int dl_f32;   // dl_in is a CV_32FC1 map (adf_wls_filter_typed_*): U0 = conf * wls_input_value(dL), one float multiply
    const void* dl_in; ptrdiff_t dl_stride, dl_pair_stride; int dl_x0, dl_y0;
    // ... or, down-scaled path (DF.cpp:268-277 then 288-290), from the LOW-resolution maps: when lo_conf is set the
    // pass interpolates the confidence map and the left disparity map itself (cv::resize INTER_LINEAR, tap for tap as
    // resize_kernels.hip / the oracle's resize_linear_*; disparity saturated, multiplied by lo_post_scale and
    // saturated again, DF.cpp:273), so neither view-sized plane is ever written.  ROI column j / row i of the pass is
    // view pixel (hi_x0 + j, hi_y0 + i).  Confidence elements outside [lo_vx0, lo_vx1) x [lo_vy0, lo_vy1) read as
    // zero when lo_zero_outside is set (the band kernel writes the maps' ROI only, DF.cpp:187-190).
    const float* lo_conf; ptrdiff_t lo_conf_stride, lo_conf_pair;      // floats
    const int16_t* lo_dl; ptrdiff_t lo_dl_stride, lo_dl_pair;          // bytes
    int lo_w, lo_h, hi_x0, hi_y0;
    double lo_scale_x, lo_scale_y; float lo_post_scale;
    int lo_zero_outside, lo_vx0, lo_vy0, lo_vx1, lo_vy1;
    int lo_half;      // 0: never the half-width form of the low-resolution prologue (ADF_LO_HALF=0: A/B and test knob)
    float* lo_taps;   // scratch, 4*ceil(len/4) floats, 16-byte aligned: the launcher fills it with the columns' taps (s0 + fx)
};

// Where a row pass of the wave solver takes its edge weights from when it forms them itself instead of reading the Chor
// plane (WavePassArgs::gw; guide null = the plane): the guide row of the pass's own row, Chor[y][x] = lut[|g(y,x) -
// g(y,x+1)|^2] (FGS.cpp:607-614).  ROI column j / row i of the pass is guide pixel (x0 + j, y0 + i).
struct GuideWeights {
    const uint8_t* guide; ptrdiff_t stride, pair_stride;   // bytes
    int ch, x0, y0;                                        // channels (1 or 3), ROI origin
    const float* lut;                                      // the full weight table (ADF_LUT_LEVELS entries)
};

// One pass of the on-chip partitioned solver (fgs_wave.hip).  Planes are row-major [rh][pitch] and
// are solved IN PLACE; horizontal: nscan = rows, len = row length; vertical: nscan = columns,
// len = column length.  The last vertical pass may fuse an epilogue and write `out` instead.
struct WavePassArgs {
    const float* C; float* U0; float* U1;
    FusedInputs fuse;
    void* out; ptrdiff_t out_stride, out_pair_stride;
    int out_x0, out_y0, out_cn, out_c;
    int nscan, len, pitch;
    size_t plane;
    float lambda;
    GuideWeights gw;   // row passes only
    // A row -> column hand-off's register image (fgs_wave_common.h): where a row pass of a call with two right-hand
    // sides stores its solutions INSTEAD of the pair plane and the column pass that follows loads them from; null = the
    // pair plane.  image_m is the column bucket's chunk length, image_plane the image's floats per pair.
    float* image; size_t image_plane; int image_m;
};
// the kernels' argument layout (the guide of the row passes' weights and the hand-off image are appended: no other member moved)
static_assert(sizeof(WavePassArgs) == 352 && offsetof(WavePassArgs, out) == 208 && offsetof(WavePassArgs, nscan) == 248 &&
              offsetof(WavePassArgs, plane) == 264 && offsetof(WavePassArgs, lambda) == 272 && offsetof(WavePassArgs, gw) == 280 &&
              offsetof(WavePassArgs, image) == 328 && sizeof(GuideWeights) == 48, "WavePassArgs layout");

// Launchers (defined in the .hip files).  All are asynchronous on `st`.
hipError_t launch_discontinuity(const DiscArgs& a, int n_pairs, hipStream_t st);
hipError_t launch_lrc_prologue(const LrcArgs& a, int n_pairs, hipStream_t st);
hipError_t launch_conf_left(const ConfLeftArgs& a, int n_pairs, hipStream_t st); // radius <= 8 only
hipError_t launch_outside(const OutsideArgs& a, int n_pairs, hipStream_t st);
bool conf_band_fits(const Geom& g, int radius);                                 // geometry / radius the band kernel covers
hipError_t launch_conf_band(const ConfBandArgs& a, int n_pairs, hipStream_t st);
// weights + confidence map + outside fill in one launch, for calls small enough to be latency-bound (conf_kernels.hip)
bool prep_small_guide_fits(const Geom& g, ptrdiff_t guide_stride, int channels);
bool prep_small_fits(const Geom& g, int radius, int channels, int n_pairs);
hipError_t launch_prep_small(const ConfBandArgs& c, const WeightArgs& w, const OutsideArgs& o, int n_pairs, hipStream_t st);
int conf_left_max_radius();
hipError_t launch_plain_prologue(const PlainPrologueArgs& a, int n_pairs, hipStream_t st);
hipError_t launch_quantise_maps(const QuantArgs& a, hipStream_t st);
hipError_t launch_weights(const WeightArgs& a, int n_pairs, hipStream_t st);   // a.chor null: Cvert only (streaming kernel)
bool weights_stream_fits(const WeightArgs& a);                                  // ... which takes these arguments?
hipError_t launch_resize_linear(const ResizeArgs& a, int n_pairs, hipStream_t st);
hipError_t launch_exact_pass(const PassArgs& a, int n_rhs, int epilogue, int n_pairs, hipStream_t st);
hipError_t launch_wave_hpass(const WavePassArgs& a, int n_rhs, int n_pairs, hipStream_t st);
hipError_t launch_wave_vpass(const WavePassArgs& a, int n_rhs, int epilogue, int n_pairs, hipStream_t st);
int wave_max_row_len();
bool wave_hpass_can_fuse(const WavePassArgs& a);
bool wave_hpass_can_fuse_lo(const WavePassArgs& a);   // the low-resolution form: scale / span limits of the LDS staging
bool wave_hpass_lo_half(const WavePassArgs& a);      // ... in its half-width form (fgs_wave_h.hip, FUSE_LO_HALF)?
bool wave_hpass_guide_fits(const WavePassArgs& a);   // can the row pass form its weights from a.gw (a.len, a.gw, a.fuse)?
int wave_max_col_len();
// A hand-off's register image (WavePassArgs::image): does the row pass of rows of `row_len` elements have the
// store form (one-wave rows); does the fused first pass on the inputs `f` have it (the view-resolution prologue on an
// int16 map); the chunk length of the column bucket of `col_len` rows, 0 where the column pass lacks the load form
// (half strips); floats per pair of the image.
bool wave_hpass_image_fits(int row_len);
bool wave_hpass_first_image(const FusedInputs& f);
int wave_vpass_image_m(int col_len);
inline size_t wave_image_floats(int pitch, int m) { return (size_t)pitch * (size_t)(64 * m) * 2; }
// largest depth-discontinuity radius the tile kernel supports (LDS bound)
int max_disc_radius();

// The block of the tile kernels of conf_kernels.hip and rhs_prologue.hip (`using namespace tile`): NT threads, TX x TY pixels.
namespace tile {
constexpr int TX = 64; // tile width  (one wavefront wide: 128-byte int16 rows, 256-byte float rows)
constexpr int TY = 32; // tile height
constexpr int NT = 256;
}

// Device-side helpers shared by kernels.
#if defined(__HIPCC__)
// float index of U0(i, j) inside an ORIENT_PAIR plane of pitch pw (U1 is ADF_STRIP floats further)
__device__ __forceinline__ size_t pair_index(int i, int j, int pw)
{
    constexpr int TR = TILE_ROWS;
    return (size_t)(i / TR) * (size_t)(2 * TR * pw) + (size_t)((j >> 4) * (32 * TR) + (i % TR) * 32 + (j & 15));
}
// float index of C(i, j) inside an ORIENT_STRIP plane of rh rows
__device__ __forceinline__ size_t strip_index(int i, int j, int rh)
{
    return ((size_t)(j >> 4) * (size_t)rh + (size_t)i) * ADF_STRIP + (size_t)(j & 15);
}
// The two right-hand sides of image pz.  ORIENT_PAIR: the one plane of 2*plane floats per image, U1 ADF_STRIP floats
// behind U0 (the U1 argument is unused); ORIENT_N / ORIENT_T: a plane each, U1 null where there is one right-hand side.
struct RhsPlanes { float* U0; float* U1; };
__device__ __forceinline__ RhsPlanes rhs_planes(float* U0, float* U1, int orient, size_t pz, size_t plane)
{
    const bool pair = orient == ORIENT_PAIR;
    float* u0 = U0 + pz * (pair ? 2 : 1) * plane;
    return RhsPlanes{u0, pair ? u0 + ADF_STRIP : U1 ? U1 + pz * plane : nullptr};
}
// float index of ROI pixel (i, j) inside a right-hand side plane (ORIENT_N, ORIENT_T or ORIENT_PAIR)
__device__ __forceinline__ size_t rhs_index(int orient, int i, int j, const Geom& g)
{
    return orient == ORIENT_PAIR ? pair_index(i, j, g.pw) : orient == ORIENT_T ? (size_t)j * g.ph + i : (size_t)i * g.pw + j;
}
// ORIENT_T from a kernel whose threads walk along image rows: thread (tx, ty) stages its pixels (tx, ty + 4*kk) in LDS
// (odd pitch); after the last one the whole block calls store() with the ROI coordinates (j0, i0) of the tile's first
// pixel -- negative where the tile starts outside the ROI -- and writes them out with the row index fastest.
struct RhsTile {
    float t0[tile::TX * (tile::TY + 1)], t1[tile::TX * (tile::TY + 1)];
    __device__ __forceinline__ void stage(int tx, int y, float v0, float v1) { t0[tx * (tile::TY + 1) + y] = v0; t1[tx * (tile::TY + 1) + y] = v1; }
    __device__ __forceinline__ void store(float* U0, float* U1, const Geom& g, int j0, int i0) const
    {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < tile::TX / 8; m++) {
            const int cidx = threadIdx.x / tile::TY + 8 * m, ridx = threadIdx.x % tile::TY, j = j0 + cidx, i = i0 + ridx;
            if ((unsigned)j < (unsigned)g.rw && (unsigned)i < (unsigned)g.rh) {   // (a negative j or i is outside too)
                const size_t o = rhs_index(ORIENT_T, i, j, g);
                U0[o] = t0[cidx * (tile::TY + 1) + ridx];
                if (U1) U1[o] = t1[cidx * (tile::TY + 1) + ridx];
            }
        }
    }
};
// One pixel of a filtered map outside the ROI: `fill` as int16, or as the float of the same value (uniform branch).
__device__ __forceinline__ void store_fill(void* map, ptrdiff_t row_offset_bytes, int j, int16_t fill, int f32)
{
    char* row = reinterpret_cast<char*>(map) + row_offset_bytes;
    if (f32) reinterpret_cast<float*>(row)[j] = (float)fill;
    else reinterpret_cast<int16_t*>(row)[j] = fill;
}
// The float epilogues' form of a value the int16 epilogues saturate to -32768 for being NaN, infinite or outside the
// int range (sat16 below): -32768.0f, so that sat16(float map) == int16 map and the float map holds no NaN or inf.
__device__ __forceinline__ float wls_f32_value(float x) { return !(__builtin_fabsf(x) < 2147483648.0f) ? -32768.0f : x; }
// A float disparity map's element as the solve takes it (include/adf_wls.h, float maps): clamped to the int16 range,
// -32768 where it is NaN or infinite; always finite.  And as the confidence arithmetic takes it: rounded half to even.
__device__ __forceinline__ float wls_input_value(float d)
{
    return __builtin_fabsf(d) < __builtin_inff() ? fminf(fmaxf(d, -32768.0f), 32767.0f) : -32768.0f;
}
__device__ __forceinline__ int16_t wls_input_q(float v) { return (int16_t)(int)rintf(v); }
// saturate_cast<short>(float): cvRound (round-half-even; NaN / out-of-int-range -> INT_MIN) + clamp.
__device__ __forceinline__ int16_t sat16(float v)
{
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return (int16_t)-32768;
    float r = rintf(v);
    r = fminf(fmaxf(r, -32768.0f), 32767.0f);
    return (int16_t)(int)r;
}
__device__ __forceinline__ uint8_t sat8(float v)
{
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return (uint8_t)0;
    float r = rintf(v);
    r = fminf(fmaxf(r, 0.0f), 255.0f);
    return (uint8_t)(int)r;
}
// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}
#endif

} // namespace adf
