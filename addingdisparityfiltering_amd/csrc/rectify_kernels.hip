// rectify_kernels.hip -- cv::initUndistortRectifyMap(K, dist, R, P, size, CV_32FC1, map1, map2) and
// cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, borderValue) (calib3d / imgproc, outside the reference
// tree: parity UNPINNED) on the device, and the two fused into one launch (adf_rectify_views_*: the maps never exist in
// memory).  The definition is the library's own (include/adf_wls.h, "rectification"); the device result is bit-exact
// against the direct NumPy statement tests/rectify_ref.py.
//
// Coordinates of destination pixel (u, v), every operator ONE binary64 operation in this order (the library is built with
// -ffp-contract=off: no fused multiply-add), ir = inverse(P[:, :3] * R) from adf_rectify_params_init:
//
//     X = (ir0*u + ir1*v) + ir2      Y = (ir3*u + ir4*v) + ir5      D = (ir6*u + ir7*v) + ir8
//     w = 1.0 / D        x = X*w        y = Y*w
//     x2 = x*x    y2 = y*y    r2 = x2 + y2    xy2 = (2.0*x)*y
//     kr = (1.0 + ((k3*r2 + k2)*r2 + k1)*r2) / (1.0 + ((k6*r2 + k5)*r2 + k4)*r2)
//     xd = (x*kr + p1*xy2) + p2*(r2 + 2.0*x2)
//     yd = (y*kr + p1*(r2 + 2.0*y2)) + p2*xy2
//     mapx = (float)(fx*xd + cx)     mapy = (float)(fy*yd + cy)
//
// Sampling, float and integer, 5 fractional bits (cv's INTER_TAB_SIZE = 32):
//
//     tx = mapx*32.0f   ty = mapy*32.0f
//     ok = -1048576.0f <= tx <= 1048575.0f and the same for ty (false for NaN); not ok: every channel = border_value[c]
//     sx = (int)rintf(tx)   ix = sx >> 5   ax = sx & 31     (same for y)
//     tap(i, j) = 0 <= i < srcW && 0 <= j < srcH ? src[j][i][c] : border_value[c]
//     out = (tap(ix,iy)*(32-ax)*(32-ay) + tap(ix+1,iy)*ax*(32-ay) + tap(ix,iy+1)*(32-ax)*ay + tap(ix+1,iy+1)*ax*ay + 512) >> 10
//
// Kernels
//   rectify_map_kernel   a pure stream: lanes along x, PX consecutive pixels per thread, one 16-byte store per plane when
//                        bases and strides allow, element by element otherwise (same bits).
//   sample_kernel<CH, FUSED>   THE sampling body for remap (FUSED = false: the coordinates are loaded, 16 bytes per plane
//                        when the maps allow) and rectifyViews (FUSED = true: the coordinates are computed).  The direct
//                        form: lanes along x, PX consecutive destination pixels per thread; a thread decides `ok` and the
//                        range of each tap, and only then forms the address of a tap and loads it -- a tap outside the source
//                        is never loaded.  Neighbouring lanes' taps share cache lines; the vector cache and L2 absorb
//                        the overlap.  A BGR row's two taps are one 12-byte load (sample_px).  The coordinates of a pixel
//                        serve up to IMAGES images of the batch (grid y walks groups of IMAGES images), so a batch pays
//                        for the binary64 arithmetic, or the map loads, once per IMAGES views.  A thread's PX pixels leave
//                        as one 4-byte (gray) or 12-byte (BGR) store when the destination's base and strides are
//                        multiples of 4: a wave writes 256 / 768 contiguous bytes per row piece.  The row tail and
//                        unaligned destinations go byte by byte through the same arithmetic.
//                        A staged form (a workgroup loads its tile's source box into LDS and samples from there) was
//                        built and measured: slower on a single 4K view, so it is not here (EXPERIMENTS.md).
#include "adf_host.h"

#include <cmath>

using namespace adf;

namespace {

constexpr int NT = 256;
constexpr int PX = 4;                  // destination pixels per thread
constexpr int IMAGES = 4;              // images of a batch that share one evaluation of the coordinates
constexpr int MAX_SRC_DIM = 32767;     // ix + 1 and iy + 1 stay inside the 16 bits sx >> 5 leaves

// THE coordinate arithmetic (include/adf_wls.h); ry = {ir1*v, ir4*v, ir7*v} of the pixel's row
__device__ __forceinline__ void map_px(const adf_rectify_params& p, const double* ry, int u, float* mx, float* my)
{
    const double ud = (double)u;
    const double X = (p.ir[0] * ud + ry[0]) + p.ir[2];
    const double Y = (p.ir[3] * ud + ry[1]) + p.ir[5];
    const double D = (p.ir[6] * ud + ry[2]) + p.ir[8];
    const double w = 1.0 / D;
    const double x = X * w, y = Y * w;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
    const double k1 = p.dist[0], k2 = p.dist[1], p1 = p.dist[2], p2 = p.dist[3], k3 = p.dist[4], k4 = p.dist[5], k5 = p.dist[6], k6 = p.dist[7];
    const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    *mx = (float)(p.fx * xd + p.cx);
    *my = (float)(p.fy * yd + p.cy);
}

__device__ __forceinline__ void row_terms(const adf_rectify_params& p, int v, double* ry)
{
    const double vd = (double)v;
    ry[0] = p.ir[1] * vd; ry[1] = p.ir[4] * vd; ry[2] = p.ir[7] * vd;
}

// ---------------------------------------------------------------------------------------------------------
// the maps
// ---------------------------------------------------------------------------------------------------------
struct MapArgs {
    char* mapx; ptrdiff_t xstride;     // bytes
    char* mapy; ptrdiff_t ystride;
    int W, H;
    int groups;        // groups of PX pixels per row (the last one may be short)
    int total;         // groups * H
    int vec;           // bases and strides allow 16-byte stores
    adf_rectify_params p;
};

__global__ void __launch_bounds__(NT) rectify_map_kernel(MapArgs a)
{
    const unsigned uidx = blockIdx.x * NT + threadIdx.x;             // (the last workgroup may reach past 2^31)
    if (uidx >= (unsigned)a.total) return;
    const int idx = (int)uidx;
    const int y = (int)((unsigned)idx / (unsigned)a.groups), x0 = (idx - y * a.groups) * PX;
    const int n = min(PX, a.W - x0);
    double ry[3];
    row_terms(a.p, y, ry);
    float mx[PX], my[PX];
#pragma unroll
    for (int i = 0; i < PX; i++) map_px(a.p, ry, x0 + i, &mx[i], &my[i]);
    float* ox = reinterpret_cast<float*>(a.mapx + (ptrdiff_t)y * a.xstride) + x0;
    float* oy = reinterpret_cast<float*>(a.mapy + (ptrdiff_t)y * a.ystride) + x0;
    if (a.vec && n == PX) {
        *reinterpret_cast<float4*>(ox) = make_float4(mx[0], mx[1], mx[2], mx[3]);
        *reinterpret_cast<float4*>(oy) = make_float4(my[0], my[1], my[2], my[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < PX; i++) {
        if (i >= n) break;
        ox[i] = mx[i]; oy[i] = my[i];
    }
}

// ---------------------------------------------------------------------------------------------------------
// sampling
// ---------------------------------------------------------------------------------------------------------
struct Tap { int ix, iy, ax, ay; bool ok; };

__device__ __forceinline__ Tap tap_of(float mx, float my)
{
    const float tx = mx * 32.0f, ty = my * 32.0f;
    Tap t;
    t.ok = tx >= -1048576.0f && tx <= 1048575.0f && ty >= -1048576.0f && ty <= 1048575.0f;   // (false for NaN)
    const int sx = t.ok ? (int)rintf(tx) : 0, sy = t.ok ? (int)rintf(ty) : 0;                  // half to even
    t.ix = sx >> 5; t.ax = sx & 31;
    t.iy = sy >> 5; t.ay = sy & 31;
    return t;
}

typedef uint32_t Words3 __attribute__((ext_vector_type(3), aligned(4)));   // 12 bytes behind a 4-byte aligned address: one load

// One destination pixel of one image.  Every address is formed after `ok` and the tap's range test have been decided.
// The two taps of a row are CH * 2 consecutive bytes.  BGR: they come with ONE load of the 12 bytes from the 4-byte
// boundary at or below the first -- whatever the image's base and stride -- when those 12 bytes all lie inside the
// row's srcW * 3 bytes; at the ends of a row, and for a pair with one tap outside, the bytes are loaded one by one.
// Gray loads its two bytes one by one everywhere (one 8-byte load per pair measured slower on a single view: EXPERIMENTS.md).
template <int CH>
__device__ __forceinline__ void sample_px(const uint8_t* img, ptrdiff_t sstride, int srcW, int srcH, const Tap& t,
                                          const uint32_t* border, uint32_t* out)
{
    if (!t.ok) {
#pragma unroll
        for (int c = 0; c < CH; c++) out[c] = border[c];
        return;
    }
    const bool x0 = (unsigned)t.ix < (unsigned)srcW, x1 = (unsigned)(t.ix + 1) < (unsigned)srcW;
    uint32_t p[2][2][CH];                                            // [row][column][channel]
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int c = 0; c < CH; c++) p[j][0][c] = p[j][1][c] = border[c];
        const int yy = t.iy + j;
        if ((unsigned)yy < (unsigned)srcH && (x0 || x1)) {
            const uint8_t* row = img + (ptrdiff_t)yy * sstride;
            const uintptr_t first = (uintptr_t)row, end = first + (uintptr_t)srcW * CH;
            const uintptr_t at = first + (uintptr_t)(x0 ? t.ix : 0) * CH, al = at & ~(uintptr_t)3;
            if (CH == 3 && x0 && x1 && al >= first && al + 12 <= end) {
                const int sh = (int)(at & 3) * 8;
                const Words3 w = *reinterpret_cast<const Words3*>(row + (al - first));
                const unsigned long long lo = (unsigned long long)w.x | ((unsigned long long)w.y << 32), hi = w.z;
                const unsigned long long b = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;   // the bytes from `at` on
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    p[j][0][c] = (uint32_t)(b >> (8 * c)) & 0xffu;
                    p[j][1][c] = (uint32_t)(b >> (8 * (CH + c))) & 0xffu;
                }
            } else {
                if (x0) {
                    const uint8_t* q = row + (ptrdiff_t)t.ix * CH;
#pragma unroll
                    for (int c = 0; c < CH; c++) p[j][0][c] = q[c];
                }
                if (x1) {
                    const uint8_t* q = row + (ptrdiff_t)(t.ix + 1) * CH;
#pragma unroll
                    for (int c = 0; c < CH; c++) p[j][1][c] = q[c];
                }
            }
        }
    }
    const uint32_t ax = (uint32_t)t.ax, ay = (uint32_t)t.ay, bx = 32u - ax, by = 32u - ay;
    const uint32_t w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
#pragma unroll
    for (int c = 0; c < CH; c++)
        out[c] = (p[0][0][c] * w00 + p[0][1][c] * w10 + p[1][0][c] * w01 + p[1][1][c] * w11 + 512u) >> 10;
}

struct SampleArgs {
    const uint8_t* src; ptrdiff_t sstride, simage;   // bytes
    int srcW, srcH;
    const char* mapx; ptrdiff_t xstride;             // remap only
    const char* mapy; ptrdiff_t ystride;
    uint8_t* dst; ptrdiff_t dstride, dimage;
    int W, H;
    int n;             // images of this launch
    int groups;        // groups of PX destination pixels per row (the last one may be short)
    int total;         // groups * H
    int vec_map;       // map bases and strides allow 16-byte loads
    int vec_dst;       // destination bases and strides allow whole 4- / 12-byte stores
    uint32_t border[3];
    adf_rectify_params p;                            // rectifyViews only
};

template <int CH, bool FUSED> __global__ void __launch_bounds__(NT) sample_kernel(SampleArgs a)
{
    const unsigned uidx = blockIdx.x * NT + threadIdx.x;             // (the last workgroup may reach past 2^31)
    if (uidx >= (unsigned)a.total) return;
    const int idx = (int)uidx;
    const int y = (int)((unsigned)idx / (unsigned)a.groups), x0 = (idx - y * a.groups) * PX;
    const int n = min(PX, a.W - x0);

    Tap t[PX];
    if (FUSED) {
        double ry[3];
        row_terms(a.p, y, ry);
#pragma unroll
        for (int i = 0; i < PX; i++) {
            float mx, my;
            map_px(a.p, ry, x0 + i, &mx, &my);
            t[i] = tap_of(mx, my);
        }
    } else {
        const float* rx = reinterpret_cast<const float*>(a.mapx + (ptrdiff_t)y * a.xstride) + x0;
        const float* ry = reinterpret_cast<const float*>(a.mapy + (ptrdiff_t)y * a.ystride) + x0;
        float mx[PX], my[PX];
        if (a.vec_map && n == PX) {
            const float4 vx = *reinterpret_cast<const float4*>(rx), vy = *reinterpret_cast<const float4*>(ry);
            mx[0] = vx.x; mx[1] = vx.y; mx[2] = vx.z; mx[3] = vx.w;
            my[0] = vy.x; my[1] = vy.y; my[2] = vy.z; my[3] = vy.w;
        } else {
#pragma unroll
            for (int i = 0; i < PX; i++) {
                mx[i] = i < n ? rx[i] : 0.0f;
                my[i] = i < n ? ry[i] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < PX; i++) t[i] = tap_of(mx[i], my[i]);
    }

    const int k0 = blockIdx.y * IMAGES, k1 = min(k0 + IMAGES, a.n);
    for (int k = k0; k < k1; k++) {
        const uint8_t* img = a.src + (ptrdiff_t)k * a.simage;
        uint8_t* d = a.dst + (ptrdiff_t)k * a.dimage + (ptrdiff_t)y * a.dstride + (ptrdiff_t)x0 * CH;
        uint32_t out[PX][CH];
#pragma unroll
        for (int i = 0; i < PX; i++) {
            if (i < n) sample_px<CH>(img, a.sstride, a.srcW, a.srcH, t[i], a.border, out[i]);
        }
        if (a.vec_dst && n == PX) {
            uint32_t w[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) w[j] = 0;
#pragma unroll
            for (int i = 0; i < PX; i++) {
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    const int b = i * CH + c;
                    w[b >> 2] |= out[i][c] << ((b & 3) * 8);
                }
            }
            uint32_t* o = reinterpret_cast<uint32_t*>(d);
#pragma unroll
            for (int j = 0; j < CH; j++) o[j] = w[j];
            continue;
        }
#pragma unroll
        for (int i = 0; i < PX; i++) {
            if (i >= n) break;
#pragma unroll
            for (int c = 0; c < CH; c++) d[i * CH + c] = (uint8_t)out[i][c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
const char* const IM = "initUndistortRectifyMap";
const char* const RM = "remap";
const char* const RV = "rectifyViews";

struct MapCall {                       // one adf_init_undistort_rectify_map_* call as its C entry point received it
    const adf_rectify_params* prm; int W, H;
    float* mapx; ptrdiff_t xstride; float* mapy; ptrdiff_t ystride;
};

// base and strides of both map planes are multiples of `align`
bool maps_aligned(const float* mapx, ptrdiff_t xstride, const float* mapy, ptrdiff_t ystride, int align)
{
    return (((uintptr_t)mapx | (uintptr_t)xstride | (uintptr_t)mapy | (uintptr_t)ystride) & (uintptr_t)(align - 1)) == 0;
}

int map_check(const MapCall& c)
{
    if (!c.prm) return fail(ADF_EBADARG, "%s: prm must not be null", IM);
    if (c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "%s: the size is empty", IM);
    if (!c.mapx || !c.mapy) return fail(ADF_EBADARG, "%s: mapx and mapy must not be null", IM);
    if ((int64_t)c.W * c.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "%s: W*H must be below 2^31", IM);
    if (!maps_aligned(c.mapx, c.xstride, c.mapy, c.ystride, 4))
        return fail(ADF_EBADARG, "%s: the maps and their strides must be 4-byte aligned", IM);
    if (c.xstride < (ptrdiff_t)c.W * 4 || c.ystride < (ptrdiff_t)c.W * 4) return fail(ADF_ESIZE, "%s: row stride smaller than a row", IM);
    return ADF_OK;
}

int map_launch(const MapCall& c, hipStream_t st)
{
    MapArgs a;
    a.mapx = reinterpret_cast<char*>(c.mapx); a.xstride = c.xstride;
    a.mapy = reinterpret_cast<char*>(c.mapy); a.ystride = c.ystride;
    a.W = c.W; a.H = c.H;
    a.groups = (c.W + PX - 1) / PX;
    a.total = (int)((int64_t)a.groups * c.H);                        // (W * H < 2^31)
    a.vec = maps_aligned(c.mapx, c.xstride, c.mapy, c.ystride, 16);
    a.p = *c.prm;
    hipLaunchKernelGGL(rectify_map_kernel, dim3((unsigned)(((int64_t)a.total + NT - 1) / NT)), dim3(NT), 0, st, a);
    return launched();
}

// One sampling call as its C entry point received it.  remap has the maps and no prm, rectifyViews prm and no maps.
struct SampleCall {
    const char* who; int n;
    const uint8_t* src; ptrdiff_t sstride, simage; int srcW, srcH, ch;
    const float* mapx; ptrdiff_t xstride; const float* mapy; ptrdiff_t ystride; const adf_rectify_params* prm;
    uint8_t* dst; ptrdiff_t dstride, dimage; int W, H, interpolation, border_mode; const uint8_t* border;
};

// Everything about a sampling call that can be refused without a device, but for its maps or its prm.
int sample_check(const SampleCall& c)
{
    if (c.n < 1) return fail(ADF_EBADARG, "%s: n_images must be at least 1", c.who);
    if (!c.src || !c.dst) return fail(ADF_EBADARG, "%s: src and dst must not be null", c.who);
    if (c.srcW < 1 || c.srcH < 1 || c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "%s: the source or the destination image is empty", c.who);
    if (c.ch != 1 && c.ch != 3) return fail(ADF_EBADARG, "%s: images must be CV_8UC1 or CV_8UC3", c.who);
    if (c.interpolation != ADF_INTER_LINEAR || c.border_mode != ADF_BORDER_CONSTANT)
        return fail(ADF_EBADARG, "%s: INTER_LINEAR with BORDER_CONSTANT only", c.who);
    if (c.srcW > MAX_SRC_DIM || c.srcH > MAX_SRC_DIM) return fail(ADF_ESIZE, "%s: srcW and srcH must not exceed 32767", c.who);
    if ((int64_t)c.W * c.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "%s: W*H must be below 2^31", c.who);
    if (c.sstride < (ptrdiff_t)c.srcW * c.ch || c.dstride < (ptrdiff_t)c.W * c.ch) return fail(ADF_ESIZE, "%s: row stride smaller than a row", c.who);
    if (c.n > 1 && c.simage < 0) return fail(ADF_EBADARG, "%s: negative image stride", c.who);
    if (!images_disjoint(c.n, (ptrdiff_t)c.W * c.ch, c.H, c.dstride, c.dimage, true))
        return fail(ADF_EBADARG, "%s: destination images overlap", c.who);
    return ADF_OK;
}

int remap_check(const SampleCall& c)
{
    if (const int rc = sample_check(c)) return rc;
    if (!c.mapx || !c.mapy) return fail(ADF_EBADARG, "remap: mapx and mapy must not be null");
    if (!maps_aligned(c.mapx, c.xstride, c.mapy, c.ystride, 4))
        return fail(ADF_EBADARG, "remap: the maps and their strides must be 4-byte aligned");
    if (c.xstride < (ptrdiff_t)c.W * 4 || c.ystride < (ptrdiff_t)c.W * 4) return fail(ADF_ESIZE, "remap: map row stride smaller than a row");
    return ADF_OK;
}

int rectify_views_check(const SampleCall& c)
{
    if (const int rc = sample_check(c)) return rc;
    return c.prm ? ADF_OK : fail(ADF_EBADARG, "%s: prm must not be null", RV);
}

int sample_launch(const SampleCall& c, hipStream_t st)
{
    SampleArgs a = {};
    a.sstride = c.sstride; a.simage = c.n > 1 ? c.simage : 0;
    a.srcW = c.srcW; a.srcH = c.srcH;
    a.mapx = reinterpret_cast<const char*>(c.mapx); a.xstride = c.xstride;
    a.mapy = reinterpret_cast<const char*>(c.mapy); a.ystride = c.ystride;
    a.dstride = c.dstride; a.dimage = c.n > 1 ? c.dimage : 0;
    a.W = c.W; a.H = c.H;
    a.groups = (c.W + PX - 1) / PX;
    a.total = (int)((int64_t)a.groups * c.H);                        // (W * H < 2^31)
    a.vec_map = maps_aligned(c.mapx, c.xstride, c.mapy, c.ystride, 16);
    a.vec_dst = (((uintptr_t)c.dst | (uintptr_t)a.dstride | (uintptr_t)a.dimage) & 3) == 0;
    for (int k = 0; k < 3; k++) a.border[k] = c.border ? c.border[k < c.ch ? k : 0] : 0;
    if (c.prm) a.p = *c.prm;
    const unsigned blocks = (unsigned)(((int64_t)a.total + NT - 1) / NT);
    const auto kernel = c.prm ? (c.ch == 3 ? sample_kernel<3, true> : sample_kernel<1, true>)
                              : (c.ch == 3 ? sample_kernel<3, false> : sample_kernel<1, false>);
    return for_batches(c.n, GRID_LIMIT * IMAGES, [&](int m0, int nm) {
        a.n = nm;
        a.src = c.src + (ptrdiff_t)m0 * a.simage;
        a.dst = c.dst + (ptrdiff_t)m0 * a.dimage;
        hipLaunchKernelGGL(kernel, dim3(blocks, (unsigned)((nm + IMAGES - 1) / IMAGES)), dim3(NT), 0, st, a);
        return launched();
    });
}

// The _host form of both sampling calls: one block holds the source images, the maps (remap) and the destination
// images, rows padded to 16 bytes.
int sample_host(const SampleCall& c)
{
    const int n = c.n;
    const size_t srow = (size_t)c.srcW * c.ch, drow = (size_t)c.W * c.ch, mrow = (size_t)c.W * 4;
    const size_t sp = pad_to(srow, 16), dp = pad_to(drow, 16), mp = pad_to(mrow, 16);
    const size_t simg = sp * c.srcH, dimg = dp * c.H, mplane = c.mapx ? mp * c.H : 0;
    Scratch blk;
    int rc;
    if ((rc = blk.take((simg + dimg) * (size_t)n + 2 * mplane, nullptr))) return rc;
    uint8_t* ds = static_cast<uint8_t*>(blk.p);
    uint8_t* dd = ds + simg * n;
    float* dx = reinterpret_cast<float*>(dd + dimg * n);
    float* dy = reinterpret_cast<float*>(reinterpret_cast<char*>(dx) + mplane);
    SampleCall d = c;                                                // the same call on the staged copies
    d.src = ds; d.sstride = (ptrdiff_t)sp; d.simage = (ptrdiff_t)simg;
    d.dst = dd; d.dstride = (ptrdiff_t)dp; d.dimage = (ptrdiff_t)dimg;
    if ((rc = copy_images(ds, sp, simg, c.src, c.sstride, c.simage, srow, c.srcH, n, hipMemcpyHostToDevice, nullptr))) return rc;
    if (c.mapx) {
        d.mapx = dx; d.mapy = dy; d.xstride = d.ystride = (ptrdiff_t)mp;
        if ((rc = copy_images(dx, mp, 0, c.mapx, c.xstride, 0, mrow, c.H, 1, hipMemcpyHostToDevice, nullptr))) return rc;
        if ((rc = copy_images(dy, mp, 0, c.mapy, c.ystride, 0, mrow, c.H, 1, hipMemcpyHostToDevice, nullptr))) return rc;
    }
    if ((rc = sample_launch(d, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(c.dst, c.dstride, c.dimage, dd, dp, dimg, drow, c.H, n, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

} // namespace

extern "C" int adf_rectify_params_init(const double K[9], const double* dist, int n_dist, const double* R, const double* P,
                                       int p_cols, adf_rectify_params* out)
{
    if (!K || !P || !out) return fail(ADF_EBADARG, "adf_rectify_params_init: K, P and out must not be null");
    if (n_dist != 0 && n_dist != 4 && n_dist != 5 && n_dist != 8)
        return fail(ADF_EBADARG, "adf_rectify_params_init: n_dist must be 0, 4, 5 or 8 (the thin-prism and tilted models of 12 "
                                 "and 14 coefficients are not built)");
    if (n_dist > 0 && !dist) return fail(ADF_EBADARG, "adf_rectify_params_init: dist must not be null when n_dist > 0");
    if (p_cols != 3 && p_cols != 4) return fail(ADF_EBADARG, "adf_rectify_params_init: p_cols must be 3 or 4");
    double a[3][3];                                                  // A = P[:, :3] * R
    for (int i = 0; i < 3; i++) {
        const double* p = P + i * p_cols;
        for (int j = 0; j < 3; j++) a[i][j] = R ? (p[0] * R[j] + p[1] * R[3 + j]) + p[2] * R[6 + j] : p[j];
    }
    // the signed cofactors: two products and one difference each
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double c10 = a[0][2] * a[2][1] - a[0][1] * a[2][2], c11 = a[0][0] * a[2][2] - a[0][2] * a[2][0], c12 = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    const double c20 = a[0][1] * a[1][2] - a[0][2] * a[1][1], c21 = a[0][2] * a[1][0] - a[0][0] * a[1][2], c22 = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = (a[0][0] * c00 + a[0][1] * c01) + a[0][2] * c02;   // by the first row
    if (det == 0.0 || !std::isfinite(det)) return fail(ADF_EBADARG, "adf_rectify_params_init: P[:, :3] * R is singular or not finite");
    adf_rectify_params o;
    o.fx = K[0]; o.fy = K[4]; o.cx = K[2]; o.cy = K[5];
    for (int i = 0; i < 8; i++) o.dist[i] = i < n_dist ? dist[i] : 0.0;
    // the inverse: the adjugate (transposed cofactors), one division per entry
    o.ir[0] = c00 / det; o.ir[1] = c10 / det; o.ir[2] = c20 / det;
    o.ir[3] = c01 / det; o.ir[4] = c11 / det; o.ir[5] = c21 / det;
    o.ir[6] = c02 / det; o.ir[7] = c12 / det; o.ir[8] = c22 / det;
    *out = o;
    return ADF_OK;
}

extern "C" int adf_init_undistort_rectify_map_device(const adf_rectify_params* prm, int W, int H, float* mapx, ptrdiff_t mapx_stride,
                                                     float* mapy, ptrdiff_t mapy_stride, void* stream)
{
    const MapCall c{prm, W, H, mapx, mapx_stride, mapy, mapy_stride};
    const int rc = map_check(c);
    return rc ? rc : map_launch(c, (hipStream_t)stream);
}

extern "C" int adf_init_undistort_rectify_map_host(const adf_rectify_params* prm, int W, int H, float* mapx, ptrdiff_t mapx_stride,
                                                   float* mapy, ptrdiff_t mapy_stride)
{
    const MapCall c{prm, W, H, mapx, mapx_stride, mapy, mapy_stride};
    int rc = map_check(c);
    if (rc) return rc;
    const size_t mrow = (size_t)W * 4, mp = pad_to(mrow, 16), plane = mp * H;
    Scratch blk;
    if ((rc = blk.take(2 * plane, nullptr))) return rc;
    MapCall d = c;                                                   // the same call into the staged planes
    d.mapx = static_cast<float*>(blk.p); d.mapy = reinterpret_cast<float*>(static_cast<char*>(blk.p) + plane);
    d.xstride = d.ystride = (ptrdiff_t)mp;
    if ((rc = map_launch(d, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(mapx, mapx_stride, 0, d.mapx, mp, 0, mrow, H, 1, hipMemcpyDeviceToHost, nullptr))) return rc;
    if ((rc = copy_images(mapy, mapy_stride, 0, d.mapy, mp, 0, mrow, H, 1, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

extern "C" int adf_remap_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW, int srcH,
                                int channels, const float* mapx, ptrdiff_t mapx_stride, const float* mapy, ptrdiff_t mapy_stride,
                                uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride, int W, int H, int interpolation,
                                int border_mode, const uint8_t* border_value, void* stream)
{
    const SampleCall c{RM, n_images, src, src_stride, src_image_stride, srcW, srcH, channels, mapx, mapx_stride, mapy, mapy_stride,
                       nullptr, dst, dst_stride, dst_image_stride, W, H, interpolation, border_mode, border_value};
    const int rc = remap_check(c);
    return rc ? rc : sample_launch(c, (hipStream_t)stream);
}

extern "C" int adf_remap_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW, int srcH,
                              int channels, const float* mapx, ptrdiff_t mapx_stride, const float* mapy, ptrdiff_t mapy_stride,
                              uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride, int W, int H, int interpolation,
                              int border_mode, const uint8_t* border_value)
{
    const SampleCall c{RM, n_images, src, src_stride, src_image_stride, srcW, srcH, channels, mapx, mapx_stride, mapy, mapy_stride,
                       nullptr, dst, dst_stride, dst_image_stride, W, H, interpolation, border_mode, border_value};
    const int rc = remap_check(c);
    return rc ? rc : sample_host(c);
}

extern "C" int adf_rectify_views_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW,
                                        int srcH, int channels, const adf_rectify_params* prm, uint8_t* dst, ptrdiff_t dst_stride,
                                        ptrdiff_t dst_image_stride, int W, int H, int interpolation, int border_mode,
                                        const uint8_t* border_value, void* stream)
{
    const SampleCall c{RV, n_images, src, src_stride, src_image_stride, srcW, srcH, channels, nullptr, 0, nullptr, 0,
                       prm, dst, dst_stride, dst_image_stride, W, H, interpolation, border_mode, border_value};
    const int rc = rectify_views_check(c);
    return rc ? rc : sample_launch(c, (hipStream_t)stream);
}

extern "C" int adf_rectify_views_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride, int srcW,
                                      int srcH, int channels, const adf_rectify_params* prm, uint8_t* dst, ptrdiff_t dst_stride,
                                      ptrdiff_t dst_image_stride, int W, int H, int interpolation, int border_mode,
                                      const uint8_t* border_value)
{
    const SampleCall c{RV, n_images, src, src_stride, src_image_stride, srcW, srcH, channels, nullptr, 0, nullptr, 0,
                       prm, dst, dst_stride, dst_image_stride, W, H, interpolation, border_mode, border_value};
    const int rc = rectify_views_check(c);
    return rc ? rc : sample_host(c);
}
