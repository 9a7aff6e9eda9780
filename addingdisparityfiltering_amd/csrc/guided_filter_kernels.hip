// guided_filter_kernels.hip -- cv::ximgproc::guidedFilter(guide, src, dst, radius, eps, dDepth) on the device, in the
// library's own definition (include/adf_wls.h, "guided filter", is the statement; tests/gf_ref.py states it in NumPy):
//
//   stage 1  per pixel the sums of I_c, I_c I_d, p, I_c p over the (2r+1)^2 window (BORDER_REFLECT), exact: integers for
//            integer sources, doubles in a fixed order for float sources; from them the linear model a_c, b of the window
//            in double, stored as float planes                                                      (gf_coef_kernel)
//   stage 2  the float32 window sums of a_c and b in ONE fixed order -- column sum top to bottom, then row sum left to
//            right, every partial sum rounded -- blended with the pixel's guide, converted, stored      (gf_apply_kernel)
//
// Both kernels: one workgroup of NT = TW x TH threads per output tile, one output pixel per thread.  A window sum is
// separable and goes through LDS (window_sum): the tile with its reflected halo of r is staged once, then per quantity
// every thread forms column sums C of the TH tile rows over the TW + 2r staged columns into one shared plane, a barrier,
// and every thread adds the 2r + 1 neighbours of its row -- 2 (2r + 1) adds per quantity and pixel, in the statement's
// order, so the same code serves the order-free integer sums and the fixed-order float / double ones.  The quantities go
// one after another through the same column plane (4 with a 1-channel guide, 13 with 3 channels; 2 / 4 planes in stage
// 2), their results stay in registers: LDS holds one staged tile and one column plane, whatever the channel count.
//
// Lanes 0..31 of a wave read 32 adjacent entries of a row (4-byte entries: all 32 banks once; the guide's bytes: four
// lanes share a word); the coefficient planes are dense float planes of the map's width, so a wave stores and loads two
// runs of 128 contiguous bytes.
//
// LDS at r = 31: stage 1 (TW + 62)(TH + 62) entries of 4 + 3 bytes + (TW + 62) TH column sums of 8 bytes = 51 KiB;
// stage 2, 4-byte entries and sums, 29 KiB.  Times and what bounds them: DESIGN.md, section 21.
#include "adf_host.h"

#include <cmath>
#include <type_traits>

using namespace adf;

namespace {

constexpr int TW = 32, TH = 8, NT = TW * TH;                             // the output tile of a workgroup
constexpr size_t tile_entries(int r) { return (size_t)(TW + 2 * r) * (TH + 2 * r); }   // the tile and its halo
constexpr size_t col_entries(int r) { return (size_t)(TW + 2 * r) * TH; }               // the column sums of the tile's rows
constexpr size_t coef_lds(int r, int ch) { return tile_entries(r) * (4 + ch) + col_entries(r) * 8; }
constexpr size_t apply_lds(int r) { return (tile_entries(r) + col_entries(r)) * 4; }
static_assert(coef_lds(ADF_GF_MAX_RADIUS, 3) <= 64 * 1024 && apply_lds(ADF_GF_MAX_RADIUS) <= 64 * 1024, "a workgroup's LDS");
// the integer sums: a window of I_c I_d fits int32, a window of I_c p and the products N S, S S fit int64 (and 2^53)
static_assert((2 * ADF_GF_MAX_RADIUS + 1) * (2 * ADF_GF_MAX_RADIUS + 1) * 255 * 255 < (1ll << 31), "S_cd fits int32");
static_assert(3969ll * 3969 * 255 * 32768 < (1ll << 53), "N S_cp and S_c S_p convert to double exactly");

struct GfArgs {
    const uint8_t* guide; ptrdiff_t guide_stride, guide_map_stride;      // bytes
    const void* src; ptrdiff_t src_stride, src_map_stride;
    void* dst; ptrdiff_t dst_stride, dst_map_stride;
    float* planes;                                                       // [map][guide channels + 1][H][W]: a_c, then b
    int W, H, r;
    unsigned tiles_x, tile0;                                             // tiles per row of tiles; first tile of this launch
    double eps;
};

// BORDER_REFLECT of index i on an axis of length n (numpy.pad's "symmetric"), for any i.
__device__ __forceinline__ int reflect(long long i, int n)
{
    if (i >= 0 && i < n) return (int)i;
    const long long p = 2ll * n;
    long long m = i % p;
    if (m < 0) m += p;
    return (int)(m < n ? m : p - 1 - m);
}

// The window sum of one quantity for this thread's pixel: tap(k) is the quantity at entry k of the staged tile, SW entries
// per row.  Column sums top to bottom into `col` (one per tile row and staged column), then the row sum left to right;
// each partial sum is an Acc.  Every thread of the workgroup calls it; `col` is free again on return.
template <class Acc, class F>
__device__ __forceinline__ Acc window_sum(Acc* col, int r, int SW, F&& tap)
{
    const int t = threadIdx.x, n = 2 * r + 1;
    for (int i = t; i < TH * SW; i += NT) {                              // tile row i / SW, staged column i % SW: entry i is its top tap
        Acc c = tap(i);
        for (int dy = 1; dy < n; dy++) c += tap(i + dy * SW);
        col[i] = c;
    }
    __syncthreads();
    const Acc* row = col + (t / TW) * SW + t % TW;
    Acc s = row[0];
    for (int dx = 1; dx < n; dx++) s += row[dx];
    __syncthreads();
    return s;
}

// A source depth in stage 1: how a tile entry holds it (4 bytes) and what its sums are made of.
template <class T> struct Source {                                       // uint8_t, int16_t: exact integer sums
    using Lds = int;
    using Sum = long long;
    static __device__ __forceinline__ Sum value(Lds v) { return v; }
    // n_c = N S_cp - S_c S_p
    static __device__ __forceinline__ double numerator(int N, Sum Scp, int Sc, Sum Sp) { return (double)((long long)N * Scp - (long long)Sc * Sp); }
};
template <> struct Source<float> {                                       // doubles in the fixed order
    using Lds = float;
    using Sum = double;
    static __device__ __forceinline__ Sum value(Lds v) { return (double)v; }
    static __device__ __forceinline__ double numerator(int N, Sum Scp, int Sc, Sum Sp) { return (double)N * Scp - (double)Sc * Sp; }
};

template <class T, int CH>
__global__ void __launch_bounds__(NT) gf_coef_kernel(GfArgs a)
{
    using S = Source<T>;
    using Sum = typename S::Sum;
    extern __shared__ __align__(16) unsigned char smem[];
    const int t = threadIdx.x, r = a.r, SW = TW + 2 * r, SH = TH + 2 * r, entries = SW * SH;
    Sum* col = reinterpret_cast<Sum*>(smem);                             // [TH][SW], 8-byte sums (the guide's int sums use its front)
    typename S::Lds* ps = reinterpret_cast<typename S::Lds*>(smem + col_entries(r) * 8);   // [SH][SW] the source
    uint8_t* gs = reinterpret_cast<uint8_t*>(ps + entries);              // [CH][SH][SW] the guide, a plane per channel
    const unsigned tid = a.tile0 + blockIdx.x;
    const int x0 = (int)(tid % a.tiles_x) * TW, y0 = (int)(tid / a.tiles_x) * TH;
    const ptrdiff_t m = blockIdx.y;
    const uint8_t* guide = a.guide + m * a.guide_map_stride;
    const char* src = static_cast<const char*>(a.src) + m * a.src_map_stride;

    for (int i = t; i < entries; i += NT) {                              // stage the tile and its reflected halo
        const int sy = i / SW, sx = i - sy * SW, gx = reflect((long long)x0 - r + sx, a.W), gy = reflect((long long)y0 - r + sy, a.H);
        ps[i] = (typename S::Lds)reinterpret_cast<const T*>(src + (ptrdiff_t)gy * a.src_stride)[gx];
        const uint8_t* g = guide + (ptrdiff_t)gy * a.guide_stride + (ptrdiff_t)gx * CH;
#pragma unroll
        for (int c = 0; c < CH; c++) gs[c * entries + i] = g[c];
    }
    __syncthreads();

    const int n = 2 * r + 1, N = n * n;
    int* icol = reinterpret_cast<int*>(col);
    int Sc[CH], Scd[CH][CH];                                             // Scd: c <= d used
    Sum Sp, Scp[CH];
    Sp = window_sum<Sum>(col, r, SW, [&](int k) { return S::value(ps[k]); });
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const uint8_t* gc = gs + c * entries;
        Sc[c] = window_sum<int>(icol, r, SW, [&](int k) { return (int)gc[k]; });
        Scp[c] = window_sum<Sum>(col, r, SW, [&](int k) { return (Sum)(int)gc[k] * S::value(ps[k]); });
#pragma unroll
        for (int d = c; d < CH; d++) {
            const uint8_t* gd = gs + d * entries;
            Scd[c][d] = window_sum<int>(icol, r, SW, [&](int k) { return (int)gc[k] * (int)gd[k]; });
        }
    }

    const int x = x0 + t % TW, y = y0 + t / TW;
    if (x >= a.W || y >= a.H) return;                                    // (no barrier follows)
    const double Nd = (double)N, E = a.eps * Nd * Nd;
    auto V = [&](int c, int d) { return (double)((long long)N * Scd[c][d] - (long long)Sc[c] * Sc[d]); };
    double nc[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) nc[c] = S::numerator(N, Scp[c], Sc[c], Sp);
    float ac[CH];
    if constexpr (CH == 1) {
        ac[0] = (float)(nc[0] / (V(0, 0) + E));
    } else {
        const double s00 = V(0, 0) + E, s11 = V(1, 1) + E, s22 = V(2, 2) + E, s01 = V(0, 1), s02 = V(0, 2), s12 = V(1, 2);
        const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
        const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
        const double det = (s00 * c00 + s01 * c01) + s02 * c02;
        const bool ok = det > 0.0 && det <= 1.79769313486231570e308;     // finite and > 0
        ac[0] = ok ? (float)(((c00 * nc[0] + c01 * nc[1]) + c02 * nc[2]) / det) : 0.0f;
        ac[1] = ok ? (float)(((c01 * nc[0] + c11 * nc[1]) + c12 * nc[2]) / det) : 0.0f;
        ac[2] = ok ? (float)(((c02 * nc[0] + c12 * nc[1]) + c22 * nc[2]) / det) : 0.0f;
    }
    double bn = (double)Sp;
#pragma unroll
    for (int c = 0; c < CH; c++) bn = bn - (double)ac[c] * (double)Sc[c];
    const size_t plane = (size_t)a.W * a.H;
    float* out = a.planes + (size_t)m * (CH + 1) * plane + (size_t)y * a.W + x;
#pragma unroll
    for (int c = 0; c < CH; c++) out[c * plane] = ac[c];
    out[CH * plane] = (float)(bn / Nd);
}

// dst = q in the output's depth: (float)q, or rint (half to even) saturated; a NaN gives the depth's minimum.
template <class T> __device__ __forceinline__ T convert(double q)
{
    if constexpr (std::is_same<T, float>::value) {
        return (float)q;
    } else {
        const double lo = std::is_same<T, uint8_t>::value ? 0.0 : -32768.0, hi = std::is_same<T, uint8_t>::value ? 255.0 : 32767.0;
        const double v = rint(q);
        return !(v >= lo) ? (T)lo : v > hi ? (T)hi : (T)v;
    }
}

template <class T, int CH>
__global__ void __launch_bounds__(NT) gf_apply_kernel(GfArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int t = threadIdx.x, r = a.r, SW = TW + 2 * r, SH = TH + 2 * r, entries = SW * SH;
    float* col = reinterpret_cast<float*>(smem);                         // [TH][SW]
    float* vs = col + col_entries(r);                                    // [SH][SW] one coefficient plane's tile
    const unsigned tid = a.tile0 + blockIdx.x;
    const int x0 = (int)(tid % a.tiles_x) * TW, y0 = (int)(tid / a.tiles_x) * TH;
    const ptrdiff_t m = blockIdx.y;
    const size_t plane = (size_t)a.W * a.H;
    const float* planes = a.planes + (size_t)m * (CH + 1) * plane;

    float sum[CH + 1];                                                   // SA_c, then SB
#pragma unroll
    for (int c = 0; c <= CH; c++) {
        const float* p = planes + c * plane;
        for (int i = t; i < entries; i += NT) {                          // (the last window_sum ended with a barrier)
            const int sy = i / SW, sx = i - sy * SW;
            vs[i] = p[(size_t)reflect((long long)y0 - r + sy, a.H) * a.W + reflect((long long)x0 - r + sx, a.W)];
        }
        __syncthreads();
        sum[c] = window_sum<float>(col, r, SW, [&](int k) { return vs[k]; });
    }

    const int x = x0 + t % TW, y = y0 + t / TW;
    if (x >= a.W || y >= a.H) return;
    const uint8_t* g = a.guide + m * a.guide_map_stride + (ptrdiff_t)y * a.guide_stride + (ptrdiff_t)x * CH;
    const int n = 2 * r + 1;
    double q = (double)sum[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) q = q + (double)sum[c] * (double)g[c];
    q = q / (double)(n * n);
    reinterpret_cast<T*>(static_cast<char*>(a.dst) + m * a.dst_map_stride + (ptrdiff_t)y * a.dst_stride)[x] = convert<T>(q);
}

struct GfCall {                        // one call as its C entry point received it
    FilterImages im;
    int r; double eps;
};

constexpr const char* WHO = "guidedFilter";

int gf_check(const GfCall& c)
{
    const FilterImages& im = c.im;
    if (!im.guide.p || !im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: guide, src and dst must be non-NULL", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(im.src_depth) || !known_depth(im.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (im.guide_channels != 1 && im.guide_channels != 3) return fail(ADF_EBADARG, "%s: guide must have 1 or 3 channels", WHO);
    if (c.r < 0 || c.r > ADF_GF_MAX_RADIUS) return fail(ADF_EBADARG, "%s: r must lie in [0, %d]", WHO, ADF_GF_MAX_RADIUS);
    if (!std::isfinite(c.eps) || !(c.eps > 0.0)) return fail(ADF_EBADARG, "%s: eps must be finite and > 0", WHO);
    return filter_geometry_check(WHO, im, "their depths", "src or guide");
}

// The launches of one stage: `kernel` over every tile of every map.
int gf_launch(const GfCall& c, const GfArgs& a, void (*kernel)(GfArgs), size_t lds, hipStream_t st)
{
    const FilterImages& im = c.im;
    const size_t planes_per_map = (size_t)(im.guide_channels + 1) * im.W * im.H;
    return launch_tiles(kernel, lds, im.W, im.H, TW, TH, im.n, a, st, [&](GfArgs& t, int m0) {
        t.guide = im.guide.map(m0); t.src = im.src.map(m0); t.dst = im.dst.map(m0);
        t.planes = a.planes + planes_per_map * m0;
    });
}

template <int CH>
int gf_stages(const GfCall& c, const GfArgs& a, hipStream_t st)
{
    const size_t l1 = coef_lds(c.r, CH), l2 = apply_lds(c.r);
    int rc = c.im.src_depth == ADF_8U    ? gf_launch(c, a, gf_coef_kernel<uint8_t, CH>, l1, st)
             : c.im.src_depth == ADF_16S ? gf_launch(c, a, gf_coef_kernel<int16_t, CH>, l1, st)
                                         : gf_launch(c, a, gf_coef_kernel<float, CH>, l1, st);
    if (rc) return rc;
    return c.im.dst_depth == ADF_8U    ? gf_launch(c, a, gf_apply_kernel<uint8_t, CH>, l2, st)
           : c.im.dst_depth == ADF_16S ? gf_launch(c, a, gf_apply_kernel<int16_t, CH>, l2, st)
                                       : gf_launch(c, a, gf_apply_kernel<float, CH>, l2, st);
}

// ws: adf_guided_filter_workspace_bytes of device memory, the coefficient planes of every map
int gf_run(const GfCall& c, void* ws, hipStream_t st)
{
    const FilterImages& im = c.im;
    GfArgs a{};
    a.guide_stride = im.guide.stride; a.guide_map_stride = im.guide.map_stride;
    a.src_stride = im.src.stride; a.src_map_stride = im.src.map_stride;
    a.dst_stride = im.dst.stride; a.dst_map_stride = im.dst.map_stride;
    a.planes = static_cast<float*>(ws);
    a.W = im.W; a.H = im.H; a.r = c.r; a.eps = c.eps;
    return im.guide_channels == 3 ? gf_stages<3>(c, a, st) : gf_stages<1>(c, a, st);
}

GfCall call_of(int n_maps, const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth, int W, int H, int r, double eps)
{
    return GfCall{{n_maps, W, H, image_of(guide, guide_stride, guide_map_stride), guide_channels, image_of(src, src_stride, src_map_stride), src_depth,
                   image_of(dst, dst_stride, dst_map_stride), dst_depth, {}}, r, eps};
}

} // namespace

extern "C" size_t adf_guided_filter_workspace_bytes(int n_maps, int W, int H, int guide_channels)
{
    if (n_maps < 1 || W < 1 || H < 1 || (guide_channels != 1 && guide_channels != 3)) return 0;
    return (size_t)n_maps * (size_t)(guide_channels + 1) * (size_t)W * (size_t)H * sizeof(float);
}

extern "C" int adf_guided_filter_device(int n_maps,
                                        const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                        const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                        void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                        int W, int H, int r, double eps,
                                        void* workspace, size_t workspace_bytes, void* stream)
{
    const GfCall c = call_of(n_maps, guide, guide_stride, guide_map_stride, guide_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, r, eps);
    int rc = gf_check(c);
    if (rc) return rc;
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch(WHO, "adf_guided_filter_workspace_bytes", workspace, workspace_bytes,
                              adf_guided_filter_workspace_bytes(n_maps, W, H, guide_channels), (hipStream_t)stream, blk, &ws);
    return rc ? rc : gf_run(c, ws, (hipStream_t)stream);
}

extern "C" int adf_guided_filter_host(int n_maps,
                                      const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                      const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                      void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                      int W, int H, int r, double eps)
{
    const GfCall c = call_of(n_maps, guide, guide_stride, guide_map_stride, guide_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, r, eps);
    int rc = gf_check(c);
    if (rc) return rc;
    // the workspace: the coefficient planes
    return staged_call(c.im, adf_guided_filter_workspace_bytes(n_maps, W, H, guide_channels), [&](const FilterImages& staged, void* ws, hipStream_t st) {
        return gf_run(GfCall{staged, c.r, c.eps}, ws, st);               // the same call on the staged images
    });
}
