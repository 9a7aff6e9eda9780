// wmf_kernels.hip -- cv::ximgproc::weightedMedianFilter(joint, src, dst, r, sigma, weightType, mask) on the device, in the
// library's own integer definition (include/adf_wls.h, "weighted median filter", is the statement; tests/wmf_ref.py states
// it in NumPy):
//
//   used(q)  = inside the image && mask(q) != 0 && !(use_ignore && src(q) == ignore_value) && !isnan(src(q))
//   w(p, q)  = T[ sum_c (joint_c(p) - joint_c(q))^2 ]                       uint32, at most 65536
//   Tot      = sum of w over the used taps of the (2r+1)^2 window, L(v) = the same over taps with src(q) <= v
//   dst(p)   = the smallest tap value v with 2 L(v) >= Tot;  Tot == 0: src(p)
//
// One workgroup of NT = TW x TH threads per output tile, one output pixel per thread.  The tile and its halo of r are
// staged in LDS as one 8-byte entry per pixel: the source value as an order-preserving unsigned 32-bit KEY and the joint
// pixel (its 1 or 3 bytes in a word).  Everything that makes a tap unused -- outside the image, mask, ignore value, NaN --
// is decided ONCE, while staging: such an entry holds the reserved key MARK, so the selection loop has no variants and
// no bounds test.  MARK is all ones: above every key of the integer depths, and among float keys the image of a NaN.
//
// Selection per pixel, all integer:
//   pass 1   Tot and the smallest and largest used key [lo, hi]
//   steps    while lo < hi: mid = lo + (hi - lo) / 2; one sweep of the window gives L(mid), the largest key <= mid
//            (`below`) and the smallest key > mid (`above`); 2 L(mid) >= Tot ? hi = below : lo = above
//   Both ends stay tap keys with 2 L(hi) >= Tot and 2 L(lo - 1) < Tot, the interval shrinks every step, and snapping
//   the ends to keys that occur ends the search after at most as many steps as the window has distinct values below /
//   above the median -- a handful in a disparity map -- and never more than the key's bit count (8 / 16 / 32).
// Each sweep re-reads the taps from LDS, a row four taps at a time with their reads in flight together and no branch: one
// 8-byte read per tap (lanes 0..31 of a wave read 32 adjacent entries, all 64 banks once: conflict-free at every row
// pitch) plus the weight: a 1-channel joint uses only T[d^2], |d| <= 255, 256 entries kept in LDS; a 3-channel joint
// indexes the 768 KiB table in global memory, which sits in L2.  No float arithmetic takes part.
//
// LDS: (TW + 2r)(TH + 2r) + 3 entries of 8 B + 1 KiB: 8.9 KiB at r = 7, 52.4 KiB at r = 31 -- three workgroups per CU of
// 160 KiB.  28 or 29 registers, no scratch.  Times and what bounds them: DESIGN.md, section 20.
#include "adf_host.h"

#include <cmath>
#include <cstring>
#include <type_traits>

using namespace adf;

namespace {

constexpr int TW = 32, TH = 8, NT = TW * TH;                             // the output tile of a workgroup
constexpr uint32_t MARK = 0xFFFFFFFFu;
constexpr int UN = 4;                                                    // taps of a row whose reads are in flight together
constexpr size_t tile_entries(int r) { return (size_t)(TW + 2 * r) * (TH + 2 * r) + (UN - 1); }   // the tile, its halo, the pad a sweep may read
static_assert(NT == 256 && TW == 32, "a wave's half reads one row of 32 adjacent entries");
static_assert(tile_entries(ADF_WMF_MAX_RADIUS) * 8 + 1024 <= 64 * 1024, "two workgroups per CU at the largest radius");
static_assert((2 * ADF_WMF_MAX_RADIUS + 1) * (2 * ADF_WMF_MAX_RADIUS + 1) * (uint64_t)ADF_WMF_WEIGHT_ONE < (1u << 28), "Tot and 2 L fit 32 bits");

struct WmfArgs {
    const uint8_t* joint; ptrdiff_t joint_stride, joint_map_stride;      // bytes
    const void* src; ptrdiff_t src_stride, src_map_stride;
    void* dst; ptrdiff_t dst_stride, dst_map_stride;
    const uint8_t* mask; ptrdiff_t mask_stride, mask_map_stride;         // mask may be null
    const uint32_t* table;                                               // T, ADF_WMF_TABLE_LEVELS entries
    int W, H, r;
    unsigned tiles_x, tile0;                                             // tiles per row of tiles; first tile of this launch
    int use_ignore; uint32_t ignore;                                     // the ignore value: an integer, or a float's bits
};

// A source depth: how its memory word becomes a key and back.  RAW is the word as loaded (a float's bits: the output is
// the bits of a tap).
template <class T> struct Depth;
template <> struct Depth<uint8_t> {
    using RAW = uint8_t;
    static __device__ __forceinline__ bool unusable(RAW v, int use_ignore, uint32_t ign) { return use_ignore && (uint32_t)v == ign; }
    static __device__ __forceinline__ uint32_t key(RAW v) { return v; }
    static __device__ __forceinline__ RAW value(uint32_t k) { return (RAW)k; }
};
template <> struct Depth<int16_t> {
    using RAW = int16_t;
    static __device__ __forceinline__ bool unusable(RAW v, int use_ignore, uint32_t ign) { return use_ignore && (int)v == (int)ign; }
    static __device__ __forceinline__ uint32_t key(RAW v) { return (uint32_t)((int)v + 32768); }
    static __device__ __forceinline__ RAW value(uint32_t k) { return (RAW)((int)k - 32768); }
};
template <> struct Depth<float> {
    using RAW = uint32_t;
    static __device__ __forceinline__ bool unusable(RAW b, int use_ignore, uint32_t ign)
    {
        if ((b & 0x7FFFFFFFu) > 0x7F800000u) return true;                                    // NaN
        // equal as numbers, on the bits (no float compare: a denormal stays what it is): the same bits, or two zeros
        return use_ignore && (b == ign || ((b | ign) & 0x7FFFFFFFu) == 0u);
    }
    // IEEE total order: negative values reversed below the positive ones; a NaN would land next to MARK or below -inf
    static __device__ __forceinline__ uint32_t key(RAW b) { return b & 0x80000000u ? ~b : b | 0x80000000u; }
    static __device__ __forceinline__ RAW value(uint32_t k) { return k & 0x80000000u ? k ^ 0x80000000u : ~k; }
};

// The joint pixel as a tile entry holds it, and the weight of a tap whose joint word is `q` for a centre `c` where the
// tap counts (`on`), else 0: T[squared distance].
//   1 channel: the word is 4 * joint, so that |q - c| is the byte offset into lds_t[d] = T[d * d] -- one instruction.  The
//   look-up is made for every tap and chosen after: no branch in the sweep.
//   3 channels: the three bytes; the table is read from global memory (L2), and only for the taps that count: a wave's
//   read of 64 scattered words is what a sweep waits for.
template <int CH> __device__ __forceinline__ uint32_t joint_word(const uint8_t* j)
{
    return CH == 1 ? 4u * j[0] : (uint32_t)j[0] | ((uint32_t)j[1] << 8) | ((uint32_t)j[2] << 16);
}
template <int CH> __device__ __forceinline__ uint32_t weight(bool on, uint32_t q, uint32_t c, const uint32_t* lds_t, const uint32_t* t);
template <> __device__ __forceinline__ uint32_t weight<1>(bool on, uint32_t q, uint32_t c, const uint32_t* lds_t, const uint32_t*)
{
    const uint32_t w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(lds_t) + __usad(q, c, 0u));
    return on ? w : 0u;
}
template <> __device__ __forceinline__ uint32_t weight<3>(bool on, uint32_t q, uint32_t c, const uint32_t*, const uint32_t* t)
{
    const int d0 = (int)(q & 255u) - (int)(c & 255u), d1 = (int)((q >> 8) & 255u) - (int)((c >> 8) & 255u), d2 = (int)((q >> 16) & 255u) - (int)((c >> 16) & 255u);
    return on ? t[d0 * d0 + d1 * d1 + d2 * d2] : 0u;
}

template <class T, int CH>
__global__ void __launch_bounds__(NT) wmf_kernel(WmfArgs a)
{
    using D = Depth<T>;
    using RAW = typename D::RAW;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ uint32_t lds_t[256];
    uint2* tile = reinterpret_cast<uint2*>(smem);                        // [(TH + 2r)][(TW + 2r)] {key, joint}
    const int t = threadIdx.x, r = a.r, SW = TW + 2 * r, SH = TH + 2 * r;
    const unsigned tid = a.tile0 + blockIdx.x;
    const int x0 = (int)(tid % a.tiles_x) * TW, y0 = (int)(tid / a.tiles_x) * TH;
    const ptrdiff_t m = blockIdx.y;
    const uint8_t* joint = a.joint + m * a.joint_map_stride;
    const char* src = static_cast<const char*>(a.src) + m * a.src_map_stride;
    const uint8_t* mask = a.mask ? a.mask + m * a.mask_map_stride : nullptr;

    if (CH == 1) lds_t[t] = a.table[t * t];
    for (int i = t; i < (int)tile_entries(r); i += NT) {                 // stage the tile and its halo; the pad is unused
        const int sy = i / SW, sx = i - sy * SW, gx = x0 - r + sx, gy = y0 - r + sy;
        uint2 e = make_uint2(MARK, 0u);
        if (sy < SH && gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const RAW v = reinterpret_cast<const RAW*>(src + (ptrdiff_t)gy * a.src_stride)[gx];
            const bool masked = mask && mask[(ptrdiff_t)gy * a.mask_stride + gx] == 0;
            if (!masked && !D::unusable(v, a.use_ignore, a.ignore)) e.x = D::key(v);
            e.y = joint_word<CH>(joint + (ptrdiff_t)gy * a.joint_stride + (ptrdiff_t)gx * CH);   // (the centre's is needed even where it is unused)
        }
        tile[i] = e;
    }
    __syncthreads();

    const int tx = t % TW, ty = t / TW, x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;                                    // (no barrier follows)
    const uint2* win = tile + ty * SW + tx;                              // the window's top-left tap
    const int n = 2 * r + 1;
    const uint32_t c = win[r * SW + r].y;

    // One sweep of the window: f(key, joint word) for every tap.  A row goes UN taps at a time, their reads in flight
    // together; the last group of a row (2r + 1 is odd) reads up to UN - 1 entries past the row's end -- inside the tile or
    // its pad -- and turns their keys into MARK.
    auto group = [&](const uint2* p, auto last, int left, auto&& f) {
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const uint2 e = p[u];
            f(decltype(last)::value && u >= left ? MARK : e.x, e.y);
        }
    };
    auto sweep = [&](auto&& f) {
#pragma unroll 1
        for (int dy = 0; dy < n; dy++) {
            const uint2* row = win + dy * SW;
            int dx = 0;
#pragma unroll 1
            for (; dx + UN <= n; dx += UN) group(row + dx, std::false_type{}, UN, f);
            group(row + dx, std::true_type{}, n - dx, f);
        }
    };
    uint32_t tot = 0, lo = MARK, hi = 0;
    sweep([&](uint32_t k, uint32_t q) {
        const bool used = k != MARK;
        tot += weight<CH>(used, q, c, lds_t, a.table);
        lo = min(lo, k);
        hi = max(hi, used ? k : 0u);
    });
    RAW* out = reinterpret_cast<RAW*>(static_cast<char*>(a.dst) + m * a.dst_map_stride + (ptrdiff_t)y * a.dst_stride) + x;
    if (tot == 0) {                                                      // nothing to choose from: the pixel as it came
        *out = reinterpret_cast<const RAW*>(src + (ptrdiff_t)y * a.src_stride)[x];
        return;
    }
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t L = 0, below = lo, above = hi;                          // lo <= mid < hi, and both are keys of the window
        sweep([&](uint32_t k, uint32_t q) {
            const bool le = k <= mid;                                    // (never MARK: mid < hi < MARK)
            L += weight<CH>(le, q, c, lds_t, a.table);
            below = max(below, le ? k : 0u);
            above = min(above, le ? MARK : k);
        });
        if (2u * L >= tot) hi = below; else lo = above;
    }
    *out = D::value(lo);
}

struct WmfCall {                       // one call as its C entry point received it
    FilterImages im;                   // guide = the joint; one depth for src and dst
    int r; double sigma; int weight_type;
    int use_ignore; double ignore_value;
};

constexpr const char* WHO = "weightedMedianFilter";

int wmf_check(const WmfCall& c)
{
    const FilterImages& im = c.im;
    if (!im.guide.p || !im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: joint, src and dst must be non-NULL", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(im.src_depth))
        return fail(ADF_EBADARG, "%s: src must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (im.guide_channels != 1 && im.guide_channels != 3) return fail(ADF_EBADARG, "%s: joint must have 1 or 3 channels", WHO);
    if (int rc = wmf_weights_check(WHO, c.sigma, c.weight_type)) return rc;
    if (c.r < 1 || c.r > ADF_WMF_MAX_RADIUS) return fail(ADF_EBADARG, "%s: r must lie in [1, %d]", WHO, ADF_WMF_MAX_RADIUS);
    if (c.use_ignore && im.src_depth != ADF_32F) {
        const double lim_lo = im.src_depth == ADF_8U ? 0.0 : -32768.0, lim_hi = im.src_depth == ADF_8U ? 255.0 : 32767.0;
        if (!(c.ignore_value >= lim_lo && c.ignore_value <= lim_hi) || c.ignore_value != std::nearbyint(c.ignore_value))
            return fail(ADF_EBADARG, "%s: ignore_value must be an integer inside the range of src's depth", WHO);
    }
    return filter_geometry_check(WHO, im, "the depth", "src, joint or mask");
}

template <class T, int CH>
int wmf_launch(const WmfCall& c, const WmfArgs& a, hipStream_t st)
{
    return launch_tiles(wmf_kernel<T, CH>, tile_entries(c.r) * sizeof(uint2), c.im.W, c.im.H, TW, TH, c.im.n, a, st, [&](WmfArgs& t, int m0) {
        t.joint = c.im.guide.map(m0); t.src = c.im.src.map(m0); t.dst = c.im.dst.map(m0);
        t.mask = c.im.mask.p ? c.im.mask.map(m0) : nullptr;
    });
}

int wmf_run(const WmfCall& c, hipStream_t st)
{
    const FilterImages& im = c.im;
    std::shared_ptr<WmfTable> table;                                     // held until the launches are queued
    WmfArgs a{};
    if (int rc = wmf_table_device(c.sigma, c.weight_type, table, &a.table)) return rc;
    a.joint_stride = im.guide.stride; a.joint_map_stride = im.guide.map_stride;
    a.src_stride = im.src.stride; a.src_map_stride = im.src.map_stride;
    a.dst_stride = im.dst.stride; a.dst_map_stride = im.dst.map_stride;
    a.mask_stride = im.mask.stride; a.mask_map_stride = im.mask.map_stride;
    a.W = im.W; a.H = im.H; a.r = c.r;
    a.use_ignore = c.use_ignore != 0;
    if (im.src_depth == ADF_32F) {
        // src is compared with ignore_value as doubles: a value no float has (NaN included) ignores nothing
        const float f = (float)c.ignore_value;
        if (a.use_ignore && !((double)f == c.ignore_value)) a.use_ignore = 0;
        memcpy(&a.ignore, &f, sizeof(f));
    } else {
        a.ignore = a.use_ignore ? (uint32_t)(int)c.ignore_value : 0u;
    }
    const bool ch3 = im.guide_channels == 3;
    switch (im.src_depth) {
    case ADF_8U: return ch3 ? wmf_launch<uint8_t, 3>(c, a, st) : wmf_launch<uint8_t, 1>(c, a, st);
    case ADF_16S: return ch3 ? wmf_launch<int16_t, 3>(c, a, st) : wmf_launch<int16_t, 1>(c, a, st);
    default: return ch3 ? wmf_launch<float, 3>(c, a, st) : wmf_launch<float, 1>(c, a, st);
    }
}

WmfCall call_of(int n_maps, const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int depth, void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                int W, int H, int r, double sigma, int weight_type, const uint8_t* mask, ptrdiff_t mask_stride, ptrdiff_t mask_map_stride,
                int use_ignore, double ignore_value)
{
    return WmfCall{{n_maps, W, H, image_of(joint, joint_stride, joint_map_stride), joint_channels, image_of(src, src_stride, src_map_stride), depth,
                    image_of(dst, dst_stride, dst_map_stride), depth, image_of(mask, mask_stride, mask_map_stride)},
                   r, sigma, weight_type, use_ignore, ignore_value};
}

} // namespace

extern "C" int adf_weighted_median_filter_device(int n_maps,
                                                 const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                                 const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int depth,
                                                 void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                                 int W, int H, int r, double sigma, int weight_type,
                                                 const uint8_t* mask, ptrdiff_t mask_stride, ptrdiff_t mask_map_stride,
                                                 int use_ignore, double ignore_value, void* stream)
{
    const WmfCall c = call_of(n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, depth,
                              dst, dst_stride, dst_map_stride, W, H, r, sigma, weight_type, mask, mask_stride, mask_map_stride,
                              use_ignore, ignore_value);
    int rc = wmf_check(c);
    return rc ? rc : wmf_run(c, (hipStream_t)stream);
}

extern "C" int adf_weighted_median_filter_host(int n_maps,
                                               const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int depth,
                                               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                               int W, int H, int r, double sigma, int weight_type,
                                               const uint8_t* mask, ptrdiff_t mask_stride, ptrdiff_t mask_map_stride,
                                               int use_ignore, double ignore_value)
{
    const WmfCall c = call_of(n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, depth,
                              dst, dst_stride, dst_map_stride, W, H, r, sigma, weight_type, mask, mask_stride, mask_map_stride,
                              use_ignore, ignore_value);
    int rc = wmf_check(c);
    return rc ? rc : staged_call(c.im, 0, [&](const FilterImages& staged, void*, hipStream_t st) {
        WmfCall d = c;                                                   // the same call on the staged images
        d.im = staged;
        return wmf_run(d, st);
    });
}
