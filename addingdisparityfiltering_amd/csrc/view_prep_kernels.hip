// view_prep_kernels.hip -- the two imgproc calls in front of the matcher in the sample's default pipeline
// (samples/disparity_filtering.cpp:130-141), on the device, for batches of equally sized 8-bit images:
//
//     resize(view, view_for_matcher, Size(), 0.5, 0.5);           // both views, colour
//     cvtColor(view_for_matcher, view_for_matcher, COLOR_BGR2GRAY);   // StereoBM only
//
//   case            CH_IN -> CH_OUT  HALF   stands for
//   shrink colour     3  ->  3       yes    resize(.., 0.5, 0.5) (the sample gives StereoSGBM colour views)
//   shrink gray       1  ->  1       yes    the same on CV_8UC1
//   gray              3  ->  1       no     cvtColor(COLOR_BGR2GRAY) (the --no-downscale StereoBM run)
//   shrink + gray     3  ->  1       yes    both calls in one sweep; the half-size colour image is never written
//
// Arithmetic, all integer (bit-exact; the fused case equals the two-step case):
//   half size   destination (cvRound(W/2), cvRound(H/2)), half to even.  cv::resize(INTER_LINEAR) at a scale of exactly 2
//               in both directions is the 2x2 mean (a + b + c + d + 2) >> 2 per channel.  A last column / row with one
//               source column / row (W or H = 3 mod 4) is the mean over the source pixels that exist,
//               cvRound((float)sum / count), half to even.  imgproc is outside the reference tree: the even-size case
//               rests on the tutorial's published images (tests/test_tutorial_replay.py), the odd tail is PARITY UNPINNED.
//   gray        (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 on the 8-bit channels (already rounded in the fused case).
//
// Shape: pure streaming, no reuse beyond the 2x2 cell, no LDS.  A lane owns RUN consecutive destination pixels of one row
// whose source bytes are one contiguous span per source row, a multiple of 16 bytes (48 or 16): it loads the span(s)
// with dwordx4 loads, works in registers, and stores 8, 16 or 24 bytes.  That needs 16-byte aligned source rows and 8-
// or 16-byte aligned destination rows (the launcher checks base pointers and strides on the host); images that are not,
// the last partial run of a row and partial cells take the byte path of the same kernel, one byte per access.
#include "adf_host.h"

using namespace adf;

namespace {

constexpr int NT = 256;
constexpr int MAX_DIM = 1 << 24;       // W, H limit: byte offsets inside a row and run counts stay far inside int32

struct ViewPrepArgs {
    const uint8_t* src; ptrdiff_t sstride, simage;   // bytes
    uint8_t* dst; ptrdiff_t dstride, dimage;
    int W, H, dW, dH;
    int runs;        // runs of RUN destination pixels per destination row (the last one may be short)
    int total;       // runs * dH
    int vec;         // rows and images are aligned for the vector path
};

template <int CH_IN, int CH_OUT, bool HALF> struct Shape {
    static constexpr int RUN = HALF ? 8 : 16;                 // destination pixels per lane
    static constexpr int SRC_BYTES = (HALF ? 2 : 1) * RUN * CH_IN;   // per source row: 48 or 16
    static constexpr int DST_BYTES = RUN * CH_OUT;            // 24, 8 or 16
    static constexpr int DST_ALIGN = DST_BYTES % 16 == 0 ? 16 : 8;
    static_assert(SRC_BYTES % 16 == 0 && DST_BYTES % 8 == 0, "whole vector accesses");
};

__device__ __forceinline__ uint32_t gray14(uint32_t b, uint32_t g, uint32_t r)
{
    return (__umul24(b, 1868u) + __umul24(g, 9617u) + __umul24(r, 4899u) + 8192u) >> 14;   // 8-bit operands
}

// mean over the n = 4, 2 or 1 source pixels of a cell: (s + 2) >> 2 for a whole cell, cvRound(s / 2.0f) (half to even) for
// a half one
__device__ __forceinline__ uint32_t cell_mean(uint32_t s, int n)
{
    if (n == 4) return (s + 2u) >> 2;
    if (n == 2) return (s >> 1) + (s & (s >> 1) & 1u);
    return s;
}

// byte i of a span held in dwords (i is a compile-time constant after unrolling)
__device__ __forceinline__ uint32_t byte_at(const uint32_t* w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

template <int N16> __device__ __forceinline__ void load_span(uint32_t* w, const uint8_t* p)
{
#pragma unroll
    for (int k = 0; k < N16; k++) {
        const uint4 v = reinterpret_cast<const uint4*>(p)[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
}

template <int CH_IN, int CH_OUT, bool HALF>
__global__ void __launch_bounds__(NT) view_prep_kernel(ViewPrepArgs a)
{
    using S = Shape<CH_IN, CH_OUT, HALF>;
    const int idx = (int)(blockIdx.x * NT + threadIdx.x);
    if (idx >= a.total) return;
    const int y = (int)((unsigned)idx / (unsigned)a.runs), x0 = (idx - y * a.runs) * S::RUN;
    const int sy = HALF ? 2 * y : y;
    const uint8_t* s0 = a.src + (ptrdiff_t)blockIdx.y * a.simage + (ptrdiff_t)sy * a.sstride;
    const bool two_rows = HALF && sy + 1 < a.H;
    const uint8_t* s1 = two_rows ? s0 + a.sstride : s0;              // (never read past the last row)
    uint8_t* d = a.dst + (ptrdiff_t)blockIdx.y * a.dimage + (ptrdiff_t)y * a.dstride;
    // destination pixels [0, whole) of this row have a whole cell
    const int whole = HALF ? (two_rows ? min(a.dW, a.W >> 1) : 0) : a.dW;

    if (a.vec && x0 + S::RUN <= whole) {
        uint32_t r0[S::SRC_BYTES / 4], r1[S::SRC_BYTES / 4], out[S::DST_BYTES / 4];
        const ptrdiff_t soff = (ptrdiff_t)x0 * (HALF ? 2 : 1) * CH_IN;
        load_span<S::SRC_BYTES / 16>(r0, s0 + soff);
        if (HALF) load_span<S::SRC_BYTES / 16>(r1, s1 + soff);
#pragma unroll
        for (int k = 0; k < S::DST_BYTES / 4; k++) out[k] = 0;
#pragma unroll
        for (int p = 0; p < S::RUN; p++) {
            uint32_t c[CH_IN];
#pragma unroll
            for (int k = 0; k < CH_IN; k++) {
                if (HALF) {
                    const int i = 2 * p * CH_IN + k;
                    c[k] = (byte_at(r0, i) + byte_at(r0, i + CH_IN) + byte_at(r1, i) + byte_at(r1, i + CH_IN) + 2u) >> 2;
                } else {
                    c[k] = byte_at(r0, p * CH_IN + k);
                }
            }
            if (CH_IN == 3 && CH_OUT == 1) {
                out[p >> 2] |= gray14(c[0], c[1], c[CH_IN - 1]) << ((p & 3) * 8);
            } else {
#pragma unroll
                for (int k = 0; k < CH_OUT; k++) {
                    const int j = p * CH_OUT + k;
                    out[j >> 2] |= c[k] << ((j & 3) * 8);
                }
            }
        }
        uint8_t* dp = d + (ptrdiff_t)x0 * CH_OUT;
        if (S::DST_ALIGN == 16) {
            *reinterpret_cast<uint4*>(dp) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int k = 0; k < S::DST_BYTES / 8; k++)
                reinterpret_cast<uint2*>(dp)[k] = make_uint2(out[2 * k], out[2 * k + 1]);
        }
        return;
    }

    // byte path: misaligned images, the last run of a row, partial cells
    const int x1 = min(x0 + S::RUN, a.dW);
    for (int x = x0; x < x1; x++) {
        uint32_t c[CH_IN];
        if (HALF) {
            const int nx = min(2, a.W - 2 * x), n = nx * (two_rows ? 2 : 1);
            const uint8_t* p0 = s0 + (ptrdiff_t)(2 * x) * CH_IN;
            const uint8_t* p1 = s1 + (ptrdiff_t)(2 * x) * CH_IN;
#pragma unroll
            for (int k = 0; k < CH_IN; k++) {
                uint32_t s = p0[k];
                if (nx == 2) s += p0[k + CH_IN];
                if (two_rows) {
                    s += p1[k];
                    if (nx == 2) s += p1[k + CH_IN];
                }
                c[k] = cell_mean(s, n);
            }
        } else {
#pragma unroll
            for (int k = 0; k < CH_IN; k++) c[k] = s0[(ptrdiff_t)x * CH_IN + k];
        }
        if (CH_IN == 3 && CH_OUT == 1) {
            d[x] = (uint8_t)gray14(c[0], c[1], c[CH_IN - 1]);
        } else {
#pragma unroll
            for (int k = 0; k < CH_OUT; k++) d[(ptrdiff_t)x * CH_OUT + k] = (uint8_t)c[k];
        }
    }
}

const char* const SUPPORTED =
    "prepare_views supports CV_8UC3 -> CV_8UC3 and CV_8UC1 -> CV_8UC1 at half size, CV_8UC3 -> CV_8UC1 at full or half "
    "size (half size = adf_half_size of the width and of the height)";

int half_of(int n) { return (n >> 1) + (n & (n >> 1) & 1); }     // cvRound(n * 0.5), half to even, n >= 0

// One call as its C entry point received it; `half` (the call shrinks) is view_prep_check's.
struct ViewPrepCall {
    int n; const uint8_t* src; ptrdiff_t sstride, simage; int W, H, sc;
    uint8_t* dst; ptrdiff_t dstride, dimage; int dW, dH, dc;
    bool half;
};

// Everything that can be refused without a device.
int view_prep_check(ViewPrepCall& c)
{
    if (c.n < 1) return fail(ADF_EBADARG, "prepare_views: n_images must be at least 1");
    if (!c.src || !c.dst) return fail(ADF_EBADARG, "prepare_views: src and dst must not be null");
    if (c.W < 1 || c.H < 1 || c.dW < 1 || c.dH < 1) return fail(ADF_EBADARG, "prepare_views: the source or the destination image is empty");
    if (!((c.sc == 3 && (c.dc == 3 || c.dc == 1)) || (c.sc == 1 && c.dc == 1))) return fail(ADF_EBADARG, "%s", SUPPORTED);
    if (c.dW == c.W && c.dH == c.H) c.half = false;
    else if (c.dW == half_of(c.W) && c.dH == half_of(c.H)) c.half = true;
    else return fail(ADF_EBADARG, "%s", SUPPORTED);
    if (!c.half && c.sc == c.dc) return fail(ADF_EBADARG, "%s", SUPPORTED);       // nothing to do is not a case either
    if (c.W > MAX_DIM || c.H > MAX_DIM) return fail(ADF_ESIZE, "prepare_views: W and H must not exceed 2^24");
    if (c.sstride < (ptrdiff_t)c.W * c.sc || c.dstride < (ptrdiff_t)c.dW * c.dc)
        return fail(ADF_EBADARG, "prepare_views: row stride smaller than a row");
    if (c.n > 1 && c.simage < 0) return fail(ADF_EBADARG, "prepare_views: negative image stride");
    if (!images_disjoint(c.n, (ptrdiff_t)c.dW * c.dc, c.dH, c.dstride, c.dimage, true))
        return fail(ADF_EBADARG, "prepare_views: destination images overlap");
    return ADF_OK;
}

template <int CH_IN, int CH_OUT, bool HALF>
int view_prep_launch(const ViewPrepCall& c, hipStream_t st)
{
    using S = Shape<CH_IN, CH_OUT, HALF>;
    ViewPrepArgs a;
    a.sstride = c.sstride; a.simage = c.n > 1 ? c.simage : 0;
    a.dstride = c.dstride; a.dimage = c.n > 1 ? c.dimage : 0;
    a.W = c.W; a.H = c.H; a.dW = c.dW; a.dH = c.dH;
    a.runs = (a.dW + S::RUN - 1) / S::RUN;
    if ((int64_t)a.runs * a.dH >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "prepare_views: image too large");
    a.total = a.runs * a.dH;
    const uintptr_t smis = (uintptr_t)c.src | (uintptr_t)a.sstride | (uintptr_t)a.simage;
    const uintptr_t dmis = (uintptr_t)c.dst | (uintptr_t)a.dstride | (uintptr_t)a.dimage;
    a.vec = (smis & 15) == 0 && (dmis & (S::DST_ALIGN - 1)) == 0;
    return for_batches(c.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.src = c.src + (ptrdiff_t)m0 * a.simage;
        a.dst = c.dst + (ptrdiff_t)m0 * a.dimage;
        hipLaunchKernelGGL((view_prep_kernel<CH_IN, CH_OUT, HALF>), dim3((unsigned)((a.total + NT - 1) / NT), nm), dim3(NT), 0, st, a);
        return launched();
    });
}

int view_prep_run(const ViewPrepCall& c, hipStream_t st)
{
    if (c.sc == 3 && c.dc == 3) return view_prep_launch<3, 3, true>(c, st);
    if (c.sc == 1) return view_prep_launch<1, 1, true>(c, st);
    return c.half ? view_prep_launch<3, 1, true>(c, st) : view_prep_launch<3, 1, false>(c, st);
}

} // namespace

extern "C" int adf_half_size(int n, int* half)
{
    if (n < 0 || !half) return fail(ADF_EBADARG, "adf_half_size: n must not be negative and half must not be null");
    *half = half_of(n);
    return ADF_OK;
}

extern "C" int adf_prepare_views_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                                        int W, int H, int src_channels,
                                        uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride,
                                        int dst_W, int dst_H, int dst_channels, void* stream)
{
    ViewPrepCall c{n_images, src, src_stride, src_image_stride, W, H, src_channels,
                   dst, dst_stride, dst_image_stride, dst_W, dst_H, dst_channels, false};
    const int rc = view_prep_check(c);
    return rc ? rc : view_prep_run(c, (hipStream_t)stream);
}

extern "C" int adf_prepare_views_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                                      int W, int H, int src_channels,
                                      uint8_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride,
                                      int dst_W, int dst_H, int dst_channels)
{
    ViewPrepCall c{n_images, src, src_stride, src_image_stride, W, H, src_channels,
                   dst, dst_stride, dst_image_stride, dst_W, dst_H, dst_channels, false};
    int rc = view_prep_check(c);
    if (rc) return rc;
    // one block: the source images, then the destination images, rows and images padded to 16 bytes (the vector path)
    const size_t srow = (size_t)W * src_channels, drow = (size_t)dst_W * dst_channels;
    const size_t sp = pad_to(srow, 16), dp = pad_to(drow, 16);
    const size_t simg = sp * H, dimg = dp * dst_H, need = (simg + dimg) * (size_t)n_images;
    Scratch blk;
    if ((rc = blk.take(need, nullptr))) return rc;
    uint8_t* ds = static_cast<uint8_t*>(blk.p);
    uint8_t* dd = ds + simg * n_images;
    ViewPrepCall d = c;                                              // the same call on the staged copies
    d.src = ds; d.sstride = (ptrdiff_t)sp; d.simage = (ptrdiff_t)simg;
    d.dst = dd; d.dstride = (ptrdiff_t)dp; d.dimage = (ptrdiff_t)dimg;
    if ((rc = copy_images(ds, sp, simg, src, src_stride, src_image_stride, srow, H, n_images, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = view_prep_run(d, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(dst, dst_stride, dst_image_stride, dd, dp, dimg, drow, dst_H, n_images, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
