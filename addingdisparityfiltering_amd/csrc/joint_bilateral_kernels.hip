// joint_bilateral_kernels.hip -- cv::ximgproc::jointBilateralFilter(joint, src, dst, d, sigmaColor, sigmaSpace, borderType)
// on the device, in the library's own definition (include/adf_wls.h, "joint bilateral filter", is the statement;
// tests/jbf_ref.py states it in NumPy):
//
//   taps     (i, j), -r <= i, j <= r, i*i + j*j <= r*r, rows outer, columns inner; outside the image: borderInterpolate
//   w(p, q)  = S[i*i + j*j] * C[ sum_c |joint_c(p) - joint_c(q)| ]             float32, both tables built on the host
//   dst(p)   = (sum of w * (float)src(q)) / (sum of w), both sums ONE float32 chain in the taps' order, no FMA
//
// The kernel is bilateral_tile.h's, which both bilateral filters share; here are its two policies (a joint of 1 and of 3
// channels), the checks and the launches.  C sits in LDS in front of the tile (1 KiB for a 1-channel joint, 3 KiB for 3
// channels).  Per tap the range weight is the L1 difference (1 channel: the joint word is 4 * joint, so |q - c| is the
// byte offset into C; 3 channels: v_sad_u8 of the packed bytes) and one 4-byte gather from C -- the one access whose
// bank conflicts depend on the data.
//
// LDS: 255 ch + 1 floats + (TW + 2r)(TH + 2r) entries of 8 B: 4.4 KiB at r = 2 (1 channel), 54.4 KiB at r = 31 (3
// channels) -- two workgroups per CU of 160 KiB.  Times and what bounds them: DESIGN.md, section 23.
#include "adf_host.h"
#include "bilateral_tile.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace adf;
using namespace adf::bilateral;

namespace {

static_assert(lds_bytes(ADF_JBF_MAX_RADIUS, jbf_colour_entries(3)) <= 64 * 1024, "two workgroups per CU at the largest radius");

// The tile kernel's policy for a joint of CH 8-bit channels: the whole of C in LDS.
template <int CH> struct Jbf {
    static __device__ __forceinline__ int source_depth(const TileArgs& a) { return a.src_depth; }
    static __device__ __forceinline__ int table_entries(const TileArgs&) { return (int)jbf_colour_entries(CH); }
    static __device__ __forceinline__ uint32_t joint_word(const TileArgs& a, ptrdiff_t m, int x, int y, uint32_t)
    {
        const uint8_t* j = static_cast<const uint8_t*>(a.joint) + m * a.joint_map_stride + (ptrdiff_t)y * a.joint_stride + (ptrdiff_t)x * CH;
        return CH == 1 ? 4u * j[0] : (uint32_t)j[0] | ((uint32_t)j[1] << 8) | ((uint32_t)j[2] << 16);
    }
    // S * C[sum_c |joint_c(p) - joint_c(q)|], tap by tap: the words' L1 difference is the byte offset into C
    template <int N> static __device__ __forceinline__ void weights(const TileArgs&, const float* lds_c, const float* s_row, int j, const uint64_t (&e)[N], uint32_t c, float (&w)[N])
    {
#pragma unroll
        for (int u = 0; u < N; u++) {
            const uint32_t q = (uint32_t)(e[u] >> 32);
            w[u] = s_row[(j + u) * (j + u)] * *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lds_c) + (CH == 1 ? __usad(q, c, 0u) : 4u * __builtin_amdgcn_sad_u8(q, c, 0u)));
        }
    }
};

struct JbfCall {                       // one call as its C entry point received it
    int n;
    const uint8_t* joint; ptrdiff_t joint_stride, joint_map_stride; int joint_channels;
    const void* src; ptrdiff_t src_stride, src_map_stride; int src_depth;
    void* dst; ptrdiff_t dst_stride, dst_map_stride; int dst_depth;
    int W, H, d; double sigma_color, sigma_space; int border;
    double sc, ss; int r;              // the clamped sigmas and the radius (jbf_check)
};

constexpr const char* WHO = "jointBilateralFilter";

int jbf_check(JbfCall& c)
{
    if (!c.joint || !c.src || !c.dst) return fail(ADF_EBADARG, "%s: joint, src and dst must be non-NULL (an empty joint is cv::bilateralFilter, which is not built)", WHO);
    if (static_cast<const void*>(c.joint) == c.src) return fail(ADF_EBADARG, "%s: joint == src is cv::bilateralFilter, which is not built", WHO);
    if (c.n < 1 || c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(c.src_depth) || !known_depth(c.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (int rc = jbf_params_check(WHO, c.d, c.sigma_color, c.sigma_space, c.joint_channels, &c.sc, &c.ss, &c.r)) return rc;
    if (int rc = border_check(WHO, c.border)) return rc;
    const ptrdiff_t ss = (ptrdiff_t)depth_size(c.src_depth), ds = (ptrdiff_t)depth_size(c.dst_depth);
    if (!aligned(c.src, c.src_stride, c.src_map_stride, ss) || !aligned(c.dst, c.dst_stride, c.dst_map_stride, ds))
        return fail(ADF_EBADARG, "%s: src and dst and their strides must be aligned to their depths", WHO);
    if ((int64_t)c.W * c.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "%s: W*H must be below 2^31", WHO);
    const ptrdiff_t srow = (ptrdiff_t)c.W * ss, drow = (ptrdiff_t)c.W * ds, jrow = (ptrdiff_t)c.W * c.joint_channels;
    if (c.src_stride < srow || c.dst_stride < drow || c.joint_stride < jrow)
        return fail(ADF_ESIZE, "%s: row stride smaller than a row", WHO);
    if (c.n > 1 && (c.src_map_stride < 0 || c.joint_map_stride < 0))
        return fail(ADF_ESIZE, "%s: map strides must not be negative", WHO);
    if (!images_disjoint(c.n, drow, c.H, c.dst_stride, c.dst_map_stride, false))
        return fail(ADF_ESIZE, "%s: destination maps of the batch overlap (map stride smaller than a map)", WHO);
    const Span d = span_of(c.dst, c.n, drow, c.H, c.dst_stride, c.dst_map_stride);
    if (overlap(d, span_of(c.src, c.n, srow, c.H, c.src_stride, c.src_map_stride)) ||
        overlap(d, span_of(c.joint, c.n, jrow, c.H, c.joint_stride, c.joint_map_stride)))
        return fail(ADF_EBADARG, "%s: dst must not overlap src or joint", WHO);
    return ADF_OK;
}

int jbf_run(const JbfCall& c, hipStream_t st)
{
    std::shared_ptr<JbfTable> table;                                     // held until the launches are queued
    TileArgs a{};
    if (int rc = jbf_table_device(c.sc, c.ss, c.r, c.joint_channels, table, &a.colour, &a.space)) return rc;
    a.joint_stride = c.joint_stride; a.joint_map_stride = c.joint_map_stride;
    a.src_stride = c.src_stride; a.src_map_stride = c.src_map_stride;
    a.dst_stride = c.dst_stride; a.dst_map_stride = c.dst_map_stride;
    a.W = c.W; a.H = c.H; a.r = c.r; a.border = c.border; a.src_depth = c.src_depth; a.dst_depth = c.dst_depth;
    a.entry_bytes = 8;
    const bool ch3 = c.joint_channels == 3;
    return launch_tiles(ch3 ? bilateral_tile_kernel<Jbf<3>> : bilateral_tile_kernel<Jbf<1>>, lds_bytes(c.r, jbf_colour_entries(c.joint_channels)),
                        c.W, c.H, TW, TH, c.n, a, st, [&](TileArgs& t, int m0) {
                            t.joint = c.joint + (ptrdiff_t)m0 * c.joint_map_stride;
                            t.src = static_cast<const char*>(c.src) + (ptrdiff_t)m0 * c.src_map_stride;
                            t.dst = static_cast<char*>(c.dst) + (ptrdiff_t)m0 * c.dst_map_stride;
                        });
}

} // namespace

extern "C" int adf_joint_bilateral_filter_device(int n_maps,
                                                 const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                                 const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                                 void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                                 int W, int H, int d, double sigma_color, double sigma_space, int border_type,
                                                 void* stream)
{
    JbfCall c{n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, src_depth,
              dst, dst_stride, dst_map_stride, dst_depth, W, H, d, sigma_color, sigma_space, border_type, 0.0, 0.0, 0};
    int rc = jbf_check(c);
    return rc ? rc : jbf_run(c, (hipStream_t)stream);
}

extern "C" int adf_joint_bilateral_filter_host(int n_maps,
                                               const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                               int W, int H, int d, double sigma_color, double sigma_space, int border_type)
{
    JbfCall c{n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, src_depth,
              dst, dst_stride, dst_map_stride, dst_depth, W, H, d, sigma_color, sigma_space, border_type, 0.0, 0.0, 0};
    int rc = jbf_check(c);
    if (rc) return rc;
    // one block: the joint images, dense, then the sources and the results
    const size_t jrow = (size_t)W * joint_channels, jmap = (size_t)H * jrow, joints = pad_to(jmap * n_maps, 256);
    const size_t srow = (size_t)W * depth_size(src_depth), smap = (size_t)H * srow, srcs = pad_to(smap * n_maps, 256);
    const size_t drow = (size_t)W * depth_size(dst_depth), dmap = (size_t)H * drow, dsts = pad_to(dmap * n_maps, 256);
    Scratch blk;
    if ((rc = blk.take(joints + srcs + dsts, nullptr))) return rc;
    char* base = static_cast<char*>(blk.p);
    JbfCall s = c;                                                       // the same call on the staged images
    s.joint = reinterpret_cast<uint8_t*>(base); s.joint_stride = (ptrdiff_t)jrow; s.joint_map_stride = (ptrdiff_t)jmap;
    s.src = base + joints; s.src_stride = (ptrdiff_t)srow; s.src_map_stride = (ptrdiff_t)smap;
    s.dst = base + joints + srcs; s.dst_stride = (ptrdiff_t)drow; s.dst_map_stride = (ptrdiff_t)dmap;
    if ((rc = copy_images(base, jrow, jmap, joint, joint_stride, joint_map_stride, jrow, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = copy_images(base + joints, srow, smap, src, src_stride, src_map_stride, srow, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = jbf_run(s, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(dst, dst_stride, dst_map_stride, base + joints + srcs, drow, dmap, drow, H, n_maps, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
