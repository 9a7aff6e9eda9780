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
    FilterImages im;                   // guide = the joint
    int d; double sigma_color, sigma_space; int border;
    double sc, ss; int r;              // the clamped sigmas and the radius (jbf_check)
};

constexpr const char* WHO = "jointBilateralFilter";

int jbf_check(JbfCall& c)
{
    const FilterImages& im = c.im;
    if (!im.guide.p || !im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: joint, src and dst must be non-NULL (an empty joint is cv::bilateralFilter, which is not built)", WHO);
    if (im.guide.p == im.src.p) return fail(ADF_EBADARG, "%s: joint == src is cv::bilateralFilter, which is not built", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(im.src_depth) || !known_depth(im.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (int rc = jbf_params_check(WHO, c.d, c.sigma_color, c.sigma_space, im.guide_channels, &c.sc, &c.ss, &c.r)) return rc;
    if (int rc = border_check(WHO, c.border)) return rc;
    return filter_geometry_check(WHO, im, "their depths", "src or joint");
}

int jbf_run(const JbfCall& c, hipStream_t st)
{
    const FilterImages& im = c.im;
    std::shared_ptr<JbfTable> table;                                     // held until the launches are queued
    TileArgs a{};
    if (int rc = jbf_table_device(c.sc, c.ss, c.r, im.guide_channels, table, &a.colour, &a.space)) return rc;
    a.joint_stride = im.guide.stride; a.joint_map_stride = im.guide.map_stride;
    a.src_stride = im.src.stride; a.src_map_stride = im.src.map_stride;
    a.dst_stride = im.dst.stride; a.dst_map_stride = im.dst.map_stride;
    a.W = im.W; a.H = im.H; a.r = c.r; a.border = c.border; a.src_depth = im.src_depth; a.dst_depth = im.dst_depth;
    a.entry_bytes = 8;
    const bool ch3 = im.guide_channels == 3;
    return launch_tiles(ch3 ? bilateral_tile_kernel<Jbf<3>> : bilateral_tile_kernel<Jbf<1>>, lds_bytes(c.r, jbf_colour_entries(im.guide_channels)),
                        im.W, im.H, TW, TH, im.n, a, st,
                        [&](TileArgs& t, int m0) { t.joint = im.guide.map(m0); t.src = im.src.map(m0); t.dst = im.dst.map(m0); });
}

JbfCall call_of(int n_maps, const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                int W, int H, int d, double sigma_color, double sigma_space, int border_type)
{
    return JbfCall{{n_maps, W, H, image_of(joint, joint_stride, joint_map_stride), joint_channels, image_of(src, src_stride, src_map_stride), src_depth,
                    image_of(dst, dst_stride, dst_map_stride), dst_depth, {}}, d, sigma_color, sigma_space, border_type, 0.0, 0.0, 0};
}

} // namespace

extern "C" int adf_joint_bilateral_filter_device(int n_maps,
                                                 const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                                 const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                                 void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                                 int W, int H, int d, double sigma_color, double sigma_space, int border_type,
                                                 void* stream)
{
    JbfCall c = call_of(n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, src_depth,
                        dst, dst_stride, dst_map_stride, dst_depth, W, H, d, sigma_color, sigma_space, border_type);
    int rc = jbf_check(c);
    return rc ? rc : jbf_run(c, (hipStream_t)stream);
}

extern "C" int adf_joint_bilateral_filter_host(int n_maps,
                                               const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                               int W, int H, int d, double sigma_color, double sigma_space, int border_type)
{
    JbfCall c = call_of(n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, src_depth,
                        dst, dst_stride, dst_map_stride, dst_depth, W, H, d, sigma_color, sigma_space, border_type);
    int rc = jbf_check(c);
    return rc ? rc : staged_call(c.im, 0, [&](const FilterImages& staged, void*, hipStream_t st) {
        JbfCall s = c;                                                   // the same call on the staged images
        s.im = staged;
        return jbf_run(s, st);
    });
}
