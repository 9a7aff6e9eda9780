// rolling_guidance_kernels.hip -- cv::ximgproc::rollingGuidanceFilter(src, dst, d, sigmaColor, sigmaSpace, numOfIter,
// borderType) on the device, in the library's own definition (include/adf_wls.h, "rolling guidance filter", is the
// statement; tests/rgf_ref.py states it in NumPy):
//
//   J_0 = src;  J_{k+1} = the joint bilateral filter of src with joint J_k, stored in the source's depth;  dst = J_num_iter
//   taps     as the joint bilateral filter's: the disc of radius r, rows outer, columns inner, borderInterpolate outside
//   w(p, q)  = S[i*i + j*j] * Wc(J_k(p), J_k(q))                                float32
//   Wc       integer depths: C[min(|J(p) - J(q)|, T - 1)], C cut after its first zero entry (T <= 256 or 65536)
//            ADF_32F: a = min(|J(p) - J(q)| * scale, 4096), G[(int)a] + frac(a) * (G[(int)a + 1] - G[(int)a]), G constant
//   J_{k+1}(p) = (sum of w * (float)src(q)) / (sum of w), both sums ONE float32 chain in the taps' order, no FMA
//
// One launch per iteration (the halo a pixel depends on grows by r with each, so they do not fuse) of bilateral_tile.h's
// kernel, which both bilateral filters share; here are its three policies, the checks and the iterations.  A tile entry
// is {(float)src, the joint word of J_k}; in the first iteration both halves come from one load of src.
//
// The range table, by kernel kind:
//   INT_NEAR  the whole of C is in LDS in front of the tile (T <= LDS_ENTRIES = 1024: every ADF_8U call, ADF_16S up to
//             sigma_color 70 -- the default 25 has T = 362).  The joint word is 4 * (J - the depth's minimum), so the
//             byte offset into C is min(v_sad_u32 of two words, 4 (T - 1)): the joint bilateral filter's tap plus one min.
//   INT_FAR   the first LDS_ENTRIES entries in LDS, the rest read from the device table (up to 256 KiB, which LDS cannot
//             hold): a group of taps in which some lane's difference lies beyond LDS_ENTRIES levels takes a branch with
//             the group's global loads in flight together; a wave whose differences are all near never takes it.
//   FLOAT     G (4098 floats, 16 KiB, the same for every call) in LDS; the joint word is J's bits.  Per tap two reads of
//             G and five float operations (subtract-abs, scale, clamp, the fraction, the interpolation's three) off
//             the accumulation chains.
// LDS at r = 31: 52.6 KiB of tile + 4 KiB (integer) or 16 KiB (float): two workgroups per CU of 160 KiB in every kind.
// Times: DESIGN.md, section 24.
#include "adf_host.h"
#include "bilateral_tile.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace adf;
using namespace adf::bilateral;

namespace {

constexpr int LDS_ENTRIES = 1024;                                        // of an integer depth's C: what LDS holds of it
enum Kind { INT_NEAR, INT_FAR, FLOAT };
static_assert(lds_bytes(ADF_JBF_MAX_RADIUS, RGF_GRID_ENTRIES) <= 80 * 1024, "two workgroups per CU at the largest radius");

// The tile kernel's policy for one kind of range table.  The joint J_k has the source's depth; a null a.joint is J_0 = src.
template <int KIND> struct Rgf {
    static __device__ __forceinline__ int source_depth(const TileArgs& a) { return KIND == FLOAT ? ADF_32F : a.src_depth == ADF_16S ? ADF_16S : ADF_8U; }
    static __device__ __forceinline__ int table_entries(const TileArgs& a) { return a.lds_entries; }
    // a float's bits, or 4 * (J - the depth's minimum).  (The word is formed on either side of the test: with one
    // selected pixel the compiler waits for the source's load before it issues the joint's.)
    static __device__ __forceinline__ uint32_t joint_word(const TileArgs& a, ptrdiff_t m, int x, int y, uint32_t raw)
    {
        const int depth = source_depth(a);
        const auto word = [&](uint32_t pixel) { return KIND == FLOAT ? pixel : 4u * (pixel + (depth == ADF_16S ? 32768u : 0u)); };
        if (!a.joint) return word(raw);
        load_pixel(static_cast<const char*>(a.joint) + m * a.joint_map_stride + (ptrdiff_t)y * a.joint_stride, x, depth, &raw);
        return word(raw);
    }
    // S * Wc: the group's range weights first, then the products
    template <int N> static __device__ __forceinline__ void weights(const TileArgs& a, const float* lds_c, const float* s_row, int j, const uint64_t (&e)[N], uint32_t c, float (&w)[N])
    {
        range_weights<N>(a, lds_c, e, c, w);
#pragma unroll
        for (int u = 0; u < N; u++) w[u] = s_row[(j + u) * (j + u)] * w[u];
    }
    // Wc of N taps whose joint words are the high halves of `e`, for a centre `c` (include/adf_wls.h: "Range weight").
    template <int N> static __device__ __forceinline__ void range_weights(const TileArgs& a, const float* lds_c, const uint64_t (&e)[N], uint32_t c, float (&w)[N])
    {
        if constexpr (KIND == FLOAT) {
#pragma unroll
            for (int u = 0; u < N; u++) {
                float t = fabsf(__uint_as_float(c) - __uint_as_float((uint32_t)(e[u] >> 32))) * a.scale;
                if (!(t < 4096.0f)) t = 4096.0f;                         // (NaN and infinity too: G[4096] = G[4097] = 0)
                const int idx = (int)t;
                const float f = t - (float)idx, g0 = lds_c[idx], g1 = lds_c[idx + 1];
                w[u] = g0 + f * (g1 - g0);
            }
        } else {
            constexpr uint32_t LDS_END = 4u * LDS_ENTRIES;               // byte offsets from here on are not in LDS
            uint32_t off[N];                                             // 4 min(L, T - 1)
            bool far = false;
#pragma unroll
            for (int u = 0; u < N; u++) {
                off[u] = min(__usad((uint32_t)(e[u] >> 32), c, 0u), a.last_offset);
                w[u] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lds_c) + (KIND == INT_FAR ? min(off[u], LDS_END - 4u) : off[u]));
                far = far || off[u] >= LDS_END;
            }
            if constexpr (KIND == INT_FAR) {
                // The LDS values are made opaque first: otherwise the compiler selects between an LDS and a global POINTER
                // per tap and issues one flat load, which counts against both memory counters.
#pragma unroll
                for (int u = 0; u < N; u++) asm("" : "+v"(w[u]));
                if (far) {                                               // lanes with a tap beyond LDS; a wave without one skips this
                    float g[N];                                          // the N loads in flight together; a near tap reads entry 0
#pragma unroll
                    for (int u = 0; u < N; u++) g[u] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.colour) + (off[u] >= LDS_END ? off[u] : 0u));
#pragma unroll
                    for (int u = 0; u < N; u++) w[u] = off[u] >= LDS_END ? g[u] : w[u];
                }
            }
        }
    }
};

struct RgfCall {                       // one call as its C entry point received it
    FilterImages im;                   // no guide; one depth for src and dst
    int d; double sigma_color, sigma_space; int num_iter, border;
    double sc, ss; int r; float scale; // the clamped sigmas, the radius and the float grid's scale (rgf_check)
};

constexpr const char* WHO = "rollingGuidanceFilter";

int rgf_check(RgfCall& c)
{
    const FilterImages& im = c.im;
    if (!im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: src and dst must be non-NULL", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (int rc = rgf_params_check(WHO, im.src_depth, c.d, c.sigma_color, c.sigma_space, &c.sc, &c.ss, &c.r, &c.scale)) return rc;
    if (c.num_iter < 0 || c.num_iter > ADF_RGF_MAX_ITERS)
        return fail(ADF_EBADARG, "%s: numOfIter must lie in [0, %d] (got %d)", WHO, ADF_RGF_MAX_ITERS, c.num_iter);
    if (int rc = border_check(WHO, c.border)) return rc;
    return filter_geometry_check(WHO, im, "the depth", "src (there is no in-place call)");
}

// ws: adf_rolling_guidance_workspace_bytes of device memory, one dense plane of the source's depth per map (unused, and
// may be null, for num_iter <= 1).  Iteration k writes dst when an even number of iterations follow it, else the plane:
// the last one writes dst.
int rgf_run(const RgfCall& c, void* ws, hipStream_t st)
{
    const FilterImages& im = c.im;
    const int depth = im.src_depth;
    const ptrdiff_t row = (ptrdiff_t)im.W * (ptrdiff_t)depth_size(depth), map = row * im.H;
    if (c.num_iter == 0)
        return copy_images(im.dst.p, (size_t)im.dst.stride, im.dst.map_stride, im.src.p, (size_t)im.src.stride, im.src.map_stride, (size_t)row,
                           (size_t)im.H, im.n, hipMemcpyDeviceToDevice, st);
    std::shared_ptr<RgfTable> table;                                     // held until the launches are queued
    TileArgs a{};
    int entries = 0;
    if (int rc = rgf_table_device(depth, c.sc, c.ss, c.r, table, &a.colour, &a.space, &entries)) return rc;
    const Kind kind = depth == ADF_32F ? FLOAT : entries > LDS_ENTRIES ? INT_FAR : INT_NEAR;
    a.lds_entries = kind == FLOAT ? entries : std::min(entries, LDS_ENTRIES);
    a.last_offset = 4u * (unsigned)(entries - 1);
    a.scale = c.scale;
    a.src = im.src.p; a.src_stride = im.src.stride; a.src_map_stride = im.src.map_stride;
    a.W = im.W; a.H = im.H; a.r = c.r; a.border = c.border; a.src_depth = a.dst_depth = depth;
    a.entry_bytes = 8;
    const auto kernel = kind == FLOAT ? bilateral_tile_kernel<Rgf<FLOAT>> : kind == INT_FAR ? bilateral_tile_kernel<Rgf<INT_FAR>> : bilateral_tile_kernel<Rgf<INT_NEAR>>;
    for (int k = 0; k < c.num_iter; k++) {
        if ((c.num_iter - 1 - k) % 2 == 0) { a.dst = im.dst.p; a.dst_stride = im.dst.stride; a.dst_map_stride = im.dst.map_stride; }
        else { a.dst = ws; a.dst_stride = row; a.dst_map_stride = map; }
        const int rc = launch_tiles(kernel, lds_bytes(c.r, (size_t)a.lds_entries), im.W, im.H, TW, TH, im.n, a, st, [&](TileArgs& t, int m0) {
            t.src = static_cast<const char*>(a.src) + (ptrdiff_t)m0 * a.src_map_stride;
            t.joint = a.joint ? static_cast<const char*>(a.joint) + (ptrdiff_t)m0 * a.joint_map_stride : nullptr;
            t.dst = static_cast<char*>(a.dst) + (ptrdiff_t)m0 * a.dst_map_stride;
        });
        if (rc) return rc;
        a.joint = a.dst; a.joint_stride = a.dst_stride; a.joint_map_stride = a.dst_map_stride;   // J_{k+1}
    }
    return ADF_OK;
}

RgfCall call_of(int n_maps, const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, void* dst, ptrdiff_t dst_stride,
                ptrdiff_t dst_map_stride, int depth, int W, int H, int d, double sigma_color, double sigma_space, int num_iter, int border_type)
{
    return RgfCall{{n_maps, W, H, {}, 0, image_of(src, src_stride, src_map_stride), depth, image_of(dst, dst_stride, dst_map_stride), depth, {}},
                   d, sigma_color, sigma_space, num_iter, border_type, 0.0, 0.0, 0, 1.0f};
}

} // namespace

extern "C" size_t adf_rolling_guidance_workspace_bytes(int n_maps, int W, int H, int depth, int num_iter)
{
    if (n_maps < 1 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) return 0;
    if (!known_depth(depth) || num_iter <= 1 || num_iter > ADF_RGF_MAX_ITERS) return 0;
    return (size_t)n_maps * (size_t)W * (size_t)H * depth_size(depth);
}

extern "C" int adf_rolling_guidance_filter_device(int n_maps,
                                                  const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride,
                                                  void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                                  int depth, int W, int H, int d, double sigma_color, double sigma_space, int num_iter,
                                                  int border_type, void* workspace, size_t workspace_bytes, void* stream)
{
    RgfCall c = call_of(n_maps, src, src_stride, src_map_stride, dst, dst_stride, dst_map_stride, depth, W, H, d, sigma_color, sigma_space,
                        num_iter, border_type);
    int rc = rgf_check(c);
    if (rc) return rc;
    const size_t need = adf_rolling_guidance_workspace_bytes(n_maps, W, H, depth, num_iter);
    Scratch blk;
    void* ws = nullptr;
    if (need) {
        const ptrdiff_t row = (ptrdiff_t)W * (ptrdiff_t)depth_size(depth);
        const Span w{reinterpret_cast<uintptr_t>(workspace), reinterpret_cast<uintptr_t>(workspace) + need};
        if (workspace && workspace_bytes >= need &&
            (overlap(w, span_of(src, n_maps, row, H, src_stride, src_map_stride)) || overlap(w, span_of(dst, n_maps, row, H, dst_stride, dst_map_stride))))
            return fail(ADF_EBADARG, "%s: the workspace must not overlap src or dst", WHO);
        if ((rc = workspace_or_scratch(WHO, "adf_rolling_guidance_workspace_bytes", workspace, workspace_bytes, need, (hipStream_t)stream, blk, &ws)))
            return rc;
    }
    return rgf_run(c, ws, (hipStream_t)stream);
}

extern "C" int adf_rolling_guidance_filter_host(int n_maps,
                                                const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride,
                                                void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride,
                                                int depth, int W, int H, int d, double sigma_color, double sigma_space, int num_iter,
                                                int border_type)
{
    RgfCall c = call_of(n_maps, src, src_stride, src_map_stride, dst, dst_stride, dst_map_stride, depth, W, H, d, sigma_color, sigma_space,
                        num_iter, border_type);
    int rc = rgf_check(c);
    if (rc) return rc;
    // the workspace: the planes between the iterations (none for num_iter <= 1)
    return staged_call(c.im, adf_rolling_guidance_workspace_bytes(n_maps, W, H, depth, num_iter), [&](const FilterImages& staged, void* ws, hipStream_t st) {
        RgfCall s = c;                                                   // the same call on the staged images
        s.im = staged;
        return rgf_run(s, ws, st);
    });
}
