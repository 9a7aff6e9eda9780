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
// One launch per iteration (the halo a pixel depends on grows by r with each, so they do not fuse): joint_bilateral_
// kernels.hip's shape.  A workgroup of NT = TW x TH threads per output tile stages tile and halo in LDS once, one 8-byte
// entry per pixel, {(float)src, the joint word of J_k}, the border rule resolved for both; in the first iteration both
// halves come from one load of src.  The tap loop has no bounds test, S comes by scalar loads, UN taps of a row are in
// flight together, and each of the two sums is one chain.
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

#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

using namespace adf;

namespace {

constexpr int TW = 32, TH = 8, NT = TW * TH;                             // the output tile of a workgroup
constexpr int UN = 4;                                                    // taps of a row in flight together
constexpr int LDS_ENTRIES = 1024;                                        // of an integer depth's C: what LDS holds of it
enum Kind { INT_NEAR, INT_FAR, FLOAT };
constexpr size_t tile_entries(int r) { return (size_t)(TW + 2 * r) * (TH + 2 * r); }   // the tile and its halo
constexpr size_t table_bytes(int lds_entries) { return pad_to((size_t)lds_entries * sizeof(float), 8); }
constexpr size_t lds_bytes(int r, int lds_entries) { return table_bytes(lds_entries) + tile_entries(r) * 8; }
static_assert(NT == 256 && TW == 32, "a wave's half reads one row of 32 adjacent entries");
static_assert(lds_bytes(ADF_JBF_MAX_RADIUS, (int)RGF_GRID_ENTRIES) <= 80 * 1024, "two workgroups per CU at the largest radius");

struct RgfArgs {
    const void* src; ptrdiff_t src_stride, src_map_stride;               // bytes
    const void* joint; ptrdiff_t joint_stride, joint_map_stride;         // J_k in src's depth; null: J_0 = src
    void* dst; ptrdiff_t dst_stride, dst_map_stride;                     // J_{k+1}, src's depth
    const float* colour; const float* space;                             // C (T entries) or G; S, r*r + 1 entries
    float scale;                                                         // FLOAT: (float)(256 / sigma_color)
    unsigned last_offset;                                                // integer kinds: 4 (T - 1)
    int lds_entries;                                                     // entries of `colour` staged in LDS
    int W, H, r, border, depth;
    unsigned tiles_x, tile0;                                             // tiles per row of tiles; first tile of this launch
    unsigned entry_bytes;                                                // 8, a tile entry, as a run-time value (see the tap loop)
};

// cv::borderInterpolate of coordinate p on an axis of length n, for any p (include/adf_wls.h: "Window").
__device__ __forceinline__ int border_index(int p, int n, int border)
{
    if (p >= 0 && p < n) return p;
    if (border == ADF_BORDER_REPLICATE) return p < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const long long period = border == ADF_BORDER_REFLECT ? 2ll * n : 2ll * n - 2;
    long long m = p % period;
    if (m < 0) m += period;
    return (int)(m < n ? m : period - (border == ADF_BORDER_REFLECT ? 1 : 0) - m);
}

// One pixel of a plane of `depth` as (float)value and as the joint word its kind of kernel compares.
template <int KIND> __device__ __forceinline__ void load(const char* row, int x, int depth, float* value, uint32_t* word)
{
    if (KIND == FLOAT) {
        *value = reinterpret_cast<const float*>(row)[x];
        *word = __float_as_uint(*value);
        return;
    }
    const int v = depth == ADF_16S ? (int)reinterpret_cast<const int16_t*>(row)[x] : (int)reinterpret_cast<const uint8_t*>(row)[x];
    *value = (float)v;
    *word = 4u * (uint32_t)(v + (depth == ADF_16S ? 32768 : 0));
}

// y in the source's depth: y, or rint (half to even) saturated; a NaN gives the depth's minimum.
__device__ __forceinline__ void store(void* row, int x, int depth, float y)
{
    if (depth == ADF_32F) { static_cast<float*>(row)[x] = y; return; }
    const float lo = depth == ADF_8U ? 0.0f : -32768.0f, hi = depth == ADF_8U ? 255.0f : 32767.0f;
    const float v = rintf(y);
    const int k = !(v >= lo) ? (int)lo : v > hi ? (int)hi : (int)v;
    if (depth == ADF_8U) static_cast<uint8_t*>(row)[x] = (uint8_t)k;
    else static_cast<int16_t*>(row)[x] = (int16_t)k;
}

// Wc of N taps whose joint words are the high halves of `e`, for a centre `c` (include/adf_wls.h: "Range weight").
template <int KIND, int N> __device__ __forceinline__ void range_weights(const RgfArgs& a, const float* lds_c, const uint64_t (&e)[N], uint32_t c, float (&w)[N])
{
    if constexpr (KIND == FLOAT) {
#pragma unroll
        for (int u = 0; u < N; u++) {
            float t = fabsf(__uint_as_float(c) - __uint_as_float((uint32_t)(e[u] >> 32))) * a.scale;
            if (!(t < 4096.0f)) t = 4096.0f;                             // (NaN and infinity too: G[4096] = G[4097] = 0)
            const int idx = (int)t;
            const float f = t - (float)idx, g0 = lds_c[idx], g1 = lds_c[idx + 1];
            w[u] = g0 + f * (g1 - g0);
        }
    } else {
        constexpr uint32_t LDS_END = 4u * LDS_ENTRIES;                   // byte offsets from here on are not in LDS
        uint32_t off[N];                                                 // 4 min(L, T - 1)
        bool far = false;
#pragma unroll
        for (int u = 0; u < N; u++) {
            off[u] = min(__usad((uint32_t)(e[u] >> 32), c, 0u), a.last_offset);
            w[u] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lds_c) + (KIND == INT_FAR ? min(off[u], LDS_END - 4u) : off[u]));
            far = far || off[u] >= LDS_END;
        }
        if constexpr (KIND == INT_FAR) {
            // The LDS values are made opaque first: otherwise the compiler selects between an LDS and a global POINTER per
            // tap and issues one flat load, which counts against both memory counters.
#pragma unroll
            for (int u = 0; u < N; u++) asm("" : "+v"(w[u]));
            if (far) {                                                   // lanes with a tap beyond LDS; a wave without one skips this
                float g[N];                                              // the N loads in flight together; a near tap reads entry 0
#pragma unroll
                for (int u = 0; u < N; u++) g[u] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.colour) + (off[u] >= LDS_END ? off[u] : 0u));
#pragma unroll
                for (int u = 0; u < N; u++) w[u] = off[u] >= LDS_END ? g[u] : w[u];
            }
        }
    }
}

template <int KIND>
__global__ void __launch_bounds__(NT) rgf_kernel(RgfArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds_c = reinterpret_cast<float*>(smem);                       // C's leading part, or G
    uint2* tile = reinterpret_cast<uint2*>(smem + table_bytes(a.lds_entries));   // [(TH + 2r)][(TW + 2r)] {(float)src, joint word}
    const int t = threadIdx.x, r = a.r, SW = TW + 2 * r, entries = SW * (TH + 2 * r);
    const unsigned tid = a.tile0 + blockIdx.x;
    const int x0 = (int)(tid % a.tiles_x) * TW, y0 = (int)(tid / a.tiles_x) * TH;
    const ptrdiff_t m = blockIdx.y;
    const char* src = static_cast<const char*>(a.src) + m * a.src_map_stride;
    const char* joint = a.joint ? static_cast<const char*>(a.joint) + m * a.joint_map_stride : nullptr;

    for (int i = t; i < a.lds_entries; i += NT) lds_c[i] = a.colour[i];
    for (int i = t; i < entries; i += NT) {                              // stage the tile and its halo, the border rule resolved
        const int sy = i / SW, sx = i - sy * SW;
        const int gx = border_index(x0 - r + sx, a.W, a.border), gy = border_index(y0 - r + sy, a.H, a.border);
        float v, unused;
        uint32_t w;
        load<KIND>(src + (ptrdiff_t)gy * a.src_stride, gx, a.depth, &v, &w);
        if (joint) load<KIND>(joint + (ptrdiff_t)gy * a.joint_stride, gx, a.depth, &unused, &w);
        tile[i] = make_uint2(__float_as_uint(v), w);
    }
    __syncthreads();

    const int tx = t % TW, ty = t / TW, x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;                                    // (no barrier follows)
    // As in jbf_kernel: an entry is read as ONE 64-bit word, and the UN reads of a group go through addresses
    // a.entry_bytes (8) apart, a distance the compiler does not know, so that it keeps them ds_read_b64.
    const char* centre = reinterpret_cast<const char*>(tile + (ty + r) * SW + tx + r);
    const uint32_t c = reinterpret_cast<const uint2*>(centre)->y;
    uint32_t apart[UN];
#pragma unroll
    for (int u = 0; u < UN; u++) apart[u] = a.entry_bytes * u;
    float sum = 0.0f, wsum = 0.0f;

    // N taps of the row at `row` from column j on: reads, range weights and products first, then the two chains in order.
    auto taps = [&](auto n, const char* row, const float* s_row, int j) {
        constexpr int N = decltype(n)::value;
        uint64_t e[N];
        float w[N];
#pragma unroll
        for (int u = 0; u < N; u++) e[u] = *reinterpret_cast<const uint64_t*>(row + apart[u] + 8 * j);
        range_weights<KIND, N>(a, lds_c, e, c, w);
#pragma unroll
        for (int u = 0; u < N; u++) w[u] = s_row[(j + u) * (j + u)] * w[u];
#pragma unroll
        for (int u = 0; u < N; u++) {
            sum = sum + w[u] * __uint_as_float((uint32_t)e[u]);
            wsum = wsum + w[u];
        }
    };
    int ext = 0;                                                         // floor(sqrt(r*r - i*i)), carried from row to row
#pragma unroll 1
    for (int i = -r; i <= r; i++) {
        const int room = r * r - i * i;
        while ((ext + 1) * (ext + 1) <= room) ext++;
        while (ext * ext > room) ext--;
        const char* row = centre + 8 * i * SW;
        const float* s_row = a.space + i * i;
        int j = -ext;
#pragma unroll 1
        for (; j + UN <= ext + 1; j += UN) taps(std::integral_constant<int, UN>{}, row, s_row, j);
        if (ext + 1 - j == 3) taps(std::integral_constant<int, 3>{}, row, s_row, j);   // (2 ext + 1 is odd: 1 or 3 taps are left)
        else taps(std::integral_constant<int, 1>{}, row, s_row, j);
    }
    store(static_cast<char*>(a.dst) + m * a.dst_map_stride + (ptrdiff_t)y * a.dst_stride, x, a.depth, sum / wsum);
}

struct RgfCall {                       // one call as its C entry point received it
    int n;
    const void* src; ptrdiff_t src_stride, src_map_stride;
    void* dst; ptrdiff_t dst_stride, dst_map_stride;
    int depth, W, H, d; double sigma_color, sigma_space; int num_iter, border;
    double sc, ss; int r; float scale; // the clamped sigmas, the radius and the float grid's scale (rgf_check)
};

constexpr const char* WHO = "rollingGuidanceFilter";

size_t depth_size(int depth) { return depth == ADF_8U ? 1 : depth == ADF_16S ? 2 : 4; }

// The bytes n images span, [lo, hi): what "overlap" is tested on.
struct Span { uintptr_t lo, hi; };
Span span_of(const void* p, int n, ptrdiff_t row_bytes, int rows, ptrdiff_t stride, ptrdiff_t map_stride)
{
    const uintptr_t b = reinterpret_cast<uintptr_t>(p);
    return Span{b, b + (uintptr_t)((ptrdiff_t)(n - 1) * map_stride + (ptrdiff_t)(rows - 1) * stride + row_bytes)};
}
bool overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

bool aligned(const void* p, ptrdiff_t stride, ptrdiff_t map_stride, ptrdiff_t es)
{
    return !(((uintptr_t)p & (es - 1)) || (stride & (es - 1)) || (map_stride & (es - 1)));
}

int rgf_check(RgfCall& c)
{
    if (!c.src || !c.dst) return fail(ADF_EBADARG, "%s: src and dst must be non-NULL", WHO);
    if (c.n < 1 || c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (int rc = rgf_params_check(WHO, c.depth, c.d, c.sigma_color, c.sigma_space, &c.sc, &c.ss, &c.r, &c.scale)) return rc;
    if (c.num_iter < 0 || c.num_iter > ADF_RGF_MAX_ITERS)
        return fail(ADF_EBADARG, "%s: numOfIter must lie in [0, %d] (got %d)", WHO, ADF_RGF_MAX_ITERS, c.num_iter);
    if (c.border == 0 || c.border == 3)
        return fail(ADF_EBADARG, "%s: %s is not built; BORDER_REPLICATE, BORDER_REFLECT and BORDER_REFLECT_101 are", WHO, c.border == 0 ? "BORDER_CONSTANT" : "BORDER_WRAP");
    if (c.border != ADF_BORDER_REPLICATE && c.border != ADF_BORDER_REFLECT && c.border != ADF_BORDER_REFLECT_101)
        return fail(ADF_EBADARG, "%s: borderType %d is not built; BORDER_REPLICATE (1), BORDER_REFLECT (2) and BORDER_REFLECT_101 (4) are", WHO, c.border);
    const ptrdiff_t es = (ptrdiff_t)depth_size(c.depth);
    if (!aligned(c.src, c.src_stride, c.src_map_stride, es) || !aligned(c.dst, c.dst_stride, c.dst_map_stride, es))
        return fail(ADF_EBADARG, "%s: src and dst and their strides must be aligned to the depth", WHO);
    if ((int64_t)c.W * c.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "%s: W*H must be below 2^31", WHO);
    const ptrdiff_t row = (ptrdiff_t)c.W * es;
    if (c.src_stride < row || c.dst_stride < row) return fail(ADF_ESIZE, "%s: row stride smaller than a row", WHO);
    if (c.n > 1 && c.src_map_stride < 0) return fail(ADF_ESIZE, "%s: map strides must not be negative", WHO);
    if (!images_disjoint(c.n, row, c.H, c.dst_stride, c.dst_map_stride, false))
        return fail(ADF_ESIZE, "%s: destination maps of the batch overlap (map stride smaller than a map)", WHO);
    if (overlap(span_of(c.dst, c.n, row, c.H, c.dst_stride, c.dst_map_stride), span_of(c.src, c.n, row, c.H, c.src_stride, c.src_map_stride)))
        return fail(ADF_EBADARG, "%s: dst must not overlap src (there is no in-place call)", WHO);
    return ADF_OK;
}

template <int KIND>
int rgf_launch(const RgfCall& c, RgfArgs a, hipStream_t st)
{
    const size_t lds = lds_bytes(c.r, a.lds_entries);
    if (lds > 48 * 1024 - 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rgf_kernel<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles_y = (unsigned)((c.H + TH - 1) / TH);
    a.tiles_x = (unsigned)((c.W + TW - 1) / TW);
    const uint64_t tiles = (uint64_t)a.tiles_x * tiles_y;               // below 2^31 / 256 + W / 32 + H / 8 + 1: 32 bits
    constexpr uint64_t PER_LAUNCH = 1u << 22;                            // (a grid's threads stay below 2^31)
    const RgfArgs first = a;
    return for_batches(c.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.src = static_cast<const char*>(first.src) + (ptrdiff_t)m0 * a.src_map_stride;
        a.joint = first.joint ? static_cast<const char*>(first.joint) + (ptrdiff_t)m0 * a.joint_map_stride : nullptr;
        a.dst = static_cast<char*>(first.dst) + (ptrdiff_t)m0 * a.dst_map_stride;
        for (uint64_t t0 = 0; t0 < tiles; t0 += PER_LAUNCH) {
            a.tile0 = (unsigned)t0;
            hipLaunchKernelGGL((rgf_kernel<KIND>), dim3((unsigned)std::min(tiles - t0, PER_LAUNCH), nm), dim3(NT), lds, st, a);
        }
        return launched();
    });
}

// ws: adf_rolling_guidance_workspace_bytes of device memory, one dense plane of the source's depth per map (unused, and
// may be null, for num_iter <= 1).  Iteration k writes dst when an even number of iterations follow it, else the plane:
// the last one writes dst.
int rgf_run(const RgfCall& c, void* ws, hipStream_t st)
{
    const ptrdiff_t row = (ptrdiff_t)c.W * (ptrdiff_t)depth_size(c.depth), map = row * c.H;
    if (c.num_iter == 0)
        return copy_images(c.dst, (size_t)c.dst_stride, c.dst_map_stride, c.src, (size_t)c.src_stride, c.src_map_stride, (size_t)row, (size_t)c.H, c.n,
                           hipMemcpyDeviceToDevice, st);
    std::shared_ptr<RgfTable> table;                                     // held until the launches are queued
    RgfArgs a{};
    int entries = 0;
    if (int rc = rgf_table_device(c.depth, c.sc, c.ss, c.r, table, &a.colour, &a.space, &entries)) return rc;
    const Kind kind = c.depth == ADF_32F ? FLOAT : entries > LDS_ENTRIES ? INT_FAR : INT_NEAR;
    a.lds_entries = kind == FLOAT ? entries : std::min(entries, LDS_ENTRIES);
    a.last_offset = 4u * (unsigned)(entries - 1);
    a.scale = c.scale;
    a.src = c.src; a.src_stride = c.src_stride; a.src_map_stride = c.src_map_stride;
    a.W = c.W; a.H = c.H; a.r = c.r; a.border = c.border; a.depth = c.depth;
    a.entry_bytes = 8;
    for (int k = 0; k < c.num_iter; k++) {
        if ((c.num_iter - 1 - k) % 2 == 0) { a.dst = c.dst; a.dst_stride = c.dst_stride; a.dst_map_stride = c.dst_map_stride; }
        else { a.dst = ws; a.dst_stride = row; a.dst_map_stride = map; }
        const int rc = kind == FLOAT ? rgf_launch<FLOAT>(c, a, st) : kind == INT_FAR ? rgf_launch<INT_FAR>(c, a, st) : rgf_launch<INT_NEAR>(c, a, st);
        if (rc) return rc;
        a.joint = a.dst; a.joint_stride = a.dst_stride; a.joint_map_stride = a.dst_map_stride;   // J_{k+1}
    }
    return ADF_OK;
}

RgfCall call_of(int n_maps, const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, void* dst, ptrdiff_t dst_stride,
                ptrdiff_t dst_map_stride, int depth, int W, int H, int d, double sigma_color, double sigma_space, int num_iter, int border_type)
{
    return RgfCall{n_maps, src, src_stride, src_map_stride, dst, dst_stride, dst_map_stride, depth, W, H, d, sigma_color, sigma_space,
                   num_iter, border_type, 0.0, 0.0, 0, 1.0f};
}

} // namespace

extern "C" size_t adf_rolling_guidance_workspace_bytes(int n_maps, int W, int H, int depth, int num_iter)
{
    if (n_maps < 1 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) return 0;
    if ((depth != ADF_8U && depth != ADF_16S && depth != ADF_32F) || num_iter <= 1 || num_iter > ADF_RGF_MAX_ITERS) return 0;
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
    // one block: the sources, dense, then the results and the planes between the iterations
    const size_t row = (size_t)W * depth_size(depth), map = (size_t)H * row, maps = pad_to(map * n_maps, 256);
    Scratch blk;
    if ((rc = blk.take(2 * maps + adf_rolling_guidance_workspace_bytes(n_maps, W, H, depth, num_iter), nullptr))) return rc;
    char* base = static_cast<char*>(blk.p);
    RgfCall s = c;                                                       // the same call on the staged images
    s.src = base; s.src_stride = (ptrdiff_t)row; s.src_map_stride = (ptrdiff_t)map;
    s.dst = base + maps; s.dst_stride = (ptrdiff_t)row; s.dst_map_stride = (ptrdiff_t)map;
    if ((rc = copy_images(base, row, map, src, src_stride, src_map_stride, row, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = rgf_run(s, base + 2 * maps, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(dst, dst_stride, dst_map_stride, base + maps, row, map, row, H, n_maps, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
