// joint_bilateral_kernels.hip -- cv::ximgproc::jointBilateralFilter(joint, src, dst, d, sigmaColor, sigmaSpace, borderType)
// on the device, in the library's own definition (include/adf_wls.h, "joint bilateral filter", is the statement;
// tests/jbf_ref.py states it in NumPy):
//
//   taps     (i, j), -r <= i, j <= r, i*i + j*j <= r*r, rows outer, columns inner; outside the image: borderInterpolate
//   w(p, q)  = S[i*i + j*j] * C[ sum_c |joint_c(p) - joint_c(q)| ]             float32, both tables built on the host
//   dst(p)   = (sum of w * (float)src(q)) / (sum of w), both sums ONE float32 chain in the taps' order, no FMA
//
// One workgroup of NT = TW x TH threads per output tile, one output pixel per thread, one launch per call.  The tile and
// its halo of r are staged in LDS once, one 8-byte entry per pixel: {(float)src, joint word}.  The border rule and the
// source's depth are resolved while staging, so the tap loop has no bounds test and no variants.  C sits in LDS in front
// of the tile (1 KiB for a 1-channel joint, 3 KiB for 3 channels).
//
// The tap loop: the rows i = -r .. r, in each the columns j = -e .. e with e = floor(sqrt(r*r - i*i)).  i, j, e and the
// spatial weight S[i*i + j*j] are the same for every lane: scalar registers, S by scalar loads from the device table.
// Per tap a lane does one 8-byte LDS read (lanes 0..31 of a wave read 32 adjacent entries, all 64 banks once:
// conflict-free at every row pitch), the L1 difference (1 channel: the joint word is 4 * joint, so |q - c| is the byte
// offset into C; 3 channels: v_sad_u8 of the packed bytes), one 4-byte gather from C -- the one access whose bank
// conflicts depend on the data --, two multiplies and two adds.  A row goes UN taps at a time, their reads, gathers and
// weight products in flight together; the two accumulations stay one chain each.
//
// LDS: 255 ch + 1 floats + (TW + 2r)(TH + 2r) entries of 8 B: 4.4 KiB at r = 2 (1 channel), 54.4 KiB at r = 31 (3
// channels) -- two workgroups per CU of 160 KiB.  Times and what bounds them: DESIGN.md, section 23.
#include "adf_host.h"

#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

using namespace adf;

namespace {

constexpr int TW = 32, TH = 8, NT = TW * TH;                             // the output tile of a workgroup
constexpr int UN = 4;                                                    // taps of a row in flight together
constexpr size_t colour_bytes(int ch) { return pad_to(jbf_colour_entries(ch) * sizeof(float), 8); }
constexpr size_t tile_entries(int r) { return (size_t)(TW + 2 * r) * (TH + 2 * r); }   // the tile and its halo
constexpr size_t lds_bytes(int r, int ch) { return colour_bytes(ch) + tile_entries(r) * 8; }
static_assert(NT == 256 && TW == 32, "a wave's half reads one row of 32 adjacent entries");
static_assert(lds_bytes(ADF_JBF_MAX_RADIUS, 3) <= 64 * 1024, "two workgroups per CU at the largest radius");

struct JbfArgs {
    const uint8_t* joint; ptrdiff_t joint_stride, joint_map_stride;      // bytes
    const void* src; ptrdiff_t src_stride, src_map_stride;
    void* dst; ptrdiff_t dst_stride, dst_map_stride;
    const float* colour; const float* space;                             // C, 255 ch + 1 entries; S, r*r + 1 entries
    int W, H, r, border, src_depth, dst_depth;
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

// The joint pixel as a tile entry holds it, and the byte offset into C of a tap whose word is `q` for a centre `c`.
template <int CH> __device__ __forceinline__ uint32_t joint_word(const uint8_t* j)
{
    return CH == 1 ? 4u * j[0] : (uint32_t)j[0] | ((uint32_t)j[1] << 8) | ((uint32_t)j[2] << 16);
}
template <int CH> __device__ __forceinline__ uint32_t colour_offset(uint32_t q, uint32_t c)
{
    return CH == 1 ? __usad(q, c, 0u) : 4u * __builtin_amdgcn_sad_u8(q, c, 0u);
}

// y in the output's depth: y, or rint (half to even) saturated; a NaN gives the depth's minimum.
__device__ __forceinline__ void store(void* row, int x, int depth, float y)
{
    if (depth == ADF_32F) { static_cast<float*>(row)[x] = y; return; }
    const float lo = depth == ADF_8U ? 0.0f : -32768.0f, hi = depth == ADF_8U ? 255.0f : 32767.0f;
    const float v = rintf(y);
    const int k = !(v >= lo) ? (int)lo : v > hi ? (int)hi : (int)v;
    if (depth == ADF_8U) static_cast<uint8_t*>(row)[x] = (uint8_t)k;
    else static_cast<int16_t*>(row)[x] = (int16_t)k;
}

template <int CH>
__global__ void __launch_bounds__(NT) jbf_kernel(JbfArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds_c = reinterpret_cast<float*>(smem);                       // C
    uint2* tile = reinterpret_cast<uint2*>(smem + colour_bytes(CH));     // [(TH + 2r)][(TW + 2r)] {(float)src, joint word}
    const int t = threadIdx.x, r = a.r, SW = TW + 2 * r, entries = SW * (TH + 2 * r);
    const unsigned tid = a.tile0 + blockIdx.x;
    const int x0 = (int)(tid % a.tiles_x) * TW, y0 = (int)(tid / a.tiles_x) * TH;
    const ptrdiff_t m = blockIdx.y;
    const uint8_t* joint = a.joint + m * a.joint_map_stride;
    const char* src = static_cast<const char*>(a.src) + m * a.src_map_stride;

    for (int i = t; i < (int)jbf_colour_entries(CH); i += NT) lds_c[i] = a.colour[i];
    for (int i = t; i < entries; i += NT) {                              // stage the tile and its halo, the border rule resolved
        const int sy = i / SW, sx = i - sy * SW;
        const int gx = border_index(x0 - r + sx, a.W, a.border), gy = border_index(y0 - r + sy, a.H, a.border);
        const char* p = src + (ptrdiff_t)gy * a.src_stride;
        const float v = a.src_depth == ADF_32F   ? reinterpret_cast<const float*>(p)[gx]
                        : a.src_depth == ADF_16S ? (float)reinterpret_cast<const int16_t*>(p)[gx]
                                                 : (float)reinterpret_cast<const uint8_t*>(p)[gx];
        tile[i] = make_uint2(__float_as_uint(v), joint_word<CH>(joint + (ptrdiff_t)gy * a.joint_stride + (ptrdiff_t)gx * CH));
    }
    __syncthreads();

    const int tx = t % TW, ty = t / TW, x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;                                    // (no barrier follows)
    // An entry is read as ONE 64-bit word, the source in its low half and the joint word in its high half: a uint2 the
    // compiler takes apart into 4-byte reads.  The UN reads of a group go through UN addresses a.entry_bytes (8) apart,
    // a distance the compiler does not know: reads it knows to be neighbours it pairs into ds_read2_b64, which moves half
    // the bytes per LDS cycle of two ds_read_b64 and banks by 16 lanes instead of 32.
    const char* centre = reinterpret_cast<const char*>(tile + (ty + r) * SW + tx + r);
    const uint32_t c = reinterpret_cast<const uint2*>(centre)->y;
    uint32_t apart[UN];
#pragma unroll
    for (int u = 0; u < UN; u++) apart[u] = a.entry_bytes * u;
    float sum = 0.0f, wsum = 0.0f;

    // N taps of the row at `row` from column j on: reads, gathers and weights first, then the two chains in order.
    auto taps = [&](auto n, const char* row, const float* s_row, int j) {
        constexpr int N = decltype(n)::value;
        uint64_t e[N];
        float w[N];
#pragma unroll
        for (int u = 0; u < N; u++) e[u] = *reinterpret_cast<const uint64_t*>(row + apart[u] + 8 * j);
#pragma unroll
        for (int u = 0; u < N; u++)
            w[u] = s_row[(j + u) * (j + u)] *
                   *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lds_c) + colour_offset<CH>((uint32_t)(e[u] >> 32), c));
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
    store(static_cast<char*>(a.dst) + m * a.dst_map_stride + (ptrdiff_t)y * a.dst_stride, x, a.dst_depth, sum / wsum);
}

struct JbfCall {                       // one call as its C entry point received it
    int n;
    const uint8_t* joint; ptrdiff_t joint_stride, joint_map_stride; int joint_channels;
    const void* src; ptrdiff_t src_stride, src_map_stride; int src_depth;
    void* dst; ptrdiff_t dst_stride, dst_map_stride; int dst_depth;
    int W, H, d; double sigma_color, sigma_space; int border;
    double sc, ss; int r;              // the clamped sigmas and the radius (jbf_check)
};

constexpr const char* WHO = "jointBilateralFilter";

bool known_depth(int depth) { return depth == ADF_8U || depth == ADF_16S || depth == ADF_32F; }
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

int jbf_check(JbfCall& c)
{
    if (!c.joint || !c.src || !c.dst) return fail(ADF_EBADARG, "%s: joint, src and dst must be non-NULL (an empty joint is cv::bilateralFilter, which is not built)", WHO);
    if (static_cast<const void*>(c.joint) == c.src) return fail(ADF_EBADARG, "%s: joint == src is cv::bilateralFilter, which is not built", WHO);
    if (c.n < 1 || c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(c.src_depth) || !known_depth(c.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (int rc = jbf_params_check(WHO, c.d, c.sigma_color, c.sigma_space, c.joint_channels, &c.sc, &c.ss, &c.r)) return rc;
    if (c.border == 0 || c.border == 3)
        return fail(ADF_EBADARG, "%s: %s is not built; BORDER_REPLICATE, BORDER_REFLECT and BORDER_REFLECT_101 are", WHO, c.border == 0 ? "BORDER_CONSTANT" : "BORDER_WRAP");
    if (c.border != ADF_BORDER_REPLICATE && c.border != ADF_BORDER_REFLECT && c.border != ADF_BORDER_REFLECT_101)
        return fail(ADF_EBADARG, "%s: borderType %d is not built; BORDER_REPLICATE (1), BORDER_REFLECT (2) and BORDER_REFLECT_101 (4) are", WHO, c.border);
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

template <int CH>
int jbf_launch(const JbfCall& c, JbfArgs a, hipStream_t st)
{
    const size_t lds = lds_bytes(c.r, CH);
    if (lds > 48 * 1024 - 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(jbf_kernel<CH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles_y = (unsigned)((c.H + TH - 1) / TH);
    a.tiles_x = (unsigned)((c.W + TW - 1) / TW);
    const uint64_t tiles = (uint64_t)a.tiles_x * tiles_y;               // below 2^31 / 256 + W / 32 + H / 8 + 1: 32 bits
    constexpr uint64_t PER_LAUNCH = 1u << 22;                            // (a grid's threads stay below 2^31)
    return for_batches(c.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.joint = c.joint + (ptrdiff_t)m0 * c.joint_map_stride;
        a.src = static_cast<const char*>(c.src) + (ptrdiff_t)m0 * c.src_map_stride;
        a.dst = static_cast<char*>(c.dst) + (ptrdiff_t)m0 * c.dst_map_stride;
        for (uint64_t t0 = 0; t0 < tiles; t0 += PER_LAUNCH) {
            a.tile0 = (unsigned)t0;
            hipLaunchKernelGGL((jbf_kernel<CH>), dim3((unsigned)std::min(tiles - t0, PER_LAUNCH), nm), dim3(NT), lds, st, a);
        }
        return launched();
    });
}

int jbf_run(const JbfCall& c, hipStream_t st)
{
    std::shared_ptr<JbfTable> table;                                     // held until the launches are queued
    JbfArgs a{};
    if (int rc = jbf_table_device(c.sc, c.ss, c.r, c.joint_channels, table, &a.colour, &a.space)) return rc;
    a.joint_stride = c.joint_stride; a.joint_map_stride = c.joint_map_stride;
    a.src_stride = c.src_stride; a.src_map_stride = c.src_map_stride;
    a.dst_stride = c.dst_stride; a.dst_map_stride = c.dst_map_stride;
    a.W = c.W; a.H = c.H; a.r = c.r; a.border = c.border; a.src_depth = c.src_depth; a.dst_depth = c.dst_depth;
    a.entry_bytes = 8;
    return c.joint_channels == 3 ? jbf_launch<3>(c, a, st) : jbf_launch<1>(c, a, st);
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
