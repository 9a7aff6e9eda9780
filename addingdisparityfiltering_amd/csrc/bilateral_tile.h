// bilateral_tile.h -- THE tile kernel of the two bilateral filters (joint_bilateral_kernels.hip, rolling_guidance_
// kernels.hip; include/adf_wls.h, "joint bilateral filter" and "rolling guidance filter", is the statement):
//
//   taps     (i, j), -r <= i, j <= r, i*i + j*j <= r*r, rows outer, columns inner; outside the image: borderInterpolate
//   w(p, q)  = S[i*i + j*j] * Wc(joint(p), joint(q))                            float32, Wc the filter's range weight
//   dst(p)   = (sum of w * (float)src(q)) / (sum of w), both sums ONE float32 chain in the taps' order, no FMA
//
// One workgroup of NT = TW x TH threads per output tile, one output pixel per thread.  The range table's leading part
// goes to LDS, and behind it the tile with its halo of r, staged once, one 8-byte entry per pixel: {(float)src, joint
// word}.  The border rule and the depths are resolved while staging, so the tap loop has no bounds test.
//
// The tap loop: the rows i = -r .. r, in each the columns j = -e .. e with e = floor(sqrt(r*r - i*i)).  i, j, e and the
// spatial weight S[i*i + j*j] are the same for every lane: scalar registers, S by scalar loads from the device table.
// Per tap a lane does one 8-byte LDS read (lanes 0..31 of a wave read 32 adjacent entries, all 64 banks once:
// conflict-free at every row pitch), the range weight, two multiplies and two adds.  A row goes UN taps at a time, their
// reads, range weights and weight products in flight together; the two accumulations stay one chain each.
//
// What differs between the filters is a Policy (five of them: the joint bilateral filter's 1 and 3 channels, the rolling
// guidance filter's three kinds of range table):
//   source_depth(a)              a.src_depth, narrowed to the depths the policy's calls can have
//   joint_word(a, m, x, y, raw)  the 32-bit word of an entry: pixel (x, y) of map m's joint as the range weight compares
//                                it (raw is the source's pixel there, for a joint that IS the source)
//   table_entries(a)             the leading entries of a.colour that go to LDS, in front of the tile
//   weights<N>(a, lds_c, s_row, j, e, c, w)
//                                w[u] = s_row[(j + u) * (j + u)] * Wc of the tap whose entry is e[u], for the centre's word c
// The product S * Wc is the statement's in every policy.  It is the policy's to write because WHERE the S loads stand
// among the range weights' reads decides how the compiler schedules a group: the joint bilateral filter forms the product
// tap by tap, the rolling guidance filter after the group's range weights (its far kind needs those together).  In the
// latter order the joint bilateral filter's batches measured 1 % slower.
#pragma once

#include "adf_internal.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace adf {
namespace bilateral {

constexpr int TW = 32, TH = 8, NT = TW * TH;                             // the output tile of a workgroup
constexpr int UN = 4;                                                    // taps of a row in flight together
constexpr size_t tile_entries(int r) { return (size_t)(TW + 2 * r) * (TH + 2 * r); }   // the tile and its halo
constexpr size_t table_bytes(size_t entries) { return (entries * sizeof(float) + 7) / 8 * 8; }
constexpr size_t lds_bytes(int r, size_t table_entries) { return table_bytes(table_entries) + tile_entries(r) * 8; }
static_assert(NT == 256 && TW == 32, "a wave's half reads one row of 32 adjacent entries");

struct TileArgs {
    const void* src; ptrdiff_t src_stride, src_map_stride;               // bytes
    const void* joint; ptrdiff_t joint_stride, joint_map_stride;         // (read by the policy's joint_word alone)
    void* dst; ptrdiff_t dst_stride, dst_map_stride;
    const float* colour; const float* space;                             // the range table; S, r*r + 1 entries
    int W, H, r, border, src_depth, dst_depth;
    unsigned tiles_x, tile0;                                             // tiles per row of tiles; first tile of this launch
    unsigned entry_bytes;                                                // 8, a tile entry, as a run-time value (see the tap loop)
    // what one policy reads
    float scale;                                                         // rolling guidance, ADF_32F: (float)(256 / sigma_color)
    unsigned last_offset;                                                // rolling guidance, integer depths: 4 (T - 1)
    int lds_entries;                                                     // rolling guidance: entries of `colour` staged in LDS
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

// Pixel x of a row of `depth` as a float; *raw = the pixel itself: the integer, or a float's bits.
__device__ __forceinline__ float load_pixel(const char* row, int x, int depth, uint32_t* raw)
{
    if (depth == ADF_32F) {
        const float v = reinterpret_cast<const float*>(row)[x];
        *raw = __float_as_uint(v);
        return v;
    }
    const int v = depth == ADF_16S ? (int)reinterpret_cast<const int16_t*>(row)[x] : (int)reinterpret_cast<const uint8_t*>(row)[x];
    *raw = (uint32_t)v;
    return (float)v;
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

template <class Policy>
__global__ void __launch_bounds__(NT) bilateral_tile_kernel(TileArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds_c = reinterpret_cast<float*>(smem);                       // the range table's leading part
    uint2* tile = reinterpret_cast<uint2*>(smem + table_bytes((size_t)Policy::table_entries(a)));   // [(TH + 2r)][(TW + 2r)] {(float)src, joint word}
    const int t = threadIdx.x, r = a.r, SW = TW + 2 * r, entries = SW * (TH + 2 * r);
    const unsigned tid = a.tile0 + blockIdx.x;
    const int x0 = (int)(tid % a.tiles_x) * TW, y0 = (int)(tid / a.tiles_x) * TH;
    const ptrdiff_t m = blockIdx.y;
    const char* src = static_cast<const char*>(a.src) + m * a.src_map_stride;

    for (int i = t; i < Policy::table_entries(a); i += NT) lds_c[i] = a.colour[i];
    for (int i = t; i < entries; i += NT) {                              // stage the tile and its halo, the border rule resolved
        const int sy = i / SW, sx = i - sy * SW;
        const int gx = border_index(x0 - r + sx, a.W, a.border), gy = border_index(y0 - r + sy, a.H, a.border);
        uint32_t raw;
        const float v = load_pixel(src + (ptrdiff_t)gy * a.src_stride, gx, Policy::source_depth(a), &raw);
        tile[i] = make_uint2(__float_as_uint(v), Policy::joint_word(a, m, gx, gy, raw));
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

    // N taps of the row at `row` from column j on: reads and weights first, then the two chains in order.
    auto taps = [&](auto n, const char* row, const float* s_row, int j) {
        constexpr int N = decltype(n)::value;
        uint64_t e[N];
        float w[N];
#pragma unroll
        for (int u = 0; u < N; u++) e[u] = *reinterpret_cast<const uint64_t*>(row + apart[u] + 8 * j);
        Policy::template weights<N>(a, lds_c, s_row, j, e, c, w);
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

} // namespace bilateral
} // namespace adf
