// reproject_kernels.hip -- cv::reprojectImageTo3D(disparity, _3dImage, Q, handleMissingValues, ddepth) (calib3d, outside
// the reference tree: parity UNPINNED) on the device, and a compact point list of the valid pixels.  The definition is the
// library's own (include/adf_wls.h, "reprojection to 3-D"); the device result is bit-exact against the direct NumPy
// statement tests/reproject_ref.py.  Per pixel (x, y) with raw source value s (CV_16SC1 or CV_32FC1):
//
//     d   = (double)s * disp_scale
//     r_i = ((Q[i][0]*x + Q[i][1]*y) + Q[i][3]) + Q[i][2]*d          i = 0..3
//     iw  = 1.0 / r_3
//     X = r_0*iw, Y = r_1*iw, Z = r_2*iw, each rounded to float once
//
// every product, sum and the division one IEEE binary64 operation in this order (the library is built with
// -ffp-contract=off: no fused multiply-add).  missing(s) <=> fabs((double)s - m) <= FLT_EPSILON gives Z = 10000.0f.
//
// Kernels
//   reproject_min_kernel   ADF_MISSING_MIN only: the minimum raw value of each map.  Values become order-preserving uint32
//                          keys (NaN skipped), 32768 pixels per workgroup, reduced per wave by shuffles, per workgroup
//                          through LDS, then AT MOST one integer atomic min per workgroup into the map's 4-byte slot (preset
//                          to 0xffffffff by hipMemsetAsync; skipped when the slot is already at or below the workgroup's
//                          key): exact and independent of the order of arrival.
//   reproject_kernel       a pure stream: lanes along x, four consecutive pixels per thread, one 8-byte (int16) or 16-byte
//                          (float) load, and 16-byte stores only -- three for XYZ, one for Z -- when bases and strides allow;
//                          a wave whose 64 lanes all do so in one row passes its XYZ pieces through LDS first, so that each
//                          store instruction writes 1024 contiguous bytes (0.52 -> 0.39 ms on 16 maps of 4K).  The row tail
//                          and unaligned images go element by element through the same arithmetic.
//   point list             three plain launches, no workgroup ever waits for another:
//     cloud_count_kernel   valid pixels per tile of TILE consecutive pixels of the ROI's raster (reads the disparity only)
//     cloud_scan_kernel    one workgroup per map: exclusive scan of the tile counts in place, counts[map] = the total
//     cloud_write_kernel   recomputes, ranks inside the tile (__ballot + mbcnt, segment offsets through LDS), stages the
//                          tile's compacted points in LDS and writes them as one contiguous run: dwords up to the first
//                          16-byte boundary, 16-byte pieces, dwords after the last.  Entries k >= capacity are not written.
//                          The W x H x 3 image is never materialised.
#include "adf_host.h"

#include <cfloat>
#include <cmath>

using namespace adf;

namespace {

constexpr int NT = 256;
constexpr int PX = 4;                  // pixels per thread of the streaming kernels
constexpr int MIN_GROUPS = 32;         // groups of PX pixels per thread of the minimum kernel: 32768 pixels per workgroup
constexpr int TILE = 1024;             // pixels per tile of the point list: TILE / NT rounds of one pixel per lane
constexpr int ROUNDS = TILE / NT, SEGS = ROUNDS * (NT / 64);
constexpr uint32_t KEY_NONE = 0xffffffffu;

struct Geometry {                      // what every kernel needs to turn (x, y, s) into a point
    double Q[16];
    double scale;                      // disp_scale
    double missing;                    // m of ADF_MISSING_VALUE
    const uint32_t* min_key;           // [map]: key of m for ADF_MISSING_MIN
    int mode;
};

// ---- order-preserving keys: a < b  <=>  key(a) < key(b) ----
__device__ __forceinline__ uint32_t key_of(int16_t v) { return (uint32_t)((int)v + 32768); }
__device__ __forceinline__ uint32_t key_of_bits(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t key_of(float v) { return v != v ? KEY_NONE : key_of_bits(__float_as_uint(v)); }
// (KEY_NONE is the key of no float but a NaN with every payload bit set: a map of NaNs only keeps it and has m = NaN, which
// is within FLT_EPSILON of nothing)
template <class SRC> __device__ __forceinline__ double value_of_key(uint32_t k);
template <> __device__ __forceinline__ double value_of_key<int16_t>(uint32_t k) { return (double)((int)k - 32768); }
template <> __device__ __forceinline__ double value_of_key<float>(uint32_t k)
{
    return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <class SRC> __device__ __forceinline__ double missing_value(const Geometry& g, int map)
{
    return g.mode == ADF_MISSING_MIN ? value_of_key<SRC>(g.min_key[map]) : g.missing;
}

__device__ __forceinline__ bool is_missing(const Geometry& g, double s, double m)
{
    return g.mode != ADF_MISSING_NONE && fabs(s - m) <= (double)FLT_EPSILON;
}

// THE arithmetic (include/adf_wls.h); qy[i] = Q[i][1] * y of the pixel's row
__device__ __forceinline__ void reproject_px(const Geometry& g, const double* qy, int x, double s, double m, float* xyz)
{
    const double d = s * g.scale, xd = (double)x;
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = ((g.Q[4 * i] * xd + qy[i]) + g.Q[4 * i + 3]) + g.Q[4 * i + 2] * d;
    const double iw = 1.0 / r[3];
    xyz[0] = (float)(r[0] * iw);
    xyz[1] = (float)(r[1] * iw);
    xyz[2] = is_missing(g, s, m) ? 10000.0f : (float)(r[2] * iw);
}

__device__ __forceinline__ void row_terms(const Geometry& g, int y, double* qy)
{
#pragma unroll
    for (int i = 0; i < 4; i++) qy[i] = g.Q[4 * i + 1] * (double)y;
}

// PX consecutive source values: one 8- or 16-byte load
__device__ __forceinline__ void load_px(const int16_t* p, int16_t* v)
{
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    v[0] = (int16_t)(w.x & 0xffffu); v[1] = (int16_t)(w.x >> 16); v[2] = (int16_t)(w.y & 0xffffu); v[3] = (int16_t)(w.y >> 16);
}
__device__ __forceinline__ void load_px(const float* p, float* v)
{
    const float4 w = *reinterpret_cast<const float4*>(p);
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
}

// ---------------------------------------------------------------------------------------------------------
// the image
// ---------------------------------------------------------------------------------------------------------
struct ImageArgs {
    const char* src; ptrdiff_t sstride, smap;     // bytes
    char* out; ptrdiff_t ostride, omap;
    int W, H;
    int groups;        // groups of PX pixels per row (the last one may be short)
    int total;         // groups * H
    int vec_src, vec_dst;
    Geometry g;
};

template <class SRC> __global__ void __launch_bounds__(NT) reproject_min_kernel(ImageArgs a, uint32_t* slots)
{
    __shared__ uint32_t wave_min[NT / 64];
    uint32_t k = KEY_NONE;
    const char* src = a.src + (ptrdiff_t)blockIdx.y * a.smap;
    for (int j = 0; j < MIN_GROUPS; j++) {
        const int64_t idx = ((int64_t)blockIdx.x * MIN_GROUPS + j) * NT + threadIdx.x;
        if (idx >= a.total) break;
        const int y = (int)(idx / a.groups), x0 = (int)(idx - (int64_t)y * a.groups) * PX;
        const SRC* row = reinterpret_cast<const SRC*>(src + (ptrdiff_t)y * a.sstride);
        if (a.vec_src && x0 + PX <= a.W) {
            SRC v[PX];
            load_px(row + x0, v);
#pragma unroll
            for (int i = 0; i < PX; i++) k = min(k, key_of(v[i]));
        } else {
            for (int x = x0; x < min(x0 + PX, a.W); x++) k = min(k, key_of(row[x]));
        }
    }
    for (int o = 32; o > 0; o >>= 1) k = min(k, (uint32_t)__shfl_xor((int)k, o));
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; w++) k = min(k, wave_min[w]);
        // (the slot only ever decreases: an older value read here can only let a needless atomic through)
        if (k < __hip_atomic_load(&slots[blockIdx.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&slots[blockIdx.y], k);
    }
}

template <class SRC, int CH> __global__ void __launch_bounds__(NT) reproject_kernel(ImageArgs a)
{
    const unsigned uidx = blockIdx.x * NT + threadIdx.x;             // (the last workgroup may reach past 2^31)
    if (uidx >= (unsigned)a.total) return;
    const int idx = (int)uidx, map = blockIdx.y;
    const int y = (int)((unsigned)idx / (unsigned)a.groups), x0 = (idx - y * a.groups) * PX;
    const SRC* row = reinterpret_cast<const SRC*>(a.src + (ptrdiff_t)map * a.smap + (ptrdiff_t)y * a.sstride);
    float* orow = reinterpret_cast<float*>(a.out + (ptrdiff_t)map * a.omap + (ptrdiff_t)y * a.ostride);
    const int n = min(PX, a.W - x0);
    const double m = missing_value<SRC>(a.g, map);
    double qy[4];
    row_terms(a.g, y, qy);

    SRC v[PX];
    if (a.vec_src && n == PX) {
        load_px(row + x0, v);
    } else {
#pragma unroll
        for (int i = 0; i < PX; i++) v[i] = i < n ? row[x0 + i] : (SRC)0;
    }
    float p[PX][3];
#pragma unroll
    for (int i = 0; i < PX; i++) reproject_px(a.g, qy, x0 + i, (double)v[i], m, p[i]);

    if (CH == 3) {
        // A lane's 48 bytes are three 16-byte pieces 48 bytes apart: stored from the lanes that computed them, each store
        // instruction would touch every 128-byte line of the wave's 3072 bytes.  When the whole wave takes the vector path
        // in ONE row its bytes are one contiguous run: the pieces change lanes through LDS (wave-local: no workgroup
        // barrier) and each store instruction writes 1024 contiguous bytes.
        __shared__ float4 stage[NT * 3];
        const int lane = threadIdx.x & 63;
        const bool full = a.vec_dst && n == PX && y == __builtin_amdgcn_readfirstlane(y);
        if (__ballot(full) == ~0ull) {
            float4* mine = stage + (threadIdx.x - lane) * 3;
            mine[lane * 3] = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
            mine[lane * 3 + 1] = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
            mine[lane * 3 + 2] = make_float4(p[2][2], p[3][0], p[3][1], p[3][2]);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            float4* o = reinterpret_cast<float4*>(orow + (ptrdiff_t)(x0 - PX * lane) * 3);   // lane 0's first pixel
#pragma unroll
            for (int j = 0; j < 3; j++) o[j * 64 + lane] = mine[j * 64 + lane];
            return;
        }
    }
    if (a.vec_dst && n == PX) {
        if (CH == 3) {
            float4* o = reinterpret_cast<float4*>(orow + (ptrdiff_t)x0 * 3);
            o[0] = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
            o[1] = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
            o[2] = make_float4(p[2][2], p[3][0], p[3][1], p[3][2]);
        } else {
            *reinterpret_cast<float4*>(orow + x0) = make_float4(p[0][2], p[1][2], p[2][2], p[3][2]);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < PX; i++) {
        if (i >= n) break;
        if (CH == 3) {
            float* o = orow + (ptrdiff_t)(x0 + i) * 3;
            o[0] = p[i][0]; o[1] = p[i][1]; o[2] = p[i][2];
        } else {
            orow[x0 + i] = p[i][2];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// the point list
// ---------------------------------------------------------------------------------------------------------
struct CloudArgs {
    const char* src; ptrdiff_t sstride, smap;     // bytes
    int W;
    adf_rect roi;
    int npx;                                      // roi.width * roi.height
    int tiles;                                    // tiles per map
    double z_min, z_max;
    const uint8_t* view; ptrdiff_t vstride, vmap; int vch;
    float* points; ptrdiff_t pmap;                // map strides in bytes
    uint8_t* colours; ptrdiff_t cmap;
    int32_t* index; ptrdiff_t imap;
    int capacity;
    uint32_t* counts;                             // [map]
    uint32_t* tile_counts;                        // [map][tiles]: counts after the first launch, exclusive offsets after the second
    Geometry g;
};

// pixel `p` of the ROI's raster: its coordinates, its point and whether the list takes it
template <class SRC>
__device__ __forceinline__ bool cloud_px(const CloudArgs& a, int map, int64_t p64, double m, int* px, int* py, float* xyz)
{
    if (p64 >= a.npx) return false;                                  // (the last tile may reach past 2^31)
    const int p = (int)p64;
    const int yy = (int)((unsigned)p / (unsigned)a.roi.width), x = a.roi.x + (p - yy * a.roi.width), y = a.roi.y + yy;
    *px = x; *py = y;
    const double s = (double)reinterpret_cast<const SRC*>(a.src + (ptrdiff_t)map * a.smap + (ptrdiff_t)y * a.sstride)[x];
    if (is_missing(a.g, s, m)) return false;                         // (a wave of missing pixels skips the arithmetic)
    double qy[4];
    row_terms(a.g, y, qy);
    reproject_px(a.g, qy, x, s, m, xyz);
    if (!(isfinite(xyz[0]) && isfinite(xyz[1]) && isfinite(xyz[2]))) return false;
    return a.z_min <= (double)xyz[2] && (double)xyz[2] <= a.z_max;
}

template <class SRC> __global__ void __launch_bounds__(NT) cloud_count_kernel(CloudArgs a)
{
    __shared__ uint32_t wave_n[NT / 64];
    const int map = blockIdx.y, tile = blockIdx.x;
    const double m = missing_value<SRC>(a.g, map);
    uint32_t n = 0;                                                  // wave-uniform
    for (int r = 0; r < ROUNDS; r++) {
        int x, y; float xyz[3];
        const bool ok = cloud_px<SRC>(a, map, (int64_t)tile * TILE + r * NT + (int)threadIdx.x, m, &x, &y, xyz);
        n += (uint32_t)__popcll(__ballot(ok));
    }
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; w++) n += wave_n[w];
        a.tile_counts[(size_t)map * a.tiles + tile] = n;
    }
}

// One workgroup per map.  Thread t owns the tiles [t * chunk, (t + 1) * chunk): sums them, the workgroup scans the NT sums
// in LDS, and the thread rewrites its tiles as exclusive offsets.
__global__ void __launch_bounds__(NT) cloud_scan_kernel(CloudArgs a)
{
    __shared__ uint32_t sums[NT];
    const int t = threadIdx.x, chunk = (a.tiles + NT - 1) / NT;
    uint32_t* tc = a.tile_counts + (size_t)blockIdx.x * a.tiles;
    const int t0 = min(t * chunk, a.tiles), t1 = min(t0 + chunk, a.tiles);
    uint32_t s = 0;
    for (int i = t0; i < t1; i++) s += tc[i];
    sums[t] = s;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {                               // inclusive scan, Hillis-Steele
        const uint32_t add = t >= o ? sums[t - o] : 0;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    uint32_t run = sums[t] - s;
    for (int i = t0; i < t1; i++) { const uint32_t c = tc[i]; tc[i] = run; run += c; }
    if (t == NT - 1) a.counts[blockIdx.x] = sums[NT - 1];
}

// n dwords from LDS to dst (4-byte aligned): the dwords before the first 16-byte boundary of dst one by one, then 16-byte
// pieces, then the rest one by one
__device__ __forceinline__ void store_run(uint32_t* dst, const uint32_t* lds, int n)
{
    const int head = min(n, (int)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
    const int body = (n - head) >> 2, tail0 = head + 4 * body;
    const int t = threadIdx.x;
    if (t < head) dst[t] = lds[t];
    for (int i = t; i < body; i += NT) {
        const uint32_t* s = lds + head + 4 * i;
        reinterpret_cast<uint4*>(dst + head)[i] = make_uint4(s[0], s[1], s[2], s[3]);
    }
    if (t < n - tail0) dst[tail0 + t] = lds[tail0 + t];
}

template <class SRC> __global__ void __launch_bounds__(NT) cloud_write_kernel(CloudArgs a)
{
    __shared__ uint32_t seg_n[SEGS];
    __shared__ uint32_t pts[TILE * 3];
    __shared__ uint32_t idx[TILE];
    __shared__ uint8_t col[TILE * 3];
    const int map = blockIdx.y, tile = blockIdx.x, t = threadIdx.x, wave = t >> 6;
    const uint32_t base = a.tile_counts[(size_t)map * a.tiles + tile];
    if (base >= (uint32_t)a.capacity) return;                        // (workgroup-uniform) nothing of this tile fits
    const double m = missing_value<SRC>(a.g, map);

    bool ok[ROUNDS]; int x[ROUNDS], y[ROUNDS]; float xyz[ROUNDS][3]; uint32_t rank[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        x[r] = y[r] = 0;
        ok[r] = cloud_px<SRC>(a, map, (int64_t)tile * TILE + r * NT + t, m, &x[r], &y[r], xyz[r]);
        const unsigned long long mask = __ballot(ok[r]);
        rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if ((t & 63) == 0) seg_n[r * (NT / 64) + wave] = (uint32_t)__popcll(mask);   // raster order: round major, wave minor
    }
    __syncthreads();
    uint32_t total = 0, seg_off[ROUNDS] = {};
#pragma unroll
    for (int sgm = 0; sgm < SEGS; sgm++) {
#pragma unroll
        for (int r = 0; r < ROUNDS; r++)
            if (sgm == r * (NT / 64) + wave) seg_off[r] = total;
        total += seg_n[sgm];
    }
    const uint8_t* vmap = a.view ? a.view + (ptrdiff_t)map * a.vmap : nullptr;
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        if (!ok[r]) continue;
        const uint32_t k = seg_off[r] + rank[r];
        pts[3 * k] = __float_as_uint(xyz[r][0]); pts[3 * k + 1] = __float_as_uint(xyz[r][1]); pts[3 * k + 2] = __float_as_uint(xyz[r][2]);
        idx[k] = (uint32_t)(y[r] * a.W + x[r]);
        if (a.colours) {
            const uint8_t* v = vmap + (ptrdiff_t)y[r] * a.vstride + (ptrdiff_t)x[r] * a.vch;
            for (int c = 0; c < a.vch; c++) col[k * a.vch + c] = v[c];
        }
    }
    __syncthreads();
    const int n = (int)min(total, (uint32_t)a.capacity - base);      // entries of this tile that fit
    store_run(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.points) + (ptrdiff_t)map * a.pmap) + (size_t)base * 3, pts, n * 3);
    if (a.index)
        store_run(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.index) + (ptrdiff_t)map * a.imap) + base, idx, n);
    if (a.colours) {
        uint8_t* c = a.colours + (ptrdiff_t)map * a.cmap + (size_t)base * a.vch;
        for (int i = t; i < n * a.vch; i += NT) c[i] = col[i];
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
int esz_of(int depth) { return depth == ADF_16S ? 2 : 4; }

const char* const RP = "reprojectImageTo3D";
const char* const PC = "pointCloud";

struct SourceMaps {                    // the arguments both calls begin with
    int n; const void* disp; int depth; ptrdiff_t stride, map_stride; int W, H;
    const adf_reproject_params* prm;
};

struct ImageCall {                     // one adf_reproject_to_3d_* call as its C entry point received it
    SourceMaps s;
    float* out; ptrdiff_t ostride, omap; int ch;
};

struct CloudCall {                     // one adf_point_cloud_* call as its C entry point received it
    SourceMaps s;
    const adf_rect* roi_arg; double z_min, z_max;
    const uint8_t* view; ptrdiff_t vstride, vmap; int vch;
    float* points; ptrdiff_t pmap; uint8_t* colours; ptrdiff_t cmap; int32_t* index; ptrdiff_t imap;
    int capacity; uint32_t* counts;
    adf_rect roi; int tiles;           // what cloud_check derives: the ROI in force and its tiles
};

// bits of a base pointer and its strides (the map stride counts only in a batch) that break an alignment of `align`
uintptr_t misaligned(int n, const void* p, ptrdiff_t stride, ptrdiff_t map_stride, int align)
{
    return ((uintptr_t)p | (uintptr_t)stride | (n > 1 ? (uintptr_t)map_stride : 0)) & (uintptr_t)(align - 1);
}

// Everything about the source maps and the parameters that can be refused without a device.
int source_check(const char* who, const SourceMaps& s)
{
    if (!s.disp || s.n < 1 || s.W < 1 || s.H < 1) return fail(ADF_EBADARG, "%s: the disparity map is empty", who);
    if (!s.prm) return fail(ADF_EBADARG, "%s: prm must not be null", who);
    if (s.depth != ADF_16S && s.depth != ADF_32F) return fail(ADF_EBADARG, "%s: disparity must be CV_16SC1 or CV_32FC1", who);
    if (s.prm->missing_mode < ADF_MISSING_NONE || s.prm->missing_mode > ADF_MISSING_VALUE)
        return fail(ADF_EBADARG, "%s: missing_mode must be ADF_MISSING_NONE, ADF_MISSING_MIN or ADF_MISSING_VALUE", who);
    if (!std::isfinite(s.prm->disp_scale)) return fail(ADF_EBADARG, "%s: disp_scale must be finite", who);
    if (s.prm->missing_mode == ADF_MISSING_VALUE && !std::isfinite(s.prm->missing_value))
        return fail(ADF_EBADARG, "%s: missing_value must be finite", who);
    if ((int64_t)s.W * s.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "%s: W*H must be below 2^31", who);
    if (misaligned(s.n, s.disp, s.stride, s.map_stride, esz_of(s.depth)))
        return fail(ADF_EBADARG, "%s: the disparity map and its strides must be aligned to its element size", who);
    if (s.stride < (ptrdiff_t)s.W * esz_of(s.depth)) return fail(ADF_ESIZE, "%s: row stride smaller than a row", who);
    return ADF_OK;
}

int image_check(const ImageCall& c)
{
    if (const int rc = source_check(RP, c.s)) return rc;
    if (!c.out) return fail(ADF_EBADARG, "%s: out must not be null", RP);
    if (c.ch != 1 && c.ch != 3) return fail(ADF_EBADARG, "%s: out_channels must be 3 (XYZ) or 1 (Z only)", RP);
    if (misaligned(c.s.n, c.out, c.ostride, c.omap, 4)) return fail(ADF_EBADARG, "%s: out and its strides must be 4-byte aligned", RP);
    if (c.ostride < (ptrdiff_t)c.s.W * c.ch * 4) return fail(ADF_ESIZE, "%s: output row stride smaller than a row", RP);
    if (!images_disjoint(c.s.n, (ptrdiff_t)c.s.W * c.ch * 4, c.s.H, c.ostride, c.omap, false))
        return fail(ADF_ESIZE, "%s: output maps of the batch overlap (map stride smaller than a map)", RP);
    return ADF_OK;
}

void set_geometry(Geometry& g, const adf_reproject_params* prm)
{
    for (int i = 0; i < 16; i++) g.Q[i] = prm->Q[i];
    g.scale = prm->disp_scale;
    g.missing = prm->missing_value;
    g.mode = prm->missing_mode;
    g.min_key = nullptr;
}

// The source side of ImageArgs for the maps from `disp` on (smap: 0 for a single map): groups of PX pixels, and whether
// base and strides allow the 8- / 16-byte loads of PX values.
ImageArgs source_args(const SourceMaps& s, const char* disp, ptrdiff_t smap)
{
    ImageArgs a = {};
    a.src = disp; a.sstride = s.stride; a.smap = smap;
    a.W = s.W; a.H = s.H;
    a.groups = (s.W + PX - 1) / PX;
    a.total = (int)((int64_t)a.groups * s.H);                        // (W * H < 2^31)
    a.vec_src = (((uintptr_t)disp | (uintptr_t)s.stride | (uintptr_t)smap) & (uintptr_t)(esz_of(s.depth) * PX - 1)) == 0;
    return a;
}

// the minimum of the nm maps of `a` into slots[0 .. nm) (ADF_MISSING_MIN)
template <class SRC> int min_run(const ImageArgs& a, unsigned nm, uint32_t* slots, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(slots, 0xff, (size_t)nm * sizeof(uint32_t), st));
    const unsigned blocks = (unsigned)(((int64_t)a.total + NT * MIN_GROUPS - 1) / (NT * MIN_GROUPS));
    hipLaunchKernelGGL((reproject_min_kernel<SRC>), dim3(blocks, nm), dim3(NT), 0, st, a, slots);
    return launched();
}

// ws: the minimum slots (adf_reproject_workspace_bytes; read with ADF_MISSING_MIN only)
template <class SRC> int image_launch(const ImageCall& c, void* ws, hipStream_t st)
{
    const SourceMaps& s = c.s;
    const char* src = static_cast<const char*>(s.disp);
    char* out = reinterpret_cast<char*>(c.out);
    ImageArgs a = source_args(s, src, s.n > 1 ? s.map_stride : 0);
    a.ostride = c.ostride; a.omap = s.n > 1 ? c.omap : 0;
    a.vec_dst = (((uintptr_t)out | (uintptr_t)a.ostride | (uintptr_t)a.omap) & 15) == 0;
    set_geometry(a.g, s.prm);
    return for_batches(s.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.src = src + (ptrdiff_t)m0 * a.smap;
        a.out = out + (ptrdiff_t)m0 * a.omap;
        if (a.g.mode == ADF_MISSING_MIN) {
            a.g.min_key = static_cast<uint32_t*>(ws) + m0;
            if (const int rc = min_run<SRC>(a, nm, static_cast<uint32_t*>(ws) + m0, st)) return rc;
        }
        const auto kernel = c.ch == 3 ? reproject_kernel<SRC, 3> : reproject_kernel<SRC, 1>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((a.total + NT - 1) / NT), nm), dim3(NT), 0, st, a);
        return launched();
    });
}

int image_launch(const ImageCall& c, void* ws, hipStream_t st)
{
    return c.s.depth == ADF_16S ? image_launch<int16_t>(c, ws, st) : image_launch<float>(c, ws, st);
}

// Sets c.roi and c.tiles.
int cloud_check(CloudCall& c)
{
    const SourceMaps& s = c.s;
    if (const int rc = source_check(PC, s)) return rc;
    if (!c.points || !c.counts) return fail(ADF_EBADARG, "%s: points and counts must not be null", PC);
    if (c.colours && !c.view) return fail(ADF_EBADARG, "%s: colours need a view", PC);
    if (c.view && c.vch != 1 && c.vch != 3) return fail(ADF_EBADARG, "%s: view_channels must be 1 or 3", PC);
    if (c.view && c.vstride < (ptrdiff_t)s.W * c.vch) return fail(ADF_ESIZE, "%s: view row stride smaller than a row", PC);
    if (c.capacity < 0) return fail(ADF_EBADARG, "%s: capacity must not be negative", PC);
    if (c.z_min != c.z_min || c.z_max != c.z_max) return fail(ADF_EBADARG, "%s: z_min and z_max must not be NaN", PC);
    if (misaligned(s.n, c.points, 0, c.pmap, 4)) return fail(ADF_EBADARG, "%s: points and its map stride must be 4-byte aligned", PC);
    if (c.index && misaligned(s.n, c.index, 0, c.imap, 4))
        return fail(ADF_EBADARG, "%s: index and its map stride must be 4-byte aligned", PC);
    c.roi = c.roi_arg ? *c.roi_arg : adf_rect{0, 0, s.W, s.H};
    const adf_rect& r = c.roi;
    if (r.x < 0 || r.y < 0 || r.width < 1 || r.height < 1 || r.x > s.W - r.width || r.y > s.H - r.height)
        return fail(ADF_ESIZE, "%s: ROI does not fit the map", PC);
    const int64_t npx = (int64_t)r.width * r.height, fit = c.capacity < npx ? c.capacity : npx;   // entries a map can write
    if (s.n > 1 && (c.pmap < fit * 12 || (c.colours && c.cmap < fit * c.vch) || (c.index && c.imap < fit * 4)))
        return fail(ADF_ESIZE, "%s: lists of the batch overlap (map stride smaller than a list)", PC);
    c.tiles = (int)((npx + TILE - 1) / TILE);
    return ADF_OK;
}

size_t min_slots_bytes(int n) { return pad_to((size_t)n * sizeof(uint32_t), 16); }

// ws: adf_point_cloud_workspace_bytes of device memory, the minimum slots and then the tile counts
template <class SRC> int cloud_launch(const CloudCall& c, void* ws, hipStream_t st)
{
    const SourceMaps& s = c.s;
    const int n = s.n;
    CloudArgs a;
    a.sstride = s.stride; a.smap = n > 1 ? s.map_stride : 0;
    a.W = s.W; a.roi = c.roi; a.npx = c.roi.width * c.roi.height; a.tiles = c.tiles;
    a.z_min = c.z_min; a.z_max = c.z_max;
    a.vstride = c.vstride; a.vmap = n > 1 ? c.vmap : 0; a.vch = c.view ? c.vch : 0;
    a.pmap = n > 1 ? c.pmap : 0; a.cmap = n > 1 ? c.cmap : 0; a.imap = n > 1 ? c.imap : 0;
    a.capacity = c.capacity;
    set_geometry(a.g, s.prm);
    uint32_t* slots = static_cast<uint32_t*>(ws);
    uint32_t* tile_counts = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + min_slots_bytes(n));
    return for_batches(n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.src = static_cast<const char*>(s.disp) + (ptrdiff_t)m0 * a.smap;
        a.view = c.view ? c.view + (ptrdiff_t)m0 * a.vmap : nullptr;
        a.points = reinterpret_cast<float*>(reinterpret_cast<char*>(c.points) + (ptrdiff_t)m0 * a.pmap);
        a.colours = c.colours ? c.colours + (ptrdiff_t)m0 * a.cmap : nullptr;
        a.index = c.index ? reinterpret_cast<int32_t*>(reinterpret_cast<char*>(c.index) + (ptrdiff_t)m0 * a.imap) : nullptr;
        a.counts = c.counts + m0;
        a.tile_counts = tile_counts + (size_t)m0 * a.tiles;
        int rc;
        if (a.g.mode == ADF_MISSING_MIN) {                           // over the whole map, not the ROI
            a.g.min_key = slots + m0;
            if ((rc = min_run<SRC>(source_args(s, a.src, a.smap), nm, slots + m0, st))) return rc;
        }
        hipLaunchKernelGGL((cloud_count_kernel<SRC>), dim3((unsigned)a.tiles, nm), dim3(NT), 0, st, a);
        if ((rc = launched())) return rc;
        hipLaunchKernelGGL(cloud_scan_kernel, dim3(nm), dim3(NT), 0, st, a);
        if ((rc = launched())) return rc;
        hipLaunchKernelGGL((cloud_write_kernel<SRC>), dim3((unsigned)a.tiles, nm), dim3(NT), 0, st, a);
        return launched();
    });
}

int cloud_launch(const CloudCall& c, void* ws, hipStream_t st)
{
    return c.s.depth == ADF_16S ? cloud_launch<int16_t>(c, ws, st) : cloud_launch<float>(c, ws, st);
}

} // namespace

extern "C" size_t adf_reproject_workspace_bytes(int n_maps)
{
    return n_maps < 1 ? 0 : (size_t)n_maps * sizeof(uint32_t);
}

extern "C" int adf_reproject_to_3d_device(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride,
                                          int W, int H, const adf_reproject_params* prm, float* out, ptrdiff_t out_stride,
                                          ptrdiff_t out_map_stride, int out_channels, void* workspace, size_t workspace_bytes,
                                          void* stream)
{
    const ImageCall c{{n_maps, disp, depth, stride, map_stride, W, H, prm}, out, out_stride, out_map_stride, out_channels};
    int rc = image_check(c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (prm->missing_mode != ADF_MISSING_MIN) return image_launch(c, nullptr, st);   // nothing to reduce: no workspace is used
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch(RP, "adf_reproject_workspace_bytes", workspace, workspace_bytes, adf_reproject_workspace_bytes(n_maps), st, blk, &ws);
    return rc ? rc : image_launch(c, ws, st);
}

extern "C" int adf_reproject_to_3d_host(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride,
                                        int W, int H, const adf_reproject_params* prm, float* out, ptrdiff_t out_stride,
                                        ptrdiff_t out_map_stride, int out_channels)
{
    const ImageCall c{{n_maps, disp, depth, stride, map_stride, W, H, prm}, out, out_stride, out_map_stride, out_channels};
    int rc = image_check(c);
    if (rc) return rc;
    // one block: the maps, the images (rows padded to 16 bytes: the vector path), the minimum slots
    const size_t srow = (size_t)W * esz_of(depth), orow = (size_t)W * out_channels * 4;
    const size_t sp = pad_to(srow, 16), op = pad_to(orow, 16), smap = sp * H, omap = op * H;
    Scratch blk;
    if ((rc = blk.take((smap + omap) * n_maps + pad_to(adf_reproject_workspace_bytes(n_maps), 16), nullptr))) return rc;
    char* ds = static_cast<char*>(blk.p);
    char* dout = ds + smap * n_maps;
    ImageCall d = c;                                                 // the same call on the staged copies
    d.s.disp = ds; d.s.stride = (ptrdiff_t)sp; d.s.map_stride = (ptrdiff_t)smap;
    d.out = reinterpret_cast<float*>(dout); d.ostride = (ptrdiff_t)op; d.omap = (ptrdiff_t)omap;
    if ((rc = copy_images(ds, sp, smap, disp, stride, map_stride, srow, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = image_launch(d, dout + omap * n_maps, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(out, out_stride, out_map_stride, dout, op, omap, orow, H, n_maps, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

extern "C" size_t adf_point_cloud_workspace_bytes(int n_maps, int W, int H)
{
    if (n_maps < 1 || W < 1 || H < 1) return 0;
    const size_t tiles = ((size_t)W * (size_t)H + TILE - 1) / TILE;
    return min_slots_bytes(n_maps) + (size_t)n_maps * tiles * sizeof(uint32_t);
}

extern "C" int adf_point_cloud_device(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                                      const adf_reproject_params* prm, const adf_rect* roi, double z_min, double z_max,
                                      const uint8_t* view, ptrdiff_t view_stride, ptrdiff_t view_map_stride, int view_channels,
                                      float* points, ptrdiff_t points_map_stride, uint8_t* colours, ptrdiff_t colours_map_stride,
                                      int32_t* index, ptrdiff_t index_map_stride, int capacity, uint32_t* counts,
                                      void* workspace, size_t workspace_bytes, void* stream)
{
    CloudCall c{{n_maps, disp, depth, stride, map_stride, W, H, prm}, roi, z_min, z_max, view, view_stride, view_map_stride, view_channels,
                points, points_map_stride, colours, colours_map_stride, index, index_map_stride, capacity, counts, {}, 0};
    int rc = cloud_check(c);
    if (rc) return rc;
    if ((uintptr_t)counts & 3) return fail(ADF_EBADARG, "%s: counts must be 4-byte aligned", PC);
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch(PC, "adf_point_cloud_workspace_bytes", workspace, workspace_bytes,
                              adf_point_cloud_workspace_bytes(n_maps, W, H), (hipStream_t)stream, blk, &ws);
    return rc ? rc : cloud_launch(c, ws, (hipStream_t)stream);
}

extern "C" int adf_point_cloud_host(int n_maps, const void* disp, int depth, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                                    const adf_reproject_params* prm, const adf_rect* roi, double z_min, double z_max,
                                    const uint8_t* view, ptrdiff_t view_stride, ptrdiff_t view_map_stride, int view_channels,
                                    float* points, ptrdiff_t points_map_stride, uint8_t* colours, ptrdiff_t colours_map_stride,
                                    int32_t* index, ptrdiff_t index_map_stride, int capacity, uint32_t* counts)
{
    CloudCall c{{n_maps, disp, depth, stride, map_stride, W, H, prm}, roi, z_min, z_max, view, view_stride, view_map_stride, view_channels,
                points, points_map_stride, colours, colours_map_stride, index, index_map_stride, capacity, counts, {}, 0};
    int rc = cloud_check(c);
    if (rc) return rc;
    if (!colours) view = nullptr;                                    // (nothing else reads it)
    // one block: the maps, the views, then per map the three lists sized for what can be written, the counts, the workspace
    const size_t npx = (size_t)c.roi.width * c.roi.height, fit = (size_t)capacity < npx ? (size_t)capacity : npx;
    const size_t srow = (size_t)W * esz_of(depth), sp = pad_to(srow, 16), smap = sp * H;
    const size_t vrow = view ? (size_t)W * view_channels : 0, vp = pad_to(vrow, 16), vmap = vp * H;
    const size_t pmap = pad_to(fit * 12, 16), cmap = colours ? pad_to(fit * view_channels, 16) : 0, imap = index ? pad_to(fit * 4, 16) : 0;
    const size_t cnt = pad_to((size_t)n_maps * sizeof(uint32_t), 16);
    Scratch blk;
    if ((rc = blk.take((smap + vmap + pmap + cmap + imap) * n_maps + cnt + adf_point_cloud_workspace_bytes(n_maps, W, H), nullptr)))
        return rc;
    char* ds = static_cast<char*>(blk.p);
    char* dv = ds + smap * n_maps;
    char* dp = dv + vmap * n_maps;
    char* dc = dp + pmap * n_maps;
    char* di = dc + cmap * n_maps;
    char* dn = di + imap * n_maps;
    CloudCall d = c;                                                 // the same call on the staged copies
    d.s.disp = ds; d.s.stride = (ptrdiff_t)sp; d.s.map_stride = (ptrdiff_t)smap;
    d.view = view ? reinterpret_cast<const uint8_t*>(dv) : nullptr; d.vstride = (ptrdiff_t)vp; d.vmap = (ptrdiff_t)vmap;
    d.points = reinterpret_cast<float*>(dp); d.pmap = (ptrdiff_t)pmap;
    d.colours = colours ? reinterpret_cast<uint8_t*>(dc) : nullptr; d.cmap = (ptrdiff_t)cmap;
    d.index = index ? reinterpret_cast<int32_t*>(di) : nullptr; d.imap = (ptrdiff_t)imap;
    d.counts = reinterpret_cast<uint32_t*>(dn);
    if ((rc = copy_images(ds, sp, smap, disp, stride, map_stride, srow, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if (view && (rc = copy_images(dv, vp, vmap, view, view_stride, view_map_stride, vrow, H, n_maps, hipMemcpyHostToDevice, nullptr)))
        return rc;
    if ((rc = cloud_launch(d, dn + cnt, nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(counts, dn, (size_t)n_maps * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    for (int k = 0; k < n_maps; k++) {                               // only what was written comes back
        const size_t got = counts[k] < fit ? counts[k] : fit;
        if (!got) continue;
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(points) + k * points_map_stride, dp + k * pmap, got * 12, hipMemcpyDeviceToHost, nullptr));
        if (colours)
            HIP_TRY(hipMemcpyAsync(colours + k * colours_map_stride, dc + k * cmap, got * view_channels, hipMemcpyDeviceToHost, nullptr));
        if (index)
            HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(index) + k * index_map_stride, di + k * imap, got * 4, hipMemcpyDeviceToHost, nullptr));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
