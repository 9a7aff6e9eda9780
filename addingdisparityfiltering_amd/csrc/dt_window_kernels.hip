// dt_window_kernels.hip -- cv::ximgproc::dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, DTF_NC, numIters) on the
// device, in the library's own definition (include/adf_wls.h, "domain transform filter, normalized convolution", is the
// statement; tests/dt_window_ref.py states it in NumPy).  Per iteration i = 1..N with radius r_i, every row and then every
// column: pixel j becomes the mean of the map over the window [lb, rb] around it, the pixels whose distance
// D = (float)steps + k * (float)(the guide's L1 differences summed over the steps) stays within r_i (<= to the left, < to the
// right), summed left to right in float32 and divided once.
//
// One kernel for both axes (dtw_pass_kernel), 2 N launches per call in one chain on the caller's stream.  A workgroup of
// 256 threads owns a tile of S scanlines by T positions along them -- 1 row x 1024 columns in the row pass, 32 columns x
// 64 rows in the column pass, so that consecutive lanes touch consecutive addresses in both -- and stages the tile plus a
// halo of R_i = floor(r_i) positions on both sides in LDS: the values as float, the guide as the 16-bit L1 difference of
// each step.  A window never reaches further than R_i steps (D >= steps), so the halo holds every window of the tile;
// positions outside the image hold clamped copies and are never read, the walks stop at the ends of the scanline.  The
// staging loads are unconditional and four per thread are in flight together: a tile is sized so that a CU's resident
// workgroups keep some 50 KiB in flight, what it takes to stream.  One thread owns one output pixel at a time (four of
// its row in the row pass, eight rows of its column in the column pass): it walks left to lb adding the steps' L as it
// goes -- one LDS read, one integer add, one product, one sum and one compare per probe, the reads of four probes issued
// together and no branch between them --, sums lb .. j, and walks right summing until D >= r_i.  The LDS image is
// [position][scanline]: the lanes of a wave read consecutive words at every step of the walk in either pass, no bank
// conflicts.  LDS is dynamic, 6 (T + 2 R_i) S bytes: 6 KiB .. 7.5 KiB in the row pass, 12 KiB .. 59.6 KiB in the column
// pass.
//
// The first row pass reads src in its depth, the last column pass writes dst in its depth; in between the map goes back
// and forth between two float planes per map in the workspace (a pass reads one plane and writes another: a window
// reaches into the neighbouring tiles).  The iteration's radius and k travel in the kernel's arguments: no device table,
// nothing to allocate, so a call with a caller workspace is capturable.  Times and what bounds them: DESIGN.md, section 26.
#include "dt_common.h"

#pragma clang fp contract(off)

using namespace adf;

namespace {

constexpr int NT = 256;                // threads of a workgroup
template <int AXIS> struct Tile;       // S scanlines by T positions along them
template <> struct Tile<0> { static constexpr int S = 1, T = 1024; };     // the row pass: a scanline is a row
template <> struct Tile<1> { static constexpr int S = 32, T = 64; };     // the column pass: a scanline is a column
constexpr size_t lds_bytes(int S, int T, int R) { return (size_t)(T + 2 * R) * S * (sizeof(float) + sizeof(unsigned short)); }
static_assert(lds_bytes(Tile<0>::S, Tile<0>::T, ADF_DT_NC_MAX_RADIUS) <= 64 * 1024 && lds_bytes(Tile<1>::S, Tile<1>::T, ADF_DT_NC_MAX_RADIUS) <= 64 * 1024,
              "a tile with the widest halo fits the LDS a workgroup may ask for without raising the kernel's limit");

struct NcArgs {
    const uint8_t* guide; ptrdiff_t guide_stride, guide_map_stride;      // bytes
    const void* in; ptrdiff_t in_stride, in_map_stride;                  // what the pass reads ...
    void* out; ptrdiff_t out_stride, out_map_stride;                     // ... and writes: never the same plane
    int W, H;
    float r, k; int R;                                                   // the iteration's radius, ss / sr, floor(r)
    unsigned tiles_p, tile0;                                             // tiles along a scanline; the first tile of the launch
};

template <int AXIS, class InT, class OutT, int CH>
__global__ void __launch_bounds__(NT) dtw_pass_kernel(NcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int S = Tile<AXIS>::S, T = Tile<AXIS>::T, QG = NT / S, PER_THREAD = T / QG;
    const int R = a.R, P = T + 2 * R;                                    // staged positions per scanline
    float* xs = reinterpret_cast<float*>(lds);                           // [P][S] the values
    unsigned short* ls = reinterpret_cast<unsigned short*>(xs + P * S);  // [P][S] L between a position and the next one
    const int n = AXIS == 0 ? a.W : a.H, ns = AXIS == 0 ? a.H : a.W;     // pixels of a scanline; scanlines
    const unsigned tile = a.tile0 + blockIdx.x;
    const int s0 = (int)(tile / a.tiles_p) * S, p0 = (int)(tile % a.tiles_p) * T;
    const ptrdiff_t m = blockIdx.y;
    const uint8_t* guide = a.guide + m * a.guide_map_stride;
    const char* in = static_cast<const char*>(a.in) + m * a.in_map_stride;
    char* out = static_cast<char*>(a.out) + m * a.out_map_stride;

    // Positions p0 - R .. p0 + T + R - 1 of scanlines s0 .. s0 + S - 1.  Coordinates outside the image are clamped into it, so
    // every load is unconditional and the loads of U entries are in flight together; what the clamped entries hold is
    // never read.
    constexpr int U = 4;
    for (int e0 = threadIdx.x; e0 < P * S; e0 += NT * U) {
        float v[U];
        unsigned ga[U], gb[U];                                           // the guide at a position and at the next one
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int e = e0 + u * NT;
            const int sl = min(s0 + e % S, ns - 1), p = min(max(p0 - R + e / S, 0), n - 1), pn = min(p + 1, n - 1);
            const ptrdiff_t row = AXIS == 0 ? sl : p, col = AXIS == 0 ? p : sl, rown = AXIS == 0 ? sl : pn, coln = AXIS == 0 ? pn : sl;
            v[u] = (float)reinterpret_cast<const InT*>(in + row * a.in_stride)[col];
            ga[u] = pixel<CH>(guide + row * a.guide_stride + col * CH);
            gb[u] = pixel<CH>(guide + rown * a.guide_stride + coln * CH);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int e = e0 + u * NT;
            if (e < P * S) {
                xs[e] = v[u];
                ls[e] = (unsigned short)l1<CH>(ga[u], gb[u]);
            }
        }
    }
    __syncthreads();

    const int s = threadIdx.x % S, sl = s0 + s;
    if (sl >= ns) return;                                                // (no barrier follows)
    const float r = a.r, k = a.k;
    constexpr int B = 4;                                                 // probes whose LDS reads are issued together
    const int last = (P - 1) * S + s;                                    // the scanline's last staged position
    for (int i = 0; i < PER_THREAD; i++) {
        const int q = threadIdx.x / S + QG * i, j = p0 + q;
        if (j >= n) break;
        const int c = (q + R) * S + s;                                   // pixel j in the LDS image
        const int left = min(R, j), right = min(R, n - 1 - j);           // the steps the scanline and the radius leave
        // A walk probes step t + 1 while it is open: B probes' reads are issued together -- past the walk's end they are
        // clamped into the scanline's image and what they return is not used -- and the chain is add, convert, multiply,
        // add, compare per probe with no branch in it.
        int t = 0;
        unsigned walked = 0;                                             // S(j - t - 1, j), exact
        bool open = left > 0;
        while (open) {                                                   // lb = j - t: the smallest a with D(a, j) <= r
            unsigned l[B];
#pragma unroll
            for (int u = 0; u < B; u++) l[u] = ls[max(c - (t + 1 + u) * S, s)];
#pragma unroll
            for (int u = 0; u < B; u++) {
                walked += l[u];
                const float ks = k * (float)walked;
                const float d = (float)(t + 1) + ks;
                open = open && d <= r;
                t += open;
                open = open && t < left;
            }
        }
        const int lb = t;
        float acc = xs[c - lb * S];
        for (int u0 = lb - 1; u0 >= 0; u0 -= B) {                        // x[lb] + ... + x[j], left to right
            float xv[B];
#pragma unroll
            for (int u = 0; u < B; u++) xv[u] = xs[c - max(u0 - u, 0) * S];
#pragma unroll
            for (int u = 0; u < B; u++) {
                const float sum = acc + xv[u];
                acc = u0 - u >= 0 ? sum : acc;
            }
        }
        t = 0;
        walked = 0;                                                      // S(j, j + t + 1)
        open = right > 0;
        while (open) {                                                   // rb = j + t: the largest b with D(j, b) < r
            unsigned l[B];
            float xv[B];
#pragma unroll
            for (int u = 0; u < B; u++) {
                const int at = min(c + (t + u) * S, last);
                l[u] = ls[at];
                xv[u] = xs[min(at + S, last)];
            }
#pragma unroll
            for (int u = 0; u < B; u++) {
                walked += l[u];
                const float ks = k * (float)walked;
                const float d = (float)(t + 1) + ks;
                open = open && d < r;
                const float sum = acc + xv[u];
                acc = open ? sum : acc;
                t += open;
                open = open && t < right;
            }
        }
        const float y = acc / (float)(lb + t + 1);
        const ptrdiff_t row = AXIS == 0 ? sl : j, col = AXIS == 0 ? j : sl;
        reinterpret_cast<OutT*>(out + row * a.out_stride)[col] = convert<OutT>(y);
    }
}

struct NcCall {                        // one call as its C entry point received it
    FilterImages im;
    double sigma_spatial, sigma_color; int mode, num_iters;
};

constexpr const char* WHO = "dtWindowFilter";

// r_i = (float)(3 sigmaH_i), i = 1..N (DT.hpp:125-128).
void radii_of(const DtParams& p, float* radii)
{
    for (int i = 1; i <= p.N; i++) radii[i - 1] = (float)(3.0 * sigma_h(p, i));
}

// What the radii depend on, refused alike by the calls and by adf_dt_nc_radii_host.
int radii_check(const char* who, double sigma_spatial, int num_iters)
{
    if (!std::isfinite(sigma_spatial) || !std::isfinite((float)sigma_spatial))
        return fail(ADF_EBADARG, "%s: sigmaSpatial must be finite (as float32 too)", who);
    if (num_iters > ADF_DT_MAX_ITERS) return fail(ADF_EBADARG, "%s: numIters must not exceed %d", who, ADF_DT_MAX_ITERS);
    return ADF_OK;
}

int nc_check(const NcCall& c)
{
    if (c.mode == ADF_DTF_IC) return fail(ADF_EBADARG, "%s: DTF_IC is not built; use ADF_DTF_NC", WHO);
    if (c.mode == ADF_DTF_RF) return fail(ADF_EBADARG, "%s: DTF_RF is the mode of adf_dt_filter_*; use ADF_DTF_NC", WHO);
    if (c.mode != ADF_DTF_NC) return fail(ADF_EBADARG, "%s: unknown mode %d", WHO, c.mode);
    const FilterImages& im = c.im;
    if (!im.guide.p || !im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: guide, src and dst must be non-NULL", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(im.src_depth) || !known_depth(im.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (im.guide_channels != 1 && im.guide_channels != 3) return fail(ADF_EBADARG, "%s: guide must have 1 or 3 channels", WHO);
    if (!std::isfinite(c.sigma_color) || !std::isfinite((float)c.sigma_color))
        return fail(ADF_EBADARG, "%s: sigmaColor must be finite (as float32 too)", WHO);
    if (int rc = radii_check(WHO, c.sigma_spatial, c.num_iters)) return rc;
    float radii[ADF_DT_MAX_ITERS];
    radii_of(clamped(c.sigma_spatial, c.sigma_color, c.num_iters), radii);
    if (!(radii[0] < (float)(ADF_DT_NC_MAX_RADIUS + 1)))
        return fail(ADF_EBADARG, "%s: the first iteration's radius %g exceeds %d pixels (sigmaSpatial is too large for numIters)", WHO,
                    (double)radii[0], ADF_DT_NC_MAX_RADIUS);
    return filter_geometry_check(WHO, im, "their depths", "src or guide");
}

// One pass of every map: `kernel` over every tile, with the iteration's radius in `a`.
template <int AXIS, class K>
int nc_launch(int n_maps, NcArgs a, K kernel, hipStream_t st)
{
    constexpr int S = Tile<AXIS>::S, T = Tile<AXIS>::T;
    const int n = AXIS == 0 ? a.W : a.H, ns = AXIS == 0 ? a.H : a.W;
    a.tiles_p = (unsigned)((n + T - 1) / T);
    const uint64_t tiles = (uint64_t)a.tiles_p * (uint64_t)((ns + S - 1) / S);    // at most W * H: 32 bits
    constexpr uint64_t PER_LAUNCH = 1u << 22;                            // (a grid's threads stay below 2^31)
    const size_t lds = lds_bytes(S, T, a.R);
    const NcArgs a0 = a;
    return for_batches(n_maps, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.guide = a0.guide + (ptrdiff_t)m0 * a0.guide_map_stride;
        a.in = static_cast<const char*>(a0.in) + (ptrdiff_t)m0 * a0.in_map_stride;
        a.out = static_cast<char*>(a0.out) + (ptrdiff_t)m0 * a0.out_map_stride;
        for (uint64_t t0 = 0; t0 < tiles; t0 += PER_LAUNCH) {
            a.tile0 = (unsigned)t0;
            hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(tiles - t0, PER_LAUNCH), nm), dim3(NT), lds, st, a);
        }
        return launched();
    });
}

template <int CH>
int nc_passes(const NcCall& c, NcArgs a, void* ws, hipStream_t st)
{
    const FilterImages& im = c.im;
    const DtParams p = clamped(c.sigma_spatial, c.sigma_color, c.num_iters);
    float radii[ADF_DT_MAX_ITERS];
    radii_of(p, radii);
    a.k = p.ss / p.sr;
    const ptrdiff_t prow = (ptrdiff_t)im.W * 4, pmap = prow * im.H;
    float* plane_a = static_cast<float*>(ws);                            // what the row passes write
    float* plane_b = plane_a + (size_t)im.n * im.W * im.H;               // what the column passes but the last write
    const NcArgs user = a;
    for (int i = 0; i < p.N; i++) {
        a.r = radii[i];
        a.R = (int)std::floor(radii[i]);
        a.out = plane_a; a.out_stride = prow; a.out_map_stride = pmap;
        int rc;
        if (i == 0) {                                                    // the first row pass reads src in its depth
            a.in = user.in; a.in_stride = user.in_stride; a.in_map_stride = user.in_map_stride;
            rc = im.src_depth == ADF_8U    ? nc_launch<0>(im.n, a, dtw_pass_kernel<0, uint8_t, float, CH>, st)
                 : im.src_depth == ADF_16S ? nc_launch<0>(im.n, a, dtw_pass_kernel<0, int16_t, float, CH>, st)
                                           : nc_launch<0>(im.n, a, dtw_pass_kernel<0, float, float, CH>, st);
        } else {
            a.in = plane_b; a.in_stride = prow; a.in_map_stride = pmap;
            rc = nc_launch<0>(im.n, a, dtw_pass_kernel<0, float, float, CH>, st);
        }
        if (rc) return rc;
        a.in = plane_a; a.in_stride = prow; a.in_map_stride = pmap;
        if (i == p.N - 1) {                                              // the last column pass writes dst in its depth
            a.out = user.out; a.out_stride = user.out_stride; a.out_map_stride = user.out_map_stride;
            rc = im.dst_depth == ADF_8U    ? nc_launch<1>(im.n, a, dtw_pass_kernel<1, float, uint8_t, CH>, st)
                 : im.dst_depth == ADF_16S ? nc_launch<1>(im.n, a, dtw_pass_kernel<1, float, int16_t, CH>, st)
                                           : nc_launch<1>(im.n, a, dtw_pass_kernel<1, float, float, CH>, st);
        } else {
            a.out = plane_b;
            rc = nc_launch<1>(im.n, a, dtw_pass_kernel<1, float, float, CH>, st);
        }
        if (rc) return rc;
    }
    return ADF_OK;
}

// ws: adf_dt_window_filter_workspace_bytes of device memory, two float planes per map
int nc_run(const NcCall& c, void* ws, hipStream_t st)
{
    const FilterImages& im = c.im;
    NcArgs a{};
    a.guide = static_cast<const uint8_t*>(im.guide.p); a.guide_stride = im.guide.stride; a.guide_map_stride = im.guide.map_stride;
    a.in = im.src.p; a.in_stride = im.src.stride; a.in_map_stride = im.src.map_stride;
    a.out = im.dst.p; a.out_stride = im.dst.stride; a.out_map_stride = im.dst.map_stride;
    a.W = im.W; a.H = im.H;
    return im.guide_channels == 3 ? nc_passes<3>(c, a, ws, st) : nc_passes<1>(c, a, ws, st);
}

NcCall call_of(int n_maps, const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
               int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters)
{
    return NcCall{{n_maps, W, H, image_of(guide, guide_stride, guide_map_stride), guide_channels, image_of(src, src_stride, src_map_stride), src_depth,
                   image_of(dst, dst_stride, dst_map_stride), dst_depth, {}}, sigma_spatial, sigma_color, mode, num_iters};
}

} // namespace

extern "C" size_t adf_dt_window_filter_workspace_bytes(int n_maps, int W, int H)
{
    if (n_maps < 1 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) return 0;
    return 2 * (size_t)n_maps * (size_t)W * (size_t)H * sizeof(float);
}

extern "C" int adf_dt_nc_radii_host(double sigma_spatial, int num_iters, float* radii)
{
    if (!radii) return fail(ADF_EBADARG, "adf_dt_nc_radii_host: radii is NULL");
    if (int rc = radii_check("adf_dt_nc_radii_host", sigma_spatial, num_iters)) return rc;
    radii_of(clamped(sigma_spatial, 1.0, num_iters), radii);
    return ADF_OK;
}

extern "C" int adf_dt_window_filter_device(int n_maps,
                                           const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                           const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                           void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                           int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters,
                                           void* workspace, size_t workspace_bytes, void* stream)
{
    const NcCall c = call_of(n_maps, guide, guide_stride, guide_map_stride, guide_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, sigma_spatial, sigma_color, mode, num_iters);
    int rc = nc_check(c);
    if (rc) return rc;
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch(WHO, "adf_dt_window_filter_workspace_bytes", workspace, workspace_bytes,
                              adf_dt_window_filter_workspace_bytes(n_maps, W, H), (hipStream_t)stream, blk, &ws);
    return rc ? rc : nc_run(c, ws, (hipStream_t)stream);
}

extern "C" int adf_dt_window_filter_host(int n_maps,
                                         const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                         const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                         void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                         int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters)
{
    const NcCall c = call_of(n_maps, guide, guide_stride, guide_map_stride, guide_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, sigma_spatial, sigma_color, mode, num_iters);
    int rc = nc_check(c);
    if (rc) return rc;
    // the workspace: the two float planes per map
    return staged_call(c.im, adf_dt_window_filter_workspace_bytes(n_maps, W, H), [&](const FilterImages& staged, void* ws, hipStream_t st) {
        return nc_run(NcCall{staged, c.sigma_spatial, c.sigma_color, c.mode, c.num_iters}, ws, st);   // the same call on the staged images
    });
}
