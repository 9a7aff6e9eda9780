// dt_filter_kernels.hip -- cv::ximgproc::dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, DTF_RF, numIters) on the
// device, in the library's own definition (include/adf_wls.h, "domain transform filter", is the statement;
// tests/dt_ref.py states it in NumPy).  Per iteration i = 1..N, with A = row i of the feedback table and L the L1
// difference of two neighbouring guide pixels:
//
//   row pass     every row left to right  x[j] = x[j] + A[L(j-1,j)] (x[j-1] - x[j]), then right to left
//                x[j] = x[j] + A[L(j,j+1)] (x[j+1] - x[j])                                            (dt_row_kernel)
//   column pass  the same down and then up every column                                              (dt_col_kernel)
//
// The order of the statement IS the definition, so one lane owns one scanline and walks it; subtraction, product and sum
// round separately (contraction off).  Both sweeps of a pass run in one launch: 2 N launches per call.
//
// Row pass: a workgroup of four waves owns 64 rows and moves them through LDS in tiles of TC columns.  A tile is loaded
// with the lane on the COLUMN (a wave instruction reads 256 contiguous bytes of one row; each wave moves 16 of the rows,
// its 48 loads unconditional and in flight together), swept by the first wave with the lane on the ROW, stored as it was
// loaded.  The float tile has a pitch of TC + 1 words: the transposed ds_read_b32 / ds_write_b32 of lane r at column c
// hits bank (r + c) mod 32, distinct within each 32-lane half, and the row-wise accesses are contiguous.  L is formed
// while staging, from the guide bytes of the two pixels, and kept as 16 bits with a pitch of TC + 2 (33 words: bank
// (r + c / 2) mod 32 on the transposed read).  The loads of the next tile are issued behind the stores of this one, so
// one barrier waits for both.  The backward sweep re-reads the tiles the forward sweep wrote, last first; every entry
// a sweep uses is written and read again by the same thread.
// Column pass: the lane is the column, every access is coalesced as it stands; loads run PF rows ahead of the chain.
// In both passes the table reads of a block of steps are issued together, off the chain, and the chain itself is one
// subtract, one multiply and one add per step with no branch in it.
// The table row of the iteration travels in the kernel's arguments (1 KiB for a gray guide, 3 KiB for 3 channels) and is
// copied to LDS: no device table, no upload, nothing to allocate, so a call with a caller workspace is capturable.
//
// The first row pass reads src in its depth, the last column pass's upward sweep writes dst in its depth; in between
// the map is one float plane per map in the workspace.  LDS per workgroup: 24.5 KiB of tiles + the table row (row pass),
// the table row (column pass).  Times and what bounds them: DESIGN.md, section 22.
#include "dt_common.h"

#pragma clang fp contract(off)

using namespace adf;

namespace {

constexpr int TC = 64;                 // columns of a row-pass tile
constexpr int XP = TC + 1;             // pitch of the float tile, words
constexpr int LP = TC + 2;             // pitch of the L tile, 16-bit entries
constexpr int RT = 256, RW = 64 / (RT / 64);   // threads of a row-pass workgroup; rows of a tile each of its waves moves
constexpr int PF = 16;                 // rows the column pass loads ahead
constexpr int levels_of(int ch) { return 255 * ch + 1; }

template <int CH> struct DtRow { float a[levels_of(CH)]; };            // one iteration's table row, a kernel argument
static_assert(sizeof(DtRow<3>) + 128 <= 4096, "the table row and DtArgs fit a kernel's arguments");

struct DtArgs {
    const uint8_t* guide; ptrdiff_t guide_stride, guide_map_stride;      // bytes
    const void* src; ptrdiff_t src_stride, src_map_stride;               // row pass: what the forward sweep reads
    void* dst; ptrdiff_t dst_stride, dst_map_stride;                     // column pass: what the upward sweep writes
    float* plane;                                                        // [map][H][W]
    int W, H;
};

// The wave's index in its workgroup, as the scalar it is: what is addressed by it gets a scalar base.
__device__ __forceinline__ int wave_of_group() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

template <int CH> __device__ __forceinline__ void table_to_lds(float* A, const DtRow<CH>& row)
{
    for (int i = threadIdx.x; i < levels_of(CH); i += blockDim.x) A[i] = row.a[i];
    __syncthreads();
}

// Columns [c0, c0 + TC) of rows [r0, r0 + 64) on their way into the tiles, lane on the column, wave w on rows 16 w ..
// 16 w + 15: fetch() issues the loads -- the values, and the guide pixels at columns j - 1 and j, j = column + off --
// and commit() writes xt, the values as floats, and lt, the guide's L between those two columns.  Coordinates outside the
// image are clamped into it, so every load is unconditional and the 48 of a thread are in flight together; what the
// clamped entries hold is never used (the sweeps and unstage() stay inside the image).
struct Fetched { float v[RW]; unsigned pa[RW], pb[RW]; };

template <class T, int CH>
__device__ __forceinline__ void fetch(Fetched& f, const char* in, ptrdiff_t in_stride, const uint8_t* guide, ptrdiff_t guide_stride,
                                      int r0, int c0, int off, int W, int H)
{
    const int lane = threadIdx.x & 63, w = wave_of_group(), col = min(c0 + lane, W - 1);
    const int ja = min(max(c0 + lane + off, 1), W - 1), jb = max(ja - 1, 0);
#pragma unroll
    for (int k = 0; k < RW; k++) {
        const int row = min(r0 + w * RW + k, H - 1);
        f.v[k] = (float)reinterpret_cast<const T*>(in + (ptrdiff_t)row * in_stride)[col];
        const uint8_t* g = guide + (ptrdiff_t)row * guide_stride;
        f.pa[k] = pixel<CH>(g + (ptrdiff_t)ja * CH);
        f.pb[k] = pixel<CH>(g + (ptrdiff_t)jb * CH);
    }
}

template <int CH> __device__ __forceinline__ void commit(const Fetched& f, float* xt, unsigned short* lt)
{
    const int lane = threadIdx.x & 63, w = wave_of_group();
#pragma unroll
    for (int k = 0; k < RW; k++) {
        xt[(w * RW + k) * XP + lane] = f.v[k];
        lt[(w * RW + k) * LP + lane] = (unsigned short)l1<CH>(f.pb[k], f.pa[k]);
    }
}

__device__ __forceinline__ void unstage(const float* xt, float* plane, int r0, int c0, int W, int H)
{
    const int lane = threadIdx.x & 63, w = wave_of_group(), col = c0 + lane;
    if (col >= W) return;
#pragma unroll
    for (int k = 0; k < RW; k++) {
        const int rr = w * RW + k;
        if (r0 + rr < H) plane[(size_t)(r0 + rr) * W + col] = xt[rr * XP + lane];
    }
}

// One lane's TC steps through its row of the tiles, DIR = 1 from column 0 up, -1 from column TC - 1 down: at image
// columns j in [lo, hi] x = x + A[L] (carry - x), elsewhere x stays (the sweep's first column, and the clamped entries
// past the image, whose values nothing uses); the carry is the x of the step before.  No branch: SB steps' reads are
// issued together, the chain is subtract, multiply, add and a select.
template <int DIR>
__device__ __forceinline__ float sweep_tile(float* xr, const unsigned short* lr, const float* A, float carry, int c0, int lo, int hi)
{
    constexpr int SB = 16;
    for (int b = 0; b < TC; b += SB) {
        float xs[SB], as[SB];
#pragma unroll
        for (int k = 0; k < SB; k++) {
            const int c = DIR > 0 ? b + k : TC - 1 - b - k;
            xs[k] = xr[c];
            as[k] = A[lr[c]];
        }
#pragma unroll
        for (int k = 0; k < SB; k++) {
            const int c = DIR > 0 ? b + k : TC - 1 - b - k, j = c0 + c;
            const float d = carry - xs[k];
            const float p = as[k] * d;
            const float nx = xs[k] + p;
            carry = (j >= lo && j <= hi) ? nx : xs[k];
            xr[c] = carry;
        }
    }
    return carry;
}

template <class InT, int CH>
__global__ void __launch_bounds__(RT) dt_row_kernel(DtArgs a, DtRow<CH> row)
{
    __shared__ float A[levels_of(CH)];
    __shared__ float xt[64 * XP];
    __shared__ unsigned short lt[64 * LP];
    table_to_lds<CH>(A, row);
    const int lane = threadIdx.x & 63, W = a.W, H = a.H, r0 = (int)blockIdx.x * 64;
    const bool sweeper = threadIdx.x < 64;                               // the wave whose lanes walk the rows
    const ptrdiff_t m = blockIdx.y;
    const uint8_t* guide = a.guide + m * a.guide_map_stride;
    const char* src = static_cast<const char*>(a.src) + m * a.src_map_stride;
    float* plane = a.plane + (size_t)m * W * H;
    const int ntile = (W + TC - 1) / TC;
    float* xr = xt + lane * XP;                                          // this lane's row of the tiles
    const unsigned short* lr = lt + lane * LP;

    // A tile: commit what was fetched, sweep it, store it, and fetch the next one behind the stores, so that the barrier
    // which frees the tiles waits for loads and stores together.  Every entry a sweep uses is fetched by the thread that
    // stored it (only clamped entries, which nothing uses, read what another thread wrote).
    const char* pl = reinterpret_cast<const char*>(plane);
    const ptrdiff_t pl_stride = (ptrdiff_t)W * 4;
    Fetched f;
    float carry = 0.0f;
    fetch<InT, CH>(f, src, a.src_stride, guide, a.guide_stride, r0, 0, 0, W, H);
    for (int t = 0; t < ntile; t++) {                                    // left to right: lt[c] = L(j - 1, j)
        const int c0 = t * TC;
        commit<CH>(f, xt, lt);
        __syncthreads();
        if (sweeper) carry = sweep_tile<1>(xr, lr, A, carry, c0, 1, W - 1);
        __syncthreads();
        unstage(xt, plane, r0, c0, W, H);
        if (t + 1 < ntile) fetch<InT, CH>(f, src, a.src_stride, guide, a.guide_stride, r0, c0 + TC, 0, W, H);
        else fetch<float, CH>(f, pl, pl_stride, guide, a.guide_stride, r0, c0, 1, W, H);    // the way back starts here
        __syncthreads();
    }
    for (int t = ntile - 1; t >= 0; t--) {                               // right to left: lt[c] = L(j, j + 1)
        const int c0 = t * TC;
        commit<CH>(f, xt, lt);
        __syncthreads();
        if (sweeper) carry = sweep_tile<-1>(xr, lr, A, carry, c0, 0, W - 2);
        __syncthreads();
        unstage(xt, plane, r0, c0, W, H);
        if (t > 0) fetch<float, CH>(f, pl, pl_stride, guide, a.guide_stride, r0, c0 - TC, 1, W, H);
        __syncthreads();
    }
}

// `count` steps of one column's sweep, step t at row first + dir * t: x = x + A[L(row, the row before it)] (carry - x),
// handed to store(row, x).  Loads run PF rows ahead of the chain.  carry / gcarry: the value and guide pixel of the row
// the sweep comes from, updated.
template <int CH, class Store>
__device__ __forceinline__ void col_sweep(const float* x, ptrdiff_t xs, const uint8_t* g, ptrdiff_t gs, int first, int dir, int count,
                                          const float* A, float& carry, unsigned& gcarry, Store&& store)
{
    if (count < 1) return;
    float nx[PF]; unsigned ng[PF];
    auto load = [&](int t0) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const ptrdiff_t i = first + dir * min(t0 + k, count - 1);    // clamped: always a row of the sweep
            nx[k] = x[i * xs];
            ng[k] = pixel<CH>(g + i * gs);
        }
    };
    load(0);
    for (int t0 = 0; t0 < count; t0 += PF) {
        float cx[PF], as[PF]; unsigned cg[PF];
#pragma unroll
        for (int k = 0; k < PF; k++) { cx[k] = nx[k]; cg[k] = ng[k]; }
        load(t0 + PF);
#pragma unroll
        for (int k = 0; k < PF; k++) as[k] = A[l1<CH>(k ? cg[k - 1] : gcarry, cg[k])];   // off the chain, issued together
        if (t0 + PF <= count) {
#pragma unroll
            for (int k = 0; k < PF; k++) {
                carry = cx[k] + as[k] * (carry - cx[k]);
                store(first + dir * (t0 + k), carry);
            }
            gcarry = cg[PF - 1];
        } else {
#pragma unroll
            for (int k = 0; k < PF; k++) {
                if (t0 + k < count) {
                    carry = cx[k] + as[k] * (carry - cx[k]);
                    store(first + dir * (t0 + k), carry);
                    gcarry = cg[k];
                }
            }
        }
    }
}

template <class OutT, int CH>
__global__ void __launch_bounds__(64) dt_col_kernel(DtArgs a, DtRow<CH> row)
{
    __shared__ float A[levels_of(CH)];
    table_to_lds<CH>(A, row);
    const int W = a.W, H = a.H, col = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (col >= W) return;                                                // (no barrier follows)
    const ptrdiff_t m = blockIdx.y;
    const uint8_t* g = a.guide + m * a.guide_map_stride + (ptrdiff_t)col * CH;
    float* x = a.plane + (size_t)m * W * H + col;
    char* out = static_cast<char*>(a.dst) + m * a.dst_map_stride;

    float carry = x[0];
    unsigned gcarry = pixel<CH>(g);
    col_sweep<CH>(x, W, g, a.guide_stride, 1, 1, H - 1, A, carry, gcarry,                      // down
                  [&](int i, float v) { x[(ptrdiff_t)i * W] = v; });
    auto put = [&](int i, float v) { reinterpret_cast<OutT*>(out + (ptrdiff_t)i * a.dst_stride)[col] = convert<OutT>(v); };
    put(H - 1, carry);
    col_sweep<CH>(x, W, g, a.guide_stride, H - 2, -1, H - 1, A, carry, gcarry, put);           // up
}

struct DtCall {                        // one call as its C entry point received it
    FilterImages im;
    double sigma_spatial, sigma_color; int mode, num_iters;
};

constexpr const char* WHO = "dtFilter";

// What the table depends on, refused alike by the calls and by adf_dt_rf_table_host.
int params_check(const char* who, double sigma_spatial, double sigma_color, int num_iters, int guide_channels)
{
    if (guide_channels != 1 && guide_channels != 3) return fail(ADF_EBADARG, "%s: guide must have 1 or 3 channels", who);
    if (!std::isfinite(sigma_spatial) || !std::isfinite(sigma_color) || !std::isfinite((float)sigma_spatial) || !std::isfinite((float)sigma_color))
        return fail(ADF_EBADARG, "%s: sigmaSpatial and sigmaColor must be finite (as float32 too)", who);
    if (num_iters > ADF_DT_MAX_ITERS) return fail(ADF_EBADARG, "%s: numIters must not exceed %d", who, ADF_DT_MAX_ITERS);
    return ADF_OK;
}

// The feedback table, N rows of 255 * channels + 1 entries (include/adf_wls.h: A_i[L]).
void build_table(const DtParams& p, int ch, float* table)
{
    const int levels = levels_of(ch);
    const float k = p.ss / p.sr;
    for (int i = 1; i <= p.N; i++) {
        const double a = -std::sqrt(2.0 / 3.0) / sigma_h(p, i);
        for (int L = 0; L < levels; L++) {
            const float kl = k * (float)L;
            const float d = 1.0f + kl;
            table[(size_t)(i - 1) * levels + L] = (float)std::exp(a * (double)d);
        }
    }
}

// The calling thread's last table: a stream of calls with one set of parameters builds it once.
const float* table_of(const DtParams& p, int ch)
{
    struct Last { DtParams p{0.0f, 0.0f, 0}; int ch = 0; std::vector<float> t; };
    static thread_local Last last;
    if (last.ch != ch || last.p.N != p.N || last.p.ss != p.ss || last.p.sr != p.sr) {
        last.t.resize((size_t)p.N * levels_of(ch));
        build_table(p, ch, last.t.data());
        last.p = p; last.ch = ch;
    }
    return last.t.data();
}

int dt_check(const DtCall& c)
{
    if (c.mode == ADF_DTF_NC || c.mode == ADF_DTF_IC)
        return fail(ADF_EBADARG, "%s: DTF_NC and DTF_IC are not built; use ADF_DTF_RF", WHO);
    if (c.mode != ADF_DTF_RF) return fail(ADF_EBADARG, "%s: unknown mode %d", WHO, c.mode);
    const FilterImages& im = c.im;
    if (!im.guide.p || !im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: guide, src and dst must be non-NULL", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(im.src_depth) || !known_depth(im.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (int rc = params_check(WHO, c.sigma_spatial, c.sigma_color, c.num_iters, im.guide_channels)) return rc;
    return filter_geometry_check(WHO, im, "their depths", "src or guide");
}

// One pass of every map: `kernel` over grid_x groups of 64 scanlines, with the iteration's table row.
template <int CH, class K>
int dt_launch(const DtCall& c, DtArgs a, K kernel, unsigned grid_x, unsigned threads, const float* table_row, hipStream_t st)
{
    DtRow<CH> row;
    std::copy(table_row, table_row + levels_of(CH), row.a);
    const DtArgs a0 = a;
    return for_batches(c.im.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.guide = a0.guide + (ptrdiff_t)m0 * a0.guide_map_stride;
        a.src = static_cast<const char*>(a0.src) + (ptrdiff_t)m0 * a0.src_map_stride;
        a.dst = static_cast<char*>(a0.dst) + (ptrdiff_t)m0 * a0.dst_map_stride;
        a.plane = a0.plane + (size_t)m0 * c.im.W * c.im.H;
        hipLaunchKernelGGL(kernel, dim3(grid_x, nm), dim3(threads), 0, st, a, row);
        return launched();
    });
}

template <int CH>
int dt_passes(const DtCall& c, const DtArgs& user, hipStream_t st)
{
    const DtParams p = clamped(c.sigma_spatial, c.sigma_color, c.num_iters);
    const float* table = table_of(p, CH);
    const unsigned rows_x = (unsigned)((c.im.H + 63) / 64), cols_x = (unsigned)((c.im.W + 63) / 64);
    const ptrdiff_t prow = (ptrdiff_t)c.im.W * 4, pmap = prow * c.im.H;
    for (int i = 0; i < p.N; i++) {
        const float* row = table + (size_t)i * levels_of(CH);
        DtArgs a = user;
        int rc;
        if (i == 0) {                                                    // the first row pass reads src in its depth
            rc = c.im.src_depth == ADF_8U    ? dt_launch<CH>(c, a, dt_row_kernel<uint8_t, CH>, rows_x, RT, row, st)
                 : c.im.src_depth == ADF_16S ? dt_launch<CH>(c, a, dt_row_kernel<int16_t, CH>, rows_x, RT, row, st)
                                             : dt_launch<CH>(c, a, dt_row_kernel<float, CH>, rows_x, RT, row, st);
        } else {
            a.src = a.plane; a.src_stride = prow; a.src_map_stride = pmap;
            rc = dt_launch<CH>(c, a, dt_row_kernel<float, CH>, rows_x, RT, row, st);
        }
        if (rc) return rc;
        if (i == p.N - 1) {                                              // the last column pass writes dst in its depth
            rc = c.im.dst_depth == ADF_8U    ? dt_launch<CH>(c, a, dt_col_kernel<uint8_t, CH>, cols_x, 64, row, st)
                 : c.im.dst_depth == ADF_16S ? dt_launch<CH>(c, a, dt_col_kernel<int16_t, CH>, cols_x, 64, row, st)
                                             : dt_launch<CH>(c, a, dt_col_kernel<float, CH>, cols_x, 64, row, st);
        } else {
            a.dst = a.plane; a.dst_stride = prow; a.dst_map_stride = pmap;
            rc = dt_launch<CH>(c, a, dt_col_kernel<float, CH>, cols_x, 64, row, st);
        }
        if (rc) return rc;
    }
    return ADF_OK;
}

// ws: adf_dt_filter_workspace_bytes of device memory, one float plane per map
int dt_run(const DtCall& c, void* ws, hipStream_t st)
{
    const FilterImages& im = c.im;
    DtArgs a{};
    a.guide = static_cast<const uint8_t*>(im.guide.p); a.guide_stride = im.guide.stride; a.guide_map_stride = im.guide.map_stride;
    a.src = im.src.p; a.src_stride = im.src.stride; a.src_map_stride = im.src.map_stride;
    a.dst = im.dst.p; a.dst_stride = im.dst.stride; a.dst_map_stride = im.dst.map_stride;
    a.plane = static_cast<float*>(ws);
    a.W = im.W; a.H = im.H;
    return im.guide_channels == 3 ? dt_passes<3>(c, a, st) : dt_passes<1>(c, a, st);
}

DtCall call_of(int n_maps, const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
               int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters)
{
    return DtCall{{n_maps, W, H, image_of(guide, guide_stride, guide_map_stride), guide_channels, image_of(src, src_stride, src_map_stride), src_depth,
                   image_of(dst, dst_stride, dst_map_stride), dst_depth, {}}, sigma_spatial, sigma_color, mode, num_iters};
}

} // namespace

extern "C" size_t adf_dt_filter_workspace_bytes(int n_maps, int W, int H)
{
    if (n_maps < 1 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) return 0;
    return (size_t)n_maps * (size_t)W * (size_t)H * sizeof(float);
}

extern "C" int adf_dt_rf_table_host(double sigma_spatial, double sigma_color, int num_iters, int guide_channels, float* table)
{
    if (!table) return fail(ADF_EBADARG, "adf_dt_rf_table_host: table is NULL");
    if (int rc = params_check("adf_dt_rf_table_host", sigma_spatial, sigma_color, num_iters, guide_channels)) return rc;
    build_table(clamped(sigma_spatial, sigma_color, num_iters), guide_channels, table);
    return ADF_OK;
}

extern "C" int adf_dt_filter_device(int n_maps,
                                    const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                    const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                    void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                    int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    const DtCall c = call_of(n_maps, guide, guide_stride, guide_map_stride, guide_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, sigma_spatial, sigma_color, mode, num_iters);
    int rc = dt_check(c);
    if (rc) return rc;
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch(WHO, "adf_dt_filter_workspace_bytes", workspace, workspace_bytes,
                              adf_dt_filter_workspace_bytes(n_maps, W, H), (hipStream_t)stream, blk, &ws);
    return rc ? rc : dt_run(c, ws, (hipStream_t)stream);
}

extern "C" int adf_dt_filter_host(int n_maps,
                                  const uint8_t* guide, ptrdiff_t guide_stride, ptrdiff_t guide_map_stride, int guide_channels,
                                  const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                  void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                  int W, int H, double sigma_spatial, double sigma_color, int mode, int num_iters)
{
    const DtCall c = call_of(n_maps, guide, guide_stride, guide_map_stride, guide_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, sigma_spatial, sigma_color, mode, num_iters);
    int rc = dt_check(c);
    if (rc) return rc;
    // the workspace: the float planes
    return staged_call(c.im, adf_dt_filter_workspace_bytes(n_maps, W, H), [&](const FilterImages& staged, void* ws, hipStream_t st) {
        return dt_run(DtCall{staged, c.sigma_spatial, c.sigma_color, c.mode, c.num_iters}, ws, st);   // the same call on the staged images
    });
}
