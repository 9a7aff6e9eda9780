// conf_kernels.hip -- confidence-map half of DisparityWLSFilter::filter for gfx950: the discontinuity, left-sweep and
// band kernels, the fill outside the ROI and the merged preparation launch.  (The two-kernel stage's second kernel,
// lrc_prologue_kernel, is in rhs_prologue.hip.)
//
//   discontinuity_kernel : DF.cpp:161-194 (box mean / mean of squares on the ROI copy,
//                          BORDER_REFLECT_101) + DF.cpp:343-373 (variance -> roll-off map)
//   outside_kernel       : out = 16*(min_disp-1) = -16 and confidence 0 outside the ROI
//                          (DF.cpp:149,254,284; :187-190)
//
// All of this is integer / elementwise float work: HBM-bound, no MFMA.  Arithmetic that must
// match the CPU restatement bit for bit is written as separate roundings (contraction off).
#include "adf_internal.h"
#include <mutex>
#include <cstdlib>
#include <type_traits>
#include "prep_bodies.h"

#pragma clang fp contract(off)

namespace adf {

namespace {

using namespace tile;
// streaming outputs are written once and read by a later kernel after gigabytes of other traffic
#define ADF_ST(p, v) __builtin_nontemporal_store((v), (p))
constexpr int MAX_RADIUS = 40;

// One value of a discontinuity map (DF.cpp:369-370) from a window's exact sum s1 and square sum; scale = 1 / window
// area.  sum2() returns the square sum as a double, formed from each kernel's own representation; it is a callable so
// that it is formed where the formula uses it ("Confidence kernels").
template <class Sum2>
__device__ __forceinline__ float disc_value(int s1, Sum2 sum2, double scale, float roll_off)
{
    const float mean = (float)((double)s1 * scale);
    const float sq = (float)(sum2() * scale);
    const float variance = sq - mean * mean;          // DF.cpp:369
    const float v = 1.0f - roll_off * variance;       // DF.cpp:370
    return v < 0.0f ? 0.0f : v;
}

// ---------------------------------------------------------------------------------------
// Depth-discontinuity maps.  One block = one TX x TY tile of ROI outputs of one view of one pair
// (blockIdx.z = 2*pair + view).  LDS: int16 input tile with halo, then horizontal window sums
// (int32 sum, int64 sum of squares; both exact), then vertical window sums, both by sliding
// windows of 8 outputs.  No integer division anywhere: all index maps are 2-D loops.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) discontinuity_kernel(DiscArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int r = a.radius, k = 2 * r + 1;
    const int IH = TY + 2 * r, IW = TX + 2 * r;
    const int IWP = IW | 1;                                              // odd pitch (in int16)
    long long* h2 = reinterpret_cast<long long*>(smem);                  // [IH][TX]
    int* h1 = reinterpret_cast<int*>(h2 + (size_t)IH * TX);              // [IH][TX]
    int16_t* in = reinterpret_cast<int16_t*>(h1 + (size_t)IH * TX);      // [IH][IWP]

    const int tid = threadIdx.x, tx = tid & (TX - 1), ty = tid / TX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int view = a.only_view >= 0 ? a.only_view : (int)(blockIdx.z & 1);
    const size_t pz = a.only_view >= 0 ? blockIdx.z : (blockIdx.z >> 1);
    const char* base = reinterpret_cast<const char*>(a.disp[view]) + (ptrdiff_t)pz * a.pair_stride[view];
    const int rx = a.rx[view];

    for (int yy = ty; yy < IH; yy += NT / TX) {
        const int gy = reflect101(y0 + yy - r, a.rh);
        const int16_t* row = reinterpret_cast<const int16_t*>(base + (ptrdiff_t)(a.ry + gy) * a.stride[view]) + rx;
        for (int xx = tx; xx < IW; xx += TX)
            in[yy * IWP + xx] = row[reflect101(x0 + xx - r, a.rw)];
    }
    __syncthreads();

    // horizontal sums: work item = (row, segment of 8 outputs); 8 segments per row
    for (int item = tid; item < IH * 8; item += NT) {
        const int yy = item >> 3, xs = (item & 7) * 8;
        const int16_t* p = in + yy * IWP + xs;
        int s1 = 0; long long s2 = 0;
        for (int q = 0; q < k; q++) { const int v = p[q]; s1 += v; s2 += (long long)(v * v); }
        int* o1 = h1 + yy * TX + xs; long long* o2 = h2 + yy * TX + xs;
        o1[0] = s1; o2[0] = s2;
#pragma unroll
        for (int i = 1; i < 8; i++) {
            const int va = p[i + k - 1], vb = p[i - 1];
            s1 += va - vb; s2 += (long long)(va * va - vb * vb);
            o1[i] = s1; o2[i] = s2;
        }
    }
    __syncthreads();

    // vertical sums: thread = (column, segment of 8 rows)
    {
        const int ys = ty * 8;
        const double scale = 1.0 / ((double)k * (double)k);
        int s1 = 0; long long s2 = 0;
        for (int q = 0; q < k; q++) { s1 += h1[(ys + q) * TX + tx]; s2 += h2[(ys + q) * TX + tx]; }
        float* dst = a.dst[view] + pz * a.frame;
        const int gx = x0 + tx;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i > 0) {
                s1 += h1[(ys + i + k - 1) * TX + tx] - h1[(ys + i - 1) * TX + tx];
                s2 += h2[(ys + i + k - 1) * TX + tx] - h2[(ys + i - 1) * TX + tx];
            }
            const int gy = y0 + ys + i;
            if (gy < a.rh && gx < a.rw) {
                dst[(size_t)(a.ry + gy) * a.W + rx + gx] = disc_value(s1, [=] { return (double)s2; }, scale, a.roll_off);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Depth-discontinuity maps, fast path for radius <= 8 (every radius the matcher factories derive:
// ceil(0.33*wsize) / ceil(0.5*wsize), DF.cpp:402,408; default 5).  One block walks down a strip of
// 256-2R output columns: every row is loaded once (coalesced), exchanged through a double-buffered
// LDS row, reduced horizontally by each thread (2R+1 LDS reads), and folded into vertical running
// sums whose 2R+1-deep history lives in registers (the row loop is unrolled by the window height so
// ring slots are compile-time).  All sums are exact 32-bit integers: the sum of squares is kept as
// sum(d^2 >> 16) and sum(d^2 & 0xffff) and recombined in double.
// ---------------------------------------------------------------------------------------
// Output rows per block of the column-walking kernels: gridDim.y row blocks share the ROI's rows.
// The launchers use 128 rows per block for big batches (halo rows and the LUT / prefetch ramp are
// amortised) and fewer when the whole launch would otherwise be too few blocks to fill 256 CUs
// (single-image latency).
constexpr int CONF_GROUP = 8; // rows per prefetch / gather group of the column-walking kernels (measured: 8 beats 16 and 32:
                              // fewer registers -> more resident waves matters more than prefetch depth)
constexpr int LRC_GROUP = 4;  // same for the fused left-view kernel (it also carries the gathered dR / cR per row)
#define DC_ROWS ((rows_total + (int)gridDim.y - 1) / (int)gridDim.y)

inline int row_blocks(int rows, int blocks_xz)
{
    int rpb = 128;
    while (rpb > 16 && ((rows + rpb - 1) / rpb) * blocks_xz < 2048) rpb >>= 1;
    return (rows + rpb - 1) / rpb;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains every outstanding
// global load (s_waitcnt vmcnt(0)), which would serialise the row prefetch and the LRC gathers of the
// column-walking kernels behind each row's barrier.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Exact window sums of an int16 map from 32-bit full-rate integer operations only.  d*d (<= 2^30) is
// formed once per pixel (24-bit multiply: int16 operands) and staged next to d; a tap of the horizontal
// sum is one 8-byte LDS read and three adds -- d, and the two 16-bit halves of d*d, which the sub-dword
// operand selectors take apart for free.  (Sums of the halves stay below 2^31 for any window the column
// kernels support; the square sum is reassembled in double, where it is exact.)  64-bit integer adds
// and shifts would need fewer instructions but issue at a quarter of the rate.
struct WinSum {
    int s1, lo, hi;
    __device__ __forceinline__ void clear() { s1 = 0; lo = 0; hi = 0; }
    __device__ __forceinline__ void tap(const int2 v) { s1 += v.x; lo += v.y & 0xffff; hi += (int)((unsigned)v.y >> 16); }
    __device__ __forceinline__ void add(const WinSum& o) { s1 += o.s1; lo += o.lo; hi += o.hi; }
    __device__ __forceinline__ void sub(const WinSum& o) { s1 -= o.s1; lo -= o.lo; hi -= o.hi; }
    __device__ __forceinline__ double sum2() const { return (double)hi * 65536.0 + (double)lo; }
    __device__ static __forceinline__ int2 stage(int d) { return make_int2(d, __mul24(d, d)); }
};

template <int RT>
__global__ void __launch_bounds__(NT) discontinuity_col_kernel(DiscArgs a)
{
    constexpr int K = 2 * RT + 1;
    constexpr int OUTW = NT - 2 * RT;
    __shared__ int2 rowbuf[2][NT];
    const int tid = threadIdx.x;
    const int rows_total = a.rh;
    const int view = a.only_view >= 0 ? a.only_view : (int)(blockIdx.z & 1);
    const size_t pz = a.only_view >= 0 ? blockIdx.z : (blockIdx.z >> 1);
    const int x_out0 = blockIdx.x * OUTW, y_out0 = blockIdx.y * DC_ROWS;
    const char* base = reinterpret_cast<const char*>(a.disp[view]) + (ptrdiff_t)pz * a.pair_stride[view];
    const int rx = a.rx[view];
    const int gx_in = reflect101(x_out0 - RT + tid, a.rw);       // input column of this thread
    const int gx_out = x_out0 + tid - RT;                        // output column (threads RT .. NT-RT-1)
    const bool writer = tid >= RT && tid < NT - RT && gx_out < a.rw;
    float* dst = a.dst[view] + pz * a.frame + (size_t)a.ry * a.W + rx + gx_out;
    const int nrows = min(DC_ROWS, a.rh - y_out0) + 2 * RT;      // input rows this block consumes
    const double scale = 1.0 / ((double)K * (double)K);

    auto load = [&](int n) -> int {                              // input row n of the block (reflected)
        const int gy = reflect101(y_out0 - RT + n, a.rh);
        return reinterpret_cast<const int16_t*>(base + (ptrdiff_t)(a.ry + gy) * a.stride[view])[rx + gx_in];
    };

    // rows are consumed in groups of U (a multiple of the window height K, so that ring slots stay
    // compile-time) and the next group's U loads are in flight while the current group is reduced
    constexpr int U = K * ((CONF_GROUP + K - 1) / K);
    WinSum ring[K], S;
    S.clear();
    int nxt[U];
#pragma unroll
    for (int s = 0; s < U; s++) nxt[s] = (s < nrows) ? load(s) : 0;
    for (int n0 = 0; n0 < nrows; n0 += U) {
        int cur[U];
#pragma unroll
        for (int s = 0; s < U; s++) { cur[s] = nxt[s]; asm volatile("" : "+v"(cur[s])); }   // the group's one wait happens here
#pragma unroll
        for (int s = 0; s < U; s++) nxt[s] = (n0 + U + s < nrows) ? load(n0 + U + s) : 0;          // in flight across the rows below
#pragma unroll
        for (int s = 0; s < U; s++) {
            const int n = n0 + s;
            const int slot = s % K;                               // compile-time after unrolling
            if (n < nrows) {                                     // block-uniform
                rowbuf[n & 1][tid] = WinSum::stage(cur[s]);
                lds_barrier();
                WinSum hsum;
                hsum.clear();
                if (tid >= RT && tid < NT - RT) {
#pragma unroll
                    for (int d = -RT; d <= RT; d++) hsum.tap(rowbuf[n & 1][tid + d]);
                }
                if (n >= K) S.sub(ring[slot]);                    // row n-K leaves the window
                ring[slot] = hsum;
                S.add(hsum);
                if (n >= 2 * RT && writer) {                     // window rows n-2RT..n are complete
                    const int oy = y_out0 + n - 2 * RT;
                    ADF_ST(&dst[(size_t)oy * a.W], disc_value(S.s1, [&] { return S.sum2(); }, scale, a.roll_off));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Left view, fused: the column-walking discontinuity sweep above, and for every completed window the
// left-right check against the (already finished) right map, x255, and the confidence map written
// straight away -- the left discontinuity map never exists in memory (DF.cpp:204-209 in one pass).
// With WRITE_U the right-hand sides conf*float(dL), conf (DF.cpp:288-290) are written as well.
// ---------------------------------------------------------------------------------------
template <int RT, bool WRITE_U>
__global__ void __launch_bounds__(NT) conf_left_kernel(ConfLeftArgs a)
{
    constexpr int K = 2 * RT + 1;
    constexpr int OUTW = NT - 2 * RT;
    constexpr int U = K * ((LRC_GROUP + K - 1) / K);
    constexpr int CR = RT > 0 ? RT : 1;
    __shared__ int2 rowbuf[2][NT];
    const Geom& g = a.g;
    const int tid = threadIdx.x;
    const int rows_total = g.rh;
    const size_t pz = blockIdx.z;
    const int x_out0 = blockIdx.x * OUTW, y_out0 = blockIdx.y * DC_ROWS;
    const char* baseL = reinterpret_cast<const char*>(a.dL) + (ptrdiff_t)pz * a.psL;
    const char* baseR = reinterpret_cast<const char*>(a.dR) + (ptrdiff_t)pz * a.psR;
    const float* cR = a.cR + pz * g.frame;
    float* conf = a.conf + pz * g.cframe + g.cx0;
    const int gx_in = reflect101(x_out0 - RT + tid, g.rw);
    const int gx_out = x_out0 + tid - RT;                          // == gx_in for writer threads
    const bool writer = tid >= RT && tid < NT - RT && gx_out < g.rw;
    const int j_abs = g.rx + gx_out;                              // frame column of this thread's output
    const int rows_out = min(DC_ROWS, g.rh - y_out0);
    const int nrows = rows_out + 2 * RT;                          // input rows this block consumes
    const double scale = 1.0 / ((double)K * (double)K);
    const int right_end = a.rrx + g.rw;

    auto load = [&](int n) -> int {
        const int gy = reflect101(y_out0 - RT + n, g.rh);
        return reinterpret_cast<const int16_t*>(baseL + (ptrdiff_t)(g.ry + gy) * a.sL)[g.rx + gx_in];
    };

    // The LRC gathers (dR and cR at column j - d/16 of the same row) depend on the disparity of the
    // window's CENTRE row, which this thread loaded itself RT rows before the window completes.  They
    // are issued for a whole group of rows as soon as the group's values have arrived and consumed as
    // the windows complete, so a group pays one memory latency instead of two per row.
    WinSum ring[K], S;
    S.clear();
    int nxt[U], cur[U];
    int gd[U]; float gc[U];                                       // gathered dR / cR of this group's centre rows
    int cd[CR], cdr[CR]; float ccr[CR];                           // carried over: last RT centre rows of the previous group
#pragma unroll
    for (int k = 0; k < CR; k++) { cd[k] = 0; cdr[k] = 0; ccr[k] = 0.0f; }
#pragma unroll
    for (int s = 0; s < U; s++) nxt[s] = (s < nrows) ? load(s) : 0;
    for (int n0 = 0; n0 < nrows; n0 += U) {
#pragma unroll
        for (int s = 0; s < U; s++) { cur[s] = nxt[s]; asm volatile("" : "+v"(cur[s])); }
#pragma unroll
        for (int s = 0; s < U; s++) {                             // gathers for centre rows n0 .. n0+U-1
            const int n = n0 + s;
            gd[s] = 0; gc[s] = 0.0f;
            if (writer && n >= RT && n < nrows - RT) {
                const int ridx = j_abs - (cur[s] >> 4);           // DF.cpp:331
                if (ridx >= a.rrx && ridx < right_end) {
                    const int i_abs = g.ry + y_out0 + n - RT;
                    gd[s] = reinterpret_cast<const int16_t*>(baseR + (ptrdiff_t)i_abs * a.sR)[ridx];
                    gc[s] = cR[(size_t)i_abs * g.W + ridx];
                }
            }
        }
        // One wait per group, placed by hand: the gathers have to be back before the first window of the
        // group completes, and behind the block-uniform branches of the row loop the compiler can only wait
        // for vmcnt(0) at every use -- which, stores counting in vmcnt here, also waits for the previous
        // row's store to be acknowledged.  After this point the group's inputs are plain registers; the next
        // group's rows are requested only now, so they and the stores stay in flight across the row loop.
#pragma unroll
        for (int s = 0; s < U; s++) asm volatile("" : "+v"(gd[s]), "+v"(gc[s]));
#pragma unroll
        for (int s = 0; s < U; s++) nxt[s] = (n0 + U + s < nrows) ? load(n0 + U + s) : 0;
#pragma unroll
        for (int s = 0; s < U; s++) {
            const int n = n0 + s;
            const int slot = s % K;
            if (n < nrows) {                                     // block-uniform
                rowbuf[n & 1][tid] = WinSum::stage(cur[s]);
                lds_barrier();
                WinSum hsum;
                hsum.clear();
                if (tid >= RT && tid < NT - RT) {
#pragma unroll
                    for (int d = -RT; d <= RT; d++) hsum.tap(rowbuf[n & 1][tid + d]);
                }
                if (n >= K) S.sub(ring[slot]);
                ring[slot] = hsum;
                S.add(hsum);
                if (n >= 2 * RT && writer) {                     // window centred on input row n-RT is complete
                    const int oy = y_out0 + n - 2 * RT;
                    const int i_abs = g.ry + oy;
                    float c = disc_value(S.s1, [&] { return S.sum2(); }, scale, a.roll_off);
                    // centre row's own disparity and its gathers: this group's slot s-RT, or carried over
                    const int d = (s >= RT) ? cur[(s >= RT) ? s - RT : 0] : cd[(s < RT) ? s : 0];
                    const int dr = (s >= RT) ? gd[(s >= RT) ? s - RT : 0] : cdr[(s < RT) ? s : 0];
                    const float b = (s >= RT) ? gc[(s >= RT) ? s - RT : 0] : ccr[(s < RT) ? s : 0];
                    const int ridx = j_abs - (d >> 4);            // DF.cpp:331
                    if (ridx >= a.rrx && ridx < right_end) {
                        if (abs(d + dr) < a.thresh) c = b < c ? b : c;   // DF.cpp:334-335
                        else c = 0.0f;                                   // DF.cpp:337
                    }
                    c = 255.0f * c;                               // DF.cpp:209
                    ADF_ST(&conf[(size_t)i_abs * g.cpitch + j_abs], c);
                    if (WRITE_U) {
                        const RhsPlanes u = rhs_planes(a.U0, a.U1, ORIENT_PAIR, pz, g.plane);
                        const size_t o = rhs_index(ORIENT_PAIR, oy, gx_out, g);
                        u.U0[o] = c * (float)d;                   // DF.cpp:289-290
                        u.U1[o] = c;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RT; k++) { cd[k] = cur[U - RT + k]; cdr[k] = gd[U - RT + k]; ccr[k] = gc[U - RT + k]; }
    }
}

// ---------------------------------------------------------------------------------------
// Both views in ONE sweep (DF.cpp:197-210 whole: 161-194 + 343-373 for both views, 306-341, :209): the right
// view's discontinuity map never exists in HBM.  A workgroup owns a band of rows over the FULL ROI width; every
// row step it forms the window statistics of both views, parks the right view's map of that row in LDS (16 KB
// at 4K) together with the raw right disparities of the last few rows, and the left-view lanes gather from
// there -- any column of the row, so the LRC is exact for arbitrary disparities without a fall-back path.
// HBM sees dL and dR once (plus 2*RT halo rows per band) and the confidence map: 8 B per ROI pixel.
//
// Layout of the work: lane = 4 adjacent columns (one 8-byte load per view and row), wave = 64 lanes = 248
// output columns for radius <= 4, 240 for radius 5..8 (the first and last ceil(radius/4) lanes only supply the
// horizontal halo, so a wave never needs another wave's sums).  Sums run VERTICAL first: each lane keeps the raw values of the last K = 2*RT+1 rows of its
// columns packed in registers and updates the column sums (sum d, and sum d^2 split in 16-bit halves: all
// 32-bit integer, exact) by new row minus oldest row; the horizontal window is then a sliding sum over the
// lane's own four column sums and the neighbours' edge columns, fetched with whole-wave DPP shifts (no LDS, no
// barrier).  Virtual columns: the row is extended by RT reflected columns on both sides (BORDER_REFLECT_101
// inside the ROI copy, DF.cpp:167-185) and the lanes at the two image edges load the reflected real columns
// (one 8-byte window + a byte permute), so the horizontal window itself never needs a border case.
// One workgroup barrier per row (right map written -> gathered).
// ---------------------------------------------------------------------------------------
constexpr int CB_COLS = 4;
#define CB_HALO(RT) (((RT) + CB_COLS - 1) / CB_COLS)                 // halo lanes on each side of a wave
#define CB_WOUT(RT) ((64 - 2 * CB_HALO(RT)) * CB_COLS)               // output columns per wave: 248 (radius <= 4), 240 (5..8)
// The right view's K raw rows of the band kernel (conf_band_body): registers at radius 1..3, LDS at 4..6 (K + 1 rows
// of any width the kernel covers fit), LDS where the ROI's width lets them fit at 7..8.
enum BandRing { RING_REGS, RING_LDS, RING_LDS_BY_WIDTH };
constexpr BandRing band_ring(int rt) { return rt < 4 ? RING_REGS : rt <= 6 ? RING_LDS : RING_LDS_BY_WIDTH; }
constexpr int CB_MAX_WAVES = 16;
constexpr int CB_MAX_BAND_ROWS = 2048;                             // output rows of a band (ColSum::lo must not wrap)
constexpr int CB_MAX_RADIUS = 2 * CB_COLS;

__device__ __forceinline__ int dpp_from_prev(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }  // wave_shr:1
__device__ __forceinline__ int dpp_from_next(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }  // wave_shl:1

struct ColSum {
    int s1; unsigned lo; int hi;
    // d enters / leaves the column window.  sum d^2 = 65536 * hi + lo exactly, carried as two 32-bit halves so that the
    // horizontal sums need no carries: the change q_new - q_old is split into its low 16 bits (added to lo: never
    // negative, so lo only grows -- by less than 65536 per row, which is why a band is at most CB_MAX_BAND_ROWS rows:
    // 17 columns x 2064 rows x 65535 < 2^32) and its arithmetic shift by 16 (added to hi).  Round 3: 7 instructions
    // instead of the 10 of summing (q & 0xffff) and (q >> 16) of both squares separately.
    __device__ __forceinline__ void slide(int dn, int dold)
    {
        const int qn = __mul24(dn, dn), qo = __mul24(dold, dold);
        s1 += dn - dold;
        const int diff = qn - qo;
        lo += (unsigned)diff & 0xffffu;
        hi += diff >> 16;
    }
};

// The four map values of a lane's columns from its column sums.  Horizontal window of output column q (0..3): virtual
// columns q-RT .. q+RT relative to the lane's first column, i.e. the lane's own columns max(0,q-RT) .. min(3,q+RT) --
// differences of the lane's prefix sums -- plus, from the j-th lane before it (columns -4j .. -4j+3), its LAST
// min(4, 4-4j+RT-q) columns and, from the j-th lane after it, its FIRST min(4, q+RT-4j+1) columns; j runs to
// CB_HALO(RT) = ceil(RT/4) (one lane for radius <= 4, two for radius 5..8: round 3).  Every neighbour contribution is
// ONE partial sum fetched by whole-wave DPP shifts (wave_shr:1 / wave_shl:1, applied j times); where a fetched value
// has a single use the compiler folds the shift into the add that consumes it.
template <int J> __device__ __forceinline__ int dpp_prev_n(int v) { if constexpr (J <= 0) return v; else return dpp_prev_n<J - 1>(dpp_from_prev(v)); }
template <int J> __device__ __forceinline__ int dpp_next_n(int v) { if constexpr (J <= 0) return v; else return dpp_next_n<J - 1>(dpp_from_next(v)); }

template <int RT, int J>
__device__ __forceinline__ void band_neighbours(const int (&p1)[CB_COLS + 1], const unsigned (&pl)[CB_COLS + 1], const int (&ph)[CB_COLS + 1],
                                                int q, int& h1, unsigned& hl, int& hh)
{
    if constexpr (J >= 1) {
        const int mp = 4 - 4 * J + RT - q, mn = q + RT - 4 * J + 1;      // columns of lane -J / lane +J inside the window
        const int m = mp < 0 ? 0 : (mp > CB_COLS ? CB_COLS : mp), m2 = mn < 0 ? 0 : (mn > CB_COLS ? CB_COLS : mn);
        if (m > 0) {
            h1 += dpp_prev_n<J>(p1[CB_COLS] - p1[CB_COLS - m]); hl += (unsigned)dpp_prev_n<J>((int)(pl[CB_COLS] - pl[CB_COLS - m]));
            hh += dpp_prev_n<J>(ph[CB_COLS] - ph[CB_COLS - m]);
        }
        if (m2 > 0) { h1 += dpp_next_n<J>(p1[m2]); hl += (unsigned)dpp_next_n<J>((int)pl[m2]); hh += dpp_next_n<J>(ph[m2]); }
        band_neighbours<RT, J - 1>(p1, pl, ph, q, h1, hl, hh);
    }
}

template <int RT>
__device__ __forceinline__ void band_row_values(const ColSum (&V)[CB_COLS], double scale, float roll_off, float (&out)[CB_COLS])
{
    static_assert(RT >= 1 && RT <= 2 * CB_COLS, "the halo must fit two lanes");
    int p1[CB_COLS + 1], ph[CB_COLS + 1];                            // prefix sums P[i] = V[0] + .. + V[i-1]
    unsigned pl[CB_COLS + 1];
    p1[0] = ph[0] = 0; pl[0] = 0u;
#pragma unroll
    for (int i = 0; i < CB_COLS; i++) { p1[i + 1] = p1[i] + V[i].s1; pl[i + 1] = pl[i] + V[i].lo; ph[i + 1] = ph[i] + V[i].hi; }
#pragma unroll
    for (int q = 0; q < CB_COLS; q++) {
        const int a = q - RT > 0 ? q - RT : 0, b = (q + RT < CB_COLS - 1 ? q + RT : CB_COLS - 1) + 1;
        int h1 = p1[b] - p1[a], hh = ph[b] - ph[a];
        unsigned hl = pl[b] - pl[a];
        band_neighbours<RT, CB_HALO(RT)>(p1, pl, ph, q, h1, hl, hh);
        // (65536 * hh + hl is an integer below 2^53: the fused form is exact, like the product and the sum it replaces)
        out[q] = disc_value(h1, [=] { return __builtin_fma((double)hh, 65536.0, (double)hl); }, scale, roll_off);
    }
}

// (band `band` of image `pz`; smem = the workgroup's dynamic LDS.  Waves past the ROI's width own no columns and only
// keep the barriers company: the merged preparation kernel launches at least four waves per block.)
template <int RT, bool RLDS = band_ring(RT) != RING_REGS>
__device__ __forceinline__ void conf_band_body(const ConfBandArgs& a, const int band, const size_t pz, unsigned char* smem)
{
    constexpr int K = 2 * RT + 1;
    // RLDS (radius 4..8 wherever K + 1 rows of the ROI's width fit the LDS: always up to radius 6, up to ~3700 columns at
    // radius 7 and ~3300 at radius 8): the right view's K raw rows live in LDS only (they are parked there for the gather
    // anyway) and the row that leaves the column window is read back from it, instead of a second register ring: 18..34
    // registers fewer per lane -- at radius 4..5 that is what lets a wave of the weight kernel sit beside the band's
    // four waves on a SIMD (the radius 1..3 kernels always could), at radius 6..8 it ends the register spills.
    // raw right rows kept in LDS: the centre row + one row of slack for the slowest wave; with RLDS all K rows + the one
    // being written (row n - K is read before this iteration's barrier, row n written before it: never the same slot)
    constexpr int RING = RLDS ? K + 1 : RT + 2;
    typedef int v2i_u __attribute__((ext_vector_type(2), aligned(2)));
    typedef float v4f_u __attribute__((ext_vector_type(4), aligned(4)));
    const Geom& g = a.g;
    const int rw = g.rw, rwp = (rw + 3) & ~3;
    float* crow = reinterpret_cast<float*>(smem);                     // [2][rwp]   right map of the current row
    int16_t* draw = reinterpret_cast<int16_t*>(crow + 2 * rwp);       // [RING][rwp] raw right disparities
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y0 = band * a.rows_per_band;
    const int rows_out = min(a.rows_per_band, g.rh - y0);
    const int nrows = rows_out + 2 * RT;               // input rows this band consumes
    constexpr int HL = CB_HALO(RT);
    const int vbase = wv * CB_WOUT(RT) + CB_COLS * (lane - HL);       // first (virtual) column of this lane
    const bool out_lane = lane >= HL && lane <= 63 - HL && vbase < rw;  // owns output columns vbase .. vbase+3 (those < rw)

    // which real columns feed this lane's four virtual columns: one 8-byte window [lcol, lcol+4) of the row and a
    // byte permute (identity for every lane away from the two image edges)
    int lcol = vbase;
    unsigned perm0 = 0x03020100u, perm1 = 0x07060504u;
    if (!(vbase >= 0 && vbase + CB_COLS - 1 < rw)) {
        int rv[CB_COLS], lo_need = rw;
#pragma unroll
        for (int q = 0; q < CB_COLS; q++) {
            const int v = vbase + q;
            const int vc = v < -RT ? -RT : (v > rw - 1 + RT ? rw - 1 + RT : v);
            rv[q] = reflect101(vc, rw);
            if (v >= -RT && v <= rw - 1 + RT) lo_need = min(lo_need, rv[q]);
        }
        lcol = lo_need >= rw ? 0 : lo_need;
        lcol = max(0, min(lcol, rw - CB_COLS));
        unsigned sb[CB_COLS];
#pragma unroll
        for (int q = 0; q < CB_COLS; q++) {
            const unsigned e = (unsigned)max(0, min(rv[q] - lcol, CB_COLS - 1));
            sb[q] = (2u * e) | ((2u * e + 1u) << 8);
        }
        perm0 = sb[0] | (sb[1] << 16);
        perm1 = sb[2] | (sb[3] << 16);
    }
    // row base = wave-uniform (scalar registers), lane part = a 32-bit byte offset
    const char* baseL = reinterpret_cast<const char*>(a.dL) + (ptrdiff_t)pz * a.psL + (ptrdiff_t)g.ry * a.sL + (ptrdiff_t)g.rx * 2;
    const char* baseR = reinterpret_cast<const char*>(a.dR) + (ptrdiff_t)pz * a.psR + (ptrdiff_t)g.ry * a.sR + (ptrdiff_t)a.rrx * 2;
    const unsigned lane_off = (unsigned)lcol * 2u;
    float* conf = a.conf + pz * g.cframe + (size_t)g.ry * g.cpitch + g.cx0 + g.rx;   // 16-byte aligned (Geom::cx0)
    const double scale = 1.0 / ((double)K * (double)K);
    const int right_end = a.rrx + rw;

    // packed raw rows: .x = columns (0,1), .y = columns (2,3) of the lane, 16 bits each
    auto load = [&](const char* base, ptrdiff_t stride, int n) -> v2i_u {
        const int nn = n < nrows ? n : nrows - 1;
        int gy = abs(y0 - RT + nn);                                  // BORDER_REFLECT_101 with one reflection:
        gy = gy >= g.rh ? 2 * (g.rh - 1) - gy : gy;                  // the launcher guarantees rh > RT
        return *reinterpret_cast<const v2i_u*>(base + (ptrdiff_t)gy * stride + lane_off);
    };
    auto permute = [&](v2i_u p) -> int2 {
        return make_int2((int)__builtin_amdgcn_perm((unsigned)p.y, (unsigned)p.x, perm0),
                         (int)__builtin_amdgcn_perm((unsigned)p.y, (unsigned)p.x, perm1));
    };
#define CB_ELEM(P, q) ((q) == 0 ? (int)(short)((P).x & 0xffff) : (q) == 1 ? ((P).x >> 16) : (q) == 2 ? (int)(short)((P).y & 0xffff) : ((P).y >> 16))

    int2 ringL[K], ringR[RLDS ? 1 : K];
    ColSum VL[CB_COLS], VR[CB_COLS];
#pragma unroll
    for (int k = 0; k < K; k++) { ringL[k] = make_int2(0, 0); if (!RLDS) ringR[k] = make_int2(0, 0); }
    // (RLDS) an 8-byte LDS read needs an 8-byte aligned address: true for every lane away from the image edges
    // (lcol = vbase, a multiple of 4 columns); waves with an edge lane read 2-byte aligned
    const bool unaligned_wave = RLDS && __builtin_amdgcn_ballot_w64((lcol & 3) != 0) != 0;
#pragma unroll
    for (int q = 0; q < CB_COLS; q++) { VL[q].s1 = VL[q].hi = 0; VL[q].lo = 0u; VR[q].s1 = VR[q].hi = 0; VR[q].lo = 0u; }

    // rows n+1 and n+2 are in flight while row n is reduced
    v2i_u pfL0 = load(baseL, a.sL, 0), pfR0 = load(baseR, a.sR, 0);
    v2i_u pfL1 = load(baseL, a.sL, 1), pfR1 = load(baseR, a.sR, 1);
    for (int n0 = 0; n0 < nrows; n0 += K) {
#pragma unroll
        for (int s = 0; s < K; s++) {
            const int n = n0 + s;
            if (n < nrows) {                                             // block-uniform
                const int2 curL = permute(pfL0), curR = permute(pfR0);
                pfL0 = pfL1; pfR0 = pfR1;
                pfL1 = load(baseL, a.sL, n + 2); pfR1 = load(baseR, a.sR, n + 2);
                // vertical: row n enters the column windows, row n-K leaves (zeros during the first K rows)
                int2 oldR;
                if constexpr (RLDS) {
                    // row n-K of the right view, this lane's four (virtual) columns: the same window + permute as the
                    // global load, from the LDS ring (zeros while the window fills)
                    const int16_t* rp = draw + (n >= K ? (n - K) % RING : 0) * rwp + lcol;
                    v2i_u q2;
                    if (unaligned_wave) q2 = *reinterpret_cast<const v2i_u*>(rp);
                    else { const int2 t = *reinterpret_cast<const int2*>(rp); q2.x = t.x; q2.y = t.y; }
                    oldR = permute(q2);
                    if (n < K) oldR = make_int2(0, 0);
                } else
                    oldR = ringR[s];
#pragma unroll
                for (int q = 0; q < CB_COLS; q++) {
                    VL[q].slide(CB_ELEM(curL, q), CB_ELEM(ringL[s], q));
                    VR[q].slide(CB_ELEM(curR, q), CB_ELEM(oldR, q));
                }
                ringL[s] = curL;
                if constexpr (!RLDS) ringR[s] = curR;
                float cl[CB_COLS], cr[CB_COLS];
                const bool complete = n >= 2 * RT;                      // windows centred on input row n-RT are complete
                if (complete) {                                          // (one basic block: the DPP fetches fold into their adds)
                    band_row_values<RT>(VR, scale, a.roll_off, cr);
                    band_row_values<RT>(VL, scale, a.roll_off, cl);
                }
                if (out_lane) {
                    // raw right row n -> LDS (it is the centre row of the window that completes RT rows from now)
                    *reinterpret_cast<int2*>(draw + (n % RING) * rwp + vbase) = curR;
                    if (complete) *reinterpret_cast<float4*>(crow + (n & 1) * rwp + vbase) = make_float4(cr[0], cr[1], cr[2], cr[3]);
                }
                lds_barrier();
                if (complete && out_lane) {
                    const int oy = y0 + n - 2 * RT;                     // ROI row of the output
                    const int2 cen = ringL[(s + K - RT) % K];            // the centre row's own disparities
                    const float* cb = crow + (n & 1) * rwp;
                    const int16_t* db = draw + ((n - RT) % RING) * rwp;
                    float res[CB_COLS];
#pragma unroll
                    for (int q = 0; q < CB_COLS; q++) {
                        const int d = CB_ELEM(cen, q);
                        const int ridx = g.rx + vbase + q - (d >> 4);    // DF.cpp:331 (frame column of the right view)
                        const bool hit = ridx >= a.rrx && ridx < right_end;  // DF.cpp:332
                        const int rr = hit ? ridx - a.rrx : 0;           // (a miss reads column 0 and discards it)
                        const float b = cb[rr];
                        const int dr = db[rr];
                        const float cmin = b < cl[q] ? b : cl[q];        // DF.cpp:334-335 (std::min)
                        const float chit = abs(d + dr) < a.thresh ? cmin : 0.0f;   // DF.cpp:337
                        res[q] = 255.0f * (hit ? chit : cl[q]);          // DF.cpp:209
                    }
                    float* dst = conf + (size_t)oy * g.cpitch + vbase;
                    if (vbase + CB_COLS <= rw) {
                        const v4f_u o = {res[0], res[1], res[2], res[3]};
                        __builtin_nontemporal_store(o, reinterpret_cast<v4f_u*>(dst));
                    } else {
#pragma unroll
                        for (int q = 0; q < CB_COLS; q++)
                            if (vbase + q < rw) ADF_ST(&dst[q], res[q]);
                    }
                }
            }
        }
    }
#undef CB_ELEM
}

template <int RT, bool RLDS = band_ring(RT) != RING_REGS>
__global__ void __launch_bounds__(64 * CB_MAX_WAVES) conf_band_kernel(ConfBandArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    conf_band_body<RT, RLDS>(a, blockIdx.x, blockIdx.y, smem);
}

constexpr int OUT_ROWS = 16; // rows per block of outside_kernel

// Non-ROI pixels of the frame: the side columns of the ROI's rows (part A: W - rw columns x rh rows, blocks of NT
// columns x OUT_ROWS rows) and the whole rows above / below the ROI (part B: (H - rh) x W pixels, a flat index in
// blocks of NT * OUT_ROWS pixels).  blockIdx.x < nA: part A, else part B -- no block without work (round 3: the BM
// factory's ROI has rows outside it, and a grid over the whole frame spent 0.49 ms per 64 x 4K step finding that out).
__device__ __forceinline__ void outside_body(const OutsideArgs& a, const int nAx, const int nA, const unsigned blk, const size_t pz)
{
    const Geom& g = a.g;
    char* out = a.out ? reinterpret_cast<char*>(a.out) + (ptrdiff_t)pz * a.pair_stride : nullptr;
    float* conf = a.conf ? a.conf + pz * g.cframe + g.cx0 : nullptr;
    if ((int)blk < nA) {
        const int bx = blk % nAx, by = blk / nAx;
        const int t = bx * NT + threadIdx.x;
        if (t >= g.W - g.rw) return;
        const int j = t < g.rx ? t : t + g.rw;
        const int i0 = g.ry + by * OUT_ROWS, i1 = min(i0 + OUT_ROWS, g.ry + g.rh);
        for (int i = i0; i < i1; i++) {
            if (out) store_fill(out, (ptrdiff_t)i * a.stride, j, a.fill, a.out_f32);
            if (conf) conf[(size_t)i * g.cpitch + j] = 0.0f;
        }
    } else {
        const size_t npix = (size_t)(g.H - g.rh) * g.W;
        size_t p = (size_t)(blk - nA) * (NT * OUT_ROWS) + threadIdx.x;
#pragma unroll 4
        for (int k = 0; k < OUT_ROWS; k++, p += NT) {
            if (p >= npix) break;
            int i = (int)(p / (size_t)g.W);
            const int j = (int)(p - (size_t)i * g.W);
            if (i >= g.ry) i += g.rh;                        // rows below the ROI
            if (out) store_fill(out, (ptrdiff_t)i * a.stride, j, a.fill, a.out_f32);
            if (conf) conf[(size_t)i * g.cpitch + j] = 0.0f;
        }
    }
}

__global__ void __launch_bounds__(NT) outside_kernel(OutsideArgs a, int nAx, int nA)
{
    outside_body(a, nAx, nA, blockIdx.x, blockIdx.z);
}

// The blocks outside_body decodes: nA of part A, nAx (at least 1) across, then nB of part B; in_range: a grid's x holds them.
struct OutsideGrid { int nAx, nA; size_t nB; bool in_range; };
inline OutsideGrid outside_grid(const Geom& g)
{
    const int side = g.W - g.rw;
    const int nAx = (side + NT - 1) / NT, nA = side > 0 ? nAx * ((g.rh + OUT_ROWS - 1) / OUT_ROWS) : 0;
    const size_t nB = ((size_t)(g.H - g.rh) * g.W + (size_t)NT * OUT_ROWS - 1) / ((size_t)NT * OUT_ROWS);
    return OutsideGrid{nAx > 0 ? nAx : 1, nA, nB, nA + nB <= 0x7fffffffu};
}

// ---------------------------------------------------------------------------------------
// Everything a confidence-mode call prepares before its first solve pass, in ONE launch (round 3): blocks
// [0, nC) are bands of the one-sweep confidence kernel (the longest role first), [nC, nC + nW) blocks of the streaming
// weight kernel, the rest fill what lies outside the ROI.  The three touch disjoint data, so for batches they are
// separate launches on two streams (adf_api.hip); for ONE small frame per call the cross-stream event and launch
// latencies are a third of the call (profiles/r03_latency_timeline.txt), which this kernel removes.  Blocks are as
// wide as the confidence role needs (at least the weight role's 256 threads); waves a role has no use for only keep
// its barriers company.
// ---------------------------------------------------------------------------------------
struct PrepArgs {
    ConfBandArgs c; WeightArgs w; OutsideArgs o;
    int nC, nW, nWx, nWy, nOAx, nOA;
};

template <int CH, int RT>
__global__ void __launch_bounds__(64 * CB_MAX_WAVES) prep_small_kernel(PrepArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ prep::WsShared<CH> ws;
    const unsigned b = blockIdx.x;
    const size_t pz = blockIdx.y;
    if ((int)b < a.nC) {
        conf_band_body<RT>(a.c, (int)b, pz, smem);
    } else if ((int)b < a.nC + a.nW) {
        const int k = (int)b - a.nC;
        prep::weights_stream_body<CH>(a.w, k % a.nWx, k / a.nWx, a.nWy, pz, ws, threadIdx.x < prep::WS_NT);
    } else {
        if (threadIdx.x < NT) outside_body(a.o, a.nOAx, a.nOA, b - (unsigned)(a.nC + a.nW), pz);
    }
}

inline size_t disc_lds_bytes(int r)
{
    const size_t IH = TY + 2 * r, IWP = (TX + 2 * r) | 1;
    return IH * TX * 8 + IH * TX * 4 + ((IH * IWP * 2 + 15) & ~(size_t)15);
}

// f(std::integral_constant<int, R>), a kernel, for the R in [LO, HI] that equals radius; nullptr if there is none.
template <int LO, int HI, class F>
inline auto dispatch_radius(int radius, F&& f) -> decltype(f(std::integral_constant<int, LO>{}))
{
    if (radius == LO) return f(std::integral_constant<int, LO>{});
    if constexpr (LO < HI) return dispatch_radius<LO + 1, HI>(radius, f);
    else return nullptr;
}

// Dynamic LDS beyond `threshold` has to be allowed per function AND device (a process may hold handles on several):
// set whenever needed, never cached process-wide.
template <class Kernel>
inline hipError_t ensure_dynamic_lds(Kernel kernel, size_t bytes, size_t threshold)
{
    if (bytes <= threshold) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

inline dim3 col_grid(int rw, int rh, int radius, int nz)   // column-walking kernels: strips of NT - 2*radius output columns
{
    const int gx = (rw + (NT - 2 * radius) - 1) / (NT - 2 * radius);
    return dim3(gx, row_blocks(rh, gx * nz), nz);
}

} // namespace

int max_disc_radius() { return MAX_RADIUS; }

hipError_t launch_discontinuity(const DiscArgs& a, int n_pairs, hipStream_t st)
{
    if (a.rw <= 0 || a.rh <= 0 || n_pairs <= 0) return hipSuccess;
    if (a.radius < 0 || a.radius > MAX_RADIUS) return hipErrorInvalidValue;
    const int nz = (a.only_view >= 0 ? 1 : 2) * n_pairs;
    if (a.radius <= 8) {
        const auto k = dispatch_radius<0, 8>(a.radius, [](auto R) { return &discontinuity_col_kernel<decltype(R)::value>; });
        hipLaunchKernelGGL(k, col_grid(a.rw, a.rh, a.radius, nz), dim3(NT), 0, st, a);
        return hipGetLastError();
    }
    static_assert(TX == 64 && TY == 32 && NT == 256, "discontinuity_kernel assumes a 64x32 tile and 256 threads");
    const size_t lds = disc_lds_bytes(a.radius);
    hipError_t e = ensure_dynamic_lds(discontinuity_kernel, lds, 48 * 1024);
    if (e != hipSuccess) return e;
    dim3 grid((a.rw + TX - 1) / TX, (a.rh + TY - 1) / TY, nz);
    hipLaunchKernelGGL(discontinuity_kernel, grid, dim3(NT), lds, st, a);
    return hipGetLastError();
}

int conf_left_max_radius() { return 8; }

constexpr size_t CB_LDS_LIMIT = 150 * 1024;

// What a band workgroup of an ROI looks like: one wave per CB_WOUT columns, the right map's two rows and the ring of
// raw right rows in LDS -- all K + 1 of them where band_ring() says so and they fit, else the centre row + slack.
struct BandShape { int waves; size_t lds; bool rlds; };
static BandShape conf_band_shape(const Geom& g, int radius)
{
    const size_t rwp = (size_t)((g.rw + 3) & ~3);
    const auto lds = [&](size_t ring_rows) { return 2 * rwp * 4 + ring_rows * rwp * 2; };
    const size_t K = 2 * (size_t)radius + 1;
    const bool rlds = band_ring(radius) != RING_REGS && lds(K + 1) <= CB_LDS_LIMIT;
    return BandShape{(g.rw + CB_WOUT(radius) - 1) / CB_WOUT(radius), lds(rlds ? K + 1 : (size_t)radius + 2), rlds};
}

bool conf_band_fits(const Geom& g, int radius)
{
    return radius >= 1 && radius <= CB_MAX_RADIUS && g.rw >= 8 && g.rw > radius && g.rw <= CB_MAX_WAVES * CB_WOUT(radius) &&
           g.rh > radius && conf_band_shape(g, radius).lds <= CB_LDS_LIMIT;
}

// The band kernel's instantiation for a radius and ring choice (nullptr: no such radius).
typedef void (*BandKernel)(ConfBandArgs);
static BandKernel conf_band_variant(int radius, bool rlds)
{
    return dispatch_radius<1, CB_MAX_RADIUS>(radius, [&](auto R) -> BandKernel {
        constexpr int RR = decltype(R)::value;
        if constexpr (band_ring(RR) == RING_LDS_BY_WIDTH) return rlds ? conf_band_kernel<RR, true> : conf_band_kernel<RR, false>;
        else return conf_band_kernel<RR>;
    });
}

// Band workgroups of this shape a CU holds at once (occupancy query, remembered per radius for the last shape asked).
static int conf_band_resident(int radius, const BandShape& sh, int dev)
{
    struct Memo { int dev; BandShape sh; int value; };
    static Memo memo[CB_MAX_RADIUS + 1] = {};
    static std::mutex mu;
    {
        std::lock_guard<std::mutex> lk(mu);
        const Memo& m = memo[radius];
        if (m.value > 0 && m.dev == dev && m.sh.waves == sh.waves && m.sh.lds == sh.lds && m.sh.rlds == sh.rlds) return m.value;
    }
    int v = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, conf_band_variant(radius, sh.rlds), 64 * sh.waves, sh.lds);
    if (e != hipSuccess || v < 1) { (void)hipGetLastError(); v = 1; }
    std::lock_guard<std::mutex> lk(mu);
    memo[radius] = Memo{dev, sh, v};
    return v;
}

// CUs of a device, read once per device (racing writers store the same value); 256 if it cannot be asked
static int cu_count(int dev)
{
    static int cache[64] = {0};
    int cus = 0;
    if (dev >= 0 && dev < 64) cus = __atomic_load_n(&cache[dev], __ATOMIC_RELAXED);
    if (cus <= 0) {
        if (dev < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        if (dev >= 0 && dev < 64) __atomic_store_n(&cache[dev], cus, __ATOMIC_RELAXED);
    }
    return cus;
}

// rows of a band asked to be `want` rows tall: at least the halo's 2 * radius (and 4), at most CB_MAX_BAND_ROWS and rh
static int conf_band_clamp_rows(int want, int rh, int radius)
{
    const int min_rpb = 2 * radius > 4 ? 2 * radius : 4;
    int rpb = want < min_rpb ? min_rpb : want;
    if (rpb > CB_MAX_BAND_ROWS) rpb = CB_MAX_BAND_ROWS;
    return rpb > rh ? rh : rpb;
}

// How tall the bands of a launch are: the policy, and what it was measured against.
static int conf_band_rows_per_band(const Geom& g, int radius, const BandShape& sh, int n_pairs)
{
    // bands: at most ONE workgroup per CU, on three quarters of the CUs (round 3; it was two rounds of the chip).  A band workgroup is 15 waves with 57 KB of
    // LDS: it only starts on a CU that has all of that free at once, and the weight kernel that runs beside this one on
    // the side stream refills every slot a finished band leaves with its own small workgroups -- the second round's
    // bands then queue until the weight kernel is done (kernel timeline: this kernel 2.38 ms beside it, 1.32 alone).
    // With no more bands than CUs every band starts at once and runs through: 1.39-1.43 ms beside the weight kernel, the
    // pair 2.19-2.22 ms instead of 2.46.  A band is walked row by row (one workgroup barrier per row, ~1.3 us each): with
    // few pairs per call the band height IS the kernel's latency (one 1242x375 frame in 32-row bands: 12 workgroups,
    // 47 us), so small calls get bands down to max(4, 2 * radius) rows.
    static const int bands_env = [] { const char* e = getenv("ADF_CONF_BANDS_TOTAL"); return e ? atoi(e) : 0; }();   // A/B knob
    int bands_total = bands_env;
    if (bands_total <= 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
        const int cus = cu_count(dev);
        // a quarter of the CUs left to the weight kernel (and the fill) alone: radius 2 -- both finish together, 1.82 / 1.92 ms
        // instead of 1.35 / 2.0 with a band on every CU, the step 13.12-13.18 -> 13.04-13.09 ms; radius 3 -- 13.55-13.78 ->
        // 13.09-13.13 ms; radius 5 on the StereoBM factory's ROI -- 13.87-14.16 -> 13.69-13.96 (the band kernels of radius 4..8
        // fill a SIMD's registers with four waves: nothing runs BESIDE them, but the fill no longer crawls behind them)
        // (narrow ROIs make small band workgroups, several of which share a CU: ask the runtime how many -- 256 frames of
        // 1242x375 per call lost 6 % with one tall band per frame)
        const int per_cu = conf_band_resident(radius, sh, dev);   // (at least 1)
        // (after the slide's instruction diet the kernels whose registers leave room for a wave of the weight kernel beside
        // the band's four on a SIMD -- at most 104 per lane: radius 1..3, and 4..5 since their right-view ring moved to
        // LDS -- do better with a band on EVERY CU: radius 2 12.81-13.24 against 13.05-13.20 ms per 64 x 4K step, four
        // alternating runs each; radius 3 12.78-13.22 against 13.18-13.33; StereoBM factory's geometry (radius 5)
        // 13.04-13.17 against 13.46-13.63, and 13.59-13.64 with the ring in registers; radius 4 13.02-13.17 against 13.54.
        // Radius 6..8 (108..128 registers) keep the quarter free: radius 6 13.65-13.78 against 13.92)
        // (narrow ROIs, whose small band workgroups share a CU, keep the quarter free at every radius: 256 frames of
        // 1242x375 per call 2.95-2.97 against 3.06 ms)
        const int quarters = radius <= 5 && per_cu == 1 ? 4 : 3;
        bands_total = cus * quarters / 4 * per_cu;
    }
    const int bands = (bands_total + n_pairs - 1) / n_pairs;
    return conf_band_clamp_rows((g.rh + bands - 1) / bands, g.rh, radius);
}

hipError_t launch_conf_band(const ConfBandArgs& a0, int n_pairs, hipStream_t st)
{
    if (!conf_band_fits(a0.g, a0.radius)) return hipErrorInvalidValue;
    ConfBandArgs a = a0;
    const BandShape sh = conf_band_shape(a.g, a.radius);
    a.rows_per_band = conf_band_rows_per_band(a.g, a.radius, sh, n_pairs);
    const dim3 grid((a.g.rh + a.rows_per_band - 1) / a.rows_per_band, n_pairs), block(64 * sh.waves);
    const BandKernel k = conf_band_variant(a.radius, sh.rlds);
    if (!k) return hipErrorInvalidValue;
    hipError_t e = ensure_dynamic_lds(k, sh.lds, 48 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, grid, block, sh.lds, st, a);
    return hipGetLastError();
}

// The merged preparation launch: for calls small enough that three kernels' latencies, not their work, are the time.
bool prep_small_fits(const Geom& g, int radius, int channels, int n_pairs)
{
    return conf_band_fits(g, radius) && radius <= 5 && (channels == 1 || channels == 3) &&
           (double)g.rw * g.rh * n_pairs <= 2.5e6;
}

// (the weight role reads the guide through a 32-bit buffer descriptor per block: prep_bodies.h)
bool prep_small_guide_fits(const Geom& g, ptrdiff_t guide_stride, int channels)
{
    return guide_stride > 0 && (size_t)(g.rh + 1) * (size_t)guide_stride < ((size_t)1 << 30) && (size_t)g.W * channels < ((size_t)1 << 29);
}

hipError_t launch_prep_small(const ConfBandArgs& c0, const WeightArgs& w, const OutsideArgs& o, int n_pairs, hipStream_t st)
{
    if (!prep_small_fits(c0.g, c0.radius, w.ch, n_pairs)) return hipErrorInvalidValue;
    if (!(w.chor_orient == ORIENT_N && w.cvert_orient == ORIENT_STRIP)) return hipErrorInvalidValue;
    if (!prep_small_guide_fits(c0.g, w.stride, w.ch)) return hipErrorInvalidValue;
    PrepArgs a{};
    a.c = c0; a.w = w; a.o = o;
    const Geom& g = c0.g;
    const BandShape sh = conf_band_shape(g, c0.radius);
    int waves = sh.waves;
    if (waves < prep::WS_NT / 64) waves = prep::WS_NT / 64;
    if (waves < NT / 64) waves = NT / 64;                  // (the fill role works in blocks of NT threads)
    // short bands and few rows per weight block: every role is walked row by row, a barrier per row
    // (as short as the halo allows while that still leaves no more than about one band per CU, and about two weight
    // blocks per CU: beyond that the roles only queue behind each other)
    const int rows_all = g.rh * n_pairs;
    const int rpb = conf_band_clamp_rows((rows_all + 255) / 256, g.rh, c0.radius);
    a.c.rows_per_band = rpb;
    a.nC = (g.rh + rpb - 1) / rpb;
    a.nWx = (g.rw + prep::WS_BCOLS - 1) / prep::WS_BCOLS;
    int wrows = (rows_all * a.nWx + 511) / 512;
    if (wrows < 4) wrows = 4;
    a.nWy = (g.rh + wrows - 1) / wrows;
    a.nW = a.nWx * a.nWy;
    const OutsideGrid og = outside_grid(g);
    if (!og.in_range) return hipErrorInvalidValue;
    a.nOAx = og.nAx; a.nOA = og.nA;
    const dim3 grid(a.nC + a.nW + og.nA + (int)og.nB, n_pairs), block(64 * waves);
    if (sh.lds + sizeof(prep::WsShared<3>) > 150 * 1024) return hipErrorInvalidValue;
    const auto k = dispatch_radius<1, 5>(c0.radius, [&](auto R) {
        return w.ch == 1 ? &prep_small_kernel<1, decltype(R)::value> : &prep_small_kernel<3, decltype(R)::value>;
    });
    if (!k) return hipErrorInvalidValue;
    hipError_t e = ensure_dynamic_lds(k, sh.lds, 32 * 1024);   // (lower than elsewhere: the kernel's static WsShared counts too)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, grid, block, sh.lds, st, a);
    return hipGetLastError();
}

hipError_t launch_conf_left(const ConfLeftArgs& a, int n_pairs, hipStream_t st)
{
    if (a.radius < 0 || a.radius > 8) return hipErrorInvalidValue;
    const auto k = dispatch_radius<0, 8>(a.radius, [&](auto R) {   // with or without the right-hand sides (WRITE_U)
        return a.U0 ? &conf_left_kernel<decltype(R)::value, true> : &conf_left_kernel<decltype(R)::value, false>;
    });
    hipLaunchKernelGGL(k, col_grid(a.g.rw, a.g.rh, a.radius, n_pairs), dim3(NT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_outside(const OutsideArgs& a, int n_pairs, hipStream_t st)
{
    const OutsideGrid og = outside_grid(a.g);
    if (og.nA + og.nB == 0) return hipSuccess;
    if (!og.in_range) return hipErrorInvalidValue;
    hipLaunchKernelGGL(outside_kernel, dim3((unsigned)(og.nA + og.nB), 1, n_pairs), dim3(NT), 0, st, a, og.nAx, og.nA);
    return hipGetLastError();
}

} // namespace adf
