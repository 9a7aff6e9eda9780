// sgbm_matcher.hip -- semi-global matcher on the device (second producer).
//
// The reference's sample feeds the filter from cv::StereoSGBM with MODE_SGBM_3WAY
// (samples/disparity_filtering.cpp:166-176); the filter factories only touch its parameters
// (disparity_filters.cpp:404-409, 432-445).  cv::StereoSGBM lives in OpenCV's calib3d, outside the reference tree:
// PARITY UNPINNED there.  What is built is the published algorithm (Hirschmueller 2008, formula 13, three paths,
// Birchfield-Tomasi block cost) exactly as oracle/adf_oracle_sgbm.c states it -- integer work, bit-identical to that
// oracle -- with the in-tree derivative of OpenCV's aggregation loop (modules/stereo/src/stereo_binary_sgbm.cpp) as
// the line-cited anchor of the recurrence, the winner / tie rule, the uniqueness test and the sub-pixel fit.
//
// Five kernels per call, all integer, none with a dense contraction (no MFMA):
//   sgbm_signals_kernel   per pixel and channel: clipped x-derivative + intensity, each with the extrema over its
//                         half-sample neighbours, packed as 16-bit pairs (derivative | intensity) so that one packed
//                         instruction serves both Birchfield-Tomasi terms
//   sgbm_cost_kernel      block cost volume C[y][x][d] (int16): lanes along x, 16 (8) disparities per wave, walking down
//                         a band of rows; one pixel cost per lane, row and disparity, the horizontal window from the
//                         neighbouring lanes by DPP, the vertical one as a running sum over a register ring
//                         (stereo_binary_sgbm.cpp:205-276 is the same running-sum structure)
//   sgbm_path_kernel      formula 13 along one direction, one wavefront per scanline, the D path costs of a pixel held
//                         4 (2, 1, 8) per lane; d-1 / d+1 across lanes by whole-wave DPP shifts, min_k by a DPP
//                         butterfly + 4 readlanes.  TOP writes the volume S, LEFT adds to it, RIGHT adds, picks the
//                         winner and fits the sub-pixel parabola (stereo_binary_sgbm.cpp:286-301, 419-446, 519-596)
//   sgbm_fill_kernel / sgbm_median_kernel   invalid value everywhere first; 3x3 median of the CV_16S map last
// ADF_SGBM_COST_CENSUS_* (adf_sgbm_set_cost) swaps the first two for the census transform (census_kernels.hip) and a
// Hamming pixel cost -- what the reference's own matcher, cv::stereo::StereoBinarySGBM, matches on -- through the same
// cost kernel (the pixel cost is its template policy, its bound census.h's); everything from the volume C on is the same code.
// HBM: C, S and L2 volumes of H x width1 x D int16 each (4K, 256 disparities: 4 GB each, per image in flight).
#include "census.h"

#include <algorithm>
#include <cstdlib>
#include <new>

using namespace adf;

namespace {

constexpr int SG_MAX_COST = 32767;   // SHRT_MAX: guard value of the d = -1 / d = D neighbours (stereo_binary_sgbm.cpp:323-324)
constexpr int SG_DISP_SHIFT = 4, SG_DISP_SCALE = 16;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int sat16i(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// ---------------------------------------------------------------------------------------------------------------
// signals: rec[(y*W + x)*cn + c] = {V, V0, V1}, each (derivative | intensity << 16) of channel c
// ---------------------------------------------------------------------------------------------------------------
struct SignalArgs {
    const uint8_t* img; ptrdiff_t stride, pair_stride; int cn, W, H, ftzero;
    uint32_t* rec; size_t rec_pair;     // dwords per image
};

__device__ __forceinline__ uint32_t sg_signal(const uint8_t* row, const uint8_t* up, const uint8_t* dn, int x, int c, int cn, int W, int ftzero)
{
    if (x <= 0 || x >= W - 1) return (uint32_t)ftzero | ((uint32_t)ftzero << 16);     // border columns hold ftzero
    const int a = x * cn + c;
    int g = (row[a + cn] - row[a - cn]) * 2 + up[a + cn] - up[a - cn] + dn[a + cn] - dn[a - cn];
    g = min(max(g, -ftzero), ftzero) + ftzero;
    return (uint32_t)g | ((uint32_t)row[a] << 16);
}

__global__ void __launch_bounds__(256) sgbm_signals_kernel(SignalArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const uint8_t* row = a.img + (ptrdiff_t)blockIdx.z * a.pair_stride + (ptrdiff_t)y * a.stride;
    const uint8_t* up = y > 0 ? row - a.stride : row;
    const uint8_t* dn = y < a.H - 1 ? row + a.stride : row;
    uint32_t* o = a.rec + (size_t)blockIdx.z * a.rec_pair + ((size_t)y * a.W + x) * a.cn * 3;
    for (int c = 0; c < a.cn; c++) {
        const uint32_t v = sg_signal(row, up, dn, x, c, a.cn, a.W, a.ftzero);
        const uint32_t l = sg_signal(row, up, dn, x - 1, c, a.cn, a.W, a.ftzero);
        const uint32_t r = sg_signal(row, up, dn, x + 1, c, a.cn, a.W, a.ftzero);
        uint32_t out0 = 0, out1 = 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {                          // the two signals of the pair
            const int vv = (v >> (16 * h)) & 0xffff, ll = (l >> (16 * h)) & 0xffff, rr = (r >> (16 * h)) & 0xffff;
            const int vl = x > 0 ? (vv + ll) / 2 : vv;
            const int vr = x < a.W - 1 ? (vv + rr) / 2 : vv;
            out0 |= (uint32_t)min(min(vl, vr), vv) << (16 * h);
            out1 |= (uint32_t)max(max(vl, vr), vv) << (16 * h);
        }
        o[c * 3 + 0] = v; o[c * 3 + 1] = out0; o[c * 3 + 2] = out1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// block costs
// ---------------------------------------------------------------------------------------------------------------
struct CostArgs {
    const uint32_t* rec1; const uint32_t* rec2; size_t rec_pair;     // what the pixel cost reads, per image; dwords per image
    int16_t* C; size_t vol;              // int16 elements per image volume = H * w1 * D
    int W, H, D, minD, minX1, w1, rows_per_band;
};

struct Rec { uint32_t v, v0, v1; };

// Birchfield-Tomasi cost of the pair of signals: distance of u to [v0, v1] and of v to [u0, u1], the smaller one, as
// saturating 16-bit pairs (v0 <= v1, so at most one of the two differences of a distance is non-zero); the intensity
// half is scaled by 1/4 before the terms are summed.
__device__ __forceinline__ us2 bt_pair(const Rec& u, const Rec& v)
{
    const us2 U = __builtin_bit_cast(us2, u.v), U0 = __builtin_bit_cast(us2, u.v0), U1 = __builtin_bit_cast(us2, u.v1);
    const us2 V = __builtin_bit_cast(us2, v.v), V0 = __builtin_bit_cast(us2, v.v0), V1 = __builtin_bit_cast(us2, v.v1);
    const us2 c0 = __builtin_elementwise_sub_sat(V0, U) | __builtin_elementwise_sub_sat(U, V1);
    const us2 c1 = __builtin_elementwise_sub_sat(U0, V) | __builtin_elementwise_sub_sat(V, U1);
    const us2 m = __builtin_elementwise_min(c0, c1);
    const us2 sh = {0, 2};
    return m >> sh;
}

// The pixel cost is a policy of the cost kernel: DWORDS per pixel of the planes it reads, MAX_PIXEL (the largest cost of
// one pixel: whether two disparities fit a register), Own (a lane's image-1 pixel, loaded once per row) and
// cost(own, q) against the image-2 pixel at q.
template <int CN>
struct BtCost {                                               // the signal records of sgbm_signals_kernel
    static constexpr int DWORDS = CN * 3, MAX_PIXEL = CN * 189;   // (derivative distance <= 2 * 63, intensity distance <= 255 / 4)
    struct Own { Rec u[CN]; };
    static __device__ __forceinline__ Own own(const uint32_t* p)
    {
        Own o;
#pragma unroll
        for (int c = 0; c < CN; c++) o.u[c] = Rec{p[c * 3], p[c * 3 + 1], p[c * 3 + 2]};
        return o;
    }
    static __device__ __forceinline__ uint32_t cost(const Own& o, const uint32_t* q)
    {
        us2 acc = {0, 0};
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const Rec v = {q[c * 3], q[c * 3 + 1], q[c * 3 + 2]};
            acc += bt_pair(o.u[c], v);
        }
        return (uint32_t)acc.x + (uint32_t)acc.y;
    }
};

struct CensusCost {                                           // the descriptor planes of census_kernel: one 8-byte load, one xor, two bit counts
    static constexpr int DWORDS = 2, MAX_PIXEL = CENSUS_MAX_BITS;   // (census.h pins every descriptor to at most that many bits)
    struct Own { uint64_t c; };
    static __device__ __forceinline__ Own own(const uint32_t* p) { return Own{*reinterpret_cast<const uint64_t*>(p)}; }
    static __device__ __forceinline__ uint32_t cost(const Own& o, const uint32_t* q)
    {
        return (uint32_t)__builtin_popcountll(o.c ^ *reinterpret_cast<const uint64_t*>(q));
    }
};

// Lanes run along x: lane = one matchable column (the first and last BS/2 lanes of a wave are halo and repeat the edge
// column at the borders of the matchable area = the clamped window), wave = DD consecutive disparities of 64 - 2*(BS/2)
// output columns, workgroup = 4 waves = 4*DD disparities of the same columns (their int16 results are one contiguous
// piece per column).  Per row and disparity a lane evaluates ONE pixel cost (its own column of image 1 against column
// x - d of image 2: consecutive lanes read consecutive records) and receives its neighbours' through whole-wave DPP
// shifts; the vertical window is a running sum over a register ring with static slots (the row loop is unrolled by BS).
template <int BS, class COST, int DD>
__global__ void __launch_bounds__(256) sgbm_cost_kernel(CostArgs a)
{
    constexpr int R = BS / 2, OUTW = 64 - 2 * R;
    constexpr int TD = 4 * DD;                                // disparities of the workgroup: one contiguous piece per column
    constexpr int TP = TD + 8;                                // LDS row pitch in int16 (16-byte aligned, staggers the banks)
    __shared__ __align__(16) int16_t tile[2][64 * TP];        // the workgroup's results of one row, [column][disparity]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int dbase = blockIdx.y * TD, d0 = dbase + wv * DD;
    const bool wave_active = d0 < a.D;                        // (D is a multiple of 16, DD is 8 or 16: all or nothing per wave)
    const int nbands = (a.H + a.rows_per_band - 1) / a.rows_per_band;
    const int img = blockIdx.z / nbands, band = blockIdx.z % nbands;
    const int y0 = band * a.rows_per_band;
    const int rows_out = min(a.rows_per_band, a.H - y0);
    const int xt0 = blockIdx.x * OUTW;
    const int x1 = xt0 + lane - R;
    const int X = a.minX1 + min(max(x1, 0), a.w1 - 1);         // image column (window clamped inside the matchable area)
    const uint32_t* rec1 = a.rec1 + (size_t)img * a.rec_pair;
    const uint32_t* rec2 = a.rec2 + (size_t)img * a.rec_pair;
    int16_t* C = a.C + (size_t)img * a.vol;
    const int dl = wave_active ? d0 : dbase;                  // idle waves walk along (they share the barriers and the stores)
    // Round 4: TWO disparities share a register from the pixel cost on (low / high half) wherever the block sum fits 16
    // bits -- a Birchfield-Tomasi pixel cost is at most 189 per channel, a Hamming one at most 48 --
    // so the window shifts, the running sums and the clamp run once per pair: about a third fewer vector instructions
    // in a kernel that is bound by issuing them.  (Sums of halves never carry: every intermediate stays below 2^16, and
    // the ring entry is subtracted from the running sum BEFORE the new one is added.)
    constexpr bool PACK = BS * BS * COST::MAX_PIXEL < 65536;
    int ring[PACK ? 1 : BS][PACK ? 1 : DD], csum[PACK ? 1 : DD];
    uint32_t ring2[PACK ? BS : 1][PACK ? DD / 2 : 1], csum2[PACK ? DD / 2 : 1];
    if constexpr (PACK) {
#pragma unroll
        for (int j = 0; j < DD / 2; j++) {
            csum2[j] = 0;
#pragma unroll
            for (int k = 0; k < BS; k++) ring2[k][j] = 0;
        }
    } else {
#pragma unroll
        for (int dd = 0; dd < DD; dd++) {
            csum[dd] = 0;
#pragma unroll
            for (int k = 0; k < BS; k++) ring[k][dd] = 0;
        }
    }
    // write-out: 16 bytes per thread, TD/8 threads per column => every store instruction covers whole contiguous pieces
    constexpr int TPC = TD / 8;                               // threads per column
    const int nd_blk = min(TD, a.D - dbase);                  // disparities this workgroup really has
    const int nsteps = rows_out + BS - 1;
    for (int n0 = 0; n0 < nsteps; n0 += BS) {
#pragma unroll
        for (int s = 0; s < BS; s++) {
            const int n = n0 + s;
            if (n < nsteps) {                                    // block-uniform
                const int yy = min(max(y0 - R + n, 0), a.H - 1);
                const uint32_t* pv = rec2 + ((size_t)yy * a.W + (X - (dl + a.minD))) * COST::DWORDS;
                const typename COST::Own u = COST::own(rec1 + ((size_t)yy * a.W + X) * COST::DWORDS);
                short res[PACK ? 1 : DD];
                uint32_t res2[PACK ? DD / 2 : 1];
                auto pixel_cost = [&](int dd) -> uint32_t {
                    return COST::cost(u, pv - dd * COST::DWORDS);                 // column X - (d0 + dd + minD)
                };
                if constexpr (PACK) {
#pragma unroll
                    for (int j = 0; j < DD / 2; j++) {
                        const uint32_t pp = pixel_cost(2 * j) | (pixel_cost(2 * j + 1) << 16);
                        uint32_t hs = pp, tl = pp, tr = pp;
#pragma unroll
                        for (int k = 0; k < R; k++) {               // neighbours' pixel costs, one more column per shift
                            tl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tl, 0x138, 0xf, 0xf, true);   // wave_shr:1, 0 past the wave's end
                            tr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tr, 0x130, 0xf, 0xf, true);   // wave_shl:1
                            hs += tl + tr;
                        }
                        csum2[j] = (csum2[j] - ring2[s][j]) + hs;
                        ring2[s][j] = hs;
                        const us2 cl = __builtin_elementwise_min(__builtin_bit_cast(us2, csum2[j]), (us2){(unsigned short)SG_MAX_COST, (unsigned short)SG_MAX_COST});
                        res2[j] = __builtin_bit_cast(uint32_t, cl);
                    }
                } else {
#pragma unroll
                for (int dd = 0; dd < DD; dd++) {
                    const int pix = (int)pixel_cost(dd);
                    int hs = pix, tl = pix, tr = pix;
#pragma unroll
                    for (int k = 0; k < R; k++) {                   // neighbours' pixel costs, one more column per shift
                        tl = __builtin_amdgcn_update_dpp(0, tl, 0x138, 0xf, 0xf, false);   // wave_shr:1
                        tr = __builtin_amdgcn_update_dpp(0, tr, 0x130, 0xf, 0xf, false);   // wave_shl:1
                        hs += tl + tr;
                    }
                    csum[dd] += hs - ring[s][dd];
                    ring[s][dd] = hs;
                    res[dd] = (short)min(csum[dd], SG_MAX_COST);
                }
                }
                if (n >= BS - 1) {                               // block-uniform: a row of results goes out through LDS
                    typedef short v8s __attribute__((ext_vector_type(8)));
                    int16_t* tl_ = tile[n & 1];
                    if (wave_active) {
#pragma unroll
                        for (int h = 0; h < DD / 8; h++) {
                            if constexpr (PACK) {
                                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                                *reinterpret_cast<v4u*>(tl_ + lane * TP + wv * DD + h * 8) = v4u{res2[4 * h], res2[4 * h + 1], res2[4 * h + 2], res2[4 * h + 3]};
                            } else {
                                v8s q;
#pragma unroll
                                for (int k = 0; k < 8; k++) q[k] = res[h * 8 + k];
                                *reinterpret_cast<v8s*>(tl_ + lane * TP + wv * DD + h * 8) = q;
                            }
                        }
                    }
                    __syncthreads();
                    int16_t* dst = C + (size_t)(y0 + n - (BS - 1)) * a.w1 * a.D + dbase;
                    const int part = threadIdx.x % TPC;
#pragma unroll
                    for (int col = threadIdx.x / TPC; col < OUTW; col += 256 / TPC) {
                        const int xo = xt0 + col;
                        if (xo < a.w1 && part * 8 < nd_blk)
                            *reinterpret_cast<v8s*>(dst + (size_t)xo * a.D + part * 8) = *reinterpret_cast<const v8s*>(tl_ + (col + R) * TP + part * 8);
                    }
                    // (the other tile buffer is written next: one barrier per row is enough)
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// path costs
// ---------------------------------------------------------------------------------------------------------------
// DIR_TOP: first path, writes S; DIR_ADD: any direction of travel (dx, dy) in {-1,0,1}^2, adds to S; DIR_RIGHT: the last
// path (from the right), adds, picks the winner
// DIR_ADD_OUT (round 4): the LAST accumulating path writes its costs to a volume of its own (L2) instead of adding them into
// S -- it no longer reads S (8 bytes per pixel and disparity moved instead of 12) -- and DIR_RIGHT, which is bound by
// vector issue and has bandwidth to spare, reads both and adds them in the accumulation's own order:
// sat(sat(S + L_last) + L_right).
// DIR_RIGHT_BOTH: DIR_RIGHT that also takes the RIGHT view's raw map from the same registers (include/adf_wls.h,
// ADF_SGBM_RIGHT_FROM_VOLUME): the final S(x, d) of the left view is a cost of (right column x - d, d).
enum { DIR_TOP = 0, DIR_ADD = 1, DIR_RIGHT = 2, DIR_ADD_OUT = 3, DIR_RIGHT_BOTH = 4 };

struct PathArgs {
    const int16_t* C; int16_t* S; int16_t* L2; size_t vol;
    int W, H, D, minD, minX1, w1, P1, P2, ur;
    int16_t* out; ptrdiff_t out_stride, out_pair;   // raw disparity map (elements)
    int dx, dy;                                     // DIR_ADD: direction of travel
    int disp12;                                     // DIR_RIGHT: the matcher's own left-right check (>= 100000: off)
    int16_t* out_r; ptrdiff_t out_r_stride, out_r_pair;   // DIR_RIGHT_BOTH: the right view's raw map (elements)
    int ring;                                       // DIR_RIGHT_BOTH: slots of a wave's ring of live right columns (sgbm_ring)
};

__device__ __forceinline__ int wave_min_i32(int v)
{
    // min is idempotent: rotations by 1, 2, 4, 8 inside each row of 16 lanes leave the row minimum in every lane
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));   // row_ror:1
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));   // row_ror:2
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));   // row_ror:4
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));   // row_ror:8
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), e = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, e));
}

// num / den truncated toward zero (C semantics) for |num|, den < 2^24, den > 0: float quotient + one exact correction
// step instead of the ~40-instruction integer division sequence.
__device__ __forceinline__ int div_trunc_small(int num, int den)
{
    int q = (int)((float)num * __builtin_amdgcn_rcpf((float)den));       // truncation toward zero, off by at most one
    int r = num - q * den;
    if (num >= 0) { if (r < 0) { q--; } else if (r >= den) { q++; } }
    else          { if (r > 0) { q++; } else if (r <= -den) { q--; } }
    return q;
}

template <int DPL>
__device__ __forceinline__ void load_costs(const int16_t* p, int (&o)[DPL])
{
    // unconditional (lanes without disparities read lane 0's and ignore them): no load under a branch
    typedef short vs __attribute__((ext_vector_type(DPL)));
    if constexpr (DPL == 1) o[0] = p[0];
    else {
        const vs q = *reinterpret_cast<const vs*>(p);
#pragma unroll
        for (int k = 0; k < DPL; k++) o[k] = q[k];
    }
}

template <int DPL>
__device__ __forceinline__ void store_costs(int16_t* p, bool active, const int (&v)[DPL])
{
    typedef short vs __attribute__((ext_vector_type(DPL)));
    if (!active) return;
    if constexpr (DPL == 1) p[0] = (int16_t)v[0];
    else {
        vs q;
#pragma unroll
        for (int k = 0; k < DPL; k++) q[k] = (short)v[k];
        *reinterpret_cast<vs*>(p) = q;
    }
}

template <int DPL, int DIR>
__global__ void __launch_bounds__(256) sgbm_path_kernel(PathArgs a)
{
    __shared__ int16_t sS[4][64 * DPL];                       // DIR_RIGHT: the pixel's S(d) for the sub-pixel fit
    extern __shared__ int16_t sOut[];                         // DIR_RIGHT: [4][w1] the scanline's results (written out coalesced),
                                                              // then [4][W] disp2 and [4][W] its cost (left-right check)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr bool WIN = DIR == DIR_RIGHT || DIR == DIR_RIGHT_BOTH, BOTH = DIR == DIR_RIGHT_BOTH;
    const int line = blockIdx.x * 4 + wv;                     // scanline: a column (TOP), a row (RIGHT), any straight line (ADD)
    // scanline -> first pixel (x0, y0), direction (dx, dy), length.  Diagonals: one line per pixel of the row the
    // path enters through, then one per remaining pixel of the column it enters through.
    int dx, dy, x0, y0, nlines, nsteps;
    if (DIR == DIR_TOP) { dx = 0; dy = 1; nlines = a.w1; x0 = line; y0 = 0; nsteps = a.H; }
    else if (WIN) { dx = -1; dy = 0; nlines = a.H; x0 = a.w1 - 1; y0 = line; nsteps = a.w1; }
    else {
        dx = a.dx; dy = a.dy;
        const int ys = dy > 0 ? 0 : a.H - 1, xs = dx > 0 ? 0 : a.w1 - 1;
        if (dy == 0) { nlines = a.H; x0 = xs; y0 = line; nsteps = a.w1; }
        else if (dx == 0) { nlines = a.w1; x0 = line; y0 = ys; nsteps = a.H; }
        else {
            nlines = a.w1 + a.H - 1;
            if (line < a.w1) { x0 = line; y0 = ys; }
            else { const int j = line - a.w1 + 1; x0 = xs; y0 = dy > 0 ? j : a.H - 1 - j; }
            const int nx = dx > 0 ? a.w1 - x0 : x0 + 1, ny = dy > 0 ? a.H - y0 : y0 + 1;
            nsteps = min(nx, ny);
        }
    }
    if (line >= nlines) return;
    const int d0 = lane * DPL;
    const bool active = d0 < a.D;
    const size_t vol0 = (size_t)blockIdx.y * a.vol;
    // a lane's DPL disparities are all inside [0, D) or all outside (D is a multiple of 16, DPL divides 16)
    const int16_t* C = a.C + vol0 + (active ? d0 : 0);
    int16_t* S = a.S + vol0 + (active ? d0 : 0);
    int16_t* L2 = a.L2 + vol0 + (active ? d0 : 0);
    constexpr bool READS_S = DIR == DIR_ADD || WIN;
    // element offset of step t
    auto offs = [&](int t) -> size_t {
        return ((size_t)(y0 + t * dy) * a.w1 + (size_t)(x0 + t * dx)) * a.D;
    };
    int L[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) L[k] = active ? 0 : SG_MAX_COST;      // zero start (stereo_binary_sgbm.cpp:191-194)
    int minprev = 0;
    const int16_t invalid = (int16_t)((a.minD - 1) * SG_DISP_SCALE);
    int16_t* myOut = sOut + wv * a.w1;
    // the matcher's own left-right check (stereo_binary_sgbm.cpp:548-556, 598-613): disp2 = per column of image 2 the
    // disparity of the cheapest winner pointing at it, kept in LDS for the row
    const bool lrc = WIN && a.disp12 < 100000;
    int16_t* d2p = sOut + 4 * a.w1 + wv * a.W;
    int16_t* d2c = sOut + 4 * a.w1 + 4 * a.W + wv * a.W;
    if (lrc)
        for (int x = lane; x < a.W; x += 64) { d2p[x] = invalid; d2c[x] = (int16_t)SG_MAX_COST; }   // :449-453

    // DIR_RIGHT_BOTH: the right view's map from the same S (include/adf_wls.h, ADF_SGBM_RIGHT_FROM_VOLUME).  S(x1, d) is the
    // cost of candidate d of the right column xr = x1 + cR - d.  The row is walked from the right, so the candidates of one
    // xr arrive one per step in DESCENDING d: a strict `<` keeps the largest d of the smallest cost, and xr is finished by
    // the step that brings its d = 0.  The fit of candidate (xc, d) reads S(xc+1, d+1) and S(xc-1, d-1): h1 / h2 keep the
    // previous two steps' st, and the candidates of column xc are entered one step late, when column xc-1 is known.
    //   ringR  per wave, a ring of a.ring >= D live right columns, 8 bytes each: x = cost << 16 | fit << 15 | d,
    //          y = S(d+1) | S(d-1) << 16; an empty slot holds cost SHRT_MAX, which no candidate beats
    //   rOut   per wave, the row's W raw values, written out coalesced after the loop
    // Within a step the lanes' xr are distinct, and a wave's LDS operations stay in order across steps: no atomics.
    typedef uint32_t us2x __attribute__((ext_vector_type(2)));
    constexpr uint32_t RING_EMPTY = (uint32_t)SG_MAX_COST << 16;
    const int base_r = 4 * a.w1 + (lrc ? 8 * a.W : 0);        // int16 elements of sOut before this variant's part
    int16_t* rOut = sOut + base_r + wv * a.W;
    us2x* ringR = reinterpret_cast<us2x*>(sOut + base_r + 4 * a.W) + wv * a.ring;
    const int cR = a.minX1 - a.minD;
    const int invalid_r = -(a.minD + a.D) * SG_DISP_SCALE;
    int h1[BOTH ? DPL : 1], h2[BOTH ? DPL : 1];
    if constexpr (BOTH) {
#pragma unroll
        for (int k = 0; k < DPL; k++) h1[k] = h2[k] = SG_MAX_COST;
        for (int x = lane; x < a.W; x += 64) rOut[x] = (int16_t)invalid_r;
        for (int i = lane; i < a.ring; i += 64) ringR[i] = us2x{RING_EMPTY, 0};
    }
    // a finished slot -> the raw value, in the right matcher's own index d' = D-1-d (stereo_binary_sgbm.cpp:584-596 there)
    auto right_value = [&](uint32_t e0, uint32_t e1) -> int {
        const int m = (int)e0 >> 16, d = (int)(e0 & 1023);
        int v = (a.D - 1 - d) * SG_DISP_SCALE;
        if (e0 & 0x8000u) {
            const int sp = (int)(short)(e1 & 0xffffu), sm = (int)e1 >> 16;        // S(d+1) = S'(d'-1), S(d-1) = S'(d'+1)
            const int denom2 = max(sp + sm - 2 * m, 1);
            v += div_trunc_small((sp - sm) * SG_DISP_SCALE + denom2, denom2 * 2);
        }
        return m >= SG_MAX_COST ? invalid_r : v + (1 - a.minD - a.D) * SG_DISP_SCALE;
    };
    // the candidates of column xc (costs h1) once `cur` = column xc-1 is known (below_ok) or known not to exist
    auto right_candidates = [&](int xc, const int (&cur)[BOTH ? DPL : 1], bool below_ok) {
        if constexpr (!BOTH) return;
        else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // (compiler only: the previous step's slots are written)
        const int up = __builtin_amdgcn_update_dpp(SG_MAX_COST, h2[0], 0x130, 0xf, 0xf, false);               // wave_shl:1: S(xc+1, d0+DPL)
        const int dn = __builtin_amdgcn_update_dpp(SG_MAX_COST, cur[DPL - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1: S(xc-1, d0-1)
        const bool sides_ok = below_ok && xc + 1 < a.w1;
        const int xr0 = xc + cR - d0;
#pragma unroll
        for (int k = 0; k < DPL; k++) {
            const int d = d0 + k;
            const int sp = k == DPL - 1 ? up : h2[k + 1 < DPL ? k + 1 : k], sm = k == 0 ? dn : cur[k > 0 ? k - 1 : 0];
            const bool fit = sides_ok && d > 0 && d < a.D - 1;
            const us2x mine = {((uint32_t)h1[k] << 16) | (fit ? 0x8000u : 0u) | (uint32_t)d, ((uint32_t)sp & 0xffffu) | ((uint32_t)sm << 16)};
            us2x* slot = ringR + ((xr0 - k) & (a.ring - 1));
            if (k == 0) {                                      // lane 0's is d = 0: the last candidate of its column
                const us2x old = *slot;
                const bool win = active && h1[0] < ((int)old.x >> 16);
                if (lane == 0) {
                    const us2x f = win ? mine : old;
                    rOut[xr0] = (int16_t)right_value(f.x, f.y);
                    *slot = us2x{RING_EMPTY, 0};
                } else if (win)
                    *slot = mine;
            } else if (active && h1[k] < ((int)slot->x >> 16))
                *slot = mine;
        }
        }
    };

    // one step of formula 13 at scanline position t with the operands c (block cost) and s (S so far)
    auto step = [&](int t, const int (&c)[DPL], const int (&s_in)[DPL], const int (&l2)[DPL]) {
        int s[DPL];
#pragma unroll
        for (int k = 0; k < DPL; k++) s[k] = WIN ? sat16i(s_in[k] + l2[k]) : s_in[k];   // the last accumulating path's costs
        const size_t o = offs(t);
        // stereo_binary_sgbm.cpp:419-446: neighbours d-1 / d+1, guards SHRT_MAX outside [0, D)
        const int lm = __builtin_amdgcn_update_dpp(SG_MAX_COST, L[DPL - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1
        const int lp = __builtin_amdgcn_update_dpp(SG_MAX_COST, L[0], 0x130, 0xf, 0xf, false);         // wave_shl:1
        const int delta = minprev + a.P2;
        int Ln[DPL], lmin = SG_MAX_COST;
#pragma unroll
        for (int k = 0; k < DPL; k++) {
            const int below = k == 0 ? lm : L[k - 1], above = k == DPL - 1 ? lp : L[k + 1];
            const int m = min(min(L[k], below + a.P1), min(above + a.P1, delta));
            Ln[k] = active ? sat16i(c[k] + m - delta) : SG_MAX_COST;      // :423: minus delta = min_k + P2, L in [C-P2, C]
            lmin = min(lmin, Ln[k]);
        }
#pragma unroll
        for (int k = 0; k < DPL; k++) L[k] = Ln[k];
        minprev = wave_min_i32(lmin);
        if (DIR == DIR_TOP) {
            store_costs<DPL>(S + o, active, Ln);
        } else if (DIR == DIR_ADD_OUT) {
            store_costs<DPL>(L2 + o, active, Ln);
        } else {
            int st[DPL];
#pragma unroll
            for (int k = 0; k < DPL; k++) st[k] = sat16i(s[k] + Ln[k]);
            if (DIR == DIR_ADD) {
                store_costs<DPL>(S + o, active, st);
            } else {
                // winner: the FIRST disparity with the smallest S (stereo_binary_sgbm.cpp:519-528) -- one wave minimum over
                // the key S*1024 + d: |S| < 2^15 (S is negative as a rule: every path cost lies in [C-P2, C]), d < 1024
                int key = 0x7fffffff;
#pragma unroll
                for (int k = 0; k < DPL; k++) if (active) key = min(key, st[k] * 1024 + (d0 + k));
                key = wave_min_i32(key);
                const int minS = key >> 10, best = key & 1023;
                bool reject = false;
                if (a.ur > 0) {                                // stereo_binary_sgbm.cpp:543-547
#pragma unroll
                    for (int k = 0; k < DPL; k++)
                        reject |= active && st[k] * (100 - a.ur) < minS * 100 && abs(best - (d0 + k)) > 1;
                }
                const bool any_reject = __builtin_amdgcn_ballot_w64(reject) != 0;
                store_costs<DPL>(&sS[wv][d0], active, st);
                // (results go to LDS only: no vector-memory operation under a branch inside the pipelined loop)
                int res = invalid;
                if (minS < SG_MAX_COST && !any_reject) {
                    int d = best < a.D ? best : 0;
                    if (lrc && lane == 0) {                   // :549-554 (x runs from the right: sequential in this wave)
                        const int x2 = (a.w1 - 1 - t) + a.minX1 - d - a.minD;
                        if (d2c[x2] > minS) { d2c[x2] = (int16_t)minS; d2p[x2] = (int16_t)(d + a.minD); }
                    }
                    const int dm = d > 0 ? d - 1 : 0, dp = d < a.D - 1 ? d + 1 : d;
                    const int sm = sS[wv][dm], s0 = sS[wv][d], sp = sS[wv][dp];
                    if (0 < d && d < a.D - 1) {                // stereo_binary_sgbm.cpp:584-591
                        const int denom2 = max(sm + sp - 2 * s0, 1);
                        d = d * SG_DISP_SCALE + div_trunc_small((sm - sp) * SG_DISP_SCALE + denom2, denom2 * 2);
                    } else
                        d *= SG_DISP_SCALE;
                    res = d + a.minD * SG_DISP_SCALE;           // :596
                }
                if (lane == 0) myOut[a.w1 - 1 - t] = (int16_t)res;
                if constexpr (BOTH) {
                    if (t > 0) right_candidates(a.w1 - t, st, true);       // (uniform; LDS only)
#pragma unroll
                    for (int k = 0; k < DPL; k++) { h2[k] = h1[k]; h1[k] = st[k]; }
                }
            }
        }
    };

    // Operands of the next PF steps are in flight while a step is reduced (a step is far shorter than a memory
    // latency).  The pipelined loop has NO branch around a vector-memory operation: with one, the compiler can only
    // wait for every outstanding load at each use, which serialises the ring.
    constexpr int PF = DPL >= 8 ? 4 : 8;
    int cq[PF][DPL], sq[PF][DPL], lq[WIN ? PF : 1][DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) lq[0][k] = 0;
#pragma unroll
    for (int p = 0; p < PF; p++) {
        const int tt = p < nsteps ? p : nsteps - 1;
        load_costs<DPL>(C + offs(tt), cq[p]);
        if (READS_S) load_costs<DPL>(S + offs(tt), sq[p]);
        else {
#pragma unroll
            for (int k = 0; k < DPL; k++) sq[p][k] = 0;
        }
        if (WIN) load_costs<DPL>(L2 + offs(tt), lq[p]);
    }
    int t0 = 0;
    for (; t0 + PF <= nsteps; t0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; p++) {
            const int t = t0 + p;
            int c[DPL], s[DPL], l2[DPL];
#pragma unroll
            for (int k = 0; k < DPL; k++) { c[k] = cq[p][k]; s[k] = sq[p][k]; l2[k] = lq[WIN ? p : 0][k]; }
            const int tt = t + PF < nsteps ? t + PF : nsteps - 1;
            load_costs<DPL>(C + offs(tt), cq[p]);
            if (READS_S) load_costs<DPL>(S + offs(tt), sq[p]);
            if (WIN) load_costs<DPL>(L2 + offs(tt), lq[p]);
            step(t, c, s, l2);
        }
    }
#pragma unroll
    for (int p = 0; p < PF; p++)                              // the last nsteps % PF steps: operands already in the ring
        if (t0 + p < nsteps) step(t0 + p, cq[p], sq[p], lq[WIN ? p : 0]);

    if constexpr (BOTH) {
        right_candidates(0, h1, false);                       // the candidates of column 0: nothing lies below them
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int j = lane + 1; j < a.D; j += 64) {            // the columns that never see d = 0 (partial ranges count)
            const us2x e = ringR[(cR - j) & (a.ring - 1)];
            rOut[cR - j] = (int16_t)right_value(e.x, e.y);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        int16_t* out_r = a.out_r + (ptrdiff_t)blockIdx.y * a.out_r_pair + (ptrdiff_t)line * a.out_r_stride;
        for (int x = lane; x < a.W; x += 64) out_r[x] = rOut[x];
    }
    if (WIN) {                                   // the scanline's results, coalesced
        int16_t* out = a.out + (ptrdiff_t)blockIdx.y * a.out_pair + (ptrdiff_t)line * a.out_stride + a.minX1;
        const int maxdiff = a.disp12 > 0 ? a.disp12 : 1;      // :141
        for (int x1 = lane; x1 < a.w1; x1 += 64) {
            int d1 = myOut[x1];
            if (lrc && d1 != invalid) {                       // :598-613: both roundings must disagree to invalidate
                const int x = x1 + a.minX1;
                const int dlo = d1 >> SG_DISP_SHIFT, dhi = (d1 + SG_DISP_SCALE - 1) >> SG_DISP_SHIFT;
                const int xlo = x - dlo, xhi = x - dhi;
                if (0 <= xlo && xlo < a.W && d2p[xlo] >= a.minD && abs(d2p[xlo] - dlo) > maxdiff &&
                    0 <= xhi && xhi < a.W && d2p[xhi] >= a.minD && abs(d2p[xhi] - dhi) > maxdiff)
                    d1 = invalid;
            }
            out[x1] = (int16_t)d1;
        }
    }
}

struct FillArgs { int16_t* p; ptrdiff_t stride, pair; int W, H; int16_t v; };
__global__ void __launch_bounds__(256) sgbm_fill_kernel(FillArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < a.W) a.p[(ptrdiff_t)blockIdx.z * a.pair + (ptrdiff_t)blockIdx.y * a.stride + x] = a.v;
}

struct MedianArgs { const int16_t* src; ptrdiff_t sstride, spair; int16_t* dst; ptrdiff_t dstride, dpair; int W, H; };
__device__ __forceinline__ void cswap(int& a, int& b) { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }
__global__ void __launch_bounds__(256) sgbm_median_kernel(MedianArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const int16_t* s = a.src + (ptrdiff_t)blockIdx.z * a.spair;
    int v[9];
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++)
            v[(dy + 1) * 3 + dx + 1] = s[(ptrdiff_t)min(max(y + dy, 0), a.H - 1) * a.sstride + min(max(x + dx, 0), a.W - 1)];
    // median of nine by the classic 19-exchange network
    cswap(v[1], v[2]); cswap(v[4], v[5]); cswap(v[7], v[8]); cswap(v[0], v[1]); cswap(v[3], v[4]); cswap(v[6], v[7]);
    cswap(v[1], v[2]); cswap(v[4], v[5]); cswap(v[7], v[8]); cswap(v[0], v[3]); cswap(v[5], v[8]); cswap(v[4], v[7]);
    cswap(v[3], v[6]); cswap(v[1], v[4]); cswap(v[2], v[5]); cswap(v[4], v[7]); cswap(v[4], v[2]); cswap(v[6], v[4]);
    cswap(v[4], v[2]);
    a.dst[(ptrdiff_t)blockIdx.z * a.dpair + (ptrdiff_t)y * a.dstride + x] = (int16_t)v[4];
}

template <class COST>
hipError_t launch_cost(const CostArgs& a, int bs, int n_images, hipStream_t st)
{
    // DD disparities per wave: 16 while the register ring (BS x DD) stays small, 8 for the tall windows
    const int dd = bs <= 5 ? 16 : 8;
    const int outw = 64 - 2 * (bs / 2);
    const int nbands = (a.H + a.rows_per_band - 1) / a.rows_per_band;
    const dim3 grid((a.w1 + outw - 1) / outw, (a.D + 4 * dd - 1) / (4 * dd), nbands * n_images), block(256);
    switch (bs) {
    case 1: hipLaunchKernelGGL((sgbm_cost_kernel<1, COST, 16>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((sgbm_cost_kernel<3, COST, 16>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((sgbm_cost_kernel<5, COST, 16>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL((sgbm_cost_kernel<7, COST, 8>), grid, block, 0, st, a); break;
    case 9: hipLaunchKernelGGL((sgbm_cost_kernel<9, COST, 8>), grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL((sgbm_cost_kernel<11, COST, 8>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

constexpr size_t WINNER_LDS_LIMIT = 150 * 1024;              // what the winner pass may take of a CU's 160 KiB
// The both-views call's own refusals (sgbm_check), and the widths its LDS limit comes to: 16 W + 16 KiB, with the matcher's
// own left-right check 32 W + 16 KiB, within WINNER_LDS_LIMIT.  tests/test_gpu_sgbm_both.py pins their words (the recorded
// fixture tests/matcher_refusals.json pins those of the entries it was recorded from).
constexpr int SGBM_BOTH_MAX_W = 8576, SGBM_BOTH_MAX_W_LRC = 4288;
constexpr const char* MSG_RIGHT_SOURCE = "right_source must be ADF_SGBM_RIGHT_MATCHER or ADF_SGBM_RIGHT_FROM_VOLUME";
constexpr const char* MSG_MAPS_OVERLAP = "the two disparity maps must not overlap";
constexpr const char* MSG_BOTH_WIDTH = "ADF_SGBM_RIGHT_FROM_VOLUME supports images up to %d columns (%d with the matcher's own left-right check, disp12MaxDiff)";

template <int DPL, int DIR>
hipError_t launch_winner(const PathArgs& a, int n, size_t lds_out, hipStream_t st)
{
    if (lds_out > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sgbm_path_kernel<DPL, DIR>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_out);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((sgbm_path_kernel<DPL, DIR>), dim3((a.H + 3) / 4, n), dim3(256), lds_out, st, a);   // from the right + winner
    return hipGetLastError();
}

// lds_out: the winner pass's dynamic LDS (SgbmPlan::lds_out); both: the winner pass also writes the right view's raw map
template <int DPL>
hipError_t launch_paths(const PathArgs& a0, int mode, int n, size_t lds_out, bool both, hipStream_t st)
{
    PathArgs a = a0;
    hipLaunchKernelGGL((sgbm_path_kernel<DPL, DIR_TOP>), dim3((a.w1 + 3) / 4, n), dim3(256), 0, st, a);      // from above
    // the other accumulating paths of the mode (direction of travel): MODE_SGBM_3WAY: from the left; MODE_SGBM: + the two
    // upper diagonals; MODE_HH: + the three from below (stereo_binary_sgbm.cpp:173-186, 286-301)
    static const int add[6][2] = { {1, 0}, {1, 1}, {-1, 1}, {-1, -1}, {0, -1}, {1, -1} };
    const int nadd = mode == ADF_SGBM_MODE_3WAY ? 1 : mode == ADF_SGBM_MODE_SGBM ? 3 : 6;
    for (int k = 0; k < nadd; k++) {
        a.dx = add[k][0]; a.dy = add[k][1];
        const int nlines = a.dy == 0 ? a.H : (a.dx == 0 ? a.w1 : a.w1 + a.H - 1);
        // the last of them writes its own volume (no read-modify-write of S); the winner kernel adds it in
        if (k == nadd - 1) hipLaunchKernelGGL((sgbm_path_kernel<DPL, DIR_ADD_OUT>), dim3((nlines + 3) / 4, n), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((sgbm_path_kernel<DPL, DIR_ADD>), dim3((nlines + 3) / 4, n), dim3(256), 0, st, a);
    }
    if (lds_out > WINNER_LDS_LIMIT) return hipErrorInvalidValue;
    return both ? launch_winner<DPL, DIR_RIGHT_BOTH>(a, n, lds_out, st) : launch_winner<DPL, DIR_RIGHT>(a, n, lds_out, st);
}

} // namespace

// ----------------------------------------------------------------------------------------------
// C-ABI (include/adf_wls.h, "semi-global matcher")
// ----------------------------------------------------------------------------------------------
struct adf_sgbm {
    int device = 0;
    int min_disp = 0, num_disp = 16, block = 3;
    int P1 = 0, P2 = 0, cap = 0, uniq = 0, mode = ADF_SGBM_MODE_SGBM;    // cv::StereoSGBM::create's defaults
    int disp12 = 0;                                                        // ... incl. disp12MaxDiff = 0, which the algorithm reads as 1 (check ON)
    int cost = ADF_SGBM_COST_BT, census_size = 7;                          // adf_sgbm_set_cost (census_size: read by the census costs only)
    DevBuf ws;      // the volumes of the images in flight
    DevBuf stage;   // host-pointer entry: device copies of the I/O
    size_t ws_limit = (size_t)64 << 30;
};

extern "C" int adf_sgbm_create(adf_sgbm_t** out, int min_disparity, int num_disparities, int block_size)
{
    if (!out) return fail(ADF_EBADARG, "out is NULL");
    *out = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(ADF_ENODEV, "no HIP device");
    adf_sgbm* h = new (std::nothrow) adf_sgbm;
    if (!h) return fail(ADF_ENOMEM, "out of host memory");
    h->device = dev; h->min_disp = min_disparity; h->num_disp = num_disparities; h->block = block_size;
    if (const char* e = getenv("ADF_WS_LIMIT_GB")) {
        const double gb = atof(e);
        if (gb > 0) h->ws_limit = (size_t)(gb * (double)((size_t)1 << 30));
    }
    *out = h;
    return ADF_OK;
}

extern "C" void adf_sgbm_destroy(adf_sgbm_t* h)
{
    if (!h) return;
    DeviceScope ds(h->device);
    h->ws.release();
    h->stage.release();
    delete h;
}

extern "C" int adf_sgbm_set_params(adf_sgbm_t* h, int min_disparity, int num_disparities, int block_size, int P1, int P2,
                                   int prefilter_cap, int uniqueness_ratio, int mode)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    h->min_disp = min_disparity; h->num_disp = num_disparities; h->block = block_size;
    h->P1 = P1; h->P2 = P2; h->cap = prefilter_cap; h->uniq = uniqueness_ratio; h->mode = mode;
    return ADF_OK;
}

extern "C" int adf_sgbm_get_params(const adf_sgbm_t* h, int* min_disparity, int* num_disparities, int* block_size, int* P1, int* P2,
                                   int* prefilter_cap, int* uniqueness_ratio, int* mode)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (min_disparity) *min_disparity = h->min_disp;
    if (num_disparities) *num_disparities = h->num_disp;
    if (block_size) *block_size = h->block;
    if (P1) *P1 = h->P1;
    if (P2) *P2 = h->P2;
    if (prefilter_cap) *prefilter_cap = h->cap;
    if (uniqueness_ratio) *uniqueness_ratio = h->uniq;
    if (mode) *mode = h->mode;
    return ADF_OK;
}

extern "C" int adf_sgbm_set_disp12_max_diff(adf_sgbm_t* h, int v)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    h->disp12 = v;
    return ADF_OK;
}

extern "C" int adf_sgbm_get_disp12_max_diff(const adf_sgbm_t* h, int* v)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (v) *v = h->disp12;
    return ADF_OK;
}

extern "C" int adf_sgbm_set_cost(adf_sgbm_t* h, int cost_type, int census_size)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    return census_cost_set(h->cost, h->census_size, ADF_SGBM_COST_BT, cost_type, census_size);
}

extern "C" int adf_sgbm_get_cost(const adf_sgbm_t* h, int* cost_type, int* census_size)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (cost_type) *cost_type = h->cost;
    if (census_size) *census_size = h->census_size;
    return ADF_OK;
}

extern "C" int adf_sgbm_get_device(const adf_sgbm_t* h, int* device)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (device) *device = h->device;
    return ADF_OK;
}

// One compute call as its entry received it: planes with rows `stride`, pairs `pair` bytes apart; device: device pointers
// that the kernels index (the host entry's are copied by bytes into a dense staging block).
// A both-views call (adf_sgbm_compute_both_*) carries the right view's map too, disp_r, and names its source.
template <class T> struct Plane { T* p; ptrdiff_t stride, pair; };
struct SgbmCall {
    adf_sgbm* h; int n_pairs; Plane<const uint8_t> left, right; int cn, W, H; Plane<int16_t> disp; bool device;
    bool both = false; Plane<int16_t> disp_r = {nullptr, 0, 0}; int right_source = ADF_SGBM_RIGHT_MATCHER;
    bool from_volume() const { return both && right_source == ADF_SGBM_RIGHT_FROM_VOLUME; }
};

static int sgbm_block(const adf_sgbm* h) { return h->block > 0 ? h->block : 5; }
// slots of a wave's ring of live right columns (ADF_SGBM_RIGHT_FROM_VOLUME): a power of two that holds D
static int sgbm_ring(int D) { int r = 16; while (r < D) r <<= 1; return r; }
constexpr int SGBM_RING_MAX = 512;                           // = sgbm_ring(the largest numDisparities)
// dynamic LDS of the winner pass: per wave a row of `cols` results and, with the matcher's own left-right check, two rows of
// the image's width; a call that takes the right view's map from the volume adds a row of the image's width and `ring` slots of 8 bytes
static size_t sgbm_winner_lds(const adf_sgbm* h, int cols, int W, int ring = 0)
{
    return ((size_t)cols + (h->disp12 < 100000 ? 2 * (size_t)W : 0) + (ring ? (size_t)W : 0)) * 4 * sizeof(int16_t) + (size_t)ring * 4 * 8;
}

// bytes [lo, hi) that n maps of H rows of W int16 touch
static void map_extent(const Plane<int16_t>& m, int n, int W, int H, uintptr_t& lo, uintptr_t& hi)
{
    const ptrdiff_t span = (ptrdiff_t)(n - 1) * m.pair;
    lo = reinterpret_cast<uintptr_t>(m.p) + std::min<ptrdiff_t>(span, 0);
    hi = reinterpret_cast<uintptr_t>(m.p) + std::max<ptrdiff_t>(span, 0) + (ptrdiff_t)(H - 1) * m.stride + (ptrdiff_t)W * 2;
}

static int sgbm_check(const SgbmCall& c)
{
    const adf_sgbm* h = c.h;
    const int cn = c.cn, W = c.W, H = c.H;
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (c.n_pairs <= 0 || !c.left.p || !c.right.p || !c.disp.p) return fail(ADF_EBADARG, "views and disparity must be non-NULL, n_pairs positive");
    if (cn != 1 && cn != 3) return fail(ADF_EBADARG, "views must be CV_8UC1 or CV_8UC3");
    if (h->cost != ADF_SGBM_COST_BT && cn != 1) return fail(ADF_EBADARG, "a census cost takes CV_8UC1 views (descriptor.cpp:58)");
    if (W <= 0 || H <= 0 || c.left.stride < (ptrdiff_t)W * cn || c.right.stride < (ptrdiff_t)W * cn || c.disp.stride < (ptrdiff_t)W * 2)
        return fail(ADF_ESIZE, "bad size or stride");
    if ((c.disp.stride & 1) || (reinterpret_cast<uintptr_t>(c.disp.p) & 1)) return fail(ADF_ESIZE, "disparity rows must be 2-byte aligned");
    if (h->mode != ADF_SGBM_MODE_3WAY && h->mode != ADF_SGBM_MODE_SGBM && h->mode != ADF_SGBM_MODE_HH)
        return fail(ADF_EBADARG, "mode must be StereoSGBM::MODE_SGBM, MODE_HH or MODE_SGBM_3WAY");
    if (h->num_disp <= 0 || h->num_disp % 16) return fail(ADF_EBADARG, "numDisparities must be positive and divisible by 16");
    if (h->num_disp > 512) return fail(ADF_EBADARG, "numDisparities above 512 is not supported");
    if (sgbm_block(h) % 2 == 0 || sgbm_block(h) > 11) return fail(ADF_EBADARG, "blockSize must be odd and at most 11");
    if (h->min_disp < -2047 || h->min_disp + h->num_disp > 2047) return fail(ADF_EBADARG, "disparity range does not fit CV_16S with 4 fractional bits");
    if (h->P1 < 0 || h->P2 < 0 || h->P1 > 8000 || h->P2 > 16000) return fail(ADF_EBADARG, "P1 / P2 out of range");
    // (whatever the disparity range leaves of a row: the limit is stated for the whole width)
    if (h->disp12 < 100000 && sgbm_winner_lds(h, W, W) > WINNER_LDS_LIMIT)
        return fail(ADF_ESIZE, "the matcher's own left-right check (disp12MaxDiff) supports images up to 6400 columns");
    if (c.device && c.n_pairs > 1 && (c.disp.pair & 1)) return fail(ADF_ESIZE, "disparity maps must be 2-byte aligned");
    if (!c.both) return ADF_OK;
    if (c.right_source != ADF_SGBM_RIGHT_MATCHER && c.right_source != ADF_SGBM_RIGHT_FROM_VOLUME)
        return fail(ADF_EBADARG, "%s", MSG_RIGHT_SOURCE);
    if (!c.disp_r.p) return fail(ADF_EBADARG, "views and disparity must be non-NULL, n_pairs positive");
    if (c.disp_r.stride < (ptrdiff_t)W * 2) return fail(ADF_ESIZE, "bad size or stride");
    if ((c.disp_r.stride & 1) || (reinterpret_cast<uintptr_t>(c.disp_r.p) & 1)) return fail(ADF_ESIZE, "disparity rows must be 2-byte aligned");
    if (c.device && c.n_pairs > 1 && (c.disp_r.pair & 1)) return fail(ADF_ESIZE, "disparity maps must be 2-byte aligned");
    uintptr_t l0, l1, r0, r1;
    map_extent(c.disp, c.n_pairs, W, H, l0, l1);
    map_extent(c.disp_r, c.n_pairs, W, H, r0, r1);
    if (l0 < r1 && r0 < l1) return fail(ADF_EBADARG, "%s", MSG_MAPS_OVERLAP);
    // (as above: stated for the whole width, and for the largest ring)
    if (c.from_volume() && sgbm_winner_lds(h, W, W, SGBM_RING_MAX) > WINNER_LDS_LIMIT)
        return fail(ADF_ESIZE, MSG_BOTH_WIDTH, SGBM_BOTH_MAX_W, SGBM_BOTH_MAX_W_LRC);
    return ADF_OK;
}

// What a checked call runs with: a pure function of the handle's settings and the call's sizes.
struct SgbmPlan {
    int D, minD, bs, P1, P2, ur, ftzero, minX1, w1; int16_t invalid; bool census;   // the effective parameters; matched columns [minX1, minX1 + w1)
    // per image in flight, 256-byte aligned: a signal plane (12 * cn bytes per pixel; census: a descriptor plane, 8), a cost volume, the raw map
    // (raw2_bytes: the right view's raw map of ADF_SGBM_RIGHT_FROM_VOLUME, else 0)
    size_t rec_bytes, vol_bytes, raw_bytes, raw2_bytes;
    int chunk;                                  // images in flight: what ws_limit holds of the call's pairs
    size_t rec1, rec2, C, S, L, raw, raw2, ws_bytes;  // h->ws: byte offsets of its regions, `chunk` parts each (L: the last accumulating path's own volume)
    int dpl; size_t lds_out;                    // disparities per lane of the path kernels; the winner pass's dynamic LDS
    int ring; int16_t invalid_r;                // ADF_SGBM_RIGHT_FROM_VOLUME: the ring's slots (else 0) and the right map's invalid value
};

static SgbmPlan sgbm_plan(const SgbmCall& c)
{
    const adf_sgbm* h = c.h;
    const size_t px = (size_t)c.W * c.H;
    SgbmPlan p;
    p.D = h->num_disp; p.minD = h->min_disp; p.bs = sgbm_block(h);
    p.P1 = h->P1 > 0 ? h->P1 : 2; p.P2 = std::max(h->P2 > 0 ? h->P2 : 5, p.P1 + 1);
    p.ur = h->uniq >= 0 ? h->uniq : 10; p.ftzero = std::max(h->cap, 15) | 1;
    p.minX1 = std::max(p.minD + p.D, 0); p.w1 = (c.W + std::min(p.minD, 0)) - p.minX1;
    p.invalid = (int16_t)((p.minD - 1) * SG_DISP_SCALE);
    p.census = h->cost != ADF_SGBM_COST_BT;
    p.rec_bytes = pad_to(px * (p.census ? 8 : c.cn * 3 * 4), 256);
    p.vol_bytes = pad_to(p.w1 > 0 ? (size_t)c.H * p.w1 * p.D * 2 : 0, 256);
    p.raw_bytes = pad_to(px * 2, 256);
    p.raw2_bytes = c.from_volume() ? p.raw_bytes : 0;
    p.chunk = (int)std::min<size_t>(std::max<size_t>(h->ws_limit / (2 * p.rec_bytes + 3 * p.vol_bytes + p.raw_bytes + p.raw2_bytes), 1), c.n_pairs);
    p.ws_bytes = 0;
    auto region = [&](size_t part) { const size_t at = p.ws_bytes; p.ws_bytes += part * p.chunk; return at; };
    p.rec1 = region(p.rec_bytes); p.rec2 = region(p.rec_bytes); p.C = region(p.vol_bytes); p.S = region(p.vol_bytes);
    p.L = region(p.vol_bytes); p.raw = region(p.raw_bytes); p.raw2 = region(p.raw2_bytes);
    p.dpl = p.D <= 64 ? 1 : p.D <= 128 ? 2 : p.D <= 256 ? 4 : 8;
    p.ring = c.from_volume() ? sgbm_ring(p.D) : 0;
    p.invalid_r = (int16_t)(-(p.minD + p.D) * SG_DISP_SCALE);
    p.lds_out = sgbm_winner_lds(h, p.w1, c.W, p.ring);
    return p;
}

// Images [first, first + n) of a checked call on device pointers, n <= p.chunk, through the workspace's regions.
static int sgbm_run_chunk(const SgbmCall& c, const SgbmPlan& p, int first, int n, hipStream_t st)
{
    const adf_sgbm* h = c.h;
    const int W = c.W, H = c.H;
    char* ws = (char*)h->ws.p;
    uint32_t* rec1 = (uint32_t*)(ws + p.rec1); uint32_t* rec2 = (uint32_t*)(ws + p.rec2); int16_t* raw = (int16_t*)(ws + p.raw);
    const size_t rec_pair = p.rec_bytes / 4, volp = p.vol_bytes / 2, raw_el = p.raw_bytes / 2;   // dwords, int16 elements
    const uint8_t* L = c.left.p + (ptrdiff_t)first * c.left.pair;
    const uint8_t* R = c.right.p + (ptrdiff_t)first * c.right.pair;
    int16_t* out = (int16_t*)((char*)c.disp.p + (ptrdiff_t)first * c.disp.pair);
    const dim3 per_row((W + 255) / 256, H, n);
    int16_t* raw2 = (int16_t*)(ws + p.raw2);                  // (the right view's raw map: ADF_SGBM_RIGHT_FROM_VOLUME only)
    FillArgs fa{raw, W, (ptrdiff_t)raw_el, W, H, p.invalid};
    hipLaunchKernelGGL(sgbm_fill_kernel, per_row, dim3(256), 0, st, fa);
    if (p.ring) {
        fa.p = raw2; fa.v = p.invalid_r;
        hipLaunchKernelGGL(sgbm_fill_kernel, per_row, dim3(256), 0, st, fa);
    }
    if (p.w1 > 0) {
        if (p.census) {                                    // preFilterCap plays no part in this cost
            int rc;
            if ((rc = census_run(n, L, c.left.stride, c.left.pair, W, H, h->cost, h->census_size, (uint64_t*)rec1, (ptrdiff_t)W * 8, (ptrdiff_t)p.rec_bytes, st))) return rc;
            if ((rc = census_run(n, R, c.right.stride, c.right.pair, W, H, h->cost, h->census_size, (uint64_t*)rec2, (ptrdiff_t)W * 8, (ptrdiff_t)p.rec_bytes, st))) return rc;
        } else {
            SignalArgs sa{L, c.left.stride, c.left.pair, c.cn, W, H, p.ftzero, rec1, rec_pair};
            hipLaunchKernelGGL(sgbm_signals_kernel, per_row, dim3(256), 0, st, sa);
            sa.img = R; sa.stride = c.right.stride; sa.pair_stride = c.right.pair; sa.rec = rec2;
            hipLaunchKernelGGL(sgbm_signals_kernel, per_row, dim3(256), 0, st, sa);
        }
        // bands: the bs-1 warm-up rows are paid per band; enough workgroups to fill the chip when the chunk's images are small
        int rpb = 128;
        while (rpb > 16 && (size_t)((H + rpb - 1) / rpb) * ((p.w1 + 61) / 62) * ((p.D + 63) / 64) * n < 2048) rpb >>= 1;
        CostArgs ca{rec1, rec2, rec_pair, (int16_t*)(ws + p.C), volp, W, H, p.D, p.minD, p.minX1, p.w1, rpb};
        if ((size_t)((H + rpb - 1) / rpb) * n > 65535) return fail(ADF_ESIZE, "too many images per call for the cost kernel's grid");
        hipError_t e = p.census ? launch_cost<CensusCost>(ca, p.bs, n, st)
                     : c.cn == 1 ? launch_cost<BtCost<1>>(ca, p.bs, n, st) : launch_cost<BtCost<3>>(ca, p.bs, n, st);
        if (e != hipSuccess) return fail(ADF_EHIP, "%s", hipGetErrorString(e));
        PathArgs pa{ca.C, (int16_t*)(ws + p.S), (int16_t*)(ws + p.L), volp, W, H, p.D, p.minD, p.minX1, p.w1, p.P1, p.P2, p.ur,
                    raw, (ptrdiff_t)W, (ptrdiff_t)raw_el, 0, 0, h->disp12, raw2, (ptrdiff_t)W, (ptrdiff_t)raw_el, p.ring};
        const bool both = p.ring != 0;
        e = p.dpl == 1 ? launch_paths<1>(pa, h->mode, n, p.lds_out, both, st) : p.dpl == 2 ? launch_paths<2>(pa, h->mode, n, p.lds_out, both, st)
          : p.dpl == 4 ? launch_paths<4>(pa, h->mode, n, p.lds_out, both, st) : launch_paths<8>(pa, h->mode, n, p.lds_out, both, st);
        if (e != hipSuccess) return fail(ADF_EHIP, "%s", hipGetErrorString(e));
    }
    MedianArgs ma{raw, (ptrdiff_t)W, (ptrdiff_t)raw_el, out, c.disp.stride / 2, c.disp.pair / 2, W, H};
    hipLaunchKernelGGL(sgbm_median_kernel, per_row, dim3(256), 0, st, ma);
    if (p.ring) {
        int16_t* out_r = (int16_t*)((char*)c.disp_r.p + (ptrdiff_t)first * c.disp_r.pair);
        MedianArgs mr{raw2, (ptrdiff_t)W, (ptrdiff_t)raw_el, out_r, c.disp_r.stride / 2, c.disp_r.pair / 2, W, H};
        hipLaunchKernelGGL(sgbm_median_kernel, per_row, dim3(256), 0, st, mr);
    }
    return ADF_OK;
}

// A checked call on device pointers: the workspace, then chunk after chunk.
static int sgbm_run(const SgbmCall& c, const SgbmPlan& p, hipStream_t st)
{
    DeviceScope ds(c.h->device);
    if (int rc = c.h->ws.reserve(p.ws_bytes, st, FILL_NONE)) return rc;
    for (int first = 0; first < c.n_pairs; first += p.chunk)
        if (int rc = sgbm_run_chunk(c, p, first, std::min(p.chunk, c.n_pairs - first), st)) return rc;
    return launched();
}

// The handle as createRightMatcher's matcher (disparity_filters.cpp:432-445) for the length of a scope: minDisparity
// 1 - minDisparity - numDisparities, uniqueness test and left-right check off; P1, P2, mode, cap and cost are the handle's.
struct RightMatcherScope {
    adf_sgbm* h; int md, uniq, disp12;
    explicit RightMatcherScope(adf_sgbm* h_) : h(h_), md(h_->min_disp), uniq(h_->uniq), disp12(h_->disp12)
    {
        h->min_disp = 1 - md - h->num_disp; h->uniq = 0; h->disp12 = 1000000;
    }
    ~RightMatcherScope() { h->min_disp = md; h->uniq = uniq; h->disp12 = disp12; }
    RightMatcherScope(const RightMatcherScope&) = delete;
    RightMatcherScope& operator=(const RightMatcherScope&) = delete;
};

// ADF_SGBM_RIGHT_MATCHER: the right matcher's call of a both-views call -- views swapped, the map is disp_r
static SgbmCall sgbm_right_call(const SgbmCall& c)
{
    return SgbmCall{c.h, c.n_pairs, c.right, c.left, c.cn, c.W, c.H, c.disp_r, c.device};
}

// A both-views call on device pointers, checked here: one run that writes both maps (ADF_SGBM_RIGHT_FROM_VOLUME), or the
// left matcher's run and then the right matcher's through the same workspace (ADF_SGBM_RIGHT_MATCHER).
static int sgbm_run_both(const SgbmCall& c, hipStream_t st)
{
    if (int rc = sgbm_check(c)) return rc;
    if (c.from_volume()) return sgbm_run(c, sgbm_plan(c), st);
    const SgbmCall r = sgbm_right_call(c);
    {
        RightMatcherScope as_right(c.h);
        if (int rc = sgbm_check(r)) return rc;               // (nothing is launched unless both calls can run)
    }
    SgbmCall l = c;
    l.both = false;
    if (int rc = sgbm_run(l, sgbm_plan(l), st)) return rc;
    RightMatcherScope as_right(c.h);
    return sgbm_run(r, sgbm_plan(r), st);
}

extern "C" int adf_sgbm_compute_device(adf_sgbm_t* h, int n_pairs,
                                       const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                       const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                       int channels, int W, int H,
                                       int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                                       void* stream)
{
    const SgbmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, channels, W, H,
                     {disparity, disp_stride, disp_pair_stride}, true};
    if (int rc = sgbm_check(c)) return rc;
    return sgbm_run(c, sgbm_plan(c), (hipStream_t)stream);
}

// The host entry: views in, map out through one staging block of the handle, in which the same call runs on dense copies.
extern "C" int adf_sgbm_compute_host(adf_sgbm_t* h, int n_pairs,
                                     const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                     const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                     int channels, int W, int H,
                                     int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride)
{
    const SgbmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, channels, W, H,
                     {disparity, disp_stride, disp_pair_stride}, false};
    int rc = sgbm_check(c);
    if (rc) return rc;
    DeviceScope ds(h->device);
    const ptrdiff_t vrow = (ptrdiff_t)W * channels, vbytes = vrow * H, drow = (ptrdiff_t)W * 2, dbytes = drow * H;
    if ((rc = h->stage.reserve((size_t)(2 * vbytes + dbytes) * n_pairs + 512, nullptr, FILL_NONE))) return rc;
    uint8_t* dl = (uint8_t*)h->stage.p;
    uint8_t* dr = dl + vbytes * n_pairs;
    int16_t* dd = (int16_t*)pad_to((uintptr_t)(dr + vbytes * n_pairs), 256);
    const SgbmCall d{h, n_pairs, {dl, vrow, vbytes}, {dr, vrow, vbytes}, channels, W, H, {dd, drow, dbytes}, true};   // the call, staged
    if ((rc = copy_images(dl, vrow, vbytes, left, left_stride, left_pair_stride, vrow, H, n_pairs, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = copy_images(dr, vrow, vbytes, right, right_stride, right_pair_stride, vrow, H, n_pairs, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = sgbm_run(d, sgbm_plan(d), nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(disparity, disp_stride, disp_pair_stride, dd, drow, dbytes, drow, H, n_pairs, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

extern "C" int adf_sgbm_compute_both_device(adf_sgbm_t* h, int n_pairs,
                                            const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                            const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                            int channels, int W, int H,
                                            int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                            int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                            int right_source, void* stream)
{
    const SgbmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, channels, W, H,
                     {disp_left, disp_left_stride, disp_left_pair_stride}, true,
                     true, {disp_right, disp_right_stride, disp_right_pair_stride}, right_source};
    return sgbm_run_both(c, (hipStream_t)stream);
}

// As adf_sgbm_compute_host: the same call on dense copies in the handle's staging block, which holds both maps here.
extern "C" int adf_sgbm_compute_both_host(adf_sgbm_t* h, int n_pairs,
                                          const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                          const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                          int channels, int W, int H,
                                          int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                          int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                          int right_source)
{
    const SgbmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, channels, W, H,
                     {disp_left, disp_left_stride, disp_left_pair_stride}, false,
                     true, {disp_right, disp_right_stride, disp_right_pair_stride}, right_source};
    int rc = sgbm_check(c);
    if (rc) return rc;
    DeviceScope ds(h->device);
    const ptrdiff_t vrow = (ptrdiff_t)W * channels, vbytes = vrow * H, drow = (ptrdiff_t)W * 2, dbytes = pad_to((size_t)drow * H, 256);
    if ((rc = h->stage.reserve((size_t)(2 * vbytes + 2 * dbytes) * n_pairs + 512, nullptr, FILL_NONE))) return rc;
    uint8_t* dl = (uint8_t*)h->stage.p;
    uint8_t* dr = dl + vbytes * n_pairs;
    int16_t* ddl = (int16_t*)pad_to((uintptr_t)(dr + vbytes * n_pairs), 256);
    int16_t* ddr = (int16_t*)((char*)ddl + dbytes * n_pairs);
    const SgbmCall d{h, n_pairs, {dl, vrow, vbytes}, {dr, vrow, vbytes}, channels, W, H, {ddl, drow, dbytes}, true,
                     true, {ddr, drow, dbytes}, right_source};                                                        // the call, staged
    if ((rc = copy_images(dl, vrow, vbytes, left, left_stride, left_pair_stride, vrow, H, n_pairs, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = copy_images(dr, vrow, vbytes, right, right_stride, right_pair_stride, vrow, H, n_pairs, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = sgbm_run_both(d, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(disp_left, disp_left_stride, disp_left_pair_stride, ddl, drow, dbytes, drow, H, n_pairs, hipMemcpyDeviceToHost, nullptr))) return rc;
    if ((rc = copy_images(disp_right, disp_right_stride, disp_right_pair_stride, ddr, drow, dbytes, drow, H, n_pairs, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
