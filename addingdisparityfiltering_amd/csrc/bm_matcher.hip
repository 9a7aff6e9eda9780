// bm_matcher.hip -- block matcher on the device, so a stereo pair can go from views to filtered disparity
// without leaving HBM.
//
// The reference's filter is fed by cv::StereoBM / cv::StereoSGBM (disparity_filters.cpp:386-449, sample
// disparity_filtering.cpp:151,214), which live in OpenCV's calib3d module and are NOT in the reference tree:
// PARITY UNPINNED at that boundary.  This file implements the published StereoBM algorithm exactly as
// oracle/adf_oracle_bm.c states it (x-Sobel prefilter, SAD block matching, ties to the largest disparity,
// texture / uniqueness tests, sub-pixel fit, 4 fractional bits), bit for bit -- it is integer work -- and keeps
// the conventions the reference does fix: the parameters of the right-view matcher (:421-431) and the
// settings the filter factory forces on the matcher (:389-390, 399-400).
//
// Layout.  The prefiltered views are stored "row-group interleaved": dword (g, x) holds the four
// vertically adjacent pixels (x, 4g .. 4g+3) of column x, one byte each, as value+1 (so no byte is 0); PG
// groups of replicated rows pad the top and the bottom.  One v_sad_u8 / v_msad_u8 then adds four rows of one
// column of the SAD window, and a lane reads its four adjacent columns of a group as one 16-byte load.
//
// Kernel.  One wave = 256 adjacent columns, four per lane (128, two per lane, in the instantiation with the
// uniqueness test; the outer W2 on each side are window halo) x one group of four output rows; the four waves of a workgroup take four consecutive row groups.  Per disparity
// and column a lane forms the four vertical window sums (groups fully inside all four windows are summed
// once, the partial ones through v_msad_u8 with the rows outside the window zeroed in the left operand), two
// disparities are packed in one register (low / high half; a window sum is below 2^16, and the prefix
// arithmetic is exact modulo 2^32), a local prefix plus one DPP wave scan of the lane totals gives the prefix
// over the tile's columns, the neighbours' prefix vectors come through a per-wave LDS slot, and the winner is
// tracked a pair of disparities at a time: the winner pair and the pairs before / after it are captured as whole
// registers (for the uniqueness test also the smallest pair minimum two or more pairs away), and which half won
// is decided once at the end.  Nothing but the int16 result is written -- and, for a caller that passes a cost plane
// (adf_bm_compute_cost_*), the aggregated cost of the winning integer disparity beside it, truncated to 16 bits; 0 where the
// map holds the filtered value.  The plane pointer is uniform over the launch: the existing entry points pass null and pay
// one scalar test per output row.
// The kernel is bound by integer VALU issue (about 11 instructions per pixel and disparity; EXPERIMENTS.md section 10), not
// by HBM: the views are read through L1/L2 once per disparity, HBM sees them once.
//
// Census cost (adf_bm_set_cost).  The pixel cost is a policy of the match kernel.  With
// ADF_BM_COST_CENSUS_* / _MCT_* the prefiltered views are replaced by the census descriptors (census.h) of the raw views, split into
// P = ceil(bits / 8) byte planes in the same row-group interleaved layout (plane p holds bits 8p .. 8p+7, no +1 bias),
// and the vertical sum of four rows of a column is popcount((L ^ R) & window_mask), added up over the groups and over
// the planes.  A one-plane descriptor keeps its left columns in registers as SAD does; wider ones reload them per plane
// (an L1/L2 hit).  Prefix, scan, LDS exchange, winner tracking and epilogue do not know which cost they serve.
#include "census.h"

#include <new>

using namespace adf;

namespace {

constexpr int PG = 3;        // padding groups above and below (half windows up to 10 rows)
constexpr unsigned INF = 0x7fffffffu;

struct PrefilterArgs {
    const uint8_t* src; ptrdiff_t stride, pair_stride;
    uint32_t* dst; size_t dst_pair;   // dwords per view
    int W, Wp, H, HGP, cap;
};

// x-Sobel, clipped to [-cap, cap] and offset by cap (oracle: adf_oracle_bm_prefilter_xsobel); stored +1.
__global__ void __launch_bounds__(256) bm_prefilter_kernel(PrefilterArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, gp = blockIdx.y;
    if (x >= a.W) return;
    const uint8_t* src = a.src + (ptrdiff_t)blockIdx.z * a.pair_stride;
    uint32_t out = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int y = min(max(4 * (gp - PG) + b, 0), a.H - 1);
        int v = a.cap;
        if (x > 0 && x < a.W - 1) {
            const uint8_t* r0 = src + (ptrdiff_t)(y > 0 ? y - 1 : (a.H > 1 ? 1 : 0)) * a.stride;
            const uint8_t* r1 = src + (ptrdiff_t)y * a.stride;
            const uint8_t* r2 = src + (ptrdiff_t)(y < a.H - 1 ? y + 1 : (a.H > 1 ? a.H - 2 : 0)) * a.stride;
            const int s = ((int)r0[x + 1] - (int)r0[x - 1]) + 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r2[x + 1] - (int)r2[x - 1]);
            v = min(max(s, -a.cap), a.cap) + a.cap;
        }
        out |= (uint32_t)(v + 1) << (8 * b);
    }
    a.dst[(size_t)blockIdx.z * a.dst_pair + (size_t)gp * a.Wp + x] = out;
}

struct CensusPackArgs {
    const uint8_t* src[2]; ptrdiff_t stride[2], pair_stride[2];   // left, right
    uint32_t* dst; size_t dst_view, dst_pair, dst_plane;          // dwords between the two views, the pairs, the planes
    int W, Wp, H, HGP;
};

// The census descriptors of both views (blockIdx.z = 2 * pair + view) as byte planes in the matcher's layout, straight
// from the raw views.  The descriptor lives in census.h: its shape S, the tile (four row groups) plus halo through LDS with
// clamped coordinates and the comparison loop are the ones census_kernel runs, so the bits are adf_census_transform's.  This
// kernel's own: a wave takes a row group, a lane forms the descriptors of its four rows and stores one dword per byte plane.
// Going through adf::census_run instead would write 8 bytes per pixel and read them back to keep 1..6.
// The padding groups hold the descriptors of the edge-replicated image; no window of a matched row reaches them.
template <class S>
__global__ void __launch_bounds__(CENSUS_THREADS) bm_census_pack_kernel(CensusPackArgs a)
{
    constexpr int GROUPS = CENSUS_TILE_H / 4;                  // row groups of a tile: one per wave
    static_assert(GROUPS * 64 == CENSUS_THREADS);
    __shared__ uint8_t tile[S::LH][S::LW];
    __shared__ uint16_t sums[S::SH][S::SW];                    // the mean rule's column sums; not referenced by the other rules
    const int view = blockIdx.z & 1;
    const unsigned pz = blockIdx.z >> 1;
    const int x0 = blockIdx.x * CENSUS_TILE_W, gp0 = blockIdx.y * GROUPS, y0 = 4 * (gp0 - PG);
    census_tile_load<S>(tile, sums, a.src[view] + (ptrdiff_t)pz * a.pair_stride[view], a.stride[view], x0, y0, a.W, a.H);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 + lane, gp = gp0 + wv;
    if (x >= a.W || gp >= a.HGP) return;
    uint32_t out[S::PLANES];
#pragma unroll
    for (int p = 0; p < S::PLANES; p++) out[p] = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        uint32_t hi, lo;
        census_compare<S>(tile, sums, 4 * wv + b, lane, hi, lo);
#pragma unroll
        for (int p = 0; p < S::PLANES; p++) out[p] |= (((p < 4 ? lo >> (8 * p) : hi >> (8 * (p - 4)))) & 0xFFu) << (8 * b);
    }
    uint32_t* dst = a.dst + (size_t)view * a.dst_view + (size_t)pz * a.dst_pair + (size_t)gp * a.Wp + x;
#pragma unroll
    for (int p = 0; p < S::PLANES; p++) dst[(size_t)p * a.dst_plane] = out[p];
}

// One view's search: its prefiltered "left" (reference) and "right" (searched) images, output and disparity range.
struct ViewArgs {
    const uint32_t* Lt; const uint32_t* Rt;                  // prefiltered views (census: descriptor planes), t_pair dwords per image
    int16_t* disp; ptrdiff_t dstride, dpair;                 // bytes
    int16_t* cost; ptrdiff_t cstride, cpair;                 // the winner's cost, CV_16S like calib3d's cost map; null: not wanted
    int mindisp;
    int xs, xe;            // matched columns [xs, xe)
    int texthr, uniq;
};
// A launch matches one view per image pair (nviews = 1: StereoMatcher::compute) or both views of every pair
// (nviews = 2: the left matcher and the right matcher of disparity_filters.cpp:417-431 in one grid, blockIdx.z =
// 2 * pair + view; the two views' searches are the same size, so one grid covers both).
struct MatchArgs {
    ViewArgs v[2];
    int nviews;
    size_t t_pair;
    int W, Wp, H, HG;                                        // Wp: dwords per prefiltered row (W + XPAD, multiple of 4)
    int ndisp, cap;
    int planes; size_t plane;                                // census: byte planes of a descriptor, dwords per plane
};

// The pixel cost of the match kernel: what one dword of four rows of the reference column (L) and of the searched
// column (R) adds to a vertical window sum -- all four rows (`full`) or the rows under a byte mask (`part`).
struct CostSad {
    static constexpr bool CENSUS = false, MULTI = false;
    static __device__ __forceinline__ uint32_t full(uint32_t R, uint32_t L, uint32_t acc) { return __builtin_amdgcn_sad_u8(R, L, acc); }
    // rows with a zero reference byte are skipped (the prefiltered views are stored +1)
    static __device__ __forceinline__ uint32_t part(uint32_t R, uint32_t L, uint32_t m, uint32_t acc) { return __builtin_amdgcn_msad_u8(R, L & m, acc); }
};
// Hamming distance of four 8-bit descriptor slices: one v_xor (fused with the mask), one v_bcnt_u32_b32 that accumulates.
// MULTI: a descriptor of several byte planes, their number read at run time; a one-plane descriptor (dense 3, sparse 5)
// has its own instantiation, because the plane loop costs it a third of its time.
template <bool MULTI_>
struct CostCensus {
    static constexpr bool CENSUS = true, MULTI = MULTI_;
    static __device__ __forceinline__ uint32_t full(uint32_t R, uint32_t L, uint32_t acc) { return (uint32_t)__builtin_popcount(R ^ L) + acc; }
    static __device__ __forceinline__ uint32_t part(uint32_t R, uint32_t L, uint32_t m, uint32_t acc) { return (uint32_t)__builtin_popcount((R ^ L) & m) + acc; }
};

// rows of group gi (relative to the output group) that lie in the window of output row r
constexpr uint32_t window_mask(int W2, int GB, int gi, int r)
{
    uint32_t m = 0;
    for (int b = 0; b < 4; b++) {
        const int rel = 4 * (gi - GB) + b - r;
        if (rel >= -W2 && rel <= W2) m |= 0xFFu << (8 * b);
    }
    return m;
}
constexpr bool group_common(int W2, int GB, int gi)
{
    for (int r = 0; r < 4; r++) if (window_mask(W2, GB, gi, r) != 0xFFFFFFFFu) return false;
    return true;
}

template <int CTRL, int ROWMASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v)
{
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xF, BOUND);
}
// inclusive prefix sum over the 64 lanes of the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v)
{
    v = dpp_add<0x111, 0xF, true>(v);   // row_shr:1
    v = dpp_add<0x112, 0xF, true>(v);   // row_shr:2
    v = dpp_add<0x114, 0xF, true>(v);   // row_shr:4
    v = dpp_add<0x118, 0xF, true>(v);   // row_shr:8
    v = dpp_add<0x142, 0xA, false>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xC, false>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

// adjacent columns per lane: four on the filter's path; two with the uniqueness test, whose four extra state
// registers per pixel would otherwise push the kernel past 256 registers (measured per 4K pair: 3.3 ms with four
// columns, 1.98 ms with two); two also with a census cost of several planes at window half-sizes 9 and 10, whose
// accumulators across the planes are live through the vertical sums: with four columns those two instantiations need
// 298 registers
constexpr int cpl_of(bool uniq, bool multi, int w2) { return (uniq || (multi && w2 >= 9)) ? 2 : 4; }
constexpr int XPAD = 64 * 4 + 4;       // columns of padding right of a prefiltered row (lanes past the image read it)
constexpr int floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

template <int W2, bool UNIQ, class COST>
__global__ void __launch_bounds__(256) bm_match_kernel(MatchArgs a)
{
    constexpr int CPL = cpl_of(UNIQ, COST::MULTI, W2);
    constexpr int TILE = 64 * CPL;          // columns per wave, window halo included
    constexpr int TOUT = TILE - 2 * W2;
    constexpr int GB = (W2 + 3) / 4;        // groups above the output group that the windows reach
    constexpr int NG = 2 * GB + 1;
    static_assert(GB <= PG, "padding too small for this window");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: row bases and the LDS slot stay scalar
    const int g = blockIdx.y * 4 + wave;
    if (g >= a.HG) return;                                           // whole wave; no barrier below
    const int vi = a.nviews == 2 ? (int)(blockIdx.z & 1) : 0;
    const unsigned pz = a.nviews == 2 ? blockIdx.z >> 1 : blockIdx.z;
    const ViewArgs& va = a.v[vi];
    const int xs = va.xs, xe = va.xe, mindisp = va.mindisp, texthr = va.texthr, uniq = va.uniq;
    if (xs + (int)blockIdx.x * TOUT >= xe) return;                  // tile past this view's matched columns
    const int c = xs + (int)blockIdx.x * TOUT - W2 + lane * CPL;     // this lane's first column (>= 0)
    const int Wp = a.Wp;
    const size_t voff = (size_t)pz * a.t_pair + (size_t)(g - GB + PG) * Wp;
    const uint32_t* __restrict__ Lt = va.Lt + voff;
    const uint32_t* __restrict__ Rt = va.Rt + voff;

    // one dword-aligned vector load of CPL adjacent columns; the byte offset is formed in 32 bits so that the load
    // takes the scalar row base plus a 32-bit vector offset
    auto load4 = [&](const uint32_t* row, unsigned x, uint32_t (&d)[CPL]) {   // x .. x+CPL-1 are inside the padded row
        struct __attribute__((aligned(4))) Vec { uint32_t v[CPL]; };
        const Vec q = *reinterpret_cast<const Vec*>(reinterpret_cast<const char*>(row) + x * 4u);
#pragma unroll
        for (int j = 0; j < CPL; j++) d[j] = q.v[j];
    };
    const int cl = min(c, Wp - CPL);
    uint32_t Ld[NG][CPL];
#pragma unroll
    for (int gi = 0; gi < NG; gi++) load4(Lt + (size_t)gi * Wp, cl, Ld[gi]);

    // four vertical window sums (one per output row of the group) of the pixel cost down column j of this lane
    auto vertical = [&](const uint32_t (&Rd)[NG][CPL], int j, uint32_t (&V)[4]) {
        uint32_t F = 0;
#pragma unroll
        for (int gi = 0; gi < NG; gi++)
            if (group_common(W2, GB, gi)) F = COST::full(Rd[gi][j], Ld[gi][j], F);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t acc = F;
#pragma unroll
            for (int gi = 0; gi < NG; gi++) {
                const uint32_t m = window_mask(W2, GB, gi, r);
                if (group_common(W2, GB, gi) || m == 0) continue;
                if (m == 0xFFFFFFFFu) acc = COST::full(Rd[gi][j], Ld[gi][j], acc);
                else acc = COST::part(Rd[gi][j], Ld[gi][j], m, acc);
            }
            V[r] = acc;
        }
    };
    // horizontal window sums of the lane's CPL per-column values: the prefix over the tile's columns is a local
    // prefix plus the wave scan of the lane totals; the window sum of column t is Q(t+W2) - Q(t-W2-1), both held
    // by a neighbouring lane in a register known at compile time.  The neighbours' prefixes travel through a
    // per-wave LDS slot as whole vectors (one ds_write_b128, one ds_read_b128 per lane offset): ds_bpermute_b32
    // costs the LDS pipe about 6 cycles per wave and dword, three times the vector path.
    struct __attribute__((aligned(16))) Vec { uint32_t v[CPL]; };
    __shared__ Vec xch[4][4][65];                            // [wave][output row][lane]; entry 64 stays zero = Q(-1)
    constexpr int LH0 = floordiv(W2, CPL), LH1 = floordiv(CPL - 1 + W2, CPL);          // lanes holding Q(t+W2)
    constexpr int LL0 = floordiv(-W2 - 1, CPL), LL1 = floordiv(CPL - 2 - W2, CPL);     // lanes holding Q(t-W2-1)
    const int iH0 = min(lane + LH0, 63), iH1 = min(lane + LH1, 63);
    const int iL0 = lane + LL0 < 0 ? 64 : lane + LL0, iL1 = lane + LL1 < 0 ? 64 : lane + LL1;   // a lane left of the tile: all its columns are
    if (lane < 4) {
        Vec z;
#pragma unroll
        for (int j = 0; j < CPL; j++) z.v[j] = 0;
        xch[wave][lane][64] = z;
    }
    auto horizontal = [&](uint32_t (&v)[CPL], int r) {
        uint32_t tot = v[0];
#pragma unroll
        for (int j = 1; j < CPL; j++) tot += v[j];
        Vec q;                                                // inclusive prefix: the scan result is the last column's
        q.v[CPL - 1] = wave_scan(tot);
#pragma unroll
        for (int j = CPL - 2; j >= 0; j--) q.v[j] = q.v[j + 1] - v[j + 1];
        Vec* slot = xch[wave][r];
        slot[lane] = q;
        __builtin_amdgcn_wave_barrier();                      // same wave: the LDS queue is in order
        const Vec hA = slot[iH0], hB = (LH1 != LH0) ? slot[iH1] : hA;
        const Vec lA = slot[iL0], lB = (LL1 != LL0) ? slot[iL1] : lA;
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            const int th = j + W2, tl = j - W2 - 1;                       // column offsets relative to the lane's first
            const int lh = floordiv(th, CPL), jh = th - lh * CPL, ll = floordiv(tl, CPL), jl = tl - ll * CPL;
            const uint32_t qh = (lh == LH0) ? hA.v[jh] : hB.v[jh];
            const uint32_t ql = (ll == LL0) ? lA.v[jl] : lB.v[jl];
            v[j] = qh - ql;
        }
    };

    // texture of the window: sum of |L - cap| (only needed with a texture threshold; a census cost has no prefiltered
    // image whose texture could be summed, and the host passes it a threshold of 0)
    uint32_t tex[4][CPL];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int j = 0; j < CPL; j++) tex[r][j] = INF;
    if (!COST::CENSUS && texthr > 0) {
        uint32_t Rd[NG][CPL], V[CPL][4];
        const uint32_t ft = (uint32_t)(a.cap + 1) * 0x01010101u;
#pragma unroll
        for (int gi = 0; gi < NG; gi++)
#pragma unroll
            for (int j = 0; j < CPL; j++) Rd[gi][j] = ft;
#pragma unroll
        for (int j = 0; j < CPL; j++) vertical(Rd, j, V[j]);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t h[CPL];
#pragma unroll
            for (int j = 0; j < CPL; j++) h[j] = V[j][r];
            horizontal(h, r);
#pragma unroll
            for (int j = 0; j < CPL; j++) tex[r][j] = h[j];
        }
    }

    // Winner tracking, a pair of disparities (k, k+1 = low / high half of one register) at a time.  A pair is
    // compared through its smaller half, and when it beats the winner the pair itself (capW), the pair before it
    // (pAt) and -- one step later -- the pair after it (nAt) are kept as whole registers.  Which half won (the
    // high one on a tie: ties go to the larger disparity) and which halves are the neighbours of the sub-pixel fit
    // is decided once, at the end:
    //   winner in the low half  (even k): below = high half of the previous pair, above = high half of capW
    //   winner in the high half (odd k):  below = low half of capW,              above = low half of the next pair
    // `after`: the previous pair became the winner (the previous step's compare result, kept in scalar registers).
    // Uniqueness test (UNIQ): the smallest cost at least two disparities away from the winner = the smallest pair
    // minimum at least two PAIRS before (lmin: the prefix minimum delayed by two steps, taken when the winner
    // changes) or after it (rmin: restarted when the winner changes, fed from the second pair after it on), plus
    // the halves of the two neighbouring pairs that are not adjacent to the winner -- read from pAt / nAt at the end.
    uint32_t best[4][CPL], bk1[4][CPL], capW[4][CPL], pAt[4][CPL], nAt[4][CPL], prev[4][CPL];
    uint32_t lmin[4][CPL], rmin[4][CPL], pm1[4][CPL], pm2[4][CPL];
    bool after[4][CPL];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            best[r][j] = INF; bk1[r][j] = 1u; capW[r][j] = 0; pAt[r][j] = 0; nAt[r][j] = 0; prev[r][j] = 0;
            lmin[r][j] = INF; rmin[r][j] = INF; pm1[r][j] = INF; pm2[r][j] = INF;
            after[r][j] = false;
        }
    auto track_pair = [&](int r, int j, uint32_t k, uint32_t Pk) {
        const uint32_t m = min(Pk & 0xFFFFu, Pk >> 16);
        const bool upd = m <= best[r][j];
        best[r][j] = min(best[r][j], m);
        if (UNIQ) {
            if (!upd && !after[r][j]) rmin[r][j] = min(rmin[r][j], m);
            if (upd) { lmin[r][j] = pm2[r][j]; rmin[r][j] = INF; }
            pm2[r][j] = pm1[r][j]; pm1[r][j] = min(pm1[r][j], m);
        }
        if (after[r][j]) nAt[r][j] = Pk;
        if (upd) { capW[r][j] = Pk; pAt[r][j] = prev[r][j]; bk1[r][j] = k + 1u; }
        after[r][j] = upd;
        prev[r][j] = Pk;
    };

    const int xbase = c - mindisp;                           // R column of disparity index 0; xbase - k >= 0 for matched columns
    auto rcol = [&](int k) -> unsigned { return (unsigned)min(max(xbase - k, 0), Wp - CPL); };
    // The columns of disparities k, k+1 of plane p (SAD: the one prefiltered image); a descriptor of several planes also
    // reloads the lane's own columns of that plane -- an L1/L2 hit -- since all planes of L do not fit the registers.
    const int planes = COST::MULTI ? a.planes : 1;
    uint32_t R0[NG][CPL], R1[NG][CPL];
    auto fetch = [&](int k, int p) {
        const size_t po = COST::MULTI ? (size_t)p * a.plane : 0;
        const unsigned x0 = rcol(k), x1 = rcol(k + 1);
#pragma unroll
        for (int gi = 0; gi < NG; gi++) { load4(Rt + po + (size_t)gi * (unsigned)Wp, x0, R0[gi]); load4(Rt + po + (size_t)gi * (unsigned)Wp, x1, R1[gi]); }
        if (planes > 1) {
#pragma unroll
            for (int gi = 0; gi < NG; gi++) load4(Lt + po + (size_t)gi * (unsigned)Wp, cl, Ld[gi]);
        }
    };
    fetch(0, 0);
    // One loop over (pair of disparities, plane): a plane adds its vertical sums to P, the last plane of a pair reduces it.
    uint32_t P[4][CPL];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int j = 0; j < CPL; j++) P[r][j] = 0;
    for (int k = 0, p = 0; k < a.ndisp;) {
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            uint32_t V0[4], V1[4];
            vertical(R0, j, V0);
            vertical(R1, j, V1);
#pragma unroll
            for (int r = 0; r < 4; r++) P[r][j] += V0[r] + (V1[r] << 16);   // exact: both halves stay below 2^16
        }
        // the next plane's, or the next two disparities', columns are fetched while this pair is reduced (the last fetch is unused)
        const bool last = p + 1 == planes;
        fetch(last ? k + 2 : k, last ? 0 : p + 1);
        if (!last) { p++; continue; }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            horizontal(P[r], r);
#pragma unroll
            for (int j = 0; j < CPL; j++) { track_pair(r, j, (uint32_t)k, P[r][j]); P[r][j] = 0; }
        }
        k += 2; p = 0;
    }

    const int16_t filtered = (int16_t)((mindisp - 1) * 16);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int y = 4 * g + r;
        if (y >= a.H) continue;
        int16_t* drow = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(va.disp) + (ptrdiff_t)pz * va.dpair + (ptrdiff_t)y * va.dstride);
        int16_t* crow = va.cost ? reinterpret_cast<int16_t*>(reinterpret_cast<char*>(va.cost) + (ptrdiff_t)pz * va.cpair + (ptrdiff_t)y * va.cstride) : nullptr;
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            const int t = lane * CPL + j;
            if (t < W2 || t >= TILE - W2 || c + j >= xe) continue;
            const int kw = (int)bk1[r][j] - 1;                            // first disparity of the winner pair
            const int sb = (int)best[r][j];
            const uint32_t wl = capW[r][j] & 0xFFFFu, wh = capW[r][j] >> 16;
            const uint32_t bl = pAt[r][j] & 0xFFFFu, bh = pAt[r][j] >> 16;  // the pair before (if kw > 0)
            const uint32_t al = nAt[r][j] & 0xFFFFu, ah = nAt[r][j] >> 16;  // the pair after (if kw + 2 < ndisp)
            const bool odd = wh <= wl;
            const int kb = kw + (odd ? 1 : 0);
            const uint32_t below = odd ? wl : bh, above = odd ? al : wh;
            const int pv = (int)(kb > 0 ? below : above);
            const int nv = (int)(kb < a.ndisp - 1 ? above : below);
            const int dd = pv + nv - 2 * sb + abs(pv - nv);
            int16_t out = (int16_t)(((kb + mindisp) * 256 + (dd != 0 ? (pv - nv) * 256 / dd : 0) + 15) >> 4);
            if ((int)tex[r][j] < texthr) out = filtered;
            if (y < W2 || y >= a.H - W2) out = filtered;                 // rows without a full window (calib3d's valid rectangle)
            if (UNIQ && uniq > 0) {                                       // (a view of the launch may have the test off)
                const int thresh = sb + sb * uniq / 100;
                uint32_t other = min(lmin[r][j], rmin[r][j]);
                if (kw > 0) other = min(other, odd ? min(bl, bh) : bl);                // kb-1 is adjacent, kb-2 and kb-3 are not
                if (kw + 2 < a.ndisp) other = min(other, odd ? ah : min(al, ah));      // kb+1 is adjacent, kb+2 and kb+3 are not
                if ((int)other <= thresh) out = filtered;
            }
            drow[c + j] = out;
            if (crow) crow[c + j] = out != filtered ? (int16_t)sb : (int16_t)0;   // sb: the cost at kb, before the sub-pixel fit
        }
    }
}

// columns without a full search range or window: (minDisparity - 1) * 16, and 0 in the cost plane
__global__ void __launch_bounds__(256) bm_border_kernel(MatchArgs a)
{
    const int y = blockIdx.y;
    const int vi = a.nviews == 2 ? (int)(blockIdx.z & 1) : 0;
    const unsigned pz = a.nviews == 2 ? blockIdx.z >> 1 : blockIdx.z;
    const ViewArgs& va = a.v[vi];
    const int nleft = max(min(va.xs, a.W), 0), xr = (va.xe > va.xs) ? max(va.xe, nleft) : nleft;
    const int n = nleft + (a.W - xr);
    const int16_t filtered = (int16_t)((va.mindisp - 1) * 16);
    int16_t* row = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(va.disp) + (ptrdiff_t)pz * va.dpair + (ptrdiff_t)y * va.dstride);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) row[i < nleft ? i : xr + (i - nleft)] = filtered;
    if (!va.cost) return;
    int16_t* crow = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(va.cost) + (ptrdiff_t)pz * va.cpair + (ptrdiff_t)y * va.cstride);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) crow[i < nleft ? i : xr + (i - nleft)] = 0;
}

template <bool UNIQ, class COST>
hipError_t launch_match(const MatchArgs& a, int w2, dim3 block, int n, hipStream_t st)
{
    const int tout = 64 * cpl_of(UNIQ, COST::MULTI, w2) - 2 * w2;
    int cols = a.v[0].xe - a.v[0].xs;
    if (a.nviews == 2 && a.v[1].xe - a.v[1].xs > cols) cols = a.v[1].xe - a.v[1].xs;
    dim3 grid((cols + tout - 1) / tout, (a.HG + 3) / 4, n * a.nviews);
    switch (w2) {
#define ADF_BM_CASE(K) case K: hipLaunchKernelGGL((bm_match_kernel<K, UNIQ, COST>), grid, block, 0, st, a); break;
    ADF_BM_CASE(2) ADF_BM_CASE(3) ADF_BM_CASE(4) ADF_BM_CASE(5) ADF_BM_CASE(6)
    ADF_BM_CASE(7) ADF_BM_CASE(8) ADF_BM_CASE(9) ADF_BM_CASE(10)
#undef ADF_BM_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The kernel of a call: the cost policy first (SAD; census with its one plane resident or with the plane loop), then UNIQ.
hipError_t launch_match_for(const MatchArgs& a, bool census, bool uniq, int w2, int n, hipStream_t st)
{
    auto with = [&](auto cost) {
        return uniq ? launch_match<true, decltype(cost)>(a, w2, dim3(256), n, st) : launch_match<false, decltype(cost)>(a, w2, dim3(256), n, st);
    };
    return !census ? with(CostSad{}) : a.planes > 1 ? with(CostCensus<true>{}) : with(CostCensus<false>{});
}

} // namespace

// ----------------------------------------------------------------------------------------------
// C-ABI (include/adf_wls.h, "block matcher")
// ----------------------------------------------------------------------------------------------
struct adf_bm {
    int device = 0;
    int min_disp = 0, num_disp = 0, block = 21;
    int cap = 31, texthr = 10, uniq = 15;       // cv::StereoBM's defaults
    int cost = ADF_BM_COST_SAD, census_size = 7;   // adf_bm_set_cost (census_size: read by the census costs only)
    DevBuf views;   // prefiltered left + right views of the batch, or their census descriptor planes
    DevBuf stage;   // host-pointer entry: device copies of the I/O
};

extern "C" int adf_bm_create(adf_bm_t** out, int num_disparities, int block_size)
{
    if (!out) return fail(ADF_EBADARG, "out is NULL");
    *out = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(ADF_ENODEV, "no HIP device");
    adf_bm* h = new (std::nothrow) adf_bm;
    if (!h) return fail(ADF_ENOMEM, "out of host memory");
    h->device = dev; h->num_disp = num_disparities; h->block = block_size;
    *out = h;
    return ADF_OK;
}

extern "C" void adf_bm_destroy(adf_bm_t* h)
{
    if (!h) return;
    DeviceScope ds(h->device);
    h->views.release();
    h->stage.release();
    delete h;
}

extern "C" int adf_bm_set_params(adf_bm_t* h, int min_disparity, int num_disparities, int block_size,
                                 int prefilter_cap, int texture_threshold, int uniqueness_ratio)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    h->min_disp = min_disparity; h->num_disp = num_disparities; h->block = block_size;
    h->cap = prefilter_cap; h->texthr = texture_threshold; h->uniq = uniqueness_ratio;
    return ADF_OK;
}

extern "C" int adf_bm_set_cost(adf_bm_t* h, int cost_type, int census_size)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    return census_cost_set(h->cost, h->census_size, ADF_BM_COST_SAD, cost_type, census_size);
}

extern "C" int adf_bm_get_cost(const adf_bm_t* h, int* cost_type, int* census_size)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (cost_type) *cost_type = h->cost;
    if (census_size) *census_size = h->census_size;
    return ADF_OK;
}

extern "C" int adf_bm_get_device(const adf_bm_t* h, int* device)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (device) *device = h->device;
    return ADF_OK;
}

extern "C" int adf_bm_get_params(const adf_bm_t* h, int* min_disparity, int* num_disparities, int* block_size,
                                 int* prefilter_cap, int* texture_threshold, int* uniqueness_ratio)
{
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (min_disparity) *min_disparity = h->min_disp;
    if (num_disparities) *num_disparities = h->num_disp;
    if (block_size) *block_size = h->block;
    if (prefilter_cap) *prefilter_cap = h->cap;
    if (texture_threshold) *texture_threshold = h->texthr;
    if (uniqueness_ratio) *uniqueness_ratio = h->uniq;
    return ADF_OK;
}

// One compute call as its entry received it: planes with rows `stride`, pairs `pair` bytes apart.  disp / cost [0]: the
// left view's, [1]: the right view's (nviews == 2: a both-views entry); with_cost: a cost entry, which takes the cost
// plane of every view it matches.  device: device pointers that the kernels index (a host entry's are copied by bytes).
template <class T> struct Plane { T* p; ptrdiff_t stride, pair; };
struct BmCall {
    adf_bm* h; int n_pairs; Plane<const uint8_t> left, right; int W, H;
    int nviews; bool with_cost; Plane<int16_t> disp[2], cost[2]; bool device;
};

// a CV_16S plane that does not start every row (with `pairs`: and every pair) on an even address
static bool odd(const Plane<int16_t>& m, bool pairs) { return (m.stride & 1) || (reinterpret_cast<uintptr_t>(m.p) & 1) || (pairs && (m.pair & 1)); }

// The rules of every compute call, then those of maps that a kernel indexes and of the right view's map.
static int bm_check(const BmCall& c)
{
    const adf_bm* h = c.h;
    const int W = c.W, H = c.H;
    const Plane<int16_t>& d = c.disp[0];
    if (!h) return fail(ADF_EBADARG, "handle is NULL");
    if (c.n_pairs <= 0 || !c.left.p || !c.right.p || !d.p) return fail(ADF_EBADARG, "views and disparity must be non-NULL, n_pairs positive");
    if (W <= 0 || H <= 0 || c.left.stride < W || c.right.stride < W || d.stride < (ptrdiff_t)W * 2) return fail(ADF_ESIZE, "bad size or stride");
    if (odd(d, false)) return fail(ADF_ESIZE, "disparity rows must be 2-byte aligned");
    // the checks cv::StereoBM::compute makes on its parameters; the window is limited to 21 so that a
    // window sum fits 16 bits
    if (h->num_disp <= 0 || h->num_disp % 16) return fail(ADF_EBADARG, "numDisparities must be positive and divisible by 16");
    if (h->block < 5 || h->block > 21 || h->block % 2 == 0) return fail(ADF_EBADARG, "blockSize must be odd and within 5..21");
    if (h->block >= (W < H ? W : H)) return fail(ADF_EBADARG, "blockSize must be smaller than the image");
    if (h->cap < 1 || h->cap > 63) return fail(ADF_EBADARG, "preFilterCap must be within 1..63");
    if (h->texthr < 0 || h->uniq < 0) return fail(ADF_EBADARG, "textureThreshold and uniquenessRatio must be non-negative");
    if (h->min_disp < -32768 || h->min_disp + h->num_disp > 2047) return fail(ADF_EBADARG, "disparity range does not fit CV_16S with 4 fractional bits");
    if (c.device && odd(d, c.n_pairs > 1)) return fail(ADF_ESIZE, "disparity maps must be 2-byte aligned");
    if (c.nviews == 2 && (c.disp[1].stride < (ptrdiff_t)W * 2 || odd(c.disp[1], c.n_pairs > 1)))
        return fail(ADF_ESIZE, "bad stride or alignment of the right disparity map");
    return ADF_OK;
}

// The planes that a both-views or a cost entry adds to compute's.  A function of its own because the entries differ in
// WHEN they report them: the device entries before bm_check, adf_bm_compute_cost_host after it (tests/matcher_refusals.json).
static int bm_check_added(const BmCall& c)
{
    if (c.nviews == 2 && !c.disp[1].p) return fail(ADF_EBADARG, "disp_right is NULL");
    static const char* const names[2][2] = {{"the", ""}, {"the left", "the right"}};
    for (int v = 0; c.with_cost && v < c.nviews; v++) {
        const Plane<int16_t>& k = c.cost[v];
        const char* which = names[c.nviews - 1][v];
        if (!k.p) return fail(ADF_EBADARG, "%s cost plane is NULL", which);
        if (k.stride < (ptrdiff_t)c.W * 2) return fail(ADF_ESIZE, "%s cost plane: row stride smaller than a row", which);
        if (odd(k, c.n_pairs > 1)) return fail(ADF_ESIZE, "%s cost plane must be 2-byte aligned", which);
    }
    return ADF_OK;
}

// The geometry of a checked call: a pure function of the handle's settings and the call's sizes.
struct BmSearch { int mindisp, xs, xe, texthr, uniq; };   // matched columns [xs, xe)
struct BmPlan {
    int HG, HGP, Wp;             // row groups of the image, with the padding groups; dwords per padded row (lanes past the image read, and discard, it)
    bool census; int planes, w2;
    size_t plane, image;         // dwords per prefiltered view or descriptor plane / per image: sized from the handle's cost of THIS call
    size_t views_bytes;          // h->views: the left images of the batch, then the right ones
    BmSearch v[2];               // the left view's search, and the right view's in the left image
};

static BmPlan bm_plan(const BmCall& c)
{
    const adf_bm* h = c.h;
    BmPlan p;
    p.HG = (c.H + 3) / 4; p.HGP = p.HG + 2 * PG; p.Wp = (c.W + XPAD + 3) / 4 * 4;
    p.census = h->cost != ADF_BM_COST_SAD; p.planes = p.census ? census_planes(h->cost, h->census_size) : 1; p.w2 = h->block / 2;
    p.plane = (size_t)p.HGP * p.Wp; p.image = p.plane * (size_t)p.planes;
    p.views_bytes = 2 * p.image * (size_t)c.n_pairs * sizeof(uint32_t);
    auto search = [&](int md, int texthr, int uniq) {
        const int maxd = md + h->num_disp - 1;
        return BmSearch{md, (maxd > 0 ? maxd : 0) + p.w2, c.W - (md < 0 ? -md : 0) - p.w2, texthr, uniq};
    };
    // (a census cost has no prefiltered image to sum a texture of: textureThreshold is validated and not used)
    p.v[0] = search(h->min_disp, p.census ? 0 : h->texthr, h->uniq);
    // the right-view matcher of createRightMatcher (disparity_filters.cpp:421-431): views swapped,
    // minDisparity = -(min_disp + num_disp) + 1, texture and uniqueness tests off
    p.v[1] = search(-(h->min_disp + h->num_disp) + 1, 0, 0);
    return p;
}

// A checked call on device pointers: prefilter both images once (census: form their descriptor planes), then one launch
// for the left view alone or for both views; each view with or without its cost plane.
static int bm_run(const BmCall& c, const BmPlan& p, hipStream_t st)
{
    adf_bm* h = c.h;
    const int W = c.W, H = c.H, n = c.n_pairs;
    DeviceScope ds(h->device);
    if (int rc = h->views.reserve(p.views_bytes, st, FILL_NONE)) return rc;
    uint32_t* const T[2] = {(uint32_t*)h->views.p, (uint32_t*)h->views.p + p.image * (size_t)n};

    if (p.census) {
        CensusPackArgs a;
        a.src[0] = c.left.p; a.stride[0] = c.left.stride; a.pair_stride[0] = c.left.pair;
        a.src[1] = c.right.p; a.stride[1] = c.right.stride; a.pair_stride[1] = c.right.pair;
        a.dst = T[0]; a.dst_view = p.image * (size_t)n; a.dst_pair = p.image; a.dst_plane = p.plane;
        a.W = W; a.Wp = p.Wp; a.H = H; a.HGP = p.HGP;
        const dim3 grid((W + CENSUS_TILE_W - 1) / CENSUS_TILE_W, (p.HGP * 4 + CENSUS_TILE_H - 1) / CENSUS_TILE_H, 2 * n);
        // (adf_bm_set_cost keeps every pair that census_dispatch does not list out of the handle)
        census_dispatch(h->cost, h->census_size, [&](auto s) { hipLaunchKernelGGL((bm_census_pack_kernel<decltype(s)>), grid, dim3(CENSUS_THREADS), 0, st, a); });
    } else {
        PrefilterArgs a;
        a.W = W; a.Wp = p.Wp; a.H = H; a.HGP = p.HGP; a.cap = h->cap; a.dst_pair = p.plane;
        const dim3 grid((W + 255) / 256, p.HGP, n);
        a.src = c.left.p; a.stride = c.left.stride; a.pair_stride = c.left.pair; a.dst = T[0];
        hipLaunchKernelGGL(bm_prefilter_kernel, grid, dim3(256), 0, st, a);
        a.src = c.right.p; a.stride = c.right.stride; a.pair_stride = c.right.pair; a.dst = T[1];
        hipLaunchKernelGGL(bm_prefilter_kernel, grid, dim3(256), 0, st, a);
    }

    MatchArgs a;
    a.nviews = c.nviews; a.t_pair = p.image; a.planes = p.planes; a.plane = p.plane;
    a.W = W; a.Wp = p.Wp; a.H = H; a.HG = p.HG; a.ndisp = h->num_disp; a.cap = h->cap;
    for (int i = 0; i < 2; i++) {
        const int v = i < c.nviews ? i : 0;                    // (one view: the second slot repeats the first)
        const BmSearch& s = p.v[v];
        ViewArgs& va = a.v[i];
        va.Lt = T[v]; va.Rt = T[1 - v];                        // reference and searched image
        va.disp = c.disp[v].p; va.dstride = c.disp[v].stride; va.dpair = c.disp[v].pair;
        va.cost = c.cost[v].p; va.cstride = c.cost[v].stride; va.cpair = c.cost[v].pair;
        va.mindisp = s.mindisp; va.xs = s.xs; va.xe = s.xe; va.texthr = s.texthr; va.uniq = s.uniq;
    }
    hipLaunchKernelGGL(bm_border_kernel, dim3(4, H, n * c.nviews), dim3(256), 0, st, a);
    if (a.v[0].xe > a.v[0].xs || (c.nviews == 2 && a.v[1].xe > a.v[1].xs)) {
        hipError_t e = launch_match_for(a, p.census, h->uniq > 0, p.w2, n, st);
        if (e != hipSuccess) return fail(ADF_EHIP, "%s", hipGetErrorString(e));
    }
    return launched();
}

// A checked call on host pointers: views in, map (and cost plane, when wanted) out through one staging block of the
// handle, in which the same call runs on dense copies.
static int bm_run_host(const BmCall& c, const BmPlan& p)
{
    adf_bm* h = c.h;
    const int n = c.n_pairs;
    DeviceScope ds(h->device);
    const ptrdiff_t vrow = c.W, vbytes = vrow * c.H, drow = vrow * 2, dbytes = drow * c.H;
    int rc = h->stage.reserve((size_t)(2 * vbytes + (c.with_cost ? 2 : 1) * dbytes) * n, nullptr, FILL_NONE);
    if (rc) return rc;
    uint8_t* dl = (uint8_t*)h->stage.p;
    uint8_t* dr = dl + vbytes * n;
    int16_t* dd = (int16_t*)(dr + vbytes * n);
    int16_t* dc = dd + (size_t)c.W * c.H * n;                         // (used with a cost plane only)
    BmCall d = c;                                                     // the call on its staged copies
    d.device = true;
    d.left = {dl, vrow, vbytes}; d.right = {dr, vrow, vbytes}; d.disp[0] = {dd, drow, dbytes};
    if (c.with_cost) d.cost[0] = {dc, drow, dbytes};
    if ((rc = copy_images(dl, vrow, vbytes, c.left.p, c.left.stride, c.left.pair, vrow, c.H, n, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = copy_images(dr, vrow, vbytes, c.right.p, c.right.stride, c.right.pair, vrow, c.H, n, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = bm_run(d, p, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(c.disp[0].p, c.disp[0].stride, c.disp[0].pair, dd, drow, dbytes, drow, c.H, n, hipMemcpyDeviceToHost, nullptr))) return rc;
    if (c.with_cost && (rc = copy_images(c.cost[0].p, c.cost[0].stride, c.cost[0].pair, dc, drow, dbytes, drow, c.H, n, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

// Every compute entry: its record through the checks, the plan and the run.  A device entry reports an added plane's
// fault before the call's, adf_bm_compute_cost_host after it (tests/matcher_refusals.json).
static int bm_compute(const BmCall& c, void* stream)
{
    if (int rc = c.device ? bm_check_added(c) : bm_check(c)) return rc;
    if (int rc = c.device ? bm_check(c) : bm_check_added(c)) return rc;
    return c.device ? bm_run(c, bm_plan(c), (hipStream_t)stream) : bm_run_host(c, bm_plan(c));
}

extern "C" int adf_bm_compute_device(adf_bm_t* h, int n_pairs,
                                     const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                     const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                     int W, int H,
                                     int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                                     void* stream)
{
    const BmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, W, H, 1, false,
                   {{disparity, disp_stride, disp_pair_stride}, {}}, {}, true};
    return bm_compute(c, stream);
}

extern "C" int adf_bm_compute_cost_device(adf_bm_t* h, int n_pairs,
                                          const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                          const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                          int W, int H,
                                          int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                                          int16_t* cost, ptrdiff_t cost_stride, ptrdiff_t cost_pair_stride,
                                          void* stream)
{
    const BmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, W, H, 1, true,
                   {{disparity, disp_stride, disp_pair_stride}, {}}, {{cost, cost_stride, cost_pair_stride}, {}}, true};
    return bm_compute(c, stream);
}

extern "C" int adf_bm_compute_both_device(adf_bm_t* h, int n_pairs,
                                          const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                          const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                          int W, int H,
                                          int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                          int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                          void* stream)
{
    const BmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, W, H, 2, false,
                   {{disp_left, disp_left_stride, disp_left_pair_stride}, {disp_right, disp_right_stride, disp_right_pair_stride}}, {}, true};
    return bm_compute(c, stream);
}

extern "C" int adf_bm_compute_both_cost_device(adf_bm_t* h, int n_pairs,
                                               const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                               const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                               int W, int H,
                                               int16_t* disp_left, ptrdiff_t disp_left_stride, ptrdiff_t disp_left_pair_stride,
                                               int16_t* disp_right, ptrdiff_t disp_right_stride, ptrdiff_t disp_right_pair_stride,
                                               int16_t* cost_left, ptrdiff_t cost_left_stride, ptrdiff_t cost_left_pair_stride,
                                               int16_t* cost_right, ptrdiff_t cost_right_stride, ptrdiff_t cost_right_pair_stride,
                                               void* stream)
{
    const BmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, W, H, 2, true,
                   {{disp_left, disp_left_stride, disp_left_pair_stride}, {disp_right, disp_right_stride, disp_right_pair_stride}},
                   {{cost_left, cost_left_stride, cost_left_pair_stride}, {cost_right, cost_right_stride, cost_right_pair_stride}}, true};
    return bm_compute(c, stream);
}

extern "C" int adf_bm_compute_host(adf_bm_t* h, int n_pairs,
                                   const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                   const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                   int W, int H,
                                   int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride)
{
    const BmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, W, H, 1, false,
                   {{disparity, disp_stride, disp_pair_stride}, {}}, {}, false};
    return bm_compute(c, nullptr);
}

extern "C" int adf_bm_compute_cost_host(adf_bm_t* h, int n_pairs,
                                        const uint8_t* left, ptrdiff_t left_stride, ptrdiff_t left_pair_stride,
                                        const uint8_t* right, ptrdiff_t right_stride, ptrdiff_t right_pair_stride,
                                        int W, int H,
                                        int16_t* disparity, ptrdiff_t disp_stride, ptrdiff_t disp_pair_stride,
                                        int16_t* cost, ptrdiff_t cost_stride, ptrdiff_t cost_pair_stride)
{
    const BmCall c{h, n_pairs, {left, left_stride, left_pair_stride}, {right, right_stride, right_pair_stride}, W, H, 1, true,
                   {{disparity, disp_stride, disp_pair_stride}, {}}, {{cost, cost_stride, cost_pair_stride}, {}}, false};
    return bm_compute(c, nullptr);
}
