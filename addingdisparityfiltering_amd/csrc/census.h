// census.h -- the census descriptor, stated once for the transform (census_kernels.hip), the block matcher's pack kernel
// (bm_matcher.hip) and the semi-global matcher's cost (sgbm_matcher.hip): its compile-time facts (CensusShape: sampling
// grid and comparison rule), the one list of the (type, size) pairs that exist (census_dispatch), the LDS tile load and
// the comparison loop, the shared host rules.
#pragma once

#include "adf_host.h"

namespace adf {

// the block matcher's setter hands its cost type to census_check, which names the semi-global matcher's constants
static_assert(ADF_BM_COST_CENSUS_DENSE == ADF_SGBM_COST_CENSUS_DENSE && ADF_BM_COST_CENSUS_SPARSE == ADF_SGBM_COST_CENSUS_SPARSE);
static_assert(ADF_BM_COST_MCT_DENSE == ADF_SGBM_COST_MCT_DENSE && ADF_BM_COST_MCT_SPARSE == ADF_SGBM_COST_MCT_SPARSE &&
              ADF_BM_COST_CENSUS_CS == ADF_SGBM_COST_CENSUS_CS);
constexpr int CENSUS_TILE_W = 64, CENSUS_TILE_H = 16, CENSUS_THREADS = 256;   // pixels and threads of a workgroup: a wave per row, four rows per sweep
// relied on by CensusCost::MAX_PIXEL (two disparities per register at every block size) and by the block matcher (window sums below 2^16)
constexpr int CENSUS_MAX_BITS = 48, CENSUS_MAX_PLANES = 6;

// What a neighbour is compared with.  CENTRE: the centre pixel (Zabih & Woodfill 1994).  MEAN: the mean of the whole
// K x K window, centre included, as K * K * neighbour > window sum (the modified census transform, Froeba & Ernst 2004).
// MIRROR: the neighbour's mirror image through the centre (the centre-symmetric census, Spangenberg et al. 2013).
enum CensusRule { CENSUS_CENTRE, CENSUS_MEAN, CENSUS_MIRROR };

// The descriptor at odd window size K.  Dense: every offset of the K x K window but the centre (descriptor.cpp:65-69).
// Sparse: every second offset, -K/2, -K/2 + 2, ... (descriptor.cpp:70-74); the offset (0, 0) is skipped where the grid
// passes through it.  CENSUS_MIRROR (dense only): the offsets before (0, 0) in raster order, each standing for a pair.
// PLANES: the bytes that hold the bits.  LW x LH: the workgroup's tile with its halo.  SW x SH: the column sums of the
// CENSUS_MEAN rule (census_tile_load), nothing for the other rules.
template <bool SPARSE, int K, CensusRule RULE_ = CENSUS_CENTRE>
struct CensusShape {
    static constexpr CensusRule RULE = RULE_;
    static_assert(!(SPARSE && RULE == CENSUS_MIRROR));
    static constexpr int N2 = K / 2, STEP = SPARSE ? 2 : 1, SIZE = K;
    static constexpr int PER_AXIS = 2 * N2 / STEP + 1, GRID_BITS = PER_AXIS * PER_AXIS - (N2 % STEP == 0 ? 1 : 0);
    static constexpr int NBITS = RULE == CENSUS_MIRROR ? GRID_BITS / 2 : GRID_BITS;
    static constexpr int PLANES = (NBITS + 7) / 8;
    static constexpr int LW = CENSUS_TILE_W + 2 * N2, LH = CENSUS_TILE_H + 2 * N2;
    static constexpr int SW = RULE == CENSUS_MEAN ? LW : 1, SH = RULE == CENSUS_MEAN ? CENSUS_TILE_H : 1;
};
template <bool SPARSE, int K, int BITS, int PLANES, CensusRule RULE = CENSUS_CENTRE, class S = CensusShape<SPARSE, K, RULE>>
constexpr bool census_shape_is = S::NBITS == BITS && S::PLANES == PLANES && BITS <= CENSUS_MAX_BITS && PLANES <= CENSUS_MAX_PLANES;
static_assert(census_shape_is<false, 3, 8, 1> && census_shape_is<false, 5, 24, 3> && census_shape_is<false, 7, 48, 6>);
static_assert(census_shape_is<true, 5, 8, 1> && census_shape_is<true, 7, 16, 2> && census_shape_is<true, 9, 24, 3> && census_shape_is<true, 11, 36, 5>);
static_assert(census_shape_is<false, 7, 48, 6, CENSUS_MEAN> && census_shape_is<true, 11, 36, 5, CENSUS_MEAN>);   // the rule changes no count
static_assert(census_shape_is<false, 3, 4, 1, CENSUS_MIRROR> && census_shape_is<false, 5, 12, 2, CENSUS_MIRROR> &&
              census_shape_is<false, 7, 24, 3, CENSUS_MIRROR> && census_shape_is<false, 9, 40, 5, CENSUS_MIRROR>);
static_assert(CensusShape<false, 11, CENSUS_MIRROR>::NBITS == 60);             // above CENSUS_MAX_BITS: not in the list

// THE list of descriptors: f(CensusShape<..>{}) and true for the pair (census_type, k); false, and nothing touched (adf_last_error included), when there is none.
template <class F>
bool census_dispatch(int census_type, int k, F&& f)
{
    constexpr int DENSE = ADF_SGBM_COST_CENSUS_DENSE, SPARSE = ADF_SGBM_COST_CENSUS_SPARSE, MCT_DENSE = ADF_SGBM_COST_MCT_DENSE,
                  MCT_SPARSE = ADF_SGBM_COST_MCT_SPARSE, CS = ADF_SGBM_COST_CENSUS_CS;
    const bool in_range = census_type >= DENSE && census_type <= CS && k > 0 && k < 16;
    switch (in_range ? census_type * 16 + k : 0) {
    case DENSE * 16 + 3: f(CensusShape<false, 3>{}); return true;
    case DENSE * 16 + 5: f(CensusShape<false, 5>{}); return true;
    case DENSE * 16 + 7: f(CensusShape<false, 7>{}); return true;
    case SPARSE * 16 + 5: f(CensusShape<true, 5>{}); return true;
    case SPARSE * 16 + 7: f(CensusShape<true, 7>{}); return true;
    case SPARSE * 16 + 9: f(CensusShape<true, 9>{}); return true;
    case SPARSE * 16 + 11: f(CensusShape<true, 11>{}); return true;
    case MCT_DENSE * 16 + 3: f(CensusShape<false, 3, CENSUS_MEAN>{}); return true;
    case MCT_DENSE * 16 + 5: f(CensusShape<false, 5, CENSUS_MEAN>{}); return true;
    case MCT_DENSE * 16 + 7: f(CensusShape<false, 7, CENSUS_MEAN>{}); return true;
    case MCT_SPARSE * 16 + 5: f(CensusShape<true, 5, CENSUS_MEAN>{}); return true;
    case MCT_SPARSE * 16 + 7: f(CensusShape<true, 7, CENSUS_MEAN>{}); return true;
    case MCT_SPARSE * 16 + 9: f(CensusShape<true, 9, CENSUS_MEAN>{}); return true;
    case MCT_SPARSE * 16 + 11: f(CensusShape<true, 11, CENSUS_MEAN>{}); return true;
    case CS * 16 + 3: f(CensusShape<false, 3, CENSUS_MIRROR>{}); return true;
    case CS * 16 + 5: f(CensusShape<false, 5, CENSUS_MIRROR>{}); return true;
    case CS * 16 + 7: f(CensusShape<false, 7, CENSUS_MIRROR>{}); return true;
    case CS * 16 + 9: f(CensusShape<false, 9, CENSUS_MIRROR>{}); return true;
    default: return false;
    }
}
// Bits / byte planes of the descriptor of `census_type` (ADF_SGBM_COST_CENSUS_* / _MCT_*) at window size k; 0: no such descriptor.
inline int census_bits(int census_type, int k) { int v = 0; census_dispatch(census_type, k, [&](auto s) { v = decltype(s)::NBITS; }); return v; }
inline int census_planes(int census_type, int k) { int v = 0; census_dispatch(census_type, k, [&](auto s) { v = decltype(s)::PLANES; }); return v; }

// ADF_EBADARG with a message when (census_type, k) is not a descriptor of this library, ADF_OK otherwise.
int census_check(int census_type, int k);

// adf_bm_set_cost / adf_sgbm_set_cost on a handle's (cost, size): `plain_cost` (SAD, BT) leaves the size alone, a refused census pair leaves both.
inline int census_cost_set(int& cost, int& size, int plain_cost, int cost_type, int census_size)
{
    if (cost_type != plain_cost) {
        if (int rc = census_check(cost_type, census_size)) return rc;
        size = census_size;
    }
    cost = cost_type;
    return ADF_OK;
}

// The transform of n CV_8UC1 device images (rows `sstride`, images `simage` bytes apart) into uint64 planes (rows
// `dstride`, images `dimage` BYTES apart, all 8-byte aligned), asynchronously on `st`.  Arguments are the caller's to check.
int census_run(int n, const uint8_t* src, ptrdiff_t sstride, ptrdiff_t simage, int W, int H, int census_type, int k,
               uint64_t* dst, ptrdiff_t dstride, ptrdiff_t dimage, hipStream_t st);

// The tile of `src` with origin (x0, y0) plus its N2 halo on every side, into LDS by the whole workgroup; complete on return.
// Coordinates are clamped to the W x H image while loading (replicated edge): a tile may lie partly or wholly outside it.
// CENSUS_MEAN also fills `sums`: sums[r][c] = tile[r][c] + ... + tile[r + K - 1][c], the K rows of the window of the
// tile's pixel row r at tile column c, so a window sum is K adds of neighbouring entries (at most 11 * 255 each).
template <class S>
__device__ __forceinline__ void census_tile_load(uint8_t (&tile)[S::LH][S::LW], uint16_t (&sums)[S::SH][S::SW],
                                                 const uint8_t* src, ptrdiff_t stride, int x0, int y0, int W, int H)
{
    for (int i = threadIdx.x; i < S::LH * S::LW; i += CENSUS_THREADS) {
        const int r = i / S::LW, c = i - r * S::LW;
        const int y = min(max(y0 - S::N2 + r, 0), H - 1), x = min(max(x0 - S::N2 + c, 0), W - 1);
        tile[r][c] = src[(ptrdiff_t)y * stride + x];
    }
    __syncthreads();
    if constexpr (S::RULE == CENSUS_MEAN) {
        for (int i = threadIdx.x; i < S::SH * S::SW; i += CENSUS_THREADS) {
            const int r = i / S::SW, c = i - r * S::SW;
            uint32_t s = 0;
#pragma unroll
            for (int j = 0; j < S::SIZE; j++) s += tile[r + j][c];
            sums[r][c] = (uint16_t)s;
        }
        __syncthreads();
    }
}

// A value read from LDS that the compiler has to take as it is.  Left alone, it packs the pair compares of the MIRROR rule
// and the adds of the window sum into vectors and merges their reads into 4- to 16-byte LDS reads at addresses aligned to
// nothing (a lane's window starts at any byte); those measured 3 x (centre-symmetric 9) to 6 x (modified census dense 7)
// the time of single reads on a 3840 x 2160 image.  The empty statement costs no instruction.
__device__ __forceinline__ uint32_t census_single(uint32_t v) { asm("" : "+v"(v)); return v; }

// The descriptor of the tile's pixel (r, c), halo not counted, as two 32-bit halves, fully unrolled; a bit is 1 on strict
// `>`; rows top to bottom, left to right, first comparison = bit NBITS - 1.  CENTRE: neighbour > centre.  MEAN:
// K * K * neighbour > S, the sum of the K x K window (from `sums`; at most 121 * 255), taken as neighbour > S / (K * K)
// rounded down -- the same for integers, and the byte compare of the CENTRE rule.  MIRROR: neighbour > its mirror image
// through the centre, for the offsets before (0, 0).
template <class S>
__device__ __forceinline__ void census_compare(const uint8_t (&tile)[S::LH][S::LW], const uint16_t (&sums)[S::SH][S::SW],
                                               int r, int c, uint32_t& hi, uint32_t& lo)
{
    uint32_t against = 0;                                      // CENTRE: the centre pixel; MEAN: the window mean, rounded down
    if constexpr (S::RULE == CENSUS_CENTRE) against = tile[r + S::N2][c + S::N2];
    if constexpr (S::RULE == CENSUS_MEAN) {
#pragma unroll
        for (int j = 0; j < S::SIZE; j++) against += census_single(sums[r][c + j]);
        against /= S::SIZE * S::SIZE;
    }
    hi = 0; lo = 0;
    int bit = S::NBITS - 1;                                    // (a compile-time constant at every use: both loops unroll)
#pragma unroll
    for (int dy = -S::N2; dy <= (S::RULE == CENSUS_MIRROR ? 0 : S::N2); dy += S::STEP)
#pragma unroll
        for (int dx = -S::N2; dx <= S::N2; dx += S::STEP) {
            if (dy == 0 && (dx == 0 || (S::RULE == CENSUS_MIRROR && dx > 0))) continue;
            uint32_t b;
            if constexpr (S::RULE == CENSUS_MIRROR)
                b = census_single(tile[r + S::N2 + dy][c + S::N2 + dx]) > census_single(tile[r + S::N2 - dy][c + S::N2 - dx]) ? 1u : 0u;
            else b = tile[r + S::N2 + dy][c + S::N2 + dx] > against ? 1u : 0u;
            if (bit >= 32) hi |= b << (bit - 32);
            else lo |= b << bit;
            bit--;
        }
}

} // namespace adf
