// census.h -- the census descriptor, stated once for the transform (census_kernels.hip), the block matcher's pack kernel
// (bm_matcher.hip) and the semi-global matcher's cost (sgbm_matcher.hip): its compile-time facts (CensusShape), the one list
// of the (type, size) pairs that exist (census_dispatch), the LDS tile load and the comparison loop, the shared host rules.
#pragma once

#include "adf_host.h"

namespace adf {

// the block matcher's setter hands its cost type to census_check, which names the semi-global matcher's constants
static_assert(ADF_BM_COST_CENSUS_DENSE == ADF_SGBM_COST_CENSUS_DENSE && ADF_BM_COST_CENSUS_SPARSE == ADF_SGBM_COST_CENSUS_SPARSE);
constexpr int CENSUS_TILE_W = 64, CENSUS_TILE_H = 16, CENSUS_THREADS = 256;   // pixels and threads of a workgroup: a wave per row, four rows per sweep
// relied on by CensusCost::MAX_PIXEL (two disparities per register at every block size) and by the block matcher (window sums below 2^16)
constexpr int CENSUS_MAX_BITS = 48, CENSUS_MAX_PLANES = 6;

// The descriptor at odd window size K.  Dense: every offset of the K x K window but the centre (descriptor.cpp:65-69).
// Sparse: every second offset, -K/2, -K/2 + 2, ... (descriptor.cpp:70-74); the offset (0, 0) is skipped where the grid
// passes through it.  PLANES: the bytes that hold the bits.  LW x LH: the workgroup's tile with its halo.
template <bool SPARSE, int K>
struct CensusShape {
    static constexpr int N2 = K / 2, STEP = SPARSE ? 2 : 1;
    static constexpr int PER_AXIS = 2 * N2 / STEP + 1, NBITS = PER_AXIS * PER_AXIS - (N2 % STEP == 0 ? 1 : 0);
    static constexpr int PLANES = (NBITS + 7) / 8;
    static constexpr int LW = CENSUS_TILE_W + 2 * N2, LH = CENSUS_TILE_H + 2 * N2;
};
template <bool SPARSE, int K, int BITS, int PLANES, class S = CensusShape<SPARSE, K>>
constexpr bool census_shape_is = S::NBITS == BITS && S::PLANES == PLANES && BITS <= CENSUS_MAX_BITS && PLANES <= CENSUS_MAX_PLANES;
static_assert(census_shape_is<false, 3, 8, 1> && census_shape_is<false, 5, 24, 3> && census_shape_is<false, 7, 48, 6>);
static_assert(census_shape_is<true, 5, 8, 1> && census_shape_is<true, 7, 16, 2> && census_shape_is<true, 9, 24, 3> && census_shape_is<true, 11, 36, 5>);

// THE list of descriptors: f(CensusShape<..>{}) and true for the pair (census_type, k); false, and nothing touched (adf_last_error included), when there is none.
template <class F>
bool census_dispatch(int census_type, int k, F&& f)
{
    const bool dense = census_type == ADF_SGBM_COST_CENSUS_DENSE, sparse = census_type == ADF_SGBM_COST_CENSUS_SPARSE;
    switch (k <= 0 ? 0 : dense ? k : sparse ? -k : 0) {
    case 3: f(CensusShape<false, 3>{}); return true;
    case 5: f(CensusShape<false, 5>{}); return true;
    case 7: f(CensusShape<false, 7>{}); return true;
    case -5: f(CensusShape<true, 5>{}); return true;
    case -7: f(CensusShape<true, 7>{}); return true;
    case -9: f(CensusShape<true, 9>{}); return true;
    case -11: f(CensusShape<true, 11>{}); return true;
    default: return false;
    }
}
// Bits / byte planes of the descriptor of `census_type` (ADF_SGBM_COST_CENSUS_DENSE / _SPARSE) at window size k; 0: no such descriptor.
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
template <class S>
__device__ __forceinline__ void census_tile_load(uint8_t (&tile)[S::LH][S::LW], const uint8_t* src, ptrdiff_t stride, int x0, int y0, int W, int H)
{
    for (int i = threadIdx.x; i < S::LH * S::LW; i += CENSUS_THREADS) {
        const int r = i / S::LW, c = i - r * S::LW;
        const int y = min(max(y0 - S::N2 + r, 0), H - 1), x = min(max(x0 - S::N2 + c, 0), W - 1);
        tile[r][c] = src[(ptrdiff_t)y * stride + x];
    }
    __syncthreads();
}

// The descriptor of the tile's pixel (r, c), halo not counted, as two 32-bit halves: byte compares against the centre,
// fully unrolled; a bit is 1 when the neighbour is larger; rows top to bottom, left to right, first comparison = bit NBITS - 1.
template <class S>
__device__ __forceinline__ void census_compare(const uint8_t (&tile)[S::LH][S::LW], int r, int c, uint32_t& hi, uint32_t& lo)
{
    const uint32_t centre = tile[r + S::N2][c + S::N2];
    hi = 0; lo = 0;
    int bit = S::NBITS - 1;                                    // (a compile-time constant at every use: both loops unroll)
#pragma unroll
    for (int dy = -S::N2; dy <= S::N2; dy += S::STEP)
#pragma unroll
        for (int dx = -S::N2; dx <= S::N2; dx += S::STEP) {
            if (dy == 0 && dx == 0) continue;
            const uint32_t b = tile[r + S::N2 + dy][c + S::N2 + dx] > centre ? 1u : 0u;
            if (bit >= 32) hi |= b << (bit - 32);
            else lo |= b << bit;
            bit--;
        }
}

} // namespace adf
