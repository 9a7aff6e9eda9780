// census.h -- what the census transform (census_kernels.hip) and the semi-global matcher's census cost
// (sgbm_matcher.hip) share: which (type, size) pairs exist, and the launch of the transform on device images.
#pragma once

#include "adf_host.h"

namespace adf {

// Bits of the descriptor of `census_type` (ADF_SGBM_COST_CENSUS_DENSE / _SPARSE) at window size k; 0: no such descriptor.
// Dense: every offset of the k x k window but the centre (descriptor.cpp:65-69), k in {3, 5, 7}: 8 / 24 / 48 bits.
// Sparse: every second offset, -k/2, -k/2 + 2, ... (descriptor.cpp:70-74), k in {5, 7, 9, 11}: 8 / 16 / 24 / 36 bits.
inline int census_bits(int census_type, int k)
{
    const bool dense = census_type == ADF_SGBM_COST_CENSUS_DENSE, sparse = census_type == ADF_SGBM_COST_CENSUS_SPARSE;
    if (k % 2 == 0 || !((dense && 3 <= k && k <= 7) || (sparse && 5 <= k && k <= 11))) return 0;
    const int step = dense ? 1 : 2, per_axis = 2 * (k / 2) / step + 1;
    return per_axis * per_axis - ((k / 2) % step == 0 ? 1 : 0);   // the offset (0, 0) is skipped where the grid passes through it
}

// ADF_EBADARG with a message when (census_type, k) is not a descriptor of this library, ADF_OK otherwise.
int census_check(int census_type, int k);

// The transform of n CV_8UC1 device images (rows `sstride`, images `simage` bytes apart) into uint64 planes (rows
// `dstride`, images `dimage` BYTES apart, all 8-byte aligned), asynchronously on `st`.  Arguments are the caller's to check.
int census_run(int n, const uint8_t* src, ptrdiff_t sstride, ptrdiff_t simage, int W, int H, int census_type, int k,
               uint64_t* dst, ptrdiff_t dstride, ptrdiff_t dimage, hipStream_t st);

} // namespace adf
