// census_kernels.hip -- the census transform on the device: the descriptor the semi-global matcher's Hamming cost
// compares (sgbm_matcher.hip, ADF_SGBM_COST_CENSUS_*), and adf_census_transform_* of include/adf_wls.h.  The descriptor -- the
// pairs that exist, their bits, the tile load, the comparison loop -- is stated in census.h; the kernel here sweeps rows and stores.
//
// The reference's own semi-global matcher, cv::stereo::StereoBinarySGBM, matches on census descriptors
// (modules/stereo/src/stereo_binary_sgbm.cpp, include/opencv2/stereo/descriptor.hpp, src/descriptor.cpp).  What is built
// here is the published transform (Zabih & Woodfill 1994) with the bit rule of descriptor.hpp:182-194 (a bit is 1 when
// the neighbour is larger than the centre, the first comparison ends up most significant) and the two sampling grids
// of descriptor.cpp:65-74 (every offset / every second offset).  It is THIS LIBRARY'S definition, not a bit-level copy
// of the in-tree code, which is no usable oracle: its row ranges read one row past Range::end (descriptor.hpp:219), it
// compares a row OFFSET with a row INDEX to skip the centre (`ii != i`, descriptor.hpp:234), and it leaves the border
// pixels unwritten (descriptor.hpp:222).  Here neighbour coordinates are clamped to the image (replicated edge), so every
// pixel has a descriptor, and the offset (0, 0) is skipped where the grid passes through it.
//
// Two more comparison rules run through the same kernel (census.h, CensusRule): the modified census
// transform (Froeba & Ernst 2004; ADF_SGBM_COST_MCT_*: neighbours against the window mean) and the centre-symmetric census
// (Spangenberg et al. 2013; ADF_SGBM_COST_CENSUS_CS: neighbours against their mirror image, half the bits).
//
// Bit order: rows top to bottom, left to right within a row; the first comparison is bit nbits-1, the upper 64 - nbits
// bits are zero.  One uint64 per pixel.
#include "census.h"

using namespace adf;

namespace {

struct CensusArgs {
    const uint8_t* src; ptrdiff_t sstride, simage;
    uint64_t* dst; ptrdiff_t dstride, dimage;       // bytes
    int W, H;
};

// One workgroup: the 64 x 16 tile plus its K/2 halo on every side in LDS (census_tile_load; with the window-mean rule
// also the tile's column sums), then one pixel per lane and sweep: the descriptor's compares (census_compare) and one
// 8-byte store per lane.
template <class S>
__global__ void __launch_bounds__(CENSUS_THREADS) census_kernel(CensusArgs a)
{
    __shared__ uint8_t tile[S::LH][S::LW];
    __shared__ uint16_t sums[S::SH][S::SW];                    // the mean rule's column sums; not referenced by the other rules
    const int x0 = blockIdx.x * CENSUS_TILE_W, y0 = blockIdx.y * CENSUS_TILE_H;
    census_tile_load<S>(tile, sums, a.src + (ptrdiff_t)blockIdx.z * a.simage, a.sstride, x0, y0, a.W, a.H);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 + lane;
    if (x >= a.W) return;
    for (int r = wv; r < CENSUS_TILE_H; r += CENSUS_THREADS / 64) {
        const int y = y0 + r;
        if (y >= a.H) break;
        uint32_t hi, lo;
        census_compare<S>(tile, sums, r, lane, hi, lo);
        uint64_t* row = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(a.dst) + (ptrdiff_t)blockIdx.z * a.dimage + (ptrdiff_t)y * a.dstride);
        row[x] = ((uint64_t)hi << 32) | lo;
    }
}

int census_args_check(int n, const void* src, ptrdiff_t sstride, ptrdiff_t simage, int W, int H, int type, int k,
                      const void* dst, ptrdiff_t dstride, ptrdiff_t dimage)
{
    if (n <= 0 || !src || !dst) return fail(ADF_EBADARG, "censusTransform: images must be non-NULL, n_images positive");
    if (int rc = census_check(type, k)) return rc;
    if (W <= 0 || H <= 0 || sstride < (ptrdiff_t)W || dstride < (ptrdiff_t)W * 8) return fail(ADF_ESIZE, "censusTransform: bad size or stride");
    if (n > 1 && (simage < 0 || dimage < 0)) return fail(ADF_ESIZE, "censusTransform: image strides must not be negative");
    if ((reinterpret_cast<uintptr_t>(dst) & 7) || (dstride & 7) || (n > 1 && (dimage & 7)))
        return fail(ADF_EBADARG, "censusTransform: dst and its strides must be 8-byte aligned (one uint64 per pixel)");
    return ADF_OK;
}

} // namespace

int adf::census_check(int census_type, int k)
{
    if (census_type < ADF_SGBM_COST_CENSUS_DENSE || census_type > ADF_SGBM_COST_CENSUS_CS || census_type == 3)
        return fail(ADF_EBADARG, "census type %d is not ADF_SGBM_COST_CENSUS_DENSE (1), ADF_SGBM_COST_CENSUS_SPARSE (2), ADF_SGBM_COST_MCT_DENSE (4), "
                                 "ADF_SGBM_COST_MCT_SPARSE (5) or ADF_SGBM_COST_CENSUS_CS (6)", census_type);
    if (census_bits(census_type, k) == 0)
        return fail(ADF_EBADARG, "census size %d is not supported: odd, 3..7 for the dense, 5..11 for the sparse (census and modified census) "
                                 "and 3..9 for the centre-symmetric descriptor (at most 48 bits)", k);
    return ADF_OK;
}

int adf::census_run(int n, const uint8_t* src, ptrdiff_t sstride, ptrdiff_t simage, int W, int H, int census_type, int k,
                    uint64_t* dst, ptrdiff_t dstride, ptrdiff_t dimage, hipStream_t st)
{
    return for_batches(n, GRID_LIMIT, [&](int m0, int nm) {
        const CensusArgs a{src + (ptrdiff_t)m0 * simage, sstride, n > 1 ? simage : 0,
                           reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(dst) + (ptrdiff_t)m0 * dimage), dstride, n > 1 ? dimage : 0, W, H};
        const dim3 grid((W + CENSUS_TILE_W - 1) / CENSUS_TILE_W, (H + CENSUS_TILE_H - 1) / CENSUS_TILE_H, nm);
        const bool known = census_dispatch(census_type, k, [&](auto s) { hipLaunchKernelGGL((census_kernel<decltype(s)>), grid, dim3(CENSUS_THREADS), 0, st, a); });
        return known ? launched() : fail(ADF_EBADARG, "census size %d is not supported", k);
    });
}

// ----------------------------------------------------------------------------------------------
// C-ABI (include/adf_wls.h, "census transform")
// ----------------------------------------------------------------------------------------------
extern "C" int adf_census_transform_device(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                                           int W, int H, int census_type, int census_size,
                                           uint64_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride, void* stream)
{
    const int rc = census_args_check(n_images, src, src_stride, src_image_stride, W, H, census_type, census_size, dst, dst_stride, dst_image_stride);
    if (rc) return rc;
    return census_run(n_images, src, src_stride, src_image_stride, W, H, census_type, census_size, dst, dst_stride, dst_image_stride,
                      (hipStream_t)stream);
}

extern "C" int adf_census_transform_host(int n_images, const uint8_t* src, ptrdiff_t src_stride, ptrdiff_t src_image_stride,
                                         int W, int H, int census_type, int census_size,
                                         uint64_t* dst, ptrdiff_t dst_stride, ptrdiff_t dst_image_stride)
{
    int rc = census_args_check(n_images, src, src_stride, src_image_stride, W, H, census_type, census_size, dst, dst_stride, dst_image_stride);
    if (rc) return rc;
    // one block: the descriptor planes (8-byte aligned at its start), then the source images
    const size_t srow = (size_t)W, drow = (size_t)W * 8, simg = srow * H, dimg = drow * H;
    Scratch blk;
    if ((rc = blk.take((simg + dimg) * (size_t)n_images, nullptr))) return rc;
    uint64_t* dd = static_cast<uint64_t*>(blk.p);
    uint8_t* ds = static_cast<uint8_t*>(blk.p) + dimg * n_images;
    if ((rc = copy_images(ds, srow, simg, src, src_stride, src_image_stride, srow, H, n_images, hipMemcpyHostToDevice, nullptr))) return rc;
    rc = census_run(n_images, ds, (ptrdiff_t)srow, (ptrdiff_t)simg, W, H, census_type, census_size, dd, (ptrdiff_t)drow, (ptrdiff_t)dimg, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(dst, dst_stride, dst_image_stride, dd, drow, dimg, drow, H, n_images, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
