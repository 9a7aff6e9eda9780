// adf_host.h -- the host toolkit every C-ABI source shares (adf_host.hip): error returns, the device scope, device
// memory (growable buffers, the process-wide block cache, scratch taken from it), the weight tables, the image copies
// of the host-pointer entry points, and what the stateless operators' launches share: the launch check, rounding up,
// THE batch loop over the grid limit, THE launch of a tile kernel over every tile of every image, the rule for
// destination images that must not overlap, the choice between a caller's workspace and library scratch, and what the
// five edge-aware filters' entry points share: the depths, alignment, the bytes a batch spans, the borders that are
// built, THE record of a call's images (FilterImages), THE tail of their checks from alignment to overlap
// (filter_geometry_check) and THE host-pointer call on staged images (staged_call).  Host code only; what kernels and
// host code share is adf_internal.h.
#pragma once

#include "adf_internal.h"
#include "../../include/adf_wls.h"

#include <algorithm>
#include <memory>
#include <vector>

namespace adf {

// Records the calling thread's last error message (adf_last_error), printf-style, and returns `code`.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return adf::fail(e_ == hipErrorOutOfMemory ? ADF_ENOMEM : ADF_EHIP, "%s failed: %s",   \
                             #expr, hipGetErrorString(e_));                                        \
    } while (0)
#define NEED_HANDLE(h) do { if (!(h)) return adf::fail(ADF_EBADARG, "%s: handle is NULL", __func__); } while (0)

// RAII: run on the handle's device, restore the caller's on exit.
struct DeviceScope {
    int prev = -1; bool switched = false;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() { if (switched) hipSetDevice(prev); }
};

bool stream_is_capturing(hipStream_t st);

#define ADF_LOCAL __attribute__((visibility("hidden")))   // shared by the library's sources, not a dynamic symbol
ADF_LOCAL int launched();                      // after a call's launches: ADF_OK, or ADF_EHIP with the runtime's message
constexpr size_t pad_to(size_t v, size_t a) { return (v + a - 1) / a * a; }   // v rounded up to a multiple of a

// THE loop over a batch that one grid dimension cannot hold: f(m0, nm) launches images [m0, m0 + nm), nm <= per_launch,
// re-pointing whatever it addresses per image by m0; the first non-zero return ends the loop and is returned.
constexpr int GRID_LIMIT = 65535;              // what a grid holds along y or z: the images of one launch
template <class F> int for_batches(int n, int per_launch, F&& f)
{
    for (int m0 = 0, nm; m0 < n; m0 += nm)
        if (int rc = f(m0, nm = std::min(n - m0, per_launch))) return rc;
    return ADF_OK;
}

// THE launch of a tile kernel -- one workgroup of tile_w x tile_h threads per tile of as many output pixels, the images
// along the grid's y -- over every tile of n images of W x H.  ARGS has tiles_x (tiles per row of tiles, set here) and
// tile0 (the first tile of a launch); a launch holds up to GRID_LIMIT images and PER_LAUNCH tiles.  point(a, m0)
// re-points the args at image m0.  A kernel whose dynamic LDS comes near the default limit has the limit raised first.
template <class ARGS, class POINT>
ADF_LOCAL int launch_tiles(void (*kernel)(ARGS), size_t lds, int W, int H, int tile_w, int tile_h, int n, ARGS a, hipStream_t st, POINT&& point)
{
    if (lds > 48 * 1024 - 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles_y = (unsigned)((H + tile_h - 1) / tile_h);
    a.tiles_x = (unsigned)((W + tile_w - 1) / tile_w);
    const uint64_t tiles = (uint64_t)a.tiles_x * tiles_y;               // W*H is below 2^31 and a tile has 256 pixels: 32 bits
    constexpr uint64_t PER_LAUNCH = 1u << 22;                            // (a grid's threads stay below 2^31)
    return for_batches(n, GRID_LIMIT, [&](int m0, unsigned nm) {
        point(a, m0);
        for (uint64_t t0 = 0; t0 < tiles; t0 += PER_LAUNCH) {
            a.tile0 = (unsigned)t0;
            hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(tiles - t0, PER_LAUNCH), nm), dim3((unsigned)(tile_w * tile_h)), lds, st, a);
        }
        return launched();
    });
}

// n images of `rows` rows of `row_bytes` (rows `stride`, images `image_stride` bytes apart) stay clear of one another:
// they follow one another or, where the operator allows it, interleave row by row.
ADF_LOCAL bool images_disjoint(int n, ptrdiff_t row_bytes, int rows, ptrdiff_t stride, ptrdiff_t image_stride, bool may_interleave);

// What the edge-aware filters' checks share.  An image depth (ADF_8U, ADF_16S, ADF_32F) and its bytes per pixel:
constexpr bool known_depth(int depth) { return depth == ADF_8U || depth == ADF_16S || depth == ADF_32F; }
constexpr size_t depth_size(int depth) { return depth == ADF_8U ? 1 : depth == ADF_16S ? 2 : 4; }
// A pointer and its strides are multiples of the element size `es` (a power of two).
inline bool aligned(const void* p, ptrdiff_t stride, ptrdiff_t map_stride, ptrdiff_t es)
{
    return !(((uintptr_t)p & (es - 1)) || (stride & (es - 1)) || (map_stride & (es - 1)));
}
// The bytes n images span, [lo, hi): what "overlap" is tested on.
struct Span { uintptr_t lo, hi; };
inline Span span_of(const void* p, int n, ptrdiff_t row_bytes, int rows, ptrdiff_t stride, ptrdiff_t map_stride)
{
    const uintptr_t b = reinterpret_cast<uintptr_t>(p);
    return Span{b, b + (uintptr_t)((ptrdiff_t)(n - 1) * map_stride + (ptrdiff_t)(rows - 1) * stride + row_bytes)};
}
inline bool overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }
// The borders the bilateral filters build are BORDER_REPLICATE, BORDER_REFLECT and BORDER_REFLECT_101: BORDER_CONSTANT
// and BORDER_WRAP are refused by name, any other value by number.
ADF_LOCAL int border_check(const char* who, int border);

// THE images of one edge-aware filter call (weighted median, guided, domain transform, joint bilateral, rolling
// guidance): n maps of W x H each.  A filter's call record holds one next to its own parameters.
struct FilterImage {
    void* p; ptrdiff_t stride, map_stride;     // bytes between rows and between maps; p null: the call has no such image
    uint8_t* map(int m0) const { return static_cast<uint8_t*>(p) + (ptrdiff_t)m0 * map_stride; }   // map m0: what a launch is pointed at
};
struct FilterImages {
    int n, W, H;
    FilterImage guide; int guide_channels;     // 8-bit guide or joint (read only); none: rolling guidance
    FilterImage src; int src_depth;            // (read only)
    FilterImage dst; int dst_depth;
    FilterImage mask;                          // 8-bit (read only); none: every filter but the weighted median, and there optional
};
inline FilterImage image_of(const void* p, ptrdiff_t stride, ptrdiff_t map_stride) { return FilterImage{const_cast<void*>(p), stride, map_stride}; }
// The tail of the five filters' checks, after each one's own head (NULL, empty, depths, parameters), in this order:
// alignment to the depths, W*H below 2^31, row strides, negative map strides, destination maps that overlap one
// another, a destination that overlaps an input.  `depths` ("their depths", "the depth") and `inputs` (the names after
// "dst must not overlap") are the two phrases in which the filters' texts differ.
ADF_LOCAL int filter_geometry_check(const char* who, const FilterImages& im, const char* depths, const char* inputs);

// Growable device buffer (never shrinks; freed with the handle).  Growing drains `st` before the old block is freed.
// FILL_ZERO clears a newly allocated block on `st` (the filters: the sweeps read, and discard, pitch padding);
// FILL_NONE leaves it as the driver gave it (the matchers' workspaces: gigabytes that are written before they are read).
enum Fill { FILL_NONE, FILL_ZERO };
struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    int reserve(size_t need, hipStream_t st, Fill fill);
    void release() { if (p) hipFree(p); p = nullptr; bytes = 0; }
};

// hipMalloc that, when the driver refuses, first hands the library's own cache of device blocks (below, up to 3 GB)
// back to the driver and tries once more: no call may fail for want of memory the library itself is sitting on.
hipError_t device_malloc(void** p, size_t bytes);
// The process-wide cache of device blocks (adf_host.hip: BlockCache).  take: a cached block of at least `need` bytes
// on `device`, ordered into `st` behind its last user, or null.  give: after queueing the work that uses the block --
// `ready` (may be null: idle), or an event recorded on `st`, goes with it, so nobody synchronises the host.
void* cache_take(int device, size_t need, hipStream_t st, size_t* bytes);
void cache_give(int device, void* p, size_t bytes, hipStream_t st);
void cache_give_event(int device, void* p, size_t bytes, hipEvent_t ready);

// Library scratch of one call on the current device: a block of the cache, else a fresh allocation, ordered into `st`;
// it goes back to the cache behind `st` when the scope ends -- on an error return too.
struct Scratch {
    int device = 0; void* p = nullptr; size_t bytes = 0; hipStream_t st = nullptr;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    int take(size_t need, hipStream_t stream);
    ~Scratch() { if (p) cache_give(device, p, bytes, st); }
};

// *ws = the caller's workspace of a `who` call when there is one (refused when smaller than `need`, the result of
// `size_fn`, or not 4-byte aligned), else library scratch in `blk` ordered into `st` (refused inside a stream capture).
ADF_LOCAL int workspace_or_scratch(const char* who, const char* size_fn, void* workspace, size_t workspace_bytes, size_t need,
                                   hipStream_t st, Scratch& blk, void** ws);

// The weight tables of one handle (FGS.cpp:150-154, 663-675): up to LUT_CACHE sigmas, each an immutable device table
// shared with every handle of the process on the same device (adf_host.hip: LutStore).
struct LutTable;
struct Lut {
    static constexpr int LUT_CACHE = 8;
    struct Entry { std::shared_ptr<LutTable> t; unsigned long long used; };
    std::vector<Entry> tables;
    const float* cur = nullptr;
    unsigned long long tick = 0;
    size_t bytes() const { return tables.size() * sizeof(float) * ADF_LUT_LEVELS; }
    int ensure(float s, hipStream_t st);
    // (the caller has made sure no kernel still reads the tables: handle destruction synchronises first)
    void release() { tables.clear(); cur = nullptr; }
};

// The weighted median filter's weight table (include/adf_wls.h: T, ADF_WMF_TABLE_LEVELS uint32 entries): an immutable
// device table per (device, sigma, weight type), shared by every call of the process (adf_host.hip: WmfStore, 16 of them).
struct WmfTable;
ADF_LOCAL int wmf_weights_check(const char* who, double sigma, int weight_type);   // the refusals both entry kinds share
// The table of the current device: a look-up when the key was seen before (no device work, capturable), else built on
// the host and uploaded with one synchronous copy.  The caller holds `out` until its launches are queued.
ADF_LOCAL int wmf_table_device(double sigma, int weight_type, std::shared_ptr<WmfTable>& out, const uint32_t** dev);

// The joint bilateral filter's tables (include/adf_wls.h: C, then S, in one block of floats): an immutable device table
// per (device, sigma_color, sigma_space, r, joint channels), shared by every call of the process (adf_host.hip: JbfStore).
struct JbfTable;
// The refusals both entry kinds and adf_jbf_tables_host share; on ADF_OK the clamped sigmas and the radius.
ADF_LOCAL int jbf_params_check(const char* who, int d, double sigma_color, double sigma_space, int joint_channels,
                               double* sc, double* ss, int* r);
constexpr size_t jbf_colour_entries(int channels) { return (size_t)255 * channels + 1; }
constexpr size_t jbf_space_entries(int r) { return (size_t)r * r + 1; }
// The tables of the current device, as wmf_table_device: a look-up when the key was seen before (capturable), else built
// on the host and uploaded with one synchronous copy.  The caller holds `out` until its launches are queued.
ADF_LOCAL int jbf_table_device(double sc, double ss, int r, int channels, std::shared_ptr<JbfTable>& out,
                               const float** colour, const float** space);

// The rolling guidance filter's tables (include/adf_wls.h: the range table C of T entries, or G of RGF_GRID_ENTRIES
// for ADF_32F, then S, in one block of floats): an immutable device table per (device, depth, sigma_color, sigma_space,
// r), kept like the joint bilateral filter's (adf_host.hip: RgfStore).
struct RgfTable;
constexpr size_t RGF_GRID_ENTRIES = 4098;  // G[0 .. 4097]
// The refusals the entry points and adf_rgf_tables_host share (jbf_params_check's, an unknown depth, a `scale` that is
// not finite); on ADF_OK the clamped sigmas, the radius and scale (1.0f for the integer depths).
ADF_LOCAL int rgf_params_check(const char* who, int depth, int d, double sigma_color, double sigma_space,
                               double* sc, double* ss, int* r, float* scale);
// T for an integer depth (the entries up to and including the first that rounds to 0.0f), 4098 for ADF_32F.
ADF_LOCAL size_t rgf_colour_entries(int depth, double sc);
// As jbf_table_device; *entries = what rgf_colour_entries gives.
ADF_LOCAL int rgf_table_device(int depth, double sc, double ss, int r, std::shared_ptr<RgfTable>& out,
                               const float** colour, const float** space, int* entries);

// The host-pointer entry points' copies: `n` images of `rows` rows of `row_bytes`, image k at `k * image_stride` bytes
// with rows `pitch` bytes apart on either side, asynchronously on `st` (a host destination is complete once `st` has
// been synchronised).  The layout of a staging block stays with the caller.
int copy_images(void* dst, size_t dst_pitch, ptrdiff_t dst_image_stride, const void* src, size_t src_pitch,
                ptrdiff_t src_image_stride, size_t row_bytes, size_t rows, int n, hipMemcpyKind kind, hipStream_t st);

// THE host-pointer entry of an edge-aware filter, after its check: one scratch block holds the guides, dense, then the
// sources, the masks, the results and `ws_bytes` of workspace, each part padded to 256 bytes (an image the call does not
// have takes none); the inputs are copied in, run(the same images on the device, the workspace, the null stream) queues
// the filter, and the results are copied out and waited for.
template <class RUN> int staged_call(const FilterImages& host, size_t ws_bytes, RUN&& run)
{
    FilterImages dev = host;
    const FilterImage* from[4] = {&host.guide, &host.src, &host.mask, &host.dst};
    FilterImage* to[4] = {&dev.guide, &dev.src, &dev.mask, &dev.dst};
    const size_t pixel[4] = {(size_t)host.guide_channels, depth_size(host.src_depth), 1, depth_size(host.dst_depth)};
    size_t row[4], at[5] = {0};
    for (int k = 0; k < 4; k++) {
        row[k] = from[k]->p ? pixel[k] * (size_t)host.W : 0;
        at[k + 1] = at[k] + pad_to(row[k] * (size_t)host.H * (size_t)host.n, 256);
    }
    Scratch blk;
    if (int rc = blk.take(at[4] + ws_bytes, nullptr)) return rc;
    char* base = static_cast<char*>(blk.p);
    for (int k = 0; k < 4; k++) {
        if (!row[k]) continue;
        *to[k] = FilterImage{base + at[k], (ptrdiff_t)row[k], (ptrdiff_t)(row[k] * (size_t)host.H)};
        if (k == 3) break;                                               // the results: nothing to copy in
        if (int rc = copy_images(to[k]->p, row[k], to[k]->map_stride, from[k]->p, (size_t)from[k]->stride, from[k]->map_stride, row[k],
                                 (size_t)host.H, host.n, hipMemcpyHostToDevice, nullptr))
            return rc;
    }
    if (int rc = run(dev, static_cast<void*>(base + at[4]), (hipStream_t)nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (int rc = copy_images(host.dst.p, (size_t)host.dst.stride, host.dst.map_stride, dev.dst.p, row[3], dev.dst.map_stride, row[3],
                             (size_t)host.H, host.n, hipMemcpyDeviceToHost, nullptr))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

} // namespace adf
