// speckle_kernels.hip -- cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, buf) (calib3d; in-tree call site
// modules/stereo/src/stereo_binary_sgbm.cpp:716-718) on the device, for CV_16SC1 maps: connected-component labelling
// of the tolerance graph, then every component of at most maxSpeckleSize pixels becomes newVal.
//
//   pixels equal to newVal belong to no component; 4-neighbours p, q are joined when both differ from newVal and
//   |d(p) - d(q)| <= maxDiff (int32: int16 extremes differ by 65535).  maxSpeckleSize <= 0 and a negative maxDiff
//   need no special case: no component has fewer than one pixel, and no pair differs by a negative amount.
//
// Four launches per batch, no workgroup ever waits for another (phases that need another workgroup's writes are
// separate launches):
//   1. tile    one workgroup per 64 x 32 tile: union-find in LDS over the tile's left / up edges, then every pixel's
//              label = map-linear index of its tile-local root, and the root's pixel count in `sizes` (0 elsewhere)
//   2. merge   one thread per edge crossing a tile boundary: union of the two labels in global memory, every parent
//              read and write an agent-scope atomic (per-XCD L2s / per-CU L1s are not coherent)
//   3. count   every tile root that is no longer a root adds its count to its component's root (one atomic per
//              (tile, root), skipped once the root is past maxSpeckleSize) and points straight at that root
//   4. apply   pixel -> tile root -> component root; components of at most maxSpeckleSize pixels become newVal
// Workspace: int32 labels + int32 sizes per pixel (8 B/px).  The result does not depend on the order in which unions
// happen (a component is a set; its size is a number), so it is bit-exact and identical from run to run.
//
// Termination.  A parent pointer never exceeds its own index (tile pass: the smaller root is the parent; merge: a CAS
// only replaces a root's self-pointer by a smaller label; path halving and the count pass only store ancestors, which
// are smaller).  So every find loop strictly decreases its index and ends within index + 1 steps, and every union
// loop strictly decreases a + b per retry (a failed CAS returns the smaller label a was linked to meanwhile) and ends
// within a + b + 1 retries.  Labels are map-linear int32 indices: W * H < 2^31 is required.
#include "adf_host.h"

using namespace adf;

namespace {

constexpr int TW = 64, TH = 32, TN = TW * TH, NT = 256, PPT = TN / NT;

struct SpeckleArgs {
    int16_t* img; ptrdiff_t stride, map_stride;   // bytes
    int W, H, tiles_x, tiles_y;
    int new_val, max_size, max_diff;
    int* labels; int* sizes;                      // [map][W*H] each
    int plane;                                    // W * H
};

__device__ __forceinline__ bool joined(int p, int q, int nv, int md)
{
    return p != nv && q != nv && abs(p - q) <= md;
}

// ---- union-find in LDS (one workgroup; workgroup-scope atomics) ----
__device__ __forceinline__ int lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ int lds_find(int* par, int x)
{
    // par[x] < x except at a root: x strictly decreases, at most x + 1 steps.  Path halving stores the grandparent,
    // an ancestor, so the bound survives concurrent halving.
    int p = lds_ld(&par[x]);
    while (p != x) {
        const int g = lds_ld(&par[p]);
        if (g != p) __hip_atomic_store(&par[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        x = p;
        p = g;
    }
    return x;
}

__device__ void lds_union(int* par, int a, int b)
{
    for (;;) {                                   // a + b strictly decreases per retry
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expected = a;                        // link the larger root under the smaller one, if it is still a root
        if (__hip_atomic_compare_exchange_strong(&par[a], &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP))
            return;
        a = expected;                            // a was linked meanwhile, to a smaller label
    }
}

// ---- union-find in global memory (merge pass; agent-scope atomics for every parent access) ----
__device__ __forceinline__ int glb_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int glb_find(int* L, int x)
{
    // A load may return an older value of a pointer; every value ever stored there is an ancestor (or, for a root that
    // has been linked since, the root itself -- the CAS below then fails and hands back the newer parent).
    int p = glb_ld(&L[x]);
    while (p != x) {
        const int g = glb_ld(&L[p]);
        if (g != p) __hip_atomic_store(&L[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

__device__ void glb_union(int* L, int a, int b)
{
    for (;;) {                                   // a + b strictly decreases per retry
        a = glb_find(L, a);
        b = glb_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expected = a;
        if (__hip_atomic_compare_exchange_strong(&L[a], &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = expected;
    }
}

__global__ void __launch_bounds__(NT) speckle_tile_kernel(SpeckleArgs a)
{
    __shared__ int val[TN], par[TN], cnt[TN];
    const int t = threadIdx.x, map = blockIdx.y;
    const int x0 = (int)(blockIdx.x % a.tiles_x) * TW, y0 = (int)(blockIdx.x / a.tiles_x) * TH;
    const char* src = reinterpret_cast<const char*>(a.img) + (ptrdiff_t)map * a.map_stride;
    for (int k = 0; k < PPT; k++) {
        const int i = t + k * NT, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        // outside the map = newVal: no component, no edge
        val[i] = (x < a.W && y < a.H) ? (int)reinterpret_cast<const int16_t*>(src + (ptrdiff_t)y * a.stride)[x] : a.new_val;
        par[i] = i;
        cnt[i] = 0;
    }
    __syncthreads();
    for (int k = 0; k < PPT; k++) {
        const int i = t + k * NT, v = val[i];
        if (v == a.new_val) continue;
        if ((i & (TW - 1)) > 0 && joined(v, val[i - 1], a.new_val, a.max_diff)) lds_union(par, i, i - 1);
        if (i >= TW && joined(v, val[i - TW], a.new_val, a.max_diff)) lds_union(par, i, i - TW);
    }
    __syncthreads();
    int root[PPT];
    for (int k = 0; k < PPT; k++) {
        const int i = t + k * NT;
        root[k] = i;
        if (val[i] != a.new_val) {
            root[k] = lds_find(par, i);
            atomicAdd(&cnt[root[k]], 1);
        }
    }
    __syncthreads();
    int* lab = a.labels + (size_t)map * a.plane;
    int* siz = a.sizes + (size_t)map * a.plane;
    for (int k = 0; k < PPT; k++) {
        const int i = t + k * NT, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        if (x >= a.W || y >= a.H) continue;
        const int r = root[k];
        // tile-local order = map-linear order, so the root is still its tile component's smallest index
        lab[y * a.W + x] = (y0 + r / TW) * a.W + x0 + (r & (TW - 1));
        siz[y * a.W + x] = r == i ? cnt[i] : 0;       // (newVal pixels: their own label, count 0)
    }
}

// Edges crossing a tile boundary: first (tiles_x-1) * H edges (x-1, y)-(x, y) at x = multiples of TW, then
// (tiles_y-1) * W edges (x, y-1)-(x, y) at y = multiples of TH.
__global__ void __launch_bounds__(256) speckle_merge_kernel(SpeckleArgs a, int n_vert, int n_edges)
{
    int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= n_edges) return;
    int px, py, qx, qy;
    if (e < n_vert) {
        const int b = e / a.H;
        py = qy = e - b * a.H;
        qx = (b + 1) * TW;
        px = qx - 1;
    } else {
        e -= n_vert;
        const int b = e / a.W;
        px = qx = e - b * a.W;
        qy = (b + 1) * TH;
        py = qy - 1;
    }
    const char* src = reinterpret_cast<const char*>(a.img) + (ptrdiff_t)blockIdx.y * a.map_stride;
    const int vp = reinterpret_cast<const int16_t*>(src + (ptrdiff_t)py * a.stride)[px];
    const int vq = reinterpret_cast<const int16_t*>(src + (ptrdiff_t)qy * a.stride)[qx];
    if (!joined(vp, vq, a.new_val, a.max_diff)) return;
    glb_union(a.labels + (size_t)blockIdx.y * a.plane, py * a.W + px, qy * a.W + qx);
}

__global__ void __launch_bounds__(256) speckle_count_kernel(SpeckleArgs a)
{
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= a.plane) return;
    int* lab = a.labels + (size_t)blockIdx.y * a.plane;
    int* siz = a.sizes + (size_t)blockIdx.y * a.plane;
    const int s = siz[p];
    if (s == 0) return;                               // only tile roots carry a count
    int r = p;                                        // (the merge launch has finished: plain loads see its unions;
    for (int q = lab[r]; q != r; q = lab[r]) r = q;   //  the stores below only ever write a root)
    if (r == p) return;
    lab[p] = r;                                       // apply: pixel -> tile root -> root, two steps
    if (glb_ld(&siz[r]) <= a.max_size) atomicAdd(&siz[r], s);   // past max_size the exact count is not needed
}

__global__ void __launch_bounds__(256) speckle_apply_kernel(SpeckleArgs a)
{
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= a.plane) return;
    const int y = p / a.W, x = p - y * a.W;
    int16_t* row = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(a.img) + (ptrdiff_t)blockIdx.y * a.map_stride +
                                              (ptrdiff_t)y * a.stride);
    if (row[x] == a.new_val) return;
    const int* lab = a.labels + (size_t)blockIdx.y * a.plane;
    int r = p;
    for (int q = lab[r]; q != r; q = lab[r]) r = q;
    if (a.sizes[(size_t)blockIdx.y * a.plane + r] <= a.max_size) row[x] = (int16_t)a.new_val;
}

struct SpeckleCall {                   // one call as its C entry point received it
    int n; int16_t* img; ptrdiff_t stride, map_stride; int W, H;
    int new_val, max_size, max_diff;
};

int speckle_check(const SpeckleCall& c)
{
    if (!c.img || c.n < 1 || c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "filterSpeckles: the image is empty");
    if (c.new_val < -32768 || c.new_val > 32767) return fail(ADF_EBADARG, "filterSpeckles: newVal is outside the CV_16S range");
    if ((int64_t)c.W * c.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "filterSpeckles: W*H must be below 2^31 (int32 labels)");
    if ((uint64_t)c.n * (uint64_t)c.W * (uint64_t)c.H > ((uint64_t)1 << 40)) return fail(ADF_ESIZE, "filterSpeckles: batch too large");
    if (((uintptr_t)c.img & 1) || (c.stride & 1) || (c.map_stride & 1))
        return fail(ADF_EBADARG, "filterSpeckles: CV_16S image and strides must be 2-byte aligned");
    if (c.stride < (ptrdiff_t)c.W * 2) return fail(ADF_ESIZE, "filterSpeckles: row stride smaller than a row");
    if (!images_disjoint(c.n, (ptrdiff_t)c.W * 2, c.H, c.stride, c.map_stride, false))
        return fail(ADF_ESIZE, "filterSpeckles: maps of the batch overlap (map stride smaller than a map)");
    return ADF_OK;
}

// ws: adf_filter_speckles_workspace_bytes of device memory, the labels of every map and then their sizes
int speckle_run(const SpeckleCall& c, void* ws, hipStream_t st)
{
    const size_t plane = (size_t)c.W * c.H;
    SpeckleArgs a;
    a.stride = c.stride; a.map_stride = c.map_stride;
    a.W = c.W; a.H = c.H; a.tiles_x = (c.W + TW - 1) / TW; a.tiles_y = (c.H + TH - 1) / TH;
    a.new_val = c.new_val; a.max_size = c.max_size; a.max_diff = c.max_diff;
    a.plane = (int)plane;
    const int n_vert = (a.tiles_x - 1) * c.H, n_edges = n_vert + (a.tiles_y - 1) * c.W;
    const unsigned pix_blocks = (unsigned)((plane + 255) / 256);
    return for_batches(c.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.img = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(c.img) + (ptrdiff_t)m0 * c.map_stride);
        a.labels = static_cast<int*>(ws) + plane * m0;
        a.sizes = static_cast<int*>(ws) + plane * c.n + plane * m0;
        hipLaunchKernelGGL(speckle_tile_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y), nm), dim3(NT), 0, st, a);
        if (n_edges > 0)
            hipLaunchKernelGGL(speckle_merge_kernel, dim3((unsigned)((n_edges + 255) / 256), nm), dim3(256), 0, st, a, n_vert, n_edges);
        hipLaunchKernelGGL(speckle_count_kernel, dim3(pix_blocks, nm), dim3(256), 0, st, a);
        hipLaunchKernelGGL(speckle_apply_kernel, dim3(pix_blocks, nm), dim3(256), 0, st, a);
        return launched();
    });
}

} // namespace

extern "C" size_t adf_filter_speckles_workspace_bytes(int n_maps, int W, int H)
{
    if (n_maps < 1 || W < 1 || H < 1) return 0;
    return (size_t)n_maps * (size_t)W * (size_t)H * 2 * sizeof(int);
}

extern "C" int adf_filter_speckles_device(int n_maps, int16_t* img, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                                          int new_val, int max_speckle_size, int max_diff,
                                          void* workspace, size_t workspace_bytes, void* stream)
{
    const SpeckleCall c{n_maps, img, stride, map_stride, W, H, new_val, max_speckle_size, max_diff};
    int rc = speckle_check(c);
    if (rc) return rc;
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch("filterSpeckles", "adf_filter_speckles_workspace_bytes", workspace, workspace_bytes,
                              adf_filter_speckles_workspace_bytes(n_maps, W, H), (hipStream_t)stream, blk, &ws);
    return rc ? rc : speckle_run(c, ws, (hipStream_t)stream);
}

extern "C" int adf_filter_speckles_host(int n_maps, int16_t* img, ptrdiff_t stride, ptrdiff_t map_stride, int W, int H,
                                        int new_val, int max_speckle_size, int max_diff)
{
    const SpeckleCall c{n_maps, img, stride, map_stride, W, H, new_val, max_speckle_size, max_diff};
    int rc = speckle_check(c);
    if (rc) return rc;
    // one block: the maps, dense, then the workspace
    const size_t row = (size_t)W * 2, map = (size_t)H * row, maps = pad_to(map * n_maps, 256);
    Scratch blk;
    if ((rc = blk.take(maps + adf_filter_speckles_workspace_bytes(n_maps, W, H), nullptr))) return rc;
    char* dm = static_cast<char*>(blk.p);
    SpeckleCall d = c;                                               // the same call on the staged maps
    d.img = reinterpret_cast<int16_t*>(dm); d.stride = (ptrdiff_t)row; d.map_stride = (ptrdiff_t)map;
    if ((rc = copy_images(dm, row, map, img, stride, map_stride, row, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = speckle_run(d, dm + maps, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(img, stride, map_stride, dm, row, map, row, H, n_maps, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
