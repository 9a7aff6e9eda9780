// validate_kernels.hip -- calib3d's validateDisparity(disp, cost, minDisparity, numberOfDisparities, disp12MaxDiff), the
// left-right check cv::StereoBM::compute runs on its own map and on the aggregated cost of each winning disparity, on the
// device, for CV_16SC1 maps and a CV_16S or CV_32S cost plane (include/adf_wls.h, "validateDisparity", is the statement).
//
//   minD, maxD = minD + numDisparities, INV = (minD-1)*16, columns [X0, X1) = [max(maxD,0), W + min(minD,0)); per row:
//   1. disp2[x2] = INV, cost2[x2] = INT_MAX
//   2. x ascending, d = disp[x] != INV, c = cost[x]: x2 = x - ((d+8) >> 4); cost2[x2] > c  ->  (cost2, disp2)[x2] = (c, d)
//   3. d = disp[x] != INV, d0 = d >> 4, d1 = (d+15) >> 4: disp[x] = INV when BOTH x-d0 and x-d1 lie in the row, hold a
//      disp2 > INV, and that disp2 differs from d by more than 16*disp12MaxDiff
// A vote whose x2 falls outside [0, W) is dropped (calib3d indexes out of bounds there); the matcher's own maps never cast one.
//
// One workgroup per (row, map), the row on chip.  The row of disp is staged in LDS; step 2 is one LDS atomic minimum per
// voting pixel on a packed key per x2 -- the cost, biased to unsigned, in the high half and x in the low half (32-bit keys
// for CV_16S costs, 64-bit keys for CV_32S) -- so the smallest key is the smallest cost and among equal costs the smallest
// x: the sequential rule's strict `>` with x ascending.  The empty key, all ones, is above every vote: x stays below
// MAX_WIDTH < 65535, and a CV_32S cost of INT_MAX (biased: all ones in the high half) never votes, as it never wins the
// sequential rule.  After a barrier disp2[x2] is the staged disp at the key's x.  A minimum does not depend on the order of
// its operands, no workgroup reads what another writes, nothing is atomic in global memory: the result is bit-exact
// against the sequential statement and identical from run to run.
//
// Every thread takes four adjacent columns at a time -- one 8-byte load of the map, one 8- or 16-byte load of the cost, one
// 8-byte store of a chunk in which a pixel was invalidated -- when the rows are aligned to that, column by column otherwise;
// four such chunks' loads are in flight per thread, the first costs' while the row is staged.
//
// LDS: (key + int16) per column = 6 B (CV_16S) or 10 B (CV_32S).  A CU has 160 KiB; a workgroup may take 150 KiB of it as
// dynamic LDS (allowed per function above the default), which is MAX_WIDTH = 15360 columns of 10 B.  Memory traffic is
// 2 + sizeof(cost) bytes read per pixel and 2 written for each invalidated one.
#include "adf_host.h"

#include <climits>

using namespace adf;

namespace {

constexpr int NT = 256;
constexpr int MAX_WIDTH = ADF_VALIDATE_MAX_WIDTH;
static_assert((size_t)MAX_WIDTH * 10 <= 150 * 1024 && MAX_WIDTH < 65535, "row does not fit LDS / the key's x field");

struct ValidateArgs {
    int16_t* disp; ptrdiff_t stride, map_stride;                 // bytes
    const void* cost; ptrdiff_t cost_stride, cost_map_stride;    // bytes
    int W, X0, X1, inv, tol;                                     // tol = 16 * disp12MaxDiff
};

// The packed vote of one cost type: KEY, its empty value, and whether a cost may vote at all.
template <class COST> struct Vote;
template <> struct Vote<int16_t> {
    using KEY = uint32_t;
    static constexpr KEY EMPTY = 0xFFFFFFFFu;
    static __device__ __forceinline__ bool votes(int) { return true; }
    static __device__ __forceinline__ KEY pack(int c, int x) { return ((uint32_t)(c + 32768) << 16) | (uint32_t)x; }
    static __device__ __forceinline__ int x_of(KEY k) { return (int)(k & 0xFFFFu); }
};
template <> struct Vote<int32_t> {
    using KEY = unsigned long long;
    static constexpr KEY EMPTY = ~0ull;
    static __device__ __forceinline__ bool votes(int c) { return c != INT_MAX; }    // cost2 starts at INT_MAX and the test is strict
    static __device__ __forceinline__ KEY pack(int c, int x) { return ((KEY)((uint32_t)c ^ 0x80000000u) << 32) | (uint32_t)x; }
    static __device__ __forceinline__ int x_of(KEY k) { return (int)(uint32_t)k; }
};

// Four adjacent columns as one access: global rows when they are aligned to it (`vec`, uniform over the workgroup), the
// staged row always (its LDS base is 16-byte aligned and chunks start at multiples of four columns).
template <class T> using Quad = T __attribute__((ext_vector_type(4)));    // (a register value: never an array in scratch)
constexpr int CH = 4, PASS = CH * NT;     // columns per chunk; columns the workgroup covers with one chunk per thread
constexpr int UN = 4;                     // chunks whose loads a thread has in flight

constexpr size_t lds_keys(int W, size_t key_bytes) { return ((size_t)W * key_bytes + 15) / 16 * 16; }

template <class COST>
__global__ void __launch_bounds__(NT) validate_kernel(ValidateArgs a)
{
    using V = Vote<COST>;
    using KEY = typename V::KEY;
    extern __shared__ __align__(16) unsigned char smem[];
    KEY* key = reinterpret_cast<KEY*>(smem);                                          // [W]
    int16_t* sd = reinterpret_cast<int16_t*>(smem + lds_keys(a.W, sizeof(KEY)));      // [W] the row as it came in
    const int t = threadIdx.x, W = a.W;
    int16_t* drow = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(a.disp) + (ptrdiff_t)blockIdx.y * a.map_stride +
                                               (ptrdiff_t)blockIdx.x * a.stride);
    const COST* crow = reinterpret_cast<const COST*>(reinterpret_cast<const char*>(a.cost) + (ptrdiff_t)blockIdx.y * a.cost_map_stride +
                                                     (ptrdiff_t)blockIdx.x * a.cost_stride);
    const bool vec = (reinterpret_cast<uintptr_t>(drow) & (sizeof(Quad<int16_t>) - 1)) == 0 &&
                     (reinterpret_cast<uintptr_t>(crow) & (sizeof(Quad<COST>) - 1)) == 0;
    // columns x .. x+3 of a global row (x a multiple of four); columns past the row read as `past`
    auto load4 = [&](const auto* row, int x, auto past) {
        using T = decltype(past);
        Quad<T> q;
        if (vec && x + CH <= W) return *reinterpret_cast<const Quad<T>*>(row + x);
#pragma unroll
        for (int i = 0; i < CH; i++) q[i] = x + i < W ? row[x + i] : past;
        return q;
    };
    auto staged4 = [&](int x) {
        Quad<int16_t> q;
        if (x + CH <= W) return *reinterpret_cast<const Quad<int16_t>*>(sd + x);
#pragma unroll
        for (int i = 0; i < CH; i++) q[i] = x + i < W ? sd[x + i] : (int16_t)a.inv;
        return q;
    };
    // A thread issues the loads of its next UN chunks, PASS columns apart, before it uses the first: one chunk per thread in
    // flight is 2 KB per workgroup, too little to cover the latency of HBM.  The costs of the first UN chunks of step 2
    // are requested before the row is staged, so they travel meanwhile; a 3840-column row has no more.
    const int xa = a.X0 & ~(CH - 1);                              // chunks start at multiples of four columns
    auto load_costs = [&](int x0, Quad<COST> (&c)[UN]) {
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int x = x0 + u * PASS;
            c[u] = x < a.X1 ? load4(crow, x, (COST)0) : Quad<COST>((COST)0);
        }
    };
    Quad<COST> c[UN];
    load_costs(xa + CH * t, c);
    for (int x0 = CH * t; x0 < W; x0 += UN * PASS) {              // step 1: stage the row, empty the votes
        Quad<int16_t> d[UN];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int x = x0 + u * PASS;
            d[u] = x < W ? load4(drow, x, (int16_t)a.inv) : Quad<int16_t>((int16_t)a.inv);
        }
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int x = x0 + u * PASS;
            if (x >= W) continue;
            if (x + CH <= W) *reinterpret_cast<Quad<int16_t>*>(sd + x) = d[u];
#pragma unroll
            for (int i = 0; i < CH; i++) {
                if (x + i >= W) break;
                if (x + CH > W) sd[x + i] = d[u][i];
                key[x + i] = V::EMPTY;
            }
        }
    }
    __syncthreads();
    for (int x0 = xa + CH * t; x0 < a.X1; x0 += UN * PASS) {      // step 2: every pixel votes on its x2
        if (x0 != xa + CH * t) load_costs(x0, c);
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int x = x0 + u * PASS;
            if (x >= a.X1) continue;
            const Quad<int16_t> d = staged4(x);
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const int xi = x + i, di = d[i], ci = c[u][i];
                if (xi < a.X0 || xi >= a.X1 || di == a.inv) continue;
                const int x2 = xi - ((di + 8) >> 4);
                if (x2 < 0 || x2 >= W || !V::votes(ci)) continue;
                atomicMin(&key[x2], V::pack(ci, xi));
            }
        }
    }
    __syncthreads();
    for (int x = xa + CH * t; x < a.X1; x += CH * NT) {           // step 3
        const Quad<int16_t> d = staged4(x);
        Quad<int16_t> o = d;
        bool any = false;
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int xi = x + i, di = d[i];
            if (xi < a.X0 || xi >= a.X1 || di == a.inv) continue;
            auto contradicts = [&](int xc) {                      // the candidate holds a disparity that disagrees with di
                if (xc < 0 || xc >= W) return false;
                const KEY k = key[xc];
                if (k == V::EMPTY) return false;
                const int d2 = sd[V::x_of(k)];
                return d2 > a.inv && abs(d2 - di) > a.tol;
            };
            if (contradicts(xi - (di >> 4)) && contradicts(xi - ((di + 15) >> 4))) { o[i] = (int16_t)a.inv; any = true; }
        }
        if (!any) continue;
        // the chunk is this thread's alone and every read of the row has been served from LDS since the first barrier:
        // its unchanged columns go back as they came
        if (vec && x + CH <= W) *reinterpret_cast<Quad<int16_t>*>(drow + x) = o;
        else {
#pragma unroll
            for (int i = 0; i < CH; i++)
                if (o[i] != d[i]) drow[x + i] = o[i];
        }
    }
}

struct ValidateCall {                  // one call as its C entry point received it
    int n; int16_t* disp; ptrdiff_t stride, map_stride;
    const void* cost; ptrdiff_t cost_stride, cost_map_stride; int cost_type;
    int W, H, min_disp, num_disp, max_diff;
};

size_t cost_size(int cost_type) { return cost_type == ADF_32S ? 4 : 2; }

int validate_check(const ValidateCall& c)
{
    if (!c.disp || !c.cost) return fail(ADF_EBADARG, "validateDisparity: disp and cost must be non-NULL");
    if (c.n < 1 || c.W < 1 || c.H < 1) return fail(ADF_EBADARG, "validateDisparity: the map is empty");
    if (c.cost_type != ADF_16S && c.cost_type != ADF_32S)
        return fail(ADF_EBADARG, "validateDisparity: cost must be CV_16S (ADF_16S) or CV_32S (ADF_32S)");
    if (c.max_diff < 0) return fail(ADF_EBADARG, "validateDisparity: disp12MaxDiff must not be negative (a switched-off check is the caller's not to call)");
    if (c.max_diff > (1 << 26)) return fail(ADF_EBADARG, "validateDisparity: disp12MaxDiff must not exceed 2^26");
    if (c.num_disp <= 0) return fail(ADF_EBADARG, "validateDisparity: numberOfDisparities must be positive");
    const int64_t inv = ((int64_t)c.min_disp - 1) * 16;
    if (inv < -32768 || inv > 32767 || (int64_t)c.min_disp + c.num_disp > INT_MAX)
        return fail(ADF_EBADARG, "validateDisparity: (minDisparity-1)*16 is outside the CV_16S range");
    if (c.W > MAX_WIDTH) return fail(ADF_ESIZE, "validateDisparity: maps wider than %d columns are not supported (a row is held in LDS)", MAX_WIDTH);
    const ptrdiff_t cs = (ptrdiff_t)cost_size(c.cost_type);
    if (((uintptr_t)c.disp & 1) || (c.stride & 1) || (c.map_stride & 1))
        return fail(ADF_EBADARG, "validateDisparity: CV_16S map and strides must be 2-byte aligned");
    if (((uintptr_t)c.cost & (cs - 1)) || (c.cost_stride & (cs - 1)) || (c.cost_map_stride & (cs - 1)))
        return fail(ADF_EBADARG, "validateDisparity: cost plane and strides must be aligned to the cost type");
    if (c.stride < (ptrdiff_t)c.W * 2 || c.cost_stride < (ptrdiff_t)c.W * cs) return fail(ADF_ESIZE, "validateDisparity: row stride smaller than a row");
    if (!images_disjoint(c.n, (ptrdiff_t)c.W * 2, c.H, c.stride, c.map_stride, false))
        return fail(ADF_ESIZE, "validateDisparity: maps of the batch overlap (map stride smaller than a map)");
    return ADF_OK;
}

template <class COST>
int validate_launch(const ValidateCall& c, ValidateArgs a, hipStream_t st)
{
    const size_t lds = lds_keys(c.W, sizeof(typename Vote<COST>::KEY)) + (size_t)c.W * sizeof(int16_t);
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(validate_kernel<COST>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return for_batches(c.n, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.disp = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(c.disp) + (ptrdiff_t)m0 * c.map_stride);
        a.cost = reinterpret_cast<const char*>(c.cost) + (ptrdiff_t)m0 * c.cost_map_stride;
        hipLaunchKernelGGL(validate_kernel<COST>, dim3((unsigned)c.H, nm), dim3(NT), lds, st, a);
        return launched();
    });
}

int validate_run(const ValidateCall& c, hipStream_t st)
{
    ValidateArgs a;
    a.stride = c.stride; a.map_stride = c.map_stride; a.cost_stride = c.cost_stride; a.cost_map_stride = c.cost_map_stride;
    const int maxD = c.min_disp + c.num_disp;
    a.W = c.W; a.inv = (c.min_disp - 1) * 16; a.tol = 16 * c.max_diff;
    a.X0 = maxD > 0 ? maxD : 0;
    a.X1 = c.W + (c.min_disp < 0 ? c.min_disp : 0);
    if (a.X0 >= a.X1) return ADF_OK;                              // no column has a full search range: nothing to test
    return c.cost_type == ADF_32S ? validate_launch<int32_t>(c, a, st) : validate_launch<int16_t>(c, a, st);
}

} // namespace

extern "C" int adf_validate_disparity_device(int n_maps, int16_t* disp, ptrdiff_t stride, ptrdiff_t map_stride,
                                             const void* cost, ptrdiff_t cost_stride, ptrdiff_t cost_map_stride, int cost_type,
                                             int W, int H, int min_disparity, int num_disparities, int disp12_max_diff, void* stream)
{
    const ValidateCall c{n_maps, disp, stride, map_stride, cost, cost_stride, cost_map_stride, cost_type, W, H,
                         min_disparity, num_disparities, disp12_max_diff};
    int rc = validate_check(c);
    return rc ? rc : validate_run(c, (hipStream_t)stream);
}

extern "C" int adf_validate_disparity_host(int n_maps, int16_t* disp, ptrdiff_t stride, ptrdiff_t map_stride,
                                           const void* cost, ptrdiff_t cost_stride, ptrdiff_t cost_map_stride, int cost_type,
                                           int W, int H, int min_disparity, int num_disparities, int disp12_max_diff)
{
    const ValidateCall c{n_maps, disp, stride, map_stride, cost, cost_stride, cost_map_stride, cost_type, W, H,
                         min_disparity, num_disparities, disp12_max_diff};
    int rc = validate_check(c);
    if (rc) return rc;
    // one block: the maps, dense, then the cost planes
    const size_t drow = (size_t)W * 2, dmap = (size_t)H * drow, maps = pad_to(dmap * n_maps, 256);
    const size_t crow = (size_t)W * cost_size(cost_type), cmap = (size_t)H * crow;
    Scratch blk;
    if ((rc = blk.take(maps + cmap * n_maps, nullptr))) return rc;
    char* dm = static_cast<char*>(blk.p);
    ValidateCall d = c;                                              // the same call on the staged images
    d.disp = reinterpret_cast<int16_t*>(dm); d.stride = (ptrdiff_t)drow; d.map_stride = (ptrdiff_t)dmap;
    d.cost = dm + maps; d.cost_stride = (ptrdiff_t)crow; d.cost_map_stride = (ptrdiff_t)cmap;
    if ((rc = copy_images(dm, drow, dmap, disp, stride, map_stride, drow, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = copy_images(dm + maps, crow, cmap, cost, cost_stride, cost_map_stride, crow, H, n_maps, hipMemcpyHostToDevice, nullptr))) return rc;
    if ((rc = validate_run(d, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = copy_images(disp, stride, map_stride, dm, drow, dmap, drow, H, n_maps, hipMemcpyDeviceToHost, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}
