// am_filter_kernels.hip -- cv::ximgproc::amFilter(joint, src, dst, sigma_s, sigma_r, adjust_outliers) (Gastal & Oliveira's
// adaptive manifolds) on the device, in the library's own definition (include/adf_wls.h, "adaptive manifold filter", is
// the statement; tests/am_ref.py states it in NumPy).  A complete binary tree of 2^height - 1 manifolds is visited in
// pre-order; every node weighs the pixels by their distance to its manifold eta (w), splats src * w and w to the small
// plane (1/df of the map), blurs both there with one recursive sweep whose feedback follows eta, slices them back
// (num += up(psi) w, den += up(psi0) w) and, above the leaves, splits its cluster by the sign of the first principal
// direction of J - eta and forms both children's manifolds.  The result is num / den.
//
// One chain of launches on the caller's stream, nothing synchronised and nothing allocated when a workspace is given:
//   per node      am_splat_kernel (w, f w and w at the taps down() reads -> psi, psi0), am_feedback_kernel (ah, av),
//                 am_row_sweep_kernel + am_col_sweep_kernel (psi and psi0 in one launch each), am_slice_kernel (num, den,
//                 the outliers' minimum distance)
//   per split     am_pca_kernel (three joint channels: the sums as exact 64-bit integers, one atomic per workgroup and
//                 channel), am_split_kernel (the cluster bit of every pixel), am_children_kernel (both children's tm and
//                 tm J_c at small size), the two sweeps over those 2 (1 + channels) planes, am_divide_kernel
//   per call      am_root_kernel + the two sweeps at full size + am_down_kernel (the root manifold), am_finish_kernel
// 5 launches per node, 5 (gray joint) or 6 (BGR) per split, 5 per call: 55 at height 3 with a gray joint, 58 and a memset
// of the PCA sums with a BGR one.
//
// Only the root manifold is ever a full-size plane: below it etaF = up(eta) is evaluated from the small planes wherever
// it is read (the same function, the same bits), J is Jtab of the joint's bytes (a 256-entry LDS table per workgroup)
// and a pixel's clusters are the bits of one byte.  The sweeps: a row sweep workgroup is one wave that owns 16 rows and
// walks 64-column tiles through LDS (pitch 65: the tile is loaded and stored with consecutive lanes on consecutive
// addresses, all its loads in flight together; the chain runs with one lane per row); a column sweep lane owns one
// column and loads eight rows ahead of the chain.  Times and what bounds them: DESIGN.md, section 27.
#include "dt_common.h"

#include <cstring>

#pragma clang fp contract(off)

using namespace adf;

namespace {

// exp(x) for x <= 0 from float32 operations alone, so that the host, the device and the NumPy statement agree bit for
// bit: x = (n + f) ln 2 with n the nearest integer, 2^f = exp(f ln 2) by its Taylor polynomial of degree 7 in Horner
// form (multiply, then add; c_k = (float)(ln2^k / k!)), times 2^n built from bits.  0 where n < -126 or x is a NaN.
__host__ __device__ inline float am_exp(float x)
{
    const float t = x * 0x1.715476p+0f;
    const float n = floorf(t + 0.5f);
    if (!(n >= -126.0f)) return 0.0f;
    const float f = t - n;
    float p = 0x1.ffcbfcp-17f;
    p = p * f + 0x1.430912p-13f;
    p = p * f + 0x1.5d87fep-10f;
    p = p * f + 0x1.3b2ab6p-7f;
    p = p * f + 0x1.c6b08ep-5f;
    p = p * f + 0x1.ebfbep-3f;
    p = p * f + 0x1.62e43p-1f;
    p = p * f + 1.0f;
    const uint32_t bits = (uint32_t)((int)n + 127) << 23;
    float e;
    memcpy(&e, &bits, sizeof e);
    return p * e;
}

__host__ __device__ inline float div0(float a, float b) { return b == 0.0f ? 0.0f : a / b; }   // cv::divide's rule

constexpr int NT = 256;                // threads of a pointwise workgroup (and the entries of the joint table)
constexpr int ST = 64;                 // a sweep workgroup: one wave; the columns of a row sweep's tile and of a column sweep
constexpr int SR = 16;                 // rows of a row sweep's tile
constexpr int SB = 8;                  // rows a column sweep loads ahead of its chain

struct AmArgs {
    const uint8_t* joint; ptrdiff_t joint_stride, joint_map_stride;      // bytes
    const char* src; ptrdiff_t src_stride, src_map_stride;
    char* dst; ptrdiff_t dst_stride, dst_map_stride;
    int W, H, sw, sh;
    double down_scale, up_x, up_y;                                       // df; sw / W; sh / H
    float argW, ratio, lnA, argOut;
    int adjust;
    float* ws; size_t per_map;                                           // map m's block of the workspace: ws + m * per_map floats
    size_t num, den, mind, etaF, path, psi, fb;                          // planes of a block, in floats from its start
    long long* acc; int nodes;                                           // the PCA sums: [map][node][channel]
    size_t eta, child;                                                   // the node's small manifold planes; its children's slot
    int level, code, first, node;                                        // (first: the node opens num, den and mind)
    int m0;                                                              // the first map of the launch
};

// A tap pair of cv::resize INTER_LINEAR (resize_kernels.hip's header): along a row a tap that would leave it has the
// weights (1, 0); along a column the rows are clamped and the weights stay.
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap tap_x(int d, double scale, int n)
{
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(fx);
    fx -= (float)s;
    if (s < 0) { fx = 0.0f; s = 0; }
    if (s >= n - 1) { fx = 0.0f; s = n - 1; }
    return Tap{s, min(s + 1, n - 1), 1.0f - fx, fx};
}
__device__ __forceinline__ Tap tap_y(int d, double scale, int n)
{
    float fy = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)floorf(fy);
    fy -= (float)s;
    return Tap{min(max(s, 0), n - 1), min(max(s + 1, 0), n - 1), 1.0f - fy, fy};
}
// Row blend first, then column blend: v[row tap][column tap].
__device__ __forceinline__ float blend(const float (&v)[2][2], const Tap& tx, const Tap& ty)
{
    const float r0 = v[0][0] * tx.w0 + v[0][1] * tx.w1, r1 = v[1][0] * tx.w0 + v[1][1] * tx.w1;
    return r0 * ty.w0 + r1 * ty.w1;
}
__device__ __forceinline__ float bilerp(const float* p, int pitch, const Tap& tx, const Tap& ty)
{
    const float* r0 = p + (size_t)ty.i0 * pitch;
    const float* r1 = p + (size_t)ty.i1 * pitch;
    const float v[2][2] = {{r0[tx.i0], r0[tx.i1]}, {r1[tx.i0], r1[tx.i1]}};
    return blend(v, tx, ty);
}

__device__ __forceinline__ void joint_table(float* jtab)                // Jtab[v] = (float)(v / 255.0), by all NT threads
{
    jtab[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
    __syncthreads();
}
__device__ __forceinline__ float* block_of(const AmArgs& a) { return a.ws + (size_t)(a.m0 + (int)blockIdx.y) * a.per_map; }
__device__ __forceinline__ const uint8_t* joint_of(const AmArgs& a) { return a.joint + (ptrdiff_t)(a.m0 + (int)blockIdx.y) * a.joint_map_stride; }

// Pixel (x, y): J_c and etaF_c -- the root's plane, or up(eta) from the node's small planes.
template <int CH, bool ROOT>
__device__ __forceinline__ void pixel_at(const AmArgs& a, const float* blk, const uint8_t* joint, const float* jtab, int x, int y,
                                         float (&J)[CH], float (&E)[CH])
{
    const uint8_t* g = joint + (ptrdiff_t)y * a.joint_stride + (ptrdiff_t)x * CH;
    const size_t WH = (size_t)a.W * a.H, S = (size_t)a.sw * a.sh;
    Tap ux{}, uy{};
    if (!ROOT) { ux = tap_x(x, a.up_x, a.sw); uy = tap_y(y, a.up_y, a.sh); }
#pragma unroll
    for (int c = 0; c < CH; c++) {
        J[c] = jtab[g[c]];
        E[c] = ROOT ? blk[a.etaF + c * WH + (size_t)y * a.W + x] : bilerp(blk + a.eta + c * S, a.sw, ux, uy);
    }
}
template <int CH> __device__ __forceinline__ float dist2(const float (&J)[CH], const float (&E)[CH])
{
    float d2 = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const float e = E[c] - J[c], q = e * e;
        d2 = c == 0 ? q : d2 + q;
    }
    return d2;
}
__device__ __forceinline__ bool in_cluster(const AmArgs& a, unsigned path) { return (path & ((1u << (a.level - 1)) - 1u)) == (unsigned)a.code; }

// The root manifold before its blur: etaF_c = J_c at full size.
template <int CH> __global__ void __launch_bounds__(NT) am_root_kernel(AmArgs a)
{
    __shared__ float jtab[NT];
    joint_table(jtab);
    const size_t WH = (size_t)a.W * a.H, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= WH) return;
    const int x = (int)(i % a.W), y = (int)(i / a.W);
    const uint8_t* g = joint_of(a) + (ptrdiff_t)y * a.joint_stride + (ptrdiff_t)x * CH;
    float* blk = block_of(a);
#pragma unroll
    for (int c = 0; c < CH; c++) blk[a.etaF + c * WH + i] = jtab[g[c]];
}

// eta = down(etaF) of the root.
template <int CH> __global__ void __launch_bounds__(NT) am_down_kernel(AmArgs a)
{
    const size_t WH = (size_t)a.W * a.H, S = (size_t)a.sw * a.sh, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= S) return;
    float* blk = block_of(a);
    const Tap tx = tap_x((int)(i % a.sw), a.down_scale, a.W), ty = tap_y((int)(i / a.sw), a.down_scale, a.H);
#pragma unroll
    for (int c = 0; c < CH; c++) blk[a.eta + c * S + i] = bilerp(blk + a.etaF + c * WH, a.W, tx, ty);
}

// psi = down(f w), psi0 = down(w): w and f w at the four pixels down() reads.
template <int CH, bool ROOT, class SrcT> __global__ void __launch_bounds__(NT) am_splat_kernel(AmArgs a)
{
    __shared__ float jtab[NT];
    joint_table(jtab);
    const size_t S = (size_t)a.sw * a.sh, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= S) return;
    float* blk = block_of(a);
    const uint8_t* joint = joint_of(a);
    const char* src = a.src + (ptrdiff_t)(a.m0 + (int)blockIdx.y) * a.src_map_stride;
    const Tap tx = tap_x((int)(i % a.sw), a.down_scale, a.W), ty = tap_y((int)(i / a.sw), a.down_scale, a.H);
    float fw[2][2], ww[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int x = q ? tx.i1 : tx.i0, y = r ? ty.i1 : ty.i0;
            float J[CH], E[CH];
            pixel_at<CH, ROOT>(a, blk, joint, jtab, x, y, J, E);
            const float w = am_exp(dist2<CH>(J, E) * a.argW);
            const float f = (float)reinterpret_cast<const SrcT*>(src + (ptrdiff_t)y * a.src_stride)[x];
            fw[r][q] = f * w;
            ww[r][q] = w;
        }
    blk[a.psi + i] = blend(fw, tx, ty);
    blk[a.psi + S + i] = blend(ww, tx, ty);
}

// The sweeps' feedback at small size: ah between a pixel and its right neighbour, av between it and the one below.
template <int CH> __global__ void __launch_bounds__(NT) am_feedback_kernel(AmArgs a)
{
    const size_t S = (size_t)a.sw * a.sh, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= S) return;
    float* blk = block_of(a);
    const int x = (int)(i % a.sw), y = (int)(i / a.sw);
    const bool h = x + 1 < a.sw, v = y + 1 < a.sh;
    float dh = 0.0f, dv = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const float* e = blk + a.eta + c * S + i;
        const float eh = e[0] - e[h ? 1 : 0], ev = e[0] - e[v ? a.sw : 0];
        dh = c == 0 ? eh * eh : dh + eh * eh;
        dv = c == 0 ? ev * ev : dv + ev * ev;
    }
    if (h) blk[a.fb + i] = am_exp(sqrtf(dh * a.ratio + 1.0f) * a.lnA);
    if (v) blk[a.fb + S + i] = am_exp(sqrtf(dv * a.ratio + 1.0f) * a.lnA);
}

// num += up(psi) w, den += up(psi0) w; the outliers' mind = min(mind, d2).
template <int CH, bool ROOT> __global__ void __launch_bounds__(NT) am_slice_kernel(AmArgs a)
{
    __shared__ float jtab[NT];
    joint_table(jtab);
    const size_t WH = (size_t)a.W * a.H, S = (size_t)a.sw * a.sh, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= WH) return;
    float* blk = block_of(a);
    const int x = (int)(i % a.W), y = (int)(i / a.W);
    float J[CH], E[CH];
    pixel_at<CH, ROOT>(a, blk, joint_of(a), jtab, x, y, J, E);
    const float d2 = dist2<CH>(J, E), w = am_exp(d2 * a.argW);
    const Tap ux = tap_x(x, a.up_x, a.sw), uy = tap_y(y, a.up_y, a.sh);
    const float u = bilerp(blk + a.psi, a.sw, ux, uy), u0 = bilerp(blk + a.psi + S, a.sw, ux, uy);
    const float n0 = a.first ? 0.0f : blk[a.num + i], d0 = a.first ? 0.0f : blk[a.den + i];
    blk[a.num + i] = n0 + u * w;
    blk[a.den + i] = d0 + u0 * w;
    if (a.adjust) blk[a.mind + i] = a.first ? d2 : fminf(blk[a.mind + i], d2);
}

// Three joint channels: s_c = sum over the cluster of m X_c, m = 0.5 X_0 - 0.5 X_1 + 0.5 X_2, every float32 product scaled
// by 2^30 and rounded to an integer: the sum is exact, whatever the order.
template <bool ROOT> __global__ void __launch_bounds__(NT) am_pca_kernel(AmArgs a)
{
    __shared__ float jtab[NT];
    __shared__ long long part[3][NT / 64];
    joint_table(jtab);
    const size_t WH = (size_t)a.W * a.H, i = (size_t)blockIdx.x * NT + threadIdx.x;
    const float* blk = block_of(a);
    long long q[3] = {0, 0, 0};
    if (i < WH && (ROOT || in_cluster(a, reinterpret_cast<const uint8_t*>(blk + a.path)[i]))) {
        float J[3], E[3], X[3];
        pixel_at<3, ROOT>(a, blk, joint_of(a), jtab, (int)(i % a.W), (int)(i / a.W), J, E);
#pragma unroll
        for (int c = 0; c < 3; c++) X[c] = J[c] - E[c];
        float m = 0.5f * X[0];
        m = m + -0.5f * X[1];
        m = m + 0.5f * X[2];
#pragma unroll
        for (int c = 0; c < 3; c++) q[c] = (long long)rintf((m * X[c]) * 0x1p+30f);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        for (int o = 32; o > 0; o >>= 1) q[c] += __shfl_down(q[c], o, 64);
        if (threadIdx.x % 64 == 0) part[c][threadIdx.x / 64] = q[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long s = 0;
        for (int k = 0; k < NT / 64; k++) s += part[threadIdx.x][k];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(a.acc + ((size_t)(a.m0 + (int)blockIdx.y) * a.nodes + a.node) * 3 + threadIdx.x),
                         (unsigned long long)s);
    }
}

// A pixel of the cluster goes to the minus child (o < 0) or to the plus child: bit level - 1 of its path byte.
template <int CH, bool ROOT> __global__ void __launch_bounds__(NT) am_split_kernel(AmArgs a)
{
    __shared__ float jtab[NT];
    __shared__ float vec[3];
    if (CH == 3 && threadIdx.x == 0) {                                   // vec = (float)(s / |s|) in double, 0 if |s| = 0
        const long long* s = a.acc + ((size_t)(a.m0 + (int)blockIdx.y) * a.nodes + a.node) * 3;
        const double s0 = (double)s[0] * 0x1p-30, s1 = (double)s[1] * 0x1p-30, s2 = (double)s[2] * 0x1p-30;
        const double norm = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
        vec[0] = norm != 0.0 ? (float)(s0 / norm) : 0.0f;
        vec[1] = norm != 0.0 ? (float)(s1 / norm) : 0.0f;
        vec[2] = norm != 0.0 ? (float)(s2 / norm) : 0.0f;
    }
    joint_table(jtab);
    const size_t WH = (size_t)a.W * a.H, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= WH) return;
    float* blk = block_of(a);
    uint8_t* path = reinterpret_cast<uint8_t*>(blk + a.path) + i;
    const unsigned before = ROOT ? 0u : *path;
    if (!ROOT && !in_cluster(a, before)) return;
    float J[CH], E[CH];
    pixel_at<CH, ROOT>(a, blk, joint_of(a), jtab, (int)(i % a.W), (int)(i / a.W), J, E);
    float o = J[0] - E[0];
    if constexpr (CH == 3) {
        o = vec[0] * o;
        o = o + vec[1] * (J[1] - E[1]);
        o = o + vec[2] * (J[2] - E[2]);
    }
    *path = (uint8_t)((unsigned)a.code | (o >= 0.0f ? 1u << (a.level - 1) : 0u));
}

// Both children at small size: tb = down(tm), eta_c = down(tm J_c), tm = 1 - w inside the child's cluster and 0 outside.
// The slot holds [child][tb, eta_0 .. eta_{CH-1}] planes.
template <int CH, bool ROOT> __global__ void __launch_bounds__(NT) am_children_kernel(AmArgs a)
{
    __shared__ float jtab[NT];
    joint_table(jtab);
    const size_t S = (size_t)a.sw * a.sh, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= S) return;
    float* blk = block_of(a);
    const uint8_t* joint = joint_of(a);
    const uint8_t* path = reinterpret_cast<const uint8_t*>(blk + a.path);
    const Tap tx = tap_x((int)(i % a.sw), a.down_scale, a.W), ty = tap_y((int)(i / a.sw), a.down_scale, a.H);
    float tm[2][2][2], tj[2][CH][2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int x = q ? tx.i1 : tx.i0, y = r ? ty.i1 : ty.i0;
            float J[CH], E[CH];
            pixel_at<CH, ROOT>(a, blk, joint, jtab, x, y, J, E);
            const float t = 1.0f - am_exp(dist2<CH>(J, E) * a.argW);
            const unsigned p = path[(size_t)y * a.W + x];
            const bool member = in_cluster(a, p), plus = p >> (a.level - 1) & 1u;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const float v = member && plus == (k == 1) ? t : 0.0f;
                tm[k][r][q] = v;
#pragma unroll
                for (int c = 0; c < CH; c++) tj[k][c][r][q] = v * J[c];
            }
        }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        float* slot = blk + a.child + (size_t)k * (1 + CH) * S + i;
        slot[0] = blend(tm[k], tx, ty);
#pragma unroll
        for (int c = 0; c < CH; c++) slot[(size_t)(1 + c) * S] = blend(tj[k][c], tx, ty);
    }
}

// eta_c = eta_c / tb of both children, after their blur.
template <int CH> __global__ void __launch_bounds__(NT) am_divide_kernel(AmArgs a)
{
    const size_t S = (size_t)a.sw * a.sh, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= S) return;
    float* blk = block_of(a);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        float* slot = blk + a.child + (size_t)k * (1 + CH) * S + i;
        const float tb = slot[0];
#pragma unroll
        for (int c = 0; c < CH; c++) slot[(size_t)(1 + c) * S] = div0(slot[(size_t)(1 + c) * S], tb);
    }
}

// dst = num / den, pulled back to src where the pixel is far from every manifold.
template <class SrcT, class OutT> __global__ void __launch_bounds__(NT) am_finish_kernel(AmArgs a)
{
    const size_t WH = (size_t)a.W * a.H, i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= WH) return;
    const float* blk = block_of(a);
    const int x = (int)(i % a.W), y = (int)(i / a.W);
    const ptrdiff_t m = a.m0 + (int)blockIdx.y;
    float g = div0(blk[a.num + i], blk[a.den + i]);
    if (a.adjust) {
        const float f = (float)reinterpret_cast<const SrcT*>(a.src + m * a.src_map_stride + (ptrdiff_t)y * a.src_stride)[x];
        const float alpha = am_exp(blk[a.mind + i] * a.argOut);
        g = alpha * (g - f) + f;
    }
    reinterpret_cast<OutT*>(a.dst + m * a.dst_map_stride + (ptrdiff_t)y * a.dst_stride)[x] = convert<OutT>(g);
}

// sweep(P, ah, av) of `planes` planes that share one feedback -- the plane fb, or the constant a where fb is null --, in
// place: the rows here, the columns below.
struct SweepArgs {
    float* base; size_t plane_stride, map_stride;                        // floats
    const float* fb; size_t fb_map_stride;
    float a;
    int w, h;                                                            // (the planes and fb are dense: pitch w)
    int m0;
};

__global__ void __launch_bounds__(ST) am_row_sweep_kernel(SweepArgs s)
{
    __shared__ float xt[SR * (ST + 1)], ft[SR * (ST + 1)];               // [row][column], odd pitch
    const int lane = threadIdx.x, r0 = blockIdx.x * SR, w = s.w, h = s.h, row = r0 + lane;
    const size_t m = (size_t)(s.m0 + (int)blockIdx.z);
    float* P = s.base + blockIdx.y * s.plane_stride + m * s.map_stride;
    const float* F = s.fb ? s.fb + m * s.fb_map_stride : nullptr;
    const int tiles = (w + ST - 1) / ST;
    float carry = 0.0f;
    for (int pass = 0; pass < 2; pass++) {                               // left to right, then right to left
        for (int t = 0; t < tiles; t++) {
            const int c0 = (pass ? tiles - 1 - t : t) * ST;
            // x[j] pairs with ah[j - 1] on the way right and with ah[j] on the way left
            const int cx = min(c0 + lane, w - 1), cf = pass ? cx : max(cx - 1, 0);
            float xv[SR], fv[SR];
#pragma unroll
            for (int r = 0; r < SR; r++) {                               // every load of the tile is in flight together
                const size_t at = (size_t)min(r0 + r, h - 1) * w;
                xv[r] = P[at + cx];
                fv[r] = F ? F[at + cf] : s.a;
            }
#pragma unroll
            for (int r = 0; r < SR; r++) {
                xt[r * (ST + 1) + lane] = xv[r];
                ft[r * (ST + 1) + lane] = fv[r];
            }
            __syncthreads();
            if (lane < SR && row < h) {
                for (int k0 = 0; k0 < ST; k0++) {
                    const int k = pass ? ST - 1 - k0 : k0, j = c0 + k;
                    if (j >= w) continue;
                    float x = xt[lane * (ST + 1) + k];
                    const float f = ft[lane * (ST + 1) + k];
                    if (pass ? j < w - 1 : j > 0) x = x + f * (carry - x);
                    xt[lane * (ST + 1) + k] = x;
                    carry = x;
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < SR; r++)
                if (r0 + r < h && c0 + lane < w) P[(size_t)(r0 + r) * w + c0 + lane] = xt[r * (ST + 1) + lane];
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(ST) am_col_sweep_kernel(SweepArgs s)
{
    const int col = blockIdx.x * ST + threadIdx.x, w = s.w, h = s.h;
    if (col >= w) return;
    const size_t m = (size_t)(s.m0 + (int)blockIdx.z);
    float* P = s.base + blockIdx.y * s.plane_stride + m * s.map_stride + col;
    const float* F = s.fb ? s.fb + m * s.fb_map_stride + col : nullptr;
    float carry = 0.0f;
    for (int i0 = 0; i0 < h; i0 += SB) {                                 // down: x[i] pairs with av[i - 1]
        float x[SB], f[SB];
#pragma unroll
        for (int u = 0; u < SB; u++) {
            const int i = min(i0 + u, h - 1);
            x[u] = P[(size_t)i * w];
            f[u] = F ? F[(size_t)max(i - 1, 0) * w] : s.a;
        }
#pragma unroll
        for (int u = 0; u < SB; u++) {
            const int i = i0 + u;
            if (i < h) {
                if (i > 0) x[u] = x[u] + f[u] * (carry - x[u]);
                carry = x[u];
            }
        }
#pragma unroll
        for (int u = 0; u < SB; u++)
            if (i0 + u < h) P[(size_t)(i0 + u) * w] = x[u];
    }
    for (int i0 = (h - 1) / SB * SB; i0 >= 0; i0 -= SB) {                // up: x[i] pairs with av[i]
        float x[SB], f[SB];
#pragma unroll
        for (int u = 0; u < SB; u++) {
            const int i = min(i0 + u, h - 1);
            x[u] = P[(size_t)i * w];
            f[u] = F ? F[(size_t)i * w] : s.a;
        }
#pragma unroll
        for (int u = SB - 1; u >= 0; u--) {
            const int i = i0 + u;
            if (i < h) {
                if (i < h - 1) x[u] = x[u] + f[u] * (carry - x[u]);
                carry = x[u];
            }
        }
#pragma unroll
        for (int u = 0; u < SB; u++)
            if (i0 + u < h) P[(size_t)(i0 + u) * w] = x[u];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The host half: call record, plan, check, run.

struct AmCall {                        // one call as its C entry point received it
    FilterImages im;
    double sigma_s, sigma_r; int tree_height, adjust_outliers;
};

constexpr const char* WHO = "amFilter";

// What the plan depends on, refused alike by the calls, adf_am_plan_host and adf_am_filter_workspace_bytes.
int plan_check(const char* who, double sigma_s, double sigma_r, int tree_height, int W, int H, adf_am_plan* p)
{
    if (!std::isfinite(sigma_s) || sigma_s < 1.0) return fail(ADF_EBADARG, "%s: sigma_s must be finite and at least 1", who);
    if (!std::isfinite(sigma_r) || !(sigma_r > 0.0 && sigma_r <= 1.0)) return fail(ADF_EBADARG, "%s: sigma_r must be in (0, 1]", who);
    if (tree_height == 0 || tree_height < -1 || tree_height > ADF_AM_MAX_TREE_HEIGHT)
        return fail(ADF_EBADARG, "%s: tree_height must be -1 (automatic) or 1 .. %d", who, ADF_AM_MAX_TREE_HEIGHT);
    if (W < 1 || H < 1) return fail(ADF_EBADARG, "%s: the map is empty", who);
    const double ln2 = std::log(2.0);
    // adaptive_manifold_filter_n.cpp:172-178, 70-75
    const double df = std::max(1.0, std::pow(2.0, std::floor(std::log(std::min(sigma_s / 4.0, 256.0 * sigma_r)) / ln2)));
    const int height = tree_height > 0 ? tree_height
                                       : std::max(2, (int)std::ceil((std::floor(std::log(sigma_s) / ln2) - 1.0) * (1.0 - sigma_r)));
    if (height > ADF_AM_MAX_TREE_HEIGHT)
        return fail(ADF_EBADARG, "%s: the automatic tree height %d exceeds %d; set tree_height", who, height, ADF_AM_MAX_TREE_HEIGHT);
    p->df = (int)df;
    p->height = height;
    p->sh = (int)std::nearbyint((double)H * (1.0 / df));                // cvRound: ties to even
    p->sw = (int)std::nearbyint((double)W * (1.0 / df));
    if (p->sh < 1 || p->sw < 1) return fail(ADF_EBADARG, "%s: the map is smaller than half a cell of the small plane (df = %d)", who, p->df);
    p->manifolds = (1 << height) - 1;
    p->a_root = (float)std::exp(-std::sqrt(2.0) / sigma_s);
    p->a_child = (float)std::exp(-std::sqrt(2.0) / (sigma_s / df));
    p->sr2 = (float)(sigma_r / std::sqrt(2.0));
    p->arg_w = -0.5f / (p->sr2 * p->sr2);
    p->ss = (float)(sigma_s / df);
    const float q = p->ss / p->sr2;
    p->ratio = q * q;
    p->ln_a = (float)(-std::sqrt(2.0) / (double)p->ss);
    p->arg_out = (float)(-0.5 / (sigma_r * sigma_r));
    return ADF_OK;
}

// The workspace: the PCA sums of every map first (8-byte aligned, whatever the caller's pointer), then a block per map.
struct Layout {
    size_t acc_bytes, per_map;                                           // per_map: floats
    size_t num, den, mind, etaF, path, psi, fb, levels, slot;            // floats from a block's start; a level's slot
    size_t bytes;
};
Layout layout_of(int n_maps, int W, int H, int ch, const adf_am_plan& p)
{
    Layout l{};
    const size_t WH = (size_t)W * H, S = (size_t)p.sw * p.sh;
    l.acc_bytes = pad_to((size_t)n_maps * p.manifolds * 3 * sizeof(long long), 256);
    size_t at = 0;
    l.num = at; at += WH;
    l.den = at; at += WH;
    l.mind = at; at += WH;
    l.etaF = at; at += ch * WH;
    l.path = at; at += (WH + 3) / 4;
    l.psi = at; at += 2 * S;
    l.fb = at; at += 2 * S;
    l.slot = 2 * (size_t)(1 + ch) * S;                                   // [child][tb, eta_c]
    l.levels = at; at += (size_t)p.height * l.slot;
    l.per_map = pad_to(at, 4);
    l.bytes = 8 + l.acc_bytes + (size_t)n_maps * l.per_map * sizeof(float);
    return l;
}

int am_check(const AmCall& c, adf_am_plan* p)
{
    const FilterImages& im = c.im;
    if (!im.guide.p) return fail(ADF_EBADARG, "%s: joint is NULL (filtering src by itself is not built)", WHO);
    if (!im.src.p || !im.dst.p) return fail(ADF_EBADARG, "%s: src and dst must be non-NULL", WHO);
    if (im.n < 1 || im.W < 1 || im.H < 1) return fail(ADF_EBADARG, "%s: the map is empty", WHO);
    if (!known_depth(im.src_depth) || !known_depth(im.dst_depth))
        return fail(ADF_EBADARG, "%s: src and dst must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", WHO);
    if (im.guide_channels != 1 && im.guide_channels != 3) return fail(ADF_EBADARG, "%s: joint must have 1 or 3 channels", WHO);
    if (int rc = plan_check(WHO, c.sigma_s, c.sigma_r, c.tree_height, im.W, im.H, p)) return rc;
    return filter_geometry_check(WHO, im, "their depths", "src or joint");
}

// `kernel` over `count` elements of every map, NT threads a workgroup, the maps along the grid's y.
template <class K> int am_launch(K kernel, size_t count, int n_maps, AmArgs a, hipStream_t st)
{
    return for_batches(n_maps, GRID_LIMIT, [&](int m0, unsigned nm) {
        a.m0 = m0;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((count + NT - 1) / NT), nm), dim3(NT), 0, st, a);
        return launched();
    });
}

int am_sweep(SweepArgs s, int planes, int n_maps, hipStream_t st)
{
    return for_batches(n_maps, GRID_LIMIT, [&](int m0, unsigned nm) {
        s.m0 = m0;
        hipLaunchKernelGGL(am_row_sweep_kernel, dim3((unsigned)((s.h + SR - 1) / SR), (unsigned)planes, nm), dim3(ST), 0, st, s);
        SweepArgs v = s;
        if (v.fb) v.fb += (size_t)s.w * s.h;                             // av follows ah
        hipLaunchKernelGGL(am_col_sweep_kernel, dim3((unsigned)((s.w + ST - 1) / ST), (unsigned)planes, nm), dim3(ST), 0, st, v);
        return launched();
    });
}

template <int CH> struct AmRun {
    const AmCall& c; const adf_am_plan& p; const Layout& l; AmArgs a; hipStream_t st;
    int visited = 0;

    // The node at `level` whose manifold lies at `eta`, its cluster the pixels whose path bits equal `code`; then its
    // children, minus before plus.
    template <bool ROOT> int node(int level, int code, size_t eta)
    {
        const int n = c.im.n;
        const size_t WH = (size_t)a.W * a.H, S = (size_t)a.sw * a.sh;
        a.level = level; a.code = code; a.eta = eta; a.node = visited; a.first = visited == 0;
        a.child = l.levels + (size_t)level * l.slot;                     // level + 1's slot
        visited++;
        int rc = c.im.src_depth == ADF_8U    ? am_launch(am_splat_kernel<CH, ROOT, uint8_t>, S, n, a, st)
                 : c.im.src_depth == ADF_16S ? am_launch(am_splat_kernel<CH, ROOT, int16_t>, S, n, a, st)
                                             : am_launch(am_splat_kernel<CH, ROOT, float>, S, n, a, st);
        if (rc) return rc;
        if ((rc = am_launch(am_feedback_kernel<CH>, S, n, a, st))) return rc;
        if ((rc = am_sweep(SweepArgs{a.ws + l.psi, S, l.per_map, a.ws + l.fb, l.per_map, 0.0f, a.sw, a.sh, 0}, 2, n, st))) return rc;
        if ((rc = am_launch(am_slice_kernel<CH, ROOT>, WH, n, a, st))) return rc;
        if (level >= p.height) return ADF_OK;
        if constexpr (CH == 3)
            if ((rc = am_launch(am_pca_kernel<ROOT>, WH, n, a, st))) return rc;
        if ((rc = am_launch(am_split_kernel<CH, ROOT>, WH, n, a, st))) return rc;
        if ((rc = am_launch(am_children_kernel<CH, ROOT>, S, n, a, st))) return rc;
        if ((rc = am_sweep(SweepArgs{a.ws + a.child, S, l.per_map, nullptr, 0, p.a_child, a.sw, a.sh, 0}, 2 * (1 + CH), n, st))) return rc;
        if ((rc = am_launch(am_divide_kernel<CH>, S, n, a, st))) return rc;
        const size_t child = a.child;                                    // (a is rewritten by the minus subtree)
        if ((rc = node<false>(level + 1, code, child + S))) return rc;
        return node<false>(level + 1, code | 1 << (level - 1), child + (size_t)(2 + CH) * S);
    }

    int run()
    {
        const int n = c.im.n;
        const size_t WH = (size_t)a.W * a.H, S = (size_t)a.sw * a.sh;
        if (CH == 3 && p.height > 1) HIP_TRY(hipMemsetAsync(a.acc, 0, (size_t)n * p.manifolds * 3 * sizeof(long long), st));
        a.eta = l.levels + S;                                            // the root's manifold: the first slot's first eta planes
        int rc = am_launch(am_root_kernel<CH>, WH, n, a, st);
        if (rc) return rc;
        if ((rc = am_sweep(SweepArgs{a.ws + l.etaF, WH, l.per_map, nullptr, 0, p.a_root, a.W, a.H, 0}, CH, n, st))) return rc;
        if ((rc = am_launch(am_down_kernel<CH>, S, n, a, st))) return rc;
        if ((rc = node<true>(1, 0, a.eta))) return rc;
        const int sd = c.im.src_depth, dd = c.im.dst_depth;
#define AM_FINISH(SrcT) (dd == ADF_8U ? am_launch(am_finish_kernel<SrcT, uint8_t>, WH, n, a, st) \
                         : dd == ADF_16S ? am_launch(am_finish_kernel<SrcT, int16_t>, WH, n, a, st) \
                                         : am_launch(am_finish_kernel<SrcT, float>, WH, n, a, st))
        rc = sd == ADF_8U ? AM_FINISH(uint8_t) : sd == ADF_16S ? AM_FINISH(int16_t) : AM_FINISH(float);
#undef AM_FINISH
        return rc;
    }
};

// ws: adf_am_filter_workspace_bytes of device memory
int am_run(const AmCall& c, const adf_am_plan& p, void* ws, hipStream_t st)
{
    const FilterImages& im = c.im;
    const Layout l = layout_of(im.n, im.W, im.H, im.guide_channels, p);
    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 7) & ~(uintptr_t)7);
    AmArgs a{};
    a.joint = static_cast<const uint8_t*>(im.guide.p); a.joint_stride = im.guide.stride; a.joint_map_stride = im.guide.map_stride;
    a.src = static_cast<const char*>(im.src.p); a.src_stride = im.src.stride; a.src_map_stride = im.src.map_stride;
    a.dst = static_cast<char*>(im.dst.p); a.dst_stride = im.dst.stride; a.dst_map_stride = im.dst.map_stride;
    a.W = im.W; a.H = im.H; a.sw = p.sw; a.sh = p.sh;
    a.down_scale = (double)p.df; a.up_x = (double)p.sw / im.W; a.up_y = (double)p.sh / im.H;
    a.argW = p.arg_w; a.ratio = p.ratio; a.lnA = p.ln_a; a.argOut = p.arg_out;
    a.adjust = c.adjust_outliers != 0;
    a.acc = reinterpret_cast<long long*>(base); a.nodes = p.manifolds;
    a.ws = reinterpret_cast<float*>(base + l.acc_bytes); a.per_map = l.per_map;
    a.num = l.num; a.den = l.den; a.mind = l.mind; a.etaF = l.etaF; a.path = l.path; a.psi = l.psi; a.fb = l.fb;
    return im.guide_channels == 3 ? AmRun<3>{c, p, l, a, st}.run() : AmRun<1>{c, p, l, a, st}.run();
}

AmCall call_of(int n_maps, const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
               const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
               void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
               int W, int H, double sigma_s, double sigma_r, int tree_height, int adjust_outliers)
{
    return AmCall{{n_maps, W, H, image_of(joint, joint_stride, joint_map_stride), joint_channels, image_of(src, src_stride, src_map_stride), src_depth,
                   image_of(dst, dst_stride, dst_map_stride), dst_depth, {}}, sigma_s, sigma_r, tree_height, adjust_outliers};
}

} // namespace

extern "C" int adf_am_plan_host(double sigma_s, double sigma_r, int tree_height, int W, int H, adf_am_plan* plan, float* jtab)
{
    if (!plan) return fail(ADF_EBADARG, "adf_am_plan_host: plan is NULL");
    adf_am_plan p{};
    if (int rc = plan_check("adf_am_plan_host", sigma_s, sigma_r, tree_height, W, H, &p)) return rc;
    *plan = p;
    if (jtab)
        for (int v = 0; v < 256; v++) jtab[v] = (float)((double)v / 255.0);
    return ADF_OK;
}

extern "C" int adf_am_exp_host(const float* x, float* y, size_t n)
{
    if (n && (!x || !y)) return fail(ADF_EBADARG, "adf_am_exp_host: x and y must be non-NULL");
    for (size_t i = 0; i < n; i++) y[i] = am_exp(x[i]);
    return ADF_OK;
}

extern "C" size_t adf_am_filter_workspace_bytes(int n_maps, int W, int H, int joint_channels, double sigma_s, double sigma_r, int tree_height)
{
    adf_am_plan p{};
    if (n_maps < 1 || W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31) || (joint_channels != 1 && joint_channels != 3)) return 0;
    if (plan_check("adf_am_filter_workspace_bytes", sigma_s, sigma_r, tree_height, W, H, &p)) return 0;
    return layout_of(n_maps, W, H, joint_channels, p).bytes;
}

extern "C" int adf_am_filter_device(int n_maps,
                                    const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                    const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                    void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                    int W, int H, double sigma_s, double sigma_r, int tree_height, int adjust_outliers,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    const AmCall c = call_of(n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, sigma_s, sigma_r, tree_height, adjust_outliers);
    adf_am_plan p{};
    int rc = am_check(c, &p);
    if (rc) return rc;
    Scratch blk;
    void* ws;
    rc = workspace_or_scratch(WHO, "adf_am_filter_workspace_bytes", workspace, workspace_bytes,
                              layout_of(n_maps, W, H, joint_channels, p).bytes, (hipStream_t)stream, blk, &ws);
    return rc ? rc : am_run(c, p, ws, (hipStream_t)stream);
}

extern "C" int adf_am_filter_host(int n_maps,
                                  const uint8_t* joint, ptrdiff_t joint_stride, ptrdiff_t joint_map_stride, int joint_channels,
                                  const void* src, ptrdiff_t src_stride, ptrdiff_t src_map_stride, int src_depth,
                                  void* dst, ptrdiff_t dst_stride, ptrdiff_t dst_map_stride, int dst_depth,
                                  int W, int H, double sigma_s, double sigma_r, int tree_height, int adjust_outliers)
{
    const AmCall c = call_of(n_maps, joint, joint_stride, joint_map_stride, joint_channels, src, src_stride, src_map_stride, src_depth,
                             dst, dst_stride, dst_map_stride, dst_depth, W, H, sigma_s, sigma_r, tree_height, adjust_outliers);
    adf_am_plan p{};
    int rc = am_check(c, &p);
    if (rc) return rc;
    return staged_call(c.im, layout_of(n_maps, W, H, joint_channels, p).bytes, [&](const FilterImages& staged, void* ws, hipStream_t st) {
        return am_run(AmCall{staged, c.sigma_s, c.sigma_r, c.tree_height, c.adjust_outliers}, p, ws, st);   // the same call on the staged images
    });
}
