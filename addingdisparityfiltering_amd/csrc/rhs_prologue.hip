// rhs_prologue.hip -- the kernels that write the right-hand sides of the solve as float planes, for gfx950 (the
// default WLS path forms them inside its first row pass instead: fgs_wave_h.hip).
//
//   lrc_prologue_kernel  : DF.cpp:306-341 (discontinuity-aware left-right check), DF.cpp:209
//                          (x255) and DF.cpp:288-290 (conf*float(disp)), fused; writes the
//                          two right-hand sides of the solve in the orientation the first
//                          pass wants
//   plain_prologue_kernel: source channel -> float right-hand side: the no-confidence path's
//                          float(disp) (DF.cpp:250,257) and FGS.cpp:191-205 (split + convertTo); WLS_F32: the
//                          float disparity maps of adf_wls_filter_typed_*, every element through
//                          wls_input_value -- after the confidence-only left-view kernel where the first row
//                          pass is not fused (that kernel sees the int16 planes q, not the maps)
//   quantise_maps_kernel : float disparity maps -> the int16 planes q the confidence kernels read unchanged
//                          (and the left map's v as a float plane for the down-scaled path's resize)
//
// Elementwise float work: HBM-bound, no MFMA.  Arithmetic that must match the CPU restatement bit for bit is written
// as separate roundings (contraction off).
#include "adf_internal.h"

#pragma clang fp contract(off)

namespace adf {

namespace {

using namespace tile;

// LRC + x255 + prologue.  Grid covers the full frame so the confidence plane is written
// exactly once everywhere (zero outside the ROI, DF.cpp:187-190,209).
// F32: the left map is CV_32FC1 (LrcArgs::dl_f32): its element is loaded as it is in the first phase and becomes v and q
// at the start of the second, where the int16 form first uses its own value too.
template <bool F32>
__global__ void __launch_bounds__(NT) lrc_prologue_kernel(LrcArgs a)
{
    __shared__ RhsTile lds;
    const Geom& g = a.g;
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const size_t pz = blockIdx.z;
    const char* pL = reinterpret_cast<const char*>(a.dL) + (ptrdiff_t)pz * a.psL;
    const char* pR = reinterpret_cast<const char*>(a.dR) + (ptrdiff_t)pz * a.psR;
    const float* cL = a.cL + pz * g.frame;
    const float* cR = a.cR + pz * g.frame;
    float* conf = a.conf + pz * g.cframe + g.cx0;
    const RhsPlanes u = a.U0 ? rhs_planes(a.U0, a.U1, a.orient, pz, g.plane) : RhsPlanes{nullptr, nullptr};   // null: confidence only (down-scaled path)
    const int j = x0 + tx;
    const int right_end = a.rrx + g.rw;

    // Three phases over the thread's TY/4 pixels -- own values, the gathers they address, then arithmetic and
    // stores -- so that no loaded value is first used inside the storing loop (stores count in vmcnt on this
    // target: a wait for a load there would also wait for every store issued before it).
    constexpr int NK = TY / 4;
    int dv[NK], drv[NK]; float cv[NK], bv[NK], fv[F32 ? NK : 1]; bool roi_k[NK], hit[NK];
    (void)fv;
#pragma unroll
    for (int kk = 0; kk < NK; kk++) {
        const int i = y0 + ty + 4 * kk;
        roi_k[kk] = i < g.H && j < g.W && j >= g.rx && j < g.rx + g.rw && i >= g.ry && i < g.ry + g.rh;
        dv[kk] = 0; cv[kk] = 0.0f;
        if constexpr (F32) fv[kk] = 0.0f;
        if (roi_k[kk]) {
            if constexpr (F32) fv[kk] = reinterpret_cast<const float*>(pL + (ptrdiff_t)i * a.sL)[j];
            else dv[kk] = reinterpret_cast<const int16_t*>(pL + (ptrdiff_t)i * a.sL)[j];
            cv[kk] = cL[(size_t)i * g.W + j];
        }
    }
#pragma unroll
    for (int kk = 0; kk < NK; kk++) {
        const int i = y0 + ty + 4 * kk;
        if constexpr (F32) { fv[kk] = wls_input_value(fv[kk]); dv[kk] = wls_input_q(fv[kk]); }
        const int ridx = j - (dv[kk] >> 4);                             // DF.cpp:331
        hit[kk] = roi_k[kk] && ridx >= a.rrx && ridx < right_end;
        drv[kk] = 0; bv[kk] = 0.0f;
        if (hit[kk]) {
            drv[kk] = reinterpret_cast<const int16_t*>(pR + (ptrdiff_t)i * a.sR)[ridx];
            bv[kk] = cR[(size_t)i * g.W + ridx];
        }
    }
#pragma unroll
    for (int kk = 0; kk < NK; kk++) asm volatile("" : "+v"(drv[kk]), "+v"(bv[kk]));   // the one wait for the gathers
#pragma unroll
    for (int kk = 0; kk < NK; kk++) {
        const int i = y0 + ty + 4 * kk;
        const bool in_frame = i < g.H && j < g.W;
        const bool in_roi = roi_k[kk];
        const int d = dv[kk];
        float c = cv[kk], u0 = 0.0f;
        if (in_roi) {
            if (hit[kk]) {
                if (abs(d + drv[kk]) < a.thresh) c = bv[kk] < c ? bv[kk] : c;   // DF.cpp:334-335 (std::min)
                else c = 0.0f;                                                  // DF.cpp:337
            }
            c = 255.0f * c;                                             // DF.cpp:209
            if constexpr (F32) u0 = c * fv[kk];                         // one float multiply
            else u0 = c * (float)d;                                     // DF.cpp:289-290
        }
        if (in_frame) {
            conf[(size_t)i * g.cpitch + j] = c;
            if (a.out && !in_roi)                                          // DF.cpp:284
                store_fill(a.out, (ptrdiff_t)pz * a.psO + (ptrdiff_t)i * a.sO, j, a.fill, a.out_f32);
        }
        if (!u.U0) continue;
        if (a.orient == ORIENT_T) lds.stage(tx, ty + 4 * kk, u0, c);
        else if (in_roi) {
            const size_t o = rhs_index(a.orient, i - g.ry, j - g.rx, g);
            u.U0[o] = u0; u.U1[o] = c;
        }
    }
    if (u.U0 && a.orient == ORIENT_T) lds.store(u.U0, u.U1, g, x0 - g.rx, y0 - g.ry);
}

// One element of a source row as float (FGS.cpp:203-205 convertTo; DF.cpp:250,257)
__device__ __forceinline__ float load_as_float(const char* row, size_t element, int depth)
{
    if (depth == ADF_16S) return (float)reinterpret_cast<const int16_t*>(row)[element];
    if (depth == ADF_8U) return (float)reinterpret_cast<const uint8_t*>(row)[element];
    return reinterpret_cast<const float*>(row)[element];   // ADF_32F
}

template <bool WLS_F32>
__global__ void __launch_bounds__(NT) plain_prologue_kernel(PlainPrologueArgs a)
{
    __shared__ RhsTile lds;
    const Geom& g = a.g;
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY; // ROI coordinates
    const size_t pz = blockIdx.z;
    const char* pL = reinterpret_cast<const char*>(a.src) + (ptrdiff_t)pz * a.pair_stride;
    const float* cf = a.conf ? a.conf + pz * g.cframe + g.cx0 : nullptr;
    const RhsPlanes u = rhs_planes(a.U0, a.U1, a.orient, pz, g.plane);   // (ORIENT_PAIR only with two right-hand sides)
    float* U1 = (a.conf != nullptr || a.pair2) ? u.U1 : nullptr;        // null: one right-hand side
    const int j = x0 + tx;
    // Loads of all TY/4 pixels first, stores afterwards (see lrc_prologue_kernel).  The depth is decided once, around
    // the pixel loop: with the decision inside it, small edits elsewhere in this kernel made the compiler lay the
    // uniform branches out in a longer way that measured 2 % slower (profiles/rhs_prologue_refactor_isa.txt).
    constexpr int NK = TY / 4;
    float v0[NK], v1[NK];
    const auto load_pixels = [&](int depth) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < NK; kk++) {
            const int i = y0 + ty + 4 * kk;
            const bool ok = i < g.rh && j < g.rw;
            float u0 = 0.0f, u1 = 0.0f;
            if (ok) {
                const char* row = pL + (ptrdiff_t)(g.ry + i) * a.stride;
                u0 = load_as_float(row, (size_t)(g.rx + j) * a.cn + a.c, depth);
                if constexpr (WLS_F32) u0 = wls_input_value(u0);
                if (a.pair2) u1 = load_as_float(row, (size_t)(g.rx + j) * a.cn + a.c2, depth);   // second channel, FGS.cpp:200-205
                if (cf) {                                                                    // DF.cpp:286-290
                    u1 = cf[(size_t)(g.ry + i) * g.cpitch + g.rx + j];
                    u0 = u1 * u0;
                }
            }
            v0[kk] = u0; v1[kk] = u1;
        }
    };
    if constexpr (WLS_F32) load_pixels(ADF_32F);
    else if (a.depth == ADF_16S) load_pixels(ADF_16S);
    else if (a.depth == ADF_8U) load_pixels(ADF_8U);
    else load_pixels(ADF_32F);
#pragma unroll
    for (int kk = 0; kk < NK; kk++) asm volatile("" : "+v"(v0[kk]), "+v"(v1[kk]));   // every load waited for before the first store
#pragma unroll
    for (int kk = 0; kk < NK; kk++) {
        const int i = y0 + ty + 4 * kk;
        if (a.orient == ORIENT_T) lds.stage(tx, ty + 4 * kk, v0[kk], v1[kk]);
        else if (i < g.rh && j < g.rw) {
            const size_t o = rhs_index(a.orient, i, j, g);
            u.U0[o] = v0[kk]; if (U1) U1[o] = v1[kk];
        }
    }
    if (a.orient == ORIENT_T) lds.store(u.U0, U1, g, x0, y0);
}

// One thread: 8 adjacent elements of a map row -- two 16-byte loads at the caller's 4-byte alignment, one 16-byte store
// of q (two more of v).  The last, partial group of a row is read element by element: never past the caller's row.
constexpr int QN = 8;
__global__ void __launch_bounds__(NT) quantise_maps_kernel(QuantArgs a)
{
    typedef float v4f_u __attribute__((ext_vector_type(4), aligned(4)));
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * QN, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.pitch || y >= a.H) return;
    const int m = (int)blockIdx.z / a.n_pairs;
    const size_t pz = blockIdx.z % a.n_pairs;
    const float* s = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.src[m]) + (ptrdiff_t)pz * a.pair_stride[m] +
                                                    (ptrdiff_t)y * a.stride[m]) + x;
    float d[QN];
    if (x + QN <= a.W) {
        const v4f_u lo = __builtin_nontemporal_load(reinterpret_cast<const v4f_u*>(s));
        const v4f_u hi = __builtin_nontemporal_load(reinterpret_cast<const v4f_u*>(s + 4));
#pragma unroll
        for (int e = 0; e < 4; e++) { d[e] = lo[e]; d[4 + e] = hi[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < QN; e++) d[e] = x + e < a.W ? s[e] : 0.0f;
    }
    unsigned w[QN / 2];
#pragma unroll
    for (int e = 0; e < QN; e++) d[e] = wls_input_value(d[e]);
#pragma unroll
    for (int e = 0; e < QN / 2; e++)
        w[e] = (unsigned)(unsigned short)wls_input_q(d[2 * e]) | ((unsigned)(unsigned short)wls_input_q(d[2 * e + 1]) << 16);
    const size_t o = pz * a.frame + (size_t)y * a.pitch + x;          // pitch, frame: multiples of 8 elements
    if (a.q[m]) *reinterpret_cast<v4u*>(a.q[m] + o) = v4u{w[0], w[1], w[2], w[3]};
    if (m == 0 && a.v) {
        *reinterpret_cast<v4f*>(a.v + o) = v4f{d[0], d[1], d[2], d[3]};
        *reinterpret_cast<v4f*>(a.v + o + 4) = v4f{d[4], d[5], d[6], d[7]};
    }
}

} // namespace

hipError_t launch_quantise_maps(const QuantArgs& a, hipStream_t st)
{
    const int maps = a.src[1] ? 2 : 1;
    if (!a.src[0] || a.n_pairs < 1 || a.W < 1 || a.H < 1 || a.pitch % QN != 0 || a.pitch < a.W || a.frame % QN != 0 ||
        a.frame < (size_t)a.pitch * a.H || (maps == 2 && !a.q[1])) return hipErrorInvalidValue;
    dim3 grid((a.pitch / QN + 63) / 64, (a.H + 3) / 4, maps * a.n_pairs);
    hipLaunchKernelGGL(quantise_maps_kernel, grid, dim3(NT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_lrc_prologue(const LrcArgs& a, int n_pairs, hipStream_t st)
{
    dim3 grid((a.g.W + TX - 1) / TX, (a.g.H + TY - 1) / TY, n_pairs);
    if (a.dl_f32) hipLaunchKernelGGL(lrc_prologue_kernel<true>, grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(lrc_prologue_kernel<false>, grid, dim3(NT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_plain_prologue(const PlainPrologueArgs& a, int n_pairs, hipStream_t st)
{
    dim3 grid((a.g.rw + TX - 1) / TX, (a.g.rh + TY - 1) / TY, n_pairs);
    if (a.depth == DEPTH_WLS_F32) hipLaunchKernelGGL(plain_prologue_kernel<true>, grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(plain_prologue_kernel<false>, grid, dim3(NT), 0, st, a);
    return hipGetLastError();
}

} // namespace adf
