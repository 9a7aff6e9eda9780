// fgs_wave_common.h -- on-chip partitioned Thomas solve (ADF_SOLVER_WAVE).
//
// Same tridiagonal systems as FastGlobalSmootherFilterImpl::process_row / VerticalPass_ParBody
// (FGS.cpp:439-464, 484-584):  a_j x_{j-1} + b_j x_j + c_j x_{j+1} = f_j  with  c_j = lambda*C[j],
// a_j = c_{j-1}, b_j = 1 - a_j - c_j -- but solved so that every scanline stays on chip and HBM sees
// only the algorithmic traffic (read C and the R right-hand sides, write the R solutions: 4+8R bytes
// per pixel instead of the 12+16R of a lane-per-scanline sweep that must spill D and the eliminated
// right-hand sides).
//
// A scanline is cut into 64 chunks of M elements.  The last element of each chunk is a separator:
//   phase 1  two running sweeps over the chunk interior (left->right LU, right->left UL) give, with
//            O(1) state, how the interior's two end elements depend on the neighbouring separators:
//            x_first = GS - PS*xL - QS*xR,  x_last = GE - PE*xL - QE*xR;
//   reduce   the 64 separator equations form a tridiagonal system (alpha,beta,gamma,phi) solved by
//            parallel cyclic reduction across the 64 lanes of a wavefront (6 shuffle steps);
//   phase 2  with xL, xR known, a plain Thomas solve of the interior held entirely in registers.
// The matrix is strictly diagonally dominant (b = 1 + |a| + |c|), so every step is stable without
// pivoting.  Arithmetic is re-associated (FMA, v_rcp + one Newton step) => results differ from the
// scalar order in the last bits; the tests hold them to the reference's own reproducibility bar
// (<=1 LSB of the CV_16S output, mean <=1/256 LSB: test_disparity_wls_filter.cpp:104-105).
//
//   horizontal pass: one wavefront per image row; lane l owns columns [l*M, l*M+M); the row goes
//                    HBM -> (coalesced 16 B/lane) -> LDS -> (chunk per lane) -> registers and back.
//   vertical pass:   one 512-thread workgroup per strip of 16 columns; thread (chunk, column pair)
//                    owns M rows of 2 columns; the whole strip (16 x H x 3 floats) lives in the CU's
//                    register file; neighbour / separator exchange through LDS.
//
// Data layout (everything is solved in place, nothing is transposed between the passes):
//   Chor            row-major [rh][pw]
//   Cvert           strip-major [pw/16][rh][16]: the weights of a vertical strip are one contiguous stream
//   one right-hand side (R == 1)    row-major [rh][pw]; a strip row is then a 64-byte half line (the
//                   other half is served from L2/MALL to the neighbouring strip)
//   two right-hand sides (R == 2)   ONE pair plane [rh/2][pw/16][row parity][U0 x16 | U1 x16] of 2*plane
//                   floats per image: a strip row of the column pass is one full 128-byte line holding
//                   both right-hand sides and two consecutive rows are 256 contiguous bytes; the row pass
//                   reads an image row as 128-byte pieces at a 256-byte stride (the other row of the pair
//                   fills the gaps) and de-interleaves in its LDS staging buffer.  Measured against plain
//                   row-major pair rows: column pass -6 %, row pass +3.5 %.  U1 pointers are ignored.
//   the last hand-off (WavePassArgs::image; two right-hand sides, one-wave rows, whole-strip columns)   what the last
//                   row pass writes only the last column pass reads, so it may be that pass's REGISTER IMAGE:
//                   [pw/16 strips][8 waves][Mc rows of a chunk][64 lanes = (chunk % 8) * 8 + column pair][U0 c, U0 c+1,
//                   U1 c, U1 c+1], Mc the column bucket's chunk length, 64 * Mc rows per strip (those past the
//                   column's end stay zero), pw * 64 * Mc * 2 floats per image.  A thread's two columns of both
//                   right-hand sides of a row are one 16-byte element, a wave instruction of the column pass one
//                   contiguous KiB, a strip one contiguous stream; the row pass stores a strip's 16 columns of a row as
//                   one whole 128-byte line.  Measured: profiles/last_handoff_floor.txt, last_handoff_ab.txt.
#pragma once
#include "adf_internal.h"

#include <type_traits>

namespace adf {
namespace wave {

// ---------------------------------------------------------------------------------------------
// Element type T of the chunk templates: float in the row pass (a lane owns one chunk), v2f in the column pass (a
// thread owns the same rows of two adjacent columns).  On 2-vectors the sweeps compile to the packed fp32 instructions
// (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32: two lanes of work per issue slot), and the register pair an 8-byte load
// fills is the pair the arithmetic and the 8-byte store use; v_rcp_f32 has no packed form and is issued per element.
// ---------------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f vfma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f vsplat(float x) { return (v2f){x, x}; }
__device__ __forceinline__ v2f vrcp_nr(v2f x)
{
    const v2f r = {__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)};
    return vfma(vfma(-x, r, vsplat(1.0f)), r, r);
}
__device__ __forceinline__ float rcp_nr(float x)
{
    float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ v2f rcp_nr(v2f x) { return vrcp_nr(x); }
// fma on either element type: the builtin itself (v_fma_f32 / v_pk_fma_f32).  A macro, not a function: behind a
// wrapper the row pass's sweeps come out in another instruction order (several kernels, other register counts).
#define ADF_FMA(a, b, c) __builtin_elementwise_fma(a, b, c)
template <class T>
__device__ __forceinline__ T splat(float x)
{
    if constexpr (std::is_same_v<T, v2f>) return vsplat(x);
    else return x;
}

// ---------------------------------------------------------------------------------------------
// Chunk kernels shared by both passes.  c[] is already multiplied by lambda; element M-1 is the
// separator, elements 0..M-2 the interior; a_s is c of the element before the chunk (0 for chunk 0).
// ---------------------------------------------------------------------------------------------
template <class T, int R>
struct Boundary { T GS0, GS1, PS, QS, GE0, GE1, PE, QE; };

// The sweeps below are serial recurrences; hipcc's scheduler, left alone, hoists every
// chain-independent temporary (b_i = 1 - a_i - c_i, c_i^2, negations) of a fully unrolled sweep to the
// front and keeps them alive -- several extra registers per element, i.e. spills at the chunk lengths
// a 4K scanline needs.  A scheduling barrier per element keeps the source order (temporaries die
// within their own step), and an empty asm on c[] keeps temporaries from being shared between sweeps.
#define ADF_STEP_FENCE() __builtin_amdgcn_sched_barrier(0)

template <int M, class T>
__device__ __forceinline__ void launder(T (&v)[M])
{
#pragma unroll
    for (int i = 0; i < M; i++) asm volatile("" : "+v"(v[i]));
}

// Which chains an empty asm pins to their step -- the one difference between the two passes' sweeps, kept as each
// pass was tuned.  The column pass (v2f) pins all of them:
// pin every chain to its step: pure arithmetic is not ordered against the fence below by
// instruction selection, and a chain that drifts out of the loop drags one reciprocal per
// step along with it (the right-hand-side chains feed nothing until the end)
// The row pass (float) pins only p and q of the boundary sweeps (they feed nothing until the end: keep their chains
// in step); its M = 60 bucket is within five registers of spilling (wave_hpass_lo_half), so its schedule is left alone.
template <class T>
constexpr bool pin_rhs_chains = std::is_same_v<T, v2f>;
// Likewise how a sweep receives its scalar operands (a_s, xL, xR): by reference in the row pass, by value in the
// column pass, as the two passes' former copies did -- the generated code of either pass changes with it.
template <class T>
using In = std::conditional_t<std::is_same_v<T, v2f>, T, const T&>;

// Quotients x / den are formed as x * r from r = rcp_nr(den): v_rcp_f32 is accurate to 1 ulp, and one Newton step
// makes it (nearly) correctly rounded at the price of two more dependent FMAs on the serial chain.  x * r carries the
// reciprocal's rounding AND the product's.  A residual step (two FMAs) would make the quotient correctly rounded in all
// but rare cases, i.e. as good as the IEEE division of the scalar order.  Measured against the float64 banded solve on
// the badly conditioned draws of tests/test_gpu_fuzz.py (mean |error| of the float planes, in LSB of the output):
// scalar order 0.060; wave solver 0.073 with plain products, 0.059 with the residual step in the boundary sweeps (the
// other two phases do not matter), at +2.3 % of a BASELINE step (the fused first row pass +11 %).  It changes nothing in
// how often the two float32 evaluations round differently, which is what the parity tests measure, so the plain
// product stays (the residual-step variant was removed; it is in the history at a483289).

// Phase 1: boundary coefficients with O(1) state.  The left->right (LU) and right->left (UL) sweeps are independent
// serial chains; they advance together, one element each per step, so that every step carries two independent chains
// (the passes are bound by VALU dependency stalls, not by issue slots).
template <int M, int R, class T>
__device__ __forceinline__ void chunk_boundary(const T (&c)[M], const T (&f0)[M], const T (&f1)[M], In<T> a_s, Boundary<T, R>& o)
{
    const T one = splat<T>(1.0f), zero = splat<T>(0.0f);
    // left -> right: x_i + D_i x_{i+1} = g_i - p_i xL;   right -> left: x_i + E_i x_{i-1} = h_i - q_i xR
    T D, g0, g1, p, r, dr, h0, h1, q;
    {
        const T dl = (one - a_s) - c[0];
        const T rl = rcp_nr(dl);
        D = c[0] * rl; g0 = f0[0] * rl; g1 = (R > 1) ? f1[0] * rl : zero; p = a_s * rl;
        const T ci = c[M - 2];
        const T ar = (M - 2 == 0) ? a_s : c[(M - 3 > 0) ? M - 3 : 0];
        dr = (one - ar) - ci;
        r = rcp_nr(dr);
        h0 = f0[M - 2] * r; h1 = (R > 1) ? f1[M - 2] * r : zero; q = ci * r;
    }
#pragma unroll
    for (int t = 1; t <= M - 2; t++) {
        const int i = t, j = M - 2 - t; // LU element, UL element
        {
            const T a = c[i - 1];
            const T b = (one - a) - c[i];
            const T dl = ADF_FMA(-a, D, b);
            const T rl = rcp_nr(dl);
            D = c[i] * rl;
            g0 = ADF_FMA(-a, g0, f0[i]) * rl;
            if (R > 1) g1 = ADF_FMA(-a, g1, f1[i]) * rl;
            p = -a * p * rl;
            if constexpr (!pin_rhs_chains<T>) asm volatile("" : "+v"(p));
            else if (R > 1) asm volatile("" : "+v"(g0), "+v"(g1), "+v"(p));
            else asm volatile("" : "+v"(g0), "+v"(p));
        }
        {
            // opaque copies: without them the compiler shares b_j = 1 - a_j - c_j between the two
            // sweeps and keeps it alive from one sweep's visit of j to the other's
            T ci = c[j];
            T a = (j == 0) ? a_s : c[(j > 0) ? j - 1 : 0];
            asm volatile("" : "+v"(ci), "+v"(a));
            const T b = (one - a) - ci;
            dr = ADF_FMA(-ci * ci, r, b);
            r = rcp_nr(dr);
            h0 = ADF_FMA(-ci, h0, f0[j]) * r;
            if (R > 1) h1 = ADF_FMA(-ci, h1, f1[j]) * r;
            q = -ci * q * r;
            if constexpr (!pin_rhs_chains<T>) asm volatile("" : "+v"(q));
            else if (R > 1) asm volatile("" : "+v"(h0), "+v"(h1), "+v"(q));
            else asm volatile("" : "+v"(h0), "+v"(q));
        }
        ADF_STEP_FENCE();
    }
    o.GE0 = g0; o.GE1 = g1; o.PE = p; o.QE = D;
    o.GS0 = h0; o.GS1 = h1; o.PS = a_s * r; o.QS = q;
}

// Phase 2: interior Thomas solve with both neighbours known; solutions overwrite f0 / f1.
template <int M, int R, class T>
__device__ __forceinline__ void chunk_solve(T (&c)[M], T (&f0)[M], T (&f1)[M], In<T> a_s, In<T> xL0, In<T> xL1, In<T> xR0, In<T> xR1)
{
    const T one = splat<T>(1.0f), zero = splat<T>(0.0f);
    launder(c);
    T corig = c[0], D, g0, g1;
    {
        const T dn = (one - a_s) - corig;
        const T r = rcp_nr(dn);
        D = corig * r;
        g0 = ADF_FMA(-a_s, xL0, f0[0]) * r;
        g1 = (R > 1) ? ADF_FMA(-a_s, xL1, f1[0]) * r : zero;
        c[0] = D; f0[0] = g0; if (R > 1) f1[0] = g1;
    }
#pragma unroll
    for (int i = 1; i <= M - 2; i++) {
        const T a = corig;
        corig = c[i];
        const T b = (one - a) - corig;
        const T dn = ADF_FMA(-a, D, b);
        const T r = rcp_nr(dn);
        D = corig * r;
        g0 = ADF_FMA(-a, g0, f0[i]) * r;
        if (R > 1) g1 = ADF_FMA(-a, g1, f1[i]) * r;
        c[i] = D; f0[i] = g0; if (R > 1) f1[i] = g1;
        if constexpr (pin_rhs_chains<T>) {
            if (R > 1) asm volatile("" : "+v"(D), "+v"(g0), "+v"(g1));
            else asm volatile("" : "+v"(D), "+v"(g0));
        }
        ADF_STEP_FENCE();
    }
    T x0 = xR0, x1 = xR1;
    f0[M - 1] = x0; if (R > 1) f1[M - 1] = x1;
#pragma unroll
    for (int i = M - 2; i >= 0; i--) {
        x0 = ADF_FMA(-c[i], x0, f0[i]);
        f0[i] = x0;
        if (R > 1) { x1 = ADF_FMA(-c[i], x1, f1[i]); f1[i] = x1; }
        if constexpr (pin_rhs_chains<T>) {
            if (R > 1) asm volatile("" : "+v"(x0), "+v"(x1));
            else asm volatile("" : "+v"(x0));
        }
        ADF_STEP_FENCE();
    }
}

// Separator equation of a chunk: alpha*x_prev + beta*x + gamma*x_next = phi.
// nGS*/nPS/nQS are the NEXT chunk's left-end coefficients (zero for the last chunk).
template <int M, int R, class T>
__device__ __forceinline__ void separator_row(const T (&c)[M], const T (&f0)[M], const T (&f1)[M], const Boundary<T, R>& o,
                                              T nGS0, T nGS1, T nPS, T nQS, T& al, T& be, T& ga, T& p0, T& p1)
{
    const T ae = c[M - 2], ce = c[M - 1];
    const T bb = (splat<T>(1.0f) - ae) - ce;
    al = -ae * o.PE;
    be = ADF_FMA(-ce, nPS, ADF_FMA(-ae, o.QE, bb));
    ga = -ce * nQS;
    p0 = ADF_FMA(-ce, nGS0, ADF_FMA(-ae, o.GE0, f0[M - 1]));
    p1 = (R > 1) ? ADF_FMA(-ce, nGS1, ADF_FMA(-ae, o.GE1, f1[M - 1])) : splat<T>(0.0f);
}

// pcr64 and reduced128 are scalar in both passes: they run one separator row per lane.
// Parallel cyclic reduction of a 64-row tridiagonal system held one row per lane.
template <int R>
__device__ __forceinline__ void pcr64(int lane, float al, float be, float ga, float p0, float p1, float& x0, float& x1)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        float am = __shfl_up(al, d), bm = __shfl_up(be, d), gm = __shfl_up(ga, d), fm0 = __shfl_up(p0, d);
        float fm1 = (R > 1) ? __shfl_up(p1, d) : 0.0f;
        float ap = __shfl_down(al, d), bp = __shfl_down(be, d), gp = __shfl_down(ga, d), fp0 = __shfl_down(p0, d);
        float fp1 = (R > 1) ? __shfl_down(p1, d) : 0.0f;
        if (lane < d) { am = 0.0f; bm = 1.0f; gm = 0.0f; fm0 = 0.0f; fm1 = 0.0f; }
        if (lane + d > 63) { ap = 0.0f; bp = 1.0f; gp = 0.0f; fp0 = 0.0f; fp1 = 0.0f; }
        const float k1 = al * rcp_nr(bm), k2 = ga * rcp_nr(bp);
        be = __builtin_fmaf(-ap, k2, __builtin_fmaf(-gm, k1, be));
        p0 = __builtin_fmaf(-fp0, k2, __builtin_fmaf(-fm0, k1, p0));
        if (R > 1) p1 = __builtin_fmaf(-fp1, k2, __builtin_fmaf(-fm1, k1, p1));
        al = -am * k1;
        ga = -gp * k2;
    }
    const float rb = rcp_nr(be);
    x0 = p0 * rb;
    x1 = (R > 1) ? p1 * rb : 0.0f;
}


// A 128-row reduced system (scanlines longer than 64 chunks: two waves per row / 128 chunks per column, round 3), solved
// by ONE wavefront from LDS: lane l takes rows 2l-1, 2l, 2l+1, eliminates the odd neighbours from the even row (one
// step of cyclic reduction), the 64 even rows go through the wave-wide PCR above, and the odd rows follow by
// substitution.  Rows are read as row[k * stride]; solutions are written the same way.  The caller puts a workgroup
// barrier before (rows complete) and after (solutions visible).
template <int R>
__device__ __forceinline__ void reduced128(int lane, const float* al, const float* be, const float* ga, const float* p0, const float* p1,
                                           int stride, float* x0, float* x1)
{
    const int e = 2 * lane, o = e + 1, m = lane > 0 ? e - 1 : 0;
    const float al_e = al[e * stride], be_e = be[e * stride], ga_e = ga[e * stride], p0_e = p0[e * stride];
    const float al_o = al[o * stride], be_o = be[o * stride], ga_o = ga[o * stride], p0_o = p0[o * stride];
    const float al_m = al[m * stride], be_m = be[m * stride], ga_m = ga[m * stride], p0_m = p0[m * stride];
    const float p1_e = (R > 1) ? p1[e * stride] : 0.0f, p1_o = (R > 1) ? p1[o * stride] : 0.0f, p1_m = (R > 1) ? p1[m * stride] : 0.0f;
    const float k1 = lane > 0 ? al_e * rcp_nr(be_m) : 0.0f;     // (row 0 has no predecessor: its alpha is 0)
    const float k2 = ga_e * rcp_nr(be_o);
    const float AL = -al_m * k1, GA = -ga_o * k2;
    const float BE = __builtin_fmaf(-al_o, k2, __builtin_fmaf(-ga_m, k1, be_e));
    const float P0 = __builtin_fmaf(-p0_o, k2, __builtin_fmaf(-p0_m, k1, p0_e));
    const float P1 = (R > 1) ? __builtin_fmaf(-p1_o, k2, __builtin_fmaf(-p1_m, k1, p1_e)) : 0.0f;
    float xe0, xe1;
    pcr64<R>(lane, AL, BE, GA, P0, P1, xe0, xe1);
    const float xn0 = __shfl_down(xe0, 1), xn1 = (R > 1) ? __shfl_down(xe1, 1) : 0.0f;   // (lane 63: row 127's gamma is 0)
    const float rb = rcp_nr(be_o);
    const float xo0 = __builtin_fmaf(-ga_o, xn0, __builtin_fmaf(-al_o, xe0, p0_o)) * rb;
    x0[e * stride] = xe0; x0[o * stride] = xo0;
    if (R > 1) {
        const float xo1 = __builtin_fmaf(-ga_o, xn1, __builtin_fmaf(-al_o, xe1, p1_o)) * rb;
        x1[e * stride] = xe1; x1[o * stride] = xo1;
    }
}

// ---------------------------------------------------------------------------------------------
// Host side: each pass keeps ONE constexpr list of its buckets, shortest first; the launcher's choice and its
// dispatch to the kernel instantiations both come from that list.
// ---------------------------------------------------------------------------------------------
struct Bucket { int m, chunks; };   // chunk length M, chunks per scanline: holds scanlines of up to m * chunks elements

template <int N>
constexpr int bucket_index(const Bucket (&b)[N], int len)   // the first bucket that holds len (the last one if none does)
{
    int i = 0;
    while (i < N - 1 && len > b[i].m * b[i].chunks) i++;
    return i;
}

// f(std::integral_constant<int, i>{}) for a run-time i in [0, N)
template <int N, int I = 0, class F>
inline hipError_t dispatch_index(int i, F&& f)
{
    if (i == I) return f(std::integral_constant<int, I>{});
    if constexpr (I + 1 < N) return dispatch_index<N, I + 1>(i, f);
    else return hipErrorInvalidValue;
}

} // namespace wave
} // namespace adf
