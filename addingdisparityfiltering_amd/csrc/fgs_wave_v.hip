// fgs_wave_v.hip -- vertical pass of the on-chip partitioned solver (see fgs_wave_common.h).
// Built with -fno-slp-vectorize: the SLP vectorizer packs the per-element temporaries of the unrolled
// sweeps into v_pk_* bundles hoisted to the front of the sweep, which costs ~50 registers at the
// chunk length a 2160-row column needs and turns into scratch spills.
#include "fgs_wave_common.h"

namespace adf {

namespace {
using namespace wave;

// ---------------------------------------------------------------------------------------------
// Vertical pass: one 512-thread workgroup per 16-column strip, in place (or fused epilogue).
// thread = (chunk cidx in [0,64), column pair xp in [0,8)); M rows x 2 columns per thread.
// ---------------------------------------------------------------------------------------------
constexpr int VT = 512;  // threads per strip
constexpr int VC = 16;   // columns per strip (the layouts' strip: fgs_wave_common.h)
typedef float v4f __attribute__((ext_vector_type(4)));
// Round 3: columns longer than 64 chunks of 34 rows (ROIs taller than 2176 rows: 8K frames) run HALF strips of 128 chunks
// -- VCW = 8 columns, NCH = 128, still 512 threads and the same rows and registers per thread, i.e. the same 415 KB of a
// CU's register file per workgroup -- with a 128-row reduced system per column (fgs_wave_common.h, reduced128).  Half
// strips read 32-byte pieces (a quarter less bandwidth on a full chip, tools/micro/vpattern.hip), still well ahead of
// the exact solver such ROIs fell back to.  Everything below is written for VCW columns x NCH chunks.

// saturate_cast<short> of both columns of a thread, packed (low half = first column).  cvRound semantics as sat16() in
// adf_internal.h: round half to even; NaN and anything outside the int range become INT_MIN and hence -32768; the clamp
// to [-32768, 32767] is v_cvt_pk_i16_i32's.  EPI_WLS_CONF forms u0 * (1 / (u1 + EPS)) first (DF.cpp:295-296) with
// v_rcp_f32 + one Newton step instead of the IEEE division's ten instructions: this solver is held to the reference's
// 1-LSB bar, not to bit identity.  Two things the division did must be kept:
//  * far from every confident pixel the filtered confidence u1 (and u0 with it) decays into the DENORMAL range while
//    the ratio stays an ordinary disparity (config 2: thousands of such pixels), and v_rcp_f32 flushes denormal
//    operands: the denominator is scaled by 2^64 before the reciprocal and the reciprocal by 2^64 after it --
//    unconditionally (u1 never exceeds a few thousand, so neither product leaves the normal range at the top);
//  * u1 == 0 exactly: 1 / 1e-43 overflows to +inf -- here 2^64 * rcp(2^64 * 1e-43) does -- and 0 * inf, x * inf and NaN
//    all leave the int range -> -32768, as in the reference (tests: zero-confidence edge case).
// (u1 * 2^64 + EPS * 2^64 in one FMA: it differs from (u1 + EPS) * 2^64 only below the last bit of a denormal sum.)
// epi_value is the float both forms of an epilogue start from: epi_pack16 rounds it, epi_f32 stores it.
template <int EPI>
__device__ __forceinline__ v2f epi_value(v2f u0, v2f u1)
{
    if (EPI == EPI_WLS_CONF || EPI == EPI_WLS_CONF_F32) {
        const v2f sc = vsplat(0x1p64f);
        return u0 * (vrcp_nr(vfma(u1, sc, vsplat(ADF_EPS * 0x1p64f))) * sc);
    }
    return u0;
}

template <int EPI>
__device__ __forceinline__ unsigned epi_pack16(v2f u0, v2f u1)
{
    const v2f x = epi_value<EPI>(u0, u1);
    const bool o0 = !(__builtin_fabsf(x.x) < 2147483648.0f), o1 = !(__builtin_fabsf(x.y) < 2147483648.0f);
    const int i0 = (int)(o0 ? -32768.0f : __builtin_rintf(x.x)), i1 = (int)(o1 ? -32768.0f : __builtin_rintf(x.y));
    typedef short s2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, (s2)__builtin_amdgcn_cvt_pk_i16(i0, i1));
}

// Both columns of a thread as the float map holds them.  EPI_WLS_CONF_F32: the ratio, with -32768.0f wherever
// epi_pack16 saturates to -32768 for a value that is NaN, infinite or outside the int range (u1 == 0 above), so the
// map holds no NaN or inf and saturate_cast<short> of it is the int16 map bit for bit.  EPI_F32: u0 as it is.
template <int EPI>
__device__ __forceinline__ v2f epi_f32(v2f u0, v2f u1)
{
    const v2f x = epi_value<EPI>(u0, u1);
    if (EPI == EPI_WLS_CONF_F32) return (v2f){wls_f32_value(x.x), wls_f32_value(x.y)};
    return x;
}

// ---- the single-channel store forms of the fused epilogues ----
// Both columns of a thread in the map's own type: a packed dword with 2-byte halves (int16 maps) or a v2f with 4-byte
// halves (float maps).
template <int EPI, bool F32>
__device__ __forceinline__ auto epi_out(v2f u0, v2f u1)
{
    if constexpr (F32) return epi_f32<EPI>(u0, u1);
    else return epi_pack16<EPI>(u0, u1);
}
__device__ __forceinline__ void put_first(char* dst, unsigned v) { reinterpret_cast<uint16_t*>(dst)[0] = (uint16_t)v; }
__device__ __forceinline__ void put_first(char* dst, v2f v) { reinterpret_cast<float*>(dst)[0] = v.x; }
__device__ __forceinline__ void put_second(char* dst, unsigned v) { reinterpret_cast<uint16_t*>(dst)[1] = (uint16_t)(v >> 16); }
__device__ __forceinline__ void put_second(char* dst, v2f v) { reinterpret_cast<float*>(dst)[1] = v.y; }
__device__ __forceinline__ void put_both(char* dst, unsigned v) { *reinterpret_cast<unsigned*>(dst) = v; }
__device__ __forceinline__ void put_both(char* dst, v2f v) { *reinterpret_cast<v2f*>(dst) = v; }

// Can a column pair of a single-channel map of `esz`-byte elements go out as ONE store of 2 * esz bytes: do the map's
// base, its strides and the ROI's first column keep every pair that much aligned?  (uniform over the launch)
__device__ __forceinline__ bool out_pairs_aligned(const WavePassArgs& a, unsigned esz)
{
    const unsigned m = 2u * esz - 1u;
    return ((reinterpret_cast<uintptr_t>(a.out) | (uintptr_t)a.out_stride | (uintptr_t)a.out_pair_stride) & m) == 0 &&
           (((unsigned)a.out_x0 * esz) & m) == 0;
}

// The thread's M rows of a single-channel map, from dst down: row i < hv2 stores both columns -- as one store when
// `aligned`, as two halves otherwise -- and, in the form with LAST_ODD, row i < hv1 its first column only (the thread
// that holds the last column of an odd-width ROI).  No branch but the row masks; every other condition is uniform
// over the launch.  Without LAST_ODD neither the hv1 compare nor its store is compiled: that is the form of every
// disparity-filter call on an even-width ROI.
template <int EPI, bool F32, bool LAST_ODD, int M>
__device__ __forceinline__ void store_rows(const v2f (&f0)[M], const v2f (&f1)[M], char* dst, ptrdiff_t stride, bool aligned, int hv2, int hv1)
{
#pragma unroll
    for (int i = 0; i < M; i++) {
        const auto v = epi_out<EPI, F32>(f0[i], f1[i]);
        if (i < hv2) {
            if (aligned) put_both(dst, v);
            else { put_first(dst, v); put_second(dst, v); }
        }
        if constexpr (LAST_ODD) {
            if (i < hv1) put_first(dst, v);
        }
        dst += stride;
        ADF_STEP_FENCE();
    }
}

// Bytes from row r0 + i of a column to row r0 + i + 1 in the plane of the right-hand sides.  Pair plane (R == 2):
// [row tile][strip][row in tile][32 floats]; consecutive rows are 128 bytes apart inside a tile and a tile apart
// (minus the rows already walked) at a tile boundary -- which rows those are depends on the chunk's start.
template <int R>
__device__ __forceinline__ unsigned vstep(int r0, int i, int pitch)
{
    constexpr unsigned TR = TILE_ROWS;
    if (R > 1) return ((((unsigned)r0 + (unsigned)i + 1u) & (TR - 1u)) == 0u) ? 2u * TR * (unsigned)pitch * 4u - (TR - 1u) * 128u : 128u;
    return (unsigned)pitch * 4u;
}

// IMG (a pass of two right-hand sides whose row pass stored the hand-off's register image, a.image): f0[i], f1[i] come
// from the image instead of the pair plane -- [strip][wave][row in chunk i][lane][U0 c, U0 c+1, U1 c, U1 c+1], the
// thread's two columns of both right-hand sides of a row as ONE 16-byte element, a wave instruction one contiguous
// KiB, 1 KiB from row to row, the strip one contiguous stream like its weights.  Whole strips only.  The plain pass
// (EPI_PLANES) stores to the pair plane as ever: the next row pass needs its contiguous rows.
template <int M, int R, int EPI, int VCW = VC, int NCH = 64, bool IMG = false>
__global__ void __launch_bounds__(VT) wave_vpass_kernel(WavePassArgs a)
{
    static_assert((VCW == 16 && NCH == 64) || (VCW == 8 && NCH == 128), "whole strips of 64 chunks or half strips of 128");
    static_assert(!IMG || (R == 2 && VCW == VC && (EPI == EPI_PLANES || EPI == EPI_WLS_CONF || EPI == EPI_WLS_CONF_F32)), "the image: whole strips, both right-hand sides, the plain pass or the filter's epilogues");
    static_assert((VCW / 2) * NCH == VT, "one thread per (chunk, column pair)");
    constexpr int XPN = VCW / 2;         // column pairs per workgroup
    __shared__ float nb[4][NCH][VCW];   // next-chunk exchange: GS0, GS1, PS, QS
    __shared__ float red[5][VCW][NCH];  // separator rows by (column, chunk)
    __shared__ float xs[2][VCW][NCH];   // separator solutions
    const int tid = threadIdx.x;
    const int xp = tid & (XPN - 1), cidx = tid / XPN;
    // A strip row is a 64-byte half of a 128-byte line of a single right-hand-side plane (R == 1) and a
    // 32-byte quarter of a line of the int16 output; the rest of the line belongs to the neighbouring
    // strips (the pair plane of R == 2 and the weights are laid out so that this does not happen).  Blocks b,
    // b+8, b+16, b+24 are dealt to the same XCD back to back (speed only, never correctness), so four
    // consecutive strips are mapped to them: later requests for a line hit (or merge in) that XCD's L2
    // instead of going to the fabric again, and partial-line writes combine there before eviction.
    int strip = VCW == VC ? (int)blockIdx.x : (int)(blockIdx.x >> 1);   // the layouts' 16-column strip this workgroup works in
    if (VCW == VC) {
        const int nfull = (int)(gridDim.x / 32) * 32;
        // (round 3: only the passes that WRITE partial lines are remapped -- the plain pass of two right-hand sides reads
        // and writes whole lines, and with consecutive blocks on consecutive strips it runs 4 % faster)
        if ((EPI != EPI_PLANES || R == 1) && (int)blockIdx.x < nfull) {
            const int grp = blockIdx.x >> 5, w = blockIdx.x & 31;
            strip = (grp << 5) + ((w & 7) << 2) + (w >> 3);
        }
    }
    const unsigned c16 = 2u * (unsigned)xp + (VCW == VC ? 0u : 8u * (blockIdx.x & 1u));   // the thread's first column inside the strip
    const int col = strip * VC + (int)c16;           // < pitch by construction of the grid
    const size_t pb = (size_t)blockIdx.y * a.plane;
    const int r0 = cidx * M;
    const int h = a.len;                            // scanline length = ROI height

    // Addressing: wave-uniform plane bases (SGPRs) + 32-bit byte offsets per thread that walk down the
    // rows.  Keeping a 64-bit address per row alive from the loads to the stores would cost more
    // registers than the strip itself.
    //   C (Cvert)  strip-major [strip][row][16]: the strip's weights are one contiguous stream
    //   R == 2     pair plane [row pair][strip][row parity][U0 x16 | U1 x16]: a strip row is one full 128-byte
    //              line, two consecutive rows 256 contiguous bytes
    //   R == 1     plain row-major plane: a strip row is a 64-byte half line
    // (see fgs_wave_common.h; measured -17 % on the pass against three row-major planes)
    const char* bC = reinterpret_cast<const char*>(a.C + pb);
    char* b0 = reinterpret_cast<char*>(a.U0 + (R > 1 ? 2 * pb : pb));
    char* b1 = (R > 1) ? b0 + 4 * VC : nullptr;
    constexpr unsigned TR = TILE_ROWS;
    const unsigned voff0 = (R > 1) ? (((unsigned)r0 / TR) * (2u * TR * (unsigned)a.pitch) + (unsigned)strip * (32u * TR) + ((unsigned)r0 % TR) * 32u + c16) * 4u
                                   : ((unsigned)r0 * (unsigned)a.pitch + (unsigned)col) * 4u;
    const unsigned pitch_c = 4u * VC;
    const unsigned coff0 = (((unsigned)strip * (unsigned)h + (unsigned)r0) * VC + c16) * 4u;

    // both columns of a row in one register pair, from the 8-byte load to the 8-byte store (the chunk
    // templates of fgs_wave_common.h on v2f)
    v2f c[M], f0[M], f1[M];
    // row 0 of the column: always inside the planes
    const unsigned safe = (R > 1) ? ((unsigned)strip * (32u * TR) + c16) * 4u : (unsigned)col * 4u;
    const unsigned csafe = ((unsigned)strip * (unsigned)h * VC + c16) * 4u;
    v2f a_s = vsplat(0.0f);
    if (cidx > 0 && r0 - 1 < h) a_s = *reinterpret_cast<const v2f*>(bC + (coff0 - pitch_c)) * vsplat(a.lambda);
    // Rows past the end of the column are loaded from row 0 of the same column (always inside the
    // planes, no load under a divergent branch) and NOT masked: Cvert is 0 in the last row
    // (FGS.cpp:658-660), so whatever finite, diagonally dominant system those rows form is decoupled
    // from the real one by exact zeros (0 * finite), and the stores below skip them.  Untouched
    // loaded pairs stay where the load put them -- a select here would copy every pair.
    // IMG: the image holds all 64 * M rows of every strip, and the rows past the column's end are its padding -- zero
    // since the workspace was last laid out, which no kernel writes -- so they are loaded where they lie.
    {
        unsigned voff = voff0, coff = coff0;
        const v2f lam = vsplat(a.lambda);
        const char* bI = IMG ? reinterpret_cast<const char*>(a.image + (size_t)blockIdx.y * a.image_plane) : nullptr;
        unsigned ioff = (((unsigned)strip * (NCH / 8) + ((unsigned)tid >> 6)) * (unsigned)M) * 1024u + ((unsigned)tid & 63u) * 16u;
#pragma unroll
        for (int i = 0; i < M; i++) {
            const bool ok = r0 + i < h;
            c[i] = *reinterpret_cast<const v2f*>(bC + (ok ? coff : csafe));
            if constexpr (IMG) {
                const v4f q = *reinterpret_cast<const v4f*>(bI + ioff);
                f0[i] = (v2f){q.x, q.y}; f1[i] = (v2f){q.z, q.w};
                ioff += 1024u;
            } else {
                const unsigned vo = ok ? voff : safe;
                f0[i] = *reinterpret_cast<const v2f*>(b0 + vo);
                f1[i] = (R > 1) ? *reinterpret_cast<const v2f*>(b1 + vo) : vsplat(0.0f);
                voff += vstep<R>(r0, i, a.pitch);
            }
            coff += pitch_c;
            ADF_STEP_FENCE();   // one row's addresses at a time: hoisting all of them costs 2 registers per row
        }
#pragma unroll
        for (int i = 0; i < M; i++) c[i] *= lam;
    }

    Boundary<v2f, R> bd;
    chunk_boundary<M, R>(c, f0, f1, a_s, bd);
    *reinterpret_cast<v2f*>(&nb[0][cidx][2 * xp]) = bd.GS0;
    *reinterpret_cast<v2f*>(&nb[1][cidx][2 * xp]) = bd.GS1;
    *reinterpret_cast<v2f*>(&nb[2][cidx][2 * xp]) = bd.PS;
    *reinterpret_cast<v2f*>(&nb[3][cidx][2 * xp]) = bd.QS;
    __syncthreads();
    {
        v2f nGS0 = vsplat(0.f), nGS1 = nGS0, nPS = nGS0, nQS = nGS0;
        if (cidx < NCH - 1) {
            nGS0 = *reinterpret_cast<const v2f*>(&nb[0][cidx + 1][2 * xp]); nGS1 = *reinterpret_cast<const v2f*>(&nb[1][cidx + 1][2 * xp]);
            nPS = *reinterpret_cast<const v2f*>(&nb[2][cidx + 1][2 * xp]); nQS = *reinterpret_cast<const v2f*>(&nb[3][cidx + 1][2 * xp]);
        }
        v2f al, be, ga, p0, p1;
        separator_row<M, R>(c, f0, f1, bd, nGS0, nGS1, nPS, nQS, al, be, ga, p0, p1);
        red[0][2 * xp][cidx] = al.x; red[1][2 * xp][cidx] = be.x; red[2][2 * xp][cidx] = ga.x;
        red[3][2 * xp][cidx] = p0.x; red[4][2 * xp][cidx] = p1.x;
        red[0][2 * xp + 1][cidx] = al.y; red[1][2 * xp + 1][cidx] = be.y; red[2][2 * xp + 1][cidx] = ga.y;
        red[3][2 * xp + 1][cidx] = p0.y; red[4][2 * xp + 1][cidx] = p1.y;
    }
    __syncthreads();
    if constexpr (NCH == 64) {   // 8 wavefronts x 2 columns each: one separator row per lane
        const int wv = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int cc = 2 * wv + e;
            float x0, x1;
            pcr64<R>(lane, red[0][cc][lane], red[1][cc][lane], red[2][cc][lane], red[3][cc][lane], red[4][cc][lane], x0, x1);
            xs[0][cc][lane] = x0; xs[1][cc][lane] = x1;
        }
    } else {                     // 8 wavefronts, one column each: a 128-row system, two rows per lane
        const int cc = tid >> 6, lane = tid & 63;
        reduced128<R>(lane, red[0][cc], red[1][cc], red[2][cc], red[3][cc], red[4][cc], 1, xs[0][cc], xs[1][cc]);
    }
    __syncthreads();
    {
        const int cc = 2 * xp;
        const v2f xR0 = {xs[0][cc][cidx], xs[0][cc + 1][cidx]}, xR1 = {xs[1][cc][cidx], xs[1][cc + 1][cidx]};
        v2f xL0 = vsplat(0.0f), xL1 = xL0;
        if (cidx > 0) {
            xL0 = (v2f){xs[0][cc][cidx - 1], xs[0][cc + 1][cidx - 1]};
            xL1 = (v2f){xs[1][cc][cidx - 1], xs[1][cc + 1][cidx - 1]};
        }
        chunk_solve<M, R>(c, f0, f1, a_s, xL0, xL1, xR0, xR1);
    }

    unsigned voff = voff0;
    asm volatile("" : "+v"(voff)); // recompute the row offsets instead of keeping the load addresses alive
    if (EPI == EPI_PLANES) {
#pragma unroll
        for (int i = 0; i < M; i++) {
            if (r0 + i < h) {
                *reinterpret_cast<v2f*>(b0 + voff) = f0[i];
                if (R > 1) *reinterpret_cast<v2f*>(b1 + voff) = f1[i];
            }
            voff += vstep<R>(r0, i, a.pitch);
        }
    } else {
        // (opaque copies made AFTER the solve: nothing of the epilogue's addressing may be formed while the strip
        // and the sweeps' temporaries fill the register file)
        int r0e = r0, cole = col;
        asm volatile("" : "+v"(r0e), "+v"(cole));
        char* ob = reinterpret_cast<char*>(a.out) + (ptrdiff_t)blockIdx.y * a.out_pair_stride +
                   (ptrdiff_t)(a.out_y0 + r0e) * a.out_stride;
        const int esz = (EPI == EPI_F32 || EPI == EPI_WLS_CONF_F32) ? 4 : (EPI == EPI_U8) ? 1 : 2;
        unsigned ooff = (unsigned)((a.out_x0 + cole) * a.out_cn + a.out_c) * (unsigned)esz;
        // Single-channel int16 output with an even number of columns (every call of the disparity filter on an even-width
        // ROI): both columns of the thread go out as one packed dword -- or, when the ROI starts on an odd column (the
        // StereoBM factory's ROIs do: DF.cpp:401), as its two halves -- with no per-row alignment test and no branch but
        // the row mask.  Round 3: the general loop below spent 4.5 us per strip (of 38) on IEEE divisions, conversions
        // and exec-mask branches (profiles/r03_vphase.txt).  All three conditions are uniform over the launch.
        // Round 4: an ODD number of columns takes the same path -- the one thread per strip row that holds the ROI's last
        // column stores its low half only (2 bytes), everything else is unchanged.
        const bool fast16 = (EPI == EPI_WLS_CONF || EPI == EPI_I16) && a.out_cn == 1;
        // Single-channel float output (adf_wls_filter_f32_*, a one-channel generic smoother): the same, as one float2
        // -- the eight column pairs of a strip row are one contiguous 64-byte piece -- or as two dwords.
        const bool fast32 = (EPI == EPI_WLS_CONF_F32 || (EPI == EPI_F32 && R == 1)) && a.out_cn == 1;
        if (fast16 || fast32) {
            const int hv2 = (cole + 1 < a.nscan ? h : 0) - r0e;   // rows of a thread with two columns inside the ROI
            const int hv1 = (cole + 1 == a.nscan ? h : 0) - r0e;  // ... with only its first column inside
            char* dst = ob + ooff;
            if (fast16 && (a.nscan & 1)) store_rows<EPI, false, true>(f0, f1, dst, a.out_stride, out_pairs_aligned(a, 2), hv2, hv1);
            else if (fast16) {
                const int hv = (cole < a.nscan ? h : 0) - r0e;    // rows of this thread to store (threads on pitch padding: none)
                if (out_pairs_aligned(a, 2)) store_rows<EPI, false, false>(f0, f1, dst, a.out_stride, true, hv, 0);
                else store_rows<EPI, false, false>(f0, f1, dst, a.out_stride, false, hv, 0);
            } else if (out_pairs_aligned(a, 4)) store_rows<EPI, true, true>(f0, f1, dst, a.out_stride, true, hv2, hv1);
            else store_rows<EPI, true, true>(f0, f1, dst, a.out_stride, false, hv2, hv1);
        } else if (EPI != EPI_WLS_CONF_F32) {   // (the ratio as a float is single-channel only: launch_wave_vpass)
#pragma unroll
        for (int i = 0; i < M; i++) {
            if (r0 + i < h) {
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    if (col + e < a.nscan) {
                        char* dst = ob + ooff + (unsigned)(e * a.out_cn * esz);
                        if (EPI == EPI_WLS_CONF) {
                            const float rcp = 1.0f / (f1[i][e] + ADF_EPS);             // DF.cpp:295
                            *reinterpret_cast<int16_t*>(dst) = sat16(f0[i][e] * rcp);  // DF.cpp:296
                        } else {
                            // generic FGS (FGS.cpp:216-218): with two right-hand sides the second one is
                            // the next interleaved channel of the same image
#pragma unroll
                            for (int r = 0; r < R; r++) {
                                const float x = r ? f1[i][e] : f0[i][e];
                                char* d = dst + r * esz;
                                if (EPI == EPI_I16) *reinterpret_cast<int16_t*>(d) = sat16(x);
                                else if (EPI == EPI_U8) *reinterpret_cast<uint8_t*>(d) = sat8(x);
                                else *reinterpret_cast<float*>(d) = x;
                            }
                        }
                    }
                }
            }
            ooff += (unsigned)a.out_stride;
        }
        }
    }
}

template <int M, int VCW = VC, int NCH = 64>
hipError_t launch_v(const WavePassArgs& a, int n_rhs, int epi, int n_pairs, hipStream_t st)
{
    dim3 grid(a.pitch / VCW, n_pairs), block(VT);
    constexpr int N_EPI = N_EPILOGUES;
    if (n_rhs < 1 || n_rhs > 2 || epi < 0 || epi >= N_EPI) return hipErrorInvalidValue;
    return dispatch_index<2 * N_EPI>((n_rhs - 1) * N_EPI + epi, [&](auto K) {
        constexpr int R = decltype(K)::value / N_EPI + 1, EPI = decltype(K)::value % N_EPI;
        // (two right-hand sides with a generic epilogue: channel pairs of a generic FGS source)
        if constexpr (R == 1 && (EPI == EPI_WLS_CONF || EPI == EPI_WLS_CONF_F32)) return hipErrorInvalidValue;   // the ratio needs both right-hand sides
        else {
            if (a.image) {   // a hand-off's image: whole strips, the plain pass or the filter's epilogues, the image laid out for this bucket
                if constexpr (R == 2 && VCW == VC && (EPI == EPI_PLANES || EPI == EPI_WLS_CONF || EPI == EPI_WLS_CONF_F32)) {
                    if (a.image_m != M || a.image_plane < wave_image_floats(a.pitch, M)) return hipErrorInvalidValue;
                    hipLaunchKernelGGL((wave_vpass_kernel<M, R, EPI, VCW, NCH, true>), grid, block, 0, st, a);
                    return hipGetLastError();
                } else return hipErrorInvalidValue;
            }
            hipLaunchKernelGGL((wave_vpass_kernel<M, R, EPI, VCW, NCH>), grid, block, 0, st, a);
            return hipGetLastError();
        }
    });
}

// The column buckets: full strips of 64 chunks up to 2176 rows, half strips of 128 chunks above.
constexpr Bucket COL_BUCKETS[] = {{2, 64}, {4, 64}, {8, 64}, {12, 64}, {18, 64}, {26, 64}, {34, 64}, {20, 128}, {26, 128}, {34, 128}};
constexpr int N_COL_BUCKETS = sizeof(COL_BUCKETS) / sizeof(COL_BUCKETS[0]);

} // namespace

int wave_max_col_len() { return COL_BUCKETS[N_COL_BUCKETS - 1].m * COL_BUCKETS[N_COL_BUCKETS - 1].chunks; }

int wave_vpass_image_m(int col_len)
{
    if (col_len < 2 || col_len > wave_max_col_len()) return 0;
    const Bucket& b = COL_BUCKETS[bucket_index(COL_BUCKETS, col_len)];
    return b.chunks == 64 ? b.m : 0;
}

hipError_t launch_wave_vpass(const WavePassArgs& a, int n_rhs, int epilogue, int n_pairs, hipStream_t st)
{
    if (a.len < 2 || a.len > wave_max_col_len() || a.pitch % 64 != 0 || a.pitch < a.nscan) return hipErrorInvalidValue;
    if (epilogue == EPI_WLS_CONF_F32 && a.out_cn != 1) return hipErrorInvalidValue;
    return dispatch_index<N_COL_BUCKETS>(bucket_index(COL_BUCKETS, a.len), [&](auto I) {
        constexpr Bucket b = COL_BUCKETS[decltype(I)::value];
        return launch_v<b.m, b.chunks == 64 ? VC : VC / 2, b.chunks>(a, n_rhs, epilogue, n_pairs, st);
    });
}

} // namespace adf
