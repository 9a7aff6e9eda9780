// fgs_wave_h.hip -- horizontal pass of the on-chip partitioned solver (see fgs_wave_common.h).
#include "fgs_wave_common.h"
#include "prep_bodies.h"

#include <algorithm>

namespace adf {

namespace {
using namespace wave;

constexpr int H_TWO_WAVE_MAX = 60;   // longest chunk whose two-right-hand-side kernel fits two waves per SIMD

// ---------------------------------------------------------------------------------------------
// Horizontal pass: one wavefront per row (two beyond 4096 columns), in place.  wave_hpass_kernel reads
//   load -> transpose in -> boundary exchange -> reduced system -> chunk_solve -> store,
// and the stages are the functions below, in that order.
// ---------------------------------------------------------------------------------------------
// Where the row's right-hand sides come from (FUSED):
//  FUSE_NONE     the planes (load_planes).
//  FUSE_VIEW     first pass of a confidence-mode call: formed on the fly from the confidence plane and the left
//                disparity map, U1 = conf, U0 = conf*float(dL) (DF.cpp:288-290), instead of being read from planes a
//                prologue kernel would have had to write (load_fused_view).
//  FUSE_LO       the down-scaled path's first pass: the maps are LOW-resolution (the sample's default: matcher on
//                half-size views) and cv::resize is part of the prologue (load_fused_lo).  The two view-sized planes the
//                resize kernels wrote (6 B/px) and this pass read back (6 B/px) never exist.
//  FUSE_LO_HALF  FUSE_LO for maps of exactly half the view's width on a ROI that starts on an even column >= 2
//                (lo_interp4).  Same operands, same arithmetic: bit-identical to FUSE_LO (tests).
//  FUSE_VIEW_F32 FUSE_VIEW on a CV_32FC1 left map (fused_f32_conf, fused_f32_map): every bucket and weight source FUSE_VIEW has.
constexpr int FUSE_NONE = 0, FUSE_VIEW = 1, FUSE_LO = 2, FUSE_LO_HALF = 3, FUSE_VIEW_F32 = 4;
// Where the row's weights come from (WS):
//  WS_PLANE            the Chor plane the weight kernel wrote (load_c, transpose_in).
//  WS_GUIDE1 / _GUIDE3 the guide row itself, one or three channels (guide_fetch, guide_weights): Chor is a pure function
//                      of it, 1 or 3 bytes per pixel to read where the plane costs 4 to write and 4 in every row pass.
//                      One-wave rows, FUSE_NONE and FUSE_VIEW.  Same table entry, same multiply: bit-identical c[].
constexpr int WS_PLANE = 0, WS_GUIDE1 = 1, WS_GUIDE3 = 3;   // (a guide form's value is its channel count)

typedef float v4f __attribute__((ext_vector_type(4)));

// Where a wavefront stands in its row and where the row lies in the planes (all but `lane` are wave-uniform).
// Two right-hand sides live in ONE pair plane, interleaved per 16 columns ([U0 x16 | U1 x16] per strip, see
// fgs_wave_common.h): a row is 2*pitch floats, and rows come in tiles of TILE_ROWS -- float4 #q of pair row r lives
// at (r/TR)*(TR*nvecU) + (q/8)*8*TR + (r%TR)*8 + q%8, i.e. at offU + pair_vec(q).
struct RowPos {
    int lane, wv;
    int v0;          // first float4 of this wave's columns in a row-major row
    int nvec;        // float4s of a row-major row
    int nvecU;       // float4s of a row of the right-hand sides: 2 * nvec in the pair plane
    size_t off;      // the row's first float in a single plane (C; U0 when there is one right-hand side)
    size_t offU;     // ... in the plane of the right-hand sides
};

template <int M, bool PAIR, int NW>
__device__ __forceinline__ RowPos row_pos(const WavePassArgs& a)
{
    constexpr int TR = TILE_ROWS;
    RowPos p;
    p.lane = threadIdx.x & 63; p.wv = NW == 2 ? (int)(threadIdx.x >> 6) : 0;
    p.v0 = p.wv * 16 * M;
    p.off = (size_t)blockIdx.y * a.plane + (size_t)blockIdx.x * a.pitch;
    p.nvec = a.pitch >> 2;
    p.offU = PAIR ? (size_t)blockIdx.y * 2 * a.plane + (size_t)(blockIdx.x / TR) * (size_t)(2 * TR * a.pitch) + (size_t)(blockIdx.x % TR) * 32 : p.off;
    p.nvecU = PAIR ? 2 * p.nvec : p.nvec;
    return p;
}

// float4 #q of a row of the right-hand sides, counted from the row's first float4
template <bool PAIR>
__device__ __forceinline__ constexpr int rhs_vec(int q) { return PAIR ? (((q >> 3) * (8 * TILE_ROWS)) + (q & 7)) : q; }

// Pair plane, half a row (2M strips of [U0 x16 | U1 x16]) in the staging buffer: the float4 that holds U0 of columns
// j .. j+3 of the half (j a multiple of 4); U1 of the same columns is 4 float4s behind it.
__device__ __forceinline__ constexpr int pair_slot(int j) { return ((j >> 4) << 3) + ((j & 15) >> 2); }

// Non-temporal: every byte of a row pass is used exactly once (measured -5 % on the pass).
__device__ __forceinline__ float4 load_nt(const float4* p)
{
    const v4f q = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(q.x, q.y, q.z, q.w);
}
__device__ __forceinline__ void store_nt(float4 q, float4* p)
{
    const v4f o = {q.x, q.y, q.z, q.w};
    __builtin_nontemporal_store(o, reinterpret_cast<v4f*>(p));
}

// ---- load: the row as float4 #(64k + lane) of the wave's columns, tC / t0 / t1 ----
// All of the row's coalesced loads (16 B per lane, 1 KiB per instruction) are issued before the
// first use so that a row pays one memory latency, not one per plane; each plane is then turned
// from "float4 #(64k+lane)" into "chunk of lane" through the wave's LDS staging buffer.
// Columns [len, pitch) of every plane are zero by construction (the host zeroes the workspace
// whenever the geometry changes and no kernel writes non-zeros there), and float4s past the pitch
// are loaded as zeros: the tail of the row is identity rows without masks.

// The wave's float4 #k of the C row.
// (an explicit branch per load: "cond ? *p : zero" would make the compiler select between
// addresses and park the zero in scratch memory)
__device__ __forceinline__ float4 load_c(const WavePassArgs& a, const RowPos& p, int k)
{
    const int idx = p.v0 + 64 * k + p.lane;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < p.nvec) t = load_nt(reinterpret_cast<const float4*>(a.C + p.off) + idx);
    return t;
}

// FUSE_NONE.  One right-hand side: t0 = U0, t1 = 0.  Two: t0 / t1 hold the first / second half of this wave's part
// of the interleaved pair row (2 * M * 64 floats) instead of U0 / U1.
template <int M, int R, bool WITH_C>
__device__ __forceinline__ void load_planes(const WavePassArgs& a, const RowPos& p, float4 (&tC)[M / 4], float4 (&t0)[M / 4], float4 (&t1)[M / 4])
{
    constexpr bool PAIR = R > 1;
    constexpr int MQ = M / 4;
    const float4* s0 = reinterpret_cast<const float4*>(a.U0 + p.offU);
    const int u0 = PAIR ? 2 * p.v0 : p.v0;
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        const int uidx = u0 + 64 * k + p.lane;
        if constexpr (WITH_C) tC[k] = load_c(a, p, k);
        t0[k] = make_float4(0.f, 0.f, 0.f, 0.f); t1[k] = t0[k];
        if (uidx < p.nvecU) t0[k] = load_nt(s0 + rhs_vec<PAIR>(uidx));
        if (PAIR && uidx + 64 * MQ < p.nvecU) t1[k] = load_nt(s0 + rhs_vec<PAIR>(uidx + 64 * MQ));
    }
}

// float4s of a fused row: ceil(len / 4)
__device__ __forceinline__ int fused_vecs(int len) { return (len >> 2) + ((len & 3) ? 1 : 0); }

// FUSE_VIEW: t1 = conf, t0 = conf * float(dL) (DF.cpp:288-290) from the view-resolution confidence plane and the
// caller's left disparity map (a.fuse.conf_* / dl_*).  The launcher guarantees a 16-byte aligned conf row start and
// len >= 4 (wave_hpass_can_fuse): conf (the library's own plane, Geom::cx0 / cpitch) is always 16-byte aligned, dL is
// the caller's and only 2-byte aligned for an odd ROI x (8-byte loads at any even address).
// A ROI width that is not a multiple of 4 ends in a partial vector: its dL load is moved back so that it
// ends with the row (never past the caller's buffer) and shifted into place afterwards, its conf elements
// past the row are cleared -- both in the second loop, behind one wave-uniform branch, so that no loaded
// value is touched while loads are still being issued.
template <int M, bool WITH_C>
__device__ __forceinline__ void load_fused_view(const WavePassArgs& a, const RowPos& p, float4 (&tC)[M / 4], float4 (&t0)[M / 4], float4 (&t1)[M / 4])
{
    constexpr int MQ = M / 4;
    typedef short v4s_u __attribute__((ext_vector_type(4), aligned(2)));
    const float4* sF = reinterpret_cast<const float4*>(a.fuse.conf_in + (size_t)blockIdx.y * a.fuse.conf_frame +
                                                       (size_t)(a.fuse.conf_y0 + blockIdx.x) * a.fuse.conf_pitch + a.fuse.conf_x0);
    const char* sD = reinterpret_cast<const char*>(a.fuse.dl_in) + (ptrdiff_t)blockIdx.y * a.fuse.dl_pair_stride +
                     (ptrdiff_t)(a.fuse.dl_y0 + blockIdx.x) * a.fuse.dl_stride + (ptrdiff_t)a.fuse.dl_x0 * 2;
    const int nfull = a.len >> 2, rem = a.len & 3;
    const int nfused = fused_vecs(a.len);
    const unsigned dl_last = (unsigned)a.len * 2u - 8u;      // byte offset of the last whole vector (len >= 4)
    short4 draw[MQ];                                         // the row of the left disparity map
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        const int idx = p.v0 + 64 * k + p.lane;
        if constexpr (WITH_C) tC[k] = load_c(a, p, k);
        t0[k] = make_float4(0.f, 0.f, 0.f, 0.f); t1[k] = t0[k];
        draw[k] = make_short4(0, 0, 0, 0);
        // loads only: the products conf*float(dL) wait for the second loop, or every iteration would
        // wait for its own loads before the next one's are issued (14 memory latencies per row)
        if (idx < nfused) {
            const unsigned doff = min((unsigned)idx * 8u, dl_last);
            t1[k] = load_nt(sF + idx);
            const v4s_u dq = __builtin_nontemporal_load(reinterpret_cast<const v4s_u*>(sD + doff));
            draw[k] = make_short4(dq.x, dq.y, dq.z, dq.w);
        }
    }
    const int tl = nfull - p.v0;                             // the partial vector, counted from this wave's first
    const int ktail = (rem && tl >= 0 && tl < 16 * M) ? (tl >> 6) : -1;   // wave-uniform: the one k that holds it
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        if (k == ktail && p.lane == (tl & 63)) {             // elements rem..3 lie past the row
            const int sh = 16 * (4 - rem);
            unsigned long long w = (unsigned long long)(unsigned short)draw[k].x | ((unsigned long long)(unsigned short)draw[k].y << 16) |
                                   ((unsigned long long)(unsigned short)draw[k].z << 32) | ((unsigned long long)(unsigned short)draw[k].w << 48);
            w >>= sh;
            draw[k] = make_short4((short)(w & 0xffff), (short)((w >> 16) & 0xffff), (short)((w >> 32) & 0xffff), (short)(w >> 48));
            if (rem < 2) t1[k].y = 0.0f;
            if (rem < 3) t1[k].z = 0.0f;
            t1[k].w = 0.0f;
        }
        t0[k] = make_float4(t1[k].x * (float)draw[k].x, t1[k].y * (float)draw[k].y, t1[k].z * (float)draw[k].z, t1[k].w * (float)draw[k].w);
    }
}

// FUSE_VIEW_F32: FUSE_VIEW on a CV_32FC1 left map (adf_wls_filter_typed_*): t0 = conf * v, v = wls_input_value(dL), ONE
// float multiply where the int16 form has conf * float(dL).  One 16-byte load per lane and vector at any 4-byte aligned
// address, landing in t0 itself.  Two steps, each "loads only, then arithmetic": fused_f32_conf issues the confidence
// (and weight) loads, fused_f32_map the map's loads and then forms the clamp, the partial vector and the products.  The
// kernel runs them back to back -- every load of the row in flight at once, as in the int16 form -- except in the guide
// forms of the long buckets (fused_f32_defer), where a map row in flight is 2 registers per vector more than the int16
// form's and the weights' table look-ups would spill: there the map is loaded once the weights are made.
// The partial last vector is loaded so that it ends with the row (len >= 4), never past the caller's buffer, and its
// elements are moved down; what lies past the row becomes 0.0f * 0.0f, the +0 the int16 form leaves there.
constexpr bool fused_f32_defer(int m, bool guide) { return guide && m >= 56; }

template <int M, bool WITH_C>
__device__ __forceinline__ void fused_f32_conf(const WavePassArgs& a, const RowPos& p, float4 (&tC)[M / 4], float4 (&t1)[M / 4])
{
    constexpr int MQ = M / 4;
    const float4* sF = reinterpret_cast<const float4*>(a.fuse.conf_in + (size_t)blockIdx.y * a.fuse.conf_frame +
                                                       (size_t)(a.fuse.conf_y0 + blockIdx.x) * a.fuse.conf_pitch + a.fuse.conf_x0);
    const int nfused = fused_vecs(a.len);
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        const int idx = p.v0 + 64 * k + p.lane;
        if constexpr (WITH_C) tC[k] = load_c(a, p, k);
        t1[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < nfused) t1[k] = load_nt(sF + idx);
    }
}

template <int M>
__device__ __forceinline__ void fused_f32_map(const WavePassArgs& a, const RowPos& p, float4 (&t0)[M / 4], float4 (&t1)[M / 4])
{
    constexpr int MQ = M / 4;
    typedef float v4f_u __attribute__((ext_vector_type(4), aligned(4)));
    const char* sD = reinterpret_cast<const char*>(a.fuse.dl_in) + (ptrdiff_t)blockIdx.y * a.fuse.dl_pair_stride +
                     (ptrdiff_t)(a.fuse.dl_y0 + blockIdx.x) * a.fuse.dl_stride + (ptrdiff_t)a.fuse.dl_x0 * 4;
    const int nfull = a.len >> 2, rem = a.len & 3;
    const int nfused = fused_vecs(a.len);
    const unsigned dl_last = (unsigned)a.len * 4u - 16u;     // byte offset of the last whole vector (len >= 4)
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        const int idx = p.v0 + 64 * k + p.lane;
        t0[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < nfused) {
            const unsigned doff = min((unsigned)idx * 16u, dl_last);
            const v4f_u dq = __builtin_nontemporal_load(reinterpret_cast<const v4f_u*>(sD + doff));
            t0[k] = make_float4(dq.x, dq.y, dq.z, dq.w);
        }
    }
    const int tl = nfull - p.v0;                             // the partial vector, counted from this wave's first
    const int ktail = (rem && tl >= 0 && tl < 16 * M) ? (tl >> 6) : -1;   // wave-uniform: the one k that holds it
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        if (k == ktail && p.lane == (tl & 63)) {             // the vector holds columns len-4 .. len-1: keep the last `rem`
            const float4 d = t0[k];
            t0[k] = rem == 1 ? make_float4(d.w, 0.f, 0.f, 0.f) : rem == 2 ? make_float4(d.z, d.w, 0.f, 0.f) : make_float4(d.y, d.z, d.w, 0.f);
            if (rem < 2) t1[k].y = 0.0f;
            if (rem < 3) t1[k].z = 0.0f;
            t1[k].w = 0.0f;
        }
        t0[k] = make_float4(t1[k].x * wls_input_value(t0[k].x), t1[k].y * wls_input_value(t0[k].y),
                            t1[k].z * wls_input_value(t0[k].z), t1[k].w * wls_input_value(t0[k].w));
    }
}

// cv::resize's INTER_LINEAR tap of destination index d: source index s0 (and s0 + 1) with weights (1 - fx, fx);
// borders clamp with weight (1, 0).  Same operations, same order as resize_linear_kernel / the oracle (host and device).
__host__ __device__ __forceinline__ void lin_tap(int d, double scale, int sn, int& s0, float& fx)
{
    fx = (float)(((double)d + 0.5) * scale - 0.5);
    s0 = (int)floorf(fx);
    fx -= (float)s0;
    if (s0 < 0) { fx = 0.0f; s0 = 0; }
    if (s0 >= sn - 1) { fx = 0.0f; s0 = sn - 1; }
}
// The taps of a call's ROI columns are the same for every row and every pair: lo_tap_table_kernel forms them once per
// call (the double arithmetic and the conversions are slow instructions; per row they cost more than the interpolation).
// table[j], j < n (n = the row's float4 count * 4) = the tap of ROI column min(j, len - 1) as ONE float: the source
// coordinate with the border rules already applied -- s0 + fx, which is exact: fx is what the coordinate's own
// fraction bits hold -- so that the row pass recovers s0 = (int)t and fx = fract(t) in two instructions.
__global__ void __launch_bounds__(256) lo_tap_table_kernel(float* table, int n, int len, int hi_x0, double scale, int sn)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int s0; float fx;
    lin_tap(hi_x0 + min(j, len - 1), scale, sn, s0, fx);
    table[j] = (float)s0 + fx;
}
// floats per staged confidence row = shorts per staged disparity row: two of each fit the wave's M*256-byte buffer
// (the shortest bucket's buffer is enlarged instead: its single float4 group per lane spans 256 columns)
__host__ __device__ constexpr int lo_row_cap(int m) { return (((m * 64) / 3) & ~7) < 168 ? 168 : (((m * 64) / 3) & ~7); }
__host__ __device__ constexpr int lo_stage_vec4(int m) { return 12 * lo_row_cap(m) > 256 * m ? (12 * lo_row_cap(m) + 15) / 16 : m * 16; }

// ---- FUSE_LO / FUSE_LO_HALF: the low-resolution prologue ----
// The two source rows an output row taps (confidence and left disparity) are staged in the wave's LDS buffer,
// coalesced, one half of the wave's columns at a time, and every lane interpolates its own columns from there with
// the exact tap arithmetic of resize_kernels.hip.
template <int M>
struct LoShape {
    static constexpr int MQ = M / 4;
    static constexpr int KH = (MQ + 1) / 2;                   // float4 groups of the first half of the wave's columns
    static constexpr int CROW = lo_row_cap(M);
    static constexpr int TC4 = (CROW / 4 + 63) / 64, TD8 = (CROW / 8 + 63) / 64;   // vectors per lane of a staged row
    static_assert(12 * CROW <= 16 * lo_stage_vec4(M) && CROW % 8 == 0, "two confidence rows and two disparity rows fit the staging buffer");
};
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef short s8u __attribute__((ext_vector_type(8), aligned(2)));

// One half's two source rows as the lanes fetched them: lane i holds source elements ss + 4i .. of the confidence
// rows, ss + 8i .. of the disparity rows.
template <int M>
struct LoRaw { v4f c[2][LoShape<M>::TC4]; s8u d[2][LoShape<M>::TD8]; };

// What an output row's prologue knows before it loads anything (all wave-uniform).
struct LoRow {
    int yr[2];            // the two source rows (clamped; rows clamp with their weights kept, like the resize kernel)
    float b0, b1;         // ... and their weights
    // per half of the wave's columns: first source element and number of staged slots (the slot behind the last tap
    // included: past the row's end it repeats the edge element, which carries weight 0; 0 for an empty half)
    int ss[2], ns[2];
    // does a staged element of the half lie outside the confidence map's window?  Zero-window masks are applied only
    // where a half's staged span leaves the window.
    bool need_mask[2];
};

template <int M>
__device__ __forceinline__ LoRow lo_row(const FusedInputs& f, int wv, int len)
{
    constexpr int MQ = LoShape<M>::MQ, KH = LoShape<M>::KH;
    const int sw = f.lo_w, sh = f.lo_h;
    LoRow r;
    int sy; float fy;
    {
        const int dy = f.hi_y0 + (int)blockIdx.x;
        fy = (float)(((double)dy + 0.5) * f.lo_scale_y - 0.5);
        sy = (int)floorf(fy);
        fy -= (float)sy;
    }
    r.b0 = 1.0f - fy; r.b1 = fy;
    r.yr[0] = min(max(sy, 0), sh - 1); r.yr[1] = min(max(sy + 1, 0), sh - 1);
    r.yr[0] = __builtin_amdgcn_readfirstlane(r.yr[0]); r.yr[1] = __builtin_amdgcn_readfirstlane(r.yr[1]);
#pragma unroll
    for (int hh = 0; hh < 2; hh++) {
        const int cfirst = 64 * M * wv + 256 * (hh ? KH : 0);
        const int clast = min(64 * M * wv + 256 * (hh ? MQ : KH), len) - 1;
        int s_first = 0, s_last = -2; float f_;
        if (clast >= cfirst) { lin_tap(f.hi_x0 + cfirst, f.lo_scale_x, sw, s_first, f_); lin_tap(f.hi_x0 + clast, f.lo_scale_x, sw, s_last, f_); }
        r.ss[hh] = __builtin_amdgcn_readfirstlane(s_first);
        r.ns[hh] = __builtin_amdgcn_readfirstlane(s_last + 2 - s_first);
    }
#pragma unroll
    for (int hh = 0; hh < 2; hh++)
        r.need_mask[hh] = f.lo_zero_outside && (r.yr[0] < f.lo_vy0 || r.yr[1] >= f.lo_vy1 || r.ss[hh] < f.lo_vx0 || min(r.ss[hh] + r.ns[hh], sw) > f.lo_vx1);
    return r;
}

// Half hh's two source rows, global memory -> registers: coalesced; a vector that would cross the row's end is fetched
// element by element, clamped, which also fills the slots behind the row with the edge element.
template <int M>
__device__ inline void lo_fetch(const FusedInputs& f, const LoRow& row, int hh, int lane, LoRaw<M>& q)
{
    const int sw = f.lo_w;
    const float* cbase = f.lo_conf + (ptrdiff_t)blockIdx.y * f.lo_conf_pair;
    const char* dbase = reinterpret_cast<const char*>(f.lo_dl) + (ptrdiff_t)blockIdx.y * f.lo_dl_pair;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const float* crow = cbase + (ptrdiff_t)row.yr[r] * f.lo_conf_stride;
        const int16_t* drow = reinterpret_cast<const int16_t*>(dbase + (ptrdiff_t)row.yr[r] * f.lo_dl_stride);
#pragma unroll
        for (int t = 0; t < LoShape<M>::TC4; t++) {
            const int e = row.ss[hh] + 4 * (64 * t + lane);
            q.c[r][t] = v4f{0.f, 0.f, 0.f, 0.f};
            if (4 * (64 * t + lane) < row.ns[hh]) {
                if (e + 3 < sw) q.c[r][t] = *reinterpret_cast<const f4u*>(crow + e);
                else {
#pragma unroll
                    for (int c = 0; c < 4; c++) q.c[r][t][c] = crow[min(e + c, sw - 1)];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < LoShape<M>::TD8; t++) {
            const int e = row.ss[hh] + 8 * (64 * t + lane);
            q.d[r][t] = s8u{0, 0, 0, 0, 0, 0, 0, 0};
            if (8 * (64 * t + lane) < row.ns[hh]) {
                if (e + 7 < sw) q.d[r][t] = *reinterpret_cast<const s8u*>(drow + e);
                else {
#pragma unroll
                    for (int c = 0; c < 8; c++) q.d[r][t][c] = drow[min(e + c, sw - 1)];
                }
            }
        }
    }
}

// Half hh's fetched rows, registers -> the wave's staging buffer (confidence outside the map's window zeroed).
// LDS layout: slot s of the half holds (row0[s], row1[s]) -- two floats of the confidence rows, then, behind
// all confidence slots, two shorts of the disparity rows -- so that a tap's four values (slots s and s + 1
// of both rows) are ONE 16-byte / ONE 8-byte read, and a lane, which holds the same source elements of
// both rows, stages them with whole 16-byte writes.
template <int M>
__device__ inline void lo_put(const FusedInputs& f, const LoRow& row, int hh, int lane, const LoRaw<M>& q, float4* stage)
{
    constexpr int CROW = LoShape<M>::CROW;
    typedef short s8a __attribute__((ext_vector_type(8)));
    v4f* Lf4 = reinterpret_cast<v4f*>(stage);
    s8a* Ls8 = reinterpret_cast<s8a*>(stage) + CROW / 2;     // behind the 2 * CROW confidence floats
    const int sw = f.lo_w;
    const bool rin0 = !f.lo_zero_outside || (row.yr[0] >= f.lo_vy0 && row.yr[0] < f.lo_vy1);
    const bool rin1 = !f.lo_zero_outside || (row.yr[1] >= f.lo_vy0 && row.yr[1] < f.lo_vy1);
#pragma unroll
    for (int t = 0; t < LoShape<M>::TC4; t++) {
        const int i4 = 64 * t + lane, e = row.ss[hh] + 4 * i4;
        v4f q0 = q.c[0][t], q1 = q.c[1][t];
        if (row.need_mask[hh]) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int ec = min(e + c, sw - 1);
                const bool cin = ec >= f.lo_vx0 && ec < f.lo_vx1;
                if (!(rin0 && cin)) q0[c] = 0.0f;
                if (!(rin1 && cin)) q1[c] = 0.0f;
            }
        }
        if (4 * i4 < CROW) {
            Lf4[2 * i4] = v4f{q0[0], q1[0], q0[1], q1[1]};
            Lf4[2 * i4 + 1] = v4f{q0[2], q1[2], q0[3], q1[3]};
        }
    }
#pragma unroll
    for (int t = 0; t < LoShape<M>::TD8; t++) {
        const int i8 = 64 * t + lane;
        const s8u q0 = q.d[0][t], q1 = q.d[1][t];
        if (8 * i8 < CROW) {
            Ls8[2 * i8] = s8a{q0[0], q1[0], q0[1], q1[1], q0[2], q1[2], q0[3], q1[3]};
            Ls8[2 * i8 + 1] = s8a{q0[4], q1[4], q0[5], q1[5], q0[6], q1[6], q0[7], q1[7]};
        }
    }
}

// Half hh's taps from the launcher's table (one float per column, the same for every row of the call: L2 hits).
template <int M>
__device__ inline void lo_load_taps(const WavePassArgs& a, const RowPos& p, int hh, v4f (&tp)[M / 4])
{
    constexpr int MQ = LoShape<M>::MQ, KH = LoShape<M>::KH;
    const int nfused = fused_vecs(a.len);
#pragma unroll
    for (int k = (hh ? KH : 0); k < (hh ? MQ : KH); k++) {
        const int idx = p.v0 + 64 * k + p.lane;
        tp[k] = v4f{0.f, 0.f, 0.f, 0.f};
        if (idx < nfused) tp[k] = reinterpret_cast<const v4f*>(a.fuse.lo_taps)[idx];
    }
}

// The four columns of float4 #(vec0 + lane) of the row, interpolated from half hh's staged rows at the taps tpk:
// u1 = conf, u0 = conf * float(dL) (DF.cpp:288-290); columns behind the row's end are zero.
// HALF (maps of exactly half the view's width, ROI on an even column >= 2): the four columns share FOUR consecutive
// source elements whatever the lane -- columns 2m, 2m+1, 2m+2, 2m+3 tap (m-1, m), (m, m+1), (m, m+1), (m+1, m+2) -- so
// the group makes three LDS reads instead of eight and decodes one tap position instead of four.
template <int M, bool HALF>
__device__ inline void lo_interp4(const WavePassArgs& a, const LoRow& row, int hh, const float4* stage, v4f tpk, int vec0, int lane,
                                           float4& u0, float4& u1)
{
    const int idx = vec0 + lane;                              // vec0: the group's float4 of lane 0
    constexpr int CROW = LoShape<M>::CROW;
    typedef float f4a8 __attribute__((ext_vector_type(4), aligned(8)));
    typedef short s4a4 __attribute__((ext_vector_type(4), aligned(4)));
    const float* Lf = reinterpret_cast<const float*>(stage);
    const short* Ls = reinterpret_cast<const short*>(stage) + 4 * CROW;      // behind the 2 * CROW confidence floats
    const v2f bb0 = {row.b0, row.b0}, bb1 = {row.b1, row.b1};
    const bool post_scaled = a.fuse.lo_post_scale != 1.0f;
    // all four columns' staged values first (eight LDS reads in flight), the arithmetic afterwards
    f4a8 cq[4]; s4a4 dq[4]; float fxs[4];
    if constexpr (HALF) {
        typedef short s8a4 __attribute__((ext_vector_type(8), aligned(4)));
        // (the group's first column taps m - 1: in range by construction, clamped like the general form)
        const int sl0 = min(max((int)tpk[0] - row.ss[hh], 0), CROW - 4);
        const f4a8 ca = *reinterpret_cast<const f4a8*>(Lf + 2 * sl0), cb = *reinterpret_cast<const f4a8*>(Lf + 2 * sl0 + 4);
        const s8a4 da = *reinterpret_cast<const s8a4*>(Ls + 2 * sl0);
        cq[0] = f4a8{ca[0], ca[1], ca[2], ca[3]}; dq[0] = s4a4{da[0], da[1], da[2], da[3]};
        cq[1] = f4a8{ca[2], ca[3], cb[0], cb[1]}; dq[1] = s4a4{da[2], da[3], da[4], da[5]};
        cq[2] = cq[1]; dq[2] = dq[1];
        cq[3] = f4a8{cb[0], cb[1], cb[2], cb[3]}; dq[3] = s4a4{da[4], da[5], da[6], da[7]};
        // the weights from the table all the same: 0.75 / 0.25, and 0 at the frame's clamped last column
#pragma unroll
        for (int c = 0; c < 4; c++) fxs[c] = __builtin_amdgcn_fractf(tpk[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float t = tpk[c];
            fxs[c] = __builtin_amdgcn_fractf(t);                          // exact: t = s0 + fx, t >= 0
            const int sl = min(max((int)t - row.ss[hh], 0), CROW - 2);      // (in range by construction; the clamp keeps a bug from reading other waves' LDS)
            cq[c] = *reinterpret_cast<const f4a8*>(Lf + 2 * sl);         // conf: row0[s], row1[s], row0[s+1], row1[s+1]
            dq[c] = *reinterpret_cast<const s4a4*>(Ls + 2 * sl);         // disparity, the same four
        }
    }
    float cv[4], dv[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        // {confidence, disparity} side by side: packed multiplies / adds, every rounding where the scalar
        // statement has it (products and sums separately: no fused multiply-add)
        const float a0 = 1.0f - fxs[c], a1 = fxs[c];
        const v2f aa0 = {a0, a0}, aa1 = {a1, a1};
        const v2f p0 = {cq[c][0], (float)dq[c][0]}, p1 = {cq[c][1], (float)dq[c][1]};     // rows 0 / 1 at s
        const v2f n0 = {cq[c][2], (float)dq[c][2]}, n1 = {cq[c][3], (float)dq[c][3]};     // ... at s + 1
        const v2f h0 = p0 * aa0 + n0 * aa1, h1 = p1 * aa0 + n1 * aa1;
        const v2f v = h0 * bb0 + h1 * bb1;                          // DF.cpp:274 | DF.cpp:272
        // saturate_cast<short> twice (DF.cpp:272, then x_ratio, :273) without branches: both arguments are
        // finite and far inside the int range here (a convex combination of int16 values; that times the
        // size ratio), so sat16's guard for NaN / out-of-int-range cannot fire -- and a branch per column
        // would let the compiler sink every column's arithmetic behind the last one's (registers)
        const float q1 = fminf(fmaxf(rintf(v[1]), -32768.0f), 32767.0f);
        const float q2 = fminf(fmaxf(rintf(q1 * a.fuse.lo_post_scale), -32768.0f), 32767.0f);
        cv[c] = v[0];
        dv[c] = post_scaled ? q2 : q1;
    }
    // columns behind the row's end (the last, partial float4 and the lanes past it) are zero
    if (4 * (vec0 + 64) > a.len) {                   // (wave-uniform: only the group that holds the row's end, and those past it)
        const int left = a.len - 4 * idx;
#pragma unroll
        for (int c = 0; c < 4; c++) { const bool on = c < left; cv[c] = on ? cv[c] : 0.0f; dv[c] = on ? dv[c] : 0.0f; }
    }
    u1 = make_float4(cv[0], cv[1], cv[2], cv[3]);
    u0 = make_float4(cv[0] * dv[0], cv[1] * dv[1], cv[2] * dv[2], cv[3] * dv[3]);
}

// FUSE_LO / FUSE_LO_HALF: t1 = conf, t0 = conf * float(dL), both interpolated from the low-resolution confidence map
// and left disparity map (a.fuse.lo_*) at the taps of a.fuse.lo_taps.  Per half of the wave's columns: fetch the two
// source rows, stage them, tap them.  The second half's loads are issued when the first half has been staged, so they
// fly during its taps and only one half's raw rows occupy registers.
template <int M, bool HALF>
__device__ __forceinline__ void load_fused_lo(const WavePassArgs& a, const RowPos& p, float4* stage, float4 (&tC)[M / 4], float4 (&t0)[M / 4], float4 (&t1)[M / 4])
{
    constexpr int MQ = LoShape<M>::MQ, KH = LoShape<M>::KH;
    // the C row first: its loads are in flight while the low-resolution rows are fetched and staged
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        tC[k] = load_c(a, p, k);
        t0[k] = make_float4(0.f, 0.f, 0.f, 0.f); t1[k] = t0[k];
    }
    const LoRow row = lo_row<M>(a.fuse, p.wv, a.len);
    LoRaw<M> raw[2];
    v4f tp[MQ];
    lo_fetch<M>(a.fuse, row, 0, p.lane, raw[0]);
    lo_load_taps<M>(a, p, 0, tp); lo_load_taps<M>(a, p, 1, tp);     // all of them requested with the row's first loads
#pragma unroll
    for (int hh = 0; hh < 2; hh++) {
        lo_put<M>(a.fuse, row, hh, p.lane, raw[hh], stage);
        __syncthreads();
        if (hh == 0) {
            asm volatile("" ::: "memory");               // (the next half's loads: not before this half is staged)
            lo_fetch<M>(a.fuse, row, 1, p.lane, raw[1]);
        }
#pragma unroll
        for (int k = (hh ? KH : 0); k < (hh ? MQ : KH); k++) {
            // (opaque: nothing here depends on a load, and the compiler would otherwise form every group's
            // taps while the loads are in flight, spilling the row)
            int lane_t = p.lane;
            asm volatile("" : "+v"(lane_t) :: "memory");
            lo_interp4<M, HALF>(a, row, hh, stage, tp[k], p.v0 + 64 * k, lane_t, t0[k], t1[k]);
            // (pinned here: nothing reads t0 / t1 before the transposes, and the compiler would sink the arithmetic
            // down to them, holding sixteen staged values per column in registers all the way)
            asm volatile("" : "+v"(t1[k].x), "+v"(t1[k].y), "+v"(t1[k].z), "+v"(t1[k].w),
                              "+v"(t0[k].x), "+v"(t0[k].y), "+v"(t0[k].z), "+v"(t0[k].w));
            __builtin_amdgcn_sched_barrier(0);           // one float4 of columns at a time (register pressure)
        }
        __syncthreads();
    }
}

// ---- weights from the guide row (WS_GUIDE1 / WS_GUIDE3) ----
// c[i] of lane l is lambda * lut[|g(l*M + i) - g(l*M + i + 1)|^2] (FGS.cpp:607-612), 0 in the ROI's last column
// (FGS.cpp:614) and behind it.  The wave's span of the guide row -- 64*M + 1 pixels -- is fetched as coalesced 16-byte
// vectors from the 16-byte boundary at or below its first byte, with the row's other loads; the raw bytes go through the
// wave's staging buffer, from which every lane reads the bytes of its own chunk and of the pixel behind it (a chunk is
// CH*M bytes and M a multiple of 4: lane offsets are dword-aligned up to the wave-uniform misalignment of the row).
// The indices come from the packed-byte helpers of prep_bodies.h, the weights from the first GW_HEAD table entries held
// in LDS; indices beyond it take one gather each from the full table (L2-resident), issued only in rows that have any.
constexpr int GW_HEAD = 1024;   // 4 KiB beside the staging buffer: eight one-wave workgroups of the M = 56 / 60 buckets still fit a CU's LDS

template <int M, int CH>
struct GuideShape {
    static constexpr int NV = (CH * (64 * M + 1) + 15 + 1023) / 1024;   // 16-byte vectors per lane, at any misalignment 0..15
    static constexpr int ND = (CH * (M + 1) + 3 + 3) / 4;               // dwords a lane reads back, at any byte offset 0..3
    static constexpr int NH = GW_HEAD / 256;                            // float4s per lane of the table head
    static_assert(NV * 1024 <= 256 * M, "the guide vectors fit the wave's staging buffer");
    static_assert(4 * (3 + 63 * (CH * M / 4) + ND) <= 256 * M, "the last lane reads inside the staging buffer");
};
template <int M, int CH>
struct GuideRaw { prep::ws_v4u g[GuideShape<M, CH>::NV]; prep::ws_v4f h[GuideShape<M, CH>::NH]; unsigned mis; };
template <int M>
struct GuideRaw<M, WS_PLANE> {};

// The loads: the guide row through a range-checked window on exactly the bytes the weights need -- pixels 0 .. len-1 of
// the ROI row, rounded out to whole dwords -- so that vectors reaching past them (the row's tail, the end of the
// caller's buffer in the last row of the last image) read zeros there instead of touching memory; and the table head.
template <int M, int CH>
__device__ __forceinline__ void guide_fetch(const WavePassArgs& a, int lane, GuideRaw<M, CH>& q)
{
    const uintptr_t row = reinterpret_cast<uintptr_t>(a.gw.guide) + (uintptr_t)((ptrdiff_t)blockIdx.y * a.gw.pair_stride +
                          (ptrdiff_t)(a.gw.y0 + (int)blockIdx.x) * a.gw.stride + (ptrdiff_t)a.gw.x0 * CH);
    q.mis = (unsigned)__builtin_amdgcn_readfirstlane((int)(row & 15u));
    const __amdgpu_buffer_rsrc_t win = prep::ws_window(reinterpret_cast<const void*>(row - q.mis), (q.mis + (unsigned)a.len * CH + 3u) & ~3u);
#pragma unroll
    for (int k = 0; k < GuideShape<M, CH>::NV; k++)
        q.g[k] = __builtin_amdgcn_raw_buffer_load_b128(win, (unsigned)(64 * k + lane) * 16u, 0, 2 /* nt: used once */);
#pragma unroll
    for (int k = 0; k < GuideShape<M, CH>::NH; k++)
        q.h[k] = reinterpret_cast<const prep::ws_v4f*>(a.gw.lut)[64 * k + lane];
}

// head look-up, ROI mask and lambda of a lane's M elements: c[i] holds a table index, or (FAR) a weight already fetched
// from the full table -- weights are -exp(..) <= -0, so the sign bit tells them from an index
template <int M, bool FAR>
__device__ __forceinline__ void guide_finish(const float* head, int lim, float lambda, float (&c)[M])
{
#pragma unroll
    for (int i = 0; i < M; i++) {
        const unsigned u = __float_as_uint(c[i]);
        float w = head[min(u, (unsigned)(GW_HEAD - 1))];
        if (FAR) {
            // (opaque: the read stays unconditional -- left alone, the compiler puts it behind a branch per element and
            // selects between an LDS and a scratch address)
            asm volatile("" : "+v"(w));
            w = (int)u < 0 ? c[i] : w;
        }
        c[i] = (i < lim ? w : 0.0f) * lambda;                      // one multiply, as transpose_in
    }
}

template <int M, int CH>
__device__ __forceinline__ void guide_weights(const WavePassArgs& a, float4* stage, float* head, int lane, const GuideRaw<M, CH>& q, float (&c)[M])
{
    typedef GuideShape<M, CH> S;
#pragma unroll
    for (int k = 0; k < S::NH; k++) reinterpret_cast<prep::ws_v4f*>(head)[64 * k + lane] = q.h[k];
#pragma unroll
    for (int k = 0; k < S::NV; k++) reinterpret_cast<prep::ws_v4u*>(stage)[64 * k + lane] = q.g[k];
    __syncthreads();
    // The window ends with the ROI row, so the pixel behind it reads as zeros and the last column's index -- whose weight
    // is masked below -- would nearly always lie beyond the head and send the whole row to the full table for nothing:
    // the last pixel is repeated behind the row instead (index 0).
    if (lane == 0) {
        unsigned char* B = reinterpret_cast<unsigned char*>(stage) + q.mis + (unsigned)(a.len - 1) * CH;
#pragma unroll
        for (int ci = 0; ci < CH; ci++) B[CH + ci] = B[ci];
    }
    __syncthreads();
    const unsigned* L = reinterpret_cast<const unsigned*>(stage) + (q.mis >> 2) + lane * (CH * M / 4);
    const unsigned mb = q.mis & 3u;
    unsigned d[S::ND];
#pragma unroll
    for (int j = 0; j < S::ND; j++) d[j] = L[j];
    // dword #j of the lane's bytes, counted from its first pixel
    auto e = [&](int j) -> unsigned { return __builtin_amdgcn_alignbyte(j + 1 < S::ND ? d[j + 1 < S::ND ? j + 1 : 0] : 0u, d[j], mb); };
    int far = 0;                                                   // the lane's largest index
    if constexpr (CH == 3) {
        unsigned p[5], pa[5];
        p[4] = e(0) & 0x00ffffffu; pa[4] = prep::ws_norm2(p[4]);
#pragma unroll
        for (int g = 0; g < M / 4; g++) {
            prep::ws_unpack3(e(3 * g), e(3 * g + 1), e(3 * g + 2), p);
            pa[0] = pa[4];
            p[4] = e(3 * g + 3) & 0x00ffffffu;                     // the next group's first pixel
#pragma unroll
            for (int k = 1; k <= 4; k++) pa[k] = prep::ws_norm2(p[k]);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int idx = prep::ws_dist2(p[k], pa[k], p[k + 1], pa[k + 1]);
                far = max(far, idx);
                c[4 * g + k] = __int_as_float(idx);
            }
        }
    } else {
#pragma unroll
        for (int g = 0; g < M / 4; g++) {
            const unsigned eg = e(g), nb = e(g + 1) & 0xffu;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int v = (int)((eg >> (8 * k)) & 0xffu);
                const int r = k < 3 ? (int)((eg >> (8 * k + 8)) & 0xffu) : (int)nb;
                const int idx = prep::ws_dist2_c1(v, r);
                far = max(far, idx);
                c[4 * g + k] = __int_as_float(idx);
            }
        }
    }
    const int lim = a.len - 1 - lane * M;                          // elements i < lim have their right neighbour inside the ROI
    if (__builtin_amdgcn_ballot_w64(far >= GW_HEAD) != 0) {        // wave-uniform: some index of the row lies beyond the head
        // One gather per element through a range-checked window, at an offset no window reaches for the lanes whose
        // index the head holds (they fetch nothing and get +0, which no weight is), sixteen in flight at a time.
        const __amdgpu_buffer_rsrc_t lutwin = prep::ws_window(a.gw.lut, sizeof(float) * ADF_LUT_LEVELS);
        constexpr int G = 16;
#pragma unroll
        for (int i0 = 0; i0 < M; i0 += G) {
            unsigned w[G];
#pragma unroll
            for (int k = 0; k < G; k++)
                if (i0 + k < M) {
                    const int idx = __float_as_int(c[i0 + k]);
                    w[k] = __builtin_amdgcn_raw_buffer_load_b32(lutwin, idx >= GW_HEAD ? (unsigned)idx * 4u : prep::WS_DROP, 0, 0);
                }
#pragma unroll
            for (int k = 0; k < G; k++)
                if (i0 + k < M) c[i0 + k] = w[k] != 0u ? __uint_as_float(w[k]) : c[i0 + k];
        }
        guide_finish<M, true>(head, lim, a.lambda, c);
    } else {
        guide_finish<M, false>(head, lim, a.lambda, c);
    }
    __syncthreads();
}

// ---- transpose in: "float4 #(64k + lane)" -> "chunk of lane", through the wave's staging buffer ----
template <int M>
__device__ __forceinline__ void transpose_in(float4* stage, int lane, const float4 (&t)[M / 4], float (&dst)[M], float scale)
{
#pragma unroll
    for (int k = 0; k < M / 4; k++) stage[64 * k + lane] = t[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < M / 4; k++) {
        const float4 v = stage[lane * (M / 4) + k];
        dst[4 * k + 0] = v.x * scale; dst[4 * k + 1] = v.y * scale;
        dst[4 * k + 2] = v.z * scale; dst[4 * k + 3] = v.w * scale;
    }
    __syncthreads();
}

// Pair plane (load_planes): half `half` of the wave's interleaved row (strips [2M*half, 2M*half + 2M)) holds both
// right-hand sides of the chunks of lanes [32*half, 32*half + 32); float4 #k of a chunk starts at column
// j = lane'*M + 4k of the half.
template <int M>
__device__ __forceinline__ void pair_in(float4* stage, int lane, const float4 (&t)[M / 4], int half, float (&f0)[M], float (&f1)[M])
{
    constexpr int MQ = M / 4;
#pragma unroll
    for (int k = 0; k < MQ; k++) stage[64 * k + lane] = t[k];
    __syncthreads();
    if ((lane >> 5) == half) {
#pragma unroll
        for (int k = 0; k < MQ; k++) {
            const int sidx = pair_slot((lane & 31) * M + 4 * k);
            const float4 v = stage[sidx], w = stage[sidx + 4];
            f0[4 * k + 0] = v.x; f0[4 * k + 1] = v.y; f0[4 * k + 2] = v.z; f0[4 * k + 3] = v.w;
            f1[4 * k + 0] = w.x; f1[4 * k + 1] = w.y; f1[4 * k + 2] = w.z; f1[4 * k + 3] = w.w;
        }
    }
    __syncthreads();
}

// ---- store: the solutions back to where the right-hand sides were loaded from ----
// `lane` is the kernel's opaque copy of the lane index (see there).
template <int M>
__device__ __forceinline__ void store_plain(const WavePassArgs& a, const RowPos& p, float4* stage, int lane, const float (&f0)[M])
{
    constexpr int MQ = M / 4;
#pragma unroll
    for (int k = 0; k < MQ; k++)
        stage[p.lane * MQ + k] = make_float4(f0[4 * k], f0[4 * k + 1], f0[4 * k + 2], f0[4 * k + 3]);
    __syncthreads();
    float4* d4 = reinterpret_cast<float4*>(a.U0 + p.off);
#pragma unroll
    for (int k = 0; k < MQ; k++) {
        const int idx = 64 * k + lane;
        if (p.v0 + idx < p.nvec) store_nt(stage[idx], d4 + p.v0 + idx);
    }
}

// the mirror image of pair_in: half a row of the pair plane at a time
template <int M>
__device__ __forceinline__ void store_pair(const WavePassArgs& a, const RowPos& p, float4* stage, int lane, const float (&f0)[M], const float (&f1)[M])
{
    constexpr int MQ = M / 4;
    float4* d4 = reinterpret_cast<float4*>(a.U0 + p.offU);
#pragma unroll
    for (int half = 0; half < 2; half++) {
        if ((p.lane >> 5) == half) {
#pragma unroll
            for (int k = 0; k < MQ; k++) {
                const int sidx = pair_slot((p.lane & 31) * M + 4 * k);
                stage[sidx] = make_float4(f0[4 * k], f0[4 * k + 1], f0[4 * k + 2], f0[4 * k + 3]);
                stage[sidx + 4] = make_float4(f1[4 * k], f1[4 * k + 1], f1[4 * k + 2], f1[4 * k + 3]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MQ; k++) {
            const int idx = 2 * p.v0 + 64 * (k + half * MQ) + lane;
            if (idx < p.nvecU) store_nt(stage[64 * k + lane], d4 + rhs_vec<true>(idx));
        }
        __syncthreads();
    }
}

// A row -> column hand-off (IMAGE): what a row pass writes is read by nobody but the column pass that follows it, so
// the row pass stores its solutions as that pass's register image (fgs_wave_common.h) instead of the pair plane.  (The
// column -> row hand-off stays on the pair plane: the row pass needs its contiguous rows.)  The plain pass and the
// FUSE_VIEW first pass have the form; FUSE_VIEW_F32 and the low-resolution prologues keep the pair plane for the first
// hand-off.  Same staging buffer, same values, half a row
// at a time; the staged order is the image's -- a strip's 16 columns as eight float4s [U0 c, U0 c+1, U1 c, U1 c+1] --
// so the eight lanes that store a strip of this row write one whole 128-byte line: row i of chunk ch of strip s lies at
// float4 s*(512*Mc) + (ch/8)*(64*Mc) + i*64 + (ch%8)*8 of the pair's image, Mc = a.image_m the column bucket's chunk.
__device__ __forceinline__ constexpr int image_slot(int j) { return ((j >> 4) << 3) + ((j & 15) >> 1); }

template <int M>
__device__ __forceinline__ void store_image(const WavePassArgs& a, const RowPos& p, float4* stage, int lane, const float (&f0)[M], const float (&f1)[M])
{
    constexpr int MQ = M / 4;
    const unsigned mc = (unsigned)a.image_m, ch = (unsigned)blockIdx.x / mc, i = (unsigned)blockIdx.x - ch * mc;   // wave-uniform
    float4* d4 = reinterpret_cast<float4*>(a.image + (size_t)blockIdx.y * a.image_plane) + ((ch >> 3) * (64u * mc) + i * 64u + (ch & 7u) * 8u);
    const unsigned strip_step = 512u * mc;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        if ((p.lane >> 5) == half) {
#pragma unroll
            for (int k = 0; k < MQ; k++) {
                // (8-byte writes of register pairs as the solve left them: a float4 gathered from f0 and f1 would be
                // four copies per slot, and at M = 56 / 60 those spill)
                v2f* s2 = reinterpret_cast<v2f*>(stage + image_slot((p.lane & 31) * M + 4 * k));
                s2[0] = (v2f){f0[4 * k], f0[4 * k + 1]}; s2[1] = (v2f){f1[4 * k], f1[4 * k + 1]};
                s2[2] = (v2f){f0[4 * k + 2], f0[4 * k + 3]}; s2[3] = (v2f){f1[4 * k + 2], f1[4 * k + 3]};
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MQ; k++) {
            const int idx = 64 * (k + half * MQ) + lane;      // float4 of the interleaved row: strip idx / 8, piece idx % 8
            if (idx < p.nvecU) store_nt(stage[64 * k + lane], d4 + ((unsigned)(idx >> 3) * strip_step + (unsigned)(idx & 7)));
        }
        __syncthreads();
    }
}

// NW = 2: rows longer than 64 chunks of 64 elements (ROIs wider than 4096 columns: 8K frames) are solved by TWO
// wavefronts of one workgroup, wave w owning columns [w*64*M, (w+1)*64*M) -- its own staging buffer, its own loads and
// stores, the chunk sweeps unchanged -- and meeting the other three times through LDS: the weight in front of chunk 64,
// the left-end coefficients of chunk 64 for chunk 63's separator row, and the 128-row reduced system, which wave 0
// solves (fgs_wave_common.h, reduced128).
// (the longest chunk with two right-hand sides does not fit two waves per SIMD without spilling: the
// pair staging keeps both right-hand sides and two of the three load batches alive at once)
template <int M, int R, int FUSED, int NW = 1, int WS = WS_PLANE, bool IMAGE = false>
__global__ void __launch_bounds__(64 * NW, (M > (NW == 2 ? 40 : H_TWO_WAVE_MAX) && R > 1) ? 1 : 2) wave_hpass_kernel(WavePassArgs a)
{
    static_assert(M % 4 == 0 && M >= 4, "chunk length must be a multiple of 4");
    static_assert(NW == 1 || NW == 2, "one or two wavefronts per row");
    static_assert(!IMAGE || (R == 2 && (FUSED == FUSE_NONE || FUSED == FUSE_VIEW) && NW == 1),
                  "a hand-off's image: a one-wave pass of two right-hand sides, plain or with the view-resolution int16 prologue");
    constexpr bool LO = FUSED == FUSE_LO || FUSED == FUSE_LO_HALF;
    constexpr bool PAIR = R > 1;
    constexpr bool GUIDE = WS != WS_PLANE;
    static_assert(!GUIDE || (NW == 1 && !LO), "the guide forms: one-wave rows whose prologue leaves the staging buffer alone");
    __shared__ __attribute__((aligned(16))) float lut_head[GUIDE ? GW_HEAD : 1];
    __shared__ float4 stage_all[NW][LO ? lo_stage_vec4(M) : M * 16];
    __shared__ float xch[NW == 2 ? 5 : 1];              // c in front of chunk 64; GS0, GS1, PS, QS of chunk 64
    __shared__ float red[NW == 2 ? 5 : 1][NW == 2 ? 128 : 1];   // separator rows
    __shared__ float xsol[NW == 2 ? 2 : 1][NW == 2 ? 128 : 1];  // their solutions
    const RowPos p = row_pos<M, PAIR, NW>(a);
    const int lane = p.lane, wv = p.wv;
    float4* stage = stage_all[wv];

    float4 tC[M / 4], t0[M / 4], t1[M / 4];
    GuideRaw<M, WS> tG;
    if constexpr (GUIDE) guide_fetch<M, WS>(a, lane, tG);
    if constexpr (LO) load_fused_lo<M, FUSED == FUSE_LO_HALF>(a, p, stage, tC, t0, t1);
    else if constexpr (FUSED == FUSE_VIEW) load_fused_view<M, !GUIDE>(a, p, tC, t0, t1);
    else if constexpr (FUSED == FUSE_VIEW_F32) {
        fused_f32_conf<M, !GUIDE>(a, p, tC, t1);
        if constexpr (!fused_f32_defer(M, GUIDE)) fused_f32_map<M>(a, p, t0, t1);
    }
    else load_planes<M, R, !GUIDE>(a, p, tC, t0, t1);

    float c[M], f0[M], f1[M];
    if constexpr (GUIDE) guide_weights<M, WS>(a, stage, lut_head, lane, tG, c);
    else transpose_in<M>(stage, lane, tC, c, a.lambda);
    if constexpr (FUSED == FUSE_VIEW_F32 && fused_f32_defer(M, GUIDE)) fused_f32_map<M>(a, p, t0, t1);
    if constexpr (PAIR && FUSED == FUSE_NONE) {
        pair_in<M>(stage, lane, t0, 0, f0, f1);
        pair_in<M>(stage, lane, t1, 1, f0, f1);
    } else {
        transpose_in<M>(stage, lane, t0, f0, 1.0f);
        if constexpr (R > 1) transpose_in<M>(stage, lane, t1, f1, 1.0f);
        else {
#pragma unroll
            for (int i = 0; i < M; i++) f1[i] = 0.0f;
        }
    }

    float a_s = __shfl_up(c[M - 1], 1);
    if (lane == 0) a_s = 0.0f;
    if constexpr (NW == 2) {                                     // chunk 64 follows chunk 63
        if (wv == 0 && lane == 63) xch[0] = c[M - 1];
        __syncthreads();
        if (wv == 1 && lane == 0) a_s = xch[0];
    }

    Boundary<float, R> bd;
    chunk_boundary<M, R>(c, f0, f1, a_s, bd);
    float nGS0 = __shfl_down(bd.GS0, 1), nGS1 = (R > 1) ? __shfl_down(bd.GS1, 1) : 0.0f;
    float nPS = __shfl_down(bd.PS, 1), nQS = __shfl_down(bd.QS, 1);
    if (lane == 63) { nGS0 = 0.0f; nGS1 = 0.0f; nPS = 0.0f; nQS = 0.0f; }
    if constexpr (NW == 2) {                                     // chunk 63's next chunk is wave 1's first
        if (wv == 1 && lane == 0) { xch[1] = bd.GS0; xch[2] = (R > 1) ? bd.GS1 : 0.0f; xch[3] = bd.PS; xch[4] = bd.QS; }
        __syncthreads();
        if (wv == 0 && lane == 63) { nGS0 = xch[1]; nGS1 = xch[2]; nPS = xch[3]; nQS = xch[4]; }
    }
    float al, be, ga, p0, p1, xs0, xs1;
    separator_row<M, R>(c, f0, f1, bd, nGS0, nGS1, nPS, nQS, al, be, ga, p0, p1);
    float xL0, xL1;
    if constexpr (NW == 2) {
        const int g = 64 * wv + lane;                            // chunk of this lane
        red[0][g] = al; red[1][g] = be; red[2][g] = ga; red[3][g] = p0; red[4][g] = p1;
        __syncthreads();
        if (wv == 0) reduced128<R>(lane, red[0], red[1], red[2], red[3], red[4], 1, xsol[0], xsol[1]);
        __syncthreads();
        xs0 = xsol[0][g]; xs1 = (R > 1) ? xsol[1][g] : 0.0f;
        xL0 = g > 0 ? xsol[0][g - 1] : 0.0f; xL1 = (R > 1 && g > 0) ? xsol[1][g - 1] : 0.0f;
    } else {
        pcr64<R>(lane, al, be, ga, p0, p1, xs0, xs1);
        xL0 = __shfl_up(xs0, 1); xL1 = (R > 1) ? __shfl_up(xs1, 1) : 0.0f;
        if (lane == 0) { xL0 = 0.0f; xL1 = 0.0f; }
    }
    chunk_solve<M, R>(c, f0, f1, a_s, xL0, xL1, xs0, xs1);

    // The pass works in place: the store addresses ARE the load addresses, and the compiler would keep
    // those (a 64-bit pointer per load) alive across the whole solve to reuse them.  An opaque copy of
    // the lane index makes it recompute them here instead.
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    if constexpr (IMAGE) store_image<M>(a, p, stage, lane_s, f0, f1);
    else if constexpr (PAIR) store_pair<M>(a, p, stage, lane_s, f0, f1);
    else store_plain<M>(a, p, stage, lane_s, f0);
}

// Buckets that have the half-width form of the low-resolution prologue: all but the longest one-wave chunk below the
// single-occupancy kernels, whose half-width form needs five registers more than a lane has (it takes the general form).
constexpr bool lo_half_bucket(int m, int nw) { return !(m == 60 && nw == 1); }

// Is the image form of the FUSE_VIEW first pass built?  Every one-wave bucket and weight source has it: none spills and
// each keeps its pair-plane form's occupancy (profiles/inner_handoff_isa.txt).
constexpr bool FIRST_IMAGE = true;

// the guide forms of a bucket: every one-wave bucket has them
constexpr bool guide_bucket(int nw) { return nw == 1; }

// the plain and the fused-view pass with their weights from the guide (a.gw)
template <int M, int WS>
hipError_t launch_h_guide(const WavePassArgs& a, int n_rhs, dim3 grid, hipStream_t st)
{
    if (a.fuse.conf_in) {
        if (n_rhs != 2) return hipErrorInvalidValue;
        if (a.fuse.dl_f32) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_VIEW_F32, 1, WS>), grid, dim3(64), 0, st, a);
        else if (a.image) {
            if constexpr (FIRST_IMAGE) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_VIEW, 1, WS, true>), grid, dim3(64), 0, st, a);
            else return hipErrorInvalidValue;
        } else hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_VIEW, 1, WS>), grid, dim3(64), 0, st, a);
    } else if (n_rhs == 2 && a.image) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_NONE, 1, WS, true>), grid, dim3(64), 0, st, a);
    else if (n_rhs == 2) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_NONE, 1, WS>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((wave_hpass_kernel<M, 1, FUSE_NONE, 1, WS>), grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

template <int M, int NW = 1>
hipError_t launch_h(const WavePassArgs& a, int n_rhs, int n_pairs, hipStream_t st)
{
    dim3 grid(a.nscan, n_pairs), block(64 * NW);
    if (a.gw.guide) {
        if constexpr (guide_bucket(NW)) {
            if (a.gw.ch == 1) return launch_h_guide<M, WS_GUIDE1>(a, n_rhs, grid, st);
            if (a.gw.ch == 3) return launch_h_guide<M, WS_GUIDE3>(a, n_rhs, grid, st);
        }
        return hipErrorInvalidValue;
    }
    if (a.fuse.lo_conf) {
        if (n_rhs != 2 || !a.fuse.lo_taps) return hipErrorInvalidValue;
        const int n = ((a.len + 3) / 4) * 4;
        hipLaunchKernelGGL(lo_tap_table_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a.fuse.lo_taps, n, a.len, a.fuse.hi_x0, a.fuse.lo_scale_x, a.fuse.lo_w);
        // maps of exactly half the view's width, ROI on an even column >= 2: the form with shared source elements
        bool half = false;
        if constexpr (lo_half_bucket(M, NW)) {
            half = wave_hpass_lo_half(a);
            if (half) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_LO_HALF, NW>), grid, block, 0, st, a);
        }
        if (!half) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_LO, NW>), grid, block, 0, st, a);
    } else if (a.fuse.conf_in) {
        if (n_rhs != 2) return hipErrorInvalidValue;
        if (a.fuse.dl_f32) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_VIEW_F32, NW>), grid, block, 0, st, a);
        else if (a.image) {
            if constexpr (FIRST_IMAGE && NW == 1) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_VIEW, 1, WS_PLANE, true>), grid, block, 0, st, a);
            else return hipErrorInvalidValue;                     // two-wave rows have no image form
        } else hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_VIEW, NW>), grid, block, 0, st, a);
    } else if (n_rhs == 2 && a.image) {
        if constexpr (NW == 1) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_NONE, 1, WS_PLANE, true>), grid, block, 0, st, a);
        else return hipErrorInvalidValue;                     // two-wave rows have no image form
    } else if (n_rhs == 2) hipLaunchKernelGGL((wave_hpass_kernel<M, 2, FUSE_NONE, NW>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((wave_hpass_kernel<M, 1, FUSE_NONE, NW>), grid, block, 0, st, a);
    return hipGetLastError();
}

// The row buckets: one wavefront per row of 64 chunks up to 4096 columns, two wavefronts (128 chunks) above.
// (60 x 64 = 3840 columns: a full 4K row; 60 x 128 = 7680: a full 8K row)
constexpr Bucket ROW_BUCKETS[] = {{4, 64}, {8, 64}, {16, 64}, {20, 64}, {28, 64}, {40, 64}, {56, 64}, {60, 64}, {64, 64},
                                  {40, 128}, {48, 128}, {56, 128}, {60, 128}, {64, 128}};
constexpr int N_ROW_BUCKETS = sizeof(ROW_BUCKETS) / sizeof(ROW_BUCKETS[0]);

// chunk length / wavefronts per row the launcher picks for a row of `len` elements
void pick_row_bucket(int len, int& m, int& nw)
{
    const Bucket& b = ROW_BUCKETS[bucket_index(ROW_BUCKETS, len)];
    m = b.m; nw = b.chunks / 64;
}

} // namespace

int wave_max_row_len() { return ROW_BUCKETS[N_ROW_BUCKETS - 1].m * ROW_BUCKETS[N_ROW_BUCKETS - 1].chunks; }

// The fused first pass reads conf as float4s -- the confidence plane is the library's own and laid out so that the ROI
// row starts 16-byte aligned whatever the ROI is (Geom::cx0 / cpitch) -- and dL, the caller's map, in 8-byte pieces at
// any 2-byte aligned address (round 3: any ROI x / width, any even stride).  Rows shorter than one vector go through
// the prologue kernels instead.
bool wave_hpass_can_fuse(const WavePassArgs& a)
{
    if (!a.fuse.conf_in || !a.fuse.dl_in) return false;
    if (a.len < 4 || a.fuse.conf_pitch % 4 != 0 || a.fuse.conf_x0 % 4 != 0 || a.fuse.conf_frame % 4 != 0) return false;
    if ((reinterpret_cast<uintptr_t>(a.fuse.conf_in) & 15u) != 0) return false;
    const unsigned em = a.fuse.dl_f32 ? 3u : 1u;              // the map's element alignment: 16-byte loads at any 4-byte address
    if ((a.fuse.dl_stride & em) != 0 || (a.fuse.dl_pair_stride & em) != 0 || (reinterpret_cast<uintptr_t>(a.fuse.dl_in) & em) != 0) return false;
    return true;
}

// The guide forms exist for one-wave rows whose right-hand sides come from the planes or the view-resolution fused
// prologue; the guide needs no alignment (the kernel aligns its window itself), the table a 16-byte aligned base.
bool wave_hpass_guide_fits(const WavePassArgs& a)
{
    if (!a.gw.guide || !a.gw.lut || (a.gw.ch != 1 && a.gw.ch != 3) || a.fuse.lo_conf) return false;
    if ((reinterpret_cast<uintptr_t>(a.gw.lut) & 15u) != 0 || a.gw.x0 < 0 || a.gw.y0 < 0) return false;
    if (a.len < 2 || a.len > wave_max_row_len()) return false;
    int m, nw;
    pick_row_bucket(a.len, m, nw);
    return guide_bucket(nw);
}

bool wave_hpass_image_fits(int row_len)
{
    if (row_len < 2 || row_len > wave_max_row_len()) return false;
    int m, nw;
    pick_row_bucket(row_len, m, nw);
    return nw == 1;
}

bool wave_hpass_first_image(const FusedInputs& f) { return FIRST_IMAGE && f.conf_in && !f.lo_conf && !f.dl_f32; }

bool wave_hpass_lo_half(const WavePassArgs& a)
{
    if (!(a.fuse.lo_conf && a.fuse.lo_half && a.fuse.lo_scale_x == 0.5 && (a.fuse.hi_x0 & 1) == 0 && a.fuse.hi_x0 >= 2)) return false;
    int m, nw;
    pick_row_bucket(a.len, m, nw);
    return lo_half_bucket(m, nw);
}

// The low-resolution form stages, per wavefront and per half of its columns, the source elements its taps touch plus
// one: that span must fit lo_row_cap(M) slots (scale factors up to about 0.66 do, whatever the bucket), the strides
// must keep rows 4-byte / 2-byte aligned.  The same tap function runs here and in the kernel.
bool wave_hpass_can_fuse_lo(const WavePassArgs& a)
{
    if (!a.fuse.lo_conf || !a.fuse.lo_dl || a.fuse.lo_w < 2 || a.fuse.lo_w > 65535 || a.fuse.lo_h < 1 || a.len < 2 || a.len > wave_max_row_len()) return false;
    if ((reinterpret_cast<uintptr_t>(a.fuse.lo_conf) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a.fuse.lo_dl) & 1u) != 0) return false;
    if (a.fuse.lo_dl_stride % 2 != 0 || a.fuse.lo_dl_pair % 2 != 0) return false;
    if (!(a.fuse.lo_scale_x > 0.0 && a.fuse.lo_scale_y > 0.0) || a.fuse.hi_x0 < 0 || a.fuse.hi_y0 < 0) return false;
    int m, nw;
    pick_row_bucket(a.len, m, nw);
    const int mq = m / 4, kh = (mq + 1) / 2, cap = lo_row_cap(m);
    for (int wv = 0; wv < nw; wv++)
        for (int hh = 0; hh < 2; hh++) {
            const int cfirst = 64 * m * wv + 256 * (hh ? kh : 0);
            const int clast = std::min(64 * m * wv + 256 * (hh ? mq : kh), a.len) - 1;
            if (clast < cfirst) continue;
            int s_first, s_last; float f_;
            lin_tap(a.fuse.hi_x0 + cfirst, a.fuse.lo_scale_x, a.fuse.lo_w, s_first, f_);
            lin_tap(a.fuse.hi_x0 + clast, a.fuse.lo_scale_x, a.fuse.lo_w, s_last, f_);
            if (s_last + 2 - s_first > cap) return false;
        }
    return true;
}

hipError_t launch_wave_hpass(const WavePassArgs& a, int n_rhs, int n_pairs, hipStream_t st)
{
    if (a.len < 2 || a.len > wave_max_row_len() || a.pitch % 64 != 0 || a.pitch < a.len) return hipErrorInvalidValue;
    if (a.fuse.lo_conf && !wave_hpass_can_fuse_lo(a)) return hipErrorInvalidValue;
    if (!a.fuse.lo_conf && a.fuse.conf_in && !wave_hpass_can_fuse(a)) return hipErrorInvalidValue;
    if (a.gw.guide && !wave_hpass_guide_fits(a)) return hipErrorInvalidValue;
    // a hand-off's image: a pass of two right-hand sides on one-wave rows -- plain or, where that form is built, with the
    // view-resolution prologue on an int16 map -- every row inside the image
    if (a.image && (n_rhs != 2 || a.fuse.lo_conf || (a.fuse.conf_in && (a.fuse.dl_f32 || !FIRST_IMAGE)) || !wave_hpass_image_fits(a.len) || a.image_m < 1 ||
                    a.nscan > 64 * a.image_m || a.image_plane < wave_image_floats(a.pitch, a.image_m)))
        return hipErrorInvalidValue;
    return dispatch_index<N_ROW_BUCKETS>(bucket_index(ROW_BUCKETS, a.len), [&](auto I) {
        constexpr Bucket b = ROW_BUCKETS[decltype(I)::value];
        return launch_h<b.m, b.chunks / 64>(a, n_rhs, n_pairs, st);
    });
}

} // namespace adf
