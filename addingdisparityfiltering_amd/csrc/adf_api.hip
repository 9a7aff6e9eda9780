// adf_api.hip -- host side of the C-ABI declared in include/adf_wls.h.
//
// Orchestrates DisparityWLSFilterImpl::filter (DF.cpp:219-298) and
// FastGlobalSmootherFilterImpl::{init,filter} (FGS.cpp:141-233) as a fixed sequence of HIP kernel
// launches on the caller's stream.  No host<->device synchronisation happens on the device-pointer
// path after the workspace exists, so a caller may capture it into a hipGraph.  Errors, device memory, the weight
// tables and the host entry points' copies come from the shared host toolkit (adf_host.h).
#include "adf_host.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace adf;

// ----------------------------------------------------------------------------------------------
// shared pieces
// ----------------------------------------------------------------------------------------------
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// image k of a batch whose images lie `pair_stride` bytes apart (null stays null)
template <class T> static const T* pairs_on(const T* p, ptrdiff_t pair_stride, int k)
{
    return p ? (const T*)((const char*)p + (ptrdiff_t)k * pair_stride) : nullptr;
}

static Geom make_geom(int W, int H, int rx, int ry, int rw, int rh)
{
    Geom g;
    g.W = W; g.H = H; g.rx = rx; g.ry = ry; g.rw = rw; g.rh = rh;
    g.pw = round_up(rw, 64);
    g.ph = round_up(rh, 64);
    size_t a = (size_t)round_up(rh, TILE_ROWS) * g.pw, b = (size_t)rw * g.ph;   // (the wave solver's pair plane holds rows in tiles)
    g.plane = ((a > b ? a : b) + 63) / 64 * 64;
    g.frame = (size_t)W * H;
    // confidence plane: ROI column 0 16-byte aligned, >= 3 zero floats behind a row, pitch a multiple of 4 (adf_internal.h)
    g.cx0 = (4 - (rx & 3)) & 3;
    g.cpitch = round_up(W + g.cx0 + 3, 4);
    g.cframe = (size_t)g.cpitch * H;
    return g;
}

// Confidence plane as a plain W-pitch frame (the low-resolution scratch map of the down-scaled path).
static Geom plain_conf_layout(Geom g) { g.cx0 = 0; g.cpitch = g.W; g.cframe = g.frame; return g; }

// Per-launch HIP-event timing (adf_wls_profile_*).  Events are pooled and reused.
enum KClass { K_FILL = 0, K_WEIGHTS, K_DISC, K_LRC, K_PROLOGUE, K_PASS_H_FIRST, K_PASS_H, K_PASS_V, K_PASS_V_LAST, K_RESIZE, K_QUANT, K_COUNT };
static const char* const kclass_names[K_COUNT] = {"fill_outside", "weights", "discontinuity", "lrc_confidence",
                                                  "plain_prologue", "pass_h_first", "pass_h", "pass_v", "pass_v_last", "resize", "quantise_maps"};
// What a launch reports: the bytes the algorithm has to move, and the bytes this kernel moves.  One function
// per class of the preparation stage (run_passes has the solve passes'); P = ROI pixels, F = frame pixels, outside =
// F - P, all times the pair count; out_b / map_b = bytes per element of the filtered map / the disparity maps.
struct Bytes { double alg, moved; };
static Bytes same_bytes(double b) { return Bytes{b, b}; }
static Bytes fill_bytes(double outside, bool conf, double out_b) { return same_bytes(((conf ? 4.0 : 0.0) + out_b) * outside); }
static Bytes weights_bytes(double P, int gch, bool chor) { return same_bytes((gch + (chor ? 8.0 : 4.0)) * P); }
// reads the int16 ROIs, writes the float maps (the maps themselves are not algorithmic I/O); one view or both
static Bytes disc_bytes(double P, bool both) { return both ? Bytes{4.0 * P, 12.0 * P} : Bytes{2.0 * P, 6.0 * P}; }
// lrc_confidence, band kernel: dL 2 + dR 2 read, conf 4 written
static Bytes band_bytes(double P) { return same_bytes(8.0 * P); }
// ... merged launch: the band kernel's, the weight kernel's with both planes, the fill's with the confidence plane
static Bytes merged_bytes(double P, double outside, int gch, double out_b) { return same_bytes((8.0 + gch + 8.0) * P + (4.0 + out_b) * outside); }
// ... left-view kernel: alg conf (4P); moved dL 2 + dR 2 + cR 4 reads, conf 4 (+8 when U0/U1 are materialised)
static Bytes conf_left_bytes(double P, bool rhs) { const double wu = rhs ? 8.0 : 0.0; return Bytes{(4.0 + wu) * P, (12.0 + wu) * P}; }
// ... LRC kernel: alg confidence map out (4F) + the two rhs planes (8P); moved adds dL, dR, cL, cR reads; `fill`: the
// filtered map outside the ROI where the kernel writes that too
static Bytes lrc_bytes(double F, double P, bool rhs, double map_b, double fill)
{
    return Bytes{4.0 * F + (rhs ? 8.0 * P : 0.0) + fill, 4.0 * F + (rhs ? 18.0 + map_b : 12.0) * P + fill};
}
// float(src) (4P written), or conf * float(src) and conf (conf read, 8P written)
static Bytes prologue_bytes(double P, bool weighted, double map_b) { return same_bytes(((weighted ? 12.0 : 4.0) + map_b) * P); }
static Bytes resize_bytes(double dst_px, double src_px, double elem_b) { return same_bytes(elem_b * dst_px + elem_b * src_px); }
// per map 4 read and, for q, 2 written; v: 4 written
static Bytes quant_bytes(double px, bool q, bool right, bool v) { return same_bytes(((right ? 8.0 : 4.0) + (q ? (right ? 4.0 : 2.0) : 0.0) + (v ? 4.0 : 0.0)) * px); }

struct Profiler {
    bool on = false;
    struct Rec { int cls; hipEvent_t a, b; double alg, moved; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    void clear() { for (auto& r : recs) { pool.push_back(r.a); pool.push_back(r.b); } recs.clear(); }
    void destroy() { clear(); for (auto e : pool) hipEventDestroy(e); pool.clear(); }
};
// Brackets one launch: start event in the constructor, stop event in the destructor.
struct ProfScope {
    Profiler* p; hipStream_t st; Profiler::Rec r{};
    ProfScope(Profiler* prof, int cls, double alg, double moved, hipStream_t s) : p(prof && prof->on ? prof : nullptr), st(s)
    {
        if (!p) return;
        r.cls = cls; r.alg = alg; r.moved = moved; r.a = p->get(); r.b = p->get();
        if (r.a) hipEventRecord(r.a, st);
    }
    ProfScope(Profiler* prof, int cls, Bytes b, hipStream_t s) : ProfScope(prof, cls, b.alg, b.moved, s) {}
    ~ProfScope()
    {
        if (!p) return;
        if (r.b) hipEventRecord(r.b, st);
        if (r.a && r.b) p->recs.push_back(r);
    }
};

// The six (2*num_iter) solve passes of FGS.cpp:207-212 on planes already resident on the device.
// `A` holds the right-hand sides in the orientation the first (horizontal) pass wants.
struct SolvePlanes {
    float* CH; float* CV;       // weights (orientation depends on the solver)
    float* D; float* F0; float* F1;
    float* A0; float* A1;       // ping
    float* B0; float* B1;       // pong
};

struct FinalOut {
    int epilogue; void* out; ptrdiff_t stride, pair_stride; int x0, y0, cn, c;
};

// output bytes per pixel of a fused epilogue
static double epilogue_bytes(int epilogue)
{
    return (epilogue == EPI_F32 || epilogue == EPI_WLS_CONF_F32) ? 4.0 : epilogue == EPI_U8 ? 1.0 : 2.0;
}

template <class Args>
static void set_final_out(Args& a, const FinalOut& fo)
{
    a.out = fo.out; a.out_stride = fo.stride; a.out_pair_stride = fo.pair_stride;
    a.out_x0 = fo.x0; a.out_y0 = fo.y0; a.out_cn = fo.cn; a.out_c = fo.c;
}

// Which row -> column hand-offs of a chunk's passes go through the column pass's register image (fgs_wave_common.h)
// instead of the pair plane: the last one (`image` set), the inner ones behind the first (`inner`), the first one
// (`first`: the fused first pass has the image form).  A one-iteration call's only hand-off keeps the pair plane.
struct HandoffImage {
    float* image = nullptr; int m = 0; bool inner = false, first = false;
    bool at(int it, int num_iter) const
    {
        if (!image || num_iter < 2) return false;
        return it == num_iter - 1 ? true : it > 0 ? inner : first;
    }
    int inner_count(int num_iter) const
    {
        int n = 0;
        for (int it = 0; it + 1 < num_iter; it++) n += at(it, num_iter);
        return n;
    }
};

// The passes on either solver.  exact: the planes ping-pong between A and B, the horizontal pass reads the row index
// fastest; wave: the on-chip partitioned solver, row-major planes solved in place.  `fuse` (wave only): the inputs the
// first row pass forms its right-hand sides from.
static int run_passes(bool wave, const Geom& g, const SolvePlanes& p, int n_rhs, float lambda, float atten, int num_iter,
                      const FinalOut& fo, int n_pairs, hipStream_t st, Profiler* prof = nullptr,
                      const FusedInputs* fuse = nullptr, const GuideWeights* gw = nullptr, const HandoffImage& ho = HandoffImage{})
{
    const double px = (double)g.rw * g.rh * n_pairs;
    float lam = lambda;
    for (int it = 0; it < num_iter; it++, lam *= atten) {                      // FGS.cpp:211 (float)
        const bool fused = it == 0 && fuse, last = it == num_iter - 1;
        const int epi = last ? fo.epilogue : EPI_PLANES;
        // algorithmic bytes: the row pass reads the weight (the Chor plane, or `gw`: the guide row itself)
        // + R right-hand sides and writes R -- fused, C + conf + dL read (low-resolution maps: their bytes per view pixel,
        // each row counted once), U0/U1 written; the column pass writes the fused epilogue's output instead of 4R bytes
        // per pixel on the last iteration
        const double lo_b = (fused && fuse->lo_conf) ? 6.0 * fuse->lo_scale_x * fuse->lo_scale_y : (fused && fuse->dl_f32) ? 8.0 : 6.0;
        const double wb = gw ? (double)gw->ch : 4.0;
        const double hb = fused ? (wb + lo_b + 8.0) * px : (wb + 8.0 * n_rhs) * px;
        const double out_b = (last ? epilogue_bytes(fo.epilogue) : 4.0 * n_rhs) * px;
        const double vb = (4.0 + 4.0 * n_rhs) * px + out_b;
        if (wave) {
            WavePassArgs h{}, v{};
            h.C = p.CH; h.U0 = p.A0; h.U1 = p.A1;
            h.nscan = g.rh; h.len = g.rw; h.pitch = g.pw; h.plane = g.plane; h.lambda = lam;
            if (fused) h.fuse = *fuse;
            if (gw) h.gw = *gw;
            v.C = p.CV; v.U0 = p.A0; v.U1 = p.A1;
            v.nscan = g.rw; v.len = g.rh; v.pitch = g.pw; v.plane = g.plane; v.lambda = lam;
            if (last) set_final_out(v, fo);
            // The row -> column hand-offs: nobody but the column pass of the same iteration reads what a row pass writes, so
            // the row pass stores that pass's register image instead of the pair plane (same bytes: 8 written, 8 read per
            // pixel).  Ordering: within an iteration the row pass writes the image and the column pass reads it; the column
            // pass writes the pair plane and the next iteration's row pass reads that.  Nothing is read and written in
            // the same launch except the column pass's own strip of the pair plane, and the column pass holds its whole
            // strip in registers before its first store.
            if (ho.at(it, num_iter)) {
                h.image = v.image = ho.image; h.image_m = v.image_m = ho.m;
                h.image_plane = v.image_plane = wave_image_floats(g.pw, ho.m);
            }
            {
                ProfScope ps(prof, fused ? K_PASS_H_FIRST : K_PASS_H, hb, hb, st);
                HIP_TRY(launch_wave_hpass(h, n_rhs, n_pairs, st));             // FGS.cpp:209
            }
            ProfScope ps(prof, last ? K_PASS_V_LAST : K_PASS_V, vb, vb, st);
            HIP_TRY(launch_wave_vpass(v, n_rhs, epi, n_pairs, st));           // FGS.cpp:210
        } else {
            // moved bytes: the exact solver's D and eliminated right-hand sides round-trip through memory
            PassArgs h{}, v{};
            h.C = p.CH; h.U0 = p.A0; h.U1 = p.A1; h.D = p.D; h.F0 = p.F0; h.F1 = p.F1; h.O0 = p.B0; h.O1 = p.B1;
            h.nscan = g.rh; h.len = g.rw; h.pitch_in = g.ph; h.pitch_out = g.pw; h.plane = g.plane; h.lambda = lam;
            v.C = p.CV; v.U0 = p.B0; v.U1 = p.B1; v.D = p.D; v.F0 = p.F0; v.F1 = p.F1; v.O0 = p.A0; v.O1 = p.A1;
            v.nscan = g.rw; v.len = g.rh; v.pitch_in = g.pw; v.pitch_out = g.ph; v.plane = g.plane; v.lambda = lam;
            if (last) set_final_out(v, fo);
            {
                ProfScope ps(prof, K_PASS_H, hb, (12.0 + 16.0 * n_rhs) * px, st);
                HIP_TRY(launch_exact_pass(h, n_rhs, EPI_PLANES, n_pairs, st)); // FGS.cpp:209
            }
            ProfScope ps(prof, last ? K_PASS_V_LAST : K_PASS_V, vb, (12.0 + 12.0 * n_rhs) * px + out_b, st);
            HIP_TRY(launch_exact_pass(v, n_rhs, epi, n_pairs, st));           // FGS.cpp:210
        }
    }
    return ADF_OK;
}

static bool wave_fits(const Geom& g)
{
    return g.rw >= 2 && g.rh >= 2 && g.rw <= wave_max_row_len() && g.rh <= wave_max_col_len();
}

// ----------------------------------------------------------------------------------------------
// DisparityWLSFilter
// ----------------------------------------------------------------------------------------------
// The down-scaled path's low-resolution confidence maps and what cv::resize of them into the handle's view-sized planes
// needs (DF.cpp:274).
struct ConfResize {
    float* clo; int dW, dH; adf_rect rlo; // the maps (W = dW pitch, one per pair) and their ROI
    Geom ghi;                             // the view's geometry
    bool band_map;                        // the band kernel made them: zero outside the ROI (DF.cpp:187-190)
    int n_pairs;
};

// The smallest chunk of a call, in ROI pixels, whose last hand-off takes the register image.  Measured on batches of
// 1 ... 64 pairs of 3840 x 2160 (ROI 3584 x 2160), both forms alternating in one process (tools/last_handoff_time.py,
// profiles/last_handoff_ab.txt, "chunk size series"): up to 8 pairs the row pass's scattered lines cost what the column
// pass's loads gain (the two passes' sum within +-1 %, the call 0.3-1.6 % slower with the image); 12 pairs is the
// smallest batch at which the sum is lower outside both forms' spread and the call is not slower.  Other geometries are
// taken by their pixel count: estimated, not measured.
// The inner hand-offs take the image under the same threshold: in the same series with three handles (all hand-offs /
// the last only / none; profiles/inner_handoff_ab.txt, "chunk size series") they do not need a larger chunk than the
// last one -- level with "last only" within both spreads up to 4 pairs, lower from 8 pairs on, and at 12 pairs lower
// outside both spreads (2.54-2.61 against 2.60-2.68 ms per call).
constexpr long long HANDOFF_IMAGE_MIN_PX = 12LL * 3584 * 2160;

struct adf_wls {
    int device = 0;
    // DF.cpp:142-159
    int left_offset = 0, right_offset = 0, top_offset = 0, bottom_offset = 0;
    int min_disp = 0;
    bool use_confidence = true;
    double lambda = 8000.0, sigma_color = 1.0;
    int lrc_thresh = 24, disc_radius = 5;
    float roll_off = 0.001f;
    // EF.hpp:393 defaults used by DF.cpp:292
    double atten = 0.25; int num_iter = 3;
    int solver = ADF_SOLVER_WAVE;      // default: the throughput path (see include/adf_wls.h)
    int last_solver = ADF_SOLVER_WAVE;
    // state of the last call
    adf_rect roi{0, 0, 0, 0};
    int last_W = 0, last_H = 0, last_pairs = 0;
    int last_cpitch = 0, last_cx0 = 0;       // layout of the confidence planes of the last call (Geom::cpitch, cx0)
    long long conf_sig[4] = {0, 0, 0, 0};    // (W, H, cx0, pairs) the confidence planes were last zeroed for
    int last_path = 0;                       // ADF_PATH_* bits of the last call (adf_wls_get_last_path)
    int last_solver_path = 0;                // ... of its solve passes (adf_wls_get_last_solver_path)
    // device memory
    Lut lut;
    DevBuf ws;    // per-chunk workspace
    DevBuf conf;  // confidence maps of the last call (n_pairs full frames)
    DevBuf stage; // host-pointer path staging
    DevBuf scaled; // down-scaled path: resized disparity + low-resolution confidence scratch
    size_t ws_limit = (size_t)64 << 30;
    Profiler prof;
    // (geometry, solver) the workspace planes were last laid out for; a change re-zeroes them so that
    // pitch padding is zero again (the wave solver treats it as identity rows without masking)
    long long ws_sig[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // side stream: the weight kernel (guide only) runs beside the confidence kernels (disparity maps only)
    // of the same call, forked from and joined back into the caller's stream with events
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap = true;
    // Down-scaled call whose first row pass interpolated the maps itself: the view-sized confidence map of
    // getConfidenceMap() (DF.cpp:274) has not been materialised; adf_wls_get_confidence_* runs the float resize then.
    struct LazyConf { bool pending = false; ConfResize resize{}; } lazy_conf;
    bool scaled_half = true; // ADF_LO_HALF=0: never the half-width form of the fused low-resolution prologue (A/B, tests)
    bool scaled_fuse = true; // ADF_SCALED_FUSE=0: the down-scaled path through the two resize kernels (A/B measurements)
    bool conf_band = true;   // ADF_CONF_BAND=0: the two-kernel confidence stage (A/B measurements)
    bool merge_small = true; // ADF_MERGE_SMALL=0: never the merged preparation launch (A/B measurements)
    bool row_weights_guide = true; // ADF_ROW_WEIGHTS_GUIDE=0: the row passes always read the Chor plane (A/B measurements, tests)
    bool handoff_image = true;     // ADF_LAST_HANDOFF_IMAGE=0: every row pass writes the pair plane (A/B measurements, the tests' reference)
    bool handoff_inner = true;     // ADF_INNER_HANDOFF_IMAGE=0: all but the last row pass write the pair plane (A/B measurements)
    // ... and the smallest chunk, in ROI pixels, whose last hand-off takes the image (ADF_LAST_HANDOFF_MIN_PX: tests only)
    long long handoff_min_px = HANDOFF_IMAGE_MIN_PX;
    int last_handoff = ADF_HANDOFF_PAIR_PLANE;   // the form the last call's last hand-off took (adf_wls_get_last_handoff)
    int last_inner[2] = {0, 0};    // inner hand-offs of the last call's full / tail chunk that took the image (adf_wls_get_inner_handoffs)
    // HIP maps the streams of ONE priority level onto a small pool of hardware queues (4 by default) and two streams that
    // share a queue run one after the other: a side stream of the caller's priority lost the overlap for about one caller
    // stream in four (tools/batch_cpp.cpp: 13.5-13.6 ms per 64 x 4K call instead of 12.8-13.2).  Each priority level has a pool
    // of its own, so the side stream is created on a level the caller's stream is NOT on.
    static bool null_caller_of(hipStream_t s) { return s == nullptr || s == hipStreamLegacy || s == hipStreamPerThread; }
    int ensure_side(hipStream_t caller)
    {
        if (side) return ADF_OK;
        int least = 0, greatest = 0, prio = 0, cp = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; (void)hipGetLastError(); }
        if (null_caller_of(caller) || stream_is_capturing(caller) || hipStreamGetPriority(caller, &cp) != hipSuccess) { cp = 0; (void)hipGetLastError(); }
        prio = (cp != greatest) ? greatest : (greatest < least ? greatest + 1 : greatest);   // the highest level, or the one below it
        // (the NULL stream is the exception: beside a side stream of another level its calls took 13.9-14.0 ms, with one of
        // its own level 12.8-13.0 -- torch's default stream is the NULL stream)
        if (null_caller_of(caller)) HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));   // the default level, as rounds 1-3 did
        else HIP_TRY(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio));
        HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        return ADF_OK;
    }
};

extern "C" int adf_wls_create(adf_wls_t** out, int use_confidence, int l, int r, int t, int b, int min_disp)
{
    if (!out) return fail(ADF_EBADARG, "adf_wls_create: out is NULL");
    *out = nullptr;
    if (l < 0 || r < 0 || t < 0 || b < 0) return fail(ADF_EBADARG, "adf_wls_create: negative offset");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(ADF_ENODEV, "adf_wls_create: no HIP device visible");
    adf_wls* h = new (std::nothrow) adf_wls();
    if (!h) return fail(ADF_ENOMEM, "adf_wls_create: out of host memory");
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail(ADF_EHIP, "hipGetDevice failed"); }
    h->use_confidence = use_confidence != 0;
    h->left_offset = l; h->right_offset = r; h->top_offset = t; h->bottom_offset = b;
    h->min_disp = 0; (void)min_disp; // DF.cpp:146 then :149
    if (const char* e = getenv("ADF_WS_LIMIT_GB")) {
        double gb = atof(e);
        if (gb > 0) h->ws_limit = (size_t)(gb * (double)((size_t)1 << 30));
    }
    if (const char* e = getenv("ADF_NO_OVERLAP")) h->overlap = atoi(e) == 0;   // measurement knob
    if (const char* e = getenv("ADF_CONF_BAND")) h->conf_band = atoi(e) != 0;    // measurement knob
    if (const char* e = getenv("ADF_SCALED_FUSE")) h->scaled_fuse = atoi(e) != 0;  // measurement knob
    if (const char* e = getenv("ADF_ROW_WEIGHTS_GUIDE")) h->row_weights_guide = atoi(e) != 0;   // measurement knob
    if (const char* e = getenv("ADF_LO_HALF")) h->scaled_half = atoi(e) != 0;
    if (const char* e = getenv("ADF_LAST_HANDOFF_IMAGE")) h->handoff_image = atoi(e) != 0;   // measurement knob
    if (const char* e = getenv("ADF_INNER_HANDOFF_IMAGE")) h->handoff_inner = atoi(e) != 0;  // measurement knob
    if (const char* e = getenv("ADF_LAST_HANDOFF_MIN_PX")) h->handoff_min_px = atoll(e);      // test knob
    if (const char* e = getenv("ADF_MERGE_SMALL")) h->merge_small = atoi(e) != 0;   // measurement knob
    *out = h;
    return ADF_OK;
}

extern "C" void adf_wls_destroy(adf_wls_t* h)
{
    if (!h) return;
    DeviceScope ds(h->device);
    h->lut.release(); h->ws.release(); h->conf.release(); h->stage.release(); h->scaled.release();
    h->prof.destroy();
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->side) hipStreamDestroy(h->side);
    delete h;
}


extern "C" int adf_wls_set_lambda(adf_wls_t* h, double v) { NEED_HANDLE(h); h->lambda = v; return ADF_OK; }
extern "C" int adf_wls_get_lambda(const adf_wls_t* h, double* v) { NEED_HANDLE(h); if (v) *v = h->lambda; return ADF_OK; }
extern "C" int adf_wls_set_sigma_color(adf_wls_t* h, double v) { NEED_HANDLE(h); h->sigma_color = v; return ADF_OK; }
extern "C" int adf_wls_get_sigma_color(const adf_wls_t* h, double* v) { NEED_HANDLE(h); if (v) *v = h->sigma_color; return ADF_OK; }
extern "C" int adf_wls_set_lrc_thresh(adf_wls_t* h, int v) { NEED_HANDLE(h); h->lrc_thresh = v; return ADF_OK; }
extern "C" int adf_wls_get_lrc_thresh(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->lrc_thresh; return ADF_OK; }
extern "C" int adf_wls_set_depth_discontinuity_radius(adf_wls_t* h, int v) { NEED_HANDLE(h); h->disc_radius = v; return ADF_OK; }
extern "C" int adf_wls_get_depth_discontinuity_radius(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->disc_radius; return ADF_OK; }

extern "C" int adf_wls_set_fgs_params(adf_wls_t* h, double atten, int num_iter)
{
    NEED_HANDLE(h);
    if (num_iter < 1) return fail(ADF_EBADARG, "num_iter must be >= 1 (FGS.cpp:143)");
    h->atten = atten; h->num_iter = num_iter;
    return ADF_OK;
}

extern "C" int adf_wls_set_solver(adf_wls_t* h, int solver)
{
    NEED_HANDLE(h);
    if (solver != ADF_SOLVER_EXACT && solver != ADF_SOLVER_WAVE) return fail(ADF_EBADARG, "unknown solver %d", solver);
    h->solver = solver;
    return ADF_OK;
}
extern "C" int adf_wls_get_solver(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->solver; return ADF_OK; }
extern "C" int adf_wls_get_last_solver(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->last_solver; return ADF_OK; }
extern "C" int adf_wls_get_last_path(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->last_path; return ADF_OK; }
extern "C" int adf_wls_get_last_solver_path(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->last_solver_path; return ADF_OK; }
extern "C" int adf_wls_get_last_handoff(const adf_wls_t* h, int* v) { NEED_HANDLE(h); if (v) *v = h->last_handoff; return ADF_OK; }

extern "C" int adf_wls_get_inner_handoffs(const adf_wls_t* h, int* full, int* tail)
{
    NEED_HANDLE(h);
    if (full) *full = h->last_inner[0];
    if (tail) *tail = h->last_inner[1];
    return ADF_OK;
}

extern "C" int adf_wls_get_device(const adf_wls_t* h, int* device) { NEED_HANDLE(h); if (device) *device = h->device; return ADF_OK; }
extern "C" int adf_wls_get_roi(const adf_wls_t* h, adf_rect* roi) { NEED_HANDLE(h); if (roi) *roi = h->roi; return ADF_OK; }
extern "C" size_t adf_wls_workspace_bytes(const adf_wls_t* h)
{
    return h ? h->ws.bytes + h->conf.bytes + h->stage.bytes + h->scaled.bytes + h->lut.bytes() : 0;
}

extern "C" int adf_wls_sync(adf_wls_t* h, void* stream)
{
    NEED_HANDLE(h);
    DeviceScope ds(h->device);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return ADF_OK;
}

// The confidence planes of a call: n_pairs planes in Geom's cpitch layout.  Whatever lies outside the ROI -- frame
// pixels and row padding alike -- must read as zero; frame pixels are written by the kernels of every call, the padding
// never is, so the buffer is cleared whenever the layout it was last used with changes.
static int ensure_conf_planes(adf_wls* h, const Geom& g, int n_pairs, hipStream_t st)
{
    int rc = h->conf.reserve(g.cframe * sizeof(float) * (size_t)n_pairs, st, FILL_ZERO);
    if (rc) return rc;
    const long long sig[4] = {g.W, g.H, g.cx0, n_pairs};
    if (memcmp(sig, h->conf_sig, sizeof(sig)) != 0) {
        HIP_TRY(hipMemsetAsync(h->conf.p, 0, h->conf.bytes, st));
        memcpy(h->conf_sig, sig, sizeof(sig));
    }
    return ADF_OK;
}

// Row pitch (elements) of the int16 planes q a call on float maps keeps for its confidence kernels: 16-byte rows.
static int quant_pitch(int W) { return round_up(W, 8); }

static size_t wls_pair_ws_bytes(const Geom& g, bool conf, bool wave, bool disc_maps, bool quant_planes, int image_m = 0, bool image_in_chor = false)
{
    // exact: ROI planes CH CV D F0 A0 B0 (+ F1 A1 B1 with confidence); wave: CH CV A0 (+ A1), in place
    // full frames: cL cR, the depth-discontinuity maps (not needed when the one-sweep confidence kernel runs)
    size_t planes = wave ? (conf ? 4 : 3) : (conf ? 9 : 6);
    // float maps (adf_wls_filter_typed_*), confidence mode: the two int16 planes q -- never part of an int16 call's workspace
    // image_m: the register image of the last hand-off (wave_image_floats >= 2 planes): a plane of its own, or Chor's
    // plane and the rest behind it
    return planes * g.plane * sizeof(float) + (conf && disc_maps ? 2 * g.frame * sizeof(float) : 0) +
           (image_m ? (wave_image_floats(g.pw, image_m) - (image_in_chor ? g.plane : 0)) * sizeof(float) : 0) +
           (quant_planes ? 2 * (size_t)quant_pitch(g.W) * g.H * sizeof(int16_t) : 0);
}

// DF.cpp:228-233: the caller's ROI, or what the handle's offsets leave of a w x hgt map
static int resolve_roi(const adf_wls* h, const adf_rect* roi_in, int w, int hgt, adf_rect& roi)
{
    if (roi_in && roi_in->width * roi_in->height != 0) roi = *roi_in;
    else roi = adf_rect{h->left_offset, h->top_offset, w - h->left_offset - h->right_offset, hgt - h->top_offset - h->bottom_offset};
    if (roi.width <= 0 || roi.height <= 0 || roi.x < 0 || roi.y < 0 || roi.x + roi.width > w || roi.y + roi.height > hgt)
        return fail(ADF_ESIZE, "ROI (%d,%d,%d,%d) does not fit a %dx%d map", roi.x, roi.y, roi.width, roi.height, w, hgt);
    return ADF_OK;
}

// The filtered map of a call: CV_16SC1 (adf_wls_filter_*) or, with f32, CV_32FC1 holding the float the int16 epilogue
// rounds (adf_wls_filter_f32_*).  Only the last column pass and the fill outside the ROI know the difference.
struct OutMap {
    void* p; ptrdiff_t stride, pair_stride; bool f32;
    size_t esz() const { return f32 ? sizeof(float) : sizeof(int16_t); }
};

// The disparity maps of a call: CV_16SC1 or, with f32, CV_32FC1 in the same units (adf_wls_filter_typed_*); the right
// map has the left one's depth.
struct DispMaps {
    const void* L; ptrdiff_t sL, psL;
    const void* R; ptrdiff_t sR, psR;
    bool f32;
    size_t esz() const { return f32 ? sizeof(float) : sizeof(int16_t); }
    DispMaps from(int k) const { return DispMaps{pairs_on(L, psL, k), sL, psL, pairs_on(R, psR, k), sR, psR, f32}; }
};

struct View { const uint8_t* p; ptrdiff_t stride, pair_stride; int ch, W, H; };

// One filter call, as check_call has accepted it.  Every entry point -- same size, down-scaled and typed; the host
// entries with their device copies -- builds one, and nothing behind it looks at the caller's arguments again.
struct WlsCall {
    int n_pairs;
    DispMaps dm; int dW, dH;         // the caller's maps and their own size
    View view;                       // W x H
    OutMap om;                       // W x H
    adf_rect rlo, rhi;               // the ROI in map coordinates (getROI(), DF.cpp:139) and in view coordinates
    float resize_factor, x_ratio;    // DF.cpp:225, 241
    bool scaled;                     // the maps are not of the view's size (DF.cpp:224-227, 239-247, 268-277)
};

static int no_right_map() { return fail(ADF_EBADARG, "disparity_map_right is required with use_confidence"); }
static int bad_view_channels() { return fail(ADF_EBADARG, "left_view must be CV_8UC1 or CV_8UC3"); }

// Float maps (include/adf_wls.h): base and strides are multiples of 4 bytes, and the filtered map overlaps neither.
static int check_float_maps(const DispMaps& dm, int n_pairs, int dW, int dH, const OutMap& om, int W, int H)
{
    if (!dm.f32) return ADF_OK;
    if ((reinterpret_cast<uintptr_t>(dm.L) | (uintptr_t)dm.sL | (uintptr_t)dm.psL) & 3u ||
        (dm.R && ((reinterpret_cast<uintptr_t>(dm.R) | (uintptr_t)dm.sR | (uintptr_t)dm.psR) & 3u)))
        return fail(ADF_EBADARG, "a float disparity map needs a 4-byte aligned base and strides");
    // [first byte, last byte] of n_pairs images of `rows` rows of `row_bytes`, whatever the signs of the strides
    auto span = [&](const void* p, ptrdiff_t s, ptrdiff_t ps, size_t row_bytes, int rows, uintptr_t& lo, uintptr_t& hi) {
        const ptrdiff_t a = s * (rows - 1), b = ps * (n_pairs - 1);
        lo = reinterpret_cast<uintptr_t>(p) + (a < 0 ? a : 0) + (b < 0 ? b : 0);
        hi = reinterpret_cast<uintptr_t>(p) + (a > 0 ? a : 0) + (b > 0 ? b : 0) + row_bytes;
    };
    if (!om.p || dW <= 0 || dH <= 0 || W <= 0 || H <= 0 || n_pairs < 1) return ADF_OK;   // (refused by the rules behind this one)
    uintptr_t olo, ohi, mlo, mhi;
    span(om.p, om.stride, om.pair_stride, (size_t)W * om.esz(), H, olo, ohi);
    const void* maps[2] = {dm.L, dm.R}; const ptrdiff_t ss[2] = {dm.sL, dm.sR}, pss[2] = {dm.psL, dm.psR};
    for (int m = 0; m < 2; m++) {
        if (!maps[m]) continue;
        span(maps[m], ss[m], pss[m], (size_t)dW * 4, dH, mlo, mhi);
        if (olo < mhi && mlo < ohi) return fail(ADF_EBADARG, "filtered_disparity_map overlaps a float disparity map");
    }
    return ADF_OK;
}

// THE argument check of DisparityWLSFilter::filter: every rule once, and the record of the accepted call.  The ROI is in
// disparity-map coordinates, like the reference's.  The rules run in one of two orders, because which of two faults a
// call is refused for is part of the interface (tests/test_abi.py and its siblings pin it): a same-size call is checked in
// the reference's order (DF.cpp:221-233, 262-264); a down-scaled call settles its maps and both ROIs before it looks at
// the view and the filtered map.
static int check_call(const adf_wls* h, int n_pairs, const DispMaps& dm, int dW, int dH, const View& view, const OutMap& om,
                      const adf_rect* roi_in, WlsCall& c)
{
    const int W = view.W, H = view.H;
    const bool conf = h->use_confidence;
    c = WlsCall{n_pairs, dm, dW, dH, view, om, adf_rect{0, 0, 0, 0}, adf_rect{0, 0, 0, 0}, 1.0f, 1.0f, !(dW == W && dH == H)};
    const auto short_row = []() -> int { return fail(ADF_ESIZE, "row stride smaller than a row"); };
    const auto refuse_if = [](bool bad, int code, const char* msg) -> int { return bad ? fail(code, "%s", msg) : ADF_OK; };
    const auto maps = [&] { return refuse_if(!dm.L || dW <= 0 || dH <= 0 || W <= 0 || H <= 0, ADF_EBADARG, "disparity_map_left is empty"); };   // DF.cpp:221-222
    const auto guide = [&]() -> int { return !view.p || (view.ch != 1 && view.ch != 3) ? bad_view_channels() : ADF_OK; };
    const auto filtered = [&] { return refuse_if(!om.p, ADF_EBADARG, "filtered_disparity_map is NULL"); };
    const auto pairs = [&] { return refuse_if(n_pairs < 1, ADF_EBADARG, "n_pairs must be >= 1"); };
    const auto map_rows = [&]() -> int { return dm.sL < (ptrdiff_t)(dW * dm.esz()) ? short_row() : ADF_OK; };
    const auto view_rows = [&]() -> int { return om.stride < (ptrdiff_t)(W * om.esz()) || view.stride < (ptrdiff_t)W * view.ch ? short_row() : ADF_OK; };
    const auto float_out = [&] {
        return refuse_if(om.f32 && ((reinterpret_cast<uintptr_t>(om.p) | (uintptr_t)om.stride | (uintptr_t)om.pair_stride) & 3u), ADF_EBADARG,
                         "a float filtered_disparity_map needs a 4-byte aligned base and strides");
    };
    const auto right_map = [&]() -> int {                                  // DF.cpp:262-264
        if (!conf || !dm.R) return conf ? no_right_map() : ADF_OK;
        return refuse_if(dm.sR < (ptrdiff_t)(dW * dm.esz()), ADF_ESIZE, "right disparity stride smaller than a row");
    };
    const auto radius = [&]() -> int {
        return conf && (h->disc_radius < 0 || h->disc_radius > max_disc_radius())
                   ? fail(ADF_EBADARG, "depth discontinuity radius %d outside [0,%d]", h->disc_radius, max_disc_radius()) : ADF_OK;
    };
    const auto smoothness = [&] { return refuse_if(h->lambda < 0 || h->sigma_color < 0, ADF_EBADARG, "lambda and sigma_color must be >= 0 (FGS.cpp:143)"); };
    const auto map_roi = [&] { return resolve_roi(h, roi_in, dW, dH, c.rlo); };
    const auto view_roi = [&]() -> int {                                   // DF.cpp:225, 241-242, 270-271
        c.resize_factor = dW / (float)W;
        const float x_ratio = c.x_ratio = W / (float)dW, y_ratio = H / (float)dH;
        c.rhi = adf_rect{(int)(c.rlo.x * x_ratio), (int)(c.rlo.y * y_ratio), (int)(c.rlo.width * x_ratio), (int)(c.rlo.height * y_ratio)};
        if (c.rhi.width > 0 && c.rhi.height > 0 && c.rhi.x + c.rhi.width <= W && c.rhi.y + c.rhi.height <= H) return ADF_OK;
        return fail(ADF_ESIZE, "scaled ROI (%d,%d,%d,%d) does not fit the %dx%d view", c.rhi.x, c.rhi.y, c.rhi.width, c.rhi.height, W, H);
    };
    int rc = check_float_maps(dm, n_pairs, dW, dH, om, W, H);
    if (rc || (rc = maps())) return rc;
    if (!c.scaled) {
        if ((rc = guide()) || (rc = filtered()) || (rc = pairs()) || (rc = map_rows()) || (rc = view_rows()) || (rc = float_out()) ||
            (rc = right_map()) || (rc = smoothness()) || (rc = map_roi()) || (rc = radius())) return rc;
        c.rhi = c.rlo;                                                     // DF.cpp:224-227: resize_factor 1
        return ADF_OK;
    }
    if ((rc = pairs()) || (rc = map_rows()) || (rc = right_map()) || (rc = radius()) || (rc = map_roi()) || (rc = view_roi()) ||
        (rc = guide()) || (rc = filtered()) || (rc = view_rows()) || (rc = float_out()) || (rc = smoothness())) return rc;
    return ADF_OK;
}

// Stand-in for a device block that is not allocated yet, in alignment checks: hipMalloc returns 256-byte aligned memory.
static float* const UNALLOCATED = reinterpret_cast<float*>(uintptr_t(256));

// The wave solver's fit checks take a pass's arguments: those of a first row pass of `len` columns fed from `f`.
static WavePassArgs first_pass_probe(const FusedInputs& f, int len)
{
    WavePassArgs a{};
    a.fuse = f; a.len = len;
    return a;
}

// What the kernels of a range of pairs read of the disparity maps.  caller_maps() starts one; quantise_maps() and the
// down-scaled path's buffers re-point it.
struct MapSource {
    // the confidence kernels' int16 maps: the caller's, or the planes q of float maps (null: float maps not quantised)
    const int16_t* L; ptrdiff_t sL, psL;
    const int16_t* R; ptrdiff_t sR, psR;
    // what the right-hand sides are formed from: the caller's left maps (a float one: DEPTH_WLS_F32) or the down-scaled
    // path's resized ones (a float one is taken as it is: ADF_32F); null where the first row pass interpolates the
    // low-resolution maps itself
    const void* rhs; ptrdiff_t s_rhs, ps_rhs; int rhs_depth;
    // down-scaled path, float maps: the left map's v plane -- resized in float, no rounding
    const float* v; ptrdiff_t sv, psv;
    bool rhs_f32() const { return rhs_depth != ADF_16S; }
    MapSource from(int k) const                                            // the same for the pairs from k on
    {
        MapSource m = *this;
        m.L = pairs_on(L, psL, k); m.R = pairs_on(R, psR, k); m.rhs = pairs_on(rhs, ps_rhs, k); m.v = pairs_on(v, psv, k);
        return m;
    }
};

static MapSource caller_maps(const DispMaps& dm)
{
    MapSource m{};
    if (!dm.f32) { m.L = (const int16_t*)dm.L; m.sL = dm.sL; m.psL = dm.psL; m.R = (const int16_t*)dm.R; m.sR = dm.sR; m.psR = dm.psR; }
    m.rhs = dm.L; m.s_rhs = dm.sL; m.ps_rhs = dm.psL; m.rhs_depth = dm.f32 ? DEPTH_WLS_F32 : ADF_16S;
    return m;
}

// Float maps: what the confidence kernels read is made by one launch (design (a)) -- the int16 planes q of the `n` pairs
// of `dm` at qL / qR (null: none) and the left map's v as a float plane at v (null: none).  `m` reads them from then on.
static int quantise_maps(Profiler* prof, const DispMaps& dm, int W, int H, int n, int16_t* qL, int16_t* qR, float* v,
                         hipStream_t st, MapSource& m)
{
    const int pitch = quant_pitch(W);
    const size_t frame = (size_t)pitch * H;                                // elements per plane
    QuantArgs qa{{dm.L, qR ? dm.R : nullptr}, {dm.sL, dm.sR}, {dm.psL, dm.psR}, {qL, qR}, v, W, H, pitch, frame, n};
    {
        ProfScope ps(prof, K_QUANT, quant_bytes((double)W * H * n, qL != nullptr, qR != nullptr, v != nullptr), st);
        HIP_TRY(launch_quantise_maps(qa, st));
    }
    m.L = qL; m.R = qR; m.sL = m.sR = (ptrdiff_t)pitch * 2; m.psL = m.psR = (ptrdiff_t)frame * 2;
    m.v = v; m.sv = (ptrdiff_t)pitch * 4; m.psv = (ptrdiff_t)frame * 4;
    return ADF_OK;
}

// Fused first row pass at view resolution: U1 = conf, U0 = conf*float(dL) read from the confidence planes from `conf`
// on and the maps the right-hand sides come from (DF.cpp:288-290).
static FusedInputs view_fuse(const float* conf, const MapSource& m, const Geom& g)
{
    FusedInputs f{};
    f.dl_f32 = m.rhs_f32() ? 1 : 0;
    f.conf_in = conf; f.conf_frame = g.cframe; f.conf_pitch = g.cpitch; f.conf_x0 = g.cx0 + g.rx; f.conf_y0 = g.ry;
    f.dl_in = m.rhs; f.dl_stride = m.s_rhs; f.dl_pair_stride = m.ps_rhs; f.dl_x0 = g.rx; f.dl_y0 = g.ry;
    return f;
}

// ... and in its low-resolution form (DF.cpp:272-274 then 288-290): the pass interpolates the low-resolution confidence
// maps from `clo` on (made by the band kernel: zero outside the ROI) and the int16 maps of `m`; g: the view's geometry.
static FusedInputs lo_fuse(const adf_wls* h, const WlsCall& c, bool band_map, const float* clo, const MapSource& m, float* taps, const Geom& g)
{
    FusedInputs f{};
    f.lo_conf = clo; f.lo_conf_stride = c.dW; f.lo_conf_pair = (ptrdiff_t)((size_t)c.dW * c.dH);
    f.lo_dl = m.L; f.lo_dl_stride = m.sL; f.lo_dl_pair = m.psL;
    f.lo_w = c.dW; f.lo_h = c.dH; f.hi_x0 = g.rx; f.hi_y0 = g.ry;
    f.lo_scale_x = (double)c.dW / g.W; f.lo_scale_y = (double)c.dH / g.H; f.lo_post_scale = c.x_ratio;
    if (band_map) {
        f.lo_zero_outside = 1; f.lo_vx0 = c.rlo.x; f.lo_vy0 = c.rlo.y; f.lo_vx1 = c.rlo.x + c.rlo.width; f.lo_vy1 = c.rlo.y + c.rlo.height;
    }
    f.lo_taps = taps; f.lo_half = h->scaled_half ? 1 : 0;
    return f;
}

// cv::resize of the low-resolution confidence maps into the handle's view-sized planes (DF.cpp:274)
static int resize_conf_planes(adf_wls_t* h, const ConfResize& c, hipStream_t st, Profiler* prof)
{
    const size_t lo = (size_t)c.dW * c.dH;
    const Geom& ghi = c.ghi;
    ResizeArgs rc32{c.clo, (ptrdiff_t)c.dW * 4, (ptrdiff_t)(lo * 4), c.dW, c.dH, (float*)h->conf.p + ghi.cx0, (ptrdiff_t)ghi.cpitch * 4,
                    (ptrdiff_t)(ghi.cframe * 4), ghi.W, ghi.H, (double)c.dW / ghi.W, (double)c.dH / ghi.H, 1.0f, 0};
    if (c.band_map) { rc32.zero_outside = 1; rc32.vx0 = c.rlo.x; rc32.vy0 = c.rlo.y; rc32.vx1 = c.rlo.x + c.rlo.width; rc32.vy1 = c.rlo.y + c.rlo.height; }
    ProfScope ps(prof, K_RESIZE, resize_bytes((double)ghi.W * ghi.H * c.n_pairs, (double)lo * c.n_pairs, 4.0), st);
    HIP_TRY(launch_resize_linear(rc32, c.n_pairs, st));
    return ADF_OK;
}

// cv::resize of the low-resolution left maps of all pairs to the view, times x_ratio (DF.cpp:243-244, 272-273), into
// `dhi`, where lo.rhs reads them: the int16 maps saturated; float maps' v through the float taps the confidence map
// goes through, nothing rounded.
static int resize_disparity(Profiler* prof, const WlsCall& c, const MapSource& lo, void* dhi, hipStream_t st)
{
    const int W = c.view.W, H = c.view.H;
    const double sx = (double)c.dW / W, sy = (double)c.dH / H;
    const ResizeArgs ra = lo.v ? ResizeArgs{lo.v, lo.sv, lo.psv, c.dW, c.dH, dhi, lo.s_rhs, lo.ps_rhs, W, H, sx, sy, c.x_ratio, 0}
                               : ResizeArgs{lo.L, lo.sL, lo.psL, c.dW, c.dH, dhi, lo.s_rhs, lo.ps_rhs, W, H, sx, sy, c.x_ratio, 1};
    ProfScope ps(prof, K_RESIZE, resize_bytes((double)W * H * c.n_pairs, (double)c.dW * c.dH * c.n_pairs, lo.v ? 4.0 : 2.0), st);
    HIP_TRY(launch_resize_linear(ra, c.n_pairs, st));
    return ADF_OK;
}

// How a WLS filter call makes its confidence map (DF.cpp:197-210), or none (DF.cpp:257).
enum ConfStage {
    CONF_NONE,        // no confidence
    CONF_SCALED,      // down-scaled: low-resolution confidence map, then both resizes
    CONF_SCALED_LO,   // down-scaled: low-resolution confidence map; the first row pass interpolates it and the disparity map
    CONF_MERGED,      // weights + one-sweep confidence map + fill outside the ROI in one launch (small calls)
    CONF_BAND,        // both views' maps, LRC and x255 in one band sweep: the right view's map lives in LDS only
    CONF_LEFT,        // the right view's map, then the left one + LRC + x255 in one sweep (cL never hits memory)
    CONF_TWO_KERNEL,  // both views' maps, then LRC + x255 (+ the right-hand sides and the fill outside the ROI)
};

// Where the first row pass finds the two right-hand sides conf*disp and conf (DF.cpp:286-290), or float(disp) without
// confidence (DF.cpp:257).
enum RhsSource {
    RHS_PLAIN,          // the plain prologue writes float(disp) (FGS.cpp:203-205)
    RHS_FUSED_VIEW,     // the pass forms them itself from the view-sized confidence planes and maps (no prologue planes)
    RHS_FUSED_LO,       // ... from the low-resolution ones, which it interpolates
    RHS_CONF_PROLOGUE,  // the confidence-weighted prologue: the down-scaled path's, and float maps' behind the left-view kernel
    RHS_CONF_KERNEL,    // the left-view or the LRC kernel writes them with the confidence map
};

// The numbers the confidence kernels take besides maps and geometry, for maps `resize_factor` times the view's size.
struct ConfRule { int rrx, thresh, radius; float roll_off; };
static ConfRule conf_rule(const adf_wls* h, const WlsCall& c)
{
    return ConfRule{c.dW - (c.rlo.x + c.rlo.width),                                        // DF.cpp:202
                    (int)(c.resize_factor * h->lrc_thresh),                               // DF.cpp:318
                    h->disc_radius, h->roll_off / (c.resize_factor * c.resize_factor)};   // DF.cpp:359
}

// What a confidence stage writes.
struct ConfOut {
    float* conf;                        // the confidence planes (x255), in the layout of the stage's Geom
    float* cL; float* cR;               // full-frame discontinuity maps (not the band kernel)
    float* U0; float* U1; int orient;   // the right-hand sides (null: not this stage's; the band kernel never)
    const OutsideArgs* fill;            // two-kernel: its LRC kernel also fills the filtered map outside the ROI (DF.cpp:284)
};

static ConfBandArgs conf_band_args(const MapSource& m, float* conf, const Geom& g, const ConfRule& r)
{
    return ConfBandArgs{m.L, m.sL, m.psL, m.R, m.sR, m.psR, conf, g, r.rrx, r.thresh, r.radius, r.roll_off, 0};
}

static DiscArgs disc_args(const MapSource& m, const ConfOut& o, const Geom& g, const ConfRule& r, int only_view)
{
    return DiscArgs{{m.L, m.R}, {m.sL, m.sR}, {m.psL, m.psR}, {g.rx, r.rrx}, g.ry, g.rw, g.rh, r.radius, r.roll_off,
                    {o.cL, o.cR}, g.W, g.frame, only_view};
}

static LrcArgs lrc_args(const MapSource& m, const ConfOut& o, const Geom& g, const ConfRule& r)
{
    // right-hand sides of float maps: the kernel reads its own pixel from the caller's left map (v, and q on the fly),
    // the gather from the right map's plane q
    const bool own_f32 = o.U0 && m.rhs_f32();
    LrcArgs a = LrcArgs{m.L, m.sL, m.psL, m.R, m.sR, m.psR, o.cL, o.cR, o.conf, nullptr, 0, 0, 0, 0, o.U0, o.U1,
                        g, r.rrx, r.thresh, o.orient, own_f32 ? 1 : 0};
    if (own_f32) { a.dL = (const int16_t*)m.rhs; a.sL = m.s_rhs; a.psL = m.ps_rhs; }
    if (o.fill) { a.out = o.fill->out; a.sO = o.fill->stride; a.psO = o.fill->pair_stride; a.fill = o.fill->fill; a.out_f32 = o.fill->out_f32; }
    return a;
}

// Queues the confidence map of `n` pairs from the int16 maps of `m` at geometry `g` (DF.cpp:197-210): the band, the
// left-view or the two-kernel stage.  The view-resolution chunk and the down-scaled path's low-resolution map both come
// here.
static int conf_stage(Profiler* prof, ConfStage kind, const MapSource& m, const Geom& g, const ConfRule& r, const ConfOut& o,
                      int n, hipStream_t st)
{
    const double F = (double)g.frame * n, P = (double)g.rw * g.rh * n;
    if (kind == CONF_BAND) {
        ProfScope ps(prof, K_LRC, band_bytes(P), st);
        HIP_TRY(launch_conf_band(conf_band_args(m, o.conf, g, r), n, st));
        return ADF_OK;
    }
    {
        ProfScope ps(prof, K_DISC, disc_bytes(P, kind != CONF_LEFT), st);
        HIP_TRY(launch_discontinuity(disc_args(m, o, g, r, kind == CONF_LEFT ? 1 : -1), n, st));   // DF.cpp:204 (left: the right view)
    }
    if (kind == CONF_LEFT) {
        ConfLeftArgs ca{m.L, m.sL, m.psL, m.R, m.sR, m.psR, o.cR, o.conf, o.U0, o.U1, g, r.rrx, r.thresh, r.radius, r.roll_off};
        ProfScope ps(prof, K_LRC, conf_left_bytes(P, o.U0 != nullptr), st);
        HIP_TRY(launch_conf_left(ca, n, st));                              // DF.cpp:204-209 (+288-290)
        return ADF_OK;
    }
    const double fill = o.fill ? fill_bytes(F - P, false, o.fill->out_f32 ? 4.0 : 2.0).alg : 0.0;
    ProfScope ps(prof, K_LRC, lrc_bytes(F, P, o.U0 != nullptr, m.rhs_f32() ? 4.0 : 2.0, fill), st);
    HIP_TRY(launch_lrc_prologue(lrc_args(m, o, g, r), n, st));             // DF.cpp:208-209 (+288-290)
    return ADF_OK;
}

// What one chunk of pairs queues.
struct ChunkPlan {
    ConfStage stage;
    bool fork_weights;     // the weight kernel runs on the side stream, beside the confidence kernels
    bool outside_on_side;  // ... behind the fill outside the ROI
    bool guide_rows;       // the row passes form their weights from the guide: the weight kernel writes Cvert only
    bool image;            // the last row pass hands the last column pass its register image instead of the pair plane
    bool inner_image;      // ... and so do the row passes before it, each to the column pass of its iteration
};

// What a WLS filter call queues, decided from its record before anything is allocated or queued.
struct WlsPlan {
    Geom g;                   // the view's geometry
    bool wave;                // the wave solver (else the exact one)
    RhsSource rhs;
    bool band;                // the one-sweep confidence kernel: no full-frame discontinuity maps in the workspace
    bool quant_planes;        // float maps of the view's size, confidence mode: the workspace holds a chunk's planes q
    // down-scaled: the maps' geometry (plain confidence layout); the band kernel makes the low-resolution confidence
    // maps (zero outside the ROI, DF.cpp:187-190); bytes per pair of the resized left maps (none with RHS_FUSED_LO)
    Geom glo; bool lo_band; size_t dhi_bytes;
    size_t per_pair; int chunk;
    int image_m;              // the workspace holds a register image for the last hand-off, laid out for this chunk length (0: none)
    bool image_in_chor;       // ... whose first g.plane floats per pair are Chor's plane, which no kernel of the call touches
    bool first_image;         // the fused first row pass has the image form (a FUSE_VIEW pass on an int16 map)
    // chunks of `chunk` pairs, and a shorter last one: the merged launch is for small calls, so it depends on the
    // chunk's pair count
    ChunkPlan full, tail;
    int path;                 // ADF_PATH_* bits of the preparation stage
    int solver_path;          // ... of the solve passes
    bool fused_first() const { return rhs == RHS_FUSED_VIEW || rhs == RHS_FUSED_LO; }
};

static ChunkPlan plan_chunk(const adf_wls* h, ConfStage stage, bool wave, bool guide_rows, bool image, bool inner_image)
{
    // confidence mode: the weights depend on the guide only and the confidence kernels on the disparity maps only -- one
    // is bound by memory latency, the others lean on the vector ALUs -- so the weight kernel is forked onto the side
    // stream and joined before the first solve pass (not beside the merged launch, which computes it)
    const bool fork = stage != CONF_NONE && stage != CONF_MERGED && h->overlap;
    // the fill of everything outside the ROI (DF.cpp:284, :187-190) touches no pixel any other kernel of the call
    // touches: on the wave path it rides the side stream too instead of sitting between the confidence kernel and the
    // first solve pass (one dependent launch less on the critical path of a single-pair call) -- and it goes FIRST
    // there: alone it takes 0.08 ms of a 64 x 4K step on the StereoBM factory's ROI, but queued behind the weight kernel
    // it starts when the confidence kernel's workgroups hold nearly every register of every CU and crawls through 0.8 ms
    // as the call's tail (round 3).  The two-kernel stage fills in its LRC kernel.
    // (the merged launch for small calls writes both weight planes: those are bound by latency, not bytes)
    return ChunkPlan{stage, fork, fork && wave && stage != CONF_TWO_KERNEL, guide_rows && stage != CONF_MERGED, image, image && inner_image};
}

// The row passes' weights straight from the guide of the pairs from `guide` on (fgs_wave_h.hip, WS_GUIDE*).
static GuideWeights guide_weights(const adf_wls* h, const uint8_t* guide, const View& v, const Geom& g)
{
    return GuideWeights{guide, v.stride, v.pair_stride, v.ch, g.rx, g.ry, h->lut.cur};
}

static WlsPlan plan_wls(const adf_wls* h, const WlsCall& c)
{
    WlsPlan p{};
    const bool conf = h->use_confidence, f32in = c.dm.f32;
    const View& v = c.view;
    const Geom g = p.g = make_geom(v.W, v.H, c.rhi.x, c.rhi.y, c.rhi.width, c.rhi.height);
    // sizes outside the register-resident kernels' range fall back to the exact solver
    p.wave = h->solver == ADF_SOLVER_WAVE && wave_fits(g);
    // what the right-hand sides would be read from: the caller's maps or, down-scaled, the resized ones (not allocated yet)
    MapSource m = caller_maps(c.dm);
    bool fuse_lo = false;
    if (c.scaled) {
        p.glo = plain_conf_layout(make_geom(c.dW, c.dH, c.rlo.x, c.rlo.y, c.rlo.width, c.rlo.height));
        p.lo_band = conf && h->conf_band && conf_band_fits(p.glo, h->disc_radius);
        // Can the first row pass interpolate the maps itself (fgs_wave_h.hip, FUSE_LO)?  Confidence mode on the wave
        // solver, scale factors within the staging buffer's reach.  Then neither the resized disparity map nor -- until
        // getConfidenceMap() asks for it -- the resized confidence map is ever written.
        // (float maps take the resize kernels: the fused low-resolution prologue has no float form)
        fuse_lo = conf && !f32in && h->scaled_fuse && p.wave &&
                  wave_hpass_can_fuse_lo(first_pass_probe(lo_fuse(h, c, p.lo_band, UNALLOCATED, m, nullptr, g), g.rw));
        p.dhi_bytes = fuse_lo ? 0 : pad_to((size_t)v.W * v.H * c.dm.esz(), 256);
        m.rhs = fuse_lo ? nullptr : UNALLOCATED; m.s_rhs = (ptrdiff_t)(v.W * c.dm.esz()); m.ps_rhs = (ptrdiff_t)p.dhi_bytes;
        m.rhs_depth = f32in ? ADF_32F : ADF_16S;
    }
    ConfStage stage = !conf ? CONF_NONE
                    : c.scaled ? (fuse_lo ? CONF_SCALED_LO : CONF_SCALED)
                    : (p.wave && h->disc_radius <= conf_left_max_radius()) ? CONF_LEFT : CONF_TWO_KERNEL;
    // The view-resolution form of the fused first pass has alignment conditions that depend only on the geometry, the
    // strides and the pointers known here, not on the chunk.
    const float* planes = h->conf.p ? (const float*)h->conf.p : UNALLOCATED;
    const bool fused_view = ((stage == CONF_SCALED && !f32in) || stage == CONF_LEFT) && p.wave &&   // (a resized float map is not clamped again: prologue)
                            wave_hpass_can_fuse(first_pass_probe(view_fuse(planes, m, g), g.rw));
    // the band kernel writes no right-hand sides: it needs the fused first pass
    p.band = stage == CONF_LEFT && fused_view && h->conf_band && conf_band_fits(g, h->disc_radius);
    if (p.band) stage = CONF_BAND;
    p.quant_planes = f32in && conf && !c.scaled;
    p.rhs = stage == CONF_NONE ? RHS_PLAIN : stage == CONF_SCALED_LO ? RHS_FUSED_LO : fused_view ? RHS_FUSED_VIEW
          : (stage == CONF_SCALED || (stage == CONF_LEFT && p.quant_planes)) ? RHS_CONF_PROLOGUE : RHS_CONF_KERNEL;
    // The guide is new on every call, so the Chor plane of a full-resolution call on the wave solver is written once and
    // read num_iter times for nothing the guide row does not say in fewer bytes: the row passes take the guide instead
    // where their bucket has that form and the streaming weight kernel (the one with a Cvert-only form) runs.
    bool guide_rows = false;
    if (p.wave && !c.scaled && h->row_weights_guide) {
        WavePassArgs probe{};
        probe.len = g.rw; probe.gw = guide_weights(h, v.p, v, g);
        WeightArgs wprobe{};
        wprobe.stride = v.stride; wprobe.ch = v.ch; wprobe.chor_orient = ORIENT_N; wprobe.g = g;
        guide_rows = wave_hpass_guide_fits(probe) && weights_stream_fits(wprobe);
    }
    // The last hand-off as the last column pass's register image: two right-hand sides on the wave solver, a row pass
    // that is not the fused first one (num_iter >= 2), one-wave rows, whole-strip columns -- and a chunk of at least
    // handoff_min_px ROI pixels, counted with the image's plane in the workspace.  Where no chunk of the call can write
    // Chor -- the row passes take the guide and not even a one-pair chunk is small enough for the merged launch, which
    // writes both weight planes -- Chor's carved-but-untouched plane is the image's first part (image_in_chor) and the
    // workspace grows by the rest only.
    const int image_m = (conf && p.wave && h->handoff_image && h->num_iter >= 2 && wave_hpass_image_fits(g.rw)) ? wave_vpass_image_m(g.rh) : 0;
    const long long roi_px = (long long)g.rw * g.rh;
    const bool may_merge = p.band && h->merge_small && prep_small_fits(g, h->disc_radius, v.ch, 1) && prep_small_guide_fits(g, v.stride, v.ch);
    auto chunk_for = [&](int im) {
        p.image_m = im;
        p.image_in_chor = im && guide_rows && !may_merge;
        p.per_pair = wls_pair_ws_bytes(g, conf, p.wave, !p.band, p.quant_planes, im, p.image_in_chor);
        p.chunk = (int)(h->ws_limit / p.per_pair);
        if (p.chunk < 1) p.chunk = 1;
        if (p.chunk > c.n_pairs) p.chunk = c.n_pairs;
    };
    chunk_for(image_m);
    if (image_m && roi_px * p.chunk < h->handoff_min_px) chunk_for(0);
    auto chunk_of = [&](int n) {
        const bool merged = p.band && h->merge_small && prep_small_fits(g, h->disc_radius, v.ch, n) && prep_small_guide_fits(g, v.stride, v.ch);
        // (the inner hand-offs under the last one's conditions: the batch-size series of profiles/inner_handoff_ab.txt)
        return plan_chunk(h, merged ? CONF_MERGED : stage, p.wave, guide_rows, p.image_m && roi_px * n >= h->handoff_min_px, h->handoff_inner);
    };
    p.first_image = p.rhs == RHS_FUSED_VIEW && wave_hpass_first_image(view_fuse(planes, m, g));
    p.full = chunk_of(p.chunk);
    p.tail = chunk_of(c.n_pairs % p.chunk ? c.n_pairs % p.chunk : p.chunk);
    p.path = ((p.band || p.lo_band) ? ADF_PATH_CONF_BAND : 0) |
             (p.fused_first() ? ADF_PATH_FUSED_FIRST_PASS : 0) |
             ((p.full.stage == CONF_MERGED || p.tail.stage == CONF_MERGED) ? ADF_PATH_MERGED_PREP : 0);
    p.solver_path = (p.full.guide_rows || p.tail.guide_rows) ? ADF_PATH_ROW_WEIGHTS_GUIDE : 0;
    if (p.rhs == RHS_FUSED_LO)
        p.path |= ADF_PATH_SCALED_FUSED |
                  (wave_hpass_lo_half(first_pass_probe(lo_fuse(h, c, p.lo_band, UNALLOCATED, m, nullptr, g), g.rw)) ? ADF_PATH_SCALED_HALF : 0);
    return p;
}

// The down-scaled path's own buffers in h->scaled, for ALL pairs of a call: the resized left maps (none with
// RHS_FUSED_LO) and, in confidence mode, the low-resolution discontinuity and confidence maps; the scratch for the
// columns' source coordinates of the fused low-resolution first pass; for float maps v and, in confidence mode, qL qR.
struct ScaledBufs { char* dhi; float *cl, *cr, *clo; float* taps; };

// Carves them, sizes the view-sized confidence planes and, for float maps, makes q and v: `lo` is what the kernels
// read of the maps from then on.
static int scaled_buffers(adf_wls_t* h, const WlsCall& c, const WlsPlan& plan, hipStream_t st, ScaledBufs& b, MapSource& lo)
{
    const bool conf = h->use_confidence, f32in = c.dm.f32, fuse_lo = plan.rhs == RHS_FUSED_LO;
    const size_t n = (size_t)c.n_pairs, lo_px = (size_t)c.dW * c.dH;
    const size_t qframe = (size_t)quant_pitch(c.dW) * c.dH;
    const size_t maps_bytes = pad_to(n * (plan.dhi_bytes + (conf ? 3 * lo_px * sizeof(float) : 0)), 256);
    const size_t taps_bytes = pad_to(fuse_lo ? 2 * ((size_t)c.rhi.width + 4) * sizeof(float) : 0, 256);
    const size_t quant_bytes = f32in ? n * qframe * (4 + (conf ? 4 : 0)) : 0;   // v (float) + the two planes q (int16), per pair
    int rc = h->scaled.reserve(maps_bytes + taps_bytes + quant_bytes, st, FILL_ZERO);
    if (rc) return rc;
    b.dhi = (char*)h->scaled.p;
    b.cl = (float*)(b.dhi + n * plan.dhi_bytes);
    b.cr = b.cl + n * lo_px;
    b.clo = b.cr + n * lo_px;
    b.taps = fuse_lo ? (float*)(b.dhi + maps_bytes) : nullptr;
    if (conf && (rc = ensure_conf_planes(h, plan.g, c.n_pairs, st))) return rc;
    lo = caller_maps(c.dm);
    if (f32in) {
        float* v = (float*)(b.dhi + maps_bytes + taps_bytes);
        int16_t* qL = conf ? (int16_t*)(v + n * qframe) : nullptr;
        int16_t* qR = conf ? qL + n * qframe : nullptr;
        if ((rc = quantise_maps(&h->prof, c.dm, c.dW, c.dH, c.n_pairs, qL, qR, v, st, lo))) return rc;
    }
    lo.rhs = fuse_lo ? nullptr : b.dhi; lo.s_rhs = (ptrdiff_t)(c.view.W * c.dm.esz()); lo.ps_rhs = (ptrdiff_t)plan.dhi_bytes;
    lo.rhs_depth = f32in ? ADF_32F : ADF_16S;                              // (a resized float map is taken as it is)
    return ADF_OK;
}

// The down-scaled path's confidence maps of ALL pairs (DF.cpp:268-277): the low-resolution map, then the resizes of it
// and of the left maps to the view -- or neither where the first row pass interpolates both.  wls_filter_impl queues this
// on the caller's stream where a same-size call runs its confidence kernels -- beside the weight kernel, which it has
// forked to the side stream by then and which needs the view only.
// Measured at 64 x 4K views / 1080p maps: everything after the fork 13.8-14.1 / 13.8-14.0 ms per call (radius 2 / 5; the
// band kernel crawls beside the weight kernel's small workgroups, 0.44 -> 0.9-1.7 ms, but the resizes then run alone),
// the low-resolution confidence map before the fork 14.20 / 14.51 (two memory-bound kernels side by side gain nothing),
// no overlap at all 14.49 / 14.69.
static int scaled_conf_maps(adf_wls_t* h, const WlsCall& c, const WlsPlan& plan, const ScaledBufs& b, const MapSource& lo,
                            const ConfRule& rule, hipStream_t st)
{
    Profiler* prof = &h->prof;
    int rc = conf_stage(prof, plan.lo_band ? CONF_BAND : CONF_TWO_KERNEL, lo, plan.glo, rule, ConfOut{b.clo, b.cl, b.cr}, c.n_pairs, st);
    if (rc) return rc;
    const ConfResize cr{b.clo, c.dW, c.dH, c.rlo, plan.g, plan.lo_band, c.n_pairs};
    if (plan.rhs != RHS_FUSED_LO)
        return (rc = resize_conf_planes(h, cr, st, prof)) ? rc : resize_disparity(prof, c, lo, b.dhi, st);
    // a call captured into a graph is replayed without this host code: the view-sized confidence maps are made
    // inside the call (the graph), so getConfidenceMap() stays current after replays; otherwise on demand
    if (stream_is_capturing(st)) return resize_conf_planes(h, cr, st, prof);
    h->lazy_conf = adf_wls::LazyConf{true, cr};
    return ADF_OK;
}

// One accepted call by its plan: the workspace, then per chunk of pairs a fixed sequence -- fork, outside fill and
// weights, quantise, confidence stage, right-hand sides, join, passes.
static int wls_filter_impl(adf_wls_t* h, const WlsCall& c, const WlsPlan& plan, hipStream_t st)
{
    const bool conf = h->use_confidence, wave = plan.wave;
    const Geom& g = plan.g;
    const View& vw = c.view;
    const OutMap& om = c.om;
    const adf_rect& roi = c.rhi;
    const int n_pairs = c.n_pairs, W = vw.W, H = vw.H, gch = vw.ch;
    const double ob_px = (double)om.esz(), db_px = (double)c.dm.esz();     // bytes per pixel of the filtered map, of the maps
    Profiler* prof = &h->prof;
    int rc;
    ScaledBufs sb{};
    MapSource lo{};
    if (c.scaled && (rc = scaled_buffers(h, c, plan, st, sb, lo))) return rc;
    h->roi = roi; h->last_W = W; h->last_H = H; h->last_pairs = n_pairs;
    h->last_cpitch = g.cpitch; h->last_cx0 = g.cx0; h->last_path = 0; h->last_solver_path = 0;
    h->last_solver = wave ? ADF_SOLVER_WAVE : ADF_SOLVER_EXACT;
    h->last_handoff = ADF_HANDOFF_PAIR_PLANE; h->last_inner[0] = h->last_inner[1] = 0;
    if ((rc = h->ws.reserve(plan.per_pair * (size_t)plan.chunk, st, FILL_ZERO))) return rc;
    if (conf && !c.scaled && (rc = ensure_conf_planes(h, g, n_pairs, st))) return rc;
    {
        const long long sig[8] = {W, H, roi.x, roi.y, roi.width, roi.height,
                                  (long long)plan.image_in_chor * 1024 + (long long)plan.image_m * 16 + (long long)plan.quant_planes * 8 + (long long)plan.band * 4 + (long long)wave * 2 + conf, plan.chunk};
        if (memcmp(sig, h->ws_sig, sizeof(sig)) != 0) {
            HIP_TRY(hipMemsetAsync(h->ws.p, 0, h->ws.bytes, st));
            memcpy(h->ws_sig, sig, sizeof(sig));
        }
    }
    // carve the workspace
    float* base = (float*)h->ws.p;
    auto take = [&](size_t elems) { float* p = base; base += elems * (size_t)plan.chunk; return p; };
    SolvePlanes p{};
    p.CH = take(g.plane);
    // the last hand-off's register image in Chor's plane (all pairs' planes, contiguous) and what it needs beyond it
    float* const image_rest = plan.image_in_chor ? take(wave_image_floats(g.pw, plan.image_m) - g.plane) : nullptr;
    (void)image_rest;
    p.CV = take(g.plane); p.A0 = take(g.plane);
    if (!wave) { p.D = take(g.plane); p.F0 = take(g.plane); p.B0 = take(g.plane); }
    float *cL = nullptr, *cR = nullptr;
    if (conf) {
        p.A1 = take(g.plane);                     // wave: directly behind A0 (the pair plane spans both)
        if (!wave) { p.F1 = take(g.plane); p.B1 = take(g.plane); }
    }
    // the last hand-off's register image: rows past the ROI's last one are never written and must read as zeros (finite
    // is what the column pass needs), which the zero fill on a signature change above gives
    float* const image = !plan.image_m ? nullptr : plan.image_in_chor ? p.CH : take(wave_image_floats(g.pw, plan.image_m));
    // float maps: the planes q of a chunk (before the full-frame maps: everything in front is a multiple of 256 bytes, so
    // the planes' rows are 16-byte aligned); 2 * qframe int16 = qframe floats per pair
    const size_t qframe = (size_t)quant_pitch(W) * H;
    int16_t* const qL = plan.quant_planes ? (int16_t*)take(qframe) : nullptr;
    int16_t* const qR = qL ? qL + qframe * (size_t)plan.chunk : nullptr;
    if (conf && !plan.band) { cL = take(g.frame); cR = take(g.frame); }
    // exact: the horizontal pass wants the row index fastest (T); wave: row-major (N), except that two
    // right-hand sides share one interleaved pair plane (A0 and A1 are adjacent: 2*plane floats per
    // image starting at A0) and Cvert is strip-major -- see fgs_wave_common.h
    const int orient_h = wave ? ORIENT_N : ORIENT_T;
    const int orient_u2 = wave ? ORIENT_PAIR : ORIENT_T;     // the two right-hand sides of a confidence-mode call
    const int orient_cv = wave ? ORIENT_STRIP : ORIENT_N;
    const int16_t fill = (int16_t)(16 * (h->min_disp - 1));            // DF.cpp:254,284
    const ConfRule rule = conf_rule(h, c);
    h->last_path = plan.path; h->last_solver_path = plan.solver_path;
    auto handoff_of = [&](const ChunkPlan& cp) { return HandoffImage{cp.image ? image : nullptr, plan.image_m, cp.inner_image, cp.inner_image && plan.first_image}; };
    if (wave) { h->last_inner[0] = handoff_of(plan.full).inner_count(h->num_iter); h->last_inner[1] = handoff_of(plan.tail).inner_count(h->num_iter); }
    h->last_handoff = (plan.full.image && plan.tail.image) ? ADF_HANDOFF_IMAGE : plan.full.image ? ADF_HANDOFF_IMAGE_PAIR_TAIL : ADF_HANDOFF_PAIR_PLANE;

    for (int first = 0; first < n_pairs; first += plan.chunk) {
        const int n = (n_pairs - first < plan.chunk) ? n_pairs - first : plan.chunk;
        const ChunkPlan& cp = n == plan.chunk ? plan.full : plan.tail;
        const uint8_t* gv = pairs_on(vw.p, vw.pair_stride, first);
        void* o = (char*)om.p + (ptrdiff_t)first * om.pair_stride;
        float* confp = conf ? (float*)h->conf.p + (size_t)first * g.cframe : nullptr;
        const double F = (double)g.frame * n, P = (double)g.rw * g.rh * n;
        // what the chunk's kernels read of the maps (float maps of the view's size: q once the chunk is quantised)
        MapSource m = c.scaled ? lo.from(first) : caller_maps(c.dm).from(first);
        // the output outside the ROI (DF.cpp:284), and the confidence plane there where this call's own kernels make it
        OutsideArgs oa{o, om.stride, om.pair_stride, fill, om.f32 ? 1 : 0, c.scaled ? nullptr : confp, g};
        auto fill_outside = [&](hipStream_t s) {
            ProfScope ps(prof, K_FILL, fill_bytes(F - P, oa.conf != nullptr, ob_px), s);
            return launch_outside(oa, n, s);
        };
        // (guide_rows: no Chor -- the plane stays carved and untouched)
        WeightArgs wa{gv, vw.stride, vw.pair_stride, gch, h->lut.cur, cp.guide_rows ? nullptr : p.CH, p.CV, orient_h, orient_cv, g,
                      wave ? nullptr : p.B0};   // exact: B0 is free until the first pass writes its output there
        const GuideWeights gw = guide_weights(h, gv, vw, g);
        auto prologue = [&](bool weighted) {                               // FGS.cpp:203-205, or DF.cpp:286-290
            PlainPrologueArgs pa{m.rhs, m.s_rhs, m.ps_rhs, m.rhs_depth, 1, 0, p.A0, g, weighted ? orient_u2 : orient_h};
            if (weighted) { pa.conf = confp; pa.U1 = p.A1; }
            ProfScope ps(prof, K_PROLOGUE, prologue_bytes(P, weighted, db_px), st);
            return launch_plain_prologue(pa, n, st);
        };

        // fork
        hipStream_t wst = st;
        if (cp.fork_weights) {
            if ((rc = h->ensure_side(st))) return rc;
            HIP_TRY(hipEventRecord(h->ev_fork, st));
            HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
            wst = h->side;
        }
        // outside fill and weights (without confidence a down-scaled call resizes its maps between the two)
        if (cp.stage == CONF_NONE || cp.outside_on_side) HIP_TRY(fill_outside(wst));
        if (cp.stage == CONF_NONE && c.scaled && first == 0 && (rc = resize_disparity(prof, c, lo, sb.dhi, st))) return rc;
        if (cp.stage != CONF_MERGED) {
            ProfScope ps(prof, K_WEIGHTS, weights_bytes(P, gch, !cp.guide_rows), wst);
            HIP_TRY(launch_weights(wa, n, wst));                           // FGS.cpp:163-172
        }
        if (cp.fork_weights) HIP_TRY(hipEventRecord(h->ev_join, h->side));
        // quantise
        if (plan.quant_planes &&
            (rc = quantise_maps(prof, c.dm.from(first), W, H, n, qL, qR, nullptr, st, m))) return rc;
        // confidence stage, with the outside fill (DF.cpp:284, :187-190) where it did not go to the side stream
        switch (cp.stage) {
        case CONF_NONE:
            break;
        case CONF_SCALED:
        case CONF_SCALED_LO:
            if (!cp.outside_on_side) HIP_TRY(fill_outside(st));
            if (first == 0 && (rc = scaled_conf_maps(h, c, plan, sb, lo, rule, st))) return rc;
            break;
        case CONF_MERGED: {
            ProfScope ps(prof, K_LRC, merged_bytes(P, F - P, gch, ob_px), st);
            HIP_TRY(launch_prep_small(conf_band_args(m, confp, g, rule), wa, oa, n, st));   // FGS.cpp:163-172 + DF.cpp:197-210 + :284
            break;
        }
        case CONF_BAND:
        case CONF_LEFT:
        case CONF_TWO_KERNEL: {
            ConfOut out{confp, cL, cR};
            if (plan.rhs == RHS_CONF_KERNEL) { out.U0 = p.A0; out.U1 = p.A1; out.orient = orient_u2; }
            if (cp.stage == CONF_TWO_KERNEL) out.fill = &oa;
            if ((rc = conf_stage(prof, cp.stage, m, g, rule, out, n, st))) return rc;
            if (cp.stage != CONF_TWO_KERNEL && !cp.outside_on_side) HIP_TRY(fill_outside(st));
            break;
        }
        }
        // right-hand sides, where neither the first row pass nor the confidence kernel forms them
        if (plan.rhs == RHS_PLAIN || plan.rhs == RHS_CONF_PROLOGUE) HIP_TRY(prologue(plan.rhs == RHS_CONF_PROLOGUE));
        // join
        if (cp.fork_weights) HIP_TRY(hipStreamWaitEvent(st, h->ev_join, 0));
        // passes
        const FusedInputs fuse = plan.rhs == RHS_FUSED_LO
            ? lo_fuse(h, c, plan.lo_band, sb.clo + (size_t)first * c.dW * c.dH, m, sb.taps, g) : view_fuse(confp, m, g);
        const int epi = conf ? (om.f32 ? EPI_WLS_CONF_F32 : EPI_WLS_CONF) : (om.f32 ? EPI_F32 : EPI_I16);
        FinalOut fo{epi, o, om.stride, om.pair_stride, roi.x, roi.y, 1, 0};
        rc = run_passes(wave, g, p, conf ? 2 : 1, (float)h->lambda, (float)h->atten, h->num_iter, fo, n, st, prof,
                        plan.fused_first() ? &fuse : nullptr, cp.guide_rows ? &gw : nullptr, handoff_of(cp));
        if (rc) return rc;                                                 // DF.cpp:257-258, 292-296
    }
    return ADF_OK;
}

// Every device entry: check, plan, run.
static int wls_filter_device(adf_wls_t* h, int n_pairs, const DispMaps& dm, int dW, int dH, const View& view, const OutMap& om,
                             const adf_rect* roi, hipStream_t st)
{
    NEED_HANDLE(h);
    WlsCall c;
    int rc = check_call(h, n_pairs, dm, dW, dH, view, om, roi, c);
    if (rc) return rc;
    DeviceScope ds(h->device);
    h->lazy_conf.pending = false;    // (the previous call's low-resolution maps are about to be overwritten or freed)
    if ((rc = h->lut.ensure((float)h->sigma_color, st))) return rc;
    const WlsPlan plan = plan_wls(h, c);
    rc = wls_filter_impl(h, c, plan, st);
    if (rc == ADF_ENOMEM && plan.image_m) {
        // the image makes the workspace larger than the pair-plane hand-off's: a call that does not fit with it runs without
        const bool keep = h->handoff_image;
        h->handoff_image = false;
        rc = wls_filter_impl(h, c, plan_wls(h, c), st);
        h->handoff_image = keep;
    }
    if (c.scaled) h->roi = c.rlo;                                          // getROI(): valid_disp_ROI (DF.cpp:139)
    return rc;
}

// Every host entry: dense device copies of the images, the device call on them, the filtered map copied back.  Refused
// here is only what has to be before anything is read through the host pointers -- the float maps' rules, which the
// copies would satisfy whatever the caller passed, and what the copies' sizes and sources depend on; wls_filter_device
// refuses the rest.
static int wls_filter_host(adf_wls_t* h, int n_pairs, const DispMaps& dm, int dW, int dH, const View& view, const OutMap& om,
                           const adf_rect* roi)
{
    NEED_HANDLE(h);
    const int W = view.W, H = view.H, gch = view.ch;
    int rc = check_float_maps(dm, n_pairs, dW, dH, om, W, H);
    if (rc) return rc;
    if (!dm.L || !view.p || !om.p || W <= 0 || H <= 0 || dW <= 0 || dH <= 0 || n_pairs < 1)
        return fail(ADF_EBADARG, "adf_wls_filter_host: empty input");
    if (gch != 1 && gch != 3) return bad_view_channels();
    if (h->use_confidence && !dm.R) return no_right_map();
    DeviceScope ds(h->device);
    hipStream_t st = nullptr;
    // dense device copies: [dispL | dispR | out | view] per batch
    const size_t orow = (size_t)W * om.esz();
    const size_t drow = (size_t)dW * dm.esz();
    const size_t dbytes = drow * dH, obytes = orow * H, gbytes = (size_t)W * H * gch;
    const size_t dpad = pad_to(dbytes, 256), opad = pad_to(obytes, 256), gpad = pad_to(gbytes, 256);
    const size_t need = (size_t)n_pairs * (2 * dpad + opad + gpad);
    if ((rc = h->stage.reserve(need, st, FILL_ZERO))) return rc;
    char* dLd = (char*)h->stage.p;
    char* dRd = dLd + (size_t)n_pairs * dpad;
    char* od = dRd + (size_t)n_pairs * dpad;
    char* gd = od + (size_t)n_pairs * opad;
    if ((rc = copy_images(dLd, drow, dpad, dm.L, dm.sL, dm.psL, drow, dH, n_pairs, hipMemcpyHostToDevice, st))) return rc;
    if (dm.R && (rc = copy_images(dRd, drow, dpad, dm.R, dm.sR, dm.psR, drow, dH, n_pairs, hipMemcpyHostToDevice, st))) return rc;
    if ((rc = copy_images(gd, (size_t)W * gch, gpad, view.p, view.stride, view.pair_stride, (size_t)W * gch, H, n_pairs, hipMemcpyHostToDevice, st))) return rc;
    const DispMaps dd{dLd, (ptrdiff_t)drow, (ptrdiff_t)dpad, dm.R ? dRd : nullptr, (ptrdiff_t)drow, (ptrdiff_t)dpad, dm.f32};
    rc = wls_filter_device(h, n_pairs, dd, dW, dH, View{(const uint8_t*)gd, (ptrdiff_t)W * gch, (ptrdiff_t)gpad, gch, W, H},
                           OutMap{od, (ptrdiff_t)orow, (ptrdiff_t)opad, om.f32}, roi, st);
    if (rc) return rc;
    if ((rc = copy_images(om.p, om.stride, om.pair_stride, od, orow, opad, orow, H, n_pairs, hipMemcpyDeviceToHost, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return ADF_OK;
}

// The eight entry points: {same size, scaled} x {device, host} x {CV_16SC1, CV_32FC1 output}.
#define ADF_WLS_SAME_ARGS const int16_t* dispL, ptrdiff_t sL, ptrdiff_t psL, \
                          const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H
#define ADF_WLS_SCALED_ARGS const int16_t* dispL, ptrdiff_t sL, ptrdiff_t psL, int dW, int dH, \
                            const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H
#define ADF_WLS_RIGHT_ARGS const int16_t* dispR, ptrdiff_t sR, ptrdiff_t psR, const adf_rect* roi
// (an entry's images as wls_filter_device / wls_filter_host take them; a same-size entry's maps have the view's size)
#define ADF_WLS_IMAGES(DW, DH, F32IN, F32OUT) DispMaps{dispL, sL, psL, dispR, sR, psR, F32IN}, DW, DH, \
                                              View{view, sG, psG, gch, W, H}, OutMap{out, sO, psO, F32OUT}, roi
#define ADF_WLS_ENTRY_PAIR(NAME, MAP_ARGS, DW, DH, T, F32)                                                                     \
    extern "C" int NAME##_device(adf_wls_t* h, int n_pairs, MAP_ARGS, T* out, ptrdiff_t sO, ptrdiff_t psO, ADF_WLS_RIGHT_ARGS, \
                                 void* stream)                                                                                \
    {                                                                                                                         \
        return wls_filter_device(h, n_pairs, ADF_WLS_IMAGES(DW, DH, false, F32), (hipStream_t)stream);                        \
    }                                                                                                                         \
    extern "C" int NAME##_host(adf_wls_t* h, int n_pairs, MAP_ARGS, T* out, ptrdiff_t sO, ptrdiff_t psO, ADF_WLS_RIGHT_ARGS)   \
    {                                                                                                                         \
        return wls_filter_host(h, n_pairs, ADF_WLS_IMAGES(DW, DH, false, F32));                                               \
    }
ADF_WLS_ENTRY_PAIR(adf_wls_filter, ADF_WLS_SAME_ARGS, W, H, int16_t, false)
ADF_WLS_ENTRY_PAIR(adf_wls_filter_f32, ADF_WLS_SAME_ARGS, W, H, float, true)
ADF_WLS_ENTRY_PAIR(adf_wls_filter_scaled, ADF_WLS_SCALED_ARGS, dW, dH, int16_t, false)
ADF_WLS_ENTRY_PAIR(adf_wls_filter_scaled_f32, ADF_WLS_SCALED_ARGS, dW, dH, float, true)
#undef ADF_WLS_ENTRY_PAIR

// The typed pair: the scaled entries' arguments with the maps' and the filtered map's depth as arguments.
static int typed_depths(int disp_depth, int out_depth)
{
    if (disp_depth != ADF_16S && disp_depth != ADF_32F) return fail(ADF_EBADARG, "disparity maps must be ADF_16S or ADF_32F (got depth %d)", disp_depth);
    if (out_depth != ADF_16S && out_depth != ADF_32F) return fail(ADF_EBADARG, "filtered_disparity_map must be ADF_16S or ADF_32F (got depth %d)", out_depth);
    return ADF_OK;
}
extern "C" int adf_wls_filter_typed_device(adf_wls_t* h, int n_pairs, const void* dispL, ptrdiff_t sL, ptrdiff_t psL, int disp_depth,
                                           int dW, int dH, const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H,
                                           void* out, ptrdiff_t sO, ptrdiff_t psO, int out_depth,
                                           const void* dispR, ptrdiff_t sR, ptrdiff_t psR, const adf_rect* roi, void* stream)
{
    NEED_HANDLE(h);
    if (int rc = typed_depths(disp_depth, out_depth)) return rc;
    return wls_filter_device(h, n_pairs, ADF_WLS_IMAGES(dW, dH, disp_depth == ADF_32F, out_depth == ADF_32F), (hipStream_t)stream);
}
extern "C" int adf_wls_filter_typed_host(adf_wls_t* h, int n_pairs, const void* dispL, ptrdiff_t sL, ptrdiff_t psL, int disp_depth,
                                         int dW, int dH, const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H,
                                         void* out, ptrdiff_t sO, ptrdiff_t psO, int out_depth,
                                         const void* dispR, ptrdiff_t sR, ptrdiff_t psR, const adf_rect* roi)
{
    NEED_HANDLE(h);
    if (int rc = typed_depths(disp_depth, out_depth)) return rc;
    return wls_filter_host(h, n_pairs, ADF_WLS_IMAGES(dW, dH, disp_depth == ADF_32F, out_depth == ADF_32F));
}
#undef ADF_WLS_IMAGES
#undef ADF_WLS_SAME_ARGS
#undef ADF_WLS_SCALED_ARGS
#undef ADF_WLS_RIGHT_ARGS

extern "C" int adf_wls_profile_enable(adf_wls_t* h, int on)
{
    NEED_HANDLE(h);
    DeviceScope ds(h->device);
    h->prof.clear();
    h->prof.on = on != 0;
    return ADF_OK;
}

extern "C" int adf_wls_profile_read(adf_wls_t* h, adf_kernel_time* out, int capacity, int* count)
{
    NEED_HANDLE(h);
    if (!out || !count || capacity < 1) return fail(ADF_EBADARG, "adf_wls_profile_read: bad output buffer");
    DeviceScope ds(h->device);
    adf_kernel_time acc[K_COUNT];
    memset(acc, 0, sizeof(acc));
    for (int k = 0; k < K_COUNT; k++) snprintf(acc[k].name, sizeof(acc[k].name), "%s", kclass_names[k]);
    for (auto& r : h->prof.recs) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        acc[r.cls].launches++; acc[r.cls].total_ms += ms; acc[r.cls].alg_bytes += r.alg; acc[r.cls].moved_bytes += r.moved;
    }
    int n = 0;
    for (int k = 0; k < K_COUNT && n < capacity; k++)
        if (acc[k].launches) out[n++] = acc[k];
    *count = n;
    return ADF_OK;
}

static int conf_copy(adf_wls_t* h, int pair, float* dst, ptrdiff_t stride, hipMemcpyKind kind, hipStream_t st)
{
    if (!dst) return fail(ADF_EBADARG, "confidence destination is NULL");
    if (!h->use_confidence || !h->conf.p || h->last_pairs == 0)
        return fail(ADF_EBADARG, "no confidence map: filter() has not run with use_confidence");
    if (pair < 0 || pair >= h->last_pairs) return fail(ADF_EBADARG, "pair %d out of range [0,%d)", pair, h->last_pairs);
    if (stride < (ptrdiff_t)h->last_W * 4) return fail(ADF_ESIZE, "confidence stride smaller than a row");
    if (h->lazy_conf.pending) {
        // a down-scaled call whose first row pass interpolated the maps itself: resize the low-resolution confidence
        // maps of the call now (DF.cpp:274; all pairs, one launch, outside the filter call), once
        int rc = resize_conf_planes(h, h->lazy_conf.resize, st, nullptr);
        if (rc) return rc;
        h->lazy_conf.pending = false;
    }
    const float* src = (const float*)h->conf.p + (size_t)pair * h->last_cpitch * h->last_H + h->last_cx0;
    HIP_TRY(hipMemcpy2DAsync(dst, stride, src, (size_t)h->last_cpitch * 4, (size_t)h->last_W * 4, h->last_H, kind, st));
    return ADF_OK;
}

extern "C" int adf_wls_get_confidence_device(adf_wls_t* h, int pair, float* dst, ptrdiff_t stride, void* stream)
{
    NEED_HANDLE(h);
    DeviceScope ds(h->device);
    return conf_copy(h, pair, dst, stride, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

extern "C" int adf_wls_get_confidence_host(adf_wls_t* h, int pair, float* dst, ptrdiff_t stride)
{
    NEED_HANDLE(h);
    DeviceScope ds(h->device);
    int rc = conf_copy(h, pair, dst, stride, hipMemcpyDeviceToHost, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return ADF_OK;
}

// ----------------------------------------------------------------------------------------------
// FastGlobalSmootherFilter
// ----------------------------------------------------------------------------------------------
struct adf_fgs {
    int device = 0;
    int w = 0, h = 0;
    float lambda = 0, sigma = 0, atten = 0.25f; int num_iter = 3; int solver = ADF_SOLVER_EXACT;
    Geom g{};
    Lut lut;
    // one device block (BlockCache): the planes CH CV D F0 A0 B0, then the src / dst image staging
    void* block = nullptr; size_t block_bytes = 0;
    DevBuf planes, io;            // views into `block` (never released on their own)
    // Recorded behind the last thing the handle queued, on whatever stream that was.  Every call first makes its stream
    // wait for it: a filter call overwrites `io` (where a device-guide create staged the guide for its weight kernel,
    // and where the previous call's result may still be copied out on another stream).  At destruction the block goes
    // to the cache together with this event.
    hipEvent_t busy = nullptr;
    bool in_capture = false;      // a call was captured into a graph at some point: replays may be in flight that `busy` does not cover
};

// A call that is being CAPTURED into a graph neither waits for nor records the handle's event (an event recorded
// outside the capture has no place inside it, and one recorded inside is a graph node, not a marker on a stream);
// every other call does both -- also after a capture: the state is not latched (round 4).  `in_capture` only remembers
// that replays the library cannot see may exist, for adf_fgs_destroy.  include/adf_wls.h: a captured handle is used
// on ONE stream.
static int fgs_begin(adf_fgs* f, hipStream_t st)
{
    if (f->busy && !stream_is_capturing(st)) HIP_TRY(hipStreamWaitEvent(st, f->busy, 0));
    return ADF_OK;
}

static int fgs_end(adf_fgs* f, hipStream_t st)
{
    if (stream_is_capturing(st)) { f->in_capture = true; return ADF_OK; }
    if (f->busy) HIP_TRY(hipEventRecord(f->busy, st));
    return ADF_OK;
}

// guide_on_device: `guide` is a HIP device pointer (copied into the handle on `st`, no host round trip).
static int fgs_create_impl(adf_fgs_t** out, const uint8_t* guide, ptrdiff_t gstride, int gch, int w, int hgt,
                           double lambda, double sigma_color, double atten, int num_iter, int solver,
                           bool guide_on_device, hipStream_t st)
{
    if (!out) return fail(ADF_EBADARG, "adf_fgs_create: out is NULL");
    *out = nullptr;
    // FGS.cpp:143-144
    if (!guide || w <= 0 || hgt <= 0) return fail(ADF_EBADARG, "guide is empty");
    if (lambda < 0 || sigma_color < 0 || num_iter < 1) return fail(ADF_EBADARG, "lambda>=0, sigma_color>=0, num_iter>=1 required");
    if (gch != 1 && gch != 3) return fail(ADF_EBADARG, "guide must be CV_8UC1 or CV_8UC3");
    if (gstride < (ptrdiff_t)w * gch) return fail(ADF_ESIZE, "guide stride smaller than a row");
    if (solver != ADF_SOLVER_EXACT && solver != ADF_SOLVER_WAVE) return fail(ADF_EBADARG, "unknown solver %d", solver);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ADF_ENODEV, "adf_fgs_create: no HIP device visible");
    adf_fgs* f = new (std::nothrow) adf_fgs();
    if (!f) return fail(ADF_ENOMEM, "out of host memory");
    hipGetDevice(&f->device);
    f->w = w; f->h = hgt;
    f->lambda = (float)lambda; f->sigma = (float)sigma_color; f->atten = (float)atten; // FGS.cpp:145-147
    f->num_iter = num_iter;
    f->g = make_geom(w, hgt, 0, 0, w, hgt);
    f->solver = (solver == ADF_SOLVER_WAVE && wave_fits(f->g)) ? ADF_SOLVER_WAVE : ADF_SOLVER_EXACT;
    int rc = f->lut.ensure(f->sigma, st);
    if (rc) { adf_fgs_destroy(f); return rc; }
    const size_t gbytes = (size_t)w * hgt * gch;
    const size_t planes_bytes = (6 * f->g.plane * sizeof(float) + 255) / 256 * 256;
    const size_t io_bytes = ((gbytes > (size_t)w * hgt * 16 ? gbytes : (size_t)w * hgt * 16) + 255) / 256 * 256;
    hipError_t e = hipSuccess;
    f->block = cache_take(f->device, planes_bytes + io_bytes, st, &f->block_bytes);
    if (!f->block) {
        e = device_malloc(&f->block, planes_bytes + io_bytes);  // (clears the cache and retries when the driver refuses)
        if (e != hipSuccess) {
            f->block = nullptr; adf_fgs_destroy(f);
            return fail(e == hipErrorOutOfMemory ? ADF_ENOMEM : ADF_EHIP, "adf_fgs_create: %s", hipGetErrorString(e));
        }
        f->block_bytes = planes_bytes + io_bytes;
    }
    f->planes.p = f->block; f->planes.bytes = planes_bytes;
    f->io.p = (char*)f->block + planes_bytes; f->io.bytes = io_bytes;
    // deterministic padding lanes: the sweeps read (and discard) pitch padding
    e = hipMemsetAsync(f->block, 0, planes_bytes + io_bytes, st);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->busy, hipEventDisableTiming);
    if (e == hipSuccess) e = guide_on_device
        ? hipMemcpy2DAsync(f->io.p, (size_t)w * gch, guide, gstride, (size_t)w * gch, hgt, hipMemcpyDeviceToDevice, st)
        : hipMemcpy2D(f->io.p, (size_t)w * gch, guide, gstride, (size_t)w * gch, hgt, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        float* base = (float*)f->planes.p;
        WeightArgs wa{(const uint8_t*)f->io.p, (ptrdiff_t)w * gch, 0, gch, f->lut.cur,
                      base, base + f->g.plane, f->solver == ADF_SOLVER_WAVE ? ORIENT_N : ORIENT_T,
                      f->solver == ADF_SOLVER_WAVE ? ORIENT_STRIP : ORIENT_N, f->g,
                      f->solver == ADF_SOLVER_WAVE ? nullptr : base + 5 * f->g.plane};   // B0
        e = launch_weights(wa, 1, st);
    }
    // host guide: the weights are finished when create returns, like the reference's init (FGS.cpp:163-172);
    // device guide: they are queued on `st`; an event behind them orders every later filter call -- whatever stream it
    // is on -- after the kernel that still reads the staged guide
    if (e == hipSuccess && !guide_on_device) e = hipStreamSynchronize(st);
    // (a failed create may have queued work on `st` that the event was never recorded behind: drain it before the block
    // goes back to the cache)
    if (e != hipSuccess) { hipStreamSynchronize(st); adf_fgs_destroy(f); return fail(ADF_EHIP, "adf_fgs_create: %s", hipGetErrorString(e)); }
    if ((rc = fgs_end(f, st))) { hipStreamSynchronize(st); adf_fgs_destroy(f); return rc; }
    *out = f;
    return ADF_OK;
}

extern "C" int adf_fgs_create(adf_fgs_t** out, const uint8_t* guide, ptrdiff_t gstride, int gch, int w, int hgt,
                              double lambda, double sigma_color, double atten, int num_iter, int solver)
{
    return fgs_create_impl(out, guide, gstride, gch, w, hgt, lambda, sigma_color, atten, num_iter, solver, false, nullptr);
}

extern "C" int adf_fgs_create_device(adf_fgs_t** out, const uint8_t* guide, ptrdiff_t gstride, int gch, int w, int hgt,
                                     double lambda, double sigma_color, double atten, int num_iter, int solver, void* stream)
{
    return fgs_create_impl(out, guide, gstride, gch, w, hgt, lambda, sigma_color, atten, num_iter, solver, true,
                           (hipStream_t)stream);
}

extern "C" int adf_fgs_get_device(const adf_fgs_t* f, int* device) { NEED_HANDLE(f); if (device) *device = f->device; return ADF_OK; }
extern "C" int adf_fgs_get_solver(const adf_fgs_t* f, int* solver) { NEED_HANDLE(f); if (solver) *solver = f->solver; return ADF_OK; }

extern "C" void adf_fgs_destroy(adf_fgs_t* f)
{
    if (!f) return;
    DeviceScope ds(f->device);
    if (f->block) {
        if (f->busy && !f->in_capture) {
            cache_give_event(f->device, f->block, f->block_bytes, f->busy);    // (the event goes with the block)
            f->busy = nullptr;
        } else {
            hipDeviceSynchronize();
            hipFree(f->block);
        }
    }
    if (f->busy) hipEventDestroy(f->busy);
    f->lut.release();
    delete f;
}

// FastGlobalSmootherFilter::filter (FGS.cpp:200-221: channels one by one) from the device image `src` into the device
// image `dst` -- the same buffer (the host path's staging area; a caller filtering in place) or two that do not overlap.
static int fgs_filter_run(adf_fgs* f, int depth, int channels, const void* src, ptrdiff_t sstride, void* dst, ptrdiff_t dstride,
                          hipStream_t st)
{
    float* base = (float*)f->planes.p;
    const Geom& g = f->g;
    SolvePlanes p{};
    p.CH = base; p.CV = base + g.plane; p.D = base + 2 * g.plane; p.F0 = base + 3 * g.plane;
    p.A0 = base + 4 * g.plane; p.B0 = base + 5 * g.plane;
    const int epi = depth == ADF_8U ? EPI_U8 : depth == ADF_16S ? EPI_I16 : EPI_F32;
    const bool wave = f->solver == ADF_SOLVER_WAVE;
    for (int c = 0; c < channels;) {
        // The reference filters the channels one by one with the same weights (FGS.cpp:200-221); the wave
        // solver takes them two at a time as the two right-hand sides of one factorisation (its pair plane
        // spans A0 and B0, which are adjacent) -- the same arithmetic per channel, half the passes.
        const int nr = (wave && c + 1 < channels) ? 2 : 1;
        PlainPrologueArgs pa{src, sstride, 0, depth, channels, c, p.A0, g,
                             wave ? (nr == 2 ? ORIENT_PAIR : ORIENT_N) : ORIENT_T};
        pa.pair2 = nr == 2; pa.c2 = c + 1;
        HIP_TRY(launch_plain_prologue(pa, 1, st));
        // the epilogue of channel c overwrites only channel c of the image, which later
        // channels never read (they read their own channel), so filtering in place is safe
        FinalOut fo{epi, dst, dstride, 0, 0, 0, channels, c};
        int rc = run_passes(wave, g, p, nr, f->lambda, f->atten, f->num_iter, fo, 1, st);
        if (rc) return rc;
        c += nr;
    }
    return ADF_OK;
}

static int fgs_check_args(adf_fgs* f, const void* src, ptrdiff_t sstride, void* dst, ptrdiff_t dstride, int depth,
                          int channels, size_t* rowb)
{
    // FGS.cpp:184
    if (!src || !dst) return fail(ADF_EBADARG, "src/dst is empty");
    if (depth != ADF_8U && depth != ADF_16S && depth != ADF_32F) return fail(ADF_EBADARG, "src depth must be CV_8U, CV_16S or CV_32F");
    if (channels < 1 || channels > 4) return fail(ADF_EBADARG, "src must have 1..4 channels");
    const size_t esz = depth == ADF_8U ? 1 : depth == ADF_16S ? 2 : 4;
    *rowb = (size_t)f->w * channels * esz;
    if (sstride < (ptrdiff_t)*rowb || dstride < (ptrdiff_t)*rowb)
        return fail(ADF_ESIZE, "Size of the filtered image must be equal to the size of the guide image"); // FGS.cpp:187
    return ADF_OK;
}

extern "C" int adf_fgs_filter_host(adf_fgs_t* f, const void* src, ptrdiff_t sstride, void* dst, ptrdiff_t dstride,
                                   int depth, int channels)
{
    NEED_HANDLE(f);
    size_t rowb = 0;
    int rc = fgs_check_args(f, src, sstride, dst, dstride, depth, channels, &rowb);
    if (rc) return rc;
    DeviceScope ds(f->device);
    hipStream_t st = nullptr;
    if ((rc = fgs_begin(f, st))) return rc;
    HIP_TRY(hipMemcpy2DAsync(f->io.p, rowb, src, sstride, rowb, f->h, hipMemcpyHostToDevice, st));
    if ((rc = fgs_filter_run(f, depth, channels, f->io.p, (ptrdiff_t)rowb, f->io.p, (ptrdiff_t)rowb, st))) return rc;
    HIP_TRY(hipMemcpy2DAsync(dst, dstride, f->io.p, rowb, rowb, f->h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return fgs_end(f, st);
}

extern "C" int adf_fgs_filter_device(adf_fgs_t* f, const void* src, ptrdiff_t sstride, void* dst, ptrdiff_t dstride,
                                     int depth, int channels, void* stream)
{
    NEED_HANDLE(f);
    size_t rowb = 0;
    int rc = fgs_check_args(f, src, sstride, dst, dstride, depth, channels, &rowb);
    if (rc) return rc;
    DeviceScope ds(f->device);
    hipStream_t st = (hipStream_t)stream;
    // the images are filtered where they are (round 3: no staging copies): the first kernel of a channel reads `src`,
    // the last one writes `dst`; dst == src (same pointer and stride) filters in place, anything else must not overlap
    const char* s0 = (const char*)src; const char* d0 = (const char*)dst;
    const size_t sspan = (size_t)sstride * (f->h - 1) + rowb, dspan = (size_t)dstride * (f->h - 1) + rowb;
    if (!(src == dst && sstride == dstride) && s0 < d0 + dspan && d0 < s0 + sspan)
        return fail(ADF_EBADARG, "dst must be src itself (same stride) or must not overlap it");
    if ((rc = fgs_begin(f, st))) return rc;
    if ((rc = fgs_filter_run(f, depth, channels, src, sstride, dst, dstride, st))) return rc;
    return fgs_end(f, st);
}
