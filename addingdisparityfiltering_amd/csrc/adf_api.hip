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

// The passes on either solver.  exact: the planes ping-pong between A and B, the horizontal pass reads the row index
// fastest; wave: the on-chip partitioned solver, row-major planes solved in place.  `fuse` (wave only): the inputs the
// first row pass forms its right-hand sides from.
static int run_passes(bool wave, const Geom& g, const SolvePlanes& p, int n_rhs, float lambda, float atten, int num_iter,
                      const FinalOut& fo, int n_pairs, hipStream_t st, Profiler* prof = nullptr,
                      const FusedInputs* fuse = nullptr, const GuideWeights* gw = nullptr)
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

static size_t wls_pair_ws_bytes(const Geom& g, bool conf, bool wave, bool disc_maps, bool quant_planes)
{
    // exact: ROI planes CH CV D F0 A0 B0 (+ F1 A1 B1 with confidence); wave: CH CV A0 (+ A1), in place
    // full frames: cL cR, the depth-discontinuity maps (not needed when the one-sweep confidence kernel runs)
    size_t planes = wave ? (conf ? 4 : 3) : (conf ? 9 : 6);
    // float maps (adf_wls_filter_typed_*), confidence mode: the two int16 planes q -- never part of an int16 call's workspace
    return planes * g.plane * sizeof(float) + (conf && disc_maps ? 2 * g.frame * sizeof(float) : 0) +
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

// DF.cpp:262-264: the right map of a confidence-mode call on maps w wide
static int check_right_map(const void* dispR, ptrdiff_t sR, int w, size_t esz)
{
    if (!dispR) return fail(ADF_EBADARG, "disparity_map_right is required with use_confidence");
    if (sR < (ptrdiff_t)(w * esz)) return fail(ADF_ESIZE, "right disparity stride smaller than a row");
    return ADF_OK;
}

static int check_radius(const adf_wls* h)
{
    if (h->disc_radius < 0 || h->disc_radius > max_disc_radius())
        return fail(ADF_EBADARG, "depth discontinuity radius %d outside [0,%d]", h->disc_radius, max_disc_radius());
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

// Fused first row pass at view resolution: U1 = conf, U0 = conf*float(dL) read from the confidence planes and the left
// disparity maps of the pairs from `conf` / `dl` on (DF.cpp:288-290).
static FusedInputs view_fuse(const float* conf, const void* dl, ptrdiff_t sL, ptrdiff_t psL, bool f32, const Geom& g)
{
    FusedInputs f{};
    f.dl_f32 = f32 ? 1 : 0;
    f.conf_in = conf; f.conf_frame = g.cframe; f.conf_pitch = g.cpitch; f.conf_x0 = g.cx0 + g.rx; f.conf_y0 = g.ry;
    f.dl_in = dl; f.dl_stride = sL; f.dl_pair_stride = psL; f.dl_x0 = g.rx; f.dl_y0 = g.ry;
    return f;
}

// The down-scaled path's own work (DF.cpp:239-247, 268-277) for ALL pairs of a call.  adf_wls_filter_scaled_device
// decides and allocates it; wls_filter_impl queues it on the caller's stream where a same-size call runs its confidence
// kernels -- beside the weight kernel, which it has forked to the side stream by then and which needs the view only.
// Measured at 64 x 4K views / 1080p maps: everything after the fork 13.8-14.1 / 13.8-14.0 ms per call (radius 2 / 5; the
// band kernel crawls beside the weight kernel's small workgroups, 0.44 -> 0.9-1.7 ms, but the resizes then run alone),
// the low-resolution confidence map before the fork 14.20 / 14.51 (two memory-bound kernels side by side gain nothing),
// no overlap at all 14.49 / 14.69.
struct ScaledStage {
    const int16_t* dispL; ptrdiff_t sL, psL;   // the caller's low-resolution maps (float maps: their int16 planes q)
    const int16_t* dispR; ptrdiff_t sR, psR;
    const float* vL; ptrdiff_t svL, psvL;      // float maps: the left map's v plane -- resized in float, no rounding
    float resize_factor, x_ratio;              // DF.cpp:225, 241
    char* dhi; size_t dhi_bytes;               // the resized left maps (not with fuse_lo)
    float *cl, *cr;                            // low-resolution discontinuity maps
    ConfResize lo;                             // low-resolution confidence maps, both geometries, pair count
    bool fuse_lo;                              // the first row pass interpolates the low-resolution maps itself ...
    float* taps;                               // ... with this scratch for the columns' source coordinates
};

// Fused first row pass in its low-resolution form, for the pairs from `first` on (DF.cpp:272-274 then 288-290).
static FusedInputs lo_fuse(const adf_wls* h, const ScaledStage& s, int first, const Geom& g)
{
    const ConfResize& c = s.lo;
    const size_t lo = (size_t)c.dW * c.dH;
    FusedInputs f{};
    f.lo_conf = c.clo + (size_t)first * lo; f.lo_conf_stride = c.dW; f.lo_conf_pair = (ptrdiff_t)lo;
    f.lo_dl = (const int16_t*)((const char*)s.dispL + (ptrdiff_t)first * s.psL); f.lo_dl_stride = s.sL; f.lo_dl_pair = s.psL;
    f.lo_w = c.dW; f.lo_h = c.dH; f.hi_x0 = g.rx; f.hi_y0 = g.ry;
    f.lo_scale_x = (double)c.dW / c.ghi.W; f.lo_scale_y = (double)c.dH / c.ghi.H; f.lo_post_scale = s.x_ratio;
    if (c.band_map) {
        f.lo_zero_outside = 1; f.lo_vx0 = c.rlo.x; f.lo_vy0 = c.rlo.y; f.lo_vx1 = c.rlo.x + c.rlo.width; f.lo_vy1 = c.rlo.y + c.rlo.height;
    }
    f.lo_taps = s.taps; f.lo_half = h->scaled_half ? 1 : 0;
    return f;
}

// cv::resize of the low-resolution confidence maps into the handle's view-sized planes (DF.cpp:274)
static int resize_conf_planes(adf_wls_t* h, const ConfResize& c, hipStream_t st, Profiler* prof)
{
    const size_t lo = (size_t)c.dW * c.dH;
    const Geom& ghi = c.ghi;
    const double Fhi = (double)ghi.W * ghi.H * c.n_pairs;
    ResizeArgs rc32{c.clo, (ptrdiff_t)c.dW * 4, (ptrdiff_t)(lo * 4), c.dW, c.dH, (float*)h->conf.p + ghi.cx0, (ptrdiff_t)ghi.cpitch * 4,
                    (ptrdiff_t)(ghi.cframe * 4), ghi.W, ghi.H, (double)c.dW / ghi.W, (double)c.dH / ghi.H, 1.0f, 0};
    if (c.band_map) { rc32.zero_outside = 1; rc32.vx0 = c.rlo.x; rc32.vy0 = c.rlo.y; rc32.vx1 = c.rlo.x + c.rlo.width; rc32.vy1 = c.rlo.y + c.rlo.height; }
    ProfScope ps(prof, K_RESIZE, 4.0 * Fhi + 4.0 * (double)lo * c.n_pairs, 4.0 * Fhi + 4.0 * (double)lo * c.n_pairs, st);
    HIP_TRY(launch_resize_linear(rc32, c.n_pairs, st));
    return ADF_OK;
}

// The low-resolution confidence maps of all pairs (DF.cpp:197-210 at the maps' resolution, DF.cpp:318, 359).
static int scaled_conf_map(adf_wls_t* h, const ScaledStage& s, hipStream_t st, Profiler* prof)
{
    const ConfResize& c = s.lo;
    const Geom glo = plain_conf_layout(make_geom(c.dW, c.dH, c.rlo.x, c.rlo.y, c.rlo.width, c.rlo.height));
    const size_t lo = (size_t)c.dW * c.dH;
    const double Plo = (double)c.rlo.width * c.rlo.height * c.n_pairs;
    const int rrx = c.dW - (c.rlo.x + c.rlo.width);                       // DF.cpp:202
    const float roll_off = h->roll_off / (s.resize_factor * s.resize_factor);   // DF.cpp:359
    const int thresh_lo = (int)(s.resize_factor * h->lrc_thresh);       // DF.cpp:318
    if (c.band_map) {
        // the one-sweep kernel at the maps' resolution: ROI pixels from the band kernel, zeros outside (DF.cpp:187-190)
        ConfBandArgs ba{s.dispL, s.sL, s.psL, s.dispR, s.sR, s.psR, c.clo, glo, rrx, thresh_lo, h->disc_radius, roll_off, 0};
        ProfScope ps(prof, K_LRC, 8.0 * Plo, 8.0 * Plo, st);
        HIP_TRY(launch_conf_band(ba, c.n_pairs, st));                    // DF.cpp:197-210
        return ADF_OK;
    }
    DiscArgs da{{s.dispL, s.dispR}, {s.sL, s.sR}, {s.psL, s.psR}, {c.rlo.x, rrx}, c.rlo.y, c.rlo.width, c.rlo.height,
                h->disc_radius, roll_off, {s.cl, s.cr}, c.dW, lo, -1};
    {
        ProfScope ps(prof, K_DISC, 4.0 * Plo, 12.0 * Plo, st);
        HIP_TRY(launch_discontinuity(da, c.n_pairs, st));                // DF.cpp:204
    }
    LrcArgs la{s.dispL, s.sL, s.psL, s.dispR, s.sR, s.psR, s.cl, s.cr, c.clo, nullptr, 0, 0, 0, 0, nullptr, nullptr, glo, rrx, thresh_lo, ORIENT_N};
    ProfScope ps(prof, K_LRC, 4.0 * (double)lo * c.n_pairs, 4.0 * (double)lo * c.n_pairs + 12.0 * Plo, st);
    HIP_TRY(launch_lrc_prologue(la, c.n_pairs, st));                     // DF.cpp:208-209
    return ADF_OK;
}

// The resizes to the view: the confidence maps (DF.cpp:274) and the left disparity maps (DF.cpp:243-244, 272-273).
static int scaled_resize(adf_wls_t* h, const ScaledStage& s, hipStream_t st, Profiler* prof)
{
    const ConfResize& c = s.lo;
    int rc = h->use_confidence ? resize_conf_planes(h, c, st, prof) : ADF_OK;
    if (rc) return rc;
    const int W = c.ghi.W, H = c.ghi.H;
    const size_t lo = (size_t)c.dW * c.dH;
    const double Fhi = (double)W * H * c.n_pairs;
    // float maps: v through the float taps the confidence map goes through, times x_ratio once, nothing rounded
    const double eb = s.vL ? 4.0 : 2.0;
    ResizeArgs r16{s.dispL, s.sL, s.psL, c.dW, c.dH, s.dhi, (ptrdiff_t)W * 2, (ptrdiff_t)s.dhi_bytes, W, H, (double)c.dW / W, (double)c.dH / H, s.x_ratio, 1};
    ResizeArgs r32{s.vL, s.svL, s.psvL, c.dW, c.dH, s.dhi, (ptrdiff_t)W * 4, (ptrdiff_t)s.dhi_bytes, W, H, (double)c.dW / W, (double)c.dH / H, s.x_ratio, 0};
    ProfScope ps(prof, K_RESIZE, eb * Fhi + eb * (double)lo * c.n_pairs, eb * Fhi + eb * (double)lo * c.n_pairs, st);
    HIP_TRY(launch_resize_linear(s.vL ? r32 : r16, c.n_pairs, st));
    return ADF_OK;
}

// How a WLS filter call makes the two right-hand sides conf*disp and conf (DF.cpp:286-290), or float(disp) without
// confidence (DF.cpp:257).
enum ConfStage {
    CONF_NONE,        // no confidence: the plain prologue
    CONF_SCALED,      // down-scaled: low-resolution confidence map, both resizes, then the prologue or the fused first pass
    CONF_SCALED_LO,   // down-scaled: low-resolution confidence map; the first row pass interpolates it and the disparity map
    CONF_MERGED,      // weights + one-sweep confidence map + fill outside the ROI in one launch (small calls)
    CONF_BAND,        // both views' maps, LRC and x255 in one band sweep: the right view's map lives in LDS only
    CONF_LEFT,        // the right view's map, then the left one + LRC + x255 in one sweep (cL never hits memory)
    CONF_TWO_KERNEL,  // both views' maps, then LRC + x255 + the right-hand sides (and the fill outside the ROI)
};

// What one chunk of pairs queues.
struct ChunkPlan {
    ConfStage stage;
    bool fork_weights;     // the weight kernel runs on the side stream, beside the confidence kernels
    bool outside_on_side;  // ... behind the fill outside the ROI
    bool guide_rows;       // the row passes form their weights from the guide: the weight kernel writes Cvert only
};

// What a WLS filter call queues, decided before its chunk loop.
struct WlsPlan {
    bool wave;                // the wave solver (else the exact one)
    bool fused_first;         // the first row pass forms its right-hand sides itself (no prologue planes)
    bool band;                // the one-sweep confidence kernel: no full-frame discontinuity maps in the workspace
    size_t per_pair; int chunk;
    // chunks of `chunk` pairs, and a shorter last one: the merged launch is for small calls, so it depends on the
    // chunk's pair count
    ChunkPlan full, tail;
    int path;                 // ADF_PATH_* bits of the preparation stage
    int solver_path;          // ... of the solve passes
};

static ChunkPlan plan_chunk(const adf_wls* h, ConfStage stage, bool wave, bool guide_rows)
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
    return ChunkPlan{stage, fork, fork && wave && stage != CONF_TWO_KERNEL, guide_rows && stage != CONF_MERGED};
}

// The row passes' weights straight from the guide of the pairs from `guide` on (fgs_wave_h.hip, WS_GUIDE*).
static GuideWeights guide_weights(const adf_wls* h, const uint8_t* guide, ptrdiff_t sG, ptrdiff_t psG, int gch, const Geom& g)
{
    return GuideWeights{guide, sG, psG, gch, g.rx, g.ry, h->lut.cur};
}

static WlsPlan plan_wls(const adf_wls* h, const Geom& g, int n_pairs, const void* dispL, ptrdiff_t sL, ptrdiff_t psL, bool f32in,
                        const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, const ScaledStage* scaled)
{
    WlsPlan p{};
    const bool conf = h->use_confidence;
    // sizes outside the register-resident kernels' range fall back to the exact solver
    p.wave = h->solver == ADF_SOLVER_WAVE && wave_fits(g);
    ConfStage stage = !conf ? CONF_NONE
                    : scaled ? (scaled->fuse_lo ? CONF_SCALED_LO : CONF_SCALED)
                    : (p.wave && h->disc_radius <= conf_left_max_radius()) ? CONF_LEFT : CONF_TWO_KERNEL;
    // The view-resolution form of the fused first pass has alignment conditions that depend only on the geometry, the
    // strides and the pointers known here, not on the chunk.
    const float* planes = h->conf.p ? (const float*)h->conf.p : UNALLOCATED;
    p.fused_first = stage == CONF_SCALED_LO ||
                    (((stage == CONF_SCALED && !f32in) || stage == CONF_LEFT) && p.wave &&   // (a resized float map is not clamped again: prologue)
                     wave_hpass_can_fuse(first_pass_probe(view_fuse(planes, dispL, sL, psL, f32in, g), g.rw)));
    // the band kernel writes no right-hand sides: it needs the fused first pass
    p.band = stage == CONF_LEFT && p.fused_first && h->conf_band && conf_band_fits(g, h->disc_radius);
    if (p.band) stage = CONF_BAND;
    p.per_pair = wls_pair_ws_bytes(g, conf, p.wave, !p.band, f32in && conf && !scaled);
    p.chunk = (int)(h->ws_limit / p.per_pair);
    if (p.chunk < 1) p.chunk = 1;
    if (p.chunk > n_pairs) p.chunk = n_pairs;
    // The guide is new on every call, so the Chor plane of a full-resolution call on the wave solver is written once and
    // read num_iter times for nothing the guide row does not say in fewer bytes: the row passes take the guide instead
    // where their bucket has that form and the streaming weight kernel (the one with a Cvert-only form) runs.
    bool guide_rows = false;
    if (p.wave && !scaled && h->row_weights_guide) {
        WavePassArgs probe{};
        probe.len = g.rw; probe.gw = guide_weights(h, view, sG, psG, gch, g);
        WeightArgs wprobe{};
        wprobe.stride = sG; wprobe.ch = gch; wprobe.chor_orient = ORIENT_N; wprobe.g = g;
        guide_rows = wave_hpass_guide_fits(probe) && weights_stream_fits(wprobe);
    }
    auto chunk_of = [&](int n) {
        const bool merged = p.band && h->merge_small && prep_small_fits(g, h->disc_radius, gch, n) && prep_small_guide_fits(g, sG, gch);
        return plan_chunk(h, merged ? CONF_MERGED : stage, p.wave, guide_rows);
    };
    p.full = chunk_of(p.chunk);
    p.tail = chunk_of(n_pairs % p.chunk ? n_pairs % p.chunk : p.chunk);
    p.path = ((p.band || (scaled && scaled->lo.band_map)) ? ADF_PATH_CONF_BAND : 0) |
             (p.fused_first ? ADF_PATH_FUSED_FIRST_PASS : 0) |
             ((p.full.stage == CONF_MERGED || p.tail.stage == CONF_MERGED) ? ADF_PATH_MERGED_PREP : 0);
    p.solver_path = (p.full.guide_rows || p.tail.guide_rows) ? ADF_PATH_ROW_WEIGHTS_GUIDE : 0;
    if (stage == CONF_SCALED_LO)
        p.path |= ADF_PATH_SCALED_FUSED |
                  (wave_hpass_lo_half(first_pass_probe(lo_fuse(h, *scaled, 0, g), g.rw)) ? ADF_PATH_SCALED_HALF : 0);
    return p;
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
};

// scaled: the down-scaled path (DF.cpp:274): its stage replaces the confidence kernels, dm.R is not used, and dm.L is
// the stage's resized map (with fuse_lo only a stand-in that is never dereferenced; float: the resized v, taken as it is).
static int wls_filter_impl(adf_wls_t* h, int n_pairs, const DispMaps& dm,
                           const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H,
                           const OutMap& om, const adf_rect* roi_in, hipStream_t st, const ScaledStage* scaled = nullptr)
{
    NEED_HANDLE(h);
    const void* const dispL = dm.L; const void* const dispR = dm.R;
    const ptrdiff_t sL = dm.sL, psL = dm.psL, sR = dm.sR, psR = dm.psR;
    const bool f32in = dm.f32;
    // DF.cpp:221-222
    if (!dispL || W <= 0 || H <= 0) return fail(ADF_EBADARG, "disparity_map_left is empty");
    if (!view || (gch != 1 && gch != 3)) return fail(ADF_EBADARG, "left_view must be CV_8UC1 or CV_8UC3");
    void* const out = om.p;
    const ptrdiff_t sO = om.stride, psO = om.pair_stride;
    const double ob_px = (double)om.esz();                                 // output bytes per pixel
    if (!out) return fail(ADF_EBADARG, "filtered_disparity_map is NULL");
    if (n_pairs < 1) return fail(ADF_EBADARG, "n_pairs must be >= 1");
    if (sL < (ptrdiff_t)(W * dm.esz()) || sO < (ptrdiff_t)(W * om.esz()) || sG < (ptrdiff_t)W * gch)
        return fail(ADF_ESIZE, "row stride smaller than a row");
    if (om.f32 && ((reinterpret_cast<uintptr_t>(out) | (uintptr_t)sO | (uintptr_t)psO) & 3u))
        return fail(ADF_EBADARG, "a float filtered_disparity_map needs a 4-byte aligned base and strides");
    const bool conf = h->use_confidence;
    int rc;
    if (conf && !scaled && (rc = check_right_map(dispR, sR, W, dm.esz()))) return rc;
    if (h->lambda < 0 || h->sigma_color < 0) return fail(ADF_EBADARG, "lambda and sigma_color must be >= 0 (FGS.cpp:143)");
    adf_rect roi;
    if ((rc = resolve_roi(h, roi_in, W, H, roi))) return rc;
    if (conf && (rc = check_radius(h))) return rc;

    DeviceScope ds(h->device);
    const Geom g = make_geom(W, H, roi.x, roi.y, roi.width, roi.height);
    h->lazy_conf.pending = false;
    h->roi = roi; h->last_W = W; h->last_H = H; h->last_pairs = n_pairs;
    h->last_cpitch = g.cpitch; h->last_cx0 = g.cx0; h->last_path = 0; h->last_solver_path = 0;

    if ((rc = h->lut.ensure((float)h->sigma_color, st))) return rc;
    const WlsPlan plan = plan_wls(h, g, n_pairs, dispL, sL, psL, f32in, view, sG, psG, gch, scaled);
    // float maps: the confidence kernels read int16 planes q of the chunk's maps, made by one launch (design (a))
    const bool quant = f32in && conf && !scaled;
    const int qpitch = quant_pitch(W);
    const size_t qframe = (size_t)qpitch * H;                              // elements per plane
    // the right-hand sides' source depth: a resized float map (scaled) is taken as it is
    const int rhs_depth = !f32in ? ADF_16S : scaled ? ADF_32F : DEPTH_WLS_F32;
    const double db_px = (double)dm.esz();                                 // map bytes per pixel
    const bool wave = plan.wave;
    h->last_solver = wave ? ADF_SOLVER_WAVE : ADF_SOLVER_EXACT;
    if ((rc = h->ws.reserve(plan.per_pair * (size_t)plan.chunk, st, FILL_ZERO))) return rc;
    if (conf && !scaled && (rc = ensure_conf_planes(h, g, n_pairs, st))) return rc;
    {
        const long long sig[8] = {W, H, roi.x, roi.y, roi.width, roi.height, (long long)quant * 8 + (long long)plan.band * 4 + (long long)wave * 2 + conf, plan.chunk};
        if (memcmp(sig, h->ws_sig, sizeof(sig)) != 0) {
            HIP_TRY(hipMemsetAsync(h->ws.p, 0, h->ws.bytes, st));
            memcpy(h->ws_sig, sig, sizeof(sig));
        }
    }
    // carve the workspace
    float* base = (float*)h->ws.p;
    auto take = [&](size_t elems) { float* p = base; base += elems * (size_t)plan.chunk; return p; };
    SolvePlanes p{};
    p.CH = take(g.plane); p.CV = take(g.plane); p.A0 = take(g.plane);
    if (!wave) { p.D = take(g.plane); p.F0 = take(g.plane); p.B0 = take(g.plane); }
    float *cL = nullptr, *cR = nullptr;
    if (conf) {
        p.A1 = take(g.plane);                     // wave: directly behind A0 (the pair plane spans both)
        if (!wave) { p.F1 = take(g.plane); p.B1 = take(g.plane); }
    }
    // (before the full-frame maps: everything in front is a multiple of 256 bytes, so the planes' rows are 16-byte aligned)
    int16_t* const qL = quant ? (int16_t*)take(qframe) : nullptr;          // 2 * qframe int16 = qframe floats per pair
    int16_t* const qR = quant ? qL + qframe * (size_t)plan.chunk : nullptr;
    if (conf && !plan.band) { cL = take(g.frame); cR = take(g.frame); }
    // exact: the horizontal pass wants the row index fastest (T); wave: row-major (N), except that two
    // right-hand sides share one interleaved pair plane (A0 and A1 are adjacent: 2*plane floats per
    // image starting at A0) and Cvert is strip-major -- see fgs_wave_common.h
    const int orient_h = wave ? ORIENT_N : ORIENT_T;
    const int orient_u2 = wave ? ORIENT_PAIR : ORIENT_T;     // the two right-hand sides of a confidence-mode call
    const int orient_cv = wave ? ORIENT_STRIP : ORIENT_N;
    const int16_t fill = (int16_t)(16 * (h->min_disp - 1));            // DF.cpp:254,284
    const int rrx = W - (roi.x + roi.width);                           // DF.cpp:202
    const int thresh = (int)(1.0f * h->lrc_thresh);                    // DF.cpp:318 (resize_factor 1)
    Profiler* prof = &h->prof;
    h->last_path = plan.path; h->last_solver_path = plan.solver_path;

    for (int first = 0; first < n_pairs; first += plan.chunk) {
        const int n = (n_pairs - first < plan.chunk) ? n_pairs - first : plan.chunk;
        const ChunkPlan& cp = n == plan.chunk ? plan.full : plan.tail;
        // the caller's maps, and what the confidence kernels read: the same, or the chunk's planes q
        const void* mL = (const char*)dispL + (ptrdiff_t)first * psL;
        const void* mR = dispR ? (const char*)dispR + (ptrdiff_t)first * psR : nullptr;
        const int16_t* dL = quant ? qL : (const int16_t*)mL;
        const int16_t* dR = quant ? qR : (const int16_t*)mR;
        const ptrdiff_t sLq = quant ? (ptrdiff_t)qpitch * 2 : sL, psLq = quant ? (ptrdiff_t)qframe * 2 : psL;
        const ptrdiff_t sRq = quant ? (ptrdiff_t)qpitch * 2 : sR, psRq = quant ? (ptrdiff_t)qframe * 2 : psR;
        const uint8_t* gv = view + (ptrdiff_t)first * psG;
        void* o = (char*)out + (ptrdiff_t)first * psO;
        float* confp = conf ? (float*)h->conf.p + (size_t)first * g.cframe : nullptr;
        const double F = (double)g.frame * n, P = (double)g.rw * g.rh * n;
        // the output outside the ROI (DF.cpp:284), and the confidence plane there where this call's own kernels make it
        OutsideArgs oa{o, sO, psO, fill, om.f32 ? 1 : 0, scaled ? nullptr : confp, g};
        const double ob = ((oa.conf ? 4.0 : 0.0) + ob_px) * (F - P);
        auto fill_outside = [&](hipStream_t s) { ProfScope ps(prof, K_FILL, ob, ob, s); return launch_outside(oa, n, s); };
        // (guide_rows: no Chor -- the plane stays carved and untouched)
        WeightArgs wa{gv, sG, psG, gch, h->lut.cur, cp.guide_rows ? nullptr : p.CH, p.CV, orient_h, orient_cv, g,
                      wave ? nullptr : p.B0};   // exact: B0 is free until the first pass writes its output there
        const GuideWeights gw = guide_weights(h, gv, sG, psG, gch, g);
        ConfBandArgs ba{dL, sLq, psLq, dR, sRq, psRq, confp, g, rrx, thresh, h->disc_radius, h->roll_off, 0};
        DiscArgs da{{dL, dR}, {sLq, sRq}, {psLq, psRq}, {roi.x, rrx}, roi.y, roi.width, roi.height, h->disc_radius, h->roll_off,
                    {cL, cR}, W, g.frame, cp.stage == CONF_LEFT ? 1 : -1};
        const FusedInputs fuse = cp.stage == CONF_SCALED_LO ? lo_fuse(h, *scaled, first, g) : view_fuse(confp, mL, sL, psL, f32in, g);
        // the right-hand sides from the caller's maps and the confidence plane (DF.cpp:286-290): the down-scaled path's
        // prologue, and the float maps' wherever the first row pass is not fused
        auto conf_prologue = [&]() {
            PlainPrologueArgs pa{mL, sL, psL, rhs_depth, 1, 0, p.A0, g, orient_u2, confp, p.A1};
            ProfScope ps(prof, K_PROLOGUE, (12.0 + db_px) * P, (12.0 + db_px) * P, st);
            return launch_plain_prologue(pa, n, st);
        };

        hipStream_t wst = st;
        if (cp.fork_weights) {
            if ((rc = h->ensure_side(st))) return rc;
            HIP_TRY(hipEventRecord(h->ev_fork, st));
            HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
            wst = h->side;
        }
        if (cp.stage == CONF_NONE || cp.outside_on_side) HIP_TRY(fill_outside(wst));
        if (cp.stage == CONF_NONE && scaled && first == 0 && (rc = scaled_resize(h, *scaled, st, prof))) return rc;
        if (cp.stage != CONF_MERGED) {
            const double wb = (gch + (cp.guide_rows ? 4.0 : 8.0)) * P;
            ProfScope ps(prof, K_WEIGHTS, wb, wb, wst);
            HIP_TRY(launch_weights(wa, n, wst));                           // FGS.cpp:163-172
        }
        if (cp.fork_weights) HIP_TRY(hipEventRecord(h->ev_join, h->side));
        if (quant) {
            QuantArgs qa{{mL, mR}, {sL, sR}, {psL, psR}, {qL, qR}, nullptr, W, H, qpitch, qframe, n};
            ProfScope ps(prof, K_QUANT, 12.0 * F, 12.0 * F, st);         // 2 maps: 4 read + 2 written per pixel
            HIP_TRY(launch_quantise_maps(qa, st));
        }

        switch (cp.stage) {
        case CONF_NONE: {
            PlainPrologueArgs pa{mL, sL, psL, rhs_depth, 1, 0, p.A0, g, orient_h};
            ProfScope ps(prof, K_PROLOGUE, (4.0 + db_px) * P, (4.0 + db_px) * P, st);
            HIP_TRY(launch_plain_prologue(pa, n, st));                     // FGS.cpp:203-205
            break;
        }
        case CONF_SCALED: {   // confidence resized to the view (DF.cpp:274): only the prologue remains (DF.cpp:286-290)
            if (!cp.outside_on_side) HIP_TRY(fill_outside(st));
            if (first == 0 && ((rc = scaled_conf_map(h, *scaled, st, prof)) || (rc = scaled_resize(h, *scaled, st, prof)))) return rc;
            if (plan.fused_first) break;
            HIP_TRY(conf_prologue());
            break;
        }
        case CONF_SCALED_LO:  // the first row pass taps the low-resolution maps itself: no resize launch, no view-sized planes
            if (!cp.outside_on_side) HIP_TRY(fill_outside(st));
            if (first != 0) break;
            if ((rc = scaled_conf_map(h, *scaled, st, prof))) return rc;
            // a call captured into a graph is replayed without this host code: the view-sized confidence maps are made
            // inside the call (the graph), so getConfidenceMap() stays current after replays; otherwise on demand
            if (!stream_is_capturing(st)) h->lazy_conf = adf_wls::LazyConf{true, scaled->lo};
            else if ((rc = resize_conf_planes(h, scaled->lo, st, prof))) return rc;
            break;
        case CONF_MERGED: {
            const double b = (8.0 + gch + 8.0) * P + (4.0 + ob_px) * (F - P);
            ProfScope ps(prof, K_LRC, b, b, st);
            HIP_TRY(launch_prep_small(ba, wa, oa, n, st));                 // FGS.cpp:163-172 + DF.cpp:197-210 + :284
            break;
        }
        case CONF_BAND: {
            {
                ProfScope ps(prof, K_LRC, 8.0 * P, 8.0 * P, st);         // dL 2 + dR 2 read, conf 4 written
                HIP_TRY(launch_conf_band(ba, n, st));                      // DF.cpp:197-210
            }
            if (!cp.outside_on_side) HIP_TRY(fill_outside(st));            // DF.cpp:284, :187-190
            break;
        }
        case CONF_LEFT: {
            {
                ProfScope ps(prof, K_DISC, 2.0 * P, 6.0 * P, st);
                HIP_TRY(launch_discontinuity(da, n, st));                  // DF.cpp:204 (right view)
            }
            // (float maps: the kernel sees q, so it writes the confidence map only and the prologue forms conf * v)
            const bool fused = plan.fused_first || quant;
            ConfLeftArgs ca{dL, sLq, psLq, dR, sRq, psRq, cR, confp, fused ? nullptr : p.A0, fused ? nullptr : p.A1,
                            g, rrx, thresh, h->disc_radius, h->roll_off};
            {   // alg: conf (4P); moved: dL 2 + dR 2 + cR 4 reads, conf 4 (+8 when U0/U1 are materialised)
                const double wu = fused ? 0.0 : 8.0;
                ProfScope ps(prof, K_LRC, (4.0 + wu) * P, (12.0 + wu) * P, st);
                HIP_TRY(launch_conf_left(ca, n, st));                      // DF.cpp:204-209 (+288-290)
            }
            if (!cp.outside_on_side) HIP_TRY(fill_outside(st));            // DF.cpp:284, :187-190
            if (quant && !plan.fused_first) HIP_TRY(conf_prologue());
            break;
        }
        case CONF_TWO_KERNEL: {
            {   // reads the int16 ROIs, writes the float maps (the maps themselves are not algorithmic I/O)
                ProfScope ps(prof, K_DISC, 4.0 * P, 12.0 * P, st);
                HIP_TRY(launch_discontinuity(da, n, st));                  // DF.cpp:204
            }
            // float maps: the kernel reads its own pixel from the caller's left map (v, and q on the fly), the gather from qR
            LrcArgs la{quant ? (const int16_t*)mL : dL, quant ? sL : sLq, quant ? psL : psLq, dR, sRq, psRq, cL, cR, confp, o, sO, psO,
                       fill, om.f32 ? 1 : 0, p.A0, p.A1, g, rrx, thresh, orient_u2, quant ? 1 : 0};
            // alg: confidence map out (4F) + the two rhs planes (8P); moved adds dL,dR,cL,cR reads
            ProfScope ps(prof, K_LRC, 4.0 * F + 8.0 * P + ob_px * (F - P), 4.0 * F + (18.0 + db_px) * P + ob_px * (F - P), st);
            HIP_TRY(launch_lrc_prologue(la, n, st));                       // DF.cpp:208-209,288-290
            break;
        }
        }
        if (cp.fork_weights) HIP_TRY(hipStreamWaitEvent(st, h->ev_join, 0));
        const int epi = conf ? (om.f32 ? EPI_WLS_CONF_F32 : EPI_WLS_CONF) : (om.f32 ? EPI_F32 : EPI_I16);
        FinalOut fo{epi, o, sO, psO, roi.x, roi.y, 1, 0};
        rc = run_passes(wave, g, p, conf ? 2 : 1, (float)h->lambda, (float)h->atten, h->num_iter, fo, n, st, prof,
                        plan.fused_first ? &fuse : nullptr, cp.guide_rows ? &gw : nullptr);
        if (rc) return rc;                                                 // DF.cpp:257-258, 292-296
    }
    return ADF_OK;
}

// Down-scaled disparity path (DF.cpp:224-227, 239-247, 268-277): disparity maps of dW x dH, view and
// output of W x H.  ROI is in disparity-map coordinates, like the reference's.
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
    if (!om.p || dW <= 0 || dH <= 0 || W <= 0 || H <= 0 || n_pairs < 1) return ADF_OK;   // (refused by the call itself)
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

static int wls_filter_scaled_device(adf_wls_t* h, int n_pairs, const DispMaps& dm, int dW, int dH,
                                    const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H,
                                    const OutMap& om, const adf_rect* roi_in, hipStream_t st)
{
    NEED_HANDLE(h);
    int rc;
    if ((rc = check_float_maps(dm, n_pairs, dW, dH, om, W, H))) return rc;
    if (dW == W && dH == H)                                                // DF.cpp:224-227: same size, resize_factor 1
        return wls_filter_impl(h, n_pairs, dm, view, sG, psG, gch, W, H, om, roi_in, st);
    const void* const dispL = dm.L; const void* const dispR = dm.R;
    const ptrdiff_t sL = dm.sL, psL = dm.psL, sR = dm.sR, psR = dm.psR;
    const bool f32in = dm.f32;
    if (!dispL || dW <= 0 || dH <= 0 || W <= 0 || H <= 0) return fail(ADF_EBADARG, "disparity_map_left is empty");
    if (n_pairs < 1) return fail(ADF_EBADARG, "n_pairs must be >= 1");
    if (sL < (ptrdiff_t)(dW * dm.esz())) return fail(ADF_ESIZE, "row stride smaller than a row");
    const bool conf = h->use_confidence;
    if (conf && ((rc = check_right_map(dispR, sR, dW, dm.esz())) || (rc = check_radius(h)))) return rc;
    adf_rect rlo;                                                          // disparity-map coordinates
    if ((rc = resolve_roi(h, roi_in, dW, dH, rlo))) return rc;
    const float resize_factor = dW / (float)W;                             // DF.cpp:225
    const float x_ratio = W / (float)dW, y_ratio = H / (float)dH;          // DF.cpp:241-242,270-271
    adf_rect rhi{(int)(rlo.x * x_ratio), (int)(rlo.y * y_ratio), (int)(rlo.width * x_ratio), (int)(rlo.height * y_ratio)};
    if (rhi.width <= 0 || rhi.height <= 0 || rhi.x + rhi.width > W || rhi.y + rhi.height > H)
        return fail(ADF_ESIZE, "scaled ROI (%d,%d,%d,%d) does not fit the %dx%d view", rhi.x, rhi.y, rhi.width, rhi.height, W, H);

    DeviceScope ds(h->device);
    h->lazy_conf.pending = false;    // (the previous call's low-resolution maps are about to be overwritten or freed)
    const size_t lo = (size_t)dW * dH, hi = (size_t)W * H;
    const Geom ghi = make_geom(W, H, rhi.x, rhi.y, rhi.width, rhi.height);   // the geometry wls_filter_impl will derive
    // float maps: the low-resolution confidence kernels read the planes q, the resize reads the plane v (set below)
    const int qpitch = quant_pitch(dW);
    const size_t qframe = (size_t)qpitch * dH;
    ScaledStage s{(const int16_t*)dispL, sL, psL, (const int16_t*)dispR, sR, psR, nullptr, 0, 0, resize_factor, x_ratio, nullptr, 0,
                  nullptr, nullptr, ConfResize{UNALLOCATED, dW, dH, rlo, ghi, false, n_pairs}, false, nullptr};
    s.lo.band_map = conf && h->conf_band &&
                    conf_band_fits(plain_conf_layout(make_geom(dW, dH, rlo.x, rlo.y, rlo.width, rlo.height)), h->disc_radius);
    // Can the first row pass interpolate the maps itself (fgs_wave_h.hip, FUSE_LO)?  Confidence mode on the wave solver,
    // scale factors within the staging buffer's reach.  Then neither the resized disparity map nor -- until
    // getConfidenceMap() asks for it -- the resized confidence map is ever written.
    // (float maps take the resize kernels: the fused low-resolution prologue has no float form)
    s.fuse_lo = conf && !f32in && h->scaled_fuse && h->solver == ADF_SOLVER_WAVE && wave_fits(ghi) &&
                wave_hpass_can_fuse_lo(first_pass_probe(lo_fuse(h, s, 0, ghi), ghi.rw));
    // scratch: resized disparity (int16, view size; not with fuse_lo) + low-resolution cL, cR, conf (float)
    s.dhi_bytes = s.fuse_lo ? 0 : pad_to(hi * dm.esz(), 256);
    const size_t maps_bytes = pad_to((size_t)n_pairs * (s.dhi_bytes + (conf ? 3 * lo * sizeof(float) : 0)), 256);
    const size_t taps_bytes = pad_to(s.fuse_lo ? 2 * ((size_t)rhi.width + 4) * sizeof(float) : 0, 256);   // + the columns' taps
    // + float maps: v (float) and, in confidence mode, the two planes q (int16), per pair
    const size_t quant_bytes = f32in ? (size_t)n_pairs * qframe * (4 + (conf ? 4 : 0)) : 0;
    const size_t need = maps_bytes + taps_bytes + quant_bytes;
    if ((rc = h->scaled.reserve(need, st, FILL_ZERO))) return rc;
    s.dhi = (char*)h->scaled.p;
    s.cl = (float*)(s.dhi + (size_t)n_pairs * s.dhi_bytes);
    s.cr = s.cl + (size_t)n_pairs * lo;
    s.lo.clo = s.cr + (size_t)n_pairs * lo;
    s.taps = s.fuse_lo ? (float*)((char*)h->scaled.p + maps_bytes) : nullptr;
    if (conf && (rc = ensure_conf_planes(h, ghi, n_pairs, st))) return rc;
    if (f32in) {
        float* v = (float*)((char*)h->scaled.p + maps_bytes + taps_bytes);
        int16_t* qL = conf ? (int16_t*)(v + (size_t)n_pairs * qframe) : nullptr;
        int16_t* qR = conf ? qL + (size_t)n_pairs * qframe : nullptr;
        QuantArgs qa{{dispL, conf ? dispR : nullptr}, {sL, sR}, {psL, psR}, {qL, qR}, v, dW, dH, qpitch, qframe, n_pairs};
        const double lo_px = (double)lo * n_pairs;
        ProfScope ps(&h->prof, K_QUANT, (conf ? 16.0 : 8.0) * lo_px, (conf ? 16.0 : 8.0) * lo_px, st);
        HIP_TRY(launch_quantise_maps(qa, st));
        s.dispL = qL; s.dispR = qR; s.sL = s.sR = (ptrdiff_t)qpitch * 2; s.psL = s.psR = (ptrdiff_t)qframe * 2;
        s.vL = v; s.svL = (ptrdiff_t)qpitch * 4; s.psvL = (ptrdiff_t)qframe * 4;
    }
    // (fuse_lo: wls_filter_impl never dereferences its dispL -- the caller's low-resolution map stands in, with its own strides)
    const DispMaps dhi{s.fuse_lo ? dispL : (const void*)s.dhi, (ptrdiff_t)(W * dm.esz()), (ptrdiff_t)s.dhi_bytes, nullptr, 0, 0, f32in};
    rc = wls_filter_impl(h, n_pairs, dhi, view, sG, psG, gch, W, H, om, &rhi, st, &s);
    h->roi = rlo;                                                          // getROI(): valid_disp_ROI (DF.cpp:139)
    return rc;
}

static int wls_filter_scaled_host(adf_wls_t* h, int n_pairs, const DispMaps& dm, int dW, int dH,
                                  const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H,
                                  const OutMap& om, const adf_rect* roi)
{
    NEED_HANDLE(h);
    const void* const dispL = dm.L; const void* const dispR = dm.R;
    const ptrdiff_t sL = dm.sL, psL = dm.psL, sR = dm.sR, psR = dm.psR;
    int rc = check_float_maps(dm, n_pairs, dW, dH, om, W, H);
    if (rc) return rc;
    if (!dispL || !view || !om.p || W <= 0 || H <= 0 || dW <= 0 || dH <= 0 || n_pairs < 1)
        return fail(ADF_EBADARG, "adf_wls_filter_host: empty input");
    if (gch != 1 && gch != 3) return fail(ADF_EBADARG, "left_view must be CV_8UC1 or CV_8UC3");
    if (h->use_confidence && !dispR) return fail(ADF_EBADARG, "disparity_map_right is required with use_confidence");
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
    if ((rc = copy_images(dLd, drow, dpad, dispL, sL, psL, drow, dH, n_pairs, hipMemcpyHostToDevice, st))) return rc;
    if (dispR && (rc = copy_images(dRd, drow, dpad, dispR, sR, psR, drow, dH, n_pairs, hipMemcpyHostToDevice, st))) return rc;
    if ((rc = copy_images(gd, (size_t)W * gch, gpad, view, sG, psG, (size_t)W * gch, H, n_pairs, hipMemcpyHostToDevice, st))) return rc;
    const DispMaps dd{dLd, (ptrdiff_t)drow, (ptrdiff_t)dpad, dispR ? dRd : nullptr, (ptrdiff_t)drow, (ptrdiff_t)dpad, dm.f32};
    rc = wls_filter_scaled_device(h, n_pairs, dd, dW, dH, (const uint8_t*)gd, (ptrdiff_t)W * gch, (ptrdiff_t)gpad, gch, W, H,
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
#define ADF_WLS_ENTRIES(SUFFIX, T, F32)                                                                                       \
    extern "C" int adf_wls_filter##SUFFIX##_device(adf_wls_t* h, int n_pairs, ADF_WLS_SAME_ARGS, T* out, ptrdiff_t sO,        \
                                                   ptrdiff_t psO, ADF_WLS_RIGHT_ARGS, void* stream)                           \
    {                                                                                                                         \
        return wls_filter_impl(h, n_pairs, DispMaps{dispL, sL, psL, dispR, sR, psR, false}, view, sG, psG, gch, W, H,         \
                               OutMap{out, sO, psO, F32}, roi, (hipStream_t)stream);                                          \
    }                                                                                                                         \
    extern "C" int adf_wls_filter_scaled##SUFFIX##_device(adf_wls_t* h, int n_pairs, ADF_WLS_SCALED_ARGS, T* out,             \
                                                          ptrdiff_t sO, ptrdiff_t psO, ADF_WLS_RIGHT_ARGS, void* stream)      \
    {                                                                                                                         \
        return wls_filter_scaled_device(h, n_pairs, DispMaps{dispL, sL, psL, dispR, sR, psR, false}, dW, dH, view, sG, psG,   \
                                        gch, W, H, OutMap{out, sO, psO, F32}, roi, (hipStream_t)stream);                      \
    }                                                                                                                         \
    extern "C" int adf_wls_filter_scaled##SUFFIX##_host(adf_wls_t* h, int n_pairs, ADF_WLS_SCALED_ARGS, T* out, ptrdiff_t sO, \
                                                        ptrdiff_t psO, ADF_WLS_RIGHT_ARGS)                                    \
    {                                                                                                                         \
        return wls_filter_scaled_host(h, n_pairs, DispMaps{dispL, sL, psL, dispR, sR, psR, false}, dW, dH, view, sG, psG,     \
                                      gch, W, H, OutMap{out, sO, psO, F32}, roi);                                             \
    }                                                                                                                         \
    extern "C" int adf_wls_filter##SUFFIX##_host(adf_wls_t* h, int n_pairs, ADF_WLS_SAME_ARGS, T* out, ptrdiff_t sO,          \
                                                 ptrdiff_t psO, ADF_WLS_RIGHT_ARGS)                                           \
    {                                                                                                                         \
        return wls_filter_scaled_host(h, n_pairs, DispMaps{dispL, sL, psL, dispR, sR, psR, false}, W, H, view, sG, psG, gch,  \
                                      W, H, OutMap{out, sO, psO, F32}, roi);                                                  \
    }
ADF_WLS_ENTRIES(, int16_t, false)
ADF_WLS_ENTRIES(_f32, float, true)
#undef ADF_WLS_ENTRIES

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
    return wls_filter_scaled_device(h, n_pairs, DispMaps{dispL, sL, psL, dispR, sR, psR, disp_depth == ADF_32F}, dW, dH, view, sG, psG,
                                    gch, W, H, OutMap{out, sO, psO, out_depth == ADF_32F}, roi, (hipStream_t)stream);
}
extern "C" int adf_wls_filter_typed_host(adf_wls_t* h, int n_pairs, const void* dispL, ptrdiff_t sL, ptrdiff_t psL, int disp_depth,
                                         int dW, int dH, const uint8_t* view, ptrdiff_t sG, ptrdiff_t psG, int gch, int W, int H,
                                         void* out, ptrdiff_t sO, ptrdiff_t psO, int out_depth,
                                         const void* dispR, ptrdiff_t sR, ptrdiff_t psR, const adf_rect* roi)
{
    NEED_HANDLE(h);
    if (int rc = typed_depths(disp_depth, out_depth)) return rc;
    return wls_filter_scaled_host(h, n_pairs, DispMaps{dispL, sL, psL, dispR, sR, psR, disp_depth == ADF_32F}, dW, dH, view, sG, psG,
                                  gch, W, H, OutMap{out, sO, psO, out_depth == ADF_32F}, roi);
}
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
