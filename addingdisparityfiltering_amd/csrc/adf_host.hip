// adf_host.hip -- the host toolkit of adf_host.h: no kernel lives here.
#include "adf_host.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <thread>

using namespace adf;

// ----------------------------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int adf::fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" int adf_version(void) { return ADF_VERSION; }
extern "C" const char* adf_last_error(void) { return g_err; }
extern "C" int adf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int adf_device_pci_bus_id(int device, char* buf, int len)
{
    if (!buf || len < 16) return fail(ADF_EBADARG, "adf_device_pci_bus_id: buffer of at least 16 bytes required");
    buf[0] = 0;
    HIP_TRY(hipDeviceGetPCIBusId(buf, len, device));
    return ADF_OK;
}

bool adf::stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

int adf::launched()
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? fail(ADF_EHIP, "%s", hipGetErrorString(e)) : ADF_OK;
}

bool adf::images_disjoint(int n, ptrdiff_t row_bytes, int rows, ptrdiff_t stride, ptrdiff_t image_stride, bool may_interleave)
{
    if (n < 2 || image_stride >= stride * (rows - 1) + row_bytes) return true;          // one image, or one after another
    return may_interleave && image_stride >= row_bytes && image_stride * (n - 1) + row_bytes <= stride;
}

int adf::border_check(const char* who, int border)
{
    if (border == 0 || border == 3)
        return fail(ADF_EBADARG, "%s: %s is not built; BORDER_REPLICATE, BORDER_REFLECT and BORDER_REFLECT_101 are", who, border == 0 ? "BORDER_CONSTANT" : "BORDER_WRAP");
    if (border != ADF_BORDER_REPLICATE && border != ADF_BORDER_REFLECT && border != ADF_BORDER_REFLECT_101)
        return fail(ADF_EBADARG, "%s: borderType %d is not built; BORDER_REPLICATE (1), BORDER_REFLECT (2) and BORDER_REFLECT_101 (4) are", who, border);
    return ADF_OK;
}

int adf::filter_geometry_check(const char* who, const FilterImages& im, const char* depths, const char* inputs)
{
    const FilterImage &g = im.guide, &s = im.src, &d = im.dst, &m = im.mask;
    const ptrdiff_t ss = (ptrdiff_t)depth_size(im.src_depth), ds = (ptrdiff_t)depth_size(im.dst_depth);
    if (!aligned(s.p, s.stride, s.map_stride, ss) || !aligned(d.p, d.stride, d.map_stride, ds))
        return fail(ADF_EBADARG, "%s: src and dst and their strides must be aligned to %s", who, depths);
    if ((int64_t)im.W * im.H >= ((int64_t)1 << 31)) return fail(ADF_ESIZE, "%s: W*H must be below 2^31", who);
    const ptrdiff_t srow = (ptrdiff_t)im.W * ss, drow = (ptrdiff_t)im.W * ds, grow = (ptrdiff_t)im.W * im.guide_channels, mrow = im.W;
    if (s.stride < srow || d.stride < drow || (g.p && g.stride < grow) || (m.p && m.stride < mrow))
        return fail(ADF_ESIZE, "%s: row stride smaller than a row", who);
    if (im.n > 1 && (s.map_stride < 0 || (g.p && g.map_stride < 0) || (m.p && m.map_stride < 0)))
        return fail(ADF_ESIZE, "%s: map strides must not be negative", who);
    if (!images_disjoint(im.n, drow, im.H, d.stride, d.map_stride, false))
        return fail(ADF_ESIZE, "%s: destination maps of the batch overlap (map stride smaller than a map)", who);
    const Span out = span_of(d.p, im.n, drow, im.H, d.stride, d.map_stride);
    if (overlap(out, span_of(s.p, im.n, srow, im.H, s.stride, s.map_stride)) ||
        (g.p && overlap(out, span_of(g.p, im.n, grow, im.H, g.stride, g.map_stride))) ||
        (m.p && overlap(out, span_of(m.p, im.n, mrow, im.H, m.stride, m.map_stride))))
        return fail(ADF_EBADARG, "%s: dst must not overlap %s", who, inputs);
    return ADF_OK;
}

int adf::DevBuf::reserve(size_t need, hipStream_t st, Fill fill)
{
    if (need <= bytes) return ADF_OK;
    if (p) { HIP_TRY(hipStreamSynchronize(st)); HIP_TRY(hipFree(p)); p = nullptr; bytes = 0; }
    need = pad_to(need, 256);
    HIP_TRY(device_malloc(&p, need));
    bytes = need;
    if (fill == FILL_ZERO) HIP_TRY(hipMemsetAsync(p, 0, need, st));
    return ADF_OK;
}

// Weight LUTs (FGS.cpp:150-154, 663-675), built on the host with libm, one immutable device table per sigma seen
// (up to LUT_CACHE of them per handle).  Round 3: a table is never rewritten, so coming back to a sigma used before --
// the common way callers vary it -- is a pointer switch with no device work and no synchronisation (capturable into a
// hipGraph), and a NEW sigma no longer drains the stream: its table goes into a fresh buffer no kernel in flight can be
// reading.  Only that first upload is a synchronous copy; a caller that captures filter calls must have used every
// sigma it switches between once before the capture (include/adf_wls.h).
//
// Tables are shared by every handle of the process on the same device (LutStore): the one-shot function
// fastGlobalSmootherFilter (EF.hpp:413) and the reference's own perf test (perf_fgs_filter.cpp:70-76) create a filter
// per call, and 3*256*256 libm calls cost ~1 ms on one core -- ten times the 720p filter call itself.  A table seen
// before is a look-up; a new one is built by a few threads (each entry is the same scalar libm expression as before:
// same bits).
//
// What every kind of immutable device table is: `count` elements of T at `dev` on `device`, found by `key`; hipFree of a
// dropped table waits for the device, so a kernel queued with it has finished reading.
template <class T, class KEY> struct ADF_LOCAL DeviceTable {
    using Elem = T;
    using Key = KEY;
    int device = 0; KEY key{}; size_t count = 0; T* dev = nullptr;
    DeviceTable() = default;
    DeviceTable(const DeviceTable&) = delete;
    DeviceTable& operator=(const DeviceTable&) = delete;
    ~DeviceTable() { if (dev) { DeviceScope ds(device); hipFree(dev); } }
};
struct adf::LutTable : DeviceTable<float, float> {};               // key: sigma

// The process-wide store of one kind of immutable device table (the filters' LutTable, the weighted median's WmfTable,
// the joint bilateral filter's JbfTable, the rolling guidance filter's RgfTable): up to CAP of them, least recently used
// dropped first.  THE way to a table is table_device: a look-up, else the one upload.
template <class TABLE> struct TableStore {
    static constexpr size_t CAP = 16;
    std::mutex m;
    std::vector<std::shared_ptr<TABLE>> tables;                  // most recently used last
    static TableStore& get() { static TableStore* s = new TableStore; return *s; }   // (never destroyed: no HIP calls at exit)
    template <class SAME> std::shared_ptr<TABLE> find(SAME&& same)
    {
        std::lock_guard<std::mutex> lk(m);
        for (size_t k = 0; k < tables.size(); k++)
            if (same(*tables[k])) {
                auto t = tables[k];
                tables.erase(tables.begin() + (ptrdiff_t)k); tables.push_back(t);
                return t;
            }
        return nullptr;
    }
    void add(const std::shared_ptr<TABLE>& t)
    {
        std::lock_guard<std::mutex> lk(m);
        // (a table dropped here lives on while a handle or a call still refers to it; with none left nothing can be reading it)
        if (tables.size() >= CAP) tables.erase(tables.begin());
        tables.push_back(t);
    }
    void clear() { std::lock_guard<std::mutex> lk(m); tables.clear(); }
};
using LutStore = TableStore<LutTable>;

// The table of `key` on the current device: a look-up when the key was seen before (no device work, capturable), else
// count(), a call made only then, gives its size, build(host) fills that many elements on the host, and one synchronous
// copy uploads them (`what` names the table where that fails).  The caller holds `out` until its launches are queued.
template <class TABLE, class COUNT, class BUILD>
static int table_device(const char* what, const typename TABLE::Key& key, COUNT&& count, BUILD&& build, std::shared_ptr<TABLE>& out)
{
    using Elem = typename TABLE::Elem;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return fail(ADF_ENODEV, "no HIP device");
    out = TableStore<TABLE>::get().find([&](const TABLE& q) { return q.device == device && q.key == key; });
    if (out) return ADF_OK;
    std::vector<Elem> host(count());
    build(host.data());
    Elem* d = nullptr;
    HIP_TRY(device_malloc(reinterpret_cast<void**>(&d), sizeof(Elem) * host.size()));
    hipError_t e = hipMemcpy(d, host.data(), sizeof(Elem) * host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d); return fail(ADF_EHIP, "%s table upload failed: %s", what, hipGetErrorString(e)); }
    out = std::make_shared<TABLE>();
    out->device = device; out->key = key; out->count = host.size(); out->dev = d;
    TableStore<TABLE>::get().add(out);
    return ADF_OK;
}

static void lut_build_host(float s, float* host)
{
    auto span = [&](int a, int b) { for (int i = a; i < b; i++) host[i] = -expf(-sqrtf((float)i) / s); };
    // Where the argument is at or below -110 the float exponential is +0 -- exp(-110) = 1.7e-48 lies 400 times below half
    // the smallest denormal, so every libm returns zero there, and the entry is -0.0f.  With the filter's usual sigma
    // (1..2) that is nine tenths of the table: those entries are stored, not computed.  The argument falls
    // monotonically with i (sqrtf and the division are monotone), so the first such index bounds the computed part.
    int n = ADF_LUT_LEVELS;
    if (s > 0.0f) {
        const double lim = 110.0 * (double)s;
        if (lim * lim * 1.001 + 2.0 < (double)ADF_LUT_LEVELS) {
            int i0 = (int)(lim * lim * 1.001) + 2;
            while (i0 < ADF_LUT_LEVELS && !(-sqrtf((float)i0) / s <= -110.0f)) i0++;   // (a check, not a search: the margin covers it)
            n = i0;
        }
    }
    for (int i = n; i < ADF_LUT_LEVELS; i++) host[i] = -0.0f;
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw >= 16 ? 8 : hw >= 4 ? hw / 2 : 1);
    if (n < 32768) nt = 1;                                        // a thread costs more to start than such a share to compute
    if (nt <= 1) { span(0, n); return; }
    std::vector<std::thread> th;
    const int per = (n + nt - 1) / nt;
    bool ok = true;
    int done = std::min(per, n);                                  // the caller's own share is [0, per)
    for (int t = 1; t < nt && ok; t++) {
        const int a = t * per, b = std::min(n, a + per);
        if (a >= b) break;
        try { th.emplace_back(span, a, b); done = b; } catch (...) { ok = false; }
    }
    span(0, std::min(per, n));
    for (auto& t : th) t.join();
    if (done < n) span(done, n);                                  // threads that could not be started
}

int adf::Lut::ensure(float s, hipStream_t st)
{
    for (auto& e : tables)
        if (e.t->key == s) { e.used = ++tick; cur = e.t->dev; return ADF_OK; }
    if ((int)tables.size() >= LUT_CACHE) {                 // drop the least recently used table: kernels of
        size_t lru = 0;                                    // earlier calls on `st` may still read it
        for (size_t k = 1; k < tables.size(); k++) if (tables[k].used < tables[lru].used) lru = k;
        HIP_TRY(hipStreamSynchronize(st));
        tables.erase(tables.begin() + (ptrdiff_t)lru);
    }
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    std::shared_ptr<LutTable> t = LutStore::get().find([&](const LutTable& q) { return q.device == device && q.key == s; });
    if (!t) {
        std::vector<float> host(ADF_LUT_LEVELS);
        lut_build_host(s, host.data());
        float* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(float) * ADF_LUT_LEVELS));
        hipError_t e = hipMemcpy(d, host.data(), sizeof(float) * ADF_LUT_LEVELS, hipMemcpyHostToDevice);
        if (e != hipSuccess) { hipFree(d); return fail(ADF_EHIP, "LUT upload failed: %s", hipGetErrorString(e)); }
        t = std::make_shared<LutTable>();
        t->device = device; t->key = s; t->count = ADF_LUT_LEVELS; t->dev = d;
        LutStore::get().add(t);
    }
    tables.push_back(Entry{t, ++tick});
    cur = t->dev;
    return ADF_OK;
}

// The weighted median filter's table (include/adf_wls.h: T), built on the host with libm like the table above and kept
// the same way: one immutable device table per (device, sigma, weight type), a look-up after its first use.
struct WmfKey {
    double sigma; int type;
    bool operator==(const WmfKey& o) const { return sigma == o.sigma && type == o.type; }
};
struct adf::WmfTable : DeviceTable<uint32_t, WmfKey> {};
using WmfStore = TableStore<WmfTable>;

static void wmf_build_host(double sigma, int weight_type, uint32_t* host)
{
    if (weight_type == ADF_WMF_OFF) { std::fill(host, host + ADF_WMF_TABLE_LEVELS, (uint32_t)ADF_WMF_WEIGHT_ONE); return; }
    // Below a quarter of the last place every later entry rounds to 0 (the argument only falls, and libm's error is far
    // below the factor of two that is left): those entries are stored, not computed.
    int i = 0;
    for (; i < ADF_WMF_TABLE_LEVELS; i++) {
        const double e = exp(-(double)i / (2.0 * sigma * sigma)) * 65536.0;
        if (e < 0.25) break;
        host[i] = (uint32_t)lrint(e);
    }
    std::fill(host + i, host + ADF_WMF_TABLE_LEVELS, 0u);
}

int adf::wmf_weights_check(const char* who, double sigma, int weight_type)
{
    if (weight_type != ADF_WMF_EXP && weight_type != ADF_WMF_OFF)
        return fail(ADF_EBADARG, "%s: weight_type must be ADF_WMF_EXP (0) or ADF_WMF_OFF (5); WMF_IV1, WMF_IV2, WMF_COS and WMF_JAC are not built", who);
    if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(ADF_EBADARG, "%s: sigma must be finite and > 0", who);
    return ADF_OK;
}

int adf::wmf_table_device(double sigma, int weight_type, std::shared_ptr<WmfTable>& out, const uint32_t** dev)
{
    if (weight_type == ADF_WMF_OFF) sigma = 1.0;                  // (one table whatever the sigma)
    if (int rc = table_device("weighted median", WmfKey{sigma, weight_type}, [] { return (size_t)ADF_WMF_TABLE_LEVELS; },
                              [&](uint32_t* host) { wmf_build_host(sigma, weight_type, host); }, out))
        return rc;
    *dev = out->dev;
    return ADF_OK;
}

extern "C" int adf_wmf_weight_table_host(double sigma, int weight_type, uint32_t* table, int levels)
{
    if (!table || levels != ADF_WMF_TABLE_LEVELS) return fail(ADF_EBADARG, "adf_wmf_weight_table_host: table must hold %d entries", ADF_WMF_TABLE_LEVELS);
    if (int rc = wmf_weights_check("adf_wmf_weight_table_host", sigma, weight_type)) return rc;
    wmf_build_host(sigma, weight_type, table);
    return ADF_OK;
}

// The joint bilateral filter's tables (include/adf_wls.h: C and S), built on the host with libm like the tables above and
// kept the same way: one block of floats, C then S, per (device, sigma_color, sigma_space, r, channels).
struct JbfKey {
    double sc, ss; int r, channels;
    bool operator==(const JbfKey& o) const { return sc == o.sc && ss == o.ss && r == o.r && channels == o.channels; }
};
struct adf::JbfTable : DeviceTable<float, JbfKey> {};
using JbfStore = TableStore<JbfTable>;

static void jbf_build_space(double ss, int r, float* space)       // S: the rolling guidance filter's too
{
    const double cs = -0.5 / (ss * ss);
    space[0] = 1.0f;
    for (int q = 1; q < (int)jbf_space_entries(r); q++) space[q] = (float)exp((double)q * cs);
}

static void jbf_build_host(double sc, double ss, int r, int channels, float* colour, float* space)
{
    const double cc = -0.5 / (sc * sc);
    colour[0] = 1.0f;
    for (int a = 1; a < (int)jbf_colour_entries(channels); a++) colour[a] = (float)exp((double)(a * a) * cc);
    jbf_build_space(ss, r, space);
}

int adf::jbf_params_check(const char* who, int d, double sigma_color, double sigma_space, int joint_channels,
                          double* sc, double* ss, int* r)
{
    if (joint_channels != 1 && joint_channels != 3) return fail(ADF_EBADARG, "%s: joint must have 1 or 3 channels", who);
    if (!std::isfinite(sigma_color) || !std::isfinite(sigma_space) || !std::isfinite((float)sigma_color) || !std::isfinite((float)sigma_space))
        return fail(ADF_EBADARG, "%s: sigmaColor and sigmaSpace must be finite (as float32 too)", who);
    *sc = sigma_color <= 0 ? 1.0 : sigma_color;
    *ss = sigma_space <= 0 ? 1.0 : sigma_space;
    const double rr = std::max(1.0, d <= 0 ? std::nearbyint(*ss * 1.5) : (double)(d / 2));   // (nearbyint: half to even, cvRound)
    if (!(rr <= (double)ADF_JBF_MAX_RADIUS))
        return fail(ADF_EBADARG, "%s: the radius (d / 2, or cvRound(1.5 sigmaSpace) for d <= 0) must not exceed %d", who, ADF_JBF_MAX_RADIUS);
    *r = (int)rr;
    return ADF_OK;
}

int adf::jbf_table_device(double sc, double ss, int r, int channels, std::shared_ptr<JbfTable>& out, const float** colour, const float** space)
{
    const size_t nc = jbf_colour_entries(channels);
    if (int rc = table_device("joint bilateral", JbfKey{sc, ss, r, channels}, [&] { return nc + jbf_space_entries(r); },
                              [&](float* host) { jbf_build_host(sc, ss, r, channels, host, host + nc); }, out))
        return rc;
    *colour = out->dev;
    *space = out->dev + nc;
    return ADF_OK;
}

extern "C" int adf_jbf_tables_host(int d, double sigma_color, double sigma_space, int joint_channels, float* colour, float* space, int* radius)
{
    double sc, ss;
    int r;
    if (int rc = jbf_params_check("adf_jbf_tables_host", d, sigma_color, sigma_space, joint_channels, &sc, &ss, &r)) return rc;
    if (radius) *radius = r;
    if (!colour && !space) return ADF_OK;                         // the radius alone: what sizes the space table
    if (!colour || !space) return fail(ADF_EBADARG, "adf_jbf_tables_host: colour and space must both be given (or neither: the radius alone)");
    jbf_build_host(sc, ss, r, joint_channels, colour, space);
    return ADF_OK;
}

// The rolling guidance filter's tables (include/adf_wls.h: "rolling guidance filter"), built and kept like the joint
// bilateral filter's: one block of floats, the range table then S, per (device, depth, sigma_color, sigma_space, r).
// The range table of an integer depth is C cut after its first zero entry (T entries, up to 65536: the square is formed
// in double); ADF_32F's is the constant grid G, and sigma_color reaches the kernel as `scale`.
struct RgfKey {
    int depth; double sc, ss; int r;
    bool operator==(const RgfKey& o) const { return depth == o.depth && sc == o.sc && ss == o.ss && r == o.r; }
};
struct adf::RgfTable : DeviceTable<float, RgfKey> {};
using RgfStore = TableStore<RgfTable>;

// C[L] for L = 0 .. the first entry that is 0.0f (or the depth's last level); `colour` may be null: the count alone.
static size_t rgf_build_colour(int depth, double sc, float* colour)
{
    if (depth == ADF_32F) {
        if (colour)
            for (size_t i = 0; i < RGF_GRID_ENTRIES; i++) colour[i] = (float)exp(-0.5 * ((double)i / 256.0) * ((double)i / 256.0));
        return RGF_GRID_ENTRIES;
    }
    const size_t levels = depth == ADF_8U ? 256 : 65536;
    const double cc = -0.5 / (sc * sc);
    if (colour) colour[0] = 1.0f;
    for (size_t L = 1; L < levels; L++) {
        const float c = (float)exp((double)L * (double)L * cc);
        if (colour) colour[L] = c;
        if (c == 0.0f) return L + 1;
    }
    return levels;
}

size_t adf::rgf_colour_entries(int depth, double sc) { return rgf_build_colour(depth, sc, nullptr); }

int adf::rgf_params_check(const char* who, int depth, int d, double sigma_color, double sigma_space,
                          double* sc, double* ss, int* r, float* scale)
{
    if (depth != ADF_8U && depth != ADF_16S && depth != ADF_32F)
        return fail(ADF_EBADARG, "%s: src must be CV_8U (ADF_8U), CV_16S (ADF_16S) or CV_32F (ADF_32F), one channel", who);
    if (int rc = jbf_params_check(who, d, sigma_color, sigma_space, 1, sc, ss, r)) return rc;
    *scale = depth == ADF_32F ? (float)(256.0 / *sc) : 1.0f;
    if (!std::isfinite(*scale))
        return fail(ADF_EBADARG, "%s: sigmaColor %g is too small for a float32 source: 256 / sigmaColor is not a finite float32", who, *sc);
    return ADF_OK;
}

int adf::rgf_table_device(int depth, double sc, double ss, int r, std::shared_ptr<RgfTable>& out,
                          const float** colour, const float** space, int* entries)
{
    if (depth == ADF_32F) sc = 1.0;                               // (G does not depend on it)
    const size_t ns = jbf_space_entries(r);
    if (int rc = table_device("rolling guidance", RgfKey{depth, sc, ss, r}, [&] { return rgf_colour_entries(depth, sc) + ns; },
                              [&](float* host) { jbf_build_space(ss, r, host + rgf_build_colour(depth, sc, host)); }, out))
        return rc;
    *entries = (int)(out->count - ns);                            // the range table, then S
    *colour = out->dev;
    *space = out->dev + *entries;
    return ADF_OK;
}

extern "C" int adf_rgf_tables_host(int depth, int d, double sigma_color, double sigma_space, float* colour, float* space,
                                   int* radius, int* colour_entries, float* scale)
{
    double sc, ss;
    int r;
    float k;
    if (int rc = rgf_params_check("adf_rgf_tables_host", depth, d, sigma_color, sigma_space, &sc, &ss, &r, &k)) return rc;
    if (radius) *radius = r;
    if (scale) *scale = k;
    if (colour_entries) *colour_entries = (int)rgf_colour_entries(depth, sc);
    if (!colour && !space) return ADF_OK;                         // the sizes alone
    if (!colour || !space) return fail(ADF_EBADARG, "adf_rgf_tables_host: colour and space must both be given (or neither: the sizes alone)");
    rgf_build_colour(depth, sc, colour);
    jbf_build_space(ss, r, space);
    return ADF_OK;
}

// Device blocks of short-lived handles (adf_fgs: the planes and the staged image of ONE image), kept for the next
// handle instead of going back to the driver: hipMalloc + hipFree of a 4K handle's 300 MB cost more than its filter
// call, and hipFree waits for the whole device.  A block comes back with the event behind its last user; whoever takes
// it makes its own stream wait for that event first, so nobody synchronises the host.
struct BlockCache {
    struct Ent { int device; void* p; size_t bytes; hipEvent_t ready; };
    static constexpr size_t CAP_BYTES = (size_t)3 << 30;
    static constexpr size_t CAP_ENTRIES = 8;
    std::mutex m;
    std::vector<Ent> ents;                                         // oldest first
    size_t total = 0;
    static BlockCache& get() { static BlockCache* c = new BlockCache; return *c; }
    static void drop(const Ent& e)
    {
        DeviceScope ds(e.device);
        if (e.ready) { hipEventSynchronize(e.ready); hipEventDestroy(e.ready); }
        hipFree(e.p);
    }
    // a cached block of at least `need` bytes (and not wastefully larger), ordered into `st`; null if there is none
    void* take(int device, size_t need, hipStream_t st, size_t* bytes)
    {
        Ent hit{};
        {
            std::lock_guard<std::mutex> lk(m);
            size_t best = ents.size();
            for (size_t k = 0; k < ents.size(); k++)
                if (ents[k].device == device && ents[k].bytes >= need && ents[k].bytes <= need + need / 4 + ((size_t)1 << 20) &&
                    (best == ents.size() || ents[k].bytes < ents[best].bytes))
                    best = k;
            if (best == ents.size()) return nullptr;
            hit = ents[best];
            ents.erase(ents.begin() + (ptrdiff_t)best);
            total -= hit.bytes;
        }
        if (hit.ready) {
            const hipError_t e = hipStreamWaitEvent(st, hit.ready, 0);
            if (e != hipSuccess) hipEventSynchronize(hit.ready);
            hipEventDestroy(hit.ready);
        }
        *bytes = hit.bytes;
        return hit.p;
    }
    void give(int device, void* p, size_t bytes, hipEvent_t ready)
    {
        std::vector<Ent> out;
        {
            std::lock_guard<std::mutex> lk(m);
            ents.push_back(Ent{device, p, bytes, ready});
            total += bytes;
            while (!ents.empty() && (total > CAP_BYTES || ents.size() > CAP_ENTRIES)) {
                out.push_back(ents.front());
                total -= ents.front().bytes;
                ents.erase(ents.begin());
            }
        }
        for (auto& e : out) drop(e);
    }
    void clear()
    {
        std::vector<Ent> out;
        { std::lock_guard<std::mutex> lk(m); out.swap(ents); total = 0; }
        for (auto& e : out) drop(e);
    }
};

extern "C" int adf_weight_table_host(float sigma_color, float* table, int levels)
{
    if (!table || levels != ADF_LUT_LEVELS) return fail(ADF_EBADARG, "table must hold %d floats", ADF_LUT_LEVELS);
    if (!(sigma_color >= 0.0f)) return fail(ADF_EBADARG, "sigma_color must be >= 0 (FGS.cpp:143)");
    lut_build_host(sigma_color, table);
    return ADF_OK;
}

namespace adf {
hipError_t device_malloc(void** p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        BlockCache::get().clear();                                   // the cache may be what fills the memory
        e = hipMalloc(p, bytes);
    }
    if (e != hipSuccess) *p = nullptr;
    return e;
}

void* cache_take(int device, size_t need, hipStream_t st, size_t* bytes) { return BlockCache::get().take(device, need, st, bytes); }

void cache_give(int device, void* p, size_t bytes, hipStream_t st)
{
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, st) != hipSuccess) {
        (void)hipGetLastError();                                     // no event: hand the block back idle
        if (ev) hipEventDestroy(ev);
        ev = nullptr;
        hipStreamSynchronize(st);
    }
    BlockCache::get().give(device, p, bytes, ev);
}

void cache_give_event(int device, void* p, size_t bytes, hipEvent_t ready) { BlockCache::get().give(device, p, bytes, ready); }

int Scratch::take(size_t need, hipStream_t stream)
{
    if (hipGetDevice(&device) != hipSuccess) return fail(ADF_ENODEV, "no HIP device");
    st = stream;
    if ((p = cache_take(device, need, st, &bytes))) return ADF_OK;
    HIP_TRY(device_malloc(&p, need));
    bytes = need;
    return ADF_OK;
}

int workspace_or_scratch(const char* who, const char* size_fn, void* workspace, size_t workspace_bytes, size_t need,
                         hipStream_t st, Scratch& blk, void** ws)
{
    *ws = workspace;
    if (workspace) {
        if (workspace_bytes < need) return fail(ADF_ESIZE, "%s: workspace smaller than %s", who, size_fn);
        return (uintptr_t)workspace & 3 ? fail(ADF_EBADARG, "%s: workspace must be 4-byte aligned", who) : ADF_OK;
    }
    // library scratch: a block of the process-wide cache, ordered behind its last user's event (no host wait)
    if (stream_is_capturing(st)) return fail(ADF_EBADARG, "%s: a call captured into a graph needs a caller workspace", who);
    const int rc = blk.take(need, st);
    *ws = blk.p;
    return rc;
}

int copy_images(void* dst, size_t dst_pitch, ptrdiff_t dst_image_stride, const void* src, size_t src_pitch,
                ptrdiff_t src_image_stride, size_t row_bytes, size_t rows, int n, hipMemcpyKind kind, hipStream_t st)
{
    for (int k = 0; k < n; k++)
        HIP_TRY(hipMemcpy2DAsync((char*)dst + k * dst_image_stride, dst_pitch, (const char*)src + k * src_image_stride, src_pitch,
                                 row_bytes, rows, kind, st));
    return ADF_OK;
}
} // namespace adf

extern "C" void adf_release_cached_memory(void)
{
    BlockCache::get().clear();
    LutStore::get().clear();
    WmfStore::get().clear();
    JbfStore::get().clear();
    RgfStore::get().clear();
}
