// adf::dtFilter / adf::createDTFilter (include/adf_ximgproc.hpp) on host Mats, compared bit for bit with the C-ABI call
// adf_dt_filter_host and with a small sequential restatement of the recurrence in include/adf_wls.h fed with
// adf_dt_rf_table_host (built and run by tests/test_cpp_dt.py, with -ffp-contract=off: the statement's expressions are
// evaluated operation by operation).
#include "adf_ximgproc.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool equal(const Mat& a, const Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols || a.depth_ != b.depth_) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<unsigned char>(y), b.ptr<unsigned char>(y), (size_t)a.cols * Mat::esz(a.depth_)) != 0) return false;
    return true;
}

static int code(int depth) { return depth == D8U ? ADF_8U : depth == D16S ? ADF_16S : ADF_32F; }

// The recurrence on an int16 map, float result: rows there and back, then columns, per iteration.
static void dt_ref(const Mat& guide, const Mat& src, std::vector<float>& x, double ss, double sr, int N)
{
    const int H = src.rows, W = src.cols, ch = guide.cn, levels = 255 * ch + 1;
    std::vector<float> table((size_t)N * levels);
    EXPECT(adf_dt_rf_table_host(ss, sr, N, ch, table.data()) == ADF_OK);
    auto L = [&](int y0, int x0, int y1, int x1) {
        int s = 0;
        for (int c = 0; c < ch; c++) s += std::abs((int)guide.ptr<uint8_t>(y0)[x0 * ch + c] - (int)guide.ptr<uint8_t>(y1)[x1 * ch + c]);
        return s;
    };
    x.resize((size_t)H * W);
    for (int y = 0; y < H; y++)
        for (int j = 0; j < W; j++) x[(size_t)y * W + j] = (float)src.ptr<int16_t>(y)[j];
    auto step = [&](float& cur, float from, float a) { const float d = from - cur; const float p = a * d; cur = cur + p; };
    for (int i = 0; i < N; i++) {
        const float* A = table.data() + (size_t)i * levels;
        for (int y = 0; y < H; y++) {
            float* r = &x[(size_t)y * W];
            for (int j = 1; j < W; j++) step(r[j], r[j - 1], A[L(y, j - 1, y, j)]);
            for (int j = W - 2; j >= 0; j--) step(r[j], r[j + 1], A[L(y, j, y, j + 1)]);
        }
        for (int c = 0; c < W; c++) {
            for (int y = 1; y < H; y++) step(x[(size_t)y * W + c], x[(size_t)(y - 1) * W + c], A[L(y - 1, c, y, c)]);
            for (int y = H - 2; y >= 0; y--) step(x[(size_t)y * W + c], x[(size_t)(y + 1) * W + c], A[L(y, c, y + 1, c)]);
        }
    }
}

static void fill(Mat& guide, Mat& src, unsigned seed)
{
    std::mt19937 rng(seed);
    static const int16_t lv[] = {-16, 32, 480, 2000, -32768, 32767};
    for (int y = 0; y < src.rows; y++)
        for (int x = 0; x < src.cols; x++) {
            src.ptr<int16_t>(y)[x] = rng() % 4 ? lv[rng() % 6] : (int16_t)((int)(rng() % 65536) - 32768);
            for (int c = 0; c < guide.cn; c++)
                guide.ptr<uint8_t>(y)[x * guide.cn + c] = (uint8_t)std::min(255u, (unsigned)((x / 6) * 40 + (y / 4) * 25 + rng() % 9));
        }
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int shapes[][3] = {{65, 130, 1}, {129, 63, 3}};                // H, W, guide channels
    unsigned seed = 1;
    for (auto& s : shapes) {
        const int H = s[0], W = s[1], ch = s[2];
        Mat guide(H, W, D8U, ch), src(H, W, D16S, 1);
        fill(guide, src, seed++);
        const double ss = 12.0, sr = 25.0;
        const int N = 3;
        const int ddepths[] = {-1, D8U, D16S, D32F};
        for (int dDepth : ddepths) {
            const int ddepth = dDepth == -1 ? D16S : dDepth;
            Mat abi(H, W, ddepth, 1), obj;
            EXPECT(adf_dt_filter_host(1, guide.data, (ptrdiff_t)guide.step, 0, ch, src.data, (ptrdiff_t)src.step, 0, ADF_16S,
                                      abi.data, (ptrdiff_t)abi.step, 0, code(ddepth), W, H, ss, sr, ADF_DTF_RF, N) == ADF_OK);
            createDTFilter(guide, ss, sr, DTF_RF, N)->filter(src, obj, dDepth);
            EXPECT(equal(obj, abi));
            if (dDepth == -1) {                                          // dtFilter has no dDepth: src's depth
                Mat got;
                dtFilter(guide, src, got, ss, sr, DTF_RF, N);
                EXPECT(equal(got, abi));
                EXPECT(!equal(got, src));                                // the case is not vacuous
            }
            if (ddepth == D32F) {                                        // ... and the C-ABI call is the statement
                std::vector<float> x;
                dt_ref(guide, src, x, ss, sr, N);
                bool same = true;
                for (int y = 0; y < H; y++) same = same && std::memcmp(abi.ptr<float>(y), &x[(size_t)y * W], (size_t)W * 4) == 0;
                EXPECT(same);
            }
        }
    }
    {   // the defaults are DTF_RF and 3 iterations, the result may land in src, and the object keeps its own guide
        Mat guide(12, 70, D8U, 3), src(12, 70, D16S, 1), a, b, c;
        fill(guide, src, 5);
        dtFilter(guide, src, a, 10.0, 30.0);
        dtFilter(guide, src, b, 10.0, 30.0, DTF_RF, 3);
        EXPECT(a.depth_ == D16S && equal(a, b));
        Ptr<DTFilter> f = createDTFilter(guide, 10.0, 30.0);
        std::memset(guide.data, 0, guide.step * guide.rows);             // the caller's guide changes; the object's does not
        f->filter(src, c);
        EXPECT(equal(c, a));
        Mat in_place = src;
        f->filter(in_place, in_place);
        EXPECT(equal(in_place, a));
    }
    {   // refusals
        Mat g(10, 40, D8U, 1), g2(10, 40, D8U, 2), g16(10, 40, D16S, 1), s(10, 40, D16S, 1), s3(10, 40, D16S, 3), s32(10, 40, D32S, 1),
            small(10, 39, D8U, 1), empty, d;
        int thrown = 0;
        try { dtFilter(g, s, d, 10.0, 30.0, DTF_NC); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s, d, 10.0, 30.0, DTF_IC); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s, d, 10.0, 30.0, 7); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s, d, std::nan(""), 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s, d, 10.0, HUGE_VAL); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s, d, 10.0, 30.0, DTF_RF, ADF_DT_MAX_ITERS + 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s3, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, s32, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g2, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g16, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(g, empty, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtFilter(empty, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTFilter(g, 10.0, 30.0)->filter(s, d, D32S); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTFilter(g2, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTFilter(g, 10.0, 30.0, DTF_NC); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTFilter(g, 10.0, 30.0, DTF_RF, 9); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 16);
        try { dtFilter(small, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        try { createDTFilter(small, 10.0, 30.0)->filter(s, d); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 18);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
