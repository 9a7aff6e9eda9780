// adf::dtWindowFilter / adf::createDTWindowFilter (include/adf_ximgproc.hpp) on host Mats, compared bit for bit with the
// C-ABI call adf_dt_window_filter_host and with a small sequential restatement of the definition in include/adf_wls.h fed
// with adf_dt_nc_radii_host (built and run by tests/test_cpp_dt_window.py, with -ffp-contract=off: the statement's
// expressions are evaluated operation by operation).
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

// One scanline of n pixels, `stride` floats apart: in -> out.  L(a): the guide's L1 difference between pixels a and a + 1.
template <class LFN>
static void pass(const float* in, float* out, int n, int stride, float r, float k, LFN L)
{
    for (int j = 0; j < n; j++) {
        int lb = j, rb = j, S = 0;
        while (lb > 0) {                                                 // the smallest a with D(a, j) <= r
            S += L(lb - 1);
            const float ks = k * (float)S;
            const float d = (float)(j - lb + 1) + ks;
            if (!(d <= r)) break;
            lb--;
        }
        S = 0;
        while (rb < n - 1) {                                             // the largest b with D(j, b) < r
            S += L(rb);
            const float ks = k * (float)S;
            const float d = (float)(rb + 1 - j) + ks;
            if (!(d < r)) break;
            rb++;
        }
        float acc = in[(size_t)lb * stride];
        for (int p = lb + 1; p <= rb; p++) acc = acc + in[(size_t)p * stride];
        out[(size_t)j * stride] = acc / (float)(rb - lb + 1);
    }
}

// The iterations on an int16 map, float result: every row, then every column, per iteration.
static void dtw_ref(const Mat& guide, const Mat& src, std::vector<float>& x, double ss, double sr, int N)
{
    const int H = src.rows, W = src.cols, ch = guide.cn;
    std::vector<float> radii(N), y((size_t)H * W);
    EXPECT(adf_dt_nc_radii_host(ss, N, radii.data()) == ADF_OK);
    const float k = std::max(1.0f, (float)ss) / std::max(0.01f, (float)sr);
    auto L = [&](int y0, int x0, int y1, int x1) {
        int s = 0;
        for (int c = 0; c < ch; c++) s += std::abs((int)guide.ptr<uint8_t>(y0)[x0 * ch + c] - (int)guide.ptr<uint8_t>(y1)[x1 * ch + c]);
        return s;
    };
    x.resize((size_t)H * W);
    for (int r = 0; r < H; r++)
        for (int j = 0; j < W; j++) x[(size_t)r * W + j] = (float)src.ptr<int16_t>(r)[j];
    for (int i = 0; i < N; i++) {
        for (int r = 0; r < H; r++) pass(&x[(size_t)r * W], &y[(size_t)r * W], W, 1, radii[i], k, [&](int a) { return L(r, a, r, a + 1); });
        for (int c = 0; c < W; c++) pass(&y[c], &x[c], H, W, radii[i], k, [&](int a) { return L(a, c, a + 1, c); });
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
    const int shapes[][3] = {{33, 1025, 1}, {129, 33, 3}};                // H, W, guide channels
    unsigned seed = 1;
    for (auto& s : shapes) {
        const int H = s[0], W = s[1], ch = s[2];
        Mat guide(H, W, D8U, ch), src(H, W, D16S, 1);
        fill(guide, src, seed++);
        const double ss = ch == 1 ? 12.0 : 80.0, sr = ch == 1 ? 25.0 : 50.0;   // radii 18, 9, 4 and 120, 60, 30
        const int N = 3;
        const int ddepths[] = {-1, D8U, D16S, D32F};
        for (int dDepth : ddepths) {
            const int ddepth = dDepth == -1 ? D16S : dDepth;
            Mat abi(H, W, ddepth, 1), obj;
            EXPECT(adf_dt_window_filter_host(1, guide.data, (ptrdiff_t)guide.step, 0, ch, src.data, (ptrdiff_t)src.step, 0, ADF_16S,
                                             abi.data, (ptrdiff_t)abi.step, 0, code(ddepth), W, H, ss, sr, ADF_DTF_NC, N) == ADF_OK);
            createDTWindowFilter(guide, ss, sr, DTF_NC, N)->filter(src, obj, dDepth);
            EXPECT(equal(obj, abi));
            if (dDepth == -1) {                                          // dtWindowFilter has no dDepth: src's depth
                Mat got;
                dtWindowFilter(guide, src, got, ss, sr, DTF_NC, N);
                EXPECT(equal(got, abi));
                EXPECT(!equal(got, src));                                // the case is not vacuous
            }
            if (ddepth == D32F) {                                        // ... and the C-ABI call is the statement
                std::vector<float> x;
                dtw_ref(guide, src, x, ss, sr, N);
                bool same = true;
                for (int y = 0; y < H; y++) same = same && std::memcmp(abi.ptr<float>(y), &x[(size_t)y * W], (size_t)W * 4) == 0;
                EXPECT(same);
            }
        }
    }
    {   // the defaults are DTF_NC and 3 iterations, the result may land in src, and the object keeps its own guide
        Mat guide(12, 70, D8U, 3), src(12, 70, D16S, 1), a, b, c;
        fill(guide, src, 5);
        dtWindowFilter(guide, src, a, 10.0, 30.0);
        dtWindowFilter(guide, src, b, 10.0, 30.0, DTF_NC, 3);
        EXPECT(a.depth_ == D16S && equal(a, b));
        Ptr<DTWindowFilter> f = createDTWindowFilter(guide, 10.0, 30.0);
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
        try { dtWindowFilter(g, s, d, 10.0, 30.0, DTF_RF); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s, d, 10.0, 30.0, DTF_IC); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s, d, 10.0, 30.0, 7); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s, d, std::nan(""), 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s, d, 10.0, HUGE_VAL); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s, d, 10.0, 30.0, DTF_NC, ADF_DT_MAX_ITERS + 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s, d, 80.0, 50.0, DTF_NC, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }   // r_1 = 138.6
        try { dtWindowFilter(g, s3, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, s32, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g2, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g16, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(g, empty, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { dtWindowFilter(empty, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTWindowFilter(g, 10.0, 30.0)->filter(s, d, D32S); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTWindowFilter(g2, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTWindowFilter(g, 10.0, 30.0, DTF_RF); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTWindowFilter(g, 10.0, 30.0, DTF_IC); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTWindowFilter(g, 10.0, 30.0, DTF_NC, 9); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createDTWindowFilter(g, 1000.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 19);
        try { dtWindowFilter(small, s, d, 10.0, 30.0); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        try { createDTWindowFilter(small, 10.0, 30.0)->filter(s, d); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 21);
        // the old names keep refusing the mode
        try { dtFilter(g, s, d, 10.0, 30.0, DTF_NC); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 22);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
