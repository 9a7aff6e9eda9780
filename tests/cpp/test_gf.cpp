// adf::guidedFilter / adf::createGuidedFilter (include/adf_ximgproc.hpp) on host Mats, checked bit for bit against a small
// sequential restatement of the definition in include/adf_wls.h (built and run by tests/test_cpp_gf.py, with
// -ffp-contract=off: the statement's expressions are evaluated operation by operation).
#include "adf_ximgproc.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <type_traits>
#include <vector>

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static int reflect(long long i, int n)
{
    const long long p = 2ll * n;
    long long m = i % p;
    if (m < 0) m += p;
    return (int)(m < n ? m : p - 1 - m);
}

// The window sum of f(y, x) in the statement's order: column sums top to bottom, then the row sum left to right, every
// partial sum an Acc.
template <class Acc, class F> static Acc window_sum(int y, int x, int r, int H, int W, F f)
{
    Acc s = 0;
    for (int dx = -r; dx <= r; dx++) {
        const int qx = reflect(x + dx, W);
        Acc c = f(reflect(y - r, H), qx);
        for (int dy = -r + 1; dy <= r; dy++) c = (Acc)(c + f(reflect(y + dy, H), qx));
        s = dx == -r ? c : (Acc)(s + c);
    }
    return s;
}

template <class T> static T convert(double q);
template <> float convert<float>(double q) { return (float)q; }
template <> uint8_t convert<uint8_t>(double q) { const double v = std::nearbyint(q); return !(v >= 0.0) ? 0 : v > 255.0 ? 255 : (uint8_t)v; }
template <> int16_t convert<int16_t>(double q) { const double v = std::nearbyint(q); return !(v >= -32768.0) ? -32768 : v > 32767.0 ? 32767 : (int16_t)v; }

template <class TS, class TD>
static void gf_ref(const Mat& guide, const Mat& src, Mat& dst, int ddepth, int r, double eps)
{
    const int H = src.rows, W = src.cols, ch = guide.cn, n = 2 * r + 1;
    const long long N = (long long)n * n;
    const double Nd = (double)N, E = eps * Nd * Nd;
    auto I = [&](int c, int y, int x) { return (long long)guide.ptr<uint8_t>(y)[x * ch + c]; };
    std::vector<float> coef((size_t)(ch + 1) * H * W);                   // a_c planes, then b
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            long long S[3] = {0, 0, 0};
            double V[3][3], nc[3];
            for (int c = 0; c < ch; c++) S[c] = window_sum<long long>(y, x, r, H, W, [&](int qy, int qx) { return I(c, qy, qx); });
            for (int c = 0; c < ch; c++)
                for (int d = c; d < ch; d++)
                    V[c][d] = (double)(N * window_sum<long long>(y, x, r, H, W, [&](int qy, int qx) { return I(c, qy, qx) * I(d, qy, qx); }) - S[c] * S[d]);
            double Sp;
            if (std::is_same<TS, float>::value) {
                Sp = window_sum<double>(y, x, r, H, W, [&](int qy, int qx) { return (double)src.ptr<TS>(qy)[qx]; });
                for (int c = 0; c < ch; c++) {
                    const double Scp = window_sum<double>(y, x, r, H, W, [&](int qy, int qx) { return (double)I(c, qy, qx) * (double)src.ptr<TS>(qy)[qx]; });
                    const double t0 = Nd * Scp, t1 = (double)S[c] * Sp;
                    nc[c] = t0 - t1;
                }
            } else {
                const long long Spi = window_sum<long long>(y, x, r, H, W, [&](int qy, int qx) { return (long long)src.ptr<TS>(qy)[qx]; });
                Sp = (double)Spi;
                for (int c = 0; c < ch; c++)
                    nc[c] = (double)(N * window_sum<long long>(y, x, r, H, W, [&](int qy, int qx) { return I(c, qy, qx) * (long long)src.ptr<TS>(qy)[qx]; }) - S[c] * Spi);
            }
            float a[3] = {0, 0, 0};
            if (ch == 1) {
                a[0] = (float)(nc[0] / (V[0][0] + E));
            } else {
                const double s00 = V[0][0] + E, s11 = V[1][1] + E, s22 = V[2][2] + E, s01 = V[0][1], s02 = V[0][2], s12 = V[1][2];
                const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
                const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
                const double det = (s00 * c00 + s01 * c01) + s02 * c02;
                if (std::isfinite(det) && det > 0.0) {
                    a[0] = (float)(((c00 * nc[0] + c01 * nc[1]) + c02 * nc[2]) / det);
                    a[1] = (float)(((c01 * nc[0] + c11 * nc[1]) + c12 * nc[2]) / det);
                    a[2] = (float)(((c02 * nc[0] + c12 * nc[1]) + c22 * nc[2]) / det);
                }
            }
            double bn = Sp;
            for (int c = 0; c < ch; c++) bn = bn - (double)a[c] * (double)S[c];
            for (int c = 0; c < ch; c++) coef[((size_t)c * H + y) * W + x] = a[c];
            coef[((size_t)ch * H + y) * W + x] = (float)(bn / Nd);
        }
    dst = Mat(H, W, ddepth, 1);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            auto SA = [&](int c) { return window_sum<float>(y, x, r, H, W, [&](int qy, int qx) { return coef[((size_t)c * H + qy) * W + qx]; }); };
            double q = (double)SA(ch);
            for (int c = 0; c < ch; c++) q = q + (double)SA(c) * (double)I(c, y, x);
            dst.ptr<TD>(y)[x] = convert<TD>(q / Nd);
        }
}

template <class TS>
static void gf_ref_to(const Mat& guide, const Mat& src, Mat& dst, int ddepth, int r, double eps)
{
    if (ddepth == D8U) gf_ref<TS, uint8_t>(guide, src, dst, ddepth, r, eps);
    else if (ddepth == D16S) gf_ref<TS, int16_t>(guide, src, dst, ddepth, r, eps);
    else gf_ref<TS, float>(guide, src, dst, ddepth, r, eps);
}

static bool equal(const Mat& a, const Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols || a.depth_ != b.depth_) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<unsigned char>(y), b.ptr<unsigned char>(y), (size_t)a.cols * Mat::esz(a.depth_)) != 0) return false;
    return true;
}

template <class T> static T sample(std::mt19937& rng);
template <> uint8_t sample<uint8_t>(std::mt19937& rng)
{
    static const uint8_t lv[] = {0, 3, 90, 255};
    return rng() % 4 ? lv[rng() % 4] : (uint8_t)(rng() % 256);
}
template <> int16_t sample<int16_t>(std::mt19937& rng)
{
    static const int16_t lv[] = {-16, 32, 480, 2000, -32768, 32767};
    return rng() % 4 ? lv[rng() % 6] : (int16_t)((int)(rng() % 65536) - 32768);
}
template <> float sample<float>(std::mt19937& rng)
{
    static const float lv[] = {0.0f, 1.5f, -2.25f, 480.125f};
    return rng() % 4 ? lv[rng() % 4] : (float)((int)(rng() % 20000) - 10000) / 64.0f;
}

template <class T>
static int run_depth(int depth, unsigned seed)
{
    int changed = 0;
    const int sizes[][2] = {{1, 1}, {3, 5}, {9, 33}, {17, 70}};
    const int ddepths[] = {-1, D8U, D16S, D32F};
    for (auto& s : sizes)
        for (int ch : {1, 3})
            for (int r : {0, 1, 3, 9}) {
                std::mt19937 rng(seed++);
                const int H = s[0], W = s[1];
                Mat guide(H, W, D8U, ch), src(H, W, depth, 1);
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++) {
                        src.ptr<T>(y)[x] = sample<T>(rng);
                        for (int c = 0; c < ch; c++)
                            guide.ptr<uint8_t>(y)[x * ch + c] = x >= W / 2 && y >= H / 2 ? 90 : (uint8_t)std::min(255u, (unsigned)((x / 6) * 40 + (y / 4) * 25 + rng() % 9));
                    }
                const double eps = r == 3 ? 0.01 : r == 9 ? 6502.5 : 1.0;
                for (int dDepth : ddepths) {
                    Mat exp, got, obj;
                    gf_ref_to<T>(guide, src, exp, dDepth == -1 ? depth : dDepth, r, eps);
                    guidedFilter(guide, src, got, r, eps, dDepth);
                    EXPECT(equal(got, exp));
                    createGuidedFilter(guide, r, eps)->filter(src, obj, dDepth);
                    EXPECT(equal(obj, exp));
                    changed += exp.depth_ != src.depth_ || !equal(exp, src);
                }
            }
    return changed;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    int changed = run_depth<uint8_t>(D8U, 1);
    changed += run_depth<int16_t>(D16S, 1000);
    changed += run_depth<float>(D32F, 2000);
    EXPECT(changed > 250);                                               // the cases are not vacuous
    {   // dDepth defaults to src's depth, the result may land in src, and the object keeps its own guide
        std::mt19937 rng(5);
        Mat guide(12, 40, D8U, 3), src(12, 40, D16S, 1), a, b, c;
        for (int y = 0; y < 12; y++)
            for (int x = 0; x < 40; x++) {
                src.ptr<int16_t>(y)[x] = sample<int16_t>(rng);
                for (int k = 0; k < 3; k++) guide.ptr<uint8_t>(y)[3 * x + k] = (uint8_t)(rng() % 256);
            }
        guidedFilter(guide, src, a, 2, 4.0);
        guidedFilter(guide, src, b, 2, 4.0, D16S);
        EXPECT(a.depth_ == D16S && equal(a, b));
        Ptr<GuidedFilter> gf = createGuidedFilter(guide, 2, 4.0);
        std::memset(guide.data, 0, guide.step * guide.rows);             // the caller's guide changes; the object's does not
        gf->filter(src, c);
        EXPECT(equal(c, a));
        Mat in_place = src;
        gf->filter(in_place, in_place);
        EXPECT(equal(in_place, a));
    }
    {   // refusals
        Mat g(10, 40, D8U, 1), g2(10, 40, D8U, 2), g16(10, 40, D16S, 1), s(10, 40, D16S, 1), s3(10, 40, D16S, 3), s32(10, 40, D32S, 1),
            small(10, 39, D8U, 1), empty, d;
        int thrown = 0;
        try { guidedFilter(g, s, d, -1, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s, d, ADF_GF_MAX_RADIUS + 1, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s, d, 2, 0.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s, d, 2, -1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s, d, 2, std::nan("")); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s, d, 2, HUGE_VAL); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s3, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s32, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g2, s, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g16, s, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, empty, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(empty, s, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { guidedFilter(g, s, d, 2, 1.0, D32S); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createGuidedFilter(g2, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createGuidedFilter(g, 32, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { createGuidedFilter(g, 2, 0.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 16);
        try { guidedFilter(small, s, d, 2, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        try { createGuidedFilter(small, 2, 1.0)->filter(s, d); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 18);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
