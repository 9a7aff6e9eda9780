// adf::jointBilateralFilter (include/adf_ximgproc.hpp) on host Mats, compared bit for bit with the C-ABI call
// adf_joint_bilateral_filter_host and with a small sequential restatement of the definition in include/adf_wls.h fed with
// adf_jbf_tables_host (built and run by tests/test_cpp_jbf.py, with -ffp-contract=off: the statement's expressions are
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

// cv::borderInterpolate as OpenCV writes it: reflect step by step until the coordinate is inside.
static int border(int p, int n, int type)
{
    if (p >= 0 && p < n) return p;
    if (type == BORDER_REPLICATE) return p < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const int delta = type == BORDER_REFLECT_101;
    do p = p < 0 ? -p - 1 + delta : n - 1 - (p - n) - delta; while (p < 0 || p >= n);
    return p;
}

// The definition on an int16 map, float quotient: the taps in row-major order, one chain per sum.
static void jbf_ref(const Mat& joint, const Mat& src, std::vector<float>& y, int d, double sc, double ss, int type)
{
    const int H = src.rows, W = src.cols, ch = joint.cn;
    int r = 0;
    EXPECT(adf_jbf_tables_host(d, sc, ss, ch, nullptr, nullptr, &r) == ADF_OK);
    std::vector<float> C((size_t)255 * ch + 1), S((size_t)r * r + 1);
    EXPECT(adf_jbf_tables_host(d, sc, ss, ch, C.data(), S.data(), &r) == ADF_OK);
    y.resize((size_t)H * W);
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            float sum = 0.0f, wsum = 0.0f;
            for (int i = -r; i <= r; i++)
                for (int j = -r; j <= r; j++) {
                    if (i * i + j * j > r * r) continue;
                    const int qy = border(py + i, H, type), qx = border(px + j, W, type);
                    int L = 0;
                    for (int c = 0; c < ch; c++) L += std::abs((int)joint.ptr<uint8_t>(py)[px * ch + c] - (int)joint.ptr<uint8_t>(qy)[qx * ch + c]);
                    const float w = S[(size_t)(i * i + j * j)] * C[(size_t)L];
                    const float p = w * (float)src.ptr<int16_t>(qy)[qx];
                    sum = sum + p;
                    wsum = wsum + w;
                }
            y[(size_t)py * W + px] = sum / wsum;
        }
}

static void fill(Mat& joint, Mat& src, unsigned seed)
{
    std::mt19937 rng(seed);
    static const int16_t lv[] = {-16, 32, 480, 2000, -32768, 32767};
    for (int y = 0; y < src.rows; y++)
        for (int x = 0; x < src.cols; x++) {
            src.ptr<int16_t>(y)[x] = rng() % 4 ? lv[rng() % 6] : (int16_t)((int)(rng() % 65536) - 32768);
            for (int c = 0; c < joint.cn; c++)
                joint.ptr<uint8_t>(y)[x * joint.cn + c] = (uint8_t)std::min(255u, (unsigned)((x / 6) * 40 + (y / 4) * 25 + rng() % 9));
        }
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int shapes[][5] = {{21, 70, 1, 9, BORDER_REFLECT_101}, {37, 33, 3, -1, BORDER_REPLICATE}};   // H, W, joint channels, d, border
    unsigned seed = 1;
    for (auto& s : shapes) {
        const int H = s[0], W = s[1], ch = s[2], d = s[3], type = s[4];
        Mat joint(H, W, D8U, ch), src(H, W, D16S, 1);
        fill(joint, src, seed++);
        const double sc = 25.0, ss = 3.0;
        Mat abi(H, W, D16S, 1), abif(H, W, D32F, 1), got;
        EXPECT(adf_joint_bilateral_filter_host(1, joint.data, (ptrdiff_t)joint.step, 0, ch, src.data, (ptrdiff_t)src.step, 0, ADF_16S,
                                               abi.data, (ptrdiff_t)abi.step, 0, ADF_16S, W, H, d, sc, ss, type) == ADF_OK);
        jointBilateralFilter(joint, src, got, d, sc, ss, type);
        EXPECT(got.depth_ == D16S && equal(got, abi));                   // the adaptor is the C-ABI call, dst of src's depth
        EXPECT(!equal(got, src));                                        // the case is not vacuous
        // ... and the C-ABI call is the statement
        EXPECT(adf_joint_bilateral_filter_host(1, joint.data, (ptrdiff_t)joint.step, 0, ch, src.data, (ptrdiff_t)src.step, 0, ADF_16S,
                                               abif.data, (ptrdiff_t)abif.step, 0, ADF_32F, W, H, d, sc, ss, type) == ADF_OK);
        std::vector<float> y;
        jbf_ref(joint, src, y, d, sc, ss, type);
        bool same = true, rounded = true;
        for (int r = 0; r < H; r++) {
            same = same && std::memcmp(abif.ptr<float>(r), &y[(size_t)r * W], (size_t)W * 4) == 0;
            for (int x = 0; x < W; x++) rounded = rounded && abi.ptr<int16_t>(r)[x] == (int16_t)std::nearbyint(y[(size_t)r * W + x]);
        }
        EXPECT(same);
        EXPECT(rounded);
    }
    {   // the default border is BORDER_DEFAULT = BORDER_REFLECT_101, and the result may land in src
        Mat joint(12, 70, D8U, 3), src(12, 70, D16S, 1), a, b, c;
        fill(joint, src, 5);
        jointBilateralFilter(joint, src, a, 7, 25.0, 3.0);
        jointBilateralFilter(joint, src, b, 7, 25.0, 3.0, BORDER_REFLECT_101);
        jointBilateralFilter(joint, src, c, 7, 25.0, 3.0, BORDER_REFLECT);
        EXPECT(BORDER_DEFAULT == 4 && a.depth_ == D16S && equal(a, b) && !equal(a, c));
        Mat in_place = src;
        jointBilateralFilter(joint, in_place, in_place, 7, 25.0, 3.0);
        EXPECT(equal(in_place, a));
    }
    {   // refusals
        Mat g(10, 40, D8U, 1), g2(10, 40, D8U, 2), g32(10, 40, D32F, 1), s(10, 40, D16S, 1), s3(10, 40, D16S, 3), s32(10, 40, D32S, 1),
            s8(10, 40, D8U, 1), small(10, 39, D8U, 1), empty, d;
        int thrown = 0;
        try { jointBilateralFilter(g, s, d, 5, 25.0, 3.0, 0 /* BORDER_CONSTANT */); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s, d, 5, 25.0, 3.0, BORDER_WRAP); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s, d, 5, 25.0, 3.0, 16); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s, d, 5, std::nan(""), 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s, d, 5, 25.0, HUGE_VAL); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s, d, 2 * ADF_JBF_MAX_RADIUS + 2, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s, d, -1, 25.0, 21.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s3, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, s32, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g2, s, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g32, s, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(g, empty, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(empty, s, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { jointBilateralFilter(s8, s8, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 14);
        try { jointBilateralFilter(small, s, d, 5, 25.0, 3.0); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 15);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
