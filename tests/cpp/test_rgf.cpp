// adf::rollingGuidanceFilter (include/adf_ximgproc.hpp) on host Mats, compared bit for bit with the C-ABI call
// adf_rolling_guidance_filter_host and with a small sequential restatement of the definition in include/adf_wls.h fed
// with adf_rgf_tables_host (built and run by tests/test_cpp_rgf.py, with -ffp-contract=off: the statement's expressions
// are evaluated operation by operation).
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

// The definition on a map of T (int16_t or float): J_0 = src, num_iter times the weighted mean with the range weight on J_k.
template <class T> static void rgf_ref(const Mat& src, Mat& dst, int depth, int d, double sc, double ss, int num_iter, int type)
{
    const int H = src.rows, W = src.cols;
    int r = 0, entries = 0;
    float scale = 0.0f;
    EXPECT(adf_rgf_tables_host(depth, d, sc, ss, nullptr, nullptr, &r, &entries, &scale) == ADF_OK);
    std::vector<float> C((size_t)entries), S((size_t)r * r + 1);
    EXPECT(adf_rgf_tables_host(depth, d, sc, ss, C.data(), S.data(), nullptr, nullptr, nullptr) == ADF_OK);
    std::vector<T> J((size_t)H * W), next((size_t)H * W);
    for (int y = 0; y < H; y++) std::memcpy(&J[(size_t)y * W], src.ptr<T>(y), (size_t)W * sizeof(T));
    for (int k = 0; k < num_iter; k++) {
        for (int py = 0; py < H; py++)
            for (int px = 0; px < W; px++) {
                float sum = 0.0f, wsum = 0.0f;
                for (int i = -r; i <= r; i++)
                    for (int j = -r; j <= r; j++) {
                        if (i * i + j * j > r * r) continue;
                        const int qy = border(py + i, H, type), qx = border(px + j, W, type);
                        float wc;
                        if (depth == ADF_32F) {
                            float a = std::fabs((float)J[(size_t)py * W + px] - (float)J[(size_t)qy * W + qx]) * scale;
                            if (!(a < 4096.0f)) a = 4096.0f;
                            const int idx = (int)a;
                            const float f = a - (float)idx, step = C[(size_t)idx + 1] - C[(size_t)idx], part = f * step;
                            wc = C[(size_t)idx] + part;
                        } else {
                            const int L = std::abs((int)J[(size_t)py * W + px] - (int)J[(size_t)qy * W + qx]);
                            wc = C[(size_t)std::min(L, entries - 1)];
                        }
                        const float w = S[(size_t)(i * i + j * j)] * wc;
                        const float p = w * (float)src.ptr<T>(qy)[qx];
                        sum = sum + p;
                        wsum = wsum + w;
                    }
                const float y = sum / wsum;
                next[(size_t)py * W + px] = depth == ADF_32F ? (T)y : (T)std::min(32767.0f, std::max(-32768.0f, std::nearbyint(y)));
            }
        J.swap(next);
    }
    dst = Mat(H, W, src.depth_, 1);
    for (int y = 0; y < H; y++) std::memcpy(dst.ptr<T>(y), &J[(size_t)y * W], (size_t)W * sizeof(T));
}

static void fill(Mat& src, unsigned seed)
{
    std::mt19937 rng(seed);
    static const int lv[] = {-16, 32, 480, 2000, 520, 90};
    for (int y = 0; y < src.rows; y++)
        for (int x = 0; x < src.cols; x++) {
            const int v = lv[((x / 6) + (y / 4) * 3) % 6] + (rng() % 3 ? 0 : (int)(rng() % 81) - 40);
            if (src.depth_ == D16S) src.ptr<int16_t>(y)[x] = (int16_t)v;
            else src.ptr<float>(y)[x] = (float)v + (float)(rng() % 16) / 16.0f;
        }
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int shapes[][6] = {{21, 70, D16S, 9, 4, BORDER_REFLECT_101}, {37, 33, D32F, -1, 3, BORDER_REPLICATE}};   // H, W, depth, d, iterations, border
    unsigned seed = 1;
    for (auto& s : shapes) {
        const int H = s[0], W = s[1], mdepth = s[2], d = s[3], n = s[4], type = s[5], depth = mdepth == D16S ? ADF_16S : ADF_32F;
        Mat src(H, W, mdepth, 1), abi(H, W, mdepth, 1), got, ref;
        fill(src, seed++);
        const double sc = 25.0, ss = 3.0;
        EXPECT(adf_rolling_guidance_filter_host(1, src.data, (ptrdiff_t)src.step, 0, abi.data, (ptrdiff_t)abi.step, 0, depth, W, H, d, sc, ss, n,
                                                type) == ADF_OK);
        rollingGuidanceFilter(src, got, d, sc, ss, n, type);
        EXPECT(got.depth_ == mdepth && equal(got, abi));                 // the adaptor is the C-ABI call, dst of src's type
        EXPECT(!equal(got, src));                                        // the case is not vacuous
        if (mdepth == D16S) rgf_ref<int16_t>(src, ref, depth, d, sc, ss, n, type);
        else rgf_ref<float>(src, ref, depth, d, sc, ss, n, type);
        EXPECT(equal(abi, ref));                                         // ... and the C-ABI call is the statement
    }
    {   // the reference's defaults (d = -1, 25, 3, 4 iterations, BORDER_DEFAULT), zero iterations, and a result that lands in src
        Mat src(12, 70, D16S, 1), a, b, c, z;
        fill(src, 5);
        rollingGuidanceFilter(src, a);
        rollingGuidanceFilter(src, b, -1, 25.0, 3.0, 4, BORDER_REFLECT_101);
        rollingGuidanceFilter(src, c, -1, 25.0, 3.0, 4, BORDER_REFLECT);
        rollingGuidanceFilter(src, z, -1, 25.0, 3.0, 0);
        EXPECT(a.depth_ == D16S && equal(a, b) && !equal(a, c) && equal(z, src));
        Mat in_place = src;
        rollingGuidanceFilter(in_place, in_place);
        EXPECT(equal(in_place, a));
    }
    {   // refusals
        Mat s(10, 40, D16S, 1), s3(10, 40, D16S, 3), s32(10, 40, D32S, 1), f(10, 40, D32F, 1), empty, d;
        int thrown = 0;
        try { rollingGuidanceFilter(s, d, 5, 25.0, 3.0, 4, 0 /* BORDER_CONSTANT */); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s, d, 5, 25.0, 3.0, 4, BORDER_WRAP); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s, d, 5, std::nan(""), 3.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s, d, 5, 25.0, HUGE_VAL); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s, d, 2 * ADF_JBF_MAX_RADIUS + 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s, d, -1, 25.0, 3.0, -1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s, d, -1, 25.0, 3.0, ADF_RGF_MAX_ITERS + 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(f, d, -1, 1e-37); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s3, d); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(s32, d); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { rollingGuidanceFilter(empty, d); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 11);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
