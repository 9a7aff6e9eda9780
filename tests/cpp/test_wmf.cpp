// adf::weightedMedianFilter (include/adf_ximgproc.hpp) on host Mats, checked bit for bit against a small sequential
// restatement of the definition in include/adf_wls.h (built and run by tests/test_cpp_wmf.py).
#include "adf_ximgproc.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <utility>
#include <vector>

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// The order of the values of one depth, as unsigned keys (floats: IEEE total order, -0.0 below +0.0).
static uint32_t key_of(uint8_t v) { return v; }
static uint32_t key_of(int16_t v) { return (uint32_t)(v + 32768); }
static uint32_t key_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
static bool is_nan(uint8_t) { return false; }
static bool is_nan(int16_t) { return false; }
static bool is_nan(float v) { return std::isnan(v); }

// The statement, pixel by pixel: the used taps sorted by key, the first whose cumulated weight reaches half the total.
template <class T>
static void wmf_ref(const Mat& joint, const Mat& src, Mat& dst, int r, const std::vector<uint32_t>& table, const Mat& mask,
                    const double* ignore)
{
    const int H = src.rows, W = src.cols, ch = joint.cn;
    dst = Mat(H, W, src.depth_, 1);
    std::vector<std::pair<uint32_t, std::pair<uint64_t, T>>> taps;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            taps.clear();
            uint64_t tot = 0;
            for (int qy = std::max(0, y - r); qy <= std::min(H - 1, y + r); qy++)
                for (int qx = std::max(0, x - r); qx <= std::min(W - 1, x + r); qx++) {
                    const T v = src.ptr<T>(qy)[qx];
                    if (!mask.empty() && mask.ptr<uint8_t>(qy)[qx] == 0) continue;
                    if (ignore && (double)v == *ignore) continue;
                    if (is_nan(v)) continue;
                    int d2 = 0;
                    for (int c = 0; c < ch; c++) {
                        const int d = (int)joint.ptr<uint8_t>(y)[x * ch + c] - (int)joint.ptr<uint8_t>(qy)[qx * ch + c];
                        d2 += d * d;
                    }
                    taps.push_back({key_of(v), {table[d2], v}});
                    tot += table[d2];
                }
            T out = src.ptr<T>(y)[x];
            if (tot > 0) {
                std::stable_sort(taps.begin(), taps.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
                uint64_t cum = 0;
                for (const auto& t : taps) {
                    cum += t.second.first;
                    if (2 * cum >= tot) { out = t.second.second; break; }
                }
            }
            dst.ptr<T>(y)[x] = out;
        }
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
    static const uint8_t lv[] = {0, 3, 3, 90, 255};
    return rng() % 4 ? lv[rng() % 5] : (uint8_t)(rng() % 256);
}
template <> int16_t sample<int16_t>(std::mt19937& rng)
{
    static const int16_t lv[] = {-16, -16, 32, 48, 160, -32768, 32767};
    return rng() % 4 ? lv[rng() % 7] : (int16_t)((int)(rng() % 600) - 300);
}
template <> float sample<float>(std::mt19937& rng)
{
    static const float lv[] = {0.0f, -0.0f, 1.5f, -2.25f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                               std::numeric_limits<float>::quiet_NaN(), 1.5f};
    return rng() % 4 ? lv[rng() % 8] : (float)((int)(rng() % 2000) - 1000) / 64.0f;
}

template <class T>
static int run_depth(int depth, double ignore_value, unsigned seed)
{
    int changed = 0;
    const int sizes[][2] = {{1, 1}, {3, 5}, {9, 33}, {17, 70}};
    for (auto& s : sizes)
        for (int ch : {1, 3})
            for (int r : {1, 3, 8})
                for (int variant = 0; variant < 4; variant++) {        // neither, mask, ignore, both
                    std::mt19937 rng(seed++);
                    const int H = s[0], W = s[1];
                    Mat joint(H, W, D8U, ch), src(H, W, depth, 1), mask;
                    for (int y = 0; y < H; y++)
                        for (int x = 0; x < W; x++) {
                            src.ptr<T>(y)[x] = sample<T>(rng);
                            for (int c = 0; c < ch; c++)
                                joint.ptr<uint8_t>(y)[x * ch + c] = (uint8_t)std::min(255u, (unsigned)((x / 6) * 40 + (y / 4) * 25 + rng() % 9));
                        }
                    if (variant & 1) {
                        mask = Mat(H, W, D8U, 1);
                        for (int y = 0; y < H; y++)
                            for (int x = 0; x < W; x++) mask.ptr<uint8_t>(y)[x] = rng() % 5 ? (uint8_t)(1 + rng() % 255) : 0;
                    }
                    const double sigma = r == 3 ? 0.75 : 10.0;
                    const int wt = r == 8 ? WMF_OFF : WMF_EXP;
                    std::vector<uint32_t> table(ADF_WMF_TABLE_LEVELS);
                    check(adf_wmf_weight_table_host(sigma, wt, table.data(), ADF_WMF_TABLE_LEVELS));
                    Mat exp, got;
                    wmf_ref<T>(joint, src, exp, r, table, mask, variant & 2 ? &ignore_value : nullptr);
                    if (variant & 2) weightedMedianFilter(joint, src, got, r, sigma, wt, mask, ignore_value);
                    else weightedMedianFilter(joint, src, got, r, sigma, wt, mask);
                    EXPECT(equal(got, exp));
                    changed += !equal(exp, src);
                }
    return changed;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    int changed = run_depth<uint8_t>(D8U, 3.0, 1);
    changed += run_depth<int16_t>(D16S, -16.0, 1000);
    changed += run_depth<float>(D32F, 1.5, 2000);
    EXPECT(changed > 150);                                               // the cases are not vacuous
    {   // the defaults are cv's, and the result may land in src
        std::mt19937 rng(5);
        Mat joint(12, 40, D8U, 1), src(12, 40, D16S, 1), a, b;
        for (int y = 0; y < 12; y++)
            for (int x = 0; x < 40; x++) { joint.ptr<uint8_t>(y)[x] = (uint8_t)(rng() % 256); src.ptr<int16_t>(y)[x] = sample<int16_t>(rng); }
        weightedMedianFilter(joint, src, a, 2);
        weightedMedianFilter(joint, src, b, 2, 25.5, WMF_EXP, Mat());
        EXPECT(equal(a, b));
        weightedMedianFilter(joint, src, src, 2);
        EXPECT(equal(src, a));
    }
    {   // refusals
        Mat j(10, 40, D8U, 1), j2(10, 40, D8U, 2), s(10, 40, D16S, 1), s3(10, 40, D16S, 3), s32(10, 40, D32S, 1), small(10, 39, D8U, 1),
            m16(10, 40, D16S, 1), empty, d;
        int thrown = 0;
        for (int wt : {(int)WMF_IV1, (int)WMF_IV2, (int)WMF_COS, (int)WMF_JAC, 6})
            try { weightedMedianFilter(j, s, d, 2, 25.5, wt); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 5);
        try { weightedMedianFilter(j, s, d, 0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s, d, ADF_WMF_MAX_RADIUS + 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s, d, 2, 0.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s, d, 2, std::nan("")); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s3, d, 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s32, d, 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j2, s, d, 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(s, s, d, 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, empty, d, 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s, d, 2, 25.5, WMF_EXP, m16); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s, d, 2, 25.5, WMF_EXP, Mat(), 0.5); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { weightedMedianFilter(j, s, d, 2, 25.5, WMF_EXP, Mat(), 32768.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 17);
        try { weightedMedianFilter(small, s, d, 2); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        try { weightedMedianFilter(j, s, d, 2, 25.5, WMF_EXP, small); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 19);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
