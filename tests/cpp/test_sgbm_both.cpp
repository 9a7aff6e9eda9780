// StereoSGBM::computeBoth through the header-only C++ adaptor (include/adf_ximgproc.hpp) on host Mats: the right
// matcher's source against the two separate computes, the volume source's left map against compute(), its right map's
// range, and the refusals (built and run by tests/test_cpp_sgbm_both.py).
#include "adf_ximgproc.hpp"

#include <cstdio>
#include <cstring>
#include <random>

using namespace adf;
using namespace adf::ximgproc;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool same(const Mat& a, const Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols || mat_depth(a) != D16S || mat_depth(b) != D16S) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<int16_t>(y), b.ptr<int16_t>(y), (size_t)a.cols * 2)) return false;
    return true;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int H = 30, W = 150, nd = 32;
    std::mt19937 rng(5);
    std::uniform_int_distribution<int> v(0, 255);
    Mat base(H, W + 40, D8U, 1), left(H, W, D8U, 1), right(H, W, D8U, 1);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W + 40; x++) base.ptr<uint8_t>(y)[x] = (uint8_t)v(rng);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) { left.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 20]; right.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 26]; }
    Ptr<StereoSGBM> lm = StereoSGBM::create(0, nd, 3);
    lm->setP1(216); lm->setP2(864); lm->setPreFilterCap(63); lm->setMode(StereoSGBM::MODE_SGBM_3WAY);
    lm->setUniquenessRatio(10); lm->setDisp12MaxDiff(1);                       // the left map keeps the matcher's own tests
    Ptr<StereoSGBM> rm = createRightMatcher(lm);
    Mat dl, dr, bl, br, vl, vr;
    lm->compute(left, right, dl);
    rm->compute(right, left, dr);
    lm->computeBoth(left, right, bl, br);                                      // the default source: the right matcher's map
    EXPECT(same(bl, dl) && same(br, dr));
    lm->computeBoth(left, right, vl, vr, ADF_SGBM_RIGHT_FROM_VOLUME);
    EXPECT(same(vl, dl));
    EXPECT(vr.rows == H && vr.cols == W && mat_depth(vr) == D16S && !same(vr, dr));
    int good = 0, in_range = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const int d = vr.ptr<int16_t>(y)[x];
            in_range += d <= 0 && d >= -nd * 16;                               // -(md + nd) * 16 (invalid) ... -md * 16
            if (x >= nd && x < W - nd) good += std::abs(d + 6 * 16) <= 8;        // the pair is shifted by 6 columns
        }
    EXPECT(in_range == H * W);
    EXPECT(good > H * (W - 2 * nd) * 9 / 10);
    Mat again;
    lm->compute(left, right, again);                                           // the handle is the left matcher's again
    EXPECT(same(again, dl));
    {   // refusals: an unknown source, the speckle filter, mismatched views
        int thrown = 0;
        try { lm->computeBoth(left, right, bl, br, 2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        lm->setSpeckleWindowSize(100);
        try { lm->computeBoth(left, right, bl, br); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        lm->setSpeckleWindowSize(0);
        Mat narrow(H, W - 1, D8U, 1);
        try { lm->computeBoth(left, narrow, bl, br); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 3);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
