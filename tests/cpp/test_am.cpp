// adf::amFilter / adf::createAMFilter / adf::AdaptiveManifoldFilter (include/adf_ximgproc.hpp) on host Mats, compared bit
// for bit with the C-ABI call adf_am_filter_host and, through two checksums, with values recorded from the NumPy statement
// tests/am_ref.py on the same formula-made images (built and run by tests/test_cpp_am.py).
#include "adf_ximgproc.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

// joint = min(255, x/6*40 + y/4*25 + (7x + 13y + 29c) % 9); src = (37x + 101y) % 4001 - 2000, 5000 higher in the right half
static void fill(Mat& joint, Mat& src)
{
    for (int y = 0; y < src.rows; y++)
        for (int x = 0; x < src.cols; x++) {
            src.ptr<int16_t>(y)[x] = (int16_t)((x * 37 + y * 101) % 4001 - 2000 + (x >= src.cols / 2 ? 5000 : 0));
            for (int c = 0; c < joint.cn; c++)
                joint.ptr<uint8_t>(y)[x * joint.cn + c] = (uint8_t)std::min(255, (x / 6) * 40 + (y / 4) * 25 + (x * 7 + y * 13 + c * 29) % 9);
        }
}

// sum of the pixels, and of the pixels times 1 + (their index % 251)
static void checksums(const Mat& m, long long* sum, long long* weighted)
{
    *sum = *weighted = 0;
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) {
            const long long v = m.ptr<int16_t>(y)[x];
            *sum += v;
            *weighted += v * (1 + (y * m.cols + x) % 251);
        }
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int H = 45, W = 66;
    // recorded from tests/am_ref.py at (sigma_s, sigma_r) = (16, 0.2): [channels 1, 3][adjust_outliers off, on] -> sum, weighted sum
    const long long recorded[2][2][2] = {{{7421467, 935284016}, {7412590, 934316181}}, {{7526999, 948229185}, {7511889, 946692658}}};
    for (int k = 0; k < 2; k++) {
        const int ch = k ? 3 : 1;
        Mat joint(H, W, D8U, ch), src(H, W, D16S, 1);
        fill(joint, src);
        for (int adjust = 0; adjust < 2; adjust++) {
            Mat abi(H, W, D16S, 1), got, obj;
            EXPECT(adf_am_filter_host(1, joint.data, (ptrdiff_t)joint.step, 0, ch, src.data, (ptrdiff_t)src.step, 0, ADF_16S,
                                      abi.data, (ptrdiff_t)abi.step, 0, ADF_16S, W, H, 16.0, 0.2, -1, adjust) == ADF_OK);
            amFilter(joint, src, got, 16.0, 0.2, adjust != 0);
            EXPECT(got.depth_ == D16S && equal(got, abi));
            EXPECT(!equal(got, src));                                    // the case is not vacuous
            createAMFilter(16.0, 0.2, adjust != 0)->filter(src, obj, joint);
            EXPECT(equal(obj, abi));
            long long sum, weighted;
            checksums(abi, &sum, &weighted);
            EXPECT(sum == recorded[k][adjust][0] && weighted == recorded[k][adjust][1]);
            if (sum != recorded[k][adjust][0]) std::printf("channels %d adjust %d: sum %lld weighted %lld\n", ch, adjust, sum, weighted);
        }
    }
    {   // the defaults, the properties, and a result that lands in src
        Mat joint(H, W, D8U, 3), src(H, W, D16S, 1), a, b;
        fill(joint, src);
        Ptr<AdaptiveManifoldFilter> f = AdaptiveManifoldFilter::create();
        EXPECT(f->getSigmaS() == 16.0 && f->getSigmaR() == 0.2 && f->getTreeHeight() == -1 && f->getPCAIterations() == 1);
        EXPECT(!f->getAdjustOutliers() && !f->getUseRNG());
        amFilter(joint, src, a, 16.0, 0.2);
        f->filter(src, b, joint);
        EXPECT(equal(a, b));
        f->setPCAIterations(0);
        EXPECT(f->getPCAIterations() == 1);
        f->setPCAIterations(7);                                          // stored; the result does not change
        f->setUseRNG(false);
        f->collectGarbage();
        Mat in_place = src;
        f->filter(in_place, in_place, joint);
        EXPECT(f->getPCAIterations() == 7 && equal(in_place, a));
        f->setTreeHeight(2);
        f->setSigmaS(8.0);
        f->setSigmaR(0.3);
        f->setAdjustOutliers(true);
        EXPECT(f->getTreeHeight() == 2 && f->getSigmaS() == 8.0 && f->getSigmaR() == 0.3 && f->getAdjustOutliers());
        Mat abi(H, W, D16S, 1), c;
        EXPECT(adf_am_filter_host(1, joint.data, (ptrdiff_t)joint.step, 0, 3, src.data, (ptrdiff_t)src.step, 0, ADF_16S,
                                  abi.data, (ptrdiff_t)abi.step, 0, ADF_16S, W, H, 8.0, 0.3, 2, 1) == ADF_OK);
        f->filter(src, c, joint);
        EXPECT(equal(c, abi));
    }
    {   // refusals
        Mat g(10, 40, D8U, 1), g2(10, 40, D8U, 2), g16(10, 40, D16S, 1), s(10, 40, D16S, 1), s3(10, 40, D16S, 3), s32(10, 40, D32S, 1),
            small(10, 39, D8U, 1), tiny_g(2, 40, D8U, 1), tiny_s(2, 40, D16S, 1), empty, d;
        int thrown = 0;
        try { amFilter(g, s, d, 0.5, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, s, d, std::nan(""), 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, s, d, 16.0, 0.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, s, d, 16.0, 1.5); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, s, d, 16.0, HUGE_VAL); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, s3, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, s32, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g2, s, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g16, s, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(g, empty, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(empty, s, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { amFilter(tiny_g, tiny_s, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }   // no small plane
        try { createAMFilter(16.0, 0.2)->filter(s, d); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }    // no joint
        try { createAMFilter(16.0, 0.2)->setUseRNG(true); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        for (int height : {0, -2, ADF_AM_MAX_TREE_HEIGHT + 1}) {
            Ptr<AdaptiveManifoldFilter> f = createAMFilter(16.0, 0.2);
            f->setTreeHeight(height);
            try { f->filter(s, d, g); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        }
        EXPECT(thrown == 17);
        try { amFilter(small, s, d, 16.0, 0.2); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 18);
        EXPECT(d.empty());
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
