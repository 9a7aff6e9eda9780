// The census cost through the header-only C++ adaptor (include/adf_ximgproc.hpp) on host Mats: adf::censusTransform
// against a direct loop, StereoSGBM's cost accessors, their way through createRightMatcher, and one matched pair
// (built and run by tests/test_cpp_census.py).
#include "adf_ximgproc.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace adf;
using namespace adf::ximgproc;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static Mat random_image(int rows, int cols, unsigned seed)
{
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> v(0, 255);
    Mat m(rows, cols, D8U, 1);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) m.ptr<uint8_t>(y)[x] = (uint8_t)v(rng);
    return m;
}

// the definition in adf_wls.h, pixel by pixel
static uint64_t census_at(const Mat& m, int y, int x, int k, bool sparse)
{
    const int n2 = k / 2, step = sparse ? 2 : 1;
    uint64_t d = 0;
    for (int dy = -n2; dy <= n2; dy += step)
        for (int dx = -n2; dx <= n2; dx += step) {
            if (dy == 0 && dx == 0) continue;
            const int yy = std::min(std::max(y + dy, 0), m.rows - 1), xx = std::min(std::max(x + dx, 0), m.cols - 1);
            d = (d << 1) | (m.ptr<uint8_t>(yy)[xx] > m.ptr<uint8_t>(y)[x] ? 1u : 0u);
        }
    return d;
}

static bool transform_matches(const Mat& img, int k, int type)
{
    Mat dist;
    censusTransform(img, k, dist, type);
    if (dist.rows != img.rows || dist.cols != img.cols || mat_depth(dist) != D32S || mat_channels(dist) != 2) return false;
    for (int y = 0; y < img.rows; y++)
        for (int x = 0; x < img.cols; x++)
            if (dist.ptr<uint64_t>(y)[x] != census_at(img, y, x, k, type == ADF_SGBM_COST_CENSUS_SPARSE)) return false;
    return true;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    {   // hand-checked: 1..9 in a 3 x 3 image, dense 3 (centre, and a corner whose window is clamped)
        Mat img(3, 3, D8U, 1), dist;
        for (int i = 0; i < 9; i++) img.ptr<uint8_t>(i / 3)[i % 3] = (uint8_t)(i + 1);
        censusTransform(img, 3, dist, ADF_SGBM_COST_CENSUS_DENSE);
        EXPECT(dist.ptr<uint64_t>(1)[1] == 0x0F);
        EXPECT(dist.ptr<uint64_t>(0)[0] == 0x2F);
        EXPECT(dist.ptr<uint64_t>(2)[2] == 0);
    }
    Mat img = random_image(37, 211, 1);
    EXPECT(transform_matches(img, 7, ADF_SGBM_COST_CENSUS_DENSE));
    EXPECT(transform_matches(img, 9, ADF_SGBM_COST_CENSUS_SPARSE));
    EXPECT(transform_matches(random_image(2, 3, 2), 11, ADF_SGBM_COST_CENSUS_SPARSE));
    {   // refusals: a size the descriptor does not have, an unknown type, a CV_16S image, an empty one
        Mat s16(10, 10, D16S, 1), empty, dist;
        int thrown = 0;
        try { censusTransform(img, 9, dist, ADF_SGBM_COST_CENSUS_DENSE); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { censusTransform(img, 5, dist, 7); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { censusTransform(s16, 5, dist, ADF_SGBM_COST_CENSUS_DENSE); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { censusTransform(empty, 5, dist, ADF_SGBM_COST_CENSUS_DENSE); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 4);
    }
    // accessors, and their way into the right-view matcher (DF.cpp:432-445 copies P1, P2 and mode the same way)
    Ptr<StereoSGBM> lm = StereoSGBM::create(0, 32, 3);
    EXPECT(lm->getCostType() == ADF_SGBM_COST_BT);
    EXPECT(createRightMatcher(lm)->getCostType() == ADF_SGBM_COST_BT);
    lm->setCostType(ADF_SGBM_COST_CENSUS_SPARSE); lm->setCensusSize(9);
    lm->setP1(10); lm->setP2(100); lm->setMode(StereoSGBM::MODE_SGBM_3WAY);
    Ptr<DisparityWLSFilter> wls = createDisparityWLSFilter(lm);
    Ptr<StereoSGBM> rm = createRightMatcher(lm);
    EXPECT(rm->getCostType() == ADF_SGBM_COST_CENSUS_SPARSE && rm->getCensusSize() == 9);
    EXPECT(lm->getCostType() == ADF_SGBM_COST_CENSUS_SPARSE && lm->getCensusSize() == 9);
    EXPECT(rm->getMinDisparity() == -31 && rm->getP1() == 10 && rm->getP2() == 100);
    {   // a pair shifted by 5 columns: both views find it, and the filter takes the maps
        Mat base = random_image(40, 200, 3), left(40, 160, D8U, 1), right(40, 160, D8U, 1), dl, dr, out;
        for (int y = 0; y < 40; y++)
            for (int x = 0; x < 160; x++) { left.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 20]; right.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 25]; }
        lm->compute(left, right, dl);
        rm->compute(right, left, dr);
        int good_l = 0, good_r = 0;
        for (int y = 0; y < 40; y++)
            for (int x = 40; x < 120; x++) {                                    // (the sub-pixel fit moves a winner by -7 .. 8)
                good_l += std::abs(dl.ptr<int16_t>(y)[x] - 5 * 16) <= 8;
                good_r += std::abs(dr.ptr<int16_t>(y)[x] + 5 * 16) <= 8;
            }
        EXPECT(good_l > 40 * 80 * 9 / 10 && good_r > 40 * 80 * 9 / 10);
        wls->filter(dl, left, out, dr);
        EXPECT(out.rows == 40 && out.cols == 160 && mat_depth(out) == D16S);
        lm->setCensusSize(13);                                                  // checked when compute() pushes it
        int thrown = 0;
        try { lm->compute(left, right, dl); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        Mat c3(40, 160, D8U, 3);
        lm->setCensusSize(9);
        try { lm->compute(c3, c3, dl); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 2);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
