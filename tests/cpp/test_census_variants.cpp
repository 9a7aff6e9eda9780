// The modified and the centre-symmetric census through the header-only C++ adaptor (include/adf_ximgproc.hpp) on host
// Mats: adf::censusTransform with ADF_SGBM_COST_CENSUS_CS, 5 against a direct loop, and a StereoBM with
// ADF_BM_COST_MCT_DENSE, 3 against the same settings straight through the C-ABI (built and run by
// tests/test_cpp_census_variants.py).
#include "adf_ximgproc.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

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

static int pixel(const Mat& m, int y, int x)
{
    return m.ptr<uint8_t>(std::min(std::max(y, 0), m.rows - 1))[std::min(std::max(x, 0), m.cols - 1)];
}

// the definitions in adf_wls.h, pixel by pixel
static uint64_t cs_at(const Mat& m, int y, int x, int k)
{
    const int n2 = k / 2;
    uint64_t d = 0;
    for (int dy = -n2; dy <= 0; dy++)
        for (int dx = -n2; dx <= n2; dx++) {
            if (dy == 0 && dx >= 0) break;
            d = (d << 1) | (pixel(m, y + dy, x + dx) > pixel(m, y - dy, x - dx) ? 1u : 0u);
        }
    return d;
}

static uint64_t mct_dense_at(const Mat& m, int y, int x, int k)
{
    const int n2 = k / 2;
    int sum = 0;
    for (int dy = -n2; dy <= n2; dy++)
        for (int dx = -n2; dx <= n2; dx++) sum += pixel(m, y + dy, x + dx);
    uint64_t d = 0;
    for (int dy = -n2; dy <= n2; dy++)
        for (int dx = -n2; dx <= n2; dx++) {
            if (dy == 0 && dx == 0) continue;
            d = (d << 1) | (k * k * pixel(m, y + dy, x + dx) > sum ? 1u : 0u);
        }
    return d;
}

template <class At>
static bool transform_matches(const Mat& img, int k, int type, At at)
{
    Mat dist;
    censusTransform(img, k, dist, type);
    if (dist.rows != img.rows || dist.cols != img.cols || mat_depth(dist) != D32S || mat_channels(dist) != 2) return false;
    for (int y = 0; y < img.rows; y++)
        for (int x = 0; x < img.cols; x++)
            if (dist.ptr<uint64_t>(y)[x] != at(img, y, x, k)) return false;
    return true;
}

// the same settings straight through the C-ABI, into a dense W x H map
static std::vector<int16_t> abi_map(const Mat& left, const Mat& right, int nd, int bs, int cost, int size)
{
    std::vector<int16_t> out((size_t)left.rows * left.cols, 12345);
    adf_bm_t* h = nullptr;
    EXPECT(adf_bm_create(&h, nd, bs) == ADF_OK);
    EXPECT(adf_bm_set_params(h, 0, nd, bs, 31, 0, 0) == ADF_OK);
    EXPECT(adf_bm_set_cost(h, cost, size) == ADF_OK);
    EXPECT(adf_bm_compute_host(h, 1, left.data, mat_step(left), 0, right.data, mat_step(right), 0, left.cols, left.rows,
                               out.data(), (ptrdiff_t)left.cols * 2, 0) == ADF_OK);
    adf_bm_destroy(h);
    return out;
}

static bool same(const Mat& m, const std::vector<int16_t>& v)
{
    if (mat_depth(m) != D16S || (size_t)m.rows * m.cols != v.size()) return false;
    for (int y = 0; y < m.rows; y++)
        if (std::memcmp(m.ptr<int16_t>(y), v.data() + (size_t)y * m.cols, (size_t)m.cols * 2) != 0) return false;
    return true;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    static_assert(ADF_SGBM_COST_MCT_DENSE == 4 && ADF_SGBM_COST_MCT_SPARSE == 5 && ADF_SGBM_COST_CENSUS_CS == 6, "adf_wls.h");
    static_assert(ADF_BM_COST_MCT_DENSE == 4 && ADF_BM_COST_MCT_SPARSE == 5 && ADF_BM_COST_CENSUS_CS == 6, "adf_wls.h");
    {   // hand-checked: one bright pixel, centre-symmetric 3 -- only the pixels that see it in the first half set a bit
        Mat img(5, 5, D8U, 1), dist;
        for (int i = 0; i < 25; i++) img.ptr<uint8_t>(i / 5)[i % 5] = 0;
        img.ptr<uint8_t>(2)[2] = 200;
        censusTransform(img, 3, dist, ADF_SGBM_COST_CENSUS_CS);
        EXPECT(dist.ptr<uint64_t>(3)[3] == 8 && dist.ptr<uint64_t>(3)[2] == 4 && dist.ptr<uint64_t>(3)[1] == 2 && dist.ptr<uint64_t>(2)[3] == 1);
        EXPECT(dist.ptr<uint64_t>(2)[2] == 0 && dist.ptr<uint64_t>(1)[1] == 0);
    }
    Mat img = random_image(37, 211, 1);
    EXPECT(transform_matches(img, 5, ADF_SGBM_COST_CENSUS_CS, cs_at));
    EXPECT(transform_matches(random_image(2, 3, 2), 5, ADF_SGBM_COST_CENSUS_CS, cs_at));
    EXPECT(transform_matches(img, 3, ADF_SGBM_COST_MCT_DENSE, mct_dense_at));
    {   // refusals: 60 bits, a size the modified census does not have
        Mat dist;
        int thrown = 0;
        try { censusTransform(img, 11, dist, ADF_SGBM_COST_CENSUS_CS); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { censusTransform(img, 9, dist, ADF_SGBM_COST_MCT_DENSE); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 2);
    }
    // a block matcher with the modified census, dense 3: a pair shifted by 5 columns
    Ptr<StereoBM> lm = StereoBM::create(16, 9);
    lm->setCostType(ADF_BM_COST_MCT_DENSE); lm->setCensusSize(3);
    Ptr<DisparityWLSFilter> wls = createDisparityWLSFilter(lm);                  // mutates the matcher, not its cost
    Ptr<StereoBM> rm = createRightMatcher(lm);
    EXPECT(lm->getCostType() == ADF_BM_COST_MCT_DENSE && lm->getCensusSize() == 3);
    EXPECT(rm->getCostType() == ADF_BM_COST_MCT_DENSE && rm->getCensusSize() == 3 && rm->getMinDisparity() == -15);
    Mat base = random_image(40, 200, 3), left(40, 160, D8U, 1), right(40, 160, D8U, 1), dl, other;
    for (int y = 0; y < 40; y++)
        for (int x = 0; x < 160; x++) { left.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 20]; right.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 25]; }
    lm->compute(left, right, dl);
    EXPECT(same(dl, abi_map(left, right, 16, 9, ADF_BM_COST_MCT_DENSE, 3)));
    EXPECT(!same(dl, abi_map(left, right, 16, 9, ADF_BM_COST_CENSUS_DENSE, 3)));  // the setter reached the library
    int good = 0;
    for (int y = 4; y < 36; y++)
        for (int x = 40; x < 120; x++) good += std::abs(dl.ptr<int16_t>(y)[x] - 5 * 16) <= 8;   // (the sub-pixel fit moves a winner by -8 .. 8)
    EXPECT(good > 32 * 80 * 9 / 10);
    lm->setCostType(ADF_BM_COST_CENSUS_CS); lm->setCensusSize(11);              // refused when compute() pushes it
    int thrown = 0;
    try { lm->compute(left, right, other); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
    EXPECT(thrown == 1);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
