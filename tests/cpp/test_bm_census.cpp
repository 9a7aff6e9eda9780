// The block matcher's census cost through the header-only C++ adaptor (include/adf_ximgproc.hpp) on host Mats:
// StereoBM's cost accessors, their way through createRightMatcher, and that the setters reach the library -- the
// adaptor's map against the map of the same settings straight through the C-ABI (built and run by
// tests/test_cpp_bm_census.py).
#include "adf_ximgproc.hpp"

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

// the same settings straight through the C-ABI, into a dense W x H map
static std::vector<int16_t> abi_map(const Mat& left, const Mat& right, int md, int nd, int bs, int uniq, int cost, int size)
{
    std::vector<int16_t> out((size_t)left.rows * left.cols, 12345);
    adf_bm_t* h = nullptr;
    EXPECT(adf_bm_create(&h, nd, bs) == ADF_OK);
    EXPECT(adf_bm_set_params(h, md, nd, bs, 31, 0, uniq) == ADF_OK);
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
    static_assert(ADF_BM_COST_SAD == 0 && ADF_BM_COST_CENSUS_DENSE == ADF_SGBM_COST_CENSUS_DENSE &&
                  ADF_BM_COST_CENSUS_SPARSE == ADF_SGBM_COST_CENSUS_SPARSE, "the two matchers share the census constants");
    // accessors, and their way into the right-view matcher
    Ptr<StereoBM> lm = StereoBM::create(16, 9);
    EXPECT(lm->getCostType() == ADF_BM_COST_SAD && lm->getCensusSize() == 7);
    EXPECT(createRightMatcher(lm)->getCostType() == ADF_BM_COST_SAD);
    lm->setCostType(ADF_BM_COST_CENSUS_SPARSE); lm->setCensusSize(9);
    Ptr<DisparityWLSFilter> wls = createDisparityWLSFilter(lm);                  // mutates the matcher, not its cost
    Ptr<StereoBM> rm = createRightMatcher(lm);
    EXPECT(lm->getCostType() == ADF_BM_COST_CENSUS_SPARSE && lm->getCensusSize() == 9 && lm->getUniquenessRatio() == 0);
    EXPECT(rm->getCostType() == ADF_BM_COST_CENSUS_SPARSE && rm->getCensusSize() == 9 && rm->getMinDisparity() == -15);

    // a pair shifted by 5 columns
    Mat base = random_image(40, 200, 3), left(40, 160, D8U, 1), right(40, 160, D8U, 1), dl, dr, dsad, out;
    for (int y = 0; y < 40; y++)
        for (int x = 0; x < 160; x++) { left.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 20]; right.ptr<uint8_t>(y)[x] = base.ptr<uint8_t>(y)[x + 25]; }
    lm->compute(left, right, dl);
    rm->compute(right, left, dr);
    EXPECT(same(dl, abi_map(left, right, 0, 16, 9, 0, ADF_BM_COST_CENSUS_SPARSE, 9)));
    EXPECT(same(dr, abi_map(right, left, -15, 16, 9, 0, ADF_BM_COST_CENSUS_SPARSE, 9)));
    int good_l = 0, good_r = 0;
    for (int y = 4; y < 36; y++)
        for (int x = 40; x < 120; x++) {                                        // (the sub-pixel fit moves a winner by -8 .. 8)
            good_l += std::abs(dl.ptr<int16_t>(y)[x] - 5 * 16) <= 8;
            good_r += std::abs(dr.ptr<int16_t>(y)[x] + 5 * 16) <= 8;
        }
    EXPECT(good_l > 32 * 80 * 9 / 10 && good_r > 32 * 80 * 9 / 10);
    wls->filter(dl, left, out, dr);
    EXPECT(out.rows == 40 && out.cols == 160 && mat_depth(out) == D16S);
    // the setters reach the library: another descriptor and SAD give other maps, each the C-ABI's
    lm->setCostType(ADF_BM_COST_CENSUS_DENSE); lm->setCensusSize(3);
    lm->compute(left, right, dsad);
    EXPECT(same(dsad, abi_map(left, right, 0, 16, 9, 0, ADF_BM_COST_CENSUS_DENSE, 3)));
    EXPECT(!same(dsad, abi_map(left, right, 0, 16, 9, 0, ADF_BM_COST_CENSUS_SPARSE, 9)));
    lm->setCostType(ADF_BM_COST_SAD);
    lm->compute(left, right, dsad);
    EXPECT(same(dsad, abi_map(left, right, 0, 16, 9, 0, ADF_BM_COST_SAD, 7)));
    // a pair the library does not have is refused when compute() pushes it
    int thrown = 0;
    lm->setCostType(ADF_BM_COST_CENSUS_DENSE); lm->setCensusSize(9);
    try { lm->compute(left, right, dl); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
    lm->setCostType(7); lm->setCensusSize(5);
    try { lm->compute(left, right, dl); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
    EXPECT(thrown == 2);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
