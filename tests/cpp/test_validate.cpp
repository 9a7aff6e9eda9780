// adf::validateDisparity and StereoBM::computeWithCost (include/adf_ximgproc.hpp) on host Mats, checked bit for bit against
// a sequential restatement of the definition in include/adf_wls.h (built and run by tests/test_cpp_validate.py).
#include "adf_ximgproc.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace adf;
using adf::ximgproc::StereoBM;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// The statement, one row at a time; COST is int16_t or int32_t.
template <class COST>
static void validate_ref(Mat& disp, const Mat& cost, int minD, int nd, int maxdiff)
{
    const int W = disp.cols, maxD = minD + nd, INV = (minD - 1) * 16;
    const int X0 = maxD > 0 ? maxD : 0, X1 = W + (minD < 0 ? minD : 0);
    std::vector<int> disp2(W), cost2(W);
    for (int y = 0; y < disp.rows; y++) {
        int16_t* d = disp.ptr<int16_t>(y);
        const COST* c = cost.ptr<COST>(y);
        for (int x = 0; x < W; x++) { disp2[x] = INV; cost2[x] = INT_MAX; }
        for (int x = X0; x < X1; x++) {
            if (d[x] == INV) continue;
            const int x2 = x - ((d[x] + 8) >> 4);
            if (x2 < 0 || x2 >= W) continue;                             // the documented deviation: no vote
            if (cost2[x2] > (int)c[x]) { cost2[x2] = (int)c[x]; disp2[x2] = d[x]; }
        }
        for (int x = X0; x < X1; x++) {
            const int v = d[x];
            if (v == INV) continue;
            const int xa = x - (v >> 4), xb = x - ((v + 15) >> 4);
            const bool a = xa >= 0 && xa < W && disp2[xa] > INV && std::abs(disp2[xa] - v) > 16 * maxdiff;
            const bool b = xb >= 0 && xb < W && disp2[xb] > INV && std::abs(disp2[xb] - v) > 16 * maxdiff;
            if (a && b) d[x] = (int16_t)INV;
        }
    }
}

static Mat clone(const Mat& m)
{
    Mat c(m.rows, m.cols, m.depth_, 1);
    std::memcpy(c.data, m.data, m.step * (size_t)m.rows);
    return c;
}

static bool equal(const Mat& a, const Mat& b)
{
    if (a.rows != b.rows || a.cols != b.cols || a.depth_ != b.depth_) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr<unsigned char>(y), b.ptr<unsigned char>(y), (size_t)a.cols * Mat::esz(a.depth_)) != 0) return false;
    return true;
}

static void random_case(int rows, int cols, int minD, int nd, int cost_depth, unsigned seed, Mat& disp, Mat& cost)
{
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> lvl(minD * 16, (minD + nd - 1) * 16), pct(0, 99), c16(-300, 2000), c32(-100000, 3000000);
    disp = Mat(rows, cols, D16S, 1);
    cost = Mat(rows, cols, cost_depth, 1);
    for (int y = 0; y < rows; y++) {
        int v = lvl(rng);
        for (int x = 0; x < cols; x++) {
            if (x % 11 == 0) v = lvl(rng);
            const int p = pct(rng);
            disp.ptr<int16_t>(y)[x] = (int16_t)(p < 25 ? (minD - 1) * 16 : p < 60 ? lvl(rng) : v);
            const int q = pct(rng);
            if (cost_depth == D16S) cost.ptr<int16_t>(y)[x] = (int16_t)(q < 3 ? -32768 : q < 6 ? 32767 : c16(rng));
            else cost.ptr<int32_t>(y)[x] = q < 3 ? INT_MAX : q < 6 ? INT_MIN : c32(rng);
        }
    }
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int sizes[][2] = {{1, 1}, {1, 257}, {9, 65}, {37, 211}, {3, 1000}};
    unsigned seed = 1;
    int changed = 0;
    for (auto& s : sizes)
        for (int depth : {(int)D16S, (int)D32S})
            for (int minD : {0, -8, 5})
                for (int maxdiff : {0, 1, 1000000}) {
                    Mat disp, cost;
                    random_case(s[0], s[1], minD, 32, depth, seed++, disp, cost);
                    Mat exp = clone(disp), in = clone(disp);
                    if (depth == D16S) validate_ref<int16_t>(exp, cost, minD, 32, maxdiff);
                    else validate_ref<int32_t>(exp, cost, minD, 32, maxdiff);
                    validateDisparity(disp, cost, minD, 32, maxdiff);
                    EXPECT(equal(disp, exp));
                    changed += !equal(exp, in);
                }
    EXPECT(changed > 20);                                                // the cases are not vacuous
    {   // the matcher's own pair: computeWithCost's map is compute()'s, filtered pixels cost 0, and the chain runs
        std::mt19937 rng(7);
        std::uniform_int_distribution<int> px(0, 255);
        const int H = 40, W = 200, shift = 6;
        Mat base(H, W + 32, D8U, 1), left(H, W, D8U, 1), right(H, W, D8U, 1);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W + 32; x++) base.ptr<uint8_t>(y)[x] = (uint8_t)px(rng);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                left.ptr<uint8_t>(y)[x] = (uint8_t)((base.ptr<uint8_t>(y)[x + 8] + base.ptr<uint8_t>(y)[x + 9]) / 2);
                right.ptr<uint8_t>(y)[x] = (uint8_t)((base.ptr<uint8_t>(y)[x + 8 + shift] + base.ptr<uint8_t>(y)[x + 9 + shift]) / 2);
            }
        Ptr<StereoBM> bm = StereoBM::create(16, 9);
        Mat plain, disp, cost;
        bm->compute(left, right, plain);
        bm->setDisp12MaxDiff(1);                                         // refused by compute(), not looked at by computeWithCost
        bm->computeWithCost(left, right, disp, cost);
        EXPECT(equal(disp, plain));
        EXPECT(mat_depth(cost) == D16S && cost.rows == H && cost.cols == W);
        int kept = 0, bad = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const bool filtered = disp.ptr<int16_t>(y)[x] == -16;
                kept += !filtered;
                bad += filtered ? cost.ptr<int16_t>(y)[x] != 0 : cost.ptr<int16_t>(y)[x] < 0;
            }
        EXPECT(kept > 1000 && bad == 0);
        Mat exp = clone(disp);
        validate_ref<int16_t>(exp, cost, 0, 16, 1);
        validateDisparity(disp, cost, 0, 16);                            // disp12MaxDiff defaults to 1
        EXPECT(equal(disp, exp));
        int thrown = 0;
        try { bm->compute(left, right, plain); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 1);
    }
    {   // refusals
        Mat d(10, 40, D16S, 1), c16(10, 40, D16S, 1), c32(10, 40, D32S, 1), u8(10, 40, D8U, 1), f32(10, 40, D32F, 1), small(10, 39, D16S, 1), empty;
        int thrown = 0;
        try { validateDisparity(d, c16, 0, 16, -1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, c32, 0, 16, (1 << 26) + 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, c16, 0, 0, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, c16, 2049, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, c16, -2048, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, u8, 0, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, f32, 0, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(u8, c16, 0, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(empty, c16, 0, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { validateDisparity(d, small, 0, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 10);
        Mat wide(1, ADF_VALIDATE_MAX_WIDTH + 1, D16S, 1), wide_cost(1, ADF_VALIDATE_MAX_WIDTH + 1, D16S, 1);
        try { validateDisparity(wide, wide_cost, 0, 16, 1); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        EXPECT(thrown == 11);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
