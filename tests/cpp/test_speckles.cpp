// adf::filterSpeckles (include/adf_ximgproc.hpp) on host Mats, checked bit for bit against the C restatement
// tests/speckle_ref.c (built and run by tests/test_cpp_speckles.py).
#include "adf_ximgproc.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

extern "C" void speckle_ref(int16_t* img, int W, int H, long stride, int new_val, int max_size, int max_diff, int* label,
                            int* list);

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static Mat random_map(int rows, int cols, unsigned seed)
{
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> lvl(0, 40), noise(-6, 6), pct(0, 99), blob(0, 1000);
    Mat m(rows, cols, D16S, 1);
    for (int y = 0; y < rows; y++) {
        int16_t* r = m.ptr<int16_t>(y);
        int v = 16 * lvl(rng);
        for (int x = 0; x < cols; x++) {
            if (x % 19 == 0) v = 16 * lvl(rng);
            const int p = pct(rng);
            r[x] = (int16_t)(p < 8 ? -16 : p < 10 ? blob(rng) : v + (y / 13) % 2 * 7 + noise(rng));
        }
    }
    return m;
}

static bool equal_to_reference(const Mat& in, const Mat& out, int nv, int ms, int md)
{
    std::vector<int16_t> ref((size_t)in.rows * in.cols);
    for (int y = 0; y < in.rows; y++) std::memcpy(&ref[(size_t)y * in.cols], in.ptr<int16_t>(y), (size_t)in.cols * 2);
    std::vector<int> label(ref.size()), list(ref.size());
    speckle_ref(ref.data(), in.cols, in.rows, in.cols, nv, ms, md, label.data(), list.data());
    for (int y = 0; y < out.rows; y++)
        if (std::memcmp(&ref[(size_t)y * in.cols], out.ptr<int16_t>(y), (size_t)in.cols * 2) != 0) return false;
    return true;
}

static Mat clone(const Mat& m)
{
    Mat c(m.rows, m.cols, D16S, 1);
    std::memcpy(c.data, m.data, m.step * (size_t)m.rows);
    return c;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int sizes[][2] = {{1, 1}, {1, 257}, {300, 1}, {37, 211}, {375, 1242}};
    unsigned seed = 1;
    for (auto& s : sizes)
        for (int ms : {0, 1, 100, 400})
            for (int md : {-1, 0, 16, 32}) {
                Mat in = random_map(s[0], s[1], seed++), img = clone(in);
                filterSpeckles(img, -16.0, ms, (double)md);
                EXPECT(equal_to_reference(in, img, -16, ms, md));
            }
    {   // doubles are rounded half-to-even: -16.5 -> -16, 16.5 -> 16, 17.5 -> 18
        Mat in = random_map(120, 170, 99), a = clone(in), b = clone(in);
        filterSpeckles(a, -16.5, 100, 16.5);
        EXPECT(equal_to_reference(in, a, -16, 100, 16));
        filterSpeckles(b, -15.5, 100, 17.5);
        EXPECT(equal_to_reference(in, b, -16, 100, 18));
    }
    {   // refusals: CV_8UC1, newVal outside CV_16S, empty
        Mat u8(10, 10, D8U, 1), s16 = random_map(10, 10, 5), empty;
        int thrown = 0;
        try { filterSpeckles(u8, 0.0, 10, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { filterSpeckles(s16, 40000.0, 10, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { filterSpeckles(s16, -32769.0, 10, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { filterSpeckles(empty, -16.0, 10, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 4);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
