// adf::resize / adf::cvtColor (include/adf_ximgproc.hpp) on host Mats, checked bit for bit against the small C
// restatement below (built and run by tests/test_cpp_view_prep.py).
#include "adf_ximgproc.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static int half_of(int n) { return n / 2 + (n & 1 & (n / 2)); }       // cvRound(n * 0.5), half to even

// mean over the n = 4, 2 or 1 source pixels of a cell
static int cell_mean(int s, int n)
{
    if (n == 4) return (s + 2) >> 2;
    if (n == 2) return s / 2 + (s & 1 & (s / 2));                      // cvRound(s / 2.0f)
    return s;
}

static std::vector<unsigned char> shrink_ref(const Mat& m, int cn)
{
    const int w = half_of(m.cols), h = half_of(m.rows);
    std::vector<unsigned char> out((size_t)w * h * cn);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int k = 0; k < cn; k++) {
                int s = 0, n = 0;
                for (int dy = 0; dy < 2; dy++)
                    for (int dx = 0; dx < 2; dx++)
                        if (2 * y + dy < m.rows && 2 * x + dx < m.cols) {
                            s += m.ptr<unsigned char>(2 * y + dy)[(2 * x + dx) * cn + k];
                            n++;
                        }
                out[((size_t)y * w + x) * cn + k] = (unsigned char)cell_mean(s, n);
            }
    return out;
}

static std::vector<unsigned char> gray_ref(const unsigned char* bgr, size_t pixels)
{
    std::vector<unsigned char> out(pixels);
    for (size_t i = 0; i < pixels; i++)
        out[i] = (unsigned char)((bgr[3 * i] * 1868 + bgr[3 * i + 1] * 9617 + bgr[3 * i + 2] * 4899 + 8192) >> 14);
    return out;
}

static Mat random_image(int rows, int cols, int cn, unsigned seed)
{
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> v(0, 255);
    Mat m(rows, cols, D8U, cn);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols * cn; x++) m.ptr<unsigned char>(y)[x] = (unsigned char)v(rng);
    return m;
}

static bool equal(const Mat& m, const std::vector<unsigned char>& ref, int rows, int cols, int cn)
{
    if (m.rows != rows || m.cols != cols || mat_channels(m) != cn || mat_depth(m) != D8U) return false;
    for (int y = 0; y < rows; y++)
        if (std::memcmp(m.ptr<unsigned char>(y), &ref[(size_t)y * cols * cn], (size_t)cols * cn) != 0) return false;
    return true;
}

static std::vector<unsigned char> dense(const Mat& m)
{
    const size_t row = (size_t)m.cols * mat_channels(m);
    std::vector<unsigned char> out(row * m.rows);
    for (int y = 0; y < m.rows; y++) std::memcpy(&out[row * y], m.ptr<unsigned char>(y), row);
    return out;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int sizes[][2] = {{2, 2}, {3, 3}, {2, 5}, {5, 17}, {64, 64}, {7, 1023}, {436, 1024}, {375, 1242}};   // rows, cols
    unsigned seed = 1;
    for (auto& s : sizes) {
        const int h = half_of(s[0]), w = half_of(s[1]);
        for (int cn : {1, 3}) {
            Mat in = random_image(s[0], s[1], cn, seed++), out;
            resize(in, out, Size(), 0.5, 0.5);
            EXPECT(equal(out, shrink_ref(in, cn), h, w, cn));
            Mat out2;
            resize(in, out2, Size(w, h));                                  // the same through dsize
            EXPECT(equal(out2, shrink_ref(in, cn), h, w, cn));
        }
        Mat bgr = random_image(s[0], s[1], 3, seed++), g;
        cvtColor(bgr, g, COLOR_BGR2GRAY);
        EXPECT(equal(g, gray_ref(dense(bgr).data(), (size_t)s[0] * s[1]), s[0], s[1], 1));
        // the sample's two lines, in place (samples/disparity_filtering.cpp:137, 155)
        Mat v = bgr;
        resize(v, v, Size(), 0.5, 0.5);
        EXPECT(equal(v, shrink_ref(bgr, 3), h, w, 3));
        const std::vector<unsigned char> half_bgr = dense(v);
        cvtColor(v, v, COLOR_BGR2GRAY);
        EXPECT(equal(v, gray_ref(half_bgr.data(), (size_t)h * w), h, w, 1));
    }
    {   // refusals
        Mat bgr = random_image(8, 8, 3, 77), gray = random_image(8, 8, 1, 78), s16(8, 8, D16S, 1), empty, out;
        int thrown = 0;
        try { resize(bgr, out, Size(), 0.25, 0.25); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { resize(bgr, out, Size(), 0.5, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { resize(bgr, out, Size(3, 4)); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { resize(bgr, out, Size(), 0.5, 0.5, 0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { resize(s16, out, Size(), 0.5, 0.5); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { resize(empty, out, Size(), 0.5, 0.5); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { cvtColor(bgr, out, 7); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { cvtColor(gray, out, COLOR_BGR2GRAY); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { cvtColor(bgr, out, COLOR_BGR2GRAY, 3); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 9);
        EXPECT(out.empty());
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
