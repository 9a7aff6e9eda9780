// adf::reprojectImageTo3D / adf::pointCloud through the header-only C++ adaptor (include/adf_ximgproc.hpp) on host Mats,
// against a direct loop over the definition in adf_wls.h (built and run by tests/test_cpp_reproject.py; compiled with
// -ffp-contract=off so that the loop's products and sums round separately, like the library's).
#include "adf_ximgproc.hpp"

#include <cfloat>
#include <cstdio>
#include <cstring>
#include <random>

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static const double QD[16] = {0.7, -0.013, 0.31, -301.3, 0.017, 1.1, -0.23, 177.7, 0.0031, -0.0007, 0.9, 517.1, 0.00011, 0.00013, 0.37, 1.9};

static bool same(float a, float b)
{
    if (a != a || b != b) return a != a && b != b;                              // NaN: position only
    return std::memcmp(&a, &b, 4) == 0;
}

// the definition, one pixel
static void point_at(const double* Q, int x, int y, double s, double scale, float* xyz)
{
    const double d = s * scale;
    double r[4];
    for (int i = 0; i < 4; i++) r[i] = ((Q[4 * i] * x + Q[4 * i + 1] * y) + Q[4 * i + 3]) + Q[4 * i + 2] * d;
    const double iw = 1.0 / r[3];
    for (int i = 0; i < 3; i++) xyz[i] = (float)(r[i] * iw);
}

template <class T> static double raw(const Mat& m, int y, int x) { return (double)m.ptr<T>(y)[x]; }

static Mat q_mat(int depth)
{
    Mat Q(4, 4, depth, 1);
    for (int i = 0; i < 16; i++) {
        if (depth == D64F) Q.ptr<double>(i / 4)[i % 4] = QD[i];
        else Q.ptr<float>(i / 4)[i % 4] = (float)QD[i];
    }
    return Q;
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int rows = 37, cols = 211;
    std::mt19937 rng(7);
    std::uniform_int_distribution<int> v(1, 3000);
    Mat d16(rows, cols, D16S, 1), d32(rows, cols, D32F, 1), view(rows, cols, D8U, 3);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            const int s = (x + y) % 5 == 0 ? -16 : v(rng);
            d16.ptr<int16_t>(y)[x] = (int16_t)s;
            d32.ptr<float>(y)[x] = s < 0 ? -16.0f : (float)s * 0.37f;
            for (int c = 0; c < 3; c++) view.ptr<uint8_t>(y)[3 * x + c] = (uint8_t)(v(rng) & 255);
        }
    d16.ptr<int16_t>(3)[7] = 0;
    double Q32[16];
    for (int i = 0; i < 16; i++) Q32[i] = (double)(float)QD[i];
    {   // cv's call: XYZ, Q as CV_64F and as CV_32F, missing values at the map's minimum (-16)
        for (int pass = 0; pass < 2; pass++) {
            Mat xyz;
            reprojectImageTo3D(d16, xyz, q_mat(pass ? D32F : D64F), true);
            EXPECT(xyz.rows == rows && xyz.cols == cols && mat_depth(xyz) == D32F && mat_channels(xyz) == 3);
            int bad = 0;
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < cols; x++) {
                    float e[3];
                    point_at(pass ? Q32 : QD, x, y, raw<int16_t>(d16, y, x), 1.0, e);
                    if (d16.ptr<int16_t>(y)[x] == -16) e[2] = 10000.0f;
                    const float* g = xyz.ptr<float>(y) + 3 * x;
                    bad += !(same(g[0], e[0]) && same(g[1], e[1]) && same(g[2], e[2]));
                }
            EXPECT(bad == 0);
        }
    }
    const double fill = -16.0;
    {   // the extensions: a float map in 1/16 units, a named missing value, the Z plane alone
        Mat z;
        reprojectImageTo3D(d32, z, q_mat(D64F), false, D32F, 1.0 / 16, &fill, true);
        EXPECT(mat_channels(z) == 1 && mat_depth(z) == D32F);
        int bad = 0;
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) {
                float e[3];
                point_at(QD, x, y, raw<float>(d32, y, x), 1.0 / 16, e);
                if (d32.ptr<float>(y)[x] == -16.0f) e[2] = 10000.0f;
                bad += !same(z.ptr<float>(y)[x], e[2]);
            }
        EXPECT(bad == 0);
    }
    {   // the point list: ROI, z range, colours, index
        std::vector<float> pts;
        std::vector<uint8_t> col;
        std::vector<int32_t> idx;
        const Rect roi(3, 5, 101, 17);
        const double z0 = 3.0, z1 = 5.0;
        const size_t n = pointCloud(d16, q_mat(D64F), pts, &col, view, roi, z0, z1, false, 1.0, &fill, &idx);
        EXPECT(pts.size() == 3 * n && col.size() == 3 * n && idx.size() == n);
        size_t k = 0;
        int bad = 0;
        for (int y = roi.y; y < roi.y + roi.height; y++)
            for (int x = roi.x; x < roi.x + roi.width; x++) {
                float e[3];
                point_at(QD, x, y, raw<int16_t>(d16, y, x), 1.0, e);
                if (d16.ptr<int16_t>(y)[x] == -16 || !std::isfinite(e[0]) || !std::isfinite(e[1]) || !std::isfinite(e[2])) continue;
                if (!(z0 <= (double)e[2] && (double)e[2] <= z1)) continue;
                if (k < n)
                    bad += !(same(pts[3 * k], e[0]) && same(pts[3 * k + 1], e[1]) && same(pts[3 * k + 2], e[2]) && idx[k] == y * cols + x &&
                             std::memcmp(&col[3 * k], view.ptr<uint8_t>(y) + 3 * x, 3) == 0);
                k++;
            }
        EXPECT(k == n && bad == 0 && n > 0 && n < (size_t)roi.width * roi.height);
        std::vector<float> all;
        const size_t m = pointCloud(d16, q_mat(D64F), all, nullptr, Mat(), Rect(), -HUGE_VAL, HUGE_VAL, true);
        size_t expect = 0;
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) expect += d16.ptr<int16_t>(y)[x] != -16;
        EXPECT(m == expect && all.size() == 3 * m);
    }
    {   // refusals
        Mat u8(4, 4, D8U, 1), q3(3, 4, D64F, 1), xyz;
        std::vector<float> pts;
        int thrown = 0;
        try { reprojectImageTo3D(u8, xyz, q_mat(D64F)); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { reprojectImageTo3D(d16, xyz, q3); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { reprojectImageTo3D(d16, xyz, q_mat(D64F), false, D16S); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { pointCloud(d16, q_mat(D64F), pts, nullptr, Mat(), Rect(200, 0, 20, 5)); } catch (const Exception& e) { thrown += e.code == ADF_ESIZE; }
        try { pointCloud(d16, q_mat(D64F), pts, nullptr, Mat(), Rect(), NAN, 1.0); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 5);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
