// adf::initUndistortRectifyMap / adf::remap / adf::rectifyViews through the header-only C++ adaptor
// (include/adf_ximgproc.hpp) on host Mats, against a direct loop over the definition in adf_wls.h (built and run by
// tests/test_cpp_rectify.py; compiled with -ffp-contract=off so that the loop's products and sums round separately, like
// the library's).  `--host-only` runs the part that needs no device -- the parameter inverse and every refusal -- and is
// what a sanitizer build of this program runs.
#include "adf_ximgproc.hpp"

#include <cstdio>
#include <cstring>
#include <random>

using namespace adf;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static const double KD[9] = {984.2439, 0.0, 105.3, 0.0, 980.8141, 18.2, 0.0, 0.0, 1.0};
static const double DD[8] = {-0.37, 0.2, 1e-3, -2e-4, -0.07, 0.01, -0.03, 0.002};
static const double RD[9] = {0.999972584682756, -0.005263306999564445, -0.005208404968566129,
                             0.005235892058122896, 0.9999724411371465, -0.005263306999564445,
                             0.00523596383141958, 0.005235892058122896, 0.999972584682756};      // 0.3 degrees about each axis
static const double PD[12] = {721.5377, 0.0, 104.6, 44.85728, 0.0, 721.5377, 17.9, 0.2163791, 0.0, 0.0, 1.0, 0.002745884};

static bool same(float a, float b)
{
    if (a != a || b != b) return a != a && b != b;                              // NaN: position only
    return std::memcmp(&a, &b, 4) == 0;
}

static Mat mat64(int rows, int cols, const double* v)
{
    Mat m(rows, cols, D64F, 1);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.ptr<double>(r)[c] = v[r * cols + c];
    return m;
}

// the definition: the inverse ...
static void inverse_of(const double* P, int p_cols, const double* R, double* ir)
{
    double a[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) a[i][j] = R ? (P[i * p_cols] * R[j] + P[i * p_cols + 1] * R[3 + j]) + P[i * p_cols + 2] * R[6 + j] : P[i * p_cols + j];
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double c10 = a[0][2] * a[2][1] - a[0][1] * a[2][2], c11 = a[0][0] * a[2][2] - a[0][2] * a[2][0], c12 = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    const double c20 = a[0][1] * a[1][2] - a[0][2] * a[1][1], c21 = a[0][2] * a[1][0] - a[0][0] * a[1][2], c22 = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = (a[0][0] * c00 + a[0][1] * c01) + a[0][2] * c02;
    const double adj[9] = {c00, c10, c20, c01, c11, c21, c02, c12, c22};
    for (int i = 0; i < 9; i++) ir[i] = adj[i] / det;
}

// ... the coordinates of one destination pixel ...
static void map_at(const double* K, const double* d, const double* ir, int ui, int vi, float* mx, float* my)
{
    const double u = ui, v = vi;
    const double X = (ir[0] * u + ir[1] * v) + ir[2], Y = (ir[3] * u + ir[4] * v) + ir[5], D = (ir[6] * u + ir[7] * v) + ir[8];
    const double w = 1.0 / D, x = X * w, y = Y * w;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
    const double kr = (1.0 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2) / (1.0 + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2);
    const double xd = (x * kr + d[2] * xy2) + d[3] * (r2 + 2.0 * x2);
    const double yd = (y * kr + d[2] * (r2 + 2.0 * y2)) + d[3] * xy2;
    *mx = (float)(K[0] * xd + K[2]);
    *my = (float)(K[4] * yd + K[5]);
}

// ... and one sample
static int sample_at(const Mat& src, int c, float mx, float my, int border)
{
    const float tx = mx * 32.0f, ty = my * 32.0f;
    if (!(tx >= -1048576.0f && tx <= 1048575.0f && ty >= -1048576.0f && ty <= 1048575.0f)) return border;
    const int sx = (int)std::nearbyint(tx), sy = (int)std::nearbyint(ty);       // default rounding mode: half to even
    const int ix = sx >> 5, ax = sx & 31, iy = sy >> 5, ay = sy & 31, cn = mat_channels(src);
    auto tap = [&](int i, int j) { return i >= 0 && i < src.cols && j >= 0 && j < src.rows ? (int)src.ptr<uint8_t>(j)[i * cn + c] : border; };
    return (tap(ix, iy) * (32 - ax) * (32 - ay) + tap(ix + 1, iy) * ax * (32 - ay) + tap(ix, iy + 1) * (32 - ax) * ay +
            tap(ix + 1, iy + 1) * ax * ay + 512) >> 10;
}

template <class F> static int code_of(F f)
{
    try { f(); } catch (const Exception& e) { return e.code; }
    return ADF_OK;
}

static void host_only()
{
    {   // the inverse: the adaptor, the C entry and the definition give the same bits
        double ir[9];
        inverse_of(PD, 4, RD, ir);
        const adf_rectify_params a = rectify_params("test", mat64(3, 3, KD), mat64(1, 5, DD), mat64(3, 3, RD), mat64(3, 4, PD));
        adf_rectify_params b;
        EXPECT(adf_rectify_params_init(KD, DD, 5, RD, PD, 4, &b) == ADF_OK);
        EXPECT(std::memcmp(&a, &b, sizeof a) == 0 && std::memcmp(a.ir, ir, sizeof ir) == 0);
        EXPECT(a.fx == KD[0] && a.fy == KD[4] && a.cx == KD[2] && a.cy == KD[5] && a.dist[4] == DD[4] && a.dist[5] == 0.0);
        // empty R and newCameraMatrix: the identity and cameraMatrix; a column of coefficients
        inverse_of(KD, 3, nullptr, ir);
        const adf_rectify_params c = rectify_params("test", mat64(3, 3, KD), mat64(8, 1, DD), Mat(), Mat());
        EXPECT(std::memcmp(c.ir, ir, sizeof ir) == 0 && c.dist[7] == DD[7]);
        double prod[9];                                                         // sanity: ir * A = I within 1e-9
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) prod[3 * i + j] = ir[3 * i] * KD[j] + ir[3 * i + 1] * KD[3 + j] + ir[3 * i + 2] * KD[6 + j];
        for (int i = 0; i < 9; i++) EXPECT(std::fabs(prod[i] - (i % 4 == 0 ? 1.0 : 0.0)) < 1e-9);
    }
    {   // refusals: none of them reaches a device
        adf_rectify_params p;
        const double ones[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1}, twelve[12] = {};
        EXPECT(adf_rectify_params_init(KD, twelve, 12, nullptr, KD, 3, &p) == ADF_EBADARG);
        EXPECT(adf_rectify_params_init(KD, twelve, 14, nullptr, KD, 3, &p) == ADF_EBADARG);
        EXPECT(adf_rectify_params_init(KD, nullptr, 0, nullptr, ones, 3, &p) == ADF_EBADARG);
        EXPECT(adf_rectify_params_init(KD, nullptr, 0, nullptr, PD, 5, &p) == ADF_EBADARG);
        Mat K = mat64(3, 3, KD), none, src(6, 10, D8U, 3), dst, m1(4, 8, D32F, 1), m2(4, 8, D32F, 1), m3(4, 7, D32F, 1), k32(3, 3, D32F, 1);
        std::memset(src.data, 0, src.step * 6);
        EXPECT(code_of([&] { initUndistortRectifyMap(K, none, none, K, Size(8, 4), 11 /* CV_16SC2 */, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { initUndistortRectifyMap(K, mat64(1, 12, twelve), none, K, Size(8, 4), M32FC1, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { initUndistortRectifyMap(k32, none, none, K, Size(8, 4), M32FC1, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { initUndistortRectifyMap(K, none, mat64(3, 4, PD), K, Size(8, 4), M32FC1, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { initUndistortRectifyMap(K, none, none, mat64(3, 3, ones), Size(8, 4), M32FC1, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { initUndistortRectifyMap(K, none, none, K, Size(0, 4), M32FC1, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { remap(src, dst, m1, m3); }) == ADF_EBADARG);
        EXPECT(code_of([&] { remap(src, dst, m1, m2, 0 /* INTER_NEAREST */); }) == ADF_EBADARG);
        EXPECT(code_of([&] { remap(src, dst, m1, m2, INTER_LINEAR, 1 /* BORDER_REPLICATE */); }) == ADF_EBADARG);
        EXPECT(code_of([&] { remap(src, dst, m1, m2, INTER_LINEAR, BORDER_CONSTANT, Scalar(256)); }) == ADF_EBADARG);
        EXPECT(code_of([&] { remap(m1, dst, m1, m2); }) == ADF_EBADARG);
        EXPECT(code_of([&] { rectifyViews(src, dst, K, mat64(1, 14, twelve), none, none, Size()); }) == ADF_EBADARG);
        EXPECT(code_of([&] { rectifyViews(none, dst, K, none, none, none, Size()); }) == ADF_EBADARG);
        EXPECT(code_of([&] { rectifyViews(src, dst, K, none, none, none, Size(-1, 4)); }) == ADF_EBADARG);
    }
}

static void on_device()
{
    const int rows = 37, cols = 211, H = 24, W = 201;
    std::mt19937 rng(7);
    std::uniform_int_distribution<int> v(0, 255);
    Mat bgr(rows, cols, D8U, 3), gray(rows, cols, D8U, 1);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            gray.ptr<uint8_t>(y)[x] = (uint8_t)v(rng);
            for (int c = 0; c < 3; c++) bgr.ptr<uint8_t>(y)[3 * x + c] = (uint8_t)v(rng);
        }
    const Mat K = mat64(3, 3, KD), D5 = mat64(1, 5, DD), D8 = mat64(1, 8, DD), R = mat64(3, 3, RD), P = mat64(3, 4, PD);
    double ir[9];
    inverse_of(PD, 4, RD, ir);
    const double d5[8] = {DD[0], DD[1], DD[2], DD[3], DD[4], 0, 0, 0};
    for (int pass = 0; pass < 2; pass++) {
        const double* d = pass ? DD : d5;
        Mat map1, map2;
        initUndistortRectifyMap(K, pass ? D8 : D5, R, P, Size(W, H), M32FC1, map1, map2);
        EXPECT(map1.rows == H && map1.cols == W && mat_depth(map1) == D32F && mat_channels(map2) == 1);
        int bad = 0, inside = 0;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                float ex, ey;
                map_at(KD, d, ir, x, y, &ex, &ey);
                bad += !(same(map1.ptr<float>(y)[x], ex) && same(map2.ptr<float>(y)[x], ey));
                inside += ex >= 0 && ex < cols - 1 && ey >= 0 && ey < rows - 1;
            }
        EXPECT(bad == 0 && inside > W * H / 2);
        const int border[3] = {7, 200, 99};
        for (int colour = 0; colour < 2; colour++) {
            const Mat& src = colour ? bgr : gray;
            Mat two, fused, plain;
            remap(src, two, map1, map2, INTER_LINEAR, BORDER_CONSTANT, Scalar(7, 200, 99));
            rectifyViews(src, fused, K, pass ? D8 : D5, R, P, Size(W, H), Scalar(7, 200, 99));
            remap(src, plain, map1, map2);
            EXPECT(two.rows == H && two.cols == W && mat_channels(two) == mat_channels(src) && mat_depth(two) == D8U);
            int bad_two = 0, bad_fused = 0, bad_plain = 0;
            const int cn = mat_channels(src);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++)
                    for (int c = 0; c < cn; c++) {
                        const float mx = map1.ptr<float>(y)[x], my = map2.ptr<float>(y)[x];
                        bad_two += two.ptr<uint8_t>(y)[x * cn + c] != sample_at(src, c, mx, my, border[c]);
                        bad_fused += fused.ptr<uint8_t>(y)[x * cn + c] != two.ptr<uint8_t>(y)[x * cn + c];
                        bad_plain += plain.ptr<uint8_t>(y)[x * cn + c] != sample_at(src, c, mx, my, 0);
                    }
            EXPECT(bad_two == 0 && bad_fused == 0 && bad_plain == 0);
        }
    }
    {   // size with zero area: the source's size; empty R and newCameraMatrix
        Mat out;
        rectifyViews(bgr, out, K, Mat(), Mat(), Mat(), Size());
        EXPECT(out.rows == rows && out.cols == cols && mat_channels(out) == 3);
    }
}

int main(int argc, char** argv)
{
    const bool host = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
    host_only();
    if (!host) {
        if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
        on_device();
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("%s\n", host ? "host part passed" : "all passed");
    return 0;
}
