// DisparityWLSFilter::filterToFloat (include/adf_ximgproc.hpp) on host Mats: the CV_32FC1 map is created at the view's
// size, and saturate_cast<short> of it is filter()'s CV_16SC1 map bit for bit -- on a same-size pair and on a pair with
// half-size maps, both solvers (built and run by tests/test_cpp_float_output.py).
#include "adf_ximgproc.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

using namespace adf;
using namespace adf::ximgproc;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// noisy view, disparity maps with a step: the confidence map is neither all 0 nor all 255
static void make_pair(int w, int h, int cn, unsigned seed, Mat& view, Mat& dl, Mat& dr)
{
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> px(0, 255), noise(-6, 6);
    view.create(h, w, D8U, cn); dl.create(h, w, D16S, 1); dr.create(h, w, D16S, 1);
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            for (int c = 0; c < cn; c++) view.ptr<unsigned char>(i)[j * cn + c] = (unsigned char)px(rng);
            const int d = j > w / 2 ? 48 : 16;
            dl.ptr<int16_t>(i)[j] = (int16_t)(d + noise(rng));
            dr.ptr<int16_t>(i)[j] = (int16_t)(-d + noise(rng));
        }
}

// cv::saturate_cast<short>(float): cvRound (half to even; NaN and anything outside the int range -> INT_MIN), clamped
static int16_t sat16(float v)
{
    if (!(std::fabs(v) < 2147483648.0f)) return (int16_t)-32768;
    const float r = std::nearbyint(v);
    return (int16_t)(r < -32768.0f ? -32768.0f : r > 32767.0f ? 32767.0f : r);
}

// the rounding relation over the whole frame, -16.0f outside `hi` (the ROI in the view's coordinates), no NaN or inf
static void check(const Mat& i16, const Mat& f32, int W, int H, Rect hi)
{
    EXPECT(f32.rows == H && f32.cols == W && mat_depth(f32) == D32F && mat_channels(f32) == 1);
    EXPECT(i16.rows == H && i16.cols == W && mat_depth(i16) == D16S);
    if (failures) return;
    long broken = 0, not_fill = 0, not_finite = 0, inside_differs = 0;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const float v = f32.ptr<float>(i)[j];
            const bool in = i >= hi.y && i < hi.y + hi.height && j >= hi.x && j < hi.x + hi.width;
            broken += sat16(v) != i16.ptr<int16_t>(i)[j];
            not_fill += !in && v != -16.0f;
            not_finite += !std::isfinite(v);
            inside_differs += in && v != std::nearbyint(v);
        }
    EXPECT(broken == 0); EXPECT(not_fill == 0); EXPECT(not_finite == 0);
    EXPECT(inside_differs > 0);                      // (the map does keep fractions of an LSB)
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    for (int solver : {ADF_SOLVER_WAVE, ADF_SOLVER_EXACT}) {
        {   // one small pair, maps of the view's size, odd ROI x and width
            const int W = 61, H = 40;
            Mat view, dl, dr;
            make_pair(W, H, 3, 3u, view, dl, dr);
            Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(true);
            wls->setSigmaColor(1.5); wls->setSolver(solver);
            const Rect roi(5, 3, 51, 33);
            Mat i16, f32;
            wls->filter(dl, view, i16, dr, roi);
            wls->filterToFloat(dl, view, f32, dr, roi);
            check(i16, f32, W, H, roi);
            Mat c = wls->getConfidenceMap();
            EXPECT(c.rows == H && c.cols == W);
            Mat again(H, W, D32F, 1);                // a map of the right type and size is written in place
            float* before = again.ptr<float>(0);
            wls->filterToFloat(dl, view, again, dr, roi);
            EXPECT(again.ptr<float>(0) == before);
            for (int i = 0; i < H && !failures; i++)
                EXPECT(std::memcmp(again.ptr<float>(i), f32.ptr<float>(i), (size_t)W * 4) == 0);
        }
        {   // half-size maps: the map is created at the VIEW's size (DF.cpp:252,282), the ROI is in the maps' coordinates
            const int W = 240, H = 120, w = W / 2, h = H / 2;
            Mat view, unused_l, unused_r, dl, dr, v2;
            make_pair(W, H, 1, 5u, view, unused_l, unused_r);
            make_pair(w, h, 1, 6u, v2, dl, dr);
            for (bool use_conf : {true, false}) {
                Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(use_conf);
                wls->setSigmaColor(1.5); wls->setDepthDiscontinuityRadius(2); wls->setSolver(solver);
                const Rect roi(6, 1, 110, 58);
                Mat i16, f32;
                wls->filter(dl, view, i16, use_conf ? dr : Mat(), roi);
                wls->filterToFloat(dl, view, f32, use_conf ? dr : Mat(), roi);
                check(i16, f32, W, H, Rect(12, 2, 220, 116));
                Rect r = wls->getROI();
                EXPECT(r.x == roi.x && r.y == roi.y && r.width == roi.width && r.height == roi.height);
            }
        }
    }
    {   // the refusals are filter()'s
        Mat view, dl, dr, out;
        make_pair(32, 16, 1, 9u, view, dl, dr);
        Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(true);
        int thrown = 0;
        try { wls->filterToFloat(dl, view, out); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { wls->filterToFloat(view, view, out, dr); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { wls->filterToFloat(dl, dl, out, dr); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 3);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
