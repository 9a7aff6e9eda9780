// CV_32FC1 disparity maps through DisparityWLSFilter::filter / filterToFloat (include/adf_ximgproc.hpp) on host Mats:
// relation R1 of adf_wls.h -- integer-valued float maps give the bits of the CV_16SC1 call, both outputs, both solvers,
// with and without confidence -- and one fractional case: the confidence map is the one of the rounded maps, the float
// output differs from the rounded maps' and keeps sat16(f32) == i16 (built and run by tests/test_cpp_float_input.py).
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

// the map as CV_32FC1 plus `frac` (|frac| < 0.5: it rounds back to the map)
static Mat as_float(const Mat& m, float frac)
{
    Mat f(m.rows, m.cols, D32F, 1);
    for (int i = 0; i < m.rows; i++)
        for (int j = 0; j < m.cols; j++) f.ptr<float>(i)[j] = (float)m.ptr<int16_t>(i)[j] + frac;
    return f;
}

static bool same_bytes(const Mat& a, const Mat& b, size_t elem)
{
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int i = 0; i < a.rows; i++)
        if (std::memcmp(a.ptr<unsigned char>(i), b.ptr<unsigned char>(i), (size_t)a.cols * elem) != 0) return false;
    return true;
}

static int16_t sat16(float v)
{
    if (!(std::fabs(v) < 2147483648.0f)) return (int16_t)-32768;
    const float r = std::nearbyint(v);
    return (int16_t)(r < -32768.0f ? -32768.0f : r > 32767.0f ? 32767.0f : r);
}

int main()
{
    if (adf_device_count() < 1) { std::printf("no GPU\n"); return 2; }
    const int W = 61, H = 40;
    const Rect roi(5, 3, 51, 33);
    Mat view, dl, dr;
    make_pair(W, H, 3, 3u, view, dl, dr);
    for (int solver : {ADF_SOLVER_WAVE, ADF_SOLVER_EXACT})
        for (bool use_conf : {true, false}) {
            Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(use_conf);
            wls->setSigmaColor(1.5); wls->setSolver(solver);
            const Mat none;
            const Mat& r16 = use_conf ? dr : none;
            Mat i16, f32, conf16, a, b;
            wls->filter(dl, view, i16, r16, roi);
            if (use_conf) conf16 = wls->getConfidenceMap();
            wls->filterToFloat(dl, view, f32, r16, roi);
            {   // R1: integer-valued float maps
                const Mat fl = as_float(dl, 0.0f), fr = use_conf ? as_float(dr, 0.0f) : Mat();
                wls->filter(fl, view, a, fr, roi);
                EXPECT(mat_depth(a) == D16S && same_bytes(a, i16, 2));
                if (use_conf) { Mat c = wls->getConfidenceMap(); EXPECT(same_bytes(c, conf16, 4)); }
                wls->filterToFloat(fl, view, b, fr, roi);
                EXPECT(mat_depth(b) == D32F && same_bytes(b, f32, 4));
            }
            {   // a fraction of an LSB on every element
                const Mat fl = as_float(dl, 0.37f), fr = use_conf ? as_float(dr, 0.37f) : Mat();
                wls->filterToFloat(fl, view, b, fr, roi);
                if (use_conf) { Mat c = wls->getConfidenceMap(); EXPECT(same_bytes(c, conf16, 4)); }   // the map of the rounded maps
                wls->filter(fl, view, a, fr, roi);
                long broken = 0, moved = 0, not_fill = 0;
                double shift = 0.0; long inside = 0;
                for (int i = 0; i < H; i++)
                    for (int j = 0; j < W; j++) {
                        const float v = b.ptr<float>(i)[j];
                        const bool in = i >= roi.y && i < roi.y + roi.height && j >= roi.x && j < roi.x + roi.width;
                        broken += sat16(v) != a.ptr<int16_t>(i)[j] || !std::isfinite(v);
                        not_fill += !in && v != -16.0f;
                        if (in && std::fabs(f32.ptr<float>(i)[j]) < 30000.0f) { moved += v != f32.ptr<float>(i)[j]; shift += v - f32.ptr<float>(i)[j]; inside++; }
                    }
                EXPECT(broken == 0); EXPECT(not_fill == 0); EXPECT(moved > 0);
                // the filter is linear in the maps and its weights sum to one: a constant offset comes out as itself
                EXPECT(inside > 0 && std::fabs(shift / (double)inside - 0.37) < 0.01);
            }
        }
    {   // a pair has one depth; float64 is not a depth of the maps
        Ptr<DisparityWLSFilter> wls = createDisparityWLSFilterGeneric(true);
        Mat out, f64(H, W, D64F, 1);
        int thrown = 0;
        try { wls->filter(as_float(dl, 0.0f), view, out, dr, roi); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { wls->filter(dl, view, out, as_float(dr, 0.0f), roi); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        try { wls->filterToFloat(f64, view, out, f64, roi); } catch (const Exception& e) { thrown += e.code == ADF_EBADARG; }
        EXPECT(thrown == 3);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all passed\n");
    return 0;
}
