/* speckle_ref.c -- sequential restatement of cv::filterSpeckles for CV_16SC1 maps (the checker of the device speckle
 * filter; tests/test_speckle_ref.py builds it with gcc).  Flood fill with an explicit worklist, one component at a time:
 *   - pixels equal to new_val belong to no component;
 *   - 4-neighbours p, q are joined when both differ from new_val and |d(p) - d(q)| <= max_diff (int32 arithmetic);
 *   - every component of at most max_size pixels is set to new_val.
 * img: H rows of W int16 at `stride` ELEMENTS, modified in place.  label: W*H ints, list: W*H ints (scratch). */
#include <stdint.h>
#include <stdlib.h>

void speckle_ref(int16_t* img, int W, int H, long stride, int new_val, int max_size, int max_diff, int* label, int* list)
{
    const long n = (long)W * H;
    for (long i = 0; i < n; i++) label[i] = 0;
    int cur = 0;
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const long p0 = (long)y * W + x;
            if (label[p0] || img[y * stride + x] == new_val) continue;
            label[p0] = ++cur;
            /* list[0..done) expanded, list[done..top) pending; at the end list[0..top) is the whole component */
            long top = 0, done = 0;
            list[top++] = (int)p0;
            while (done < top) {
                const int p = list[done++];
                const int py = p / W, px = p - py * W;
                const int v = img[py * stride + px];
                static const int dx[4] = {1, -1, 0, 0}, dy[4] = {0, 0, 1, -1};
                for (int k = 0; k < 4; k++) {
                    const int qx = px + dx[k], qy = py + dy[k];
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const long q = (long)qy * W + qx;
                    const int w = img[qy * stride + qx];
                    if (label[q] || w == new_val || abs(w - v) > max_diff) continue;
                    label[q] = cur;
                    list[top++] = (int)q;
                }
            }
            if (top <= max_size)
                for (long k = 0; k < top; k++) {
                    const int p = list[k];
                    img[(p / W) * stride + p % W] = (int16_t)new_val;
                }
        }
    }
}
