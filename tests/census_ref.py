"""Direct statement (plain numpy, independent of the product code) of the census transform and of the semi-global
matcher with a census / Hamming cost -- the definition in include/adf_wls.h (adf_census_transform_*, adf_sgbm_set_cost).

The transform is the published one (Zabih & Woodfill 1994) with the bit rule of the reference's descriptor.hpp:182-194
and the sampling grids of descriptor.cpp:65-74; borders replicate the edge.  It is the library's own definition, not the
in-tree code's bit pattern (which reads past its row range, mis-skips the centre and leaves borders unwritten).  From
the cost volume on the matcher is the one of tests/test_oracle_sgbm.py::naive_sgbm."""
import numpy as np

from test_oracle_sgbm import DIRS, SHRT_MAX

DENSE_BITS = {3: 8, 5: 24, 7: 48}
SPARSE_BITS = {5: 8, 7: 16, 9: 24, 11: 36}


def census_offsets(k, sparse):
    n2 = k // 2
    return list(range(-n2, n2 + 1, 2 if sparse else 1))


def census_transform(img, k, sparse):
    """uint64 descriptor per pixel: offsets in rows top to bottom, left to right within a row, (0, 0) skipped, bit = 1 when
    neighbour > centre, first comparison most significant of the bits used; neighbour coordinates clamped to the image."""
    assert k in (SPARSE_BITS if sparse else DENSE_BITS), (k, sparse)
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.uint64)
    for dy in census_offsets(k, sparse):
        for dx in census_offsets(k, sparse):
            if dy == 0 and dx == 0:
                continue
            nb = a[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
            out = (out << np.uint64(1)) | (nb > a).astype(np.uint64)
    return out


def popcount64(v):
    v = v.astype(np.uint64)
    n = np.zeros(v.shape, np.int64)
    for b in range(48):
        n += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    assert not (v >> np.uint64(48)).any()
    return n


def census_block_costs(img1, img2, nd, bs, md, k, sparse):
    """C[y][x1][d] over the matchable columns [minx1, maxx1): Hamming pixel cost, summed over the bs x bs window with window
    coordinates clamped to the rows and to the matchable columns (naive_sgbm's rule), clamped to SHRT_MAX."""
    H, W = img1.shape
    c1, c2 = census_transform(img1, k, sparse), census_transform(img2, k, sparse)
    minx1 = max(md + nd, 0); maxx1 = W + min(md, 0); w1 = maxx1 - minx1
    xs = np.arange(minx1, maxx1)
    pix = np.zeros((H, w1, nd), np.int64)
    for d in range(nd):
        pix[:, :, d] = popcount64(c1[:, xs] ^ c2[:, xs - (md + d)])
    r = bs // 2
    yy = np.clip(np.arange(-r, H + r), 0, H - 1); xx = np.clip(np.arange(-r, w1 + r), 0, w1 - 1)
    Cv = np.zeros_like(pix)
    for dy in range(bs):
        for dx in range(bs):
            Cv += pix[yy[dy:dy + H]][:, xx[dx:dx + w1]]
    return np.minimum(Cv, SHRT_MAX)


def _path(Cv, dx, dy, P1, P2):
    """L volume of one direction of travel (dx, dy) by formula 13 on the pixel before, (x - dx, y - dy); zeros outside.
    A whole row (or, for the horizontal paths, a whole column) of pixels takes the step at once: they do not depend on
    each other."""
    H, w1, nd = Cv.shape
    L = np.zeros((H, w1, nd), np.int64); M = np.zeros((H, w1), np.int64)

    def step(Cp, Lp, mp):
        big = np.full(Lp.shape[:-1] + (1,), SHRT_MAX, np.int64)
        lm = np.concatenate([big, Lp[..., :-1]], -1) + P1; lp = np.concatenate([Lp[..., 1:], big], -1) + P1
        delta = (mp + P2)[..., None]
        Ln = np.clip(Cp + np.minimum(np.minimum(Lp, lm), np.minimum(lp, delta)) - delta, -32768, SHRT_MAX)
        return Ln, Ln.min(-1)

    if dy == 0:
        for x in (range(w1) if dx > 0 else range(w1 - 1, -1, -1)):
            px = x - dx
            if 0 <= px < w1:
                L[:, x], M[:, x] = step(Cv[:, x], L[:, px], M[:, px])
            else:
                L[:, x], M[:, x] = step(Cv[:, x], np.zeros((H, nd), np.int64), np.zeros(H, np.int64))
        return L
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        py = y - dy
        Lp = np.zeros((w1, nd), np.int64); mp = np.zeros(w1, np.int64)
        if 0 <= py < H:
            x = np.arange(w1); px = x - dx
            ok = (0 <= px) & (px < w1)
            Lp[ok] = L[py, px[ok]]; mp[ok] = M[py, px[ok]]
        L[y], M[y] = step(Cv[y], Lp, mp)
    return L


def naive_census_sgbm(img1, img2, nd, bs, md=0, P1=0, P2=0, ur=0, mode=2, disp12=1000000, k=7, sparse=False):
    """The raw CV_16S map (before the 3x3 median) of the semi-global matcher with the census cost (k, sparse): the block
    costs above, then the recursion, the winner, the uniqueness test, the sub-pixel fit and the matcher's own left-right
    check exactly as naive_sgbm states them."""
    H, W = img1.shape
    P1 = P1 if P1 > 0 else 2
    P2 = max(P2 if P2 > 0 else 5, P1 + 1)
    minx1 = max(md + nd, 0); maxx1 = W + min(md, 0); w1 = maxx1 - minx1
    invalid = (md - 1) * 16
    out = np.full((H, W), invalid, np.int64)
    if w1 <= 0:
        return out
    Cv = census_block_costs(img1, img2, nd, bs, md, k, sparse)
    S = np.zeros((H, w1, nd), np.int64)
    for dx, dy in DIRS[mode]:
        S = np.clip(S + _path(Cv, dx, dy, P1, P2), -32768, SHRT_MAX)
    maxdiff = disp12 if disp12 > 0 else 1
    ds = np.arange(nd)
    for y in range(H):
        d2p = np.full(W, invalid, np.int64); d2c = np.full(W, SHRT_MAX, np.int64)
        for x in range(w1 - 1, -1, -1):                              # from the right (stereo_binary_sgbm.cpp:456)
            Sp = S[y, x]
            best = int(np.argmin(Sp)); ms = int(Sp[best])            # argmin: first minimum
            if ms >= SHRT_MAX:
                continue
            if ur > 0 and ((Sp * (100 - ur) < ms * 100) & (np.abs(best - ds) > 1)).any():
                continue
            d = best
            x2 = x + minx1 - d - md
            if d2c[x2] > ms:
                d2c[x2] = ms; d2p[x2] = d + md
            if 0 < d < nd - 1:
                den = max(int(Sp[d - 1] + Sp[d + 1] - 2 * Sp[d]), 1)
                num = int(Sp[d - 1] - Sp[d + 1]) * 16 + den
                d = d * 16 + int(num / (den * 2))                    # C division truncates toward zero
            else:
                d *= 16
            out[y, x + minx1] = d + md * 16
        for x in range(minx1, maxx1):                                # the matcher's own left-right check (:598-613)
            d1 = int(out[y, x])
            if d1 == invalid:
                continue
            lo, hi = d1 >> 4, (d1 + 15) >> 4
            xl, xh = x - lo, x - hi
            if (0 <= xl < W and d2p[xl] >= md and abs(d2p[xl] - lo) > maxdiff and
                    0 <= xh < W and d2p[xh] >= md and abs(d2p[xh] - hi) > maxdiff):
                out[y, x] = invalid
    return out
