"""Direct statement (plain numpy, independent of the product code) of the block matcher with a census / Hamming cost --
the definition in include/adf_wls.h (adf_bm_set_cost).

    cL, cR      census_ref.census_transform of the left / right view at (k, sparse); neighbour coordinates clamped
    pixel cost  popcount(cL(y, x) ^ cR(y, x - d))
    S[k][x]     the pixel cost summed over the full blockSize x blockSize window, d = minDisparity + k

and everything else is oracle/adf_oracle_bm.c with the SAD replaced: the valid rectangle
x in [max(maxD, 0) + w/2, W + min(minD, 0) - w/2), y in [w/2, H - w/2), (minDisparity - 1) * 16 outside it, ties to the
largest disparity, the uniqueness test, the sub-pixel formula and the +15 >> 4 rounding.  There is no prefiltered image,
so no preFilterCap and no texture test."""
import numpy as np

from census_ref import census_transform, popcount64


def block_costs(left, right, nd, bs, md, k, sparse):
    """(S, xs, xe): S[kk, y, x] for y in [w2, H - w2), x in [xs, xe), as an int64 array of the image's size (zeros
    elsewhere); xe <= xs: nothing is matched."""
    H, W = left.shape
    w2 = bs // 2
    maxd = md + nd - 1
    xs, xe = max(maxd, 0) + w2, W + min(md, 0) - w2
    S = np.zeros((nd, H, W), np.int64)
    if xe <= xs or H <= 2 * w2:
        return S, xs, xe
    cl, cr = census_transform(left, k, sparse), census_transform(right, k, sparse)
    cols = np.arange(xs - w2, xe + w2)                              # every column some window reaches
    for kk in range(nd):
        pix = popcount64(cl[:, cols] ^ cr[:, cols - (md + kk)])    # (H, len(cols))
        win = np.zeros((H - 2 * w2, xe - xs), np.int64)
        for dy in range(bs):
            for dx in range(bs):
                win += pix[dy:dy + H - 2 * w2, dx:dx + xe - xs]
        S[kk, w2:H - w2, xs:xe] = win
    return S, xs, xe


def bm_census(left, right, nd, bs, md=0, uniq=0, k=7, sparse=False):
    """The CV_16SC1 map of the block matcher with the census cost (k, sparse)."""
    left, right = np.asarray(left), np.asarray(right)
    H, W = left.shape
    w2 = bs // 2
    out = np.full((H, W), (md - 1) * 16, np.int64)
    S, xs, xe = block_costs(left, right, nd, bs, md, k, sparse)
    if xe <= xs or H <= 2 * w2:
        return out.astype(np.int16)
    bk = nd - 1 - np.argmin(S[::-1], axis=0)                        # ties: the largest disparity
    best = np.take_along_axis(S, bk[None], 0)[0]
    pv = np.take_along_axis(S, np.where(bk > 0, bk - 1, 1)[None], 0)[0]
    nv = np.take_along_axis(S, np.where(bk < nd - 1, bk + 1, nd - 2)[None], 0)[0]
    dd = pv + nv - 2 * best + np.abs(pv - nv)
    num = (pv - nv) * 256
    frac = np.where(dd != 0, np.sign(num) * (np.abs(num) // np.maximum(dd, 1)), 0)   # C division truncates toward zero
    res = ((bk + md) * 256 + frac + 15) >> 4
    keep = np.zeros((H, W), bool)
    keep[w2:H - w2, xs:xe] = True
    if uniq > 0:
        thresh = best + best * uniq // 100
        far = np.abs(np.arange(nd)[:, None, None] - bk[None]) > 1
        keep &= ~(far & (S <= thresh[None])).any(0)
    out[keep] = res[keep]
    return out.astype(np.int16)
