"""Direct statements (plain Python / numpy, independent of the product code) of the two things the block matcher's own
left-right check needs -- the definitions in include/adf_wls.h:

    validate_disparity   validateDisparity(disp, cost, minDisparity, numberOfDisparities, disp12MaxDiff) as sequential
                         loops (adf_validate_disparity_*), counting the votes that fell outside the row;
    bm_winner_cost       the aggregated cost of the winning integer disparity (adf_bm_compute_cost_*): for SAD a numpy
                         restatement of the x-Sobel prefilter and the window sums of oracle/adf_oracle_bm.c, for the census
                         costs bm_census_ref.block_costs with the descriptors of census_variants_ref; the winner is the
                         largest-disparity strict minimum; returned as int32 and as its truncation to int16.
"""
import numpy as np

import bm_census_ref
import census_variants_ref

INT_MAX = 2 ** 31 - 1
SAD = 0


def validate_disparity(disp, cost, minD, nd, maxdiff):
    """(map, votes outside the row) of one (H, W) map; the inputs are left as they are."""
    disp = np.asarray(disp)
    cost = np.asarray(cost)
    assert disp.shape == cost.shape and disp.ndim == 2
    H, W = disp.shape
    maxD = minD + nd
    INV = (minD - 1) * 16
    X0, X1 = max(maxD, 0), W + min(minD, 0)
    out = disp.copy()
    outside = 0
    for y in range(H):
        drow = [int(v) for v in disp[y]]
        crow = [int(v) for v in cost[y]]
        disp2 = [INV] * W
        cost2 = [INT_MAX] * W
        for x in range(X0, X1):
            d = drow[x]
            if d == INV:
                continue
            x2 = x - ((d + 8) >> 4)
            if not 0 <= x2 < W:
                outside += 1
                continue
            if cost2[x2] > crow[x]:
                cost2[x2] = crow[x]
                disp2[x2] = d
        for x in range(X0, X1):
            d = drow[x]
            if d == INV:
                continue
            contradicted = 0
            for dk in (d >> 4, (d + 15) >> 4):
                xc = x - dk
                if 0 <= xc < W and disp2[xc] > INV and abs(disp2[xc] - d) > 16 * maxdiff:
                    contradicted += 1
            if contradicted == 2:
                out[y, x] = INV
    return out, outside


def truncate16(c):
    """(int16_t)c of an int32 value: the low 16 bits, two's complement."""
    return (((np.asarray(c, np.int64) + 32768) & 0xFFFF) - 32768).astype(np.int16)


def prefilter_xsobel(img, cap):
    """adf_oracle_bm_prefilter_xsobel: rows reflect (row -1 -> row 1), columns 0 and W-1 hold cap."""
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape
    rows = np.arange(H)
    up = np.where(rows > 0, rows - 1, 1 if H > 1 else 0)
    dn = np.where(rows < H - 1, rows + 1, H - 2 if H > 1 else 0)
    out = np.full((H, W), cap, np.int64)
    if W > 2:
        dx = a[:, 2:] - a[:, :-2]
        out[:, 1:-1] = np.clip(dx[up] + 2 * dx + dx[dn], -cap, cap) + cap
    return out


def _window_sums(pix, bs):
    """Sums of every full bs x bs window of pix, from its integral image: (h - bs + 1, w - bs + 1)."""
    c = np.zeros((pix.shape[0] + 1, pix.shape[1] + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(pix, 0), 1)
    return c[bs:, bs:] - c[:-bs, bs:] - c[bs:, :-bs] + c[:-bs, :-bs]


def sad_block_costs(left, right, nd, bs, md, cap):
    """(S, T, xs, xe): S[k, y, x] the SAD of the prefiltered views over the window, d = md + k, and T[y, x] the texture
    sum of |L - cap|, for y in [w2, H - w2), x in [xs, xe) (zeros elsewhere), as adf_oracle_bm_compute forms them."""
    H, W = left.shape
    w2 = bs // 2
    xs, xe = max(md + nd - 1, 0) + w2, W + min(md, 0) - w2
    S = np.zeros((nd, H, W), np.int64)
    T = np.zeros((H, W), np.int64)
    if xe <= xs or H <= 2 * w2:
        return S, T, xs, xe
    L, R = prefilter_xsobel(left, cap), prefilter_xsobel(right, cap)
    cols = np.arange(xs - w2, xe + w2)
    T[w2:H - w2, xs:xe] = _window_sums(np.abs(L[:, cols] - cap), bs)
    for k in range(nd):
        S[k, w2:H - w2, xs:xe] = _window_sums(np.abs(L[:, cols] - R[:, cols - (md + k)]), bs)
    return S, T, xs, xe


def block_costs(left, right, nd, bs, md=0, cap=31, ctype=SAD, k=7):
    """(S, T, xs, xe) for any ADF_BM_COST_*; T is None for a census cost (no prefiltered image, no texture test)."""
    left, right = np.asarray(left), np.asarray(right)
    if ctype == SAD:
        return sad_block_costs(left, right, nd, bs, md, cap)
    with census_variants_ref.transform_swapped(ctype):
        S, xs, xe = bm_census_ref.block_costs(left, right, nd, bs, md, k, False)
    return S, None, xs, xe


def resolve(costs, shape, nd, bs, md=0, texthr=0, uniq=0):
    """(map, cost32, cost16) from block_costs' result: the winner (ties to the largest disparity), the texture and
    uniqueness tests, the sub-pixel fit and the +15 >> 4 rounding of oracle/adf_oracle_bm.c.  cost32 is the winner's
    cost wherever a window was matched (also where a test then rejected the pixel, 0 outside the valid rectangle);
    cost16 is what the device plane holds: the truncation where the map is not filtered, 0 elsewhere."""
    S, T, xs, xe = costs
    H, W = shape
    w2 = bs // 2
    out = np.full((H, W), (md - 1) * 16, np.int64)
    cost32 = np.zeros((H, W), np.int32)
    if xe <= xs or H <= 2 * w2:
        return out.astype(np.int16), cost32, np.zeros((H, W), np.int16)
    bk = nd - 1 - np.argmin(S[::-1], axis=0)                        # ties: the largest disparity
    best = np.take_along_axis(S, bk[None], 0)[0]
    pv = np.take_along_axis(S, np.where(bk > 0, bk - 1, 1)[None], 0)[0]
    nv = np.take_along_axis(S, np.where(bk < nd - 1, bk + 1, nd - 2)[None], 0)[0]
    dd = pv + nv - 2 * best + np.abs(pv - nv)
    num = (pv - nv) * 256
    frac = np.where(dd != 0, np.sign(num) * (np.abs(num) // np.maximum(dd, 1)), 0)   # C division truncates toward zero
    res = ((bk + md) * 256 + frac + 15) >> 4
    rect = np.zeros((H, W), bool)
    rect[w2:H - w2, xs:xe] = True
    keep = rect.copy()
    if T is not None:
        keep &= ~(T < texthr)
    if uniq > 0:
        thresh = best + best * uniq // 100
        far = np.abs(np.arange(nd)[:, None, None] - bk[None]) > 1
        keep &= ~(far & (S <= thresh[None])).any(0)
    out[keep] = res[keep]
    cost32[rect] = best[rect]
    return out.astype(np.int16), cost32, np.where(keep, truncate16(best), 0).astype(np.int16)


def bm_winner_cost(left, right, nd, bs, md=0, cap=31, texthr=0, uniq=0, ctype=SAD, k=7):
    """(map, cost32, cost16) of the block matcher at these settings (see resolve)."""
    return resolve(block_costs(left, right, nd, bs, md, cap, ctype, k), np.asarray(left).shape, nd, bs, md, texthr, uniq)
