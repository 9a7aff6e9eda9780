"""Direct statement (plain numpy, independent of the product code) of the semi-global matcher's both-views call with
the right view's map taken from the left view's aggregated volume -- the definition in include/adf_wls.h
(adf_sgbm_compute_both_*, ADF_SGBM_RIGHT_FROM_VOLUME), written as the definition reads: per right column, its candidates
along the volume's diagonal, the largest disparity of the smallest cost, the fit in the right matcher's index.

The volume is the one of tests/census_ref.py (formula 13 per direction, clipped after each addition); the left map of
the call is the existing statements' map (oracle.sgbm_compute for the Birchfield-Tomasi cost, census_ref /
census_variants_ref for the census costs)."""
import numpy as np

import census_ref
import census_variants_ref
from test_oracle_sgbm import DIRS, SHRT_MAX, naive_median3


def effective_penalties(P1, P2):
    P1 = P1 if P1 > 0 else 2
    return P1, max(P2 if P2 > 0 else 5, P1 + 1)


def aggregated_volume(Cv, mode, P1, P2):
    """S[y][x1][k]: the sum of the mode's path volumes, clipped to int16 after each addition (naive_census_sgbm's loop).
    P1 / P2 are the effective penalties."""
    S = np.zeros(Cv.shape, np.int64)
    for dx, dy in DIRS[mode]:
        S = np.clip(S + census_ref._path(Cv.astype(np.int64), dx, dy, P1, P2), -32768, SHRT_MAX)
    return S


def right_from_volume(S, W, nd, md):
    """The raw right-view map (H, W) of steps 1-5; S is (H, w1, nd) over the matched left columns [minX1, maxX1)."""
    H = S.shape[0]
    minx1 = max(md + nd, 0); maxx1 = W + min(md, 0)
    invalid = -(md + nd) * 16
    out = np.full((H, W), invalid, np.int64)
    if maxx1 - minx1 <= 0:
        return out
    assert S.shape == (H, maxx1 - minx1, nd)
    for xr in range(W):
        K = [k for k in range(nd) if minx1 <= xr + md + k < maxx1]                 # step 1
        if not K:
            continue
        s = {k: S[:, xr + md + k - minx1, k] for k in K}
        for y in range(H):
            m = min(int(s[k][y]) for k in K)
            if m >= SHRT_MAX:                                                     # step 2
                continue
            kb = max(k for k in K if int(s[k][y]) == m)                           # step 3
            d16 = (nd - 1 - kb) * 16
            if 0 < kb < nd - 1 and kb - 1 in s and kb + 1 in s:                   # step 4
                sp, sm = int(s[kb + 1][y]), int(s[kb - 1][y])
                den = max(sp + sm - 2 * m, 1)
                d16 += int(((sp - sm) * 16 + den) / (2 * den))                    # C division truncates toward zero
            out[y, xr] = d16 + (1 - md - nd) * 16                                 # step 5
    return out


def right_from_volume_rows(S, W, nd, md):
    """right_from_volume with every row of a column taken at once (the same steps on arrays): for the images a loop
    over pixels is too slow for.  tests/test_sgbm_both_ref.py holds the two to each other."""
    H = S.shape[0]
    minx1 = max(md + nd, 0); maxx1 = W + min(md, 0)
    invalid = -(md + nd) * 16
    out = np.full((H, W), invalid, np.int64)
    if maxx1 - minx1 <= 0:
        return out
    rows = np.arange(H)
    for xr in range(W):
        K = np.array([k for k in range(nd) if minx1 <= xr + md + k < maxx1], np.int64)
        if K.size == 0:
            continue
        s = S[:, xr + md + K - minx1, K].astype(np.int64)                           # (H, |K|), ascending k
        m = s.min(1)
        j = s.shape[1] - 1 - np.argmin(s[:, ::-1], 1)                              # the last (largest k) minimum
        kb = K[j]
        fit = (kb > 0) & (kb < nd - 1) & (j > 0) & (j < K.size - 1)
        sp = s[rows, np.minimum(j + 1, K.size - 1)]; sm = s[rows, np.maximum(j - 1, 0)]
        den = np.maximum(sp + sm - 2 * m, 1)
        num = (sp - sm) * 16 + den
        q = np.sign(num) * (np.abs(num) // (2 * den))                              # truncation toward zero
        v = (nd - 1 - kb) * 16 + np.where(fit, q, 0) + (1 - md - nd) * 16
        out[:, xr] = np.where(m >= SHRT_MAX, invalid, v)
    return out


def block_costs(oracle, left, right, nd, bs, md, cap, cost, k):
    """C[y][x1][d] of the left matcher: Birchfield-Tomasi (cost 0; oracle.sgbm_block_costs) or census (ctype, k)."""
    if cost == 0:
        return oracle.sgbm_block_costs(left, right, oracle.sgbm_params(nd, bs, md, prefilter_cap=cap)).astype(np.int64)
    with census_variants_ref.transform_swapped(cost):
        return census_ref.census_block_costs(left, right, nd, bs, md, k, False)


def left_raw(oracle, left, right, nd, bs, md, P1, P2, cap, ur, mode, disp12, cost, k):
    """The left view's raw map by the existing statements."""
    if cost == 0:
        return oracle.sgbm_compute(left, right, nd, bs, md, P1, P2, cap, ur, mode=mode, want_raw=True, disp12_max_diff=disp12)[1].astype(np.int64)
    return census_variants_ref.sgbm_variant(left, right, nd, bs, md, P1, P2, ur, mode, disp12, cost, k)


def both_maps(oracle, left, right, nd, bs, md=0, P1=0, P2=0, cap=0, ur=0, mode=2, disp12=1000000, cost=0, k=7, rows=True):
    """(left raw, right raw, left map, right map) of computeBoth(left, right, rightSource=SGBM_RIGHT_FROM_VOLUME): the
    raw maps and both after the 3 x 3 median, int16.  cost: 0 Birchfield-Tomasi, else an ADF_SGBM_COST_* census type."""
    H, W = left.shape[:2]
    lraw = left_raw(oracle, left, right, nd, bs, md, P1, P2, cap, ur, mode, disp12, cost, k)
    if W + min(md, 0) - max(md + nd, 0) <= 0:
        rraw = np.full((H, W), -(md + nd) * 16, np.int64)
    else:
        S = aggregated_volume(block_costs(oracle, left, right, nd, bs, md, cap, cost, k), mode, *effective_penalties(P1, P2))
        rraw = (right_from_volume_rows if rows else right_from_volume)(S, W, nd, md)
    return tuple(a.astype(np.int16) for a in (lraw, rraw, naive_median3(lraw), naive_median3(rraw)))
