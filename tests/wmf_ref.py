"""The weighted median filter of include/adf_wls.h, stated directly in NumPy (the library's own definition; nothing else
lives here).  Integer weights from a table passed in, so the result does not depend on summation order:

    used(q) = mask(q) != 0 and src(q) != ignore_value and not isnan(src(q))
    w(p, q) = table[ sum_c (joint_c(p) - joint_c(q))^2 ]
    Tot = sum of w over the used taps of the (2r+1)^2 window clipped at the border
    dst(p) = the smallest tap value v with 2 * sum(w over used taps with src(q) <= v) >= Tot;  Tot == 0: src(p)
"""
import numpy as np


def keys_of(src):
    """Order-preserving unsigned keys of a uint8 / int16 / float32 map (floats as IEEE totals, -0.0 below +0.0)."""
    if src.dtype == np.float32:
        b = src.view(np.uint32).astype(np.int64)
        return np.where(b & 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)
    return src.astype(np.int64) - np.iinfo(src.dtype).min


def weighted_median(joint, src, r, table, mask=None, ignore_value=None):
    """One map: joint (H,W) or (H,W,3) uint8, src (H,W) uint8 / int16 / float32, table the uint32 weights by squared
    joint distance.  Returns dst of src's dtype."""
    H, W = src.shape
    used = np.ones((H, W), bool) if mask is None else mask != 0
    if ignore_value is not None:
        used = used & (src.astype(np.float64) != float(ignore_value))
    if src.dtype == np.float32:
        used = used & ~np.isnan(src)
    key = keys_of(src)
    j = joint.astype(np.int64).reshape(H, W, -1)
    table = np.asarray(table).astype(np.int64)
    n = (2 * r + 1) ** 2
    # the shifted planes: key and weight of tap k of every pixel (weight 0: unused); 2 * 63^2 * 65536 < 2^31
    K = np.zeros((n, H, W), np.int64 if src.dtype == np.float32 else np.int32)
    Wt = np.zeros((n, H, W), np.int32)
    k = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)      # pixels p whose tap p + (dx, dy) is inside
            if ys < ye and xs < xe:
                q = (slice(ys + dy, ye + dy), slice(xs + dx, xe + dx))
                p = (slice(ys, ye), slice(xs, xe))
                d2 = ((j[p] - j[q]) ** 2).sum(-1)
                K[k][p] = key[q]
                Wt[k][p] = np.where(used[q], table[d2], 0)
            k += 1
    order = np.argsort(K, axis=0, kind="stable")
    Ks = np.take_along_axis(K, order, 0)
    cum = np.cumsum(np.take_along_axis(Wt, order, 0), 0, dtype=np.int32)
    tot = cum[-1]
    first = np.argmax(2 * cum >= tot[None], axis=0)                       # the first index with 2 cum >= Tot
    med = np.take_along_axis(Ks, first[None], 0)[0].astype(np.int64)
    # an unused tap has weight 0 and never is that first index unless Tot == 0, where src stays
    if src.dtype == np.float32:
        bits = np.where(med & 0x80000000, med ^ 0x80000000, med ^ 0xFFFFFFFF).astype(np.uint32)
        out = bits.view(np.float32)
    else:
        out = (med + np.iinfo(src.dtype).min).astype(src.dtype)
    return np.where(tot == 0, src, out) if src.dtype != np.float32 else \
        np.where(tot == 0, src.view(np.uint32), out.view(np.uint32)).view(np.float32)
