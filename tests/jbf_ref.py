"""The joint bilateral filter (include/adf_wls.h: "joint bilateral filter") stated directly in NumPy.

jbf(joint, src, r, C, S, border, dst_dtype) is the definition the device code is held to bit for bit.  It vectorises over
the PIXELS and loops over the TAPS in the stated order, on float32 arrays, so every product and sum rounds to float32
exactly once and the two accumulations are one chain per pixel.  The tables are ARGUMENTS (the library's
adf_jbf_tables_host / jbfTables, or tables() below): a comparison with the device never depends on two exp
implementations agreeing in the last bit.
"""
import numpy as np

MAX_RADIUS = 31
BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101 = 1, 2, 4


def clamped(d, sigma_color, sigma_space):
    """(sigma_color, sigma_space, r) as JBF.cpp:361-371 clamps them; Python's round is cvRound's half to even."""
    sc = 1.0 if sigma_color <= 0 else float(sigma_color)
    ss = 1.0 if sigma_space <= 0 else float(sigma_space)
    r = int(round(ss * 1.5)) if d <= 0 else int(d) // 2
    return sc, ss, max(r, 1)


def tables(d, sigma_color, sigma_space, channels):
    """(C, S, r) with NumPy's exp: C[a] over the L1 joint difference a, S[q] over the squared distance q, float32, one
    rounding per entry; entry 0 of both is 1."""
    sc, ss, r = clamped(d, sigma_color, sigma_space)
    a = np.arange(255 * channels + 1, dtype=np.int64)
    q = np.arange(r * r + 1, dtype=np.int64)
    with np.errstate(under="ignore"):
        C = np.exp((a * a).astype(np.float64) * (-0.5 / (sc * sc))).astype(np.float32)
        S = np.exp(q.astype(np.float64) * (-0.5 / (ss * ss))).astype(np.float32)
    C[0] = S[0] = 1.0
    return C, S, r


def border_index(p, n, border):
    """cv::borderInterpolate: where coordinate(s) p of an axis of length n are read, for any p."""
    p = np.asarray(p, dtype=np.int64)
    if border == BORDER_REPLICATE:
        return np.clip(p, 0, n - 1)
    if n == 1:
        return np.zeros_like(p)
    if border == BORDER_REFLECT:
        m = np.mod(p, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if border == BORDER_REFLECT_101:
        m = np.mod(p, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    raise ValueError("border type %r is not built" % (border,))


def taps(r):
    """The window's taps (i, j) in the order that is the definition: rows outer, columns inner, inside the disc."""
    return [(i, j) for i in range(-r, r + 1) for j in range(-r, r + 1) if i * i + j * j <= r * r]


def weighted_mean(joint, src, r, C, S, border=BORDER_REFLECT_101, dtype=np.float32):
    """y = sum / wsum in `dtype` (float32 is the definition; float64 is the yardstick of the error bound)."""
    g = np.asarray(joint).astype(np.int64)
    if g.ndim == 2:
        g = g[..., None]
    H, W = g.shape[:2]
    assert np.asarray(src).shape == (H, W)
    x = np.asarray(src).astype(dtype)
    C, S = np.asarray(C).astype(dtype), np.asarray(S).astype(dtype)
    ys, xs = np.arange(H), np.arange(W)
    total, wsum = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
    with np.errstate(all="ignore"):                       # (denormal products; non-finite sources propagate)
        for i, j in taps(r):
            qy, qx = border_index(ys + i, H, border), border_index(xs + j, W, border)
            L = np.abs(g - g[qy][:, qx]).sum(-1)
            w = (S[i * i + j * j] * C[L]).astype(dtype)
            total = (total + (w * x[qy][:, qx]).astype(dtype)).astype(dtype)
            wsum = (wsum + w).astype(dtype)
        return (total / wsum).astype(dtype)


def convert(y, dst_dtype):
    """Float: y.  uint8 / int16: rint (half to even), saturated; a NaN gives the depth's minimum."""
    dst_dtype = np.dtype(dst_dtype)
    if dst_dtype == np.float32:
        return y.astype(np.float32)
    info = np.iinfo(dst_dtype)
    with np.errstate(invalid="ignore"):
        return np.clip(np.rint(np.where(np.isnan(y), info.min, y)), info.min, info.max).astype(dst_dtype)


def jbf(joint, src, r, C, S, border=BORDER_REFLECT_101, dst_dtype=None, dtype=np.float32):
    """jointBilateralFilter(joint, src, ...) at radius r with the tables C and S; dst_dtype None = src's."""
    y = weighted_mean(joint, src, r, C, S, border, dtype)
    return convert(y, np.asarray(src).dtype if dst_dtype is None else dst_dtype)
