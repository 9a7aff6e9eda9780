"""The guided filter of include/adf_wls.h ("guided filter") as straight NumPy: the statement the device result is compared
with bit for bit.  int64 sums, float64 expressions written operation by operation (NumPy neither contracts nor
re-associates them), float32 partial sums through explicit casts.  Slow and plain on purpose."""
import numpy as np

MAX_RADIUS = 31
_RANGE = {np.dtype(np.uint8): (0.0, 255.0), np.dtype(np.int16): (-32768.0, 32767.0)}


def reflect(i, n):
    """BORDER_REFLECT: index i (any integer array) of an axis of length n."""
    m = np.mod(np.asarray(i, np.int64), 2 * n)                           # non-negative
    return np.where(m < n, m, 2 * n - 1 - m)


def window_sum(v, r):
    """The (2r+1)^2 window sum of plane v in v's dtype and the statement's order: the column sum top to bottom over
    reflected rows, then the row sum left to right over reflected columns; every partial sum is rounded to the dtype."""
    H, W = v.shape
    rows, cols = reflect(np.arange(-r, H + r), H), reflect(np.arange(-r, W + r), W)
    p = v[rows][:, cols]                                                 # the plane with its reflected halo
    c = p[0:H]
    for k in range(1, 2 * r + 1):
        c = (c + p[k:k + H]).astype(v.dtype)
    s = c[:, 0:W]
    for k in range(1, 2 * r + 1):
        s = (s + c[:, k:k + W]).astype(v.dtype)
    return s


def guided_filter_q(guide, src, r, eps):
    """q of the statement, float64, before the conversion to the output's depth."""
    guide, src = np.asarray(guide), np.asarray(src)
    assert guide.dtype == np.uint8 and src.ndim == 2 and guide.shape[:2] == src.shape and 0 <= r <= MAX_RADIUS
    g = guide[..., None] if guide.ndim == 2 else guide
    ch = g.shape[2]
    assert ch in (1, 3)
    N = (2 * r + 1) ** 2
    Nd = np.float64(N)
    E = np.float64(eps) * Nd * Nd
    I = [g[..., c].astype(np.int64) for c in range(ch)]
    S = [window_sum(I[c], r) for c in range(ch)]                         # int64: exact
    V = {(c, d): (N * window_sum(I[c] * I[d], r) - S[c] * S[d]).astype(np.float64) for c in range(ch) for d in range(c, ch)}
    if src.dtype == np.float32:
        p = src.astype(np.float64)
        Sp = window_sum(p, r)                                            # float64 sums in the fixed order
        n = [Nd * window_sum(I[c].astype(np.float64) * p, r) - S[c].astype(np.float64) * Sp for c in range(ch)]
    else:
        assert src.dtype in (np.uint8, np.int16)
        p = src.astype(np.int64)
        Sp = window_sum(p, r)
        n = [(N * window_sum(I[c] * p, r) - S[c] * Sp).astype(np.float64) for c in range(ch)]
    with np.errstate(all="ignore"):
        if ch == 1:
            a = [(n[0] / (V[0, 0] + E)).astype(np.float32)]
        else:
            s00, s11, s22 = V[0, 0] + E, V[1, 1] + E, V[2, 2] + E
            s01, s02, s12 = V[0, 1], V[0, 2], V[1, 2]
            c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
            c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
            det = (s00 * c00 + s01 * c01) + s02 * c02
            ok = np.isfinite(det) & (det > 0)
            a = [(((c00 * n[0] + c01 * n[1]) + c02 * n[2]) / det).astype(np.float32),
                 (((c01 * n[0] + c11 * n[1]) + c12 * n[2]) / det).astype(np.float32),
                 (((c02 * n[0] + c12 * n[1]) + c22 * n[2]) / det).astype(np.float32)]
            a = [np.where(ok, x, np.float32(0)) for x in a]
        bn = Sp.astype(np.float64)
        for c in range(ch):
            bn = bn - a[c].astype(np.float64) * S[c].astype(np.float64)
        b = (bn / Nd).astype(np.float32)
        q = window_sum(b, r).astype(np.float64)                          # float32 sums in the fixed order
        for c in range(ch):
            q = q + window_sum(a[c], r).astype(np.float64) * I[c].astype(np.float64)
        return q / Nd


def convert(q, dtype):
    """q in the output's depth: (float)q, or rint (half to even) saturated; a NaN gives the depth's minimum."""
    dtype = np.dtype(dtype)
    with np.errstate(all="ignore"):
        if dtype == np.float32:
            return q.astype(np.float32)
        lo, hi = _RANGE[dtype]
        v = np.rint(q)
        v = np.where(v >= lo, np.minimum(v, hi), lo)
        return v.astype(dtype)


def guided_filter(guide, src, r, eps, dst_dtype=None):
    """guidedFilter(guide, src, r, eps, dDepth) of one map: dst_dtype None = src's."""
    src = np.asarray(src)
    return convert(guided_filter_q(guide, src, r, eps), src.dtype if dst_dtype is None else dst_dtype)
