"""The domain transform filter's recursive mode (include/adf_wls.h: "domain transform filter") stated directly in NumPy.

dt_filter(guide, src, table, dst_dtype) is the definition the device code is held to bit for bit.  It vectorises ACROSS
scanlines and loops ALONG them, on float32 arrays, so every subtraction, product and sum rounds to float32 exactly once
and in the stated order.  The feedback table is an ARGUMENT (the library's adf_dt_rf_table_host / dtRfTable, or
rf_table() below): a comparison with the device never depends on two exp implementations agreeing in the last bit.
"""
import numpy as np

MAX_ITERS = 8


def clamped(sigma_spatial, sigma_color, num_iters):
    """(ss, sr, N) as DT.inl:79-83 clamps them; ss and sr are float32."""
    return max(np.float32(1.0), np.float32(sigma_spatial)), max(np.float32(0.01), np.float32(sigma_color)), max(1, int(num_iters))


def distances(ss, sr, channels):
    """d_L = 1.0f + k * (float)L for L = 0 .. 255 * channels, k = ss / sr, each operation rounded to float32."""
    k = np.float32(ss) / np.float32(sr)
    L = np.arange(255 * channels + 1, dtype=np.float32)
    return np.float32(1.0) + (k * L).astype(np.float32)


def sigma_h(ss, N, i):
    """sigmaH_i = ss * 2^(N-i) / sqrt(4^N - 1) in double, i = 1 .. N."""
    return float(ss) * 2.0 ** (N - i) / np.sqrt(4.0 ** N - 1.0)


def rf_table(sigma_spatial, sigma_color, num_iters, channels):
    """The feedback table with NumPy's exp: float32 (N, 255 * channels + 1), row i - 1 = A_i."""
    ss, sr, N = clamped(sigma_spatial, sigma_color, num_iters)
    d = distances(ss, sr, channels).astype(np.float64)
    return np.stack([np.exp((-np.sqrt(2.0 / 3.0) / sigma_h(ss, N, i)) * d).astype(np.float32) for i in range(1, N + 1)])


def l1_steps(guide):
    """(Lh, Lv): the L1 guide difference between horizontal neighbours, (H, W-1), and vertical ones, (H-1, W)."""
    g = guide.astype(np.int64)
    if g.ndim == 2:
        g = g[..., None]
    return np.abs(g[:, 1:] - g[:, :-1]).sum(-1), np.abs(g[1:] - g[:-1]).sum(-1)


def _sweeps(x, a):
    """Along axis 1 of x (S, n), in place: there and back.  a: (S, n-1), the feedback of the step between j and j + 1."""
    n = x.shape[1]
    for j in range(1, n):
        x[:, j] = x[:, j] + a[:, j - 1] * (x[:, j - 1] - x[:, j])
    for j in range(n - 2, -1, -1):
        x[:, j] = x[:, j] + a[:, j] * (x[:, j + 1] - x[:, j])


def recurrence(guide, src, table, dtype=np.float32):
    """The N iterations on x = src in `dtype` (float32 is the definition; float64 is the yardstick of the error bound)."""
    table = np.asarray(table)
    Lh, Lv = l1_steps(guide)
    x = np.array(src, dtype=dtype)
    assert x.ndim == 2 and x.shape == guide.shape[:2]
    xt = x.T                                                             # a view: columns as scanlines
    for row in table:
        a = row.astype(dtype)
        _sweeps(x, a[Lh])
        _sweeps(xt, a[Lv].T)
    return x


def convert(x, dst_dtype):
    """Float: x.  uint8 / int16: rint (half to even), saturated."""
    dst_dtype = np.dtype(dst_dtype)
    if dst_dtype == np.float32:
        return x.astype(np.float32)
    info = np.iinfo(dst_dtype)
    return np.clip(np.rint(x), info.min, info.max).astype(dst_dtype)


def dt_filter(guide, src, table, dst_dtype=None):
    """dtFilter(guide, src, ..., DTF_RF, N = len(table)) with the feedback table `table`; dst_dtype None = src's."""
    return convert(recurrence(guide, src, table), src.dtype if dst_dtype is None else dst_dtype)
