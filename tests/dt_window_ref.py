"""The domain transform filter's normalized-convolution mode (include/adf_wls.h: "domain transform filter, normalized
convolution") stated directly in NumPy.

dt_window_filter(guide, src, sigma_spatial, sigma_color, radii, dst_dtype) is the definition the device code is held to
bit for bit.  It vectorises ACROSS scanlines and pixels and loops over the offset 1 .. R to find every pixel's window, then
over the tap index to sum it in the stated order, on float32 arrays, so every product, sum and the division round to
float32 exactly once.  The radii are an ARGUMENT (the library's adf_dt_nc_radii_host / dtNcRadii, or radii() below).
"""
import numpy as np

from dt_ref import clamped, convert, l1_steps, sigma_h

MAX_RADIUS = 127


def radii(sigma_spatial, num_iters):
    """r_i = (float)(3 sigmaH_i), i = 1 .. N, with NumPy's doubles: float32 (N,)."""
    ss, _, N = clamped(sigma_spatial, 1.0, num_iters)
    return np.array([3.0 * sigma_h(ss, N, i) for i in range(1, N + 1)], np.float64).astype(np.float32)


def factor(sigma_spatial, sigma_color):
    """k = ss / sr in float32."""
    ss, sr, _ = clamped(sigma_spatial, sigma_color, 1)
    return np.float32(ss) / np.float32(sr)


def windows(L, r, k):
    """(left, right): how many pixels the window of every pixel reaches to either side.  L: (S, n-1), the guide's L1
    difference of the step between j and j + 1 of S scanlines of n pixels; the window of j is [j - left, j + right]."""
    S, n = L.shape[0], L.shape[1] + 1
    r, k = np.float32(r), np.float32(k)
    R = min(int(np.floor(r)), n - 1)
    j = np.arange(n)[None, :]
    out = []
    for side in (-1, 1):
        reach = np.zeros((S, n), np.int64)
        alive = np.ones((S, n), bool)
        walked = np.zeros((S, n), np.int64)                              # S(j - t, j) or S(j, j + t), exact
        for t in range(1, R + 1):
            step = np.zeros((S, n), np.int64)
            if side < 0:
                step[:, t:] = L[:, :n - t]                               # the step between j - t and j - t + 1
                inside = j >= t
            else:
                step[:, :n - t] = L[:, t - 1:]                           # the step between j + t - 1 and j + t
                inside = j + t <= n - 1
            walked += step
            D = np.float32(t) + (k * walked.astype(np.float32)).astype(np.float32)
            assert D.dtype == np.float32
            alive = alive & inside & ((D <= r) if side < 0 else (D < r))
            reach = np.where(alive, t, reach)
        out.append(reach)
    return out[0], out[1]


def window_pass(x, L, r, k, dtype=np.float32):
    """One pass along axis 1 of x (S, n): the mean over every pixel's window, summed left to right from x[lb] in `dtype`
    and divided once.  Returns a new array."""
    n = x.shape[1]
    left, right = windows(L, r, k)
    lb = np.arange(n)[None, :] - left
    count = left + right + 1
    acc = np.take_along_axis(x, lb, axis=1)
    for u in range(1, int(count.max())):
        tap = np.take_along_axis(x, np.minimum(lb + u, n - 1), axis=1)
        acc = np.where(u < count, acc + tap, acc)
    assert acc.dtype == np.dtype(dtype)
    return acc / count.astype(dtype)


def iterations(guide, src, radii, k, dtype=np.float32):
    """The N = len(radii) iterations on x = src in `dtype` (float32 is the definition; float64, over the same windows, is
    the yardstick of the error bound): every row, then every column, per iteration."""
    Lh, Lv = l1_steps(guide)
    x = np.array(src, dtype=dtype)
    assert x.ndim == 2 and x.shape == guide.shape[:2]
    for r in radii:
        x = window_pass(x, Lh, r, k, dtype)
        x = np.ascontiguousarray(window_pass(np.ascontiguousarray(x.T), np.ascontiguousarray(Lv.T), r, k, dtype).T)
    return x


def dt_window_filter(guide, src, sigma_spatial, sigma_color, radii, dst_dtype=None):
    """dtFilter(guide, src, ..., DTF_NC, N = len(radii)) with the radii `radii`; dst_dtype None = src's."""
    x = iterations(guide, src, radii, factor(sigma_spatial, sigma_color))
    return convert(x, src.dtype if dst_dtype is None else dst_dtype)
