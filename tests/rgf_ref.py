"""The rolling guidance filter (include/adf_wls.h: "rolling guidance filter") stated directly in NumPy.

rgf(src, r, colour, space, scale, num_iter, border) is the definition the device code is held to bit for bit.  Like
jbf_ref it vectorises over the PIXELS and loops over the TAPS in the stated order on float32 arrays, so every product
and sum rounds to float32 exactly once and the two accumulations are one chain per pixel.  The tables are ARGUMENTS
(the library's adf_rgf_tables_host / rgfTables, or tables() below): a comparison with the device never depends on two
exp implementations agreeing in the last bit.  The border rule, the taps and the output conversion are jbf_ref's.
"""
import math

import numpy as np

from jbf_ref import BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, border_index, clamped, convert, taps  # noqa: F401

MAX_ITERS = 16
GRID_ENTRIES = 4098          # G[0 .. 4097]
GRID_TOP = np.float32(4096.0)


def colour_table(dtype, sigma_color):
    """C with math.exp, cut after its first zero entry (T entries), for uint8 / int16; the constant grid G for float32."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([math.exp(-0.5 * (i / 256.0) * (i / 256.0)) for i in range(GRID_ENTRIES)], np.float64).astype(np.float32)
    sc = 1.0 if sigma_color <= 0 else float(sigma_color)
    cc = -0.5 / (sc * sc)
    out = [np.float32(1.0)]
    for L in range(1, 256 if dtype == np.uint8 else 65536):
        out.append(np.float32(math.exp(float(L) * float(L) * cc)))
        if out[-1] == 0:
            break
    return np.array(out, np.float32)


def tables(dtype, d, sigma_color, sigma_space):
    """(colour, space, r, scale) with Python's exp, as rgfTables returns them."""
    sc, ss, r = clamped(d, sigma_color, sigma_space)
    q = np.arange(r * r + 1, dtype=np.float64)
    with np.errstate(under="ignore"):
        S = np.exp(q * (-0.5 / (ss * ss))).astype(np.float32)
    S[0] = 1.0
    scale = np.float32(256.0 / sc) if np.dtype(dtype) == np.float32 else np.float32(1.0)
    return colour_table(dtype, sc), S, r, scale


def range_weight(jp, jq, colour, scale):
    """Wc for arrays of centre and tap joint values (of the source's dtype)."""
    if jp.dtype == np.float32:
        scale = np.float32(scale)
        L = np.abs((jp - jq).astype(np.float32))
        a = (L * scale).astype(np.float32)
        a = np.where(a < GRID_TOP, a, GRID_TOP).astype(np.float32)        # NaN and infinity go to the zero end
        idx = a.astype(np.int32)
        f = (a - idx.astype(np.float32)).astype(np.float32)
        g0, g1 = colour[idx], colour[idx + 1]
        return (g0 + (f * (g1 - g0).astype(np.float32)).astype(np.float32)).astype(np.float32)
    L = np.abs(jp.astype(np.int64) - jq.astype(np.int64))
    return colour[np.minimum(L, len(colour) - 1)]


def iteration(src, joint, r, colour, space, scale, border=BORDER_REFLECT_101):
    """J_{k+1} from J_k = joint: the weighted mean in float32, stored in the source's dtype."""
    src, joint = np.asarray(src), np.asarray(joint)
    assert src.ndim == 2 and joint.shape == src.shape and joint.dtype == src.dtype
    H, W = src.shape
    x = src.astype(np.float32)
    colour, space = np.asarray(colour, np.float32), np.asarray(space, np.float32)
    ys, xs = np.arange(H), np.arange(W)
    total, wsum = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    with np.errstate(all="ignore"):                       # (denormal products; non-finite sources propagate)
        for i, j in taps(r):
            qy, qx = border_index(ys + i, H, border), border_index(xs + j, W, border)
            w = (space[i * i + j * j] * range_weight(joint, joint[qy][:, qx], colour, scale)).astype(np.float32)
            total = (total + (w * x[qy][:, qx]).astype(np.float32)).astype(np.float32)
            wsum = (wsum + w).astype(np.float32)
        return convert((total / wsum).astype(np.float32), src.dtype)


def rgf(src, r, colour, space, scale, num_iter, border=BORDER_REFLECT_101):
    """rollingGuidanceFilter(src, ...) at radius r with the tables given; a batch (N,H,W) map by map."""
    src = np.asarray(src)
    if src.ndim == 3:
        return np.stack([rgf(m, r, colour, space, scale, num_iter, border) for m in src])
    joint = src.copy()
    for _ in range(num_iter):
        joint = iteration(src, joint, r, colour, space, scale, border)
    return joint


def naive(src, r, colour, space, scale, num_iter, border=BORDER_REFLECT_101):
    """The same definition pixel by pixel with scalar float32 arithmetic: what rgf's vectorisation is checked against."""
    src = np.asarray(src)
    H, W = src.shape
    f32 = np.float32
    joint = src.copy()
    with np.errstate(all="ignore"):
        for _ in range(num_iter):
            y = np.zeros((H, W), f32)
            for py in range(H):
                for px in range(W):
                    total, wsum = f32(0), f32(0)
                    for i, j in taps(r):
                        qy, qx = int(border_index(py + i, H, border)), int(border_index(px + j, W, border))
                        if src.dtype == np.float32:
                            a = f32(f32(abs(f32(joint[py, px] - joint[qy, qx]))) * f32(scale))
                            if not a < GRID_TOP:
                                a = GRID_TOP
                            idx = int(a)
                            f = f32(a - f32(idx))
                            wc = f32(colour[idx] + f32(f * f32(colour[idx + 1] - colour[idx])))
                        else:
                            wc = colour[min(abs(int(joint[py, px]) - int(joint[qy, qx])), len(colour) - 1)]
                        w = f32(space[i * i + j * j] * wc)
                        total = f32(total + f32(w * f32(src[qy, qx])))
                        wsum = f32(wsum + w)
                    y[py, px] = f32(total / wsum)
            joint = convert(y, src.dtype)
    return joint
