"""The direct NumPy statement of the reprojection to 3-D and of the point list (include/adf_wls.h, "reprojection to 3-D"):
what the device code is held to bit for bit (tests/test_gpu_reproject.py).  float64 element-wise operations, each a
single IEEE binary64 rounding, in the order the header gives; one rounding to float32 at the end."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)      # 2^-23
BIG_Z = np.float32(10000.0)
MISSING_NONE, MISSING_MIN, MISSING_VALUE = 0, 1, 2


def map_minimum(disp):
    """m of MISSING_MIN for one map: the minimum raw value, NaN ignored (a map of NaN only: NaN, nothing is missing)."""
    d = np.asarray(disp)
    if d.dtype.kind == "f":
        d = d[~np.isnan(d)]
        if d.size == 0:
            return float("nan")
    return float(d.min())


def missing_mask(disp, mode, missing_value=None):
    """missing(s) <=> fabs((double)s - m) <= FLT_EPSILON on the raw values of ONE map (H,W)."""
    if mode == MISSING_NONE:
        return np.zeros(np.shape(disp), bool)
    m = map_minimum(disp) if mode == MISSING_MIN else float(missing_value)
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(disp).astype(np.float64) - np.float64(m)) <= FLT_EPSILON


def reproject(disp, Q, disp_scale=1.0, mode=MISSING_NONE, missing_value=None):
    """(H,W) or (N,H,W) int16 / float32 -> (...,H,W,3) float32."""
    disp = np.asarray(disp)
    if disp.ndim == 3:
        return np.stack([reproject(d, Q, disp_scale, mode, missing_value) for d in disp])
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    H, W = disp.shape
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        d = disp.astype(np.float64) * np.float64(disp_scale)
        r = [((Q[i, 0] * x + Q[i, 1] * y) + Q[i, 3]) + Q[i, 2] * d for i in range(4)]
        iw = np.float64(1.0) / r[3]
        xyz = np.stack([(r[i] * iw).astype(np.float32) for i in range(3)], axis=-1)
    xyz[..., 2][missing_mask(disp, mode, missing_value)] = BIG_Z
    return xyz


def valid_mask(disp, xyz, roi=None, z_range=None, mode=MISSING_NONE, missing_value=None):
    """ONE map: inside roi (x, y, w, h), not missing, X Y Z finite, z_min <= Z <= z_max."""
    H, W = disp.shape
    ok = np.zeros((H, W), bool)
    x0, y0, w, h = roi if roi is not None else (0, 0, W, H)
    ok[y0:y0 + h, x0:x0 + w] = True
    ok &= ~missing_mask(disp, mode, missing_value)
    ok &= np.isfinite(xyz).all(axis=-1)
    if z_range is not None:
        z = xyz[..., 2].astype(np.float64)
        with np.errstate(all="ignore"):
            ok &= (np.float64(z_range[0]) <= z) & (z <= np.float64(z_range[1]))
    return ok


def point_cloud(disp, Q, view=None, roi=None, z_range=None, disp_scale=1.0, mode=MISSING_NONE, missing_value=None):
    """ONE map -> (points (count,3) float32, colours (count,C) uint8 or None, index (count,) int32): xyz[mask] in raster
    order (boolean indexing walks y major, x minor)."""
    disp = np.asarray(disp)
    xyz = reproject(disp, Q, disp_scale, mode, missing_value)
    ok = valid_mask(disp, xyz, roi, z_range, mode, missing_value)
    colours = None
    if view is not None:
        v = np.asarray(view)
        colours = (v[..., None] if v.ndim == 2 else v)[ok]
    return xyz[ok], colours, np.flatnonzero(ok.ravel()).astype(np.int32)
