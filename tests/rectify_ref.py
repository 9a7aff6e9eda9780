"""The direct NumPy statement of the library's rectification (include/adf_wls.h, "rectification"): the parameter
inverse, the CV_32FC1 map pair and the 5-bit bilinear remap with a constant border.  float64 array operations in the
stated order (NumPy never fuses a multiply with an add), one conversion to float32, integer sampling with explicit tap
masks.  The device results are compared with this bit for bit."""
import numpy as np


def inverse3(A):
    """Adjugate divided by determinant, in the header's order: cofactor products, cofactor differences, the determinant
    by the first row, one division per entry."""
    a = np.asarray(A, np.float64)
    c = np.empty((3, 3), np.float64)
    c[0, 0] = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
    c[0, 1] = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
    c[0, 2] = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
    c[1, 0] = a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]
    c[1, 1] = a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]
    c[1, 2] = a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]
    c[2, 0] = a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]
    c[2, 1] = a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]
    c[2, 2] = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    det = (a[0, 0] * c[0, 0] + a[0, 1] * c[0, 1]) + a[0, 2] * c[0, 2]
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("singular")
    return c.T / det


def product3(P, R):
    """A = P[:, :3] * R with A[i][j] = (P[i][0]*R[0][j] + P[i][1]*R[1][j]) + P[i][2]*R[2][j]; R None = P[:, :3] itself."""
    P = np.asarray(P, np.float64)[:, :3]
    if R is None:
        return P.copy()
    R = np.asarray(R, np.float64)
    return (P[:, 0:1] * R[0:1, :] + P[:, 1:2] * R[1:2, :]) + P[:, 2:3] * R[2:3, :]


def params(K, dist, R, P):
    """(fx, fy, cx, cy), dist[8], ir[9] as adf_rectify_params_init gives them."""
    K = np.asarray(K, np.float64)
    d = np.zeros(8, np.float64)
    dist = np.zeros(0) if dist is None else np.asarray(dist, np.float64).ravel()
    if dist.size not in (0, 4, 5, 8):
        raise ValueError("n_dist")
    d[:dist.size] = dist
    ir = inverse3(product3(K if P is None else P, R)).ravel()
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), d, ir


def init_map(prm, W, H):
    (fx, fy, cx, cy), d, ir = prm
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in d)
    ir = [np.float64(v) for v in ir]
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (ir[0] * u + ir[1] * v) + ir[2]
        Y = (ir[3] * u + ir[4] * v) + ir[5]
        D = (ir[6] * u + ir[7] * v) + ir[8]
        w = 1.0 / D
        x = X * w
        y = Y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
        mx = (np.float64(fx) * xd + np.float64(cx)).astype(np.float32)
        my = (np.float64(fy) * yd + np.float64(cy)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(mx, (H, W))), np.ascontiguousarray(np.broadcast_to(my, (H, W)))


def remap(src, mapx, mapy, border_value=0):
    """src (h,w) or (h,w,3) uint8; maps (H,W) float32 -> (H,W[,3]) uint8."""
    src = np.asarray(src)
    gray = src.ndim == 2
    s = src[..., None] if gray else src
    sh, sw, ch = s.shape
    border = np.broadcast_to(np.asarray(border_value, np.int64), (ch,)) if np.ndim(border_value) == 0 else np.asarray(border_value, np.int64)[:ch]
    with np.errstate(all="ignore"):
        tx = np.asarray(mapx, np.float32) * np.float32(32.0)
        ty = np.asarray(mapy, np.float32) * np.float32(32.0)
        ok = (tx >= np.float32(-1048576.0)) & (tx <= np.float32(1048575.0)) & (ty >= np.float32(-1048576.0)) & (ty <= np.float32(1048575.0))
        sx = np.rint(np.where(ok, tx, np.float32(0))).astype(np.int64)   # np.rint: half to even
        sy = np.rint(np.where(ok, ty, np.float32(0))).astype(np.int64)
    ix, ax = sx >> 5, sx & 31
    iy, ay = sy >> 5, sy & 31

    def tap(i, j):
        inside = (i >= 0) & (i < sw) & (j >= 0) & (j < sh)
        v = s[np.where(inside, j, 0), np.where(inside, i, 0)].astype(np.int64)     # masked taps never index outside
        return np.where(inside[..., None], v, border[None, None, :])

    ax, ay = ax[..., None], ay[..., None]
    out = (tap(ix, iy) * (32 - ax) * (32 - ay) + tap(ix + 1, iy) * ax * (32 - ay)
           + tap(ix, iy + 1) * (32 - ax) * ay + tap(ix + 1, iy + 1) * ax * ay + 512) >> 10
    out = np.where(ok[..., None], out, border[None, None, :]).astype(np.uint8)
    return out[..., 0] if gray else out


def rectify(src, K, dist, R, P, size=None, border_value=0):
    h, w = np.asarray(src).shape[:2]
    W, H = (w, h) if size is None else size
    mx, my = init_map(params(K, dist, R, P), W, H)
    return remap(src, mx, my, border_value)


def same_bits(a, b):
    """Equal bit for bit, except that NaNs only have to sit at the same positions (sign and payload are not contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ai, bi = a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64)
    return bool(np.array_equal(ai[~na], bi[~nb]))


# ---- the models the tests share ----
def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def models(w, h):
    """name -> (K, dist, R, P) for a source of w x h: the models of tests/test_gpu_rectify.py."""
    f = 0.8 * max(w, h, 8)
    K = np.array([[f, 0.0, (w - 1) / 2.0 + 0.3], [0.0, f * 1.01, (h - 1) / 2.0 - 0.2], [0.0, 0.0, 1.0]])
    Ki = np.array([[1.0, 0.0, float(w // 2)], [0.0, 1.0, float(h // 2)], [0.0, 0.0, 1.0]])
    a = np.deg2rad(2.0)
    R2 = rot(a, -a, a)
    P = np.array([[f * 0.9, 0.0, (w - 1) / 2.0, -f * 0.54], [0.0, f * 0.9, (h - 1) / 2.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    kitti = [-0.37, 0.2, 1e-3, -2e-4, -0.07]
    eight = [-0.37, 0.2, 1e-3, -2e-4, -0.07, 0.01, -0.03, 0.002]
    # D = ir6*u + ir7*v + ir8 crosses 0 inside the image: a strong rotation about y puts the horizon in view
    Rh = rot(0.0, np.deg2rad(80.0), 0.0)
    Kh = np.array([[0.4 * max(w, 8), 0.0, (w - 1) / 2.0], [0.0, 0.4 * max(w, 8), (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    # most of the destination falls outside the source: the principal point of P far off
    Pout = np.array([[f, 0.0, (w - 1) / 2.0 - 0.8 * w], [0.0, f, (h - 1) / 2.0 + 0.7 * h], [0.0, 0.0, 1.0]])
    # D = 0.5*u - 2 exactly (the inverse of this P is exact in binary): D == 0 in column 4, so w = inf and 0*inf = NaN
    Ppole = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.0, -0.5]])
    return {
        "pole": (Kh, None, None, Ppole),
        "identity": (Ki, None, None, Ki),
        "kitti": (K, kitti, R2, P),
        "eight": (K, eight, R2, P),
        "horizon": (Kh, kitti[:4], Rh, Kh),
        "outside": (K, kitti, None, Pout),
    }
