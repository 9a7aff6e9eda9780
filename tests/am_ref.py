"""The adaptive manifold filter (amFilter) as a direct NumPy statement of the library's definition (include/adf_wls.h,
"adaptive manifold filter"): what csrc/am_filter_kernels.hip is held to bit for bit.

am_filter(joint, src, plan, jtab, adjust_outliers, dst_dtype) takes the plan and the joint table as ARGUMENTS (the
library's adf_am_plan_host / amPlan, or plan() below, which restates the formulas).  Every + - * / sqrt is one float32
operation on float32 arrays, rounded once; the sweeps are explicit loops along the scanline, vectorised across scanlines;
am_exp is composed of float32 operations only.  `real=True` evaluates the same formulas in float64 with libm's exp
(tests/test_am_ref.py measures the statement against it).
"""
import math

import numpy as np

f32 = np.float32
LOG2E = f32(1.4426950408889634)
LN2 = 0.6931471805599453
EXP_C = [f32(LN2 ** k / math.factorial(k)) for k in range(8)]     # c_k = (float)(ln2^k / k!)
MAX_TREE_HEIGHT = 8
PCA_SCALE = f32(2.0 ** 30)


def am_exp(x):
    """exp(x) for x <= 0 in float32 operations: t = x * LOG2E, n = floor(t + 0.5), f = t - n, p = Horner form of degree 7
    in f (multiply, then add), p * 2^n with 2^n built from bits; 0 where n < -126 (or x is not a number)."""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * LOG2E
        n = np.floor(t + f32(0.5))
        f = t - n
        p = np.full(x.shape, EXP_C[7], f32)
        for k in range(6, -1, -1):
            p = p * f + EXP_C[k]
        ok = n >= f32(-126)
        e = ((np.where(ok, n, f32(0)).astype(np.int32) + 127) << 23).astype(np.uint32).view(f32)
        return np.where(ok, p * e, f32(0)).astype(f32)


def cv_round(v):
    """cvRound of a double: to nearest, ties to even."""
    return int(np.rint(np.float64(v)))


def plan(sigma_s, sigma_r, tree_height, W, H):
    """The plan's formulas (include/adf_wls.h) restated: a dict with the fields of amPlan."""
    sigma_s, sigma_r = float(sigma_s), float(sigma_r)
    df = max(1.0, 2.0 ** math.floor(math.log(min(sigma_s / 4.0, 256.0 * sigma_r)) / math.log(2.0)))
    height = tree_height if tree_height > 0 else max(2, int(math.ceil((math.floor(math.log(sigma_s) / math.log(2.0)) - 1.0) * (1.0 - sigma_r))))
    sr2 = f32(sigma_r / math.sqrt(2.0))
    ss = f32(sigma_s / df)
    q = f32(ss / sr2)
    return dict(df=int(df), height=int(height), sh=cv_round(H * (1.0 / df)), sw=cv_round(W * (1.0 / df)), manifolds=2 ** int(height) - 1,
                a_root=f32(math.exp(-math.sqrt(2.0) / sigma_s)), a_child=f32(math.exp(-math.sqrt(2.0) / (sigma_s / df))),
                sr2=sr2, argW=f32(f32(-0.5) / f32(sr2 * sr2)), ss=ss, ratio=f32(q * q), lnA=f32(-math.sqrt(2.0) / float(ss)),
                argOut=f32(-0.5 / (sigma_r * sigma_r)))


def joint_table():
    return np.array([f32(v / 255.0) for v in range(256)], f32)


def taps_x(n_dst, scale, n_src):
    """Column taps of cv::resize INTER_LINEAR (csrc/resize_kernels.hip): (s0, s1, 1 - fx, fx); a tap that would leave the
    row has weight (1, 0)."""
    fx = ((np.arange(n_dst, dtype=np.float64) + 0.5) * np.float64(scale) - 0.5).astype(f32)
    s = np.floor(fx)
    fx = (fx - s).astype(f32)
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= n_src - 1
    fx = np.where(lo | hi, f32(0), fx).astype(f32)
    s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    return s, np.minimum(s + 1, n_src - 1), (f32(1) - fx).astype(f32), fx


def taps_y(n_dst, scale, n_src):
    """Row taps: the rows are clamped, the weights are not."""
    fy = ((np.arange(n_dst, dtype=np.float64) + 0.5) * np.float64(scale) - 0.5).astype(f32)
    s = np.floor(fy)
    fy = (fy - s).astype(f32)
    s = s.astype(np.int64)
    return np.clip(s, 0, n_src - 1), np.clip(s + 1, 0, n_src - 1), (f32(1) - fy).astype(f32), fy


def resize(P, dh, dw, scale_x, scale_y):
    """Row blend first, then column blend (the statement of csrc/resize_kernels.hip's header)."""
    sh, sw = P.shape
    x0, x1, a0, a1 = taps_x(dw, scale_x, sw)
    y0, y1, b0, b1 = taps_y(dh, scale_y, sh)
    hr = P[:, x0] * a0 + P[:, x1] * a1
    return hr[y0] * b0[:, None] + hr[y1] * b1[:, None]


def sweep(P, ah, av):
    """In place: rows left to right and right to left, then columns down and up.  ah, av: arrays or constants."""
    h, w = P.shape
    ah = np.broadcast_to(ah, (h, max(w - 1, 0))) if np.ndim(ah) == 0 else ah
    av = np.broadcast_to(av, (max(h - 1, 0), w)) if np.ndim(av) == 0 else av
    for j in range(1, w):
        P[:, j] = P[:, j] + ah[:, j - 1] * (P[:, j - 1] - P[:, j])
    for j in range(w - 2, -1, -1):
        P[:, j] = P[:, j] + ah[:, j] * (P[:, j + 1] - P[:, j])
    for i in range(1, h):
        P[i] = P[i] + av[i - 1] * (P[i - 1] - P[i])
    for i in range(h - 2, -1, -1):
        P[i] = P[i] + av[i] * (P[i + 1] - P[i])
    return P


def div0(a, b):
    """a / b, 0 where b == 0 (cv::divide's rule)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b == 0, a.dtype.type(0), a / np.where(b == 0, a.dtype.type(1), b)).astype(a.dtype)


def convert(x, dtype):
    """Round half to even and saturate; float32 as it is; a NaN gives the depth's minimum."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return x.astype(f32)
    lo, hi = (0.0, 255.0) if dtype == np.uint8 else (-32768.0, 32767.0)
    with np.errstate(invalid="ignore"):
        v = np.rint(x.astype(np.float64))
        return np.where(np.isnan(v), lo, np.clip(v, lo, hi)).astype(dtype)


def am_filter(joint, src, p, jtab=None, adjust_outliers=False, dst_dtype=None, real=False, parts=False):
    """joint (H,W) or (H,W,3) uint8; src (H,W) uint8, int16 or float32; p: the plan (amPlan / plan()).  Returns dst, or
    with parts=True (g before conversion, num, den, mind)."""
    T = np.float64 if real else f32
    ex = (lambda x: np.exp(np.asarray(x, np.float64))) if real else am_exp
    H, W = src.shape
    jtab = joint_table() if jtab is None else np.asarray(jtab, f32)
    joint = joint.reshape(H, W, -1)
    C = joint.shape[2]
    J = [jtab[joint[:, :, c]].astype(T) for c in range(C)]
    f = src.astype(f32).astype(T)
    df, height, sh, sw = int(p["df"]), int(p["height"]), int(p["sh"]), int(p["sw"])
    a_root, a_child, argW, ratio, lnA, argOut = (T(p[k]) for k in ("a_root", "a_child", "argW", "ratio", "lnA", "argOut"))
    one = T(1)

    def down(P):
        return resize(P, sh, sw, float(df), float(df))

    def up(P):
        return resize(P, H, W, sw / W, sh / H)

    st = dict(num=np.zeros((H, W), T), den=np.zeros((H, W), T), mind=None)

    def node(eta, cluster, level):
        if eta[0].shape == (H, W) and level == 1:
            etaF, eta = eta, [down(e) for e in eta]
        else:
            etaF = [up(e) for e in eta]
        d2 = None
        for c in range(C):
            e = etaF[c] - J[c]
            d2 = e * e if d2 is None else d2 + e * e
        w = ex(d2 * argW).astype(T)
        if adjust_outliers:
            st["mind"] = d2 if level == 1 else np.minimum(st["mind"], d2)
        psi, psi0 = down(f * w), down(w)
        dh = dv = None
        for c in range(C):
            h_ = eta[c][:, :-1] - eta[c][:, 1:]
            v_ = eta[c][:-1] - eta[c][1:]
            dh = h_ * h_ if dh is None else dh + h_ * h_
            dv = v_ * v_ if dv is None else dv + v_ * v_
        ah = ex(np.sqrt(dh * ratio + one) * lnA).astype(T)
        av = ex(np.sqrt(dv * ratio + one) * lnA).astype(T)
        sweep(psi, ah, av)
        sweep(psi0, ah, av)
        st["num"] = st["num"] + up(psi) * w
        st["den"] = st["den"] + up(psi0) * w
        if level >= height:
            return
        X = [J[c] - etaF[c] for c in range(C)]
        if C == 1:
            o = X[0]
        else:
            m = T(0.5) * X[0]
            m = m + T(-0.5) * X[1]
            m = m + T(0.5) * X[2]
            m = np.where(cluster, m, T(0))
            if real:
                sd = np.array([np.sum(m * X[c]) for c in range(3)], np.float64)
            else:
                S = [np.rint((m * X[c]) * PCA_SCALE).astype(np.int64).sum() for c in range(3)]
                sd = np.array(S, np.int64).astype(np.float64) * np.float64(2.0 ** -30)
            norm = np.sqrt(sd[0] * sd[0] + sd[1] * sd[1] + sd[2] * sd[2])
            vec = (sd / norm).astype(T) if norm != 0 else np.zeros(3, T)
            o = vec[0] * X[0]
            o = o + vec[1] * X[1]
            o = o + vec[2] * X[2]
        children = []
        for member in (cluster & (o < 0), cluster & (o >= 0)):
            tm = np.where(member, one - w, T(0))
            tb = sweep(down(tm), a_child, a_child)
            children.append(([div0(sweep(down(tm * J[c]), a_child, a_child), tb) for c in range(C)], member))
        for eta_c, member in children:
            node(eta_c, member, level + 1)

    node([sweep(j.copy(), a_root, a_root) for j in J], np.ones((H, W), bool), 1)
    g = div0(st["num"], st["den"])
    if adjust_outliers:
        alpha = ex(st["mind"] * argOut).astype(T)
        g = alpha * (g - f) + f
    if parts:
        return g, st["num"], st["den"], st["mind"]
    return convert(g, src.dtype if dst_dtype is None else dst_dtype)
