"""Independent float64 statement of the Fast Global Smoother (test infrastructure).

Not a restatement of the reference's code order: it builds the tridiagonal
systems (I + lambda_n * L_w) explicitly and solves them with LAPACK
(scipy.linalg.solve_banded) in float64.  Used to bound the float32 oracle's
error from a second, unrelated implementation.

Maths (FGS.cpp:50-59, :439-464, :674; EF.hpp:388-391):
  w_j   = exp(-sqrt(sum_c (g_j - g_{j+1})^2) / sigma)      weight between j and j+1
  a_j   = -lambda * w_{j-1},  c_j = -lambda * w_j,  b_j = 1 - a_j - c_j
  iteration n uses lambda_n = lambda * attenuation**n, H pass then V pass.
"""
import numpy as np
from scipy.linalg import solve_banded


def edge_weights_f64(guide, sigma):
    g = np.asarray(guide).astype(np.float64)
    if g.ndim == 2:
        g = g[:, :, None]
    dh = np.sqrt(((g[:, :-1] - g[:, 1:]) ** 2).sum(axis=2))
    dv = np.sqrt(((g[:-1, :] - g[1:, :]) ** 2).sum(axis=2))
    wh = np.zeros(g.shape[:2])
    wv = np.zeros(g.shape[:2])
    wh[:, :-1] = np.exp(-dh / sigma)
    wv[:-1, :] = np.exp(-dv / sigma)
    return wh, wv  # positive weights; last column / row zero


def _solve_lines(w_lines, f_lines, lam):
    """Solve (I + lam*L_w) x = f for each line (axis 1 is the scanline)."""
    out = np.empty_like(f_lines)
    n = w_lines.shape[1]
    ab = np.zeros((3, n))
    for i in range(w_lines.shape[0]):
        w = w_lines[i]
        c = -lam * w            # super-diagonal, c[n-1] == 0
        a = np.zeros(n)
        a[1:] = -lam * w[:-1]   # sub-diagonal
        ab[0, 1:] = c[:-1]
        ab[1] = 1.0 - a - c
        ab[2, :-1] = a[1:]
        out[i] = solve_banded((1, 1), ab, f_lines[i])
    return out


def fgs_f64(guide, src, lam, sigma, atten=0.25, num_iter=3):
    """float64 FGS of a single-channel image `src` (h, w)."""
    wh, wv = edge_weights_f64(guide, sigma)
    u = np.asarray(src, np.float64).copy()
    # the reference multiplies lambda by a float32 attenuation in float32 (FGS.cpp:146-147,211)
    lam_n = np.float32(lam)
    att = np.float32(atten)
    for _ in range(num_iter):
        u = _solve_lines(wh, u, float(lam_n))
        u = _solve_lines(wv.T.copy(), u.T.copy(), float(lam_n)).T.copy()
        lam_n = np.float32(lam_n * att)
    return u


def thomas_f64(sub, diag, sup, f):
    """float64 Thomas solve of many tridiagonal systems at once, along axis 0.

    Row j of every system reads  sub[j]*x[j-1] + diag[j]*x[j] + sup[j]*x[j+1] = f[j]  (sub[0] and
    sup[n-1] are ignored).  The coefficient arrays broadcast against `f` on the trailing (line) axes,
    so one Python loop over the length solves every line of a pass with numpy.  No pivoting: meant for
    the diagonally dominant systems of the smoother."""
    f = np.asarray(f, np.float64)
    sub, diag, sup = (np.asarray(a, np.float64) for a in (sub, diag, sup))
    n = f.shape[0]
    x = np.empty(np.broadcast_shapes(f.shape, diag.shape, sub.shape, sup.shape))
    d = np.empty_like(x)                      # sup[j] / pivot[j]
    piv = diag[0] + np.zeros_like(x[0])
    d[0] = sup[0] / piv
    x[0] = f[0] / piv
    for j in range(1, n):
        piv = diag[j] - sub[j] * d[j - 1]
        d[j] = sup[j] / piv
        x[j] = (f[j] - sub[j] * x[j - 1]) / piv
    for j in range(n - 2, -1, -1):
        x[j] -= d[j] * x[j + 1]
    return x


def _solve_coupled(c, f):
    """(I + L) x = f along axis 0, where c[j] (<= 0) couples j and j+1: off-diagonals c[j-1] and c[j],
    diagonal 1 - c[j-1] - c[j] (FGS.cpp:439-464 forms exactly these terms; c[n-1] enters the last
    diagonal as given -- the weights store 0 there)."""
    prev = np.concatenate([np.zeros_like(c[:1]), c[:-1]])
    return thomas_f64(prev, 1.0 - prev - c, c, f)


def fgs_f64_coeffs(chor, cvert, src, lam, atten=0.25, num_iter=3):
    """float64 FGS on the library's own float32 coefficients.

    chor / cvert: the float32 couplings of oracle.weights(guide, sigma) (table entries -exp(-d/sigma),
    (h, w)).  src: (h, w) or (h, w, cn), every channel filtered with the same weights.  Each pass uses
    float32(lambda_n * C) with lambda_n attenuated in float32 as FGS.cpp:146-147,211 do, so this solves
    the very systems the float32 solvers solve; only the solve itself runs in float64."""
    chor = np.asarray(chor, np.float32)
    cvert = np.asarray(cvert, np.float32)
    u = np.asarray(src, np.float64)
    flat = u.ndim == 2
    if flat:
        u = u[:, :, None]
    lam_n, att = np.float32(lam), np.float32(atten)
    for _ in range(num_iter):
        ch = (lam_n * chor).astype(np.float64)       # float32 products, as the solvers form them
        cv = (lam_n * cvert).astype(np.float64)
        u = _solve_coupled(ch.T[:, :, None], u.transpose(1, 0, 2)).transpose(1, 0, 2)   # row pass (FGS.cpp:209)
        u = _solve_coupled(cv[:, :, None], u)                                           # column pass (:210)
        lam_n = np.float32(lam_n * att)
    return u[:, :, 0] if flat else u
