"""CPU checks of the float64 references in oracle/banded_f64.py and of the acceptance criterion that
tests/test_gpu_wave_f64.py holds the wave solver to: the vectorised Thomas solve is LAPACK's answer, the reference on the
library's coefficients is the float64 smoother, the scalar-order float32 oracle meets the bar at every bucket geometry,
and the bar is tight enough to reject a 1 % error in the couplings across the chunk seams of any bucket (on the
seam guide, with varied couplings)."""
import numpy as np
import pytest
from scipy.linalg import solve_banded

import wave_f64_cases as wc
from oracle.banded_f64 import fgs_f64, fgs_f64_coeffs, thomas_f64

SEAM_SCALE = 0.99          # the seam defect the criterion must catch (1.0: no defect, and the self-test must fail)
SCALAR_BOUND = 2e-4        # e_scalar at every geometry and guide (measured: at most 9.6e-5)


@pytest.mark.parametrize("n,lines", [(1, 3), (2, 5), (7, 1), (300, 17), (4096, 4)])
def test_thomas_equals_solve_banded(n, lines):
    rng = np.random.default_rng(n + lines)
    sub = -rng.uniform(0, 5000, (n, lines))
    sup = -rng.uniform(0, 5000, (n, lines))
    sub[0] = 0; sup[-1] = 0
    diag = 1.0 - sub - sup + rng.uniform(0, 1, (n, lines))     # diagonally dominant, like I + lambda * L
    f = rng.normal(0, 1000, (n, lines, 2))                     # two right-hand sides per line
    got = thomas_f64(sub[:, :, None], diag[:, :, None], sup[:, :, None], f)
    for i in range(lines):
        ab = np.zeros((3, n))
        ab[0, 1:] = sup[:-1, i]
        ab[1] = diag[:, i]
        ab[2, :-1] = sub[1:, i]
        exp = solve_banded((1, 1), ab, f[:, i])
        assert np.abs(got[:, i] - exp).max() <= 1e-12 * np.abs(exp).max()


@pytest.mark.parametrize("h,w,gch", [(40, 70, 3), (6, 600, 1), (500, 9, 3)])
@pytest.mark.parametrize("lam,sigma,num_iter", [(8000.0, 1.5, 3), (100000.0, 20.0, 1), (500.0, 4.0, 5)])
def test_coeffs_reference_equals_fgs_f64(oracle, h, w, gch, lam, sigma, num_iter):
    """The two float64 smoothers differ only in their weights (the library's float32 table against float64 exp), so
    they agree to float32 resolution."""
    rng = np.random.default_rng(h * w)
    guide = rng.integers(0, 256, (h, w) if gch == 1 else (h, w, gch), dtype=np.uint8) // 8
    src = rng.normal(0, 1000, (h, w)).astype(np.float32)
    chor, cvert = oracle.weights(guide, sigma)
    got = fgs_f64_coeffs(chor, cvert, src, lam, 0.25, num_iter)
    exp = fgs_f64(guide, src, lam, sigma, 0.25, num_iter)
    assert np.abs(got - exp).max() <= 1e-6 * np.abs(src).max()
    # channels are independent systems with shared coefficients
    two = fgs_f64_coeffs(chor, cvert, np.stack([src, -2 * src], axis=2), lam, 0.25, num_iter)
    assert np.array_equal(two[:, :, 0], got) and np.allclose(two[:, :, 1], -2 * got, rtol=0, atol=1e-9 * np.abs(src).max())


def _passes32(oracle, chor, cvert, src, lam=wc.LAM, atten=wc.ATTEN, num_iter=wc.NUM_ITER):
    """The scalar-order oracle pass by pass (FGS.cpp:207-212) on given couplings, every channel of (h, w, cn)."""
    out = np.empty_like(src)
    for c in range(src.shape[2]):
        cur, lam_n = src[:, :, c], np.float32(lam)
        for _ in range(num_iter):
            cur, _ = oracle.hpass(cur, chor, lam_n)
            cur, _ = oracle.vpass(cur, cvert, lam_n)
            lam_n = np.float32(lam_n * np.float32(atten))
        out[:, :, c] = cur
    return out


def test_pass_composition_is_the_scalar_oracle(oracle):
    g = wc.GEOMS[8]
    guide, src, _, scal = wc.case(oracle, 8, "noisy", 1)
    chor, cvert = oracle.weights(guide, wc.SIGMA)
    assert np.array_equal(_passes32(oracle, chor, cvert, src), scal), g.id


@pytest.mark.parametrize("kind", wc.GUIDES)
@pytest.mark.parametrize("gi", range(len(wc.GEOMS)), ids=[g.id for g in wc.GEOMS])
def test_scalar_oracle_meets_the_criterion(oracle, gi, kind):
    """The float32 scalar order is the yardstick of the wave solver: it must itself sit close to the float64 solve of
    the same systems, at every geometry and guide the GPU file runs."""
    guide, src, ref, scal = wc.case(oracle, gi, kind, 1)
    e = wc.err(scal, ref, src)
    assert e.max() <= SCALAR_BOUND, (wc.GEOMS[gi].id, kind, e)


_SEAMED = [gi for gi, g in enumerate(wc.GEOMS) if len(g.separators())]     # (a 2-element line has no seam)


@pytest.mark.parametrize("kind", ["seam-ramp"])
@pytest.mark.parametrize("gi", _SEAMED, ids=[wc.GEOMS[gi].id for gi in _SEAMED])
def test_criterion_rejects_a_seam_defect(oracle, gi, kind):
    """Discrimination self-test: the scalar order run on couplings scaled by SEAM_SCALE at the bucket's chunk
    separators (elements l*M + M - 1 along the bucket's axis) -- the error a partitioned solver makes when it
    mishandles its seams -- must fail the criterion.  So the GPU test can see a seam error in every bucket.  (On the
    flat and ramp guides the smoothed solution has no jump at the seams for a coupling error to act on, and the same
    defect stays under even a 4x bound in most buckets: hence the seam guide.  Its flat-based twin runs on the GPU
    too, but under the flat factor, which is too wide to see a 1 % seam error.)"""
    g = wc.GEOMS[gi]
    sep = g.separators()
    guide, src, ref, scal = wc.case(oracle, gi, kind, 1)
    chor, cvert = oracle.weights(guide, wc.SIGMA)
    if g.axis == "row":
        chor = chor.copy(); chor[:, sep] *= np.float32(SEAM_SCALE)
    else:
        cvert = cvert.copy(); cvert[sep, :] *= np.float32(SEAM_SCALE)
    bad = _passes32(oracle, chor, cvert, src)
    e_bad, e_scalar = wc.err(bad, ref, src), wc.err(scal, ref, src)
    assert not wc.accepts(e_bad, e_scalar, wc.factor(kind)), \
        "criterion accepts a %.2f seam defect in %s/%s: e=%.3g, e_scalar=%.3g" % (SEAM_SCALE, g.id, kind, e_bad.max(), e_scalar.max())
