"""The wave solver (ADF_SOLVER_WAVE) bucket by bucket against a float64 solve of the same systems.

Window: the generic Fast Global Smoother on float32 sources runs the same run_passes as the WLS filter, with no
normalisation and no rounding, so solver errors show.  Every chunk-length bucket of the row pass (pick_row_bucket) and
of the column pass (launch_wave_vpass) runs at its shortest and longest length (tests/wave_f64_cases.py), with one
(R1), two (R2: the pair plane), three (R2+R1: pair and leftover) and four (R2x2) channels.

Criterion: e(x) = max|x - ref64| / max|src| per channel, e_wave <= factor * e_scalar + 1e-6, with factor 8 where the
couplings vary and 96 where they are exactly -lambda inside the chunks (measured ratios and the reason:
tests/wave_f64_cases.py).  tests/test_banded_f64.py shows on the CPU that the bound rejects a 1 % coupling error at the
seams of any bucket on the seam guide."""
import numpy as np
import pytest

import wave_f64_cases as wc

pytestmark = pytest.mark.gpu

R_IDS = {1: "R1", 2: "R2", 3: "R2+R1", 4: "R2x2"}
# every guide with pair + leftover; the R = 1, R = 2 and two-pair layouts on the noisy and seam guides
CASES = [(kind, 3) for kind in wc.GUIDES] + [(kind, cn) for kind in ("noisy", "seam-ramp") for cn in (1, 2, 4)]
GEOM_IDS = [g.id for g in wc.GEOMS]


def _smoother(adf, guide, lam=wc.LAM, atten=wc.ATTEN, num_iter=wc.NUM_ITER):
    from addingdisparityfiltering_amd.ximgproc import FastGlobalSmootherFilter

    f = FastGlobalSmootherFilter(guide, lam, wc.SIGMA, atten, num_iter, solver=adf.SOLVER_WAVE)
    assert f.getSolver() == adf.SOLVER_WAVE, "guide %s fell back to the exact solver" % (guide.shape,)
    return f


def _filter(f, src):
    """(h, w, cn) in, (h, w, cn) out; a single channel goes in as a 2-D image, as a caller passes it."""
    out = f.filter(src[:, :, 0] if src.shape[2] == 1 else src)
    return out.reshape(src.shape)


def _check(got, src, ref, scal, kind, what):
    e_wave, e_scalar = wc.err(got, ref, src), wc.err(scal, ref, src)
    k = wc.factor(kind)
    for c in range(src.shape[2]):
        assert wc.accepts(e_wave[c], e_scalar[c], k), "%s channel %d: e_wave=%.3g > %g * e_scalar(%.3g) + %g" % (
            what, c, e_wave[c], k, e_scalar[c], wc.FLOOR)


@pytest.mark.parametrize("kind,cn", CASES, ids=["%s-%s" % (k, R_IDS[cn]) for k, cn in CASES])
@pytest.mark.parametrize("gi", range(len(wc.GEOMS)), ids=GEOM_IDS)
def test_wave_bucket_against_float64(adf, oracle, gi, kind, cn):
    guide, src, ref, scal = wc.case(oracle, gi, kind, cn)
    f = _smoother(adf, guide)
    got = _filter(f, src)
    _check(got, src, ref, scal, kind, "%s/%s/%s" % (wc.GEOMS[gi].id, kind, R_IDS[cn]))
    assert np.array_equal(_filter(f, src), got), "a second call on the same handle gave other bits"


_PARAM_GEOMS = [gi for gi, g in enumerate(wc.GEOMS) if g.id in
                ("row-M60-1wave-n3840", "row-M64-2wave-n8192", "row-M8-1wave-n257", "col-M34-full-n2176",
                 "col-M34-half-n4352", "col-M4-full-n129")]


@pytest.mark.parametrize("lam,atten,num_iter", [(1e5, 0.25, 3), (8000.0, 1.0, 1), (8000.0, 0.25, 5)],
                         ids=["lam1e5", "iter1-att1", "iter5"])
@pytest.mark.parametrize("kind", ["noisy", "seam-ramp", "flat"])
@pytest.mark.parametrize("gi", _PARAM_GEOMS, ids=[wc.GEOMS[gi].id for gi in _PARAM_GEOMS])
def test_wave_parameters_against_float64(adf, oracle, gi, kind, lam, atten, num_iter):
    g = wc.GEOMS[gi]
    guide, src = wc.make_guide(g, kind), wc.make_source(g, 3)
    ref = wc.ref64(oracle, guide, src, lam, wc.SIGMA, atten, num_iter)
    scal = wc.scalar_fgs(oracle, guide, src, lam, wc.SIGMA, atten, num_iter)
    got = _filter(_smoother(adf, guide, lam, atten, num_iter), src)
    _check(got, src, ref, scal, kind, "%s/%s lambda=%g atten=%g iter=%d" % (g.id, kind, lam, atten, num_iter))


@pytest.mark.parametrize("cn", [1, 2, 3], ids=[R_IDS[c] for c in (1, 2, 3)])
@pytest.mark.parametrize("gi", range(len(wc.GEOMS)), ids=GEOM_IDS)
def test_wave_lambda_zero_is_the_identity(adf, gi, cn):
    """lambda = 0: every coupling is 0 and every pivot 1, so each pass must return its input bit for bit -- what is
    left is the data movement (LDS staging, pair-plane de-interleave, strips, pitch padding, empty chunks)."""
    g = wc.GEOMS[gi]
    src = wc.make_source(g, cn)
    got = _filter(_smoother(adf, wc.make_guide(g, "noisy"), lam=0.0), src)
    assert np.array_equal(got.view(np.uint32), src.view(np.uint32)), \
        "%s: %d elements moved" % (g.id, int((got != src).sum()))


def _as_int(src, dt):
    if dt == np.int16:
        return np.rint(src).astype(np.int16)                          # +-1e4 impulses, N(0, 1000) noise
    return np.rint(127.5 + src * (127.5 / np.abs(src).max())).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("dt,cn", [(np.int16, 1), (np.int16, 2), (np.uint8, 1), (np.uint8, 2)],
                         ids=["i16-R1", "i16-R2", "u8-R1", "u8-R2"])
@pytest.mark.parametrize("gi", range(len(wc.GEOMS)), ids=GEOM_IDS)
def test_wave_integer_epilogue_rounds_the_float_result(adf, gi, dt, cn):
    """The int16 / uint8 epilogues of the last column pass are the float32 one plus saturate(cvRound(x)) (round half to
    even): on the same handle, an integer source must give exactly the rounded float result of its float32 copy."""
    g = wc.GEOMS[gi]
    isrc = _as_int(wc.make_source(g, cn), dt)
    f = _smoother(adf, wc.make_guide(g, "ramp"))
    got = _filter(f, isrc)
    fl = _filter(f, isrc.astype(np.float32))
    info = np.iinfo(dt)
    exp = np.rint(fl).clip(info.min, info.max).astype(dt)
    assert got.dtype == dt
    bad = got != exp
    assert not bad.any(), "%s: %d of %d differ, e.g. got %s, float %r" % (
        g.id, int(bad.sum()), bad.size, got[bad][:4], fl[bad][:4])


@pytest.mark.parametrize("shape", [(2, 8193), (4353, 40), (1, 300), (300, 1)], ids=["8193cols", "4353rows", "1row", "1col"])
def test_wave_falls_back_to_exact_outside_its_range(adf, shape):
    """getSolver() reports what runs: beyond 8192 columns or 4352 rows, or with a single row or column, the handle runs
    the exact solver even if the wave solver was asked for; at the limits it runs the wave solver."""
    from addingdisparityfiltering_amd.ximgproc import FastGlobalSmootherFilter

    guide = np.zeros(shape + (3,), np.uint8)
    assert FastGlobalSmootherFilter(guide, 100.0, 1.5, solver=adf.SOLVER_WAVE).getSolver() == adf.SOLVER_EXACT
    assert FastGlobalSmootherFilter(guide, 100.0, 1.5, solver=adf.SOLVER_EXACT).getSolver() == adf.SOLVER_EXACT
    edge = tuple(min(s, lim) if s > lim else max(s, 2) for s, lim in zip(shape, (4352, 8192)))
    g2 = np.zeros(edge + (3,), np.uint8)
    assert FastGlobalSmootherFilter(g2, 100.0, 1.5, solver=adf.SOLVER_WAVE).getSolver() == adf.SOLVER_WAVE
