"""The down-scaled call (DF.cpp:224-277) on values that saturate, on strided device maps and on a chunked strided batch.

A. Saturating values.  Plateau maps (tests/scaled_cases.py; confidence positive where the values are extreme, proved on
   the oracle by tests/test_scaled_cases.py) at every shape of CASES: the exact solver and the confidence map equal the
   oracle bit for bit; the wave solver gives the same bits whether its first row pass interpolates the maps itself or
   the resize kernels do, and in the half-width form; the float map rounds to the int16 map.  No distance between the
   wave solver and the oracle is asserted on this data: its rounding at magnitudes of 3e4 has no established bar, and
   the exact relations need none.  Without confidence, per-pixel limit values reach every output pixel: the exact
   solver equals the oracle, the wave solver equals a same-size wave call on the oracle's resized map.
B. Device maps that are slices of wider tensors (odd element offsets, padded rows, padded pairs, padding filled with
   12345): the same bits as dense copies, nothing written outside the output slice.
C. The same layout on a batch that the workspace limit cuts into chunks."""
import numpy as np
import pytest

import scaled_cases as sc
from addingdisparityfiltering_amd import synthetic
from test_gpu_float_output import _sat16
from test_scaled_path import _filter_with_env

pytestmark = pytest.mark.gpu

_CASE_IDS = [sc.case_id(c) for c in sc.CASES]
_expected = {}


def _oracle_case(oracle, i):
    """(view, dl, dr, filtered map, confidence map) of CASES[i], computed once."""
    if i not in _expected:
        c = sc.CASES[i]
        view, dl, dr = sc.case_inputs(c)
        p = oracle.default_params(sigma_color=1.5, threads=8, disc_radius=c.radius)
        exp, exp_conf = oracle.wls_filter_scaled(dl, view, dr, c.roi, p)
        for a in (view, dl, dr, exp, exp_conf):
            a.setflags(write=False)
        _expected[i] = (view, dl, dr, exp, exp_conf)
    return _expected[i]


def _setup(adf, f, solver, radius):
    f.setSolver(solver); f.setSigmaColor(1.5); f.setDepthDiscontinuityRadius(radius)
    return f


def _float_relation(f, dl, view, dr, roi, i16, hi, where):
    """sat16(filterFloat) == filter on handle `f`, finite, -16.0 outside the view-coordinate ROI `hi`."""
    path = f.getLastPath()
    f32 = f.filterFloat(dl, view, None, dr, roi)
    assert f.getLastPath() == path, where
    assert f32.dtype == np.float32 and f32.shape == i16.shape, where
    assert np.isfinite(f32).all(), "%s: NaN or inf in the float map" % where
    bad = _sat16(f32) != i16
    assert not bad.any(), "%s: %d pixels break sat16(f32) == i16, e.g. f32 %r i16 %r" % (where, int(bad.sum()), f32[bad][:4], i16[bad][:4])
    assert np.all(f32[~sc.inside(f32.shape, hi)] == np.float32(-16.0)), "%s: not -16.0 outside the ROI" % where
    return f32


# ---------------------------------------------------------------------------------------------
# A. with confidence: plateau maps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=_CASE_IDS)
def test_plateaus_exact_solver_equals_the_oracle(adf, oracle, i):
    c = sc.CASES[i]
    view, dl, dr, exp, exp_conf = _oracle_case(oracle, i)
    f = _setup(adf, adf.createDisparityWLSFilterGeneric(True), adf.SOLVER_EXACT, c.radius)
    got = f.filter(dl, view, None, dr, c.roi)
    assert f.getLastSolver() == adf.SOLVER_EXACT and not f.getLastPath() & adf.PATH_SCALED_FUSED
    assert f.getROI() == c.roi
    assert np.array_equal(f.getConfidenceMap(), exp_conf)
    bad = got != exp
    assert not bad.any(), "%d pixels differ, e.g. got %r expected %r" % (int(bad.sum()), got[bad][:4], exp[bad][:4])
    _float_relation(f, dl, view, dr, c.roi, got, sc.hi_roi(c.roi, c.view, c.maps), "exact")


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=_CASE_IDS)
def test_plateaus_fused_first_pass_equals_the_resize_kernels(adf, oracle, i):
    """Same solver, exact prologue: the wave solver fed by the fused low-resolution prologue, by its half-width form
    and by the two resize kernels gives identical maps, saturated values included; the path flags say which form ran;
    each form's float map rounds to its int16 map."""
    c = sc.CASES[i]
    view, dl, dr, _, exp_conf = _oracle_case(oracle, i)
    hi = sc.hi_roi(c.roi, c.view, c.maps)

    def run(f):
        _setup(adf, f, adf.SOLVER_WAVE, c.radius)
        out = f.filter(dl, view, None, dr, c.roi)
        path, solver = f.getLastPath(), f.getLastSolver()
        conf = f.getConfidenceMap()
        f32 = _float_relation(f, dl, view, dr, c.roi, out, hi, "wave path %d" % path)
        return (out, f32), path, conf, solver

    (fused, fused32), pf, cf, sf = _filter_with_env(adf, {"ADF_SCALED_FUSE": "1", "ADF_LO_HALF": "1"}, run)
    (plain, plain32), pp, cp, sp = _filter_with_env(adf, {"ADF_SCALED_FUSE": "0"}, run)
    assert sf == sp == adf.SOLVER_WAVE
    assert bool(pf & adf.PATH_SCALED_FUSED) == c.fused, pf
    assert bool(pf & adf.PATH_SCALED_HALF) == c.half, pf
    assert not pp & (adf.PATH_SCALED_FUSED | adf.PATH_SCALED_HALF), pp
    bad, bad32 = fused != plain, fused32.view(np.uint32) != plain32.view(np.uint32)     # the int16 maps, the float maps
    assert not bad.any() and not bad32.any(), "%d int16 / %d float pixels differ, e.g. fused %r resize kernels %r" % (
        int(bad.sum()), int(bad32.sum()), fused32[bad32][:4], plain32[bad32][:4])
    assert np.array_equal(cf, cp) and np.array_equal(cf, exp_conf)
    if c.half:
        (gen, gen32), pg, cg, _ = _filter_with_env(adf, {"ADF_SCALED_FUSE": "1", "ADF_LO_HALF": "0"}, run)
        assert pg & adf.PATH_SCALED_FUSED and not pg & adf.PATH_SCALED_HALF, pg
        assert np.array_equal(gen, fused) and np.array_equal(cg, cf)
        assert np.array_equal(gen32.view(np.uint32), fused32.view(np.uint32))
    # the data does what it was made for: the map reaches both ends of the int16 range inside the ROI
    if c.maps[0] < c.view[0]:
        inside = fused[sc.inside(fused.shape, hi)]
        assert inside.max() > 30000 and inside.min() < -30000


# ---------------------------------------------------------------------------------------------
# A. without confidence: per-pixel limit values, all three instantiations of the resize kernel
# ---------------------------------------------------------------------------------------------
_LIMIT_CASES = [
    # view, maps, ROI of the maps, channels
    ((320, 240), (160, 120), (3, 1, 155, 118), 3),       # 0.5: VEC
    ((321, 243), (107, 81), (0, 0, 107, 81), 1),         # a third: VEC, odd sizes, the whole map
    ((320, 240), (224, 168), (10, 2, 210, 164), 3),      # 0.7: UP without VEC
    ((320, 240), (288, 216), (9, 0, 279, 216), 1),       # 0.9: the general form
    ((320, 240), (400, 300), (20, 5, 375, 290), 3),      # 1.25: a reduction, post_scale 0.8
]


@pytest.mark.parametrize("case", _LIMIT_CASES, ids=["0.5", "third", "0.7", "0.9", "1.25"])
def test_limit_values_without_confidence(adf, oracle, case):
    (W, H), (mw, mh), roi, ch = case
    view = synthetic.make_artificial_example(W, H, ch, seed=W + mw)[0]
    dl = sc.limits(np.random.default_rng(mw + mh), mh, mw)
    hi = sc.hi_roi(roi, (W, H), (mw, mh))
    resized = oracle.resize_linear(dl, (W, H), post_scale=float(sc.x_ratio((W, H), (mw, mh))))
    if mw < W:
        assert (resized == 32767).any() and (resized == -32768).any()        # both clamp directions occur
    else:
        # a reduction multiplies by x_ratio < 1 after the first saturate_cast: neither clamp can be reached
        assert np.abs(resized.astype(np.int64)).max() <= 32768 * W // mw + 1
    p = oracle.default_params(sigma_color=1.5, threads=8, use_confidence=0)
    exp, _ = oracle.wls_filter_scaled(dl, view, None, roi, p)
    f = adf.createDisparityWLSFilterGeneric(False)
    f.setSolver(adf.SOLVER_EXACT); f.setSigmaColor(1.5)
    got = f.filter(dl, view, None, None, roi)
    assert f.getROI() == roi
    bad = got != exp
    assert not bad.any(), "%d pixels differ, e.g. got %r expected %r" % (int(bad.sum()), got[bad][:4], exp[bad][:4])
    _float_relation(f, dl, view, None, roi, got, hi, "exact")
    # the wave solver: the scaled call hands exactly the resized map to the passes of a same-size call
    f.setSolver(adf.SOLVER_WAVE)
    scaled = f.filter(dl, view, None, None, roi)
    assert f.getLastSolver() == adf.SOLVER_WAVE and not f.getLastPath() & adf.PATH_SCALED_FUSED
    _float_relation(f, dl, view, None, roi, scaled, hi, "wave")
    g = adf.createDisparityWLSFilterGeneric(False)
    g.setSolver(adf.SOLVER_WAVE); g.setSigmaColor(1.5)
    same = g.filter(resized, view, None, None, hi)
    assert g.getLastSolver() == adf.SOLVER_WAVE
    bad = scaled != same
    assert not bad.any(), "%d pixels differ, e.g. scaled %r same-size %r" % (int(bad.sum()), scaled[bad][:4], same[bad][:4])


# ---------------------------------------------------------------------------------------------
# B. strided and offset device maps
# ---------------------------------------------------------------------------------------------
PAD = 12345          # around the maps: an element read from the wrong side of a row boundary changes the result
SENTINEL = 7777      # around the output


def _slice_of_wider(torch, dev, a, off, extra, fill):
    """Device copy of the (N, H, W[, C]) array `a` as the slice [:, :H, off:off + W] of a tensor that is `extra`
    elements wider and one row taller (so pairs lie more than a frame apart), filled with `fill` elsewhere."""
    n, h, w = a.shape[:3]
    buf = torch.full((n, h + 1, w + off + extra) + tuple(a.shape[3:]), fill, dtype={np.int16: torch.int16, np.uint8: torch.uint8}[a.dtype.type], device=dev)
    view = buf[:, :h, off:off + w]
    view.copy_(torch.from_numpy(a))
    assert not view.is_contiguous() and view.stride(0) > h * view.stride(1)
    return view


def _batch(n, W, H, mw, mh, ch, seed):
    view = np.stack([synthetic.make_artificial_example(W, H, ch, seed=seed + 10 * k)[0] for k in range(n)])
    maps = [synthetic.make_artificial_example(mw, mh, 1, seed=seed + 10 * k + 1) for k in range(n)]
    return view, np.stack([m[1] for m in maps]), np.stack([m[2] for m in maps])


_STRIDED_FORMS = {
    # view, maps, ROI of the maps, channels, radius, fused?, half-width form?
    "general": ((320, 240), (160, 120), (0, 0, 160, 120), 1, 2, True, False),
    "half": ((320, 240), (160, 120), (16, 0, 144, 120), 3, 2, True, True),
    "unfused-0.7": ((320, 240), (224, 168), (10, 0, 214, 168), 3, 2, False, False),
    # the ROI ends flush with the maps' last column, 161 elements under a 322-wide view: the last lanes' vectors would
    # cross the row's end and are fetched element by element -- behind the row lies PAD
    "flush-half": ((322, 240), (161, 120), (9, 0, 152, 120), 3, 2, True, True),
    "flush-general": ((322, 240), (161, 120), (0, 0, 161, 120), 1, 2, True, False),
}


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("form", list(_STRIDED_FORMS))
def test_strided_device_maps_equal_dense_copies(adf, oracle, form, off):
    import torch

    (W, H), (mw, mh), roi, ch, radius, want_fused, want_half = _STRIDED_FORMS[form]
    n = 3
    dev = torch.device("cuda", 0)
    view, dl, dr = _batch(n, W, H, mw, mh, ch, seed=500 + off + len(form))
    tl = _slice_of_wider(torch, dev, dl, off, 4, PAD)                    # rows an odd number of elements apart where mw is even
    tr = _slice_of_wider(torch, dev, dr, 4 - off, 9, PAD)                # another offset, another width
    tv = _slice_of_wider(torch, dev, view, 2, 5, 99)
    assert tl.stride(1) != tr.stride(1) and (tl.data_ptr() // 2) % 2 == off % 2
    hi = sc.hi_roi(roi, (W, H), (mw, mh))
    expected = [oracle.wls_filter_scaled(dl[k], view[k], dr[k], roi, oracle.default_params(sigma_color=1.5, threads=8, disc_radius=radius))
                for k in range(n)]
    for solver in (adf.SOLVER_WAVE, adf.SOLVER_EXACT):
        f = _setup(adf, adf.createDisparityWLSFilterGeneric(True), solver, radius)
        obuf = torch.full((n, H + 2, W + 6), SENTINEL, dtype=torch.int16, device=dev)
        out = obuf[:, 1:H + 1, 3:3 + W]
        assert f.filter(tl, tv, out, tr, roi) is out
        path = f.getLastPath()
        conf = f.getConfidenceMap().cpu().numpy()
        got = out.cpu().numpy()
        if solver == adf.SOLVER_WAVE:
            assert bool(path & adf.PATH_SCALED_FUSED) == want_fused and bool(path & adf.PATH_SCALED_HALF) == want_half, path
        obuf[:, 1:H + 1, 3:3 + W] = SENTINEL
        assert bool((obuf == SENTINEL).all()), "written outside the output slice"
        dense = f.filter(tl.contiguous(), tv.contiguous(), None, tr.contiguous(), roi)
        assert f.getLastPath() == path
        assert np.array_equal(got, dense.cpu().numpy())                  # the same handle on dense copies
        assert np.array_equal(conf, f.getConfidenceMap().cpu().numpy())
        assert np.all(got[~sc.inside(got.shape, hi)] == -16)
        for k in range(n):
            exp, exp_conf = expected[k]
            assert np.array_equal(conf[k], exp_conf), "pair %d" % k
            if solver == adf.SOLVER_EXACT:
                assert np.array_equal(got[k], exp), "pair %d" % k
            else:
                d = np.abs(got[k].astype(np.int64) - exp)
                assert d.max() <= 1 and d.mean() <= 1 / 256, (k, d.max(), d.mean())


# ---------------------------------------------------------------------------------------------
# C. a strided batch cut into workspace chunks
# ---------------------------------------------------------------------------------------------
def test_chunked_strided_batch_equals_the_unchunked_dense_call(adf):
    """Each chunk's first pass must address its own pairs through the caller's pair stride."""
    import torch

    n, W, H = 5, 512, 256
    dev = torch.device("cuda", 0)
    view, dl, dr = _batch(n, W, H, W // 2, H // 2, 3, seed=900)
    roi = (19, 0, W // 2 - 19, H // 2)
    tl = _slice_of_wider(torch, dev, dl, 1, 4, PAD)
    tr = _slice_of_wider(torch, dev, dr, 3, 9, PAD)
    tv = _slice_of_wider(torch, dev, view, 2, 5, 99)

    def run(l, v, r):
        def go(f):
            _setup(adf, f, adf.SOLVER_WAVE, 5)
            out = f.filter(l, v, None, r, roi)
            return f, out.cpu().numpy(), f.getLastPath(), f.getConfidenceMap().cpu().numpy()
        return go

    f1, whole, p1, c1 = _filter_with_env(adf, {}, run(tl.contiguous(), tv.contiguous(), tr.contiguous()))
    per_pair = f1.workspaceBytes() / n
    f2, chunked, p2, c2 = _filter_with_env(adf, {"ADF_WS_LIMIT_GB": "%.6f" % (2.2 * per_pair / 2 ** 30)}, run(tl, tv, tr))
    assert f2.workspaceBytes() < f1.workspaceBytes()                     # the limit did cut the batch: fewer pairs' planes
    assert p1 & adf.PATH_SCALED_FUSED and p2 & adf.PATH_SCALED_FUSED
    assert np.array_equal(chunked, whole)
    assert np.array_equal(c2, c1)
    assert all(not np.array_equal(whole[k], whole[0]) for k in range(1, n))   # (the pairs differ: a wrong pair shows)
