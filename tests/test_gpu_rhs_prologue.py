"""The kernels that write the right-hand sides of the solve as planes (csrc/rhs_prologue.hip: plain_prologue_kernel,
lrc_prologue_kernel; csrc/conf_kernels.hip: conf_left_kernel<R, true>), one case per kernel and plane layout
(ORIENT_N, ORIENT_PAIR, ORIENT_T of adf_internal.h), each pinned to its kernel by getLastSolver / getLastPath (the
smoother: getSolver) and compared with the oracle bit for bit.

Bit for bit on both solvers: the exact solver reproduces the oracle's order, so its cases run with the default
lambda.  The wave solver re-associates the solve (tests/test_gpu_wave.py: within 1 LSB), so its cases run with
lambda = 0: the system is the identity, every pass returns its right-hand side unchanged, and the output is the
stored planes through the same epilogue the oracle applies -- a value stored in the wrong place, or not stored, is a
wrong output pixel, not a difference below a tolerance.

Shapes: the prologue tile is 64 x 32 pixels.  An ROI of 65 x 33 is one full tile and a one-pixel partial tile each
way (the LRC kernel tiles the frame, not the ROI: in a frame of 80 x 40 with the ROI at (8, 4) the ROI crosses the
tile boundary at frame column 64 and its first tile starts outside it); an ROI of 2 x 2; an ROI at the unaligned
offset (13, 7) of a 96 x 80 frame; and for the exact solver the one-pixel-wide ROIs 1 x 80 and 96 x 1 (the wave
solver takes ROIs from 2 x 2).  The smoother has no ROI: its images are 65 x 33 and 2 x 2 (exact: also 1 x 80, 96 x 1).
Two of the cases exist only where the wave solver's first row pass cannot form the right-hand sides itself, and it
refuses by geometry only for rows shorter than 4 pixels (wave_hpass_can_fuse, fgs_wave_h.hip): those run the 2 x 2
ROI and an ROI of 3 x 33 (a partial tile across, a full tile and one row down)."""
import numpy as np
import pytest

from addingdisparityfiltering_amd import synthetic

pytestmark = pytest.mark.gpu

# (frame W, H), ROI (x, y, w, h)
TILE = ((80, 40), (8, 4, 65, 33))
TINY = ((24, 16), (6, 5, 2, 2))
OFFSET = ((96, 80), (13, 7, 70, 41))
COLUMN = ((96, 80), (95, 0, 1, 80))       # exact solver only
ROW = ((96, 80), (0, 79, 96, 1))          # exact solver only
NARROW = ((24, 40), (6, 3, 3, 33))        # rows the first row pass cannot fuse
WAVE_SHAPES = [TILE, TINY, OFFSET]
EXACT_SHAPES = [TILE, TINY, OFFSET, COLUMN, ROW]
UNFUSED_SHAPES = [TINY, NARROW]
SIGMA = 1.5


def _ids(shapes):
    return ["%dx%d@%d,%d" % (r[2], r[3], r[0], r[1]) for _, r in shapes]


def _pair(frame, seed, scale=1):
    """(view, dl, dr) of a frame; scale: the view's size as a multiple of the maps' (down-scaled calls), or 1/2."""
    w, h = frame
    _, dl, dr, _ = synthetic.make_artificial_example(w, h, 1, seed=seed)
    view = synthetic.make_artificial_example(int(w * scale), int(h * scale), 3, seed=seed + 1)[0]
    return view, dl, dr


def _lam(adf, solver):
    return 0.0 if solver == adf.SOLVER_WAVE else 8000.0


def _wls(adf, oracle, solver, frame, roi, use_conf=True, radius=5, scale=1, seed=0):
    """One WLS call on `solver` and the oracle's answer: (handle, out, expected out, expected confidence map)."""
    view, dl, dr = _pair(frame, 1000 + seed + frame[0] * 7 + roi[2], scale)
    lam = _lam(adf, solver)
    p = oracle.default_params(sigma_color=SIGMA, threads=4, disc_radius=radius, use_confidence=int(use_conf), **{"lambda": lam})
    right = dr if use_conf else None
    exp, exp_conf = (oracle.wls_filter if scale == 1 else oracle.wls_filter_scaled)(dl, view, right, roi, p)
    f = adf.createDisparityWLSFilterGeneric(use_conf)
    f.setSolver(solver); f.setLambda(lam); f.setSigmaColor(SIGMA); f.setDepthDiscontinuityRadius(radius)
    out = f.filter(dl, view, None, right, roi)
    assert f.getLastSolver() == solver
    return f, out, exp, exp_conf, (dl, view, right)


def _check(f, out, exp, exp_conf):
    print("output pixels that differ: %d, largest difference %d" % (int((out != exp).sum()), int(np.abs(out.astype(np.int64) - exp).max())))
    if exp_conf is not None:
        conf = f.getConfidenceMap()
        print("confidence pixels that differ: %d" % int((conf != exp_conf).sum()))
        assert np.array_equal(conf, exp_conf)
    assert np.array_equal(out, exp)


# ---- plain_prologue_kernel --------------------------------------------------------------------------------------
def _smoother_case(adf, oracle, solver, size, dt, cn, seed):
    w, h = size
    rng = np.random.default_rng(seed + 31 * w + cn)
    guide = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    shape = (h, w) if cn == 1 else (h, w, cn)
    if dt == np.float32: src = rng.normal(0, 1000, shape).astype(np.float32)
    elif dt == np.int16: src = rng.integers(-32767, 32767, shape).astype(np.int16)
    else: src = rng.integers(0, 256, shape).astype(np.uint8)
    lam = _lam(adf, solver)
    exp = oracle.fgs_filter(guide, src, lam, SIGMA, threads=4)
    f = adf.createFastGlobalSmootherFilter(guide, lam, SIGMA, solver=solver)
    assert f.getSolver() == solver
    got = f.filter(src)
    print("%dx%d: elements that differ: %d" % (w, h, int((got != exp).sum())))
    assert got.dtype == src.dtype and np.array_equal(got, exp)


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32], ids=["u8", "i16", "f32"])
@pytest.mark.parametrize("cn", [1, 3])
def test_plain_prologue_natural_planes_wave_smoother(adf, oracle, cn, dt):
    """ORIENT_N: one channel, and the odd last channel behind a channel pair."""
    for size in ((65, 33), (2, 2)):
        _smoother_case(adf, oracle, adf.SOLVER_WAVE, size, dt, cn, seed=1)


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32], ids=["u8", "i16", "f32"])
@pytest.mark.parametrize("cn", [2, 4])
def test_plain_prologue_pair_plane_wave_smoother(adf, oracle, cn, dt):
    """ORIENT_PAIR: two channels as the two right-hand sides of one factorisation (the second typed load)."""
    for size in ((65, 33), (2, 2)):
        _smoother_case(adf, oracle, adf.SOLVER_WAVE, size, dt, cn, seed=2)


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32], ids=["u8", "i16", "f32"])
def test_plain_prologue_transposed_planes_exact_smoother(adf, oracle, dt):
    """ORIENT_T through the tile store, one right-hand side (U1 null)."""
    for size in ((65, 33), (2, 2), (1, 80), (96, 1)):
        _smoother_case(adf, oracle, adf.SOLVER_EXACT, size, dt, 3, seed=3)


@pytest.mark.parametrize("shape", WAVE_SHAPES, ids=_ids(WAVE_SHAPES))
def test_plain_prologue_natural_planes_wave_wls_without_confidence(adf, oracle, shape):
    f, out, exp, _, _ = _wls(adf, oracle, adf.SOLVER_WAVE, *shape, use_conf=False)
    assert f.getLastPath() == 0                     # no confidence stage, nothing fused: the prologue made the plane
    _check(f, out, exp, None)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids(EXACT_SHAPES))
def test_plain_prologue_transposed_planes_exact_wls_without_confidence(adf, oracle, shape):
    f, out, exp, _, _ = _wls(adf, oracle, adf.SOLVER_EXACT, *shape, use_conf=False)
    _check(f, out, exp, None)


def _half(shape):
    """A scaled call whose VIEW has the shape: maps of twice the view's size (resized DOWN to the view), ROI in the
    maps' coordinates."""
    (w, h), roi = shape
    return (2 * w, 2 * h), tuple(2 * v for v in roi)


@pytest.mark.parametrize("shape", UNFUSED_SHAPES, ids=_ids(UNFUSED_SHAPES))
def test_plain_prologue_pair_plane_scaled_confidence_wave(adf, oracle, monkeypatch, shape):
    """ORIENT_PAIR with confidence weighting: the resized maps' prologue, where the first row pass cannot fuse it.
    The first pass refuses only views with rows under 4 pixels, which leaves no room for maps smaller than the view:
    the maps here are twice the view's size (same kernels as a down-scaled call; the path bits are asserted)."""
    monkeypatch.setenv("ADF_SCALED_FUSE", "0")
    f, out, exp, exp_conf, _ = _wls(adf, oracle, adf.SOLVER_WAVE, *_half(shape), scale=0.5)
    assert not f.getLastPath() & (adf.PATH_FUSED_FIRST_PASS | adf.PATH_SCALED_FUSED), f.getLastPath()
    assert f.getROI() == _half(shape)[1]
    _check(f, out, exp, exp_conf)


# maps of half the view's size (the down-scaled call proper) on the tile shapes, and maps of twice the view's size so
# that the VIEW, which is what the prologue tiles, takes every exact-solver shape
SCALED_EXACT = [(s, 2) for s in (TILE, TINY, OFFSET)] + [(_half(s), 0.5) for s in EXACT_SHAPES]


@pytest.mark.parametrize("shape,scale", SCALED_EXACT, ids=["%s-x%g" % (i, k) for i, (_, k) in zip(_ids([s for s, _ in SCALED_EXACT]), SCALED_EXACT)])
def test_plain_prologue_transposed_planes_scaled_confidence_exact(adf, oracle, shape, scale):
    """ORIENT_T, two right-hand sides, with confidence weighting, from the resized maps."""
    f, out, exp, exp_conf, _ = _wls(adf, oracle, adf.SOLVER_EXACT, *shape, scale=scale)
    assert not f.getLastPath() & (adf.PATH_FUSED_FIRST_PASS | adf.PATH_SCALED_FUSED), f.getLastPath()
    _check(f, out, exp, exp_conf)


# ---- lrc_prologue_kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", WAVE_SHAPES, ids=_ids(WAVE_SHAPES))
def test_lrc_prologue_pair_plane_wave_radius_9(adf, oracle, shape):
    """Radius 9 is the first above the left sweep's limit: the two-kernel stage writes the pair plane."""
    f, out, exp, exp_conf, _ = _wls(adf, oracle, adf.SOLVER_WAVE, *shape, radius=9)
    assert not f.getLastPath() & (adf.PATH_FUSED_FIRST_PASS | adf.PATH_CONF_BAND | adf.PATH_MERGED_PREP), f.getLastPath()
    _check(f, out, exp, exp_conf)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids(EXACT_SHAPES))
def test_lrc_prologue_transposed_planes_exact(adf, oracle, shape):
    """ORIENT_T through the tile store from frame-coordinate tiles; then the float32 map, whose pixels outside the ROI
    this kernel fills: rounded as the int16 epilogue rounds, it is the oracle's map bit for bit."""
    f, out, exp, exp_conf, (dl, view, dr) = _wls(adf, oracle, adf.SOLVER_EXACT, *shape)
    assert not f.getLastPath() & (adf.PATH_FUSED_FIRST_PASS | adf.PATH_CONF_BAND | adf.PATH_MERGED_PREP), f.getLastPath()
    _check(f, out, exp, exp_conf)
    outf = f.filterFloat(dl, view, None, dr, shape[1])
    assert f.getLastSolver() == adf.SOLVER_EXACT and outf.dtype == np.float32
    x, y, w, h = shape[1]
    outside = np.ones(outf.shape, bool)
    outside[y:y + h, x:x + w] = False
    assert np.all(outf[outside] == np.float32(-16.0))
    rounded = np.array([oracle.sat16(v) for v in outf.ravel()], np.int16).reshape(outf.shape)
    print("float map: rounded pixels that differ: %d" % int((rounded != exp).sum()))
    assert np.array_equal(rounded, exp)
    assert np.array_equal(f.getConfidenceMap(), exp_conf)


@pytest.mark.parametrize("shape", WAVE_SHAPES, ids=_ids(WAVE_SHAPES))
def test_lrc_prologue_confidence_only_scaled_without_band(adf, oracle, monkeypatch, shape):
    """No right-hand sides (U0 null): the low-resolution confidence maps of a down-scaled call when the band kernel
    is switched off.  Maps of the shape, view of twice their size."""
    monkeypatch.setenv("ADF_CONF_BAND", "0")
    f, out, exp, exp_conf, _ = _wls(adf, oracle, adf.SOLVER_EXACT, *shape, scale=2)
    assert not f.getLastPath() & adf.PATH_CONF_BAND, f.getLastPath()
    _check(f, out, exp, exp_conf)


# ---- conf_left_kernel<R, true> ----------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [2, 5])
@pytest.mark.parametrize("shape", UNFUSED_SHAPES, ids=_ids(UNFUSED_SHAPES))
def test_conf_left_writes_the_pair_plane_when_the_first_pass_cannot_fuse(adf, oracle, shape, radius):
    f, out, exp, exp_conf, _ = _wls(adf, oracle, adf.SOLVER_WAVE, *shape, radius=radius)
    assert not f.getLastPath() & (adf.PATH_FUSED_FIRST_PASS | adf.PATH_CONF_BAND | adf.PATH_MERGED_PREP), f.getLastPath()
    _check(f, out, exp, exp_conf)
