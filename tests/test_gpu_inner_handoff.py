"""Every row -> column hand-off of the wave solver as the column pass's register image: the row passes before the last
one store the image too (fgs_wave_h.hip store_image, the fused first pass included), the plain column passes load it
(fgs_wave_v.hip IMG on EPI_PLANES) and store to the pair plane as ever.

Same operands into the same solves: every output is bit-identical whichever hand-offs take the image.  Every case runs
the call on three handles -- the default one, one made under ADF_INNER_HANDOFF_IMAGE=0 (only the last hand-off may take
the image) and one under ADF_LAST_HANDOFF_IMAGE=0 (every hand-off on the pair plane, the reference) -- all with the
plan's size threshold lowered (ADF_LAST_HANDOFF_MIN_PX, a test knob) and under ADF_MERGE_SMALL=0.  It asserts that the
int16 map, the float map and the confidence map are equal bit for bit across the three, that getInnerHandoffs() reports
the image on exactly the hand-offs the rules give, and that the profile's launch counts per pass are the reference's.

The rules: a call takes the image with two right-hand sides, at least two iterations, one-wave rows (<= 4096 columns)
and whole-strip columns (<= 2176 rows), in chunks of at least the threshold.  Of its num_iter - 1 inner hand-offs the
first takes it where the first row pass is the view-resolution fused one on int16 maps AND that pass's image form is
built (FIRST_FORM below, read once from the library's own report and then held against every other case); the later
ones always do."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("ADF_MERGE_SMALL", "ADF_ROW_WEIGHTS_GUIDE", "ADF_LAST_HANDOFF_IMAGE", "ADF_INNER_HANDOFF_IMAGE", "ADF_LAST_HANDOFF_MIN_PX",
         "ADF_WS_LIMIT_GB")
# the whole-strip column buckets hold columns of up to 64 chunks of these lengths
COL_CHUNKS = [2, 4, 8, 12, 18, 26, 34]


def _handle(adf, env, iters):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        f = adf.createDisparityWLSFilterGeneric(True)         # the knobs are read when the handle is made
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    f.setSolver(adf.SOLVER_WAVE); f.setLambda(8000.0); f.setSigmaColor(1.5); f.setDepthDiscontinuityRadius(2)
    f.setFGSParams(0.25, iters)
    return f


def _inputs(seed, n, H, W, vH=None, vW=None, f32=False):
    """Maps with steps and noise (right = -left + noise, so the LRC check passes in places) and a guide that is smooth
    with noisy stretches (table indices inside and beyond the row pass's LDS head).  vH, vW: a view of another size."""
    import torch
    rng = np.random.default_rng(seed)
    shape = (n, H, W)
    base = (rng.integers(0, 40, (n, H, 1)) * 16 + 320 * (np.arange(W) > W // 2)).astype(np.int64)
    dl = np.clip(base + rng.normal(0, 6, shape), -32768, 32767).astype(np.int16)
    dr = np.clip(-base + rng.normal(0, 6, shape), -32768, 32767).astype(np.int16)
    if f32:
        dl = dl.astype(np.float32) + rng.random(shape, dtype=np.float32)
        dr = dr.astype(np.float32) - rng.random(shape, dtype=np.float32)
    vshape = (n, vH or H, vW or W)
    x = (np.arange(vshape[2]) * 3 // 2) % 510
    ramp = np.broadcast_to(np.where(x < 256, x, 510 - x).reshape(1, 1, vshape[2], 1), vshape + (3,)).astype(np.uint8)
    pick = rng.random(vshape) < 0.1
    view = np.where(pick[..., None], rng.integers(0, 256, vshape + (3,), dtype=np.uint8), ramp).astype(np.uint8)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (dl, dr, view)]


def _run(adf, f, tl, tr, tv, roi):
    import torch
    f.enableProfiling(True)
    i16 = f.filter(tl, tv, None, tr, roi)
    torch.cuda.synchronize()
    prof = f.readProfile()
    f.enableProfiling(False)
    form, inner, spath, solver = f.getLastHandoff(), f.getInnerHandoffs(), f.getLastSolverPath(), f.getLastSolver()
    conf = f.getConfidenceMap().cpu().numpy()
    f32 = f.filterFloat(tl, tv, None, tr, roi)
    torch.cuda.synchronize()
    assert f.getLastHandoff() == form and f.getInnerHandoffs() == inner
    return i16.cpu().numpy(), f32.cpu().numpy(), conf, form, spath, solver, prof, inner


_first_form = []


def _first_form_built(adf):
    """Does the fused first row pass have the image form?  One call of the getter on a three-iteration call: two inner
    hand-offs with it, one without.  Every other case is held against this answer."""
    if not _first_form:
        tl, tr, tv = _inputs(5, 1, 80, 96)
        f = _handle(adf, {"ADF_MERGE_SMALL": 0, "ADF_LAST_HANDOFF_MIN_PX": 0}, 3)
        f.filter(tl[0], tv[0], None, tr[0], (2, 1, 90, 77))
        full, tail = f.getInnerHandoffs()
        assert full == tail and full in (1, 2), (full, tail)
        _first_form.append(full == 2)
    return _first_form[0]


def _inner_by_the_rules(adf, iters, takes, fused_view_first):
    if not takes or iters < 2:
        return 0
    return (iters - 2) + (1 if (fused_view_first and _first_form_built(adf)) else 0)


def _ab(adf, tl, tr, tv, roi, vroi=None, iters=3, guide=1, env=None, ref_env=None, chunks=1, fused_view_first=True,
        inner=None, last=None, guide_rows=None):
    """The call on the three handles.  roi: as the call takes it; vroi: the ROI in the view (down-scaled calls);
    inner: the (full, tail) counts the first handle must report (default: by the rules, both chunks alike); last: the
    form of its last hand-off (default: by the rules); env / ref_env: knobs of the image handles / the reference alone."""
    vroi = vroi or roi
    common = {"ADF_MERGE_SMALL": 0, "ADF_ROW_WEIGHTS_GUIDE": guide, "ADF_LAST_HANDOFF_MIN_PX": 0}
    common.update(env or {})
    got = _run(adf, _handle(adf, common, iters), tl, tr, tv, roi)
    mid = _run(adf, _handle(adf, dict(common, ADF_INNER_HANDOFF_IMAGE=0), iters), tl, tr, tv, roi)
    ref_common = {k: v for k, v in common.items() if k not in (ref_env or {})}
    ref = _run(adf, _handle(adf, dict(ref_common, ADF_LAST_HANDOFF_IMAGE=0, **(ref_env or {})), iters), tl, tr, tv, roi)
    takes = iters >= 2 and vroi[2] <= 4096 and vroi[3] <= 2176
    if inner is None:
        k = _inner_by_the_rules(adf, iters, takes, fused_view_first)
        inner = (k, k)
    if last is None:
        last = adf.HANDOFF_IMAGE if takes else adf.HANDOFF_PAIR_PLANE
    assert got[5] == mid[5] == ref[5] == adf.SOLVER_WAVE
    # every chunk launches one first row pass and iters - 1 plain ones, iters - 1 plain column passes and a last one
    for r in (got, mid, ref):
        launches = {k: r[6].get(k, {"launches": 0})["launches"] for k in ("pass_h_first", "pass_h", "pass_v", "pass_v_last")}
        assert launches == {"pass_h_first": chunks, "pass_h": chunks * (iters - 1), "pass_v": chunks * (iters - 1), "pass_v_last": chunks}, launches
    for cls in ("pass_h_first", "pass_h", "pass_v", "pass_v_last"):
        if cls in ref[6]:
            assert got[6][cls]["alg_bytes"] == mid[6][cls]["alg_bytes"] == ref[6][cls]["alg_bytes"], cls
    assert got[7] == tuple(inner), "the call reports %s inner hand-offs through the image, not %s" % (got[7], tuple(inner))
    assert got[3] == last, "the call reports hand-off form %d, not %d" % (got[3], last)
    assert mid[7] == (0, 0) and mid[3] == last
    assert ref[7] == (0, 0) and ref[3] == adf.HANDOFF_PAIR_PLANE
    if guide_rows is None:
        guide_rows = bool(guide) and vroi[2] <= 4096          # (the guide forms are the one-wave rows')
    assert bool(got[4] & adf.PATH_ROW_WEIGHTS_GUIDE) == bool(mid[4] & adf.PATH_ROW_WEIGHTS_GUIDE) == bool(ref[4] & adf.PATH_ROW_WEIGHTS_GUIDE) == guide_rows
    for other, who in ((mid, "inner hand-offs on the pair plane"), (ref, "every hand-off on the pair plane")):
        for a, b, what in zip(got[:3], other[:3], ("int16 map", "float map", "confidence map")):
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s against %s: %d elements differ" % (what, who, int((a != b).sum()))
    return got


def _same_size(adf, n, H, W, roi, seed=0, **kw):
    tl, tr, tv = _inputs(seed + 31 * H + W, n, H, W)
    if n == 1:
        tl, tr, tv = tl[0], tr[0], tv[0]
    return _ab(adf, tl, tr, tv, roi, **kw)


# ---- ROI heights on both sides of every whole-strip column bucket's edge, and one beyond the last (half strips) ----
HEIGHTS = sorted({h for m in COL_CHUNKS for h in (64 * m - 1, 64 * m, 64 * m + 1)} | {255, 257, 2177})


@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("rh", HEIGHTS)
def test_column_bucket_edges(adf, rh, guide):
    rw, x0, y0 = 37, 3, 1                                     # 2 full strips and a partial one, ROI x odd, odd width
    got = _same_size(adf, 1, y0 + rh + (rh % 2), x0 + rw + 4, (x0, y0, rw, rh), guide=guide)
    if rh == 2177:
        assert got[7] == (0, 0)                               # half strips keep the pair plane
    else:
        assert got[7][0] >= 1                                 # no case passes with the form not taken


# ---- widths: every one-wave row bucket's last width, widths that are no multiple of 16 / odd, ROI x odd and even ----
@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("odd_x", [0, 1])
@pytest.mark.parametrize("rw", [16, 50, 255, 256, 257, 512, 1023, 1280, 1777, 2560, 3584, 3839, 4090, 4096])
def test_row_buckets(adf, rw, odd_x, guide):
    x0 = (256 if rw == 3584 else 2 * (rw % 3)) + (3 if odd_x else 0)
    rh = 130 + rw % 7                                         # more than one chunk per wave instruction's eight, M = 4
    got = _same_size(adf, 1, rh + 2, x0 + rw + (3 if rw % 2 else 0), (x0, 2, rw, rh), guide=guide)
    assert got[7][0] >= 1


def test_two_wave_rows_keep_the_pair_plane(adf):
    got = _same_size(adf, 1, 70, 4100, (0, 0, 4100, 70), last=adf.HANDOFF_PAIR_PLANE)
    assert got[7] == (0, 0)


# ---- iterations: 0, 1, 2, 4 inner hand-offs through the image with the fused first pass's form, 0, 0, 1, 3 without ----
@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("iters", [1, 2, 3, 5])
def test_iterations(adf, iters, guide):
    got = _same_size(adf, 1, 300, 210, (5, 2, 199, 290), iters=iters, guide=guide)
    with_first, without = {1: 0, 2: 1, 3: 2, 5: 4}, {1: 0, 2: 0, 3: 1, 5: 3}
    assert got[7][0] == (with_first if _first_form_built(adf) else without)[iters]


# ---- pairs: a batch in one chunk; a chunk of two and a tail of one; a tail below the size threshold ----
def _limit_for_two(adf, H, W, roi, env):
    """ADF_WS_LIMIT_GB that holds a chunk of two pairs of this call under `env` (per-chunk bytes: whole call - one-pair chunks)."""
    tl, tr, tv = _inputs(1, 3, H, W)
    sizes = []
    for lim in (None, "1e-9"):
        f = _handle(adf, dict(env, **({"ADF_WS_LIMIT_GB": lim} if lim else {})), 3)
        f.filter(tl, tv, None, tr, roi)
        sizes.append(f.workspaceBytes())
    per_pair = (sizes[0] - sizes[1]) / 2
    assert per_pair > 0
    return "%.12f" % (2.2 * per_pair / 2 ** 30)


@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("mode", ["one-chunk", "tail", "tail-below-threshold"])
def test_pairs(adf, mode, guide):
    H, W, roi = 200, 150, (3, 1, 141, 197)
    k = _inner_by_the_rules(adf, 3, True, True)
    env, ref_env, inner, last, chunks = {}, {}, (k, k), adf.HANDOFF_IMAGE, 1
    if mode != "one-chunk":
        # each handle under its own limit: a pair of the image handles' workspace is larger than one of the reference's
        base = {"ADF_MERGE_SMALL": 0, "ADF_ROW_WEIGHTS_GUIDE": guide, "ADF_LAST_HANDOFF_MIN_PX": 0}
        env["ADF_WS_LIMIT_GB"] = _limit_for_two(adf, H, W, roi, base)
        assert env["ADF_WS_LIMIT_GB"] == _limit_for_two(adf, H, W, roi, dict(base, ADF_INNER_HANDOFF_IMAGE=0))   # no workspace byte added
        ref_env["ADF_WS_LIMIT_GB"] = _limit_for_two(adf, H, W, roi, dict(base, ADF_LAST_HANDOFF_IMAGE=0))
        assert float(env["ADF_WS_LIMIT_GB"]) > float(ref_env["ADF_WS_LIMIT_GB"])
        chunks = 2
    if mode == "tail-below-threshold":
        env["ADF_LAST_HANDOFF_MIN_PX"] = roi[2] * roi[3] * 3 // 2    # the chunk of two takes the image, the tail of one the pair plane
        inner, last = (k, 0), adf.HANDOFF_IMAGE_PAIR_TAIL
    out = _same_size(adf, 3, H, W, roi, guide=guide, env=env, ref_env=ref_env, inner=inner, last=last, chunks=chunks)
    assert out[0].shape == (3, H, W) and out[7][0] >= 1


# ---- down-scaled call: the interpolating first pass keeps the pair plane, the later hand-offs take the image ----
def test_down_scaled_call(adf):
    tl, tr, tv = _inputs(11, 1, 105, 150, vH=210, vW=300)
    got = _ab(adf, tl[0], tr[0], tv[0], (3, 1, 140, 100), vroi=(6, 2, 280, 200), fused_view_first=False, inner=(1, 1), guide_rows=False)
    assert got[0].shape == (210, 300)


# ---- float32 maps (adf_wls_filter_typed_*): the float prologue keeps the pair plane for the first hand-off ----
def test_float32_maps(adf):
    tl, tr, tv = _inputs(13, 1, 150, 180, f32=True)
    _ab(adf, tl[0], tr[0], tv[0], (4, 2, 170, 145), fused_view_first=False, inner=(1, 1))


def test_default_threshold_keeps_small_calls_on_the_pair_plane(adf):
    """Without the test knob a call this small takes the image on no hand-off and its workspace does not change."""
    import torch
    tl, tr, tv = _inputs(3, 2, 120, 200)
    sizes = []
    for env in ({"ADF_MERGE_SMALL": 0}, {"ADF_MERGE_SMALL": 0, "ADF_LAST_HANDOFF_IMAGE": 0}):
        f = _handle(adf, env, 3)
        f.filter(tl, tv, None, tr, (2, 2, 190, 110))
        torch.cuda.synchronize()
        assert f.getLastHandoff() == adf.HANDOFF_PAIR_PLANE and f.getInnerHandoffs() == (0, 0)
        sizes.append(f.workspaceBytes())
    assert sizes[0] == sizes[1]
