"""The last hand-off of the wave solver: the last row pass stores the last column pass's register image
(fgs_wave_h.hip store_image, fgs_wave_v.hip IMG) instead of the pair plane.

Same operands into the same solves: every output is bit-identical to the pair-plane hand-off.  Every case runs the call
on two handles -- one that may take the image and one made under ADF_LAST_HANDOFF_IMAGE=0, the reference -- both with
the plan's size threshold lowered (ADF_LAST_HANDOFF_MIN_PX, a test knob) and under ADF_MERGE_SMALL=0 (the merged
preparation launch of small calls stays on the Chor plane, and both row-weight forms are wanted here).  It asserts that
the int16 map, the float map and the confidence map are equal bit for bit and that getLastHandoff() reports the form
the call must have taken: the image for two right-hand sides, at least two iterations, one-wave rows (<= 4096 columns)
and whole-strip columns (<= 2176 rows); the pair plane otherwise."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("ADF_MERGE_SMALL", "ADF_ROW_WEIGHTS_GUIDE", "ADF_LAST_HANDOFF_IMAGE", "ADF_LAST_HANDOFF_MIN_PX", "ADF_WS_LIMIT_GB")
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


def _inputs(seed, n, H, W):
    """Maps with steps and noise (right = -left + noise, so the LRC check passes in places) and a guide that is smooth
    with noisy stretches (table indices inside and beyond the row pass's LDS head)."""
    import torch
    rng = np.random.default_rng(seed)
    shape = (n, H, W)
    base = (rng.integers(0, 40, (n, H, 1)) * 16 + 320 * (np.arange(W) > W // 2)).astype(np.int64)
    dl = np.clip(base + rng.normal(0, 6, shape), -32768, 32767).astype(np.int16)
    dr = np.clip(-base + rng.normal(0, 6, shape), -32768, 32767).astype(np.int16)
    x = (np.arange(W) * 3 // 2) % 510
    ramp = np.broadcast_to(np.where(x < 256, x, 510 - x).reshape(1, 1, W, 1), shape + (3,)).astype(np.uint8)
    pick = rng.random(shape) < 0.1
    view = np.where(pick[..., None], rng.integers(0, 256, shape + (3,), dtype=np.uint8), ramp).astype(np.uint8)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (dl, dr, view)]


def _run(adf, f, tl, tr, tv, roi):
    import torch
    f.enableProfiling(True)
    i16 = f.filter(tl, tv, None, tr, roi)
    torch.cuda.synchronize()
    prof = f.readProfile()
    f.enableProfiling(False)
    form, spath, solver = f.getLastHandoff(), f.getLastSolverPath(), f.getLastSolver()
    conf = f.getConfidenceMap().cpu().numpy()
    f32 = f.filterFloat(tl, tv, None, tr, roi)
    torch.cuda.synchronize()
    assert f.getLastHandoff() == form
    return i16.cpu().numpy(), f32.cpu().numpy(), conf, form, spath, solver, prof


def _ab(adf, n, H, W, roi, iters=3, guide=1, env=None, expect=None, seed=0, ref_env=None, chunks=1):
    """The call with and without the image; `expect`: the form the first handle must report (default: by the rules);
    `ref_env`: knobs of the reference handle alone; `chunks`: the chunks both calls must have run in."""
    tl, tr, tv = _inputs(seed + 31 * H + W, n, H, W)
    if n == 1:
        tl, tr, tv = tl[0], tr[0], tv[0]
    common = {"ADF_MERGE_SMALL": 0, "ADF_ROW_WEIGHTS_GUIDE": guide, "ADF_LAST_HANDOFF_MIN_PX": 0}
    common.update(env or {})
    got = _run(adf, _handle(adf, common, iters), tl, tr, tv, roi)
    ref = _run(adf, _handle(adf, dict(common, ADF_LAST_HANDOFF_IMAGE=0, **(ref_env or {})), iters), tl, tr, tv, roi)
    if expect is None:
        expect = adf.HANDOFF_IMAGE if (iters >= 2 and roi[2] <= 4096 and roi[3] <= 2176) else adf.HANDOFF_PAIR_PLANE
    assert got[5] == ref[5] == adf.SOLVER_WAVE
    # every chunk launches one fused first row pass and iters - 1 plain ones, iters - 1 plain column passes and a last one
    for r in (got, ref):
        launches = {k: r[6].get(k, {"launches": 0})["launches"] for k in ("pass_h_first", "pass_h", "pass_v", "pass_v_last")}
        assert launches == {"pass_h_first": chunks, "pass_h": chunks * (iters - 1), "pass_v": chunks * (iters - 1), "pass_v_last": chunks}, launches
    assert got[3] == expect, "the call reports hand-off form %d, not %d" % (got[3], expect)
    assert ref[3] == adf.HANDOFF_PAIR_PLANE
    guide_rows = bool(guide) and roi[2] <= 4096               # (the guide forms are the one-wave rows')
    assert bool(got[4] & adf.PATH_ROW_WEIGHTS_GUIDE) == bool(ref[4] & adf.PATH_ROW_WEIGHTS_GUIDE) == guide_rows
    for a, b, what in zip(got[:3], ref[:3], ("int16 map", "float map", "confidence map")):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: %d elements differ" % (what, int((a != b).sum()))
    return got


# ---- ROI heights on both sides of every whole-strip column bucket's edge, and one beyond the last (half strips) ----
HEIGHTS = sorted({h for m in COL_CHUNKS for h in (64 * m - 1, 64 * m, 64 * m + 1)} | {255, 257, 2177})


@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("rh", HEIGHTS)
def test_column_bucket_edges(adf, rh, guide):
    rw, x0, y0 = 37, 3, 1                                     # 2 full strips and a partial one, ROI x odd, odd width
    _ab(adf, 1, y0 + rh + (rh % 2), x0 + rw + 4, (x0, y0, rw, rh), guide=guide)


# ---- widths: every one-wave row bucket's last width, widths that are no multiple of 16 / odd, ROI x odd and even ----
@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("rw,x0", [(16, 0), (50, 1), (255, 3), (256, 2), (257, 5), (512, 0), (1023, 1), (1280, 0), (1777, 3),
                                   (2560, 4), (3584, 256), (3839, 1), (4090, 3), (4096, 0)])
def test_row_buckets(adf, rw, x0, guide):
    rh = 130 + rw % 7                                         # more than one chunk per wave instruction's eight, M = 4
    _ab(adf, 1, rh + 2, x0 + rw + (3 if rw % 2 else 0), (x0, 2, rw, rh), guide=guide)


def test_two_wave_rows_keep_the_pair_plane(adf):
    _ab(adf, 1, 70, 4100, (0, 0, 4100, 70), expect=adf.HANDOFF_PAIR_PLANE)


# ---- iterations: the last row pass of a one-iteration call is the fused first one ----
@pytest.mark.parametrize("guide", [1, 0])
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_iterations(adf, iters, guide):
    _ab(adf, 1, 300, 210, (5, 2, 199, 290), iters=iters, guide=guide)


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
    env, ref_env, expect, chunks = {}, {}, adf.HANDOFF_IMAGE, 1
    if mode != "one-chunk":
        # each handle under its own limit: a pair of the image handle's workspace is larger than one of the reference's
        base = {"ADF_MERGE_SMALL": 0, "ADF_ROW_WEIGHTS_GUIDE": guide, "ADF_LAST_HANDOFF_MIN_PX": 0}
        env["ADF_WS_LIMIT_GB"] = _limit_for_two(adf, H, W, roi, base)
        ref_env["ADF_WS_LIMIT_GB"] = _limit_for_two(adf, H, W, roi, dict(base, ADF_LAST_HANDOFF_IMAGE=0))
        assert float(env["ADF_WS_LIMIT_GB"]) > float(ref_env["ADF_WS_LIMIT_GB"])
        chunks = 2
    if mode == "tail-below-threshold":
        env["ADF_LAST_HANDOFF_MIN_PX"] = roi[2] * roi[3] * 3 // 2    # the chunk of two takes the image, the tail of one the pair plane
        expect = adf.HANDOFF_IMAGE_PAIR_TAIL
    out = _ab(adf, 3, H, W, roi, guide=guide, env=env, ref_env=ref_env, expect=expect, chunks=chunks)
    assert out[0].shape == (3, H, W)


def test_default_threshold_keeps_small_calls_on_the_pair_plane(adf):
    """Without the test knob a call this small must not change its plan or its workspace."""
    import torch
    tl, tr, tv = _inputs(3, 2, 120, 200)
    sizes = []
    for env in ({"ADF_MERGE_SMALL": 0}, {"ADF_MERGE_SMALL": 0, "ADF_LAST_HANDOFF_IMAGE": 0}):
        f = _handle(adf, env, 3)
        f.filter(tl, tv, None, tr, (2, 2, 190, 110))
        torch.cuda.synchronize()
        assert f.getLastHandoff() == adf.HANDOFF_PAIR_PLANE
        sizes.append(f.workspaceBytes())
    assert sizes[0] == sizes[1]
