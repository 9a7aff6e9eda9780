"""Wave solver row passes that form their edge weights from the guide row (fgs_wave_h.hip, WS_GUIDE1 / WS_GUIDE3)
instead of reading the Chor plane the weight kernel would have written.

Same table entry, same multiply by lambda, same masks: c[] is bit-identical to the plane path's, so every filtered map
is.  Every case runs the call on two handles -- the default one, which must report PATH_ROW_WEIGHTS_GUIDE in
getLastSolverPath() (a word beside getLastPath(), whose bits other tests compare as a whole on calls that take this
path), and one made under ADF_ROW_WEIGHTS_GUIDE=0, which must not -- and asserts that the filtered maps,
the confidence maps and workspaceBytes() are identical.  (workspaceBytes: the Chor plane stays carved on the new path;
giving it back is a later change.)  Both handles are made under ADF_MERGE_SMALL=0: calls this small would otherwise
take the merged preparation launch, which stays on the plane path.  Heights are 6-16 rows throughout."""
import os

import numpy as np
import pytest

from addingdisparityfiltering_amd import synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# the one-wave row buckets hold rows of up to these widths (chunk length 4 .. 64, times 64 lanes): all have the guide forms
BUCKET_LIMITS = [256, 512, 1024, 1280, 1792, 2560, 3584, 3840, 4096]


def _handle(adf, conf, forced_plane):
    env = {"ADF_MERGE_SMALL": "0", "ADF_ROW_WEIGHTS_GUIDE": "0" if forced_plane else None}
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        f = adf.createDisparityWLSFilterGeneric(conf)      # the knobs are read when the handle is made
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    f.setSolver(adf.SOLVER_WAVE); f.setLambda(8000.0); f.setSigmaColor(1.5); f.setDepthDiscontinuityRadius(2)
    return f


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _ab(adf, conf, call, fused_first=None):
    """call(f) -> filtered map, on the default handle and on the forced-plane one; returns the default handle's map."""
    import torch
    res = []
    for forced in (False, True):
        f = _handle(adf, conf, forced)
        out = call(f)
        torch.cuda.synchronize()
        assert f.getLastSolver() == adf.SOLVER_WAVE
        assert not f.getLastPath() & adf.PATH_MERGED_PREP
        if fused_first is not None:
            assert bool(f.getLastPath() & adf.PATH_FUSED_FIRST_PASS) == fused_first
        on = bool(f.getLastSolverPath() & adf.PATH_ROW_WEIGHTS_GUIDE)
        assert on == (not forced), "forced=%s but the guide row path %s" % (forced, "ran" if on else "did not run")
        res.append((_np(out), _np(f.getConfidenceMap()) if conf else None, f.workspaceBytes()))
    (o0, c0, w0), (o1, c1, w1) = res
    assert o0.shape == o1.shape and np.array_equal(o0.view(np.uint8), o1.view(np.uint8)), int((o0 != o1).sum())
    if conf:
        assert np.array_equal(c0, c1)
    assert w0 == w1                                          # the Chor plane stays carved
    return o0


def _maps(rng, shape):
    """A plausible pair of disparity maps: steps + noise, right = -left + noise (so the LRC check passes in places)."""
    h, w = shape[-2:]
    base = (rng.integers(0, 40, shape[:-1] + (1,)) * 16 + 320 * (np.arange(w) > w // 2)).astype(np.int64)
    dl = np.clip(base + rng.normal(0, 6, shape), -32768, 32767).astype(np.int16)
    dr = np.clip(-base + rng.normal(0, 6, shape), -32768, 32767).astype(np.int16)
    return dl, dr


def _guide(rng, kind, shape, ch):
    """(N,)H,W(,3) uint8: 'noise' = uniform (nearly every table index beyond the LDS head), 'ramp' = smooth (all inside),
    'mixed' = a ramp with noisy stretches (rows with and without far indices)."""
    full = tuple(shape) + ((3,) if ch == 3 else ())
    w = shape[-1]
    if kind == "noise":
        return rng.integers(0, 256, full, dtype=np.uint8)
    x = (np.arange(w) * 3 // 2) % 510
    x = np.where(x < 256, x, 510 - x)                        # a triangle wave: steps of 1 or 2 grey levels, no wrap
    ramp = np.broadcast_to(x.reshape((1,) * (len(shape) - 1) + (w,) + ((1,) if ch == 3 else ())), full).astype(np.uint8)
    if kind == "ramp":
        return np.ascontiguousarray(ramp)
    noisy = rng.integers(0, 256, full, dtype=np.uint8)
    pick = (rng.random(shape) < 0.1)
    pick[..., ::2, :] = False                                # every other row stays all-smooth
    return np.where(pick[..., None] if ch == 3 else pick, noisy, ramp).astype(np.uint8)


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ---- every bucket, both channel counts, R = 2 (fused first pass + two plain passes) and R = 1 ----
WIDTHS = sorted(set([w for lim in BUCKET_LIMITS for w in (lim, lim + 1) if w <= 4096] + [4095]))


@pytest.mark.parametrize("conf", [True, False])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("rw", WIDTHS)
def test_every_bucket(adf, rw, ch, conf):
    rng = np.random.default_rng(rw * 7 + ch + 2 * conf)
    n, H, x0 = 2, 6 + rw % 5, 3
    W = x0 + rw + (5 if rw % 2 else 0)                        # odd widths: the ROI ends before the frame's last column
    dl, dr = _maps(rng, (n, H, W))
    view = _guide(rng, "mixed", (n, H, W), ch)
    tl, tr, tv = _dev(dl, dr, view)
    _ab(adf, conf, lambda f: f.filter(tl, tv, None, tr if conf else None, (x0, 0, rw, H)), fused_first=conf)


# ---- alignment: ROI x, base byte offset of the guide, row and pair strides ----
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("x0", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_guide_alignment(adf, x0, base, ch):
    """The guide as a slice of a larger buffer: base byte offset 0..3, a row stride larger than the row, and a batch of 3
    whose pair stride is not the image size -- the row's 16-byte window starts at every misalignment."""
    import torch
    rng = np.random.default_rng(100 * x0 + 10 * base + ch)
    n, H, W, rw = 3, 9, 300 + x0, 277
    row = W * ch + 13 + base                                  # bytes: odd strides shift the misalignment from row to row
    pair = H * row + 29
    buf = torch.from_numpy(rng.integers(0, 256, base + n * pair + 64, dtype=np.uint8)).cuda()
    smooth = torch.from_numpy(_guide(rng, "mixed", (n, H, W), ch)).cuda()
    tv = torch.as_strided(buf, (n, H, W, 3) if ch == 3 else (n, H, W), (pair, row, 3, 1) if ch == 3 else (pair, row, 1), base)
    tv.copy_(smooth)
    assert tv.data_ptr() % 4 == (buf.data_ptr() + base) % 4
    dl, dr = _maps(rng, (n, H, W))
    tl, tr = _dev(dl, dr)
    out = _ab(adf, True, lambda f: f.filter(tl, tv, None, tr, (x0, 1, rw, H - 2)), fused_first=True)
    # a batch is its pairs, and a slice is its pixels: the dense copy of one pair gives the same map
    k = 2
    dense = tv[k].contiguous()
    one = _ab(adf, True, lambda f: f.filter(tl[k], dense, None, tr[k], (x0, 1, rw, H - 2)), fused_first=True)
    assert np.array_equal(out[k], one)


# ---- edges of the ROI and of the caller's buffer ----
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("rw,right", [(5, 0), (6, 0), (7, 0), (5, 3), (6, 1), (7, 2), (9, 0), (13, 4), (250, 0), (255, 1), (1023, 0), (1023, 7),
                                      (2, 0), (3, 1), (4, 0)])
def test_roi_edges(adf, rw, right, ch):
    """Widths that are no multiple of 4; ROIs that end at the frame's last column (`right` = 0: the row's last pixel has
    no neighbour in the row -- in the last row of the last image not even in the buffer) and before it (the neighbour
    exists and must still give weight 0 in the last ROI column); the ROI ends in the last row of the last image."""
    rng = np.random.default_rng(rw * 11 + right + ch)
    n, H, x0 = 2, 8, 2
    W = x0 + rw + right
    dl, dr = _maps(rng, (n, H, W))
    view = _guide(rng, "noise", (n, H, W), ch)
    tl, tr, tv = _dev(dl, dr, view)
    roi = (x0, 2, rw, H - 2)                                  # ... down to the last row
    # (rows shorter than one vector take the prologue kernels: not fused, the row passes are the plain ones)
    _ab(adf, True, lambda f: f.filter(tl, tv, None, tr, roi), fused_first=rw >= 4)
    _ab(adf, False, lambda f: f.filter(tl, tv, None, None, roi))


# ---- table reach ----
def _kitti_rows():
    from PIL import Image
    left = np.array(Image.open(os.path.join(GOLDEN, "kitti_left.bmp")).convert("L"))
    assert left.shape == (375, 1242)
    return np.ascontiguousarray(left[180:192])                # road, cars and trees: the crop's rows of config 5's ROI


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("kind", ["noise", "ramp", "artificial", "kitti"])
def test_table_reach(adf, oracle, kind, ch):
    """Indices beyond the LDS head of the table (uniform noise: nearly all), inside it (a smooth ramp: all), and the two
    natural mixes; the share of far indices is asserted so that the guides keep meaning what they are here for."""
    rng = np.random.default_rng(len(kind) + ch)
    if kind == "artificial":
        view, dl, dr, roi = synthetic.make_artificial_example(640, 16, ch, seed=9)
        view, dl, dr = np.stack([view, view[::-1]]), np.stack([dl, dl]), np.stack([dr, dr])
    else:
        if kind == "kitti":
            g = _kitti_rows()
            g = np.stack([g, np.roll(g, 1, 0), np.roll(g, 1, 1)], axis=2) if ch == 3 else g      # as test_gpu_real_guides.py
            view = np.stack([g, g[::-1]])
            roi = (128, 0, 1114, 12)
        else:
            view = _guide(rng, kind, (2, 12, 1242), ch)
            roi = (128, 0, 1114, 12)
        dl, dr = _maps(rng, view.shape[:3])
    x, y, w, h = roi
    v = view[:, y:y + h, x:x + w].astype(np.int64).reshape(2, h, w, -1)
    far = (((v[:, :, 1:] - v[:, :, :-1]) ** 2).sum(-1) >= 1024).mean()
    lo, hi = {"noise": (0.7, 1.0), "ramp": (0.0, 0.0), "artificial": (0.0, 1.0), "kitti": (0.001, 0.5)}[kind]
    assert lo <= far <= hi, (kind, ch, far)
    tl, tr, tv = _dev(dl, dr, view)
    out = _ab(adf, True, lambda f: f.filter(tl, tv, None, tr, roi), fused_first=True)
    # and the maps are the filter's: within the wave solver's bar of the oracle (test_disparity_wls_filter.cpp:104-105)
    p = oracle.default_params(threads=8, use_confidence=1, disc_radius=2, sigma_color=1.5)
    p.lambda_ = 8000.0
    exp, _ = oracle.wls_filter(dl[0], view[0], dr[0], roi, p)
    d = np.abs(out[0].astype(np.int64) - exp.astype(np.int64))
    assert d.max() <= 1 and d.mean() <= 1 / 256.0, (d.max(), d.mean())


# ---- the float output and a captured call ----
def test_float_output(adf):
    rng = np.random.default_rng(5)
    n, H, W, roi = 2, 10, 700, (6, 1, 690, 8)
    dl, dr = _maps(rng, (n, H, W))
    tl, tr, tv = _dev(dl, dr, _guide(rng, "mixed", (n, H, W), 3))
    f32 = _ab(adf, True, lambda f: f.filterFloat(tl, tv, None, tr, roi), fused_first=True)
    assert f32.dtype == np.float32 and np.isfinite(f32).all()
    i16 = _ab(adf, True, lambda f: f.filter(tl, tv, None, tr, roi), fused_first=True)
    assert np.array_equal(np.clip(np.rint(f32), -32768, 32767).astype(np.int16), i16)


def test_graph_capture_and_replay(adf):
    import torch
    rng = np.random.default_rng(6)
    n, H, W, roi = 2, 12, 1300, (5, 0, 1290, 12)
    dl, dr = _maps(rng, (n, H, W))
    tl, tr, tv = _dev(dl, dr, _guide(rng, "mixed", (n, H, W), 3))
    tv2 = torch.from_numpy(_guide(rng, "noise", (n, H, W), 3)).cuda()

    def call(f):
        guide = tv.clone()
        out = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
        f.filter(tl, guide, out, tr, roi)                     # warm-up outside the capture: workspace, tables, side stream
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(graph, stream=s):
                f.filter(tl, guide, out, tr, roi)
        first = out.clone()
        out.zero_(); graph.replay(); torch.cuda.synchronize()
        assert torch.equal(out, first)
        guide.copy_(tv2)                                      # the guide is new on every call: a replay reads it afresh
        out.zero_(); graph.replay(); torch.cuda.synchronize()
        assert not torch.equal(out, first)
        assert torch.equal(out, f.filter(tl, tv2, None, tr, roi))
        return out

    _ab(adf, True, call, fused_first=True)
