"""reprojectImageTo3D / pointCloud on the device (csrc/reproject_kernels.hip) against the direct NumPy statement
tests/reproject_ref.py.  Comparison rule: NaN positions are equal, and everywhere else the uint32 bit patterns are equal
(the sign and payload of a NaN are not part of the contract: x86 and the GPU differ there).

The shapes straddle what the kernels cut the work into: four pixels per thread (row tails of 1..3), 256 threads per
workgroup, 64-pixel waves and 1024-pixel tiles of the point list (more than one tile, a last tile of one pixel)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import reproject_ref as ref
from test_reproject_ref import Q_FULL, rectified_q

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (7, 4), (9, 8), (33, 63), (37, 211), (64, 128), (65, 129)]
DTYPES = [np.int16, np.float32]
Q_KITTI = rectified_q()                                  # KITTI-like: f 721.5, principal point (609.6, 172.9), B 0.54
Q_INF = rectified_q(cx=10.0, cy=3.0)                     # r_3 = d / B: zero where d == 0
Q_ZERO_ROW = np.vstack([Q_FULL[:3], np.zeros((1, 4))])   # r_3 = 0 everywhere
QS = [Q_KITTI, Q_FULL, Q_INF, Q_ZERO_ROW]
SCALES = [1.0, 1.0 / 16, 0.1]
EPS = np.float32(ref.FLT_EPSILON)
SENTINEL = 777.0


def _dev():
    import torch
    return torch.device("cuda", 0)


def same_bits(got, expect):
    got, expect = np.ascontiguousarray(got), np.ascontiguousarray(expect)
    if got.shape != expect.shape or got.dtype != expect.dtype:
        return False
    nan = np.isnan(expect)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], expect.view(np.uint32)[~nan]))


def make_map(shape, dtype, seed, variant=0):
    """Random disparities with the values the contract names sprinkled in.  int16: -32768 / 32767 / -16 / 0 (variants 1
    and 2 leave the extremes out: the minimum is -16 / -48).  float32, variant 0: NaN, +-inf, subnormals, -0.0; variant 1: no
    -inf and nothing negative, so the minimum is a zero, with neighbours within and just beyond FLT_EPSILON of it;
    variant 2: the same shifted by 3.5 (another minimum)."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    if dtype == np.int16:
        d = rng.integers(1, 4000, n).astype(np.int16)
        special = [[-32768, 32767, -16, 0], [-16, 0, -16, 17], [-48, 0, -48, 17]][variant]
    else:
        d = (rng.random(n) * 250 + 0.5).astype(np.float32)
        if variant == 0:
            special = [np.nan, np.inf, -np.inf, 1e-40, -1e-42, -0.0, 0.0]
        else:
            special = [0.0, -0.0, EPS, EPS * np.float32(0.5), np.nextafter(EPS, np.float32(1)), 2 * EPS, 1e-40, np.nan, np.inf]
    pos = rng.permutation(n)[:2 * len(special)]
    for k, p in enumerate(pos):
        d[p] = special[k % len(special)]
    if dtype == np.float32 and variant == 2:
        d = (d + np.float32(3.5)).astype(np.float32)
    return d.reshape(shape)


# ---- layouts ----
def place(torch, a, layout):
    """A device tensor with a's values in the layout named; rows stay dense."""
    dev = _dev()
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if layout in ("contiguous", "batch"):
        return t
    H, W = a.shape[-2], a.shape[-1]
    if layout == "odd_stride":
        pad = next(p for p in range(1, 9) if ((W + p) * a.dtype.itemsize) % 8 != 0)
        big = torch.zeros(a.shape[:-1] + (W + pad,), dtype=t.dtype, device=dev)
        big[..., :W] = t
        return big[..., :W]
    if layout == "offset4":
        off = 4 // a.dtype.itemsize
        flat = torch.zeros(a.size + off, dtype=t.dtype, device=dev)
        flat[off:] = t.reshape(-1)
        return flat[off:].view(a.shape)
    if layout == "view":                                  # every second row of a taller tensor
        big = torch.zeros(a.shape[:-2] + (2 * H, W), dtype=t.dtype, device=dev)
        big[..., ::2, :] = t
        return big[..., ::2, :]
    raise AssertionError(layout)


def make_dst(torch, shape, layout):
    """(dst, whole): a float32 destination of `shape` (..., H, W[, 3]) in the layout named, inside `whole`, which is
    filled with SENTINEL."""
    dev = _dev()
    if layout in ("contiguous", "batch"):
        whole = torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
        return whole, whole
    ch3 = len(shape) >= 3 and shape[-1] == 3
    hw = len(shape) - (3 if ch3 else 2)                   # index of H
    H, W = shape[hw], shape[hw + 1]
    if layout == "odd_stride":
        pad = next(p for p in range(1, 9) if ((W + p) * (12 if ch3 else 4)) % 16 != 0)
        whole = torch.full(shape[:hw + 1] + (W + pad,) + shape[hw + 2:], SENTINEL, dtype=torch.float32, device=dev)
        return whole[(slice(None),) * (hw + 1) + (slice(0, W),)], whole
    if layout == "offset4":
        n = int(np.prod(shape))
        whole = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=dev)
        return whole[1:].view(shape), whole
    if layout == "view":
        whole = torch.full(shape[:hw] + (2 * H,) + shape[hw + 1:], SENTINEL, dtype=torch.float32, device=dev)
        return whole[(slice(None),) * hw + (slice(0, 2 * H, 2),)], whole
    raise AssertionError(layout)


LAYOUTS = ["contiguous", "odd_stride", "offset4", "view", "batch"]


def _run_case(adf, torch, disp, layout, Q, scale, mode, z_only):
    """One call against the statement; the destination's surroundings must keep the sentinel."""
    kw, rkw = {}, {}
    if mode == ref.MISSING_MIN:
        kw["handleMissingValues"] = True
    elif mode == ref.MISSING_VALUE:
        mv = -16.0 if disp.dtype == np.int16 else 0.0
        kw["missingValue"] = mv
        rkw["missing_value"] = mv
    expect = ref.reproject(disp, Q, scale, mode, **rkw)
    if z_only:
        expect = np.ascontiguousarray(expect[..., 2])
    src = place(torch, disp, layout)
    dst, whole = make_dst(torch, expect.shape, layout)
    out = adf.reprojectImageTo3D(src, Q, dst=dst, dispScale=scale, zOnly=z_only, **kw)
    assert out is dst
    got = dst.cpu().numpy()
    assert same_bits(got, expect), (disp.shape, disp.dtype, layout, scale, mode, z_only)
    if whole is not dst:                                  # nothing but the destination's pixels was written
        dst.fill_(SENTINEL)
        assert bool((whole == SENTINEL).all()), (disp.shape, layout)


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_image_layouts(adf, shape, dtype):
    """Every layout x {XYZ, Z}; the (Q, scale, mode) combination rotates so that each layout meets several."""
    import torch

    combos = itertools.cycle(itertools.product(range(len(QS)), SCALES, (ref.MISSING_MIN, ref.MISSING_NONE, ref.MISSING_VALUE)))
    for _ in range(SHAPES.index(shape) * 7):
        next(combos)
    for layout in LAYOUTS:
        for z_only in (False, True):
            for variant in (0, 1):
                qi, scale, mode = next(combos)
                if layout == "batch":
                    disp = np.stack([make_map(shape, dtype, 100 + v, v) for v in (0, 1, 2)])
                    if shape[0] * shape[1] >= 64:
                        assert len({ref.map_minimum(d) for d in disp}) == 3
                else:
                    disp = make_map(shape, dtype, 7 + variant, variant)
                _run_case(adf, torch, disp, layout, QS[qi], scale, mode, z_only)


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_image_every_q_scale_and_mode(adf, shape, dtype):
    import torch

    maps = [make_map(shape, dtype, 31 + v, v) for v in (0, 1)]
    batch = np.stack([make_map(shape, dtype, 50 + v, v) for v in (0, 1, 2)])
    for k, (Q, scale, mode) in enumerate(itertools.product(QS, SCALES, (ref.MISSING_NONE, ref.MISSING_MIN, ref.MISSING_VALUE))):
        _run_case(adf, torch, maps[k % 2], "contiguous", Q, scale, mode, False)
        if mode == ref.MISSING_MIN:
            _run_case(adf, torch, batch, "batch", Q, scale, mode, k % 2 == 1)


def test_values_within_flt_epsilon_of_the_minimum(adf):
    """The minimum is exact, -0.0 and +0.0 are one value, and the neighbours split at FLT_EPSILON."""
    import torch

    row = np.array([[5.0, EPS, 0.0, np.nextafter(EPS, np.float32(1)), -0.0, EPS * np.float32(0.5), np.nan, 2 * EPS, 7.0]], np.float32)
    z = adf.reprojectImageTo3D(torch.from_numpy(row).to(_dev()), Q_FULL, handleMissingValues=True, zOnly=True).cpu().numpy()
    assert list(z[0] == 10000) == [False, True, True, False, True, True, False, False, False]
    assert same_bits(z, ref.reproject(row, Q_FULL, mode=ref.MISSING_MIN)[..., 2])
    neg = np.array([[-3.25, -3.25 + 1e-7, -3.0, np.inf, -1e-40]], np.float32)
    z = adf.reprojectImageTo3D(torch.from_numpy(neg).to(_dev()), Q_FULL, handleMissingValues=True, zOnly=True).cpu().numpy()
    assert same_bits(z, ref.reproject(neg, Q_FULL, mode=ref.MISSING_MIN)[..., 2]) and z[0, 0] == 10000 and z[0, 2] != 10000
    lo = np.array([[-32768, 32767, -32768, 5]], np.int16)
    z = adf.reprojectImageTo3D(torch.from_numpy(lo).to(_dev()), Q_KITTI, handleMissingValues=True, zOnly=True).cpu().numpy()
    assert list(z[0] == 10000) == [True, False, True, False]


def test_host_entry_gives_the_same_bits(adf):
    for dtype in DTYPES:
        disp = np.stack([make_map((37, 211), dtype, 3 + v, v) for v in (0, 1, 2)])
        for mode, kw in ((ref.MISSING_NONE, {}), (ref.MISSING_MIN, {"handleMissingValues": True})):
            got = adf.reprojectImageTo3D(disp, Q_FULL, dispScale=0.1, **kw)
            assert isinstance(got, np.ndarray) and same_bits(got, ref.reproject(disp, Q_FULL, 0.1, mode))
        z = adf.reprojectImageTo3D(disp[1][:, 3:200], Q_KITTI, zOnly=True)                  # a sliced host view
        assert same_bits(z, ref.reproject(disp[1][:, 3:200], Q_KITTI)[..., 2])


def test_filter_float_output_to_metres(adf):
    """The chain the float output was built for: matcher -> filterFloat -> reprojectImageTo3D(dispScale = 1/16,
    missingValue = -16) on the Tsukuba pair, all on the device, equals the statement applied to the same float map."""
    import torch
    from test_oracle_bm import load_tsukuba

    left, right, _ = load_tsukuba()
    tl, tr = torch.from_numpy(left).to(_dev()), torch.from_numpy(right).to(_dev())
    bm = adf.StereoBM.create(16, 9)
    wls = adf.createDisparityWLSFilter(bm)
    dl, dr = bm.compute(tl, tr), adf.createRightMatcher(bm).compute(tr, tl)
    f32 = wls.filterFloat(dl, tl, None, dr)
    Q = rectified_q(f=615.0, cx=left.shape[1] / 2.0, cy=left.shape[0] / 2.0, baseline=0.16)
    xyz = adf.reprojectImageTo3D(f32, Q, dispScale=1.0 / 16, missingValue=-16.0)
    host = f32.cpu().numpy()
    expect = ref.reproject(host, Q, 1.0 / 16, ref.MISSING_VALUE, -16.0)
    assert same_bits(xyz.cpu().numpy(), expect)
    assert (host == -16.0).any() and np.array_equal(expect[..., 2] == 10000, host == -16.0)
    inside = expect[..., 2][(host > 16.0)]
    assert inside.size > host.size // 4 and 0.5 < float(np.median(inside)) < 100.0        # metres, not fixed-point units


def test_captured_call_replays_to_the_same_bits(adf):
    import torch

    disp = np.stack([make_map((37, 211), np.float32, 60 + v, v) for v in (0, 1, 2)])
    src = torch.from_numpy(disp).to(_dev())
    eager = adf.reprojectImageTo3D(src, Q_FULL, handleMissingValues=True, dispScale=0.1).clone()
    assert same_bits(eager.cpu().numpy(), ref.reproject(disp, Q_FULL, 0.1, ref.MISSING_MIN))
    buf = torch.zeros(adf.reprojectWorkspaceBytes(3), dtype=torch.uint8, device=_dev())
    out = torch.zeros_like(eager)
    adf.reprojectImageTo3D(src, Q_FULL, handleMissingValues=True, dispScale=0.1, dst=out, buf=buf)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=s):
            adf.reprojectImageTo3D(src, Q_FULL, handleMissingValues=True, dispScale=0.1, dst=out, buf=buf)
    for _ in range(2):
        out.zero_()
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), eager.cpu().numpy())


# =============================================================================================
# the point list
# =============================================================================================
CLOUD_SHAPES = [(1, 63), (1, 64), (1, 65), (3, 341), (4, 256), (5, 205), (16, 256), (16, 257), (37, 211), (65, 129), (128, 130)]
MASKS = ["all", "none", "first", "last", "checkerboard", "half", "percent", "row"]


def make_mask(shape, name, seed=0):
    H, W = shape
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, bool)
    if name == "all":
        m[:] = True
    elif name == "first":
        m[0, 0] = True
    elif name == "last":
        m[-1, -1] = True
    elif name == "checkerboard":
        m = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
    elif name == "half":
        m = rng.random(shape) < 0.5
    elif name == "percent":
        m = rng.random(shape) < 0.01
    elif name == "row":
        m[H // 2] = True
    return m


def masked_map(shape, dtype, mask, seed):
    """Positive disparities where the mask holds, the filters' fill (-16) elsewhere: missingValue = -16 makes the mask."""
    rng = np.random.default_rng(seed)
    d = (rng.random(shape) * 200 + 1).astype(dtype) if dtype == np.float32 else rng.integers(1, 3000, shape).astype(dtype)
    d[~mask] = -16
    return d


def check_list(got, expect, what):
    (P, Cl, I, n), (eP, eC, eI) = got, expect
    assert n == len(eP), what
    assert same_bits(P.cpu().numpy() if hasattr(P, "cpu") else P, eP), what
    if eC is not None:
        assert np.array_equal(Cl.cpu().numpy() if hasattr(Cl, "cpu") else Cl, eC), what
    else:
        assert Cl is None
    if I is not None:
        assert np.array_equal(I.cpu().numpy() if hasattr(I, "cpu") else I, eI), what


@pytest.mark.parametrize("shape", CLOUD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_point_list_masks(adf, shape):
    import torch

    rng = np.random.default_rng(shape[1])
    view = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    tv = torch.from_numpy(view).to(_dev())
    for k, name in enumerate(MASKS):
        dtype = DTYPES[k % 2]
        mask = make_mask(shape, name, seed=k)
        disp = masked_map(shape, dtype, mask, seed=k)
        Q, scale = (Q_KITTI, 1.0 / 16) if k % 3 else (Q_FULL, 0.1)
        expect = ref.point_cloud(disp, Q, view, disp_scale=scale, mode=ref.MISSING_VALUE, missing_value=-16.0)
        assert len(expect[0]) == int(mask.sum())
        got = adf.pointCloud(torch.from_numpy(disp).to(_dev()), Q, tv, missingValue=-16.0, dispScale=scale, withIndex=True)
        check_list(got, expect, (shape, name))
        assert tuple(got[0].shape) == (int(mask.sum()), 3) and tuple(got[1].shape) == (int(mask.sum()), 3)


def _raw_call(adf, torch, disp, Q, capacity, view=None, with_index=True, workspace=True):
    """adf_point_cloud_device itself, on sentinel-filled outputs larger than anything it may write."""
    from addingdisparityfiltering_amd import _lib

    dev = _dev()
    n, H, W = disp.shape
    rows = H * W + 8
    src = torch.from_numpy(disp).to(dev)
    points = torch.full((n, rows, 3), SENTINEL, dtype=torch.float32, device=dev)
    vch = 0 if view is None else (1 if view.ndim == 3 else 3)
    tv = None if view is None else torch.from_numpy(view).to(dev)
    colours = None if view is None else torch.full((n, rows, vch), 201, dtype=torch.uint8, device=dev)
    index = torch.full((n, rows), -5, dtype=torch.int32, device=dev) if with_index else None
    counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ws = torch.zeros(adf.pointCloudWorkspaceBytes(n, H, W), dtype=torch.uint8, device=dev) if workspace else None
    prm = _lib.ReprojectParams()
    prm.Q[:] = [float(v) for v in np.asarray(Q).ravel()]
    prm.disp_scale, prm.missing_mode, prm.missing_value = 1.0, _lib.MISSING_VALUE, -16.0
    esz = disp.dtype.itemsize
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = _lib.lib().adf_point_cloud_device(
        n, src.data_ptr(), _lib.DEPTH_16S if disp.dtype == np.int16 else _lib.DEPTH_32F, W * esz, H * W * esz, W, H,
        C.byref(prm), None, -np.inf, np.inf, ptr(tv), W * vch, H * W * vch, vch, points.data_ptr(), rows * 12,
        ptr(colours), rows * vch, ptr(index), rows * 4, int(capacity), counts.data_ptr(),
        ptr(ws), 0 if ws is None else ws.numel(), None)
    _lib.check(rc)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(points), host(colours), host(index), host(counts)


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "float32"])
@pytest.mark.parametrize("shape", [(3, 341), (37, 211)], ids=lambda s: "%dx%d" % s)
def test_point_list_capacity(adf, shape, dtype):
    """capacity 0, count - 1, count, count + 1 (and a cut inside the first tile and at a tile's edge): counts hold the
    full count, entries below min(count, capacity) are the list's, everything beyond keeps the sentinel."""
    import torch

    masks = [make_mask(shape, "half", 1), make_mask(shape, "checkerboard"), make_mask(shape, "all")]
    disp = np.stack([masked_map(shape, dtype, m, 9 + k) for k, m in enumerate(masks)])
    view = np.random.default_rng(2).integers(0, 256, disp.shape + (3,), dtype=np.uint8)
    expect = [ref.point_cloud(d, Q_KITTI, v, mode=ref.MISSING_VALUE, missing_value=-16.0) for d, v in zip(disp, view)]
    count = len(expect[0][0])
    tile_edge = int(np.cumsum(masks[0].ravel())[1023]) if masks[0].size > 1024 else 5
    for capacity in (0, count - 1, count, count + 1, 3, tile_edge, tile_edge + 1):
        P, Cl, I, counts = _raw_call(adf, torch, disp, Q_KITTI, capacity, view)
        for k, (eP, eC, eI) in enumerate(expect):
            assert counts[k] == len(eP), (capacity, k)
            n = min(len(eP), capacity)
            assert same_bits(P[k, :n], eP[:n]) and np.array_equal(Cl[k, :n], eC[:n]) and np.array_equal(I[k, :n], eI[:n]), (capacity, k)
            assert (P[k, n:] == SENTINEL).all() and (Cl[k, n:] == 201).all() and (I[k, n:] == -5).all(), (capacity, k)


def test_point_list_roi_range_colours_index(adf):
    import torch

    shape = (37, 211)
    rng = np.random.default_rng(4)
    view3 = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    view1 = np.ascontiguousarray(view3[..., 1])
    for dtype in DTYPES:
        disp = masked_map(shape, dtype, make_mask(shape, "half", 5), 6)
        disp[3, 7] = 0                                    # r_3 = 0 under a rectified Q: not finite, not in the list
        if dtype == np.float32:
            disp[5, 9], disp[5, 10], disp[6, 11] = np.nan, np.inf, -np.inf
        t = torch.from_numpy(disp).to(_dev())
        base = dict(disp_scale=1.0 / 16, mode=ref.MISSING_VALUE, missing_value=-16.0)
        kw = dict(dispScale=1.0 / 16, missingValue=-16.0)
        # ROI at odd origins, a ROI of one pixel (taken and not taken), the whole map
        for roi in [(3, 5, 101, 17), (1, 1, 209, 35), (7, 3, 1, 1), (8, 3, 1, 1), (209, 35, 2, 2), None]:
            got = adf.pointCloud(t, Q_KITTI, torch.from_numpy(view3).to(_dev()), ROI=roi, withIndex=True, **kw)
            check_list(got, ref.point_cloud(disp, Q_KITTI, view3, roi=roi, **base), (dtype, roi))
        # a z range that cuts the set; an infinite bound switches that side off
        z = ref.reproject(disp, Q_KITTI, 1.0 / 16)[..., 2]
        lo, hi = np.nanpercentile(z[np.isfinite(z) & (disp > 0)], [30, 70])
        for zr in [(float(lo), float(hi)), (-np.inf, float(hi)), (float(lo), np.inf), (float(hi), float(lo))]:
            got = adf.pointCloud(t, Q_KITTI, torch.from_numpy(view1).to(_dev()), zRange=zr, **kw)
            e = ref.point_cloud(disp, Q_KITTI, view1, z_range=zr, **base)
            check_list(got, e, (dtype, zr))
            assert got[2] is None and tuple(got[1].shape) == (len(e[0]), 1)
        assert 0 < adf.pointCloud(t, Q_KITTI, zRange=(float(lo), float(hi)), **kw)[3] < int((disp > 0).sum())
        # without a view, with a capacity: trimmed outputs, the full count
        P, Cl, I, n = adf.pointCloud(t, Q_KITTI, capacity=10, withIndex=True, **kw)
        e = ref.point_cloud(disp, Q_KITTI, **base)
        assert Cl is None and n == len(e[0]) > 10 and same_bits(P.cpu().numpy(), e[0][:10]) and np.array_equal(I.cpu().numpy(), e[2][:10])
        # the host entry: numpy in, numpy out
        got = adf.pointCloud(disp, Q_KITTI, view3, ROI=(3, 5, 101, 17), withIndex=True, **kw)
        assert isinstance(got[0], np.ndarray)
        check_list(got, ref.point_cloud(disp, Q_KITTI, view3, roi=(3, 5, 101, 17), **base), (dtype, "host"))


def test_point_list_batch_and_identity(adf):
    """Three maps with different counts and different minima (handleMissingValues: each map its own), twice."""
    import torch

    shape = (65, 129)
    for dtype in DTYPES:
        disp = np.stack([masked_map(shape, dtype, make_mask(shape, name, 3), 20 + k) for k, name in enumerate(("half", "percent", "row"))])
        disp[1][disp[1] == -16] = -48                     # another minimum
        disp[2] += 40                                     # ... and another
        view = np.random.default_rng(8).integers(0, 256, disp.shape, dtype=np.uint8)
        t, tv = torch.from_numpy(disp).to(_dev()), torch.from_numpy(view).to(_dev())
        first = adf.pointCloud(t, Q_FULL, tv, handleMissingValues=True, withIndex=True)
        again = adf.pointCloud(t, Q_FULL, tv, handleMissingValues=True, withIndex=True)
        assert len({first[3][0], first[3][1], first[3][2]}) == 3
        for k in range(3):
            e = ref.point_cloud(disp[k], Q_FULL, view[k], mode=ref.MISSING_MIN)
            check_list(tuple(part[k] for part in first), e, (dtype, k))
            assert first[3][k] == again[3][k] and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for a, b in zip(first[:3], again[:3]))
        # the library's scratch instead of a caller workspace gives the same list
        P, Cl, I, counts = _raw_call(adf, torch, np.where(disp == disp.min(axis=(1, 2), keepdims=True), -16, disp).astype(dtype), Q_FULL, 10 ** 6, workspace=False)
        for k in range(3):
            e = ref.point_cloud(disp[k], Q_FULL, mode=ref.MISSING_MIN)
            assert counts[k] == len(e[0]) and same_bits(P[k, :counts[k]], e[0]) and np.array_equal(I[k, :counts[k]], e[2])
