"""The device preparation of the matcher's views (resize to half size, cvtColor BGR2GRAY, and both fused:
csrc/view_prep_kernels.hip) bit for bit against the NumPy reference of tests/test_view_prep_ref.py: the four cases over
shapes, batches and extreme contents; strides, misaligned bases, interleaved batches and guard bytes; host entry,
streams, graph capture; and the sample's default pipeline from colour views without leaving the device.  Every
comparison is array_equal: there is no tolerance anywhere in this feature."""
import os

import numpy as np
import pytest

import tutorial_replay as tr
from test_view_prep_ref import batch_ref, half_of, view_prep_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (source channels, half, gray)
CASES = {"shrink_colour": (3, True, False), "shrink_gray": (1, True, False), "gray": (3, False, True),
         "fused": (3, True, True)}
SHAPES = [(2, 2), (3, 3), (17, 5), (64, 64), (1023, 7), (1024, 436), (1242, 375), (1920, 1080), (3840, 2160)]   # W, H


def _dev():
    import torch

    return torch.device("cuda:0")


def run_case(adf, case, t, **kw):
    """The public call of `case` on a tensor / array."""
    if case == "gray":
        return adf.cvtColor(t, adf.COLOR_BGR2GRAY, **kw)
    if case == "fused":
        return adf.matcherViews(t, 0.5, True, **kw)
    return adf.resize(t, None, 0.5, 0.5, **kw)


def residues_image(n, H, W, c):
    """Multiples of 4 everywhere, plus 0..3 on the top-left pixel of every 2x2 cell, cycling with cell position and
    channel: the cell sums hit every residue mod 4 in every channel (the + 2 >> 2 rounding is exercised)."""
    rng = np.random.default_rng(W * 31 + H)
    a = (rng.integers(0, 63, (n, H, W, c)) * 4).astype(np.uint8)
    yy, xx = np.mgrid[0:(H + 1) // 2, 0:(W + 1) // 2]
    for k in range(c):
        a[:, 0::2, 0::2, k] += ((xx + yy + k) % 4).astype(np.uint8)
    return a


def contents(name, n, H, W, c):
    if name == "random":
        return np.random.default_rng(H * 4099 + W * 3 + n).integers(0, 256, (n, H, W, c), dtype=np.uint8)
    if name == "zeros":
        return np.zeros((n, H, W, c), np.uint8)
    if name == "ones":
        return np.full((n, H, W, c), 255, np.uint8)
    return residues_image(n, H, W, c)


def test_residues_image_hits_every_residue():
    a = residues_image(1, 64, 64, 3)[0].astype(np.int32)
    s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    for k in range(3):
        assert set(np.unique(s[:, :, k] % 4)) == {0, 1, 2, 3}


# ---- 4. the four cases x shapes x batches x contents ----
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_cases_shapes_batches(adf, case, W, H, n):
    import torch

    c, half, gray = CASES[case]
    for name in ("random", "zeros", "ones", "residues"):
        a = contents(name, n, H, W, c)
        if c == 1:
            a = a[..., 0]
        src = a if n > 1 else a[0]
        if c == 1 and n > 1 and W == 3:
            src = src[..., None]                  # (3, H, 3) would read as one colour image: a gray batch says (N,H,W,1)
        got = run_case(adf, case, torch.from_numpy(np.ascontiguousarray(src)).to(_dev())).cpu().numpy()
        if src.ndim == 4 and c == 1:
            assert got.shape[-1] == 1
            got = got[..., 0]
        exp = batch_ref(a, half, gray)
        exp = exp if n > 1 else exp[0]
        assert got.shape == exp.shape and got.dtype == np.uint8, (name, got.shape, exp.shape)
        assert np.array_equal(got, exp), (case, W, H, n, name)


# ---- 5. fused == shrink colour, then gray ----
@pytest.mark.parametrize("W,H", [(3, 3), (17, 5), (1024, 436), (1242, 375), (1243, 377), (1920, 1080)])
def test_fused_equals_two_steps(adf, W, H):
    import torch

    a = torch.from_numpy(contents("random", 2, H, W, 3)).to(_dev())
    two = adf.cvtColor(adf.resize(a, None, 0.5, 0.5), adf.COLOR_BGR2GRAY)
    assert torch.equal(adf.matcherViews(a), two)
    assert torch.equal(adf.resize(a, (half_of(W), half_of(H))), adf.resize(a, None, 0.5, 0.5))     # dsize = (width, height)
    assert torch.equal(adf.matcherViews(a, 0.5, False), adf.resize(a, None, 0.5, 0.5))
    assert torch.equal(adf.matcherViews(a, 1.0, True), adf.cvtColor(a, adf.COLOR_BGR2GRAY))


# ---- 6. strides, misaligned bases, sliced views, interleaved batches, guard bytes ----
def _strided(buf, offset, shape, strides):
    import torch

    return torch.as_strided(buf, shape, strides, offset)


@pytest.mark.parametrize("W,H", [(64, 48), (37, 21), (35, 19)])
@pytest.mark.parametrize("case", list(CASES))
def test_strides_offsets_and_guard_bytes(adf, case, W, H):
    import torch

    c, half, gray = CASES[case]
    dc = 1 if gray else c
    w, h = (half_of(W), half_of(H)) if half else (W, H)
    n = 2
    a = contents("random", n, H, W, c)
    exp = batch_ref(a if c == 3 else a[..., 0], half, gray)
    srow, drow = W * c, w * dc
    # (source row stride, destination row stride): aligned for the vector path, and not
    for sstride, dstride in ((-(-srow // 16) * 16 + 16, -(-drow // 16) * 16 + 32), (srow + 5, drow + 3), (srow, drow)):
        simg, dimg = sstride * H + 48, dstride * h + 32
        for soff in range(8):
            doff = (soff * 3) % 8 if soff else 0
            sbuf = torch.zeros(16 + n * simg + 16, dtype=torch.uint8, device=_dev())
            dbuf = torch.full((16 + n * dimg + 16,), 0xA5, dtype=torch.uint8, device=_dev())
            assert sbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
            sshape = (n, H, W, 3) if c == 3 else (n, H, W)
            dshape = (n, h, w, 3) if dc == 3 else (n, h, w)
            sv = _strided(sbuf, soff, sshape, (simg, sstride, 3, 1) if c == 3 else (simg, sstride, 1))
            dv = _strided(dbuf, doff, dshape, (dimg, dstride, 3, 1) if dc == 3 else (dimg, dstride, 1))
            sv.copy_(torch.from_numpy(a if c == 3 else a[..., 0]).to(_dev()))
            out = run_case(adf, case, sv, dst=dv)
            assert out is dv
            assert np.array_equal(dv.cpu().numpy(), exp), (case, sstride, dstride, soff, doff)
            guard = torch.full_like(dbuf, 0xA5)
            _strided(guard, doff, dshape, dv.stride()).copy_(dv)
            assert torch.equal(guard, dbuf), "bytes outside the destination rows were written"


def test_sliced_view_and_interleaved_pairs(adf):
    import torch

    H, W = 46, 80
    rng = np.random.default_rng(9)
    big = torch.from_numpy(rng.integers(0, 256, (3, H + 6, W + 10, 3), dtype=np.uint8)).to(_dev())
    view = big[:, 3:3 + H, 5:5 + W]                                          # non-contiguous: rows and images strided
    assert not view.is_contiguous()
    exp = batch_ref(view.cpu().numpy(), True, True)
    assert np.array_equal(adf.matcherViews(view).cpu().numpy(), exp)
    # left and right interleaved row by row: image k starts one row after image k-1, rows are two rows apart
    inter = torch.from_numpy(rng.integers(0, 256, (H, 2, W, 3), dtype=np.uint8)).to(_dev())
    pair = inter.permute(1, 0, 2, 3)
    assert pair.stride(0) == W * 3 and pair.stride(1) == 2 * W * 3
    dst_store = torch.full((H // 2, 2, W // 2 + 8), 0x3C, dtype=torch.uint8, device=_dev())
    dst = dst_store[:, :, :W // 2].permute(1, 0, 2)                           # interleaved destination, padded rows
    out = adf.matcherViews(pair, dst=dst)
    assert out is dst
    assert np.array_equal(dst.cpu().numpy(), batch_ref(pair.cpu().numpy(), True, True))
    assert bool((dst_store[:, :, W // 2:] == 0x3C).all()), "the padding was written"
    # "all left views, then all right views" in one call equals two calls
    lr = torch.from_numpy(rng.integers(0, 256, (2, 4, H, W, 3), dtype=np.uint8)).to(_dev())
    both = adf.matcherViews(lr.view(8, H, W, 3)).view(2, 4, H // 2, W // 2)
    assert torch.equal(both[0], adf.matcherViews(lr[0])) and torch.equal(both[1], adf.matcherViews(lr[1]))


# ---- 7. host entry, streams, graph capture ----
@pytest.mark.parametrize("case", list(CASES))
def test_host_entry_equals_device_entry(adf, case):
    import torch

    c, half, gray = CASES[case]
    for n, H, W in ((1, 436, 1024), (3, 37, 51), (2, 375, 1242)):
        a = contents("random", n, H, W, c)
        a = a if c == 3 else a[..., 0]
        src = a if n > 1 else a[0]
        host = run_case(adf, case, src)
        assert isinstance(host, np.ndarray)
        dev = run_case(adf, case, torch.from_numpy(np.ascontiguousarray(src)).to(_dev())).cpu().numpy()
        assert np.array_equal(host, dev)
        exp = batch_ref(a, half, gray)
        assert np.array_equal(host, exp if n > 1 else exp[0])
    # a host view with padded rows
    big = contents("random", 1, 40, 70, c)[0]
    big = big if c == 3 else big[..., 0]
    sl = big[2:36, 3:63]
    assert np.array_equal(run_case(adf, case, sl), view_prep_ref(sl, half, gray))


def test_non_default_stream(adf):
    import torch

    a = contents("random", 4, 1080, 1920, 3)
    exp = batch_ref(a, True, True)
    s = torch.cuda.Stream(device=_dev())
    for _ in range(2):
        t = torch.from_numpy(a).to(_dev())
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = adf.matcherViews(t)
        torch.cuda.current_stream().wait_stream(s)
        assert np.array_equal(got.cpu().numpy(), exp)


def test_graph_capture_and_replays(adf):
    import torch

    H, W = 270, 480
    static = torch.from_numpy(contents("random", 2, H, W, 3)).to(_dev())
    out = torch.zeros((2, H // 2, W // 2), dtype=torch.uint8, device=_dev())
    adf.matcherViews(static, dst=out)                                         # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                 # one linear graph: a single kernel node
        adf.matcherViews(static, dst=out)
    for seed in (41, 42, 43):
        fresh = np.random.default_rng(seed).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        static.copy_(torch.from_numpy(fresh).to(_dev()))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), batch_ref(fresh, True, True)), seed


# ---- 8. the sample's default pipeline from colour views, on the device ----
def _filter_chain(adf, matcher, gl, gr, left_view, both):
    wls = adf.createDisparityWLSFilter(matcher)
    if both:
        dl, dr = matcher.computeBoth(gl, gr)
    else:
        right = adf.createRightMatcher(matcher)
        dl, dr = matcher.compute(gl, gr), right.compute(gr, gl)
    wls.setLambda(tr.LAMBDA)
    wls.setSigmaColor(tr.SIGMA)
    out = wls.filter(dl, left_view, None, dr)
    return out.cpu().numpy(), wls.getConfidenceMap().cpu().numpy(), wls.getROI(), dl.cpu().numpy(), dr.cpu().numpy()


def test_default_pipeline_bm_from_colour_views_on_the_device(adf):
    import torch

    left, right, _, _ = tr.load_fixtures()
    hl, hr, nd = tr.matcher_views(left, right)                                # the host preparation the replay test gates
    views = torch.from_numpy(np.stack([left, right])).to(_dev())             # full-size colour, in HBM for the filter anyway
    g = adf.matcherViews(views)                                               # SAMPLE:137-138, 155-156 in one launch
    assert np.array_equal(g.cpu().numpy(), np.stack([hl, hr]))
    got = _filter_chain(adf, adf.StereoBM.create(nd, tr.WSIZE), g[0], g[1], views[0], True)
    exp = _filter_chain(adf, adf.StereoBM.create(nd, tr.WSIZE), torch.from_numpy(hl).to(_dev()),
                        torch.from_numpy(hr).to(_dev()), torch.from_numpy(left).to(_dev()), True)
    assert got[2] == exp[2]
    for a, b, what in zip(got, exp, ("filtered map", "confidence map", "ROI", "left disparity", "right disparity")):
        assert np.array_equal(a, b), what
    assert got[0].shape == left.shape[:2] and (got[0] != got[0].flat[0]).any()


def test_default_pipeline_sgbm_from_colour_views_on_the_device(adf):
    import torch

    left, right, _, _ = tr.load_fixtures()
    nd = tr.matcher_views(left, right)[2]

    def matcher():
        m = adf.StereoSGBM.create(0, nd, 3)                                   # SAMPLE:166-170
        m.setP1(24 * 9); m.setP2(96 * 9); m.setPreFilterCap(63); m.setMode(adf.StereoSGBM.MODE_SGBM_3WAY)
        return m

    views = torch.from_numpy(np.stack([left, right])).to(_dev())
    small = adf.resize(views, None, 0.5, 0.5)                                 # SGBM takes the colour views (SAMPLE:137-138)
    hl, hr = tr.half_size(left), tr.half_size(right)
    assert np.array_equal(small.cpu().numpy(), np.stack([hl, hr]))
    got = _filter_chain(adf, matcher(), small[0], small[1], views[0], False)
    exp = _filter_chain(adf, matcher(), torch.from_numpy(hl).to(_dev()), torch.from_numpy(hr).to(_dev()),
                        torch.from_numpy(left).to(_dev()), False)
    assert got[2] == exp[2]
    for a, b, what in zip(got, exp, ("filtered map", "confidence map", "ROI", "left disparity", "right disparity")):
        assert np.array_equal(a, b), what


# ---- 9. KITTI: 1242 x 375 -> 621 x 188, the odd-size tail end to end ----
def test_kitti_odd_size_end_to_end(adf):
    import torch
    from PIL import Image

    left = np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, "kitti_left.bmp")).convert("RGB"))[:, :, ::-1])
    right = np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, "kitti_right.bmp")).convert("RGB"))[:, :, ::-1])
    assert left.shape == (375, 1242, 3)
    views = torch.from_numpy(np.stack([left, right])).to(_dev())
    for case, (c, half, gray) in CASES.items():
        a = views if c == 3 else views[..., 1].contiguous()
        got = run_case(adf, case, a).cpu().numpy()
        assert np.array_equal(got, batch_ref(a.cpu().numpy(), half, gray)), case
    g = adf.matcherViews(views)
    assert tuple(g.shape) == (2, 188, 621)
    bm = adf.StereoBM.create(64, 9)
    wls = adf.createDisparityWLSFilter(bm)
    dl, dr = bm.computeBoth(g[0], g[1])
    assert tuple(dl.shape) == (188, 621)
    wls.setLambda(tr.LAMBDA)
    wls.setSigmaColor(tr.SIGMA)
    out = wls.filter(dl, views[0], None, dr)                                  # 621 x 188 maps, 1242 x 375 guide
    torch.cuda.synchronize()
    assert tuple(out.shape) == (375, 1242) and out.dtype == torch.int16
    x, y, w, h = wls.getROI()
    assert w > 0 and h > 0
    assert tuple(wls.getConfidenceMap().shape) == (375, 1242)
    assert (out != out[0, 0]).any()
