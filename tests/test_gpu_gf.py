"""GPU tests of the guided filter (csrc/guided_filter_kernels.hip; include/adf_wls.h: adf_guided_filter_*).

Every case is compared bit for bit with the direct statement tests/gf_ref.py (float outputs as uint32); every case runs
twice and must give identical bytes and leave guide and source unwritten.  A workgroup's output tile is 32 x 8 (TW x TH in
the kernel file), so the shapes are widths {1, TW-1, TW, TW+1, 2 TW+1} by heights {1, TH-1, TH, TH+1}, and the radii
{0, 1, 2, TH, 31} take the halo past the tile and past the image; every case is a few thousand pixels at the most."""
import numpy as np
import pytest

from gf_ref import guided_filter, window_sum

pytestmark = pytest.mark.gpu

TW, TH = 32, 8
BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}
DEPTHS = [np.uint8, np.int16, np.float32]


def _dev():
    import torch

    return torch.device("cuda:0")


def _ddepth(adf, dtype):
    return {None: -1, np.uint8: adf.CV_8U, np.int16: adf.CV_16S, np.float32: adf.CV_32F}[dtype]


def _src(rng, shape, dtype):
    """Steps, noise and the ends of the range next to each other; float maps carry fractions (finite values only)."""
    if dtype == np.float32:
        s = rng.choice(np.array([-2.5, 0.0, 16.25, 480.0, 2000.125], np.float32), shape)
        noisy = rng.random(shape) < 0.3
        s[noisy] = (rng.standard_normal(int(noisy.sum())) * 300).astype(np.float32)
        return s
    if dtype == np.int16:
        s = rng.choice(np.array([16, 480, 2000, -16], np.int16), shape)
        noisy = rng.random(shape) < 0.3
        s[noisy] = rng.integers(-32768, 32768, int(noisy.sum())).astype(np.int16)
        ends = rng.random(shape) < 0.1
        s[ends] = rng.choice(np.array([32767, -32767, -32768], np.int16), int(ends.sum()))
        return s
    s = rng.choice(np.array([0, 1, 7, 128, 255], np.uint8), shape)
    noisy = rng.random(shape) < 0.3
    s[noisy] = rng.integers(0, 256, int(noisy.sum())).astype(np.uint8)
    return s


def _guide(rng, shape, ch):
    """Smooth regions with edges and a little noise, and a flat patch where every covariance vanishes."""
    H, W = shape[-2:]
    base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
    g = np.clip(base[..., None] + rng.integers(-6, 7, tuple(shape) + (ch,)), 0, 255).astype(np.uint8)
    g[..., H // 2:, W // 2:, :] = 90
    return g if ch == 3 else g[..., 0]


def _expected(guide, src, r, eps, dst_dtype):
    if src.ndim == 2:
        return guided_filter(guide, src, r, eps, dst_dtype)
    return np.stack([guided_filter(guide[k], src[k], r, eps, dst_dtype) for k in range(len(src))])


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def _check(adf, guide, src, r, eps=1.0, dst_dtype=None, to_dev=None):
    """Runs the device call twice on (views of) device copies and compares with the statement."""
    import torch

    to_dev = to_dev or (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev()))
    tg, ts = to_dev(guide), to_dev(src)
    out1 = adf.guidedFilter(tg, ts, r, eps, _ddepth(adf, dst_dtype))
    out2 = adf.guidedFilter(tg, ts, r, eps, _ddepth(adf, dst_dtype))
    torch.cuda.synchronize()
    exp = _expected(guide, src, r, eps, dst_dtype)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert got1.dtype == exp.dtype
    assert _same_bits(got1, got2), "two runs differ"
    assert _same_bits(ts.cpu().numpy(), src) and np.array_equal(tg.cpu().numpy(), guide), "an input was written"
    bad = np.ascontiguousarray(got1).view(BITS[exp.dtype]) != np.ascontiguousarray(exp).view(BITS[exp.dtype])
    assert not bad.any(), "%d pixels differ from the statement, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    return got1


@pytest.mark.parametrize("W", [1, TW - 1, TW, TW + 1, 2 * TW + 1])
@pytest.mark.parametrize("H", [1, TH - 1, TH, TH + 1])
def test_shapes_around_the_tile(adf, W, H):
    rng = np.random.default_rng(W * 100 + H)
    _check(adf, _guide(rng, (H, W), 1), _src(rng, (H, W), np.int16), 2, 1.0)
    _check(adf, _guide(rng, (H, W), 3), _src(rng, (H, W), np.int16), 2, 1.0, np.float32)


@pytest.mark.parametrize("r", [0, 1, 2, TH, 31])
@pytest.mark.parametrize("ch", [1, 3])
def test_radii(adf, r, ch):
    rng = np.random.default_rng(r * 10 + ch)
    H, W = 21, 45
    got = _check(adf, _guide(rng, (H, W), ch), _src(rng, (H, W), np.int16), r, 4.0, np.float32)
    assert np.isfinite(got).all()
    src = _src(rng, (3, 2), np.float32)                                  # an image far smaller than the window
    _check(adf, _guide(rng, (3, 2), ch), src, r, 4.0)


@pytest.mark.parametrize("src_dtype", DEPTHS)
@pytest.mark.parametrize("dst_dtype", DEPTHS)
@pytest.mark.parametrize("ch", [1, 3])
def test_source_and_output_depths(adf, src_dtype, dst_dtype, ch):
    rng = np.random.default_rng(ch * 7 + DEPTHS.index(src_dtype) * 3 + DEPTHS.index(dst_dtype))
    H, W = 19, 37
    src = _src(rng, (H, W), src_dtype)
    got = _check(adf, _guide(rng, (H, W), ch), src, 3, 2.0, dst_dtype)
    assert got.dtype == np.dtype(dst_dtype)
    assert not np.array_equal(got.astype(np.float64), src.astype(np.float64))              # the case is not vacuous


@pytest.mark.parametrize("eps", [0.01, 1.0, 6502.5])
@pytest.mark.parametrize("ch", [1, 3])
def test_eps(adf, eps, ch):
    rng = np.random.default_rng(int(eps) + ch)
    H, W = 19, 37
    for dtype in (np.int16, np.float32):
        _check(adf, _guide(rng, (H, W), ch), _src(rng, (H, W), dtype), 4, eps, np.float32)


def test_int16_extremes_and_saturating_outputs(adf):
    rng = np.random.default_rng(21)
    H, W = 17, 35
    ends = rng.choice(np.array([-32768, 32767], np.int16), (H, W))
    for ch in (1, 3):
        noisy = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
        guide = noisy if ch == 3 else noisy[..., 0]
        for eps in (0.01, 100.0):
            # a model fitted to +-32768 against a noisy guide overshoots the int16 range: the output saturates
            got = _check(adf, guide, ends, 1, eps, np.int16)
            assert (got == 32767).any() and (got == -32768).any()
            got8 = _check(adf, guide, ends, 1, eps, np.uint8)
            assert set(np.unique(got8)) <= set(range(256)) and (got8 == 0).any() and (got8 == 255).any()
            _check(adf, guide, ends, 1, eps, np.float32)
    # constant maps at the ends of the range come back as they are
    for v in (-32768, 32767):
        flat = np.full((H, W), v, np.int16)
        assert np.array_equal(_check(adf, _guide(rng, (H, W), 3), flat, 5, 0.5), flat)


@pytest.mark.parametrize("ch", [1, 3])
def test_a_flat_guide_gives_the_box_mean_of_the_box_mean(adf, ch):
    H, W, r = 19, 40, 3
    guide = np.full((H, W, ch) if ch == 3 else (H, W), 117, np.uint8)
    src = np.zeros((H, W), np.int16)
    src[:, W // 2:] = 1600                                               # a step
    got = _check(adf, guide, src, r, 0.01, np.float32)
    # a = 0 exactly (exact covariances: no cancellation error to divide by eps), b = the box mean; q = the box mean of b
    N = (2 * r + 1) ** 2
    b = (window_sum(src.astype(np.int64), r).astype(np.float64) / N).astype(np.float32)
    q = (window_sum(b, r).astype(np.float64) / N).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), q.view(np.uint32))
    assert got.min() == 0.0 and got.max() == 1600.0


def test_padded_and_odd_strides_a_batch_and_a_workspace(adf):
    import torch

    rng = np.random.default_rng(11)
    N, H, W = 3, 13, 41

    def padded(a):                      # a view into a larger tensor: W + 6 pixels per row, a spare row per map
        hw = a.shape[1:3]
        big = torch.zeros((a.shape[0], hw[0] + 1, hw[1] + 6) + a.shape[3:], dtype=torch.from_numpy(a[:0]).dtype, device=_dev())
        v = big[:, :hw[0], 2:2 + hw[1]]
        v.copy_(torch.from_numpy(a))
        return v

    for dtype, ch, ddtype in ((np.uint8, 3, np.int16), (np.int16, 1, np.float32), (np.float32, 3, np.uint8)):
        src, guide = _src(rng, (N, H, W), dtype), _guide(rng, (N, H, W), ch)
        batch = _check(adf, guide, src, 2, 3.0, ddtype, to_dev=padded)
        # the batch equals three single calls
        for k in range(N):
            one = adf.guidedFilter(torch.from_numpy(guide[k]).to(_dev()), torch.from_numpy(src[k]).to(_dev()), 2, 3.0, _ddepth(adf, ddtype))
            assert _same_bits(one.cpu().numpy(), batch[k])
    # ... a destination of that kind, and a caller workspace instead of library scratch
    src, guide = _src(rng, (N, H, W), np.int16), _guide(rng, (N, H, W), 3)
    dst = padded(np.full((N, H, W), 77, np.int16))
    whole = dst._base if dst._base is not None else dst
    ws = torch.empty(adf.guidedFilterWorkspaceBytes(N, H, W, 3), dtype=torch.uint8, device=_dev())
    out = adf.guidedFilter(padded(guide), padded(src), 2, 3.0, dst=dst, workspace=ws)
    assert out is dst
    exp = _expected(guide, src, 2, 3.0, np.int16)
    assert np.array_equal(dst.cpu().numpy(), exp)
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[:, :H, 2:2 + W] = False
    assert (whole[outside] == 0).all(), "written outside the destination's pixels"
    scratch = adf.guidedFilter(torch.from_numpy(guide).to(_dev()), torch.from_numpy(src).to(_dev()), 2, 3.0)
    assert np.array_equal(scratch.cpu().numpy(), exp)
    with pytest.raises(adf.AdfError) as e:                               # a workspace one byte short
        adf.guidedFilter(padded(guide), padded(src), 2, 3.0, dst=dst, workspace=ws[:-1])
    assert e.value.code == 2


def test_host_entry_and_the_filter_object(adf):
    import torch

    rng = np.random.default_rng(12)
    src, guide = _src(rng, (2, 11, 35), np.int16), _guide(rng, (2, 11, 35), 3)
    keep = src.copy(), guide.copy()
    out = adf.guidedFilter(guide[:, :, 1:], src[:, :, 1:], 3, 2.0, adf.CV_32F)             # strided host arrays
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    exp = _expected(guide[:, :, 1:], src[:, :, 1:], 3, 2.0, np.float32)
    assert _same_bits(out, exp)
    assert np.array_equal(src, keep[0]) and np.array_equal(guide, keep[1])
    tg, ts = torch.from_numpy(np.ascontiguousarray(guide[:, :, 1:])).to(_dev()), torch.from_numpy(np.ascontiguousarray(src[:, :, 1:])).to(_dev())
    assert _same_bits(adf.guidedFilter(tg, ts, 3, 2.0, adf.CV_32F).cpu().numpy(), out)     # the device entry gives the host entry's bytes
    gf = adf.createGuidedFilter(tg, 3, 2.0)
    assert isinstance(gf, adf.GuidedFilter)
    assert _same_bits(gf.filter(ts, dDepth=adf.CV_32F).cpu().numpy(), out)
    assert _same_bits(gf.filter(ts).cpu().numpy(), _expected(guide[:, :, 1:], src[:, :, 1:], 3, 2.0, None))
    host = adf.createGuidedFilter(guide[0], 3, 2.0).filter(src[0])
    assert _same_bits(host, guided_filter(guide[0], src[0], 3, 2.0))


def test_captured_into_a_graph(adf):
    import torch

    rng = np.random.default_rng(14)
    H, W = 40, 70
    src, guide = _src(rng, (H, W), np.int16), _guide(rng, (H, W), 3)
    ts, tg = torch.from_numpy(src).to(_dev()), torch.from_numpy(guide).to(_dev())
    dst = torch.zeros_like(ts)
    ws = torch.empty(adf.guidedFilterWorkspaceBytes(1, H, W, 3), dtype=torch.uint8, device=_dev())
    warm = adf.guidedFilter(tg, ts, 4, 1.0).cpu().numpy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        adf.guidedFilter(tg, ts, 4, 1.0, dst=dst, workspace=ws)
    dst.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), warm)
    assert np.array_equal(warm, guided_filter(guide, src, 4, 1.0))
