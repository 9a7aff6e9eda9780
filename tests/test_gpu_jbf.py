"""GPU tests of the joint bilateral filter (csrc/joint_bilateral_kernels.hip; include/adf_wls.h:
adf_joint_bilateral_filter_*).

Every case is compared bit for bit with the direct statement tests/jbf_ref.py fed with the library's own tables (float
outputs as uint32); every case runs twice and must give identical bytes and leave joint and source unwritten.  A
workgroup's output tile is 32 x 8 (TW x TH in the kernel file), so the shapes are widths {1, TW-1, TW, TW+1, 2 TW+1} by
heights {1, TH-1, TH, TH+1}, and the radii {1, 2, TH, 31} take the halo past the tile and past the image; every case is a
few thousand pixels at the most."""
import numpy as np
import pytest

import jbf_ref

pytestmark = pytest.mark.gpu

TW, TH = 32, 8
BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}
DEPTHS = [np.uint8, np.int16, np.float32]
BORDERS = [jbf_ref.BORDER_REPLICATE, jbf_ref.BORDER_REFLECT, jbf_ref.BORDER_REFLECT_101]


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


def _joint(rng, shape, ch):
    """Smooth regions with edges and a little noise, a flat patch, and a patch of noise over the whole range."""
    H, W = shape[-2:]
    base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
    g = np.clip(base[..., None] + rng.integers(-6, 7, tuple(shape) + (ch,)), 0, 255).astype(np.uint8)
    g[..., H // 2:, W // 2:, :] = 90
    g[..., :H // 3, :W // 3, :] = rng.integers(0, 256, g[..., :H // 3, :W // 3, :].shape, dtype=np.uint8)
    return g if ch == 3 else g[..., 0]


def _expected(adf, joint, src, d, sc, ss, border, dst_dtype):
    ch = 3 if joint.ndim == src.ndim + 1 else 1
    C, S, r = adf.jbfTables(d, sc, ss, ch)
    if src.ndim == 2:
        return jbf_ref.jbf(joint, src, r, C, S, border, dst_dtype)
    return np.stack([jbf_ref.jbf(joint[k], src[k], r, C, S, border, dst_dtype) for k in range(len(src))])


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def _check(adf, joint, src, d, sc=25.0, ss=3.0, border=jbf_ref.BORDER_REFLECT_101, dst_dtype=None, to_dev=None, nan_ok=False):
    """Runs the device call twice on (views of) device copies and compares with the statement."""
    import torch

    to_dev = to_dev or (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev()))
    tj, ts = to_dev(joint), to_dev(src)
    out1 = adf.jointBilateralFilter(tj, ts, d, sc, ss, border, _ddepth(adf, dst_dtype))
    out2 = adf.jointBilateralFilter(tj, ts, d, sc, ss, border, _ddepth(adf, dst_dtype))
    torch.cuda.synchronize()
    exp = _expected(adf, joint, src, d, sc, ss, border, dst_dtype)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert got1.dtype == exp.dtype
    assert _same_bits(got1, got2), "two runs differ"
    assert _same_bits(ts.cpu().numpy(), src) and np.array_equal(tj.cpu().numpy(), joint), "an input was written"
    bad = np.ascontiguousarray(got1).view(BITS[exp.dtype]) != np.ascontiguousarray(exp).view(BITS[exp.dtype])
    if nan_ok:                                                           # a NaN's payload bits are not specified
        bad &= ~(np.isnan(got1) & np.isnan(exp))
    assert not bad.any(), "%d pixels differ from the statement, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    return got1


@pytest.mark.parametrize("W", [1, TW - 1, TW, TW + 1, 2 * TW + 1])
@pytest.mark.parametrize("H", [1, TH - 1, TH, TH + 1])
def test_shapes_around_the_tile(adf, W, H):
    rng = np.random.default_rng(W * 100 + H)
    _check(adf, _joint(rng, (H, W), 1), _src(rng, (H, W), np.int16), 5)
    _check(adf, _joint(rng, (H, W), 3), _src(rng, (H, W), np.int16), 5, dst_dtype=np.float32)


@pytest.mark.parametrize("r", [1, 2, TH, 31])
@pytest.mark.parametrize("border", BORDERS)
def test_radii_and_borders(adf, r, border):
    rng = np.random.default_rng(r * 10 + border)
    H, W = 21, 45
    for ch in (1, 3):
        got = _check(adf, _joint(rng, (H, W), ch), _src(rng, (H, W), np.int16), 2 * r + 1, 30.0, 0.6 * r + 1, border, np.float32)
        assert np.isfinite(got).all()
        src = _src(rng, (3, 2), np.float32)                              # an image far smaller than the window: reflection repeats
        _check(adf, _joint(rng, (3, 2), ch), src, 2 * r + 1, 30.0, 0.6 * r + 1, border)


@pytest.mark.parametrize("src_dtype", DEPTHS)
@pytest.mark.parametrize("dst_dtype", DEPTHS)
@pytest.mark.parametrize("ch", [1, 3])
def test_source_and_output_depths(adf, src_dtype, dst_dtype, ch):
    rng = np.random.default_rng(ch * 7 + DEPTHS.index(src_dtype) * 3 + DEPTHS.index(dst_dtype))
    H, W = 19, 37
    src = _src(rng, (H, W), src_dtype)
    got = _check(adf, _joint(rng, (H, W), ch), src, 7, dst_dtype=dst_dtype)
    assert got.dtype == np.dtype(dst_dtype)
    assert not np.array_equal(got.astype(np.float64), src.astype(np.float64))              # the case is not vacuous


@pytest.mark.parametrize("sc", [3.0, 25.0, 1000.0])
@pytest.mark.parametrize("ch", [1, 3])
def test_sigma_color(adf, sc, ch):
    rng = np.random.default_rng(int(sc) + ch)
    H, W = 19, 37
    C = adf.jbfTables(7, sc, 3.0, ch)[0]
    if sc == 3.0:                                                        # the case exercises what it claims: denormal entries, a zero tail
        tiny = np.finfo(np.float32).tiny
        assert (C[40:44] > 0).all() and (C[40:44] < tiny).all() and (C[44:] == 0).all() and (C[:40] >= tiny).all()
    joint = _joint(rng, (H, W), ch)
    if sc == 3.0 and ch == 1:                                            # ... and differences of 40..43 do occur next to each other
        joint[5:9, 5:25] = np.tile(np.array([10, 50, 11, 52, 12, 54, 13, 56, 14, 57], np.uint8), 2)
    for dtype in (np.int16, np.float32):
        _check(adf, joint, _src(rng, (H, W), dtype), 7, sc, 3.0, dst_dtype=np.float32)


@pytest.mark.parametrize("ss", [0.5, 3.0, 100.0])
def test_sigma_space(adf, ss):
    rng = np.random.default_rng(int(ss * 10))
    H, W = 19, 37
    for ch in (1, 3):
        _check(adf, _joint(rng, (H, W), ch), _src(rng, (H, W), np.int16), 9, 25.0, ss, dst_dtype=np.float32)


def test_the_clamps_and_the_radius_from_sigma_space(adf):
    rng = np.random.default_rng(5)
    H, W = 19, 37
    joint, src = _joint(rng, (H, W), 3), _src(rng, (H, W), np.int16)
    zero = _check(adf, joint, src, 5, 0.0, 0.0, dst_dtype=np.float32)                       # sigma <= 0 -> 1
    assert _same_bits(zero, _check(adf, joint, src, 5, 1.0, 1.0, dst_dtype=np.float32))
    assert _same_bits(zero, _check(adf, joint, src, 5, -3.0, -0.5, dst_dtype=np.float32))
    for d in (0, -1):                                                                       # r = cvRound(1.5 sigmaSpace)
        for ss, r in ((1.0, 2), (3.0, 4), (2.0, 3)):
            assert adf.jbfTables(d, 25.0, ss, 3)[2] == r
            assert _same_bits(_check(adf, joint, src, d, 25.0, ss, dst_dtype=np.float32),
                              _check(adf, joint, src, 2 * r + 1, 25.0, ss, dst_dtype=np.float32))
    assert _same_bits(_check(adf, joint, src, 1, 25.0, 2.0), _check(adf, joint, src, 3, 25.0, 2.0))   # r raised to 1


def test_int16_extremes_and_saturating_outputs(adf):
    rng = np.random.default_rng(21)
    H, W = 17, 35
    ends = rng.choice(np.array([-32768, 32767], np.int16), (H, W))
    for ch in (1, 3):
        noisy = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
        joint = noisy if ch == 3 else noisy[..., 0]
        for sc in (2.0, 100.0):
            got = _check(adf, joint, ends, 5, sc, 2.0, dst_dtype=np.int16)
            assert got.min() < -1000 and got.max() > 1000
            got8 = _check(adf, joint, ends, 5, sc, 2.0, dst_dtype=np.uint8)                 # a weighted mean of +-32768 saturates uint8
            assert (got8 == 0).any() and (got8 == 255).any()
            _check(adf, joint, ends, 5, sc, 2.0, dst_dtype=np.float32)
    for v in (-32768, 32767):                                                               # constant maps at the ends come back
        flat = np.full((H, W), v, np.int16)
        assert np.array_equal(_check(adf, _joint(rng, (H, W), 3), flat, 11), flat)
    fr = (rng.random((H, W), np.float32) * 7 - 3).astype(np.float32)                        # float sources with fractions
    got = _check(adf, _joint(rng, (H, W), 1), fr, 7)
    assert (got != np.rint(got)).any()


def test_nan_and_inf_sources(adf):
    rng = np.random.default_rng(31)
    H, W = 19, 37
    for ch in (1, 3):
        src = _src(rng, (H, W), np.float32)
        src[4, 6], src[12, 30], src[15, 3] = np.nan, np.inf, -np.inf
        got = _check(adf, _joint(rng, (H, W), ch), src, 5, 25.0, 3.0, nan_ok=True)
        assert np.isnan(got).any() and np.isfinite(got).any() and np.isfinite(got[:, 12:25]).all()


def test_padded_and_odd_strides_and_a_batch(adf):
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
        src, joint = _src(rng, (N, H, W), dtype), _joint(rng, (N, H, W), ch)
        batch = _check(adf, joint, src, 5, dst_dtype=ddtype, to_dev=padded)
        for k in range(N):              # the batch equals three single calls
            one = adf.jointBilateralFilter(torch.from_numpy(joint[k]).to(_dev()), torch.from_numpy(src[k]).to(_dev()), 5, 25.0, 3.0,
                                           dDepth=_ddepth(adf, ddtype))
            assert _same_bits(one.cpu().numpy(), batch[k])
    # ... a destination of that kind: canaries around it stay untouched
    src, joint = _src(rng, (N, H, W), np.int16), _joint(rng, (N, H, W), 3)
    dst = padded(np.full((N, H, W), 77, np.int16))
    whole = dst._base if dst._base is not None else dst
    whole[:, H:, :] = -5
    whole[:, :, :2] = -5
    whole[:, :, 2 + W:] = -5
    out = adf.jointBilateralFilter(padded(joint), padded(src), 5, 25.0, 3.0, dst=dst)
    assert out is dst
    exp = _expected(adf, joint, src, 5, 25.0, 3.0, jbf_ref.BORDER_REFLECT_101, np.int16)
    assert np.array_equal(dst.cpu().numpy(), exp)
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[:, :H, 2:2 + W] = False
    assert (whole[outside] == -5).all(), "written outside the destination's pixels"


def test_host_entry(adf):
    import torch

    rng = np.random.default_rng(12)
    src, joint = _src(rng, (2, 11, 35), np.int16), _joint(rng, (2, 11, 35), 3)
    keep = src.copy(), joint.copy()
    out = adf.jointBilateralFilter(joint[:, :, 1:], src[:, :, 1:], 7, 25.0, 3.0, adf.BORDER_REFLECT, adf.CV_32F)   # strided host arrays
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    assert _same_bits(out, _expected(adf, joint[:, :, 1:], src[:, :, 1:], 7, 25.0, 3.0, jbf_ref.BORDER_REFLECT, np.float32))
    assert np.array_equal(src, keep[0]) and np.array_equal(joint, keep[1])
    tj, ts = torch.from_numpy(np.ascontiguousarray(joint[:, :, 1:])).to(_dev()), torch.from_numpy(np.ascontiguousarray(src[:, :, 1:])).to(_dev())
    dev = adf.jointBilateralFilter(tj, ts, 7, 25.0, 3.0, adf.BORDER_REFLECT, adf.CV_32F)
    assert _same_bits(dev.cpu().numpy(), out)                            # the device entry gives the host entry's bytes
    adf.releaseCachedMemory()                                            # the tables go too, and come back
    assert _same_bits(adf.jointBilateralFilter(tj, ts, 7, 25.0, 3.0, adf.BORDER_REFLECT, adf.CV_32F).cpu().numpy(), out)


def test_captured_into_a_graph(adf):
    import torch

    rng = np.random.default_rng(14)
    H, W = 40, 70
    src, joint = _src(rng, (H, W), np.int16), _joint(rng, (H, W), 3)
    ts, tj = torch.from_numpy(src).to(_dev()), torch.from_numpy(joint).to(_dev())
    dst = torch.zeros_like(ts)
    warm = adf.jointBilateralFilter(tj, ts, 9, 25.0, 3.0).cpu().numpy()                     # (the table is warm from here on)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        adf.jointBilateralFilter(tj, ts, 9, 25.0, 3.0, dst=dst)
    for _ in range(2):
        dst.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), warm)
    assert np.array_equal(warm, _expected(adf, joint, src, 9, 25.0, 3.0, jbf_ref.BORDER_REFLECT_101, np.int16))
