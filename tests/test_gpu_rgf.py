"""GPU tests of the rolling guidance filter (csrc/rolling_guidance_kernels.hip; include/adf_wls.h:
adf_rolling_guidance_filter_*).

Every case is compared bit for bit with the direct statement tests/rgf_ref.py fed with the library's own tables (float
outputs as uint32, NaNs matched by position); every case runs twice and must give identical bytes and leave the source
unwritten.  A workgroup's output tile is 32 x 8 (TW x TH in the kernel file), so the shapes are widths {1, TW-1, TW,
TW+1, 2 TW+1} by heights {1, TH-1, TH, TH+1}; the radii {1, 2, TH, 31} take the halo past the tile and past the image;
every case is a few thousand pixels at the most."""
import numpy as np
import pytest

import rgf_ref

pytestmark = pytest.mark.gpu

TW, TH = 32, 8
LDS_ENTRIES = 1024               # of an integer range table: what the kernel keeps in LDS (the rest is read from the device table)
BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}
DEPTHS = [np.uint8, np.int16, np.float32]
BORDERS = [rgf_ref.BORDER_REPLICATE, rgf_ref.BORDER_REFLECT, rgf_ref.BORDER_REFLECT_101]


def _dev():
    import torch

    return torch.device("cuda:0")


def _src(rng, shape, dtype):
    """A disparity-like map: plateaus with edges, a ramp, noise on a third of the pixels; float maps carry fractions."""
    H, W = shape[-2:]
    base = np.add.outer(np.arange(H) // 4 * 37, np.arange(W) // 6 * 53) % 7
    noisy = rng.random(shape) < 0.3
    if dtype == np.float32:
        s = (np.array([-2.5, 0.0, 16.25, 48.0, 200.125, 90.5, 33.0], np.float32)[base] + np.zeros(shape, np.float32)).astype(np.float32)
        s[noisy] += (rng.standard_normal(int(noisy.sum())) * 20).astype(np.float32)
        return s
    if dtype == np.int16:
        s = (np.array([16, 480, 2000, -16, 520, 1000, 60])[base] + np.zeros(shape, np.int64))
        s[noisy] += rng.integers(-40, 41, int(noisy.sum()))
        return s.astype(np.int16)
    s = (np.array([0, 1, 70, 128, 255, 140, 30])[base] + np.zeros(shape, np.int64))
    s[noisy] += rng.integers(-30, 31, int(noisy.sum()))
    return np.clip(s, 0, 255).astype(np.uint8)


def _expected(adf, src, d, sc, ss, n, border):
    colour, space, r, scale = adf.rgfTables(src.dtype, d, sc, ss)
    return rgf_ref.rgf(src, r, colour, space, scale, n, border)


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def _check(adf, src, d=-1, sc=25.0, ss=3.0, n=4, border=rgf_ref.BORDER_REFLECT_101, to_dev=None, nan_ok=False):
    """Runs the device call twice on (a view of) a device copy and compares with the statement."""
    import torch

    to_dev = to_dev or (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev()))
    ts = to_dev(src)
    out1 = adf.rollingGuidanceFilter(ts, d, sc, ss, n, border)
    out2 = adf.rollingGuidanceFilter(ts, d, sc, ss, n, border)
    torch.cuda.synchronize()
    exp = _expected(adf, src, d, sc, ss, n, border)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert got1.dtype == exp.dtype == src.dtype
    assert _same_bits(got1, got2), "two runs differ"
    assert _same_bits(ts.cpu().numpy(), src), "the source was written"
    bad = np.ascontiguousarray(got1).view(BITS[exp.dtype]) != np.ascontiguousarray(exp).view(BITS[exp.dtype])
    if nan_ok:                                                           # a NaN's payload bits are not specified
        bad &= ~(np.isnan(got1) & np.isnan(exp))
    assert not bad.any(), "%d pixels differ from the statement, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    return got1


@pytest.mark.parametrize("W", [1, TW - 1, TW, TW + 1, 2 * TW + 1])
@pytest.mark.parametrize("H", [1, TH - 1, TH, TH + 1])
def test_shapes_around_the_tile(adf, W, H):
    rng = np.random.default_rng(W * 100 + H)
    _check(adf, _src(rng, (H, W), np.int16), 5, n=2)                     # r = 2


@pytest.mark.parametrize("r", [1, 2, TH, 31])
@pytest.mark.parametrize("border", BORDERS)
def test_radii_and_borders(adf, r, border):
    rng = np.random.default_rng(r * 10 + border)
    got = _check(adf, _src(rng, (29, 37), np.int16), 2 * r + 1, 30.0, 0.6 * r + 1, 2, border)
    assert got.min() >= -60 and got.max() <= 2040
    for dtype in (np.int16, np.float32):                                 # an image far smaller than the window: reflection repeats
        _check(adf, _src(rng, (2, 3), dtype), 2 * r + 1, 30.0, 0.6 * r + 1, 2, border)


@pytest.mark.parametrize("dtype", DEPTHS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_depths_and_iterations(adf, dtype, n):
    """Both parities of the buffer alternation end in dst; 0 is a copy."""
    rng = np.random.default_rng(n * 3 + DEPTHS.index(dtype))
    src = _src(rng, (19, 37), dtype)
    got = _check(adf, src, 7, 25.0, 2.0, n)
    assert _same_bits(got, src) == (n == 0)                              # the case is not vacuous
    if n == 4:                                                           # the defaults are the reference's
        import torch

        assert _same_bits(adf.rollingGuidanceFilter(torch.from_numpy(src).to(_dev())).cpu().numpy(), _expected(adf, src, -1, 25, 3, 4, 4))


@pytest.mark.parametrize("sc", [1.0, 25.0, 1000.0, 5000.0])
def test_int16_whole_range_and_table_lengths(adf, sc):
    """Differences over 0 .. 65535: the table cut short (T = 16, 362: all of it in LDS), partly outside LDS (T = 14422) and
    at full length (65536)."""
    rng = np.random.default_rng(int(sc))
    H, W = 17, 45
    T = len(adf.rgfTables(np.int16, 5, sc, 2.0)[0])
    assert T == {1.0: 16, 25.0: 362, 1000.0: 14422, 5000.0: 65536}[sc] and (T > LDS_ENTRIES) == (sc >= 1000.0)
    src = rng.integers(-32768, 32768, (H, W)).astype(np.int16)
    src[:, :12] = (rng.integers(-3, 4, (H, 12)) * max(1, T // 8) + 100).astype(np.int16)     # differences on both sides of T - 1 ...
    src[:, 12:24] = rng.integers(LDS_ENTRIES - 40, LDS_ENTRIES + 41, (H, 12)) * rng.choice([0, 1], (H, 12))   # ... and of LDS_ENTRIES
    src[3, 30:34] = (-32768, 32767, -32768, 32767)                       # L = 65535
    L = np.abs(src[:, 1:].astype(np.int64) - src[:, :-1])
    assert (L >= T - 1).any() and (L < T - 1).any() and (L == 65535).any()
    if T > LDS_ENTRIES:
        assert ((L >= LDS_ENTRIES) & (L < T - 1)).any() and (L < LDS_ENTRIES).any()
    for n in (1, 3):
        got = _check(adf, src, 5, sc, 2.0, n)
    assert not _same_bits(got, src)
    for v in (-32768, 32767):                                            # constant maps at the ends come back
        flat = np.full((H, W), v, np.int16)
        assert np.array_equal(_check(adf, flat, 5, sc, 2.0, 3), flat)


@pytest.mark.parametrize("sc", [3.0, 25.0])
def test_uint8_equals_successive_joint_bilateral_calls(adf, sc):
    import torch

    rng = np.random.default_rng(int(sc))
    src = _src(rng, (21, 45), np.uint8)
    src[2:9, 3:20] = rng.integers(0, 256, (7, 17), dtype=np.uint8)
    ts = torch.from_numpy(src).to(_dev())
    for border in (rgf_ref.BORDER_REFLECT_101, rgf_ref.BORDER_REPLICATE):
        joint = ts.clone()                                                   # (jointBilateralFilter refuses joint is src)
        for n in range(1, 5):
            joint = adf.jointBilateralFilter(joint, ts, 7, sc, 2.0, border, adf.CV_8U)      # joint = the previous result
            got = _check(adf, src, 7, sc, 2.0, n, border)
            assert np.array_equal(got, joint.cpu().numpy()), "differs from %d jointBilateralFilter calls" % n


def test_float_nan_inf_and_sixteen_sigma(adf):
    rng = np.random.default_rng(31)
    H, W = 19, 37
    src = _src(rng, (H, W), np.float32)
    src[4, 6], src[12, 30], src[15, 3] = np.nan, np.inf, -np.inf
    got = _check(adf, src, 5, 25.0, 3.0, 2, nan_ok=True)
    assert np.isnan(got).any() and np.isfinite(got).any() and np.isfinite(got[:, 12:25]).all()
    # differences that straddle 16 sigma: just inside (a denormal-sized weight), on it and beyond it (exactly 0)
    sigma = 2.0
    steps = np.array([0.0, 31.9, 32.0, 32.1, 14.4 * sigma, 14.43 * sigma, 1e6, 1e30], np.float32)
    src = (steps[rng.integers(0, len(steps), (H, W))] * rng.choice([1.0, -1.0], (H, W))).astype(np.float32)
    src[:, ::5] += rng.random((H, len(range(0, W, 5)))).astype(np.float32)
    G, _, _, scale = adf.rgfTables(np.float32, 5, sigma, 3.0)
    a = np.abs(src[:, 1:] - src[:, :-1]) * scale
    assert (a > 4096).any() and ((a > 3600) & (a < 3692)).any() and ((a >= 3692) & (a < 4096)).any() and (a < 256).any()
    got = _check(adf, src, 5, sigma, 3.0, 3, nan_ok=True)
    assert np.isfinite(got).all()
    for sc in (0.01, 1e4):
        _check(adf, _src(rng, (H, W), np.float32), 5, sc, 3.0, 2)
    flat = np.full((H, W), -4.0, np.float32)                             # (a power of two: every product is exact)
    assert _same_bits(_check(adf, flat, 7, 25.0, 3.0, 3), flat)


def test_padded_and_odd_strides_and_a_batch(adf):
    import torch

    rng = np.random.default_rng(11)
    N, H, W = 3, 13, 41

    def padded(a):                      # a view into a larger tensor: W + 5 pixels per row (an odd pitch), a spare row per map
        big = torch.zeros((a.shape[0], H + 1, W + 5), dtype=torch.from_numpy(a[:0]).dtype, device=_dev())
        v = big[:, :H, 2:2 + W]
        v.copy_(torch.from_numpy(a))
        return v

    for dtype in DEPTHS:
        src = _src(rng, (N, H, W), dtype)
        for n in (3, 4):
            batch = _check(adf, src, 5, n=n, to_dev=padded)
            for k in range(N):              # the batch equals three single calls
                one = adf.rollingGuidanceFilter(torch.from_numpy(src[k]).to(_dev()), 5, numOfIter=n)
                assert _same_bits(one.cpu().numpy(), batch[k])
    # ... a destination of that kind: canaries around it stay untouched, with library scratch and with a caller's workspace
    src = _src(rng, (N, H, W), np.int16)
    exp = _expected(adf, src, 5, 25.0, 3.0, 4, rgf_ref.BORDER_REFLECT_101)
    need = adf.rollingGuidanceWorkspaceBytes(N, H, W, np.int16, 4)
    assert need == N * H * W * 2
    for ws in (None, torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=_dev())):
        dst = padded(np.full((N, H, W), 77, np.int16))
        whole = dst._base if dst._base is not None else dst
        whole[:, H:, :] = -5
        whole[:, :, :2] = -5
        whole[:, :, 2 + W:] = -5
        out = adf.rollingGuidanceFilter(padded(src), 5, dst=dst, workspace=ws)
        assert out is dst
        assert np.array_equal(dst.cpu().numpy(), exp)
        outside = torch.ones_like(whole, dtype=torch.bool)
        outside[:, :H, 2:2 + W] = False
        assert (whole[outside] == -5).all(), "written outside the destination's pixels"
        if ws is not None:
            assert (ws[need:] == 0x5A).all(), "written past the workspace's stated size"
    with pytest.raises(adf.AdfError) as e:                                # too small a workspace
        adf.rollingGuidanceFilter(padded(src), 5, workspace=torch.zeros(need - 1, dtype=torch.uint8, device=_dev()))
    assert e.value.code == 2


def test_host_entry(adf):
    import torch

    rng = np.random.default_rng(12)
    for dtype in DEPTHS:
        src = _src(rng, (2, 11, 35), dtype)
        keep = src.copy()
        for n in (0, 1, 4):
            out = adf.rollingGuidanceFilter(src[:, :, 1:], 7, 25.0, 3.0, n, adf.BORDER_REFLECT)   # strided host arrays
            assert isinstance(out, np.ndarray) and out.dtype == src.dtype
            assert _same_bits(out, _expected(adf, src[:, :, 1:], 7, 25.0, 3.0, n, rgf_ref.BORDER_REFLECT))
            assert _same_bits(src, keep)
        ts = torch.from_numpy(np.ascontiguousarray(src[:, :, 1:])).to(_dev())
        dev = adf.rollingGuidanceFilter(ts, 7, 25.0, 3.0, 4, adf.BORDER_REFLECT)
        assert _same_bits(dev.cpu().numpy(), out)                        # the device entry gives the host entry's bytes
        adf.releaseCachedMemory()                                        # the tables go too, and come back
        assert _same_bits(adf.rollingGuidanceFilter(ts, 7, 25.0, 3.0, 4, adf.BORDER_REFLECT).cpu().numpy(), out)


@pytest.mark.parametrize("dtype,n", [(np.int16, 4), (np.float32, 3)])
def test_captured_into_a_graph(adf, dtype, n):
    import torch

    rng = np.random.default_rng(14)
    H, W = 40, 70
    src = _src(rng, (H, W), dtype)
    ts = torch.from_numpy(src).to(_dev())
    dst = torch.zeros_like(ts)
    ws = torch.zeros(adf.rollingGuidanceWorkspaceBytes(1, H, W, dtype, n), dtype=torch.uint8, device=_dev())
    warm = adf.rollingGuidanceFilter(ts, 9, 25.0, 3.0, n).cpu().numpy()                      # (the tables are warm from here on)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        adf.rollingGuidanceFilter(ts, 9, 25.0, 3.0, n, dst=dst, workspace=ws)
    for _ in range(2):
        dst.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same_bits(dst.cpu().numpy(), warm)
    assert _same_bits(warm, _expected(adf, src, 9, 25.0, 3.0, n, rgf_ref.BORDER_REFLECT_101))
