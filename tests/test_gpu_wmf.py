"""GPU tests of the weighted median filter (csrc/wmf_kernels.hip; include/adf_wls.h: adf_weighted_median_filter_*).

Integer work: every case is compared bit for bit with the direct statement tests/wmf_ref.py, with the table taken from
wmfWeightTable; every case runs twice and must give identical bytes and leave source, joint and mask unwritten.  A
workgroup's output tile is 32 x 8 (TW x TH), so the shapes are widths {1, TW-1, TW, TW+1, 2 TW+1} by heights {1, TH-1, TH,
TH+1}; every case is a few thousand pixels at the most."""
import functools

import numpy as np
import pytest

from test_oracle_bm import load_tsukuba
from wmf_ref import weighted_median

pytestmark = pytest.mark.gpu

TW, TH = 32, 8
BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}


def _dev():
    import torch

    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _table(adf, sigma, wt):
    t = adf.wmfWeightTable(sigma, wt)
    t.setflags(write=False)
    return t


def _src(rng, shape, dtype, hole=0.2):
    """A map of a few distinct values (ties), steps and noise, with holes of -16 / 0 / NaN."""
    if dtype == np.float32:
        s = rng.choice(np.array([-2.5, -0.0, 0.0, 1.25, 3.0, 1e-40, np.inf, -np.inf], np.float32), shape)
        noisy = rng.random(shape) < 0.3
        s[noisy] = rng.standard_normal(int(noisy.sum())).astype(np.float32)
        s[rng.random(shape) < hole] = np.nan
        return s
    if dtype == np.int16:
        s = rng.choice(np.array([16, 32, 48, 200, -32768, 32767], np.int16), shape)
        noisy = rng.random(shape) < 0.3
        s[noisy] = rng.integers(-300, 300, int(noisy.sum())).astype(np.int16)
        s[rng.random(shape) < hole] = -16
        return s
    s = rng.choice(np.array([0, 1, 7, 128, 255], np.uint8), shape)
    noisy = rng.random(shape) < 0.3
    s[noisy] = rng.integers(0, 256, int(noisy.sum())).astype(np.uint8)
    return s


def _joint(rng, shape, ch):
    """Smooth regions with edges: neighbouring pixels differ by little, so that weights of every size occur."""
    H, W = shape[-2:]
    base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
    j = base[..., None] + rng.integers(-6, 7, tuple(shape) + (ch,))
    j = np.clip(j, 0, 255).astype(np.uint8)
    return j if ch == 3 else j[..., 0]


def _ignore_of(dtype):
    return {np.uint8: 0, np.int16: -16, np.float32: 1.25}[dtype]


def _expected(joint, src, r, table, mask, ignore):
    if src.ndim == 2:
        return weighted_median(joint, src, r, table, mask, ignore)
    return np.stack([weighted_median(joint[k], src[k], r, table, None if mask is None else mask[k], ignore) for k in range(len(src))])


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def _check(adf, joint, src, r, sigma=25.5, wt=0, mask=None, ignore=None, to_dev=None):
    """Runs the device call twice on (views of) device copies and compares with the statement."""
    import torch

    to_dev = to_dev or (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev()))
    tj, ts, tm = to_dev(joint), to_dev(src), None if mask is None else to_dev(mask)
    out1 = adf.weightedMedianFilter(tj, ts, r, sigma, wt, tm, ignore)
    out2 = adf.weightedMedianFilter(tj, ts, r, sigma, wt, tm, ignore)
    torch.cuda.synchronize()
    exp = _expected(joint, src, r, _table(adf, sigma, wt), mask, ignore)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert _same_bits(got1, got2), "two runs differ"
    assert _same_bits(ts.cpu().numpy(), src) and np.array_equal(tj.cpu().numpy(), joint), "an input was written"
    assert mask is None or np.array_equal(tm.cpu().numpy(), mask), "the mask was written"
    bad = np.ascontiguousarray(got1).view(BITS[src.dtype]) != np.ascontiguousarray(exp).view(BITS[src.dtype])
    assert not bad.any(), "%d pixels differ from the statement, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    return got1


@pytest.mark.parametrize("W", [1, TW - 1, TW, TW + 1, 2 * TW + 1])
@pytest.mark.parametrize("H", [1, TH - 1, TH, TH + 1])
def test_shapes_around_the_tile(adf, W, H):
    rng = np.random.default_rng(W * 100 + H)
    src, joint = _src(rng, (H, W), np.int16), _joint(rng, (H, W), 1)
    mask = (rng.random((H, W)) < 0.85).astype(np.uint8)
    _check(adf, joint, src, 2, 10.0, mask=mask, ignore=-16)


@pytest.mark.parametrize("r,W,H", [(1, 45, 21), (2, 45, 21), (7, 45, 21), (31, 70, 40)])
@pytest.mark.parametrize("ch", [1, 3])
def test_radii(adf, r, W, H, ch):
    rng = np.random.default_rng(r * 10 + ch)
    _check(adf, _joint(rng, (H, W), ch), _src(rng, (H, W), np.int16), r, 10.0, ignore=-16)


@pytest.mark.parametrize("W,H", [(5, 3), (1, 1)])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_images_smaller_than_the_window(adf, W, H, dtype):
    rng = np.random.default_rng(W)
    _check(adf, _joint(rng, (H, W), 1), _src(rng, (H, W), dtype, hole=0.0), 7, 25.5)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("use", ["mask", "ignore", "both", "neither"])
def test_depths_joints_and_what_is_ignored(adf, dtype, ch, use):
    rng = np.random.default_rng(ch * 7 + len(use))
    H, W = 19, 37
    src, joint = _src(rng, (H, W), dtype), _joint(rng, (H, W), ch)
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8) if use in ("mask", "both") else None
    ignore = _ignore_of(dtype) if use in ("ignore", "both") else None
    got = _check(adf, joint, src, 3, 10.0, mask=mask, ignore=ignore)
    if use != "neither":
        assert not _same_bits(got, src)                                  # the case is not vacuous


def test_padded_and_odd_strides_and_a_batch(adf):
    import torch

    rng = np.random.default_rng(11)
    N, H, W = 3, 13, 41

    def padded(a):                      # a view into a larger tensor: W + 6 = 47 pixels per row (an odd number of bytes for uint8), a spare row per map
        big = torch.zeros((a.shape[0], a.shape[1] + 1, a.shape[2] + 6) + a.shape[3:], dtype=torch.from_numpy(a[:0]).dtype, device=_dev())
        v = big[:, :a.shape[1], 2:2 + a.shape[2]]
        v.copy_(torch.from_numpy(a))
        return v

    for dtype, ch in ((np.uint8, 3), (np.int16, 1), (np.float32, 3)):
        src, joint = _src(rng, (N, H, W), dtype), _joint(rng, (N, H, W), ch)
        mask = (rng.random((N, H, W)) < 0.8).astype(np.uint8)
        _check(adf, joint, src, 2, 10.0, mask=mask, ignore=_ignore_of(dtype), to_dev=padded)
    # ... and a destination of that kind
    src, joint = _src(rng, (N, H, W), np.int16), _joint(rng, (N, H, W), 1)
    dst = padded(np.full((N, H, W), 77, np.int16))
    whole = dst._base if dst._base is not None else dst
    out = adf.weightedMedianFilter(padded(joint), padded(src), 2, 10.0, ignoreValue=-16, dst=dst)
    assert out is dst
    assert np.array_equal(dst.cpu().numpy(), _expected(joint, src, 2, _table(adf, 10.0, 0), None, -16))
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[:, :H, 2:2 + W] = False
    assert (whole[outside] == 0).all(), "written outside the destination's pixels"


def test_host_entry(adf):
    rng = np.random.default_rng(12)
    src, joint = _src(rng, (2, 11, 35), np.int16), _joint(rng, (2, 11, 35), 3)
    mask = (rng.random((2, 11, 35)) < 0.8).astype(np.uint8)
    keep = src.copy(), joint.copy(), mask.copy()
    out = adf.weightedMedianFilter(joint[:, :, 1:], src[:, :, 1:], 3, 10.0, mask=mask[:, :, 1:], ignoreValue=-16)     # strided host arrays
    assert isinstance(out, np.ndarray)
    assert np.array_equal(out, _expected(joint[:, :, 1:], src[:, :, 1:], 3, _table(adf, 10.0, 0), mask[:, :, 1:], -16))
    assert np.array_equal(src, keep[0]) and np.array_equal(joint, keep[1]) and np.array_equal(mask, keep[2])


def test_degenerate_and_extreme_data(adf):
    rng = np.random.default_rng(13)
    H, W = 17, 35
    joint = _joint(rng, (H, W), 1)
    # an all-ignored map stays as it is
    hole = np.full((H, W), -16, np.int16)
    assert np.array_equal(_check(adf, joint, hole, 2, ignore=-16), hole)
    masked = _src(rng, (H, W), np.int16)
    assert np.array_equal(_check(adf, joint, masked, 2, mask=np.zeros((H, W), np.uint8)), masked)
    # the ends of the range
    ends = rng.choice(np.array([-32768, 32767], np.int16), (H, W))
    _check(adf, joint, ends, 2, 10.0)
    _check(adf, joint, ends, 2, 10.0, ignore=-32768)
    _check(adf, joint, ends, 2, 10.0, ignore=32767)
    u8 = rng.choice(np.array([0, 255], np.uint8), (H, W))
    _check(adf, joint, u8, 2, 10.0, ignore=255)
    # float maps: NaN, +-inf and +-0.0 (in the same window), a NaN centre among NaNs, an ignore value no float holds
    f = _src(rng, (H, W), np.float32)
    f[3:9, 4:12] = np.nan
    f[12, 20:26] = [0.0, -0.0, np.inf, -np.inf, np.nan, -0.0]
    _check(adf, joint, f, 2, 10.0)
    _check(adf, joint, f, 2, 10.0, ignore=0.0)                           # ignores -0.0 too
    _check(adf, joint, f, 2, 10.0, ignore=np.inf)
    _check(adf, joint, f, 2, 10.0, ignore=0.1)                           # no float32 equals the double 0.1
    _check(adf, joint, f, 2, 10.0, ignore=np.nan)
    _check(adf, joint, np.where(rng.random((H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)), 1, wt=adf.WMF_OFF)
    # a constant joint: every weight is 65536; WMF_OFF gives the same
    src = _src(rng, (H, W), np.int16)
    a = _check(adf, np.full((H, W), 90, np.uint8), src, 3, 10.0, ignore=-16)
    b = _check(adf, joint, src, 3, 10.0, wt=adf.WMF_OFF, ignore=-16)
    assert np.array_equal(a, b)
    # sigma = 0.5: T = 65536, 8869, 22, 0, ...: almost every weight is 0, with a noisy joint many pixels have Tot == 0 when
    # they are holes themselves
    for ch in (1, 3):
        noisy = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
        _check(adf, noisy if ch == 3 else noisy[..., 0], src, 3, 0.5, ignore=-16)
    # ties: two values only
    two = rng.choice(np.array([16, 48], np.int16), (H, W))
    _check(adf, joint, two, 3, 25.5)


def test_chain_on_tsukuba(adf, oracle):
    """StereoBM -> weightedMedianFilter(ignoreValue = -16) on the device equals the statement on the oracle matcher's map."""
    import torch

    left, right, _ = load_tsukuba()
    bm = adf.StereoBM.create(16, 7)
    bm.setTextureThreshold(0); bm.setUniquenessRatio(0)
    tl, tr = torch.from_numpy(left).to(_dev()), torch.from_numpy(right).to(_dev())
    disp = bm.compute(tl, tr)
    out = adf.weightedMedianFilter(tl, disp, 3, 25.5, ignoreValue=-16).cpu().numpy()
    raw = oracle.bm_compute(left, right, 16, 7)
    exp = weighted_median(left, raw, 3, _table(adf, 25.5, 0), ignore_value=-16)
    assert np.array_equal(out, exp)
    # holes were filled: all but those whose window holds no match at all (the band left of the first matched column)
    assert (out == -16).sum() < (raw == -16).sum()
    assert (out[:, 16 + 3 + 3:] == -16).sum() < (raw[:, 16 + 3 + 3:] == -16).sum() // 2


def test_captured_into_a_graph(adf):
    import torch

    rng = np.random.default_rng(14)
    H, W = 40, 70
    src, joint = _src(rng, (H, W), np.int16), _joint(rng, (H, W), 3)
    ts, tj = torch.from_numpy(src).to(_dev()), torch.from_numpy(joint).to(_dev())
    dst = torch.zeros_like(ts)
    warm = adf.weightedMedianFilter(tj, ts, 4, 7.25, ignoreValue=-16).cpu().numpy()        # the first call with this sigma uploads its table
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        adf.weightedMedianFilter(tj, ts, 4, 7.25, ignoreValue=-16, dst=dst)
    dst.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), warm)
    assert np.array_equal(warm, weighted_median(joint, src, 4, _table(adf, 7.25, 0), ignore_value=-16))
