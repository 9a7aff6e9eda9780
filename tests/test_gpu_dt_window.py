"""GPU tests of the domain transform filter's normalized-convolution mode (csrc/dt_window_kernels.hip; include/adf_wls.h:
adf_dt_window_filter_*).

Every case is compared bit for bit with the direct statement tests/dt_window_ref.py fed with the library's own radii
(dtNcRadii), float outputs as uint32; every case runs twice and must give identical bytes and leave guide and source
unwritten.  The row pass moves a row in tiles of 1024 columns, the column pass 32 columns in tiles of 64 rows, so the shapes
straddle 1024 and 32 in W and 64 in H; every case is a few ten thousand pixels at the most."""
import ctypes as C

import numpy as np
import pytest

from dt_window_ref import dt_window_filter

pytestmark = pytest.mark.gpu

BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}
DEPTHS = [np.uint8, np.int16, np.float32]
DEPTH_CODE = {np.uint8: 0, np.int16: 3, np.float32: 5}
SMALL, LARGE = (10.0, 30.0, 3), (80.0, 50.0, 3)    # R = 15, 7, 3: the halo is smaller than a tile; R = 120, 60, 30: larger
TIE = 4.618802070617676                            # float32(8 / sqrt(3)): r_1 = 8.0 at one iteration


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


def _guide(rng, shape, ch, kind="random"):
    """random: smooth regions with edges, a little noise and a flat patch; steps: two levels; flat: one."""
    H, W = shape[-2:]
    full = tuple(shape) + (ch,)
    if kind == "flat":
        g = np.full(full, 117, np.uint8)
    elif kind == "steps":
        g = np.where((np.add.outer(np.arange(H) // 7, np.arange(W) // 9) % 2)[..., None] > 0, 200, 20) * np.ones(full, np.int64)
        g = g.astype(np.uint8)
    else:
        base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
        g = np.clip(base[..., None] + rng.integers(-6, 7, full), 0, 255).astype(np.uint8)
        g[..., H // 2:, W // 2:, :] = 90
    return g if ch == 3 else g[..., 0]


def _expected(adf, guide, src, ss, sr, N, dst_dtype):
    radii = adf.dtNcRadii(ss, N)
    if src.ndim == 2:
        return dt_window_filter(guide, src, ss, sr, radii, dst_dtype)
    return np.stack([dt_window_filter(guide[k], src[k], ss, sr, radii, dst_dtype) for k in range(len(src))])


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def _check(adf, guide, src, ss=10.0, sr=30.0, N=3, dst_dtype=None, to_dev=None):
    """Runs the device call twice on (views of) device copies and compares with the statement."""
    import torch

    to_dev = to_dev or (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev()))
    tg, ts = to_dev(guide), to_dev(src)
    out1 = adf.dtWindowFilter(tg, ts, ss, sr, adf.DTF_NC, N, _ddepth(adf, dst_dtype))
    out2 = adf.dtWindowFilter(tg, ts, ss, sr, adf.DTF_NC, N, _ddepth(adf, dst_dtype))
    torch.cuda.synchronize()
    exp = _expected(adf, guide, src, ss, sr, N, dst_dtype)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert got1.dtype == exp.dtype
    assert _same_bits(got1, got2), "two runs differ"
    assert _same_bits(ts.cpu().numpy(), src) and np.array_equal(tg.cpu().numpy(), guide), "an input was written"
    bad = np.ascontiguousarray(got1).view(BITS[exp.dtype]) != np.ascontiguousarray(exp).view(BITS[exp.dtype])
    assert not bad.any(), "%d pixels differ from the statement, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    return got1


# a sampled cross of H in {1, 2, 63, 64, 65, 129} (the column pass's 64 rows) against W in {1, 2, 31, 32, 33, 1023, 1024, 1025}
# (its 32 columns, the row pass's 1024; the widest shapes are the flattest)
SHAPES = [(1, 1), (1, 1025), (129, 1), (64, 32), (2, 1024), (65, 33), (33, 1025), (129, 32), (2, 2), (1, 2), (2, 1), (63, 31),
          (1, 1023), (63, 33), (65, 31), (33, 1023), (129, 33), (2, 32), (64, 2), (33, 1024), (129, 31), (1, 32), (1, 1024), (65, 1),
          (2, 1025), (129, 2), (65, 300)]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("regime", [SMALL, LARGE])
def test_shapes_around_the_tiles(adf, H, W, regime):
    ss, sr, N = regime
    rng = np.random.default_rng(W * 1000 + H)
    _check(adf, _guide(rng, (H, W), 1), _src(rng, (H, W), np.int16), ss, sr, N)
    _check(adf, _guide(rng, (H, W), 3), _src(rng, (H, W), np.int16), ss, sr, N, dst_dtype=np.float32)


def test_identity_passes_still_carry_and_convert_the_map(adf):
    rng = np.random.default_rng(5)
    H, W = 66, 70
    assert [int(r) for r in adf.dtNcRadii(1.0, 3)] == [1, 0, 0]          # r = 1.51, 0.76, 0.38
    for ch, sdt, ddt in ((1, np.int16, np.float32), (3, np.float32, np.int16), (1, np.uint8, np.uint8)):
        src = _src(rng, (H, W), sdt)
        got = _check(adf, _guide(rng, (H, W), ch), src, 1.0, 30.0, 3, ddt)
        assert not np.array_equal(got.astype(np.float64), src.astype(np.float64))   # the first iteration did filter
    # ... and what the two identity iterations carry is the first iteration's result, bit for bit
    guide, src = _guide(rng, (H, W), 1), _src(rng, (H, W), np.float32)
    three = _check(adf, guide, src, 1.0, 30.0, 3)
    first = dt_window_filter(guide, src, 1.0, 30.0, adf.dtNcRadii(1.0, 3)[:1])
    assert _same_bits(three, first)


def test_the_tie_at_the_ends_of_a_window(adf):
    assert adf.dtNcRadii(TIE, 1)[0] == 8.0
    rng = np.random.default_rng(6)
    H, W = 40, 300
    flat = _guide(rng, (H, W), 1, "flat")
    x = np.arange(W, dtype=np.float32)[None].repeat(H, 0)
    got = _check(adf, flat, x, TIE, TIE, 1, np.float32)
    # rows: the window of an interior pixel is [j - 8, j + 7], 16 taps, whose mean is j - 0.5; the columns are constant (every
    # partial sum is exact)
    assert np.array_equal(got[H // 2, 8:W - 8], np.arange(8, W - 8, dtype=np.float32) - np.float32(0.5))
    _check(adf, flat, _src(rng, (H, W), np.int16), TIE, TIE, 1)
    _check(adf, _guide(rng, (H, W), 3, "flat"), _src(rng, (H, W), np.float32), TIE, TIE, 1)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("kind", ["random", "steps", "flat"])
def test_a_larger_map_and_the_kinds_of_guide(adf, ch, kind):
    rng = np.random.default_rng(ch + len(kind))
    H, W = 200, 300
    src = _src(rng, (H, W), np.int16)
    got = _check(adf, _guide(rng, (H, W), ch, kind), src, 12.0, 25.0, 3, np.float32)
    assert not np.array_equal(got, src.astype(np.float32))                                  # the case is not vacuous
    if kind == "steps":                                                                     # and the edges hold
        _check(adf, _guide(rng, (H, W), ch, kind), src, 40.0, 10.0, 3)


@pytest.mark.parametrize("src_dtype", DEPTHS)
@pytest.mark.parametrize("dst_dtype", DEPTHS)
@pytest.mark.parametrize("ch", [1, 3])
def test_source_and_output_depths(adf, src_dtype, dst_dtype, ch):
    rng = np.random.default_rng(ch * 7 + DEPTHS.index(src_dtype) * 3 + DEPTHS.index(dst_dtype))
    H, W = 19, 70
    src = _src(rng, (H, W), src_dtype)
    got = _check(adf, _guide(rng, (H, W), ch), src, 10.0, 30.0, 2, dst_dtype)
    assert got.dtype == np.dtype(dst_dtype)
    assert not np.array_equal(got.astype(np.float64), src.astype(np.float64))


@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("ch", [1, 3])
def test_iterations(adf, N, ch):
    rng = np.random.default_rng(N * 10 + ch)
    H, W = 66, 70
    _check(adf, _guide(rng, (H, W), ch), _src(rng, (H, W), np.int16), 20.0, 40.0, N)
    _check(adf, _guide(rng, (H, W), ch), _src(rng, (H, W), np.float32), 20.0, 40.0, N)
    if N == 1:                                                                              # numIters below 1 is one iteration
        src, guide = _src(rng, (H, W), np.int16), _guide(rng, (H, W), ch)
        assert np.array_equal(_check(adf, guide, src, 20.0, 40.0, 0), _check(adf, guide, src, 20.0, 40.0, 1))


@pytest.mark.parametrize("ss,sr", [(0.5, 30.0), (10.0, 0.0), (0.5, 0.0), (84.0, 0.01), (3.0, 255.0)])
def test_sigmas_at_the_clamps(adf, ss, sr):
    rng = np.random.default_rng(int(ss * 10 + sr))
    H, W = 33, 67
    for ch in (1, 3):
        guide, src = _guide(rng, (H, W), ch), _src(rng, (H, W), np.int16)
        got = _check(adf, guide, src, ss, sr, 3, np.float32)
        clamped = _check(adf, guide, src, max(ss, 1.0), max(sr, 0.01), 3, np.float32)
        assert _same_bits(got, clamped)


def test_int16_extremes_large_floats_and_constant_maps(adf):
    rng = np.random.default_rng(21)
    H, W = 65, 67
    ends = rng.choice(np.array([-32768, 32767], np.int16), (H, W))
    for ch in (1, 3):
        guide = _guide(rng, (H, W), ch)
        got = _check(adf, guide, ends, 10.0, 30.0, 3, np.int16)
        assert got.min() >= -32768 and got.max() <= 32767 and len(np.unique(got)) > 2
        got8 = _check(adf, guide, ends, 10.0, 30.0, 3, np.uint8)                            # saturates at both ends
        assert (got8 == 0).any() and (got8 == 255).any()
        big = (rng.random((H, W)) * 2e6 - 1e6).astype(np.float32)
        big[0, 0], big[-1, -1] = 1e6, -1e6
        _check(adf, guide, big, 10.0, 30.0, 3)
        _check(adf, guide, big, 10.0, 30.0, 3, np.int16)
        # an integer-valued constant map comes back exactly, whatever the guide and the radius
        for v, dtype in ((-32768, np.int16), (32767, np.int16), (255, np.uint8), (123456.0, np.float32)):
            flat = np.full((H, W), v, dtype)
            assert np.array_equal(_check(adf, guide, flat, 25.0, 12.0, 8), flat)
            assert np.array_equal(_check(adf, guide, flat, 80.0, 50.0, 3), flat)


def test_padded_strides_a_batch_and_a_workspace(adf):
    import torch

    rng = np.random.default_rng(11)
    N, H, W = 3, 66, 71

    def padded(a):                      # a view into a larger tensor: W + 6 pixels per row, a spare row per map
        hw = a.shape[1:3]
        big = torch.zeros((a.shape[0], hw[0] + 1, hw[1] + 6) + a.shape[3:], dtype=torch.from_numpy(a[:0]).dtype, device=_dev())
        v = big[:, :hw[0], 2:2 + hw[1]]
        v.copy_(torch.from_numpy(a))
        return v

    for dtype, ch, ddtype in ((np.uint8, 3, np.int16), (np.int16, 1, np.float32), (np.float32, 3, np.uint8)):
        src, guide = _src(rng, (N, H, W), dtype), _guide(rng, (N, H, W), ch)
        batch = _check(adf, guide, src, 10.0, 30.0, 2, ddtype, to_dev=padded)
        for k in range(N):                                                                  # the batch equals three single calls
            one = adf.dtWindowFilter(torch.from_numpy(guide[k]).to(_dev()), torch.from_numpy(src[k]).to(_dev()), 10.0, 30.0,
                                     adf.DTF_NC, 2, _ddepth(adf, ddtype))
            assert _same_bits(one.cpu().numpy(), batch[k])
    # ... a destination of that kind, and a caller workspace instead of library scratch
    src, guide = _src(rng, (N, H, W), np.int16), _guide(rng, (N, H, W), 3)
    dst = padded(np.full((N, H, W), 77, np.int16))
    whole = dst._base if dst._base is not None else dst
    ws = torch.empty(adf.dtWindowFilterWorkspaceBytes(N, H, W), dtype=torch.uint8, device=_dev())
    out = adf.dtWindowFilter(padded(guide), padded(src), 10.0, 30.0, dst=dst, workspace=ws)
    assert out is dst
    exp = _expected(adf, guide, src, 10.0, 30.0, 3, np.int16)
    assert np.array_equal(dst.cpu().numpy(), exp)
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[:, :H, 2:2 + W] = False
    assert (whole[outside] == 0).all(), "written outside the destination's pixels"
    scratch = adf.dtWindowFilter(torch.from_numpy(guide).to(_dev()), torch.from_numpy(src).to(_dev()), 10.0, 30.0)
    assert np.array_equal(scratch.cpu().numpy(), exp)
    with pytest.raises(adf.AdfError) as e:                               # a workspace one byte short
        adf.dtWindowFilter(padded(guide), padded(src), 10.0, 30.0, dst=dst, workspace=ws[:-1])
    assert e.value.code == 2


def test_the_c_abi_on_a_non_default_stream(adf):
    import torch
    from addingdisparityfiltering_amd import _lib

    rng = np.random.default_rng(13)
    L = _lib.lib()
    H, W = 65, 130
    for ch, sdt, ddt in ((1, np.int16, np.int16), (3, np.float32, np.int16), (3, np.uint8, np.float32)):
        guide, src = _guide(rng, (H, W), ch), _src(rng, (H, W), sdt)
        tg, ts = torch.from_numpy(guide).to(_dev()), torch.from_numpy(src).to(_dev())
        dst = torch.zeros((H, W), dtype=torch.from_numpy(np.zeros(0, ddt)).dtype, device=_dev())
        ws = torch.empty(L.adf_dt_window_filter_workspace_bytes(1, W, H), dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        rc = L.adf_dt_window_filter_device(1, tg.data_ptr(), W * ch, 0, ch, ts.data_ptr(), W * src.itemsize, 0, DEPTH_CODE[sdt],
                                           dst.data_ptr(), W * np.dtype(ddt).itemsize, 0, DEPTH_CODE[ddt], W, H, 10.0, 30.0, 0, 3,
                                           ws.data_ptr(), ws.numel(), C.c_void_p(st.cuda_stream))
        assert rc == 0, L.adf_last_error()
        st.synchronize()
        assert _same_bits(dst.cpu().numpy(), _expected(adf, guide, src, 10.0, 30.0, 3, ddt))
        with torch.cuda.stream(st):                                      # the mirror on torch's current stream
            out = adf.dtWindowFilter(tg, ts, 10.0, 30.0, dDepth=_ddepth(adf, ddt))
        st.synchronize()
        assert _same_bits(out.cpu().numpy(), dst.cpu().numpy())


def test_host_entry_and_the_filter_object(adf):
    import torch

    rng = np.random.default_rng(12)
    src, guide = _src(rng, (2, 11, 70), np.int16), _guide(rng, (2, 11, 70), 3)
    keep = src.copy(), guide.copy()
    out = adf.dtWindowFilter(guide[:, :, 1:], src[:, :, 1:], 10.0, 30.0, dDepth=adf.CV_32F)   # strided host arrays
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    exp = _expected(adf, guide[:, :, 1:], src[:, :, 1:], 10.0, 30.0, 3, np.float32)
    assert _same_bits(out, exp)
    assert np.array_equal(src, keep[0]) and np.array_equal(guide, keep[1])
    tg, ts = torch.from_numpy(np.ascontiguousarray(guide[:, :, 1:])).to(_dev()), torch.from_numpy(np.ascontiguousarray(src[:, :, 1:])).to(_dev())
    f = adf.createDTWindowFilter(tg, 10.0, 30.0)                                            # the defaults: DTF_NC, 3 iterations
    assert isinstance(f, adf.DTWindowFilter)
    assert _same_bits(f.filter(ts, dDepth=adf.CV_32F).cpu().numpy(), out)
    assert _same_bits(f.filter(ts).cpu().numpy(), _expected(adf, guide[:, :, 1:], src[:, :, 1:], 10.0, 30.0, 3, None))
    host = adf.createDTWindowFilter(guide[0], 5.0, 20.0, adf.DTF_NC, 2).filter(src[0])
    assert _same_bits(host, dt_window_filter(guide[0], src[0], 5.0, 20.0, adf.dtNcRadii(5.0, 2)))


def test_captured_into_a_graph(adf):
    import torch

    rng = np.random.default_rng(14)
    H, W = 70, 130
    src, guide = _src(rng, (H, W), np.int16), _guide(rng, (H, W), 3)
    ts, tg = torch.from_numpy(src).to(_dev()), torch.from_numpy(guide).to(_dev())
    dst = torch.zeros_like(ts)
    ws = torch.empty(adf.dtWindowFilterWorkspaceBytes(1, H, W), dtype=torch.uint8, device=_dev())
    warm = adf.dtWindowFilter(tg, ts, 10.0, 30.0).cpu().numpy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one chain of launches: no parallel branches
        adf.dtWindowFilter(tg, ts, 10.0, 30.0, dst=dst, workspace=ws)
    dst.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), warm)
    assert np.array_equal(warm, _expected(adf, guide, src, 10.0, 30.0, 3, np.int16))
