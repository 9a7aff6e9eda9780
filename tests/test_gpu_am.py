"""GPU tests of the adaptive manifold filter (csrc/am_filter_kernels.hip; include/adf_wls.h: adf_am_filter_*).

Every case is compared bit for bit with the direct statement tests/am_ref.py fed with the library's own plan (amPlan),
float outputs as uint32; every case runs twice and must give identical bytes and leave joint and source unwritten.  A row
sweep workgroup owns 16 rows and walks tiles of 64 columns, a column sweep workgroup owns 64 columns and loads 8 rows at a
time, at full size (the root manifold) and at small size, so the shapes straddle 64 in W, 16 and 64 in H at df = 1 and
twice that at df = 2;
every case is a few ten thousand pixels at the most."""
import ctypes as C

import numpy as np
import pytest

import am_ref

pytestmark = pytest.mark.gpu

BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}
DEPTHS = [np.uint8, np.int16, np.float32]
DEPTH_CODE = {np.uint8: 0, np.int16: 3, np.float32: 5}


def _dev():
    import torch

    return torch.device("cuda:0")


def _ddepth(adf, dtype):
    return {None: -1, np.uint8: adf.CV_8U, np.int16: adf.CV_16S, np.float32: adf.CV_32F}[dtype]


def _src(rng, shape, dtype):
    """Steps, noise and the ends of the range next to each other; float maps carry fractions and large values."""
    if dtype == np.float32:
        s = rng.choice(np.array([-2.5, 0.0, 16.25, 480.0, 2000.125, 3.0e6], np.float32), shape)
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


def _joint(rng, shape, ch, kind="random"):
    """random: smooth regions with edges, a little noise and a flat patch; flat: one level; blocks: two levels in blocks of
    7 x 9 with four isolated pixels."""
    H, W = shape[-2:]
    full = tuple(shape) + (ch,)
    if kind == "flat":
        g = np.full(full, 117, np.uint8)
    elif kind == "blocks":
        g = np.where((np.add.outer(np.arange(H) // 7, np.arange(W) // 9) % 2)[..., None] > 0, 200, 20) * np.ones(full, np.int64)
        g = g.astype(np.uint8)
        for (y, x), v in zip(((3, 4), (H // 2, W // 2), (H - 4, 5), (10, W - 3)), (255, 0, 110, 255)):
            g[..., y, x, :] = v
    else:
        base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
        g = np.clip(base[..., None] + rng.integers(-6, 7, full) + np.arange(ch) * 40, 0, 255).astype(np.uint8)
        g[..., H // 2:, W // 2:, :] = 90
    return g if ch == 3 else g[..., 0]


def _expected(adf, joint, src, ss, sr, adjust, dst_dtype, height=-1):
    H, W = src.shape[-2:]
    p = adf.amPlan(ss, sr, height, W, H)
    if src.ndim == 2:
        return am_ref.am_filter(joint, src, p, p["jtab"], adjust, dst_dtype)
    return np.stack([am_ref.am_filter(joint[k], src[k], p, p["jtab"], adjust, dst_dtype) for k in range(len(src))])


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def _run(adf, tj, ts, ss, sr, adjust, dst_dtype, height):
    if height == -1:
        return adf.amFilter(tj, ts, ss, sr, adjust, dDepth=_ddepth(adf, dst_dtype))
    f = adf.createAMFilter(ss, sr, adjust)
    f.setTreeHeight(height)
    return f.filter(ts, joint=tj, dDepth=_ddepth(adf, dst_dtype))


def _check(adf, joint, src, ss=16.0, sr=0.2, adjust=False, dst_dtype=None, height=-1, to_dev=None):
    """Runs the device call twice on (views of) device copies and compares with the statement."""
    import torch

    to_dev = to_dev or (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev()))
    tj, ts = to_dev(joint), to_dev(src)
    out1 = _run(adf, tj, ts, ss, sr, adjust, dst_dtype, height)
    out2 = _run(adf, tj, ts, ss, sr, adjust, dst_dtype, height)
    torch.cuda.synchronize()
    exp = _expected(adf, joint, src, ss, sr, adjust, dst_dtype, height)
    got1, got2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert got1.dtype == exp.dtype
    assert _same_bits(got1, got2), "two runs differ"
    assert _same_bits(ts.cpu().numpy(), src) and np.array_equal(tj.cpu().numpy(), joint), "an input was written"
    bad = np.ascontiguousarray(got1).view(BITS[exp.dtype]) != np.ascontiguousarray(exp).view(BITS[exp.dtype])
    assert not bad.any(), "%d pixels differ from the statement, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    return got1


# (H, W, sigma_s, sigma_r): the small plane of 10 x 6 is 2 x 2 and holds the clamped last tap; of 3 x 3, 1 x 1 (no sweep has a
# step); 1 x 40 and 40 x 1 at df = 1; then around the sweeps' 64 at full size (df = 1) and at small size (df = 2)
SHAPES = [(10, 6, 16.0, 0.2), (6, 10, 16.0, 0.2), (3, 3, 16.0, 0.2), (1, 40, 5.0, 0.2), (40, 1, 5.0, 0.2), (22, 14, 16.0, 0.2), (14, 22, 16.0, 0.2),
          (63, 65, 5.0, 0.3), (64, 64, 5.0, 0.3), (65, 63, 5.0, 0.3), (7, 129, 5.0, 0.3), (129, 9, 5.0, 0.3),
          (15, 64, 5.0, 0.3), (16, 63, 5.0, 0.3), (17, 65, 5.0, 0.3), (33, 70, 5.0, 0.3),
          (126, 130, 8.0, 0.2), (128, 128, 8.0, 0.2), (130, 126, 8.0, 0.2), (17, 258, 8.0, 0.2), (258, 15, 8.0, 0.2),
          (30, 128, 8.0, 0.2), (32, 126, 8.0, 0.2), (34, 130, 8.0, 0.2), (66, 140, 8.0, 0.2)]


@pytest.mark.parametrize("H,W,ss,sr", SHAPES)
def test_shapes_around_the_tiles(adf, H, W, ss, sr):
    rng = np.random.default_rng(W * 1000 + H)
    _check(adf, _joint(rng, (H, W), 1), _src(rng, (H, W), np.int16), ss, sr, adjust=True)
    _check(adf, _joint(rng, (H, W), 3), _src(rng, (H, W), np.int16), ss, sr, adjust=False, dst_dtype=np.float32)


# (sigma_s, sigma_r, tree_height) -> (df, height)
REGIMES = [((5.0, 0.3, -1), (1, 2)), ((8.0, 0.2, -1), (2, 2)), ((16.0, 0.2, -1), (4, 3)), ((40.0, 0.1, -1), (8, 4)), ((64.0, 0.1, -1), (16, 5)),
           ((16.0, 0.2, 1), (4, 1)), ((16.0, 0.2, 6), (4, 6))]


@pytest.mark.parametrize("regime,plan", REGIMES)
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("adjust", [False, True])
def test_regimes(adf, regime, plan, ch, adjust):
    ss, sr, height = regime
    H, W = 66, 45
    p = adf.amPlan(ss, sr, height, W, H)
    assert (p["df"], p["height"]) == plan
    rng = np.random.default_rng(int(ss) * 10 + ch)
    _check(adf, _joint(rng, (H, W), ch), _src(rng, (H, W), np.int16), ss, sr, adjust, height=height)


@pytest.mark.parametrize("sdt", DEPTHS)
@pytest.mark.parametrize("ddt", DEPTHS)
def test_source_and_output_depths(adf, sdt, ddt):
    rng = np.random.default_rng(3)
    _check(adf, _joint(rng, (37, 70), 3), _src(rng, (37, 70), sdt), 16.0, 0.2, True, ddt)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("adjust", [False, True])
def test_zero_denominators(adf, ch, adjust):
    rng = np.random.default_rng(4)
    H, W = 40, 52
    joint, src = _joint(rng, (H, W), ch, "blocks"), _src(rng, (H, W), np.int16)
    p = adf.amPlan(16.0, 0.02, -1, W, H)
    g, num, den, mind = am_ref.am_filter(joint, src, p, p["jtab"], adjust, parts=True)
    zero = den == 0
    assert zero.any(), "the case has lost its meaning: the statement's den has no zero"
    got = _check(adf, joint, src, 16.0, 0.02, adjust, np.float32)
    if adjust:
        f = src.astype(np.float32)
        alpha = am_ref.am_exp(mind * p["argOut"])
        assert _same_bits(got[zero], (alpha * (np.float32(0) - f) + f)[zero])
    else:
        assert (got[zero] == 0).all()


@pytest.mark.parametrize("ch", [1, 3])
def test_empty_clusters_on_a_flat_joint(adf, ch):
    rng = np.random.default_rng(6)
    _check(adf, _joint(rng, (30, 41), ch, "flat"), _src(rng, (30, 41), np.int16), 16.0, 0.2, True)
    _check(adf, _joint(rng, (30, 41), ch, "flat"), _src(rng, (30, 41), np.float32), 16.0, 0.2, False)


@pytest.mark.parametrize("dtype,value", [(np.uint8, 200), (np.int16, 2000), (np.int16, 32767), (np.int16, -32768)])
@pytest.mark.parametrize("adjust", [False, True])
def test_constant_sources_come_back(adf, dtype, value, adjust):
    rng = np.random.default_rng(7)
    for ch in (1, 3):
        joint = rng.integers(0, 256, (33, 47, ch), dtype=np.uint8) if ch == 3 else rng.integers(0, 256, (33, 47), dtype=np.uint8)
        got = _check(adf, joint, np.full((33, 47), value, dtype), 16.0, 0.2, adjust)
        assert (got == value).all()


def test_extremes_and_fractions(adf):
    rng = np.random.default_rng(8)
    H, W = 45, 66
    joint = _joint(rng, (H, W), 3)
    _check(adf, joint, rng.choice(np.array([32767, -32768], np.int16), (H, W)), 16.0, 0.2, True)
    _check(adf, joint, (rng.standard_normal((H, W)) * 1e30).astype(np.float32), 16.0, 0.2, False)
    _check(adf, joint, (rng.random((H, W)) * 3 - 1).astype(np.float32), 16.0, 0.2, True, np.float32)


def test_padded_strides_a_batch_and_a_workspace(adf):
    import torch

    rng = np.random.default_rng(11)
    N, H, W = 3, 46, 71

    def padded(a):                      # a view into a larger tensor: W + 6 pixels per row, a spare row per map
        hw = a.shape[1:3]
        big = torch.zeros((a.shape[0], hw[0] + 1, hw[1] + 6) + a.shape[3:], dtype=torch.from_numpy(a[:0]).dtype, device=_dev())
        v = big[:, :hw[0], 2:2 + hw[1]]
        v.copy_(torch.from_numpy(a))
        return v

    src = _src(rng, (N, H, W), np.int16)
    joint = np.stack([_joint(rng, (H, W), 3), _joint(rng, (H, W), 3, "blocks"), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)])
    batch = _check(adf, joint, src, 16.0, 0.2, True, np.float32, to_dev=padded)
    for k in range(N):                                                                      # the batch equals three single calls
        one = adf.amFilter(torch.from_numpy(joint[k]).to(_dev()), torch.from_numpy(src[k]).to(_dev()), 16.0, 0.2, True, dDepth=adf.CV_32F)
        assert _same_bits(one.cpu().numpy(), batch[k])
    dst = padded(np.full((N, H, W), 77, np.int16))
    whole = dst._base if dst._base is not None else dst
    need = adf.amFilterWorkspaceBytes(N, H, W, 3, 16.0, 0.2)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    out = adf.amFilter(padded(joint), padded(src), 16.0, 0.2, dst=dst, workspace=ws)
    assert out is dst
    exp = _expected(adf, joint, src, 16.0, 0.2, False, np.int16)
    assert np.array_equal(dst.cpu().numpy(), exp)
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[:, :H, 2:2 + W] = False
    assert (whole[outside] == 0).all(), "written outside the destination's pixels"
    with pytest.raises(adf.AdfError) as e:                               # a workspace one byte short
        adf.amFilter(padded(joint), padded(src), 16.0, 0.2, dst=dst, workspace=ws[:-1])
    assert e.value.code == 2


def test_the_c_abi_on_a_non_default_stream(adf):
    import torch
    from addingdisparityfiltering_amd import _lib

    rng = np.random.default_rng(13)
    L = _lib.lib()
    H, W = 65, 130
    for ch, sdt, ddt in ((1, np.int16, np.int16), (3, np.float32, np.int16), (3, np.uint8, np.float32)):
        joint, src = _joint(rng, (H, W), ch), _src(rng, (H, W), sdt)
        tj, ts = torch.from_numpy(joint).to(_dev()), torch.from_numpy(src).to(_dev())
        dst = torch.zeros((H, W), dtype=torch.from_numpy(np.zeros(0, ddt)).dtype, device=_dev())
        ws = torch.empty(L.adf_am_filter_workspace_bytes(1, W, H, ch, 16.0, 0.2, -1), dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        rc = L.adf_am_filter_device(1, tj.data_ptr(), W * ch, 0, ch, ts.data_ptr(), W * src.itemsize, 0, DEPTH_CODE[sdt],
                                    dst.data_ptr(), W * np.dtype(ddt).itemsize, 0, DEPTH_CODE[ddt], W, H, 16.0, 0.2, -1, 1,
                                    ws.data_ptr(), ws.numel(), C.c_void_p(st.cuda_stream))
        assert rc == 0, L.adf_last_error()
        st.synchronize()
        assert _same_bits(dst.cpu().numpy(), _expected(adf, joint, src, 16.0, 0.2, True, ddt))
        with torch.cuda.stream(st):                                      # the mirror on torch's current stream
            out = adf.amFilter(tj, ts, 16.0, 0.2, True, dDepth=_ddepth(adf, ddt))
        st.synchronize()
        assert _same_bits(out.cpu().numpy(), dst.cpu().numpy())


def test_host_entry_and_the_filter_object(adf):
    import torch

    rng = np.random.default_rng(12)
    src, joint = _src(rng, (2, 31, 70), np.int16), _joint(rng, (2, 31, 70), 3)
    keep = src.copy(), joint.copy()
    out = adf.amFilter(joint[:, :, 1:], src[:, :, 1:], 16.0, 0.2, dDepth=adf.CV_32F)        # strided host arrays
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    assert _same_bits(out, _expected(adf, joint[:, :, 1:], src[:, :, 1:], 16.0, 0.2, False, np.float32))
    assert np.array_equal(src, keep[0]) and np.array_equal(joint, keep[1])
    tj, ts = torch.from_numpy(np.ascontiguousarray(joint[:, :, 1:])).to(_dev()), torch.from_numpy(np.ascontiguousarray(src[:, :, 1:])).to(_dev())
    f = adf.createAMFilter(16.0, 0.2)
    assert isinstance(f, adf.AdaptiveManifoldFilter)
    assert _same_bits(f.filter(ts, joint=tj, dDepth=adf.CV_32F).cpu().numpy(), out)
    f.setPCAIterations(5)                                                # stored; the result does not change
    f.setAdjustOutliers(True)
    f.setSigmaS(8.0)
    f.setTreeHeight(3)
    got = f.filter(src[0], joint=joint[0])
    assert _same_bits(got, _expected(adf, joint[0], src[0], 8.0, 0.2, True, None, height=3))
    f.collectGarbage()


def test_captured_into_a_graph(adf):
    import torch

    rng = np.random.default_rng(14)
    H, W = 70, 130
    src, joint = _src(rng, (H, W), np.int16), _joint(rng, (H, W), 3)
    ts, tj = torch.from_numpy(src).to(_dev()), torch.from_numpy(joint).to(_dev())
    dst = torch.zeros_like(ts)
    ws = torch.empty(adf.amFilterWorkspaceBytes(1, H, W, 3, 16.0, 0.2), dtype=torch.uint8, device=_dev())
    warm = adf.amFilter(tj, ts, 16.0, 0.2, True).cpu().numpy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one chain of launches: no parallel branches
        adf.amFilter(tj, ts, 16.0, 0.2, True, dst=dst, workspace=ws)
    dst.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), warm)
    assert np.array_equal(warm, _expected(adf, joint, src, 16.0, 0.2, True, np.int16))
