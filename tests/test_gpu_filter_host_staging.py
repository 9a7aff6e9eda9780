"""GPU test of the host-pointer entries of the five edge-aware filters (csrc/adf_host.h: staged_call), which share one
staging path: every image of the call -- guide, src, mask AND dst -- is a strided view into a larger numpy array (3 spare
pixels per row, one spare row per map), n = 2 maps of 11 x 35.  The result must have the bits of the device entry on
contiguous copies of the same data (the per-filter tests tie that entry to the NumPy references), every byte of the
destination's backing array outside its pixels must still hold the sentinel, and the inputs must be unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W = 2, 11, 35
SENTINEL = 0x5A


def _strided(data):
    """`data` (N,H,W[,C]) as a view into a larger array: 3 spare pixels per row, one spare row per map -> (view, backing)."""
    shape = (N, H + 1, W + 3) + data.shape[3:]
    backing = np.frombuffer(bytes([SENTINEL]) * (int(np.prod(shape)) * data.itemsize), data.dtype).reshape(shape).copy()
    view = backing[:, :H, :W]
    view[...] = data
    return view, backing


def _inputs(dtype, channels, seed):
    rng = np.random.default_rng(seed)
    guide = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    guide[:, :, W // 2:] //= 4                                               # an edge
    src = (rng.integers(-2000, 2000, (N, H, W)) if dtype != np.uint8 else rng.integers(0, 256, (N, H, W))).astype(dtype)
    if dtype == np.float32:
        src += np.float32(0.375)
    mask = (rng.random((N, H, W)) < 0.8).astype(np.uint8)
    return (guide if channels == 3 else np.ascontiguousarray(guide[..., 0])), src, mask


# name -> (src dtype, guide channels, dst dtype, uses the mask, call(adf, guide, src, mask, dst, ddepth))
CASES = {
    "wmf-mask": (np.int16, 3, np.int16, True, lambda adf, g, s, m, dst, dd: adf.weightedMedianFilter(g, s, 2, 20.0, mask=m, dst=dst)),
    "wmf-no-mask": (np.int16, 1, np.int16, False, lambda adf, g, s, m, dst, dd: adf.weightedMedianFilter(g, s, 3, 20.0, dst=dst)),
    "gf": (np.int16, 3, np.float32, False, lambda adf, g, s, m, dst, dd: adf.guidedFilter(g, s, 3, 50.0, dDepth=dd, dst=dst)),
    "dt": (np.uint8, 1, np.int16, False, lambda adf, g, s, m, dst, dd: adf.dtFilter(g, s, 8.0, 30.0, numIters=2, dDepth=dd, dst=dst)),
    "jbf": (np.float32, 3, np.uint8, False, lambda adf, g, s, m, dst, dd: adf.jointBilateralFilter(g, s, 5, 30.0, 2.0, dDepth=dd, dst=dst)),
    "rgf-1-iteration": (np.int16, 0, np.int16, False, lambda adf, g, s, m, dst, dd: adf.rollingGuidanceFilter(s, 5, 40.0, 2.0, 1, dst=dst)),
    "rgf-3-iterations": (np.float32, 0, np.float32, False, lambda adf, g, s, m, dst, dd: adf.rollingGuidanceFilter(s, 5, 40.0, 2.0, 3, dst=dst)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_strided_host_call_matches_the_device_entry(adf, name):
    import torch

    dtype, channels, dst_dtype, masked, call = CASES[name]
    guide, src, mask = _inputs(dtype, channels or 1, sorted(CASES).index(name))
    ddepth = {np.uint8: adf.CV_8U, np.int16: adf.CV_16S, np.float32: adf.CV_32F}[dst_dtype]
    # the device entry on contiguous copies
    dev = torch.device("cuda:0")
    expected = torch.empty((N, H, W), dtype=getattr(torch, np.dtype(dst_dtype).name), device=dev)
    call(adf, torch.from_numpy(guide).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(mask).to(dev) if masked else None, expected, ddepth)
    torch.cuda.synchronize()
    expected = expected.cpu().numpy()
    # the host entry on strided views
    (g, g_back), (s, s_back), (m, m_back) = _strided(guide), _strided(src), _strided(mask)
    kept = [b.copy() for b in (g_back, s_back, m_back)]
    d, d_back = _strided(np.frombuffer(bytes([SENTINEL]) * (N * H * W * np.dtype(dst_dtype).itemsize), dst_dtype).reshape(N, H, W))
    assert not s.flags.c_contiguous and not d.flags.c_contiguous and s.strides[1] == (W + 3) * s.itemsize
    got = call(adf, g, s, m if masked else None, d, ddepth)
    assert got is d
    bits = np.dtype("u%d" % np.dtype(dst_dtype).itemsize)
    assert np.array_equal(np.ascontiguousarray(d).view(bits), expected.view(bits))
    assert not (np.ascontiguousarray(d).view(np.uint8) == SENTINEL).all()        # the call wrote its maps
    outside = d_back.copy()
    outside[:, :H, :W] = np.frombuffer(bytes([SENTINEL]) * outside.itemsize, outside.dtype)[0]
    assert (outside.view(np.uint8) == SENTINEL).all(), "the call wrote outside the destination's pixels"
    for back, before in zip((g_back, s_back, m_back), kept):
        assert np.array_equal(back.view(np.uint8), before.view(np.uint8)), "the call wrote an input"
