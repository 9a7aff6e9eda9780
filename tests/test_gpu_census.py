"""GPU tests of the census transform (csrc/census_kernels.hip) and of the semi-global matcher's census / Hamming cost
(csrc/sgbm_matcher.hip, ADF_SGBM_COST_CENSUS_*), through the C-ABI and the Python mirror.

Integer work: every comparison is bit-exact against the direct statement tests/census_ref.py (checked on its own by
tests/test_census_ref.py).  The reference-held anchor is its stereo module's semi-global test, whose matcher uses a
census cost (modules/stereo/test/test_block_matching.cpp:157-238: the Tsukuba pair, at most 10 %)."""
import ctypes as C

import numpy as np
import pytest

from census_ref import census_transform, naive_census_sgbm
from test_oracle_bm import load_tsukuba
from test_oracle_sgbm import _pair, naive_median3, ref_error_level

pytestmark = pytest.mark.gpu

DENSE, SPARSE = 1, 2                                   # ADF_SGBM_COST_CENSUS_DENSE / _SPARSE
DESCRIPTORS = [(DENSE, 3), (DENSE, 5), (DENSE, 7), (SPARSE, 5), (SPARSE, 7), (SPARSE, 9), (SPARSE, 11)]
EBADARG = 1


def _image(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _bits(t):
    """The uint64 bit pattern an int64 tensor carries."""
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------
# transform
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype,k", DESCRIPTORS)
def test_transform_every_descriptor_device_and_host(adf, ctype, k):
    """(1, 1) and (3, 5) are smaller than every window (all clamped), (7, 64) is one full tile row, (33, 257) and
    (41, 150) have several workgroups in both directions with partial ones at the edges."""
    import torch
    for H, W in ((1, 1), (3, 5), (7, 64), (33, 257), (41, 150)):
        img = _image(H * W + k, H, W)
        exp = census_transform(img, k, ctype == SPARSE)
        host = adf.censusTransform(img, k, ctype)
        assert host.dtype == np.uint64 and np.array_equal(host, exp), (H, W)
        t = torch.from_numpy(img).cuda()
        dev = adf.censusTransform(t, k, ctype)
        again = adf.censusTransform(t, k, ctype)
        assert dev.dtype == torch.int64 and dev.is_cuda
        assert np.array_equal(_bits(dev), exp), (H, W)
        assert torch.equal(dev, again)                                   # a run repeated is identical


def test_transform_padded_rows_and_batch_with_image_stride(adf):
    import torch
    N, H, W = 3, 19, 70
    imgs = np.stack([_image(50 + i, H, W) for i in range(N)])
    exp = np.stack([census_transform(im, 7, False) for im in imgs])
    src = np.zeros((N, H + 2, W + 5), np.uint8); src[:, :H, :W] = imgs    # rows and images further apart than they need be
    dst = np.full((N, H + 1, W + 3), 77, np.uint64)
    res = adf.censusTransform(src[:, :H, :W], 7, DENSE, dst[:, :H, :W])
    assert res.base is dst and np.array_equal(dst[:, :H, :W], exp)
    assert (dst[:, H:] == 77).all() and (dst[:, :, W:] == 77).all()
    tsrc = torch.from_numpy(src).cuda()
    tdst = torch.full((N, H + 1, W + 3), 77, dtype=torch.int64, device="cuda")
    adf.censusTransform(tsrc[:, :H, :W], 7, DENSE, tdst[:, :H, :W])
    assert np.array_equal(_bits(tdst[:, :H, :W].contiguous()), exp)
    assert (tdst[:, H:] == 77).all() and (tdst[:, :, W:] == 77).all()
    one = adf.censusTransform(tsrc[1, :H, :W], 9, SPARSE)                 # unbatched, strided rows
    assert np.array_equal(_bits(one), census_transform(imgs[1], 9, True))


# ------------------------------------------------------------------------------------------------
# matcher against the direct statement
# ------------------------------------------------------------------------------------------------
def _matcher(adf, nd, bs, md=0, P1=10, P2=100, ur=0, mode=2, ctype=DENSE, k=5, disp12=1000000):
    m = adf.StereoSGBM.create(md, nd, bs)
    m.setP1(P1); m.setP2(P2); m.setUniquenessRatio(ur); m.setMode(mode)
    m.setDisp12MaxDiff(disp12); m.setSpeckleWindowSize(0)
    m.setCostType(ctype); m.setCensusSize(k)
    return m


def _expected(a, b, nd, bs, md=0, P1=10, P2=100, ur=0, mode=2, ctype=DENSE, k=5, disp12=1000000):
    return naive_median3(naive_census_sgbm(a, b, nd, bs, md, P1, P2, ur, mode, disp12, k, ctype == SPARSE))


@pytest.mark.parametrize("bs", [1, 3, 5, 7, 9, 11])
def test_every_block_size_bit_exact(adf, bs):
    """Both disparities-per-wave instantiations (16 up to blockSize 5, 8 above), several row bands, two column tiles."""
    a, b = _pair(bs, 41, 150, shift=5)
    assert np.array_equal(_matcher(adf, 32, bs).compute(a, b), _expected(a, b, 32, bs))


@pytest.mark.parametrize("ctype,k", DESCRIPTORS)
def test_every_descriptor_bit_exact(adf, ctype, k):
    a, b = _pair(100 + k, 13, 40)
    assert np.array_equal(_matcher(adf, 16, 3, ctype=ctype, k=k).compute(a, b), _expected(a, b, 16, 3, ctype=ctype, k=k))


@pytest.mark.parametrize("H,W,nd,bs,kw", [
    (12, 45, 16, 1, dict(md=-15)),                       # the right matcher's range (minDisparity = -(0 + 16) + 1)
    (10, 50, 32, 3, dict(md=2, ur=15)),                  # positive minimum disparity, uniqueness test on
    (20, 150, 80, 3, dict()),                            # 80 disparities: the second workgroup in d is partly filled
    (7, 20, 32, 3, dict()),                              # search range wider than the image: everything invalid
    (12, 40, 16, 3, dict(mode=0)),                       # MODE_SGBM
    (12, 40, 16, 3, dict(mode=1)),                       # MODE_HH
    (14, 70, 16, 3, dict(disp12=1)),                     # the matcher's own left-right check
    (9, 60, 16, 5, dict(ctype=SPARSE, k=11, P1=0, P2=0)),   # default penalties (2 / 5)
])
def test_parameter_corners_bit_exact(adf, H, W, nd, bs, kw):
    a, b = _pair(H * W + nd, H, W, shift=4)
    got = _matcher(adf, nd, bs, **kw).compute(a, b)
    exp = _expected(a, b, nd, bs, **kw)
    assert got.shape == (H, W) and np.array_equal(got, exp)
    md = kw.get("md", 0)
    if W - max(md + nd, 0) + min(md, 0) <= 0:
        assert (got == (md - 1) * 16).all()


def test_left_right_check_fires_on_occlusions(adf):
    rng = np.random.default_rng(41)
    H, W = 14, 70
    base = rng.integers(0, 256, (H, W + 40), dtype=np.uint8)
    a = np.ascontiguousarray(base[:, 20:20 + W])
    b = np.ascontiguousarray(base[:, 23:23 + W]).copy()
    b[:, 30:] = base[:, 20 + 39:20 + 39 + W - 30]                    # right half at a larger disparity: occlusions
    raw_on = naive_census_sgbm(a, b, 16, 3, 0, 10, 100, 0, 2, 1, 5, False)
    raw_off = naive_census_sgbm(a, b, 16, 3, 0, 10, 100, 0, 2, 1000000, 5, False)
    assert (raw_on != raw_off).any() and ((raw_on == raw_off) | (raw_on == -16)).all()
    assert np.array_equal(_matcher(adf, 16, 3, disp12=1).compute(a, b), naive_median3(raw_on))


def test_device_batch_strided_and_host_entry(adf):
    import torch
    N, H, W = 3, 21, 90
    pairs = [_pair(300 + i, H, W, shift=3 + i) for i in range(N)]
    exp = [_expected(l, r, 32, 3, k=7) for l, r in pairs]
    bl = torch.zeros((N, H, W + 5), dtype=torch.uint8, device="cuda"); br = torch.zeros((N, H + 1, W + 9), dtype=torch.uint8, device="cuda")
    for i, (l, r) in enumerate(pairs):
        bl[i, :, :W] = torch.from_numpy(l).cuda(); br[i, :H, :W] = torch.from_numpy(r).cuda()
    out = torch.full((N, H, W + 3), 777, dtype=torch.int16, device="cuda")
    m = _matcher(adf, 32, 3, k=7)
    res = m.compute(bl[:, :, :W], br[:, :H, :W], out[:, :, :W])
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and (out[:, :, W:] == 777).all()
    for i in range(N):
        assert np.array_equal(out[i, :, :W].cpu().numpy(), exp[i])
    assert torch.equal(m.compute(bl[1, :, :W], br[1, :H, :W]), out[1, :, :W])      # unbatched, same handle
    hl = np.zeros((N, H, W + 9), np.uint8); hr = np.zeros((N, H, W + 5), np.uint8)  # the host entry, padded rows
    for i, (l, r) in enumerate(pairs):
        hl[i, :, :W] = l; hr[i, :, :W] = r
    hout = np.full((N, H, W + 3), 555, np.int16)
    m.compute(hl[:, :, :W], hr[:, :, :W], hout[:, :, :W])
    assert (hout[:, :, W:] == 555).all()
    for i in range(N):
        assert np.array_equal(hout[i, :, :W], exp[i])


def test_compute_is_capturable_once_the_workspace_exists(adf):
    """No allocation and no synchronisation inside compute() after the first call of a size: a captured call replays."""
    import torch
    a, b = _pair(8, 30, 120, shift=6)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = _matcher(adf, 32, 5, k=7)
    eager = m.compute(ta, tb).clone()
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                             # one linear graph
        m.compute(ta, tb, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and np.array_equal(eager.cpu().numpy(), _expected(a, b, 32, 5, k=7))


# ------------------------------------------------------------------------------------------------
# the reference's bar on its own data
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype,k,bs,P1,P2,ur", [
    (DENSE, 5, 3, 10, 100, 1),
    (DENSE, 7, 5, 10, 100, 1),
    (SPARSE, 9, 5, 10, 100, 1),
    (DENSE, 7, 1, 10, 100, 1),
    (DENSE, 7, 3, 24, 96, 0),
    (DENSE, 3, 5, 10, 100, 1),
])
def test_reference_fixture_bar(adf, ctype, k, bs, P1, P2, ur):
    left, right, gt = load_tsukuba()
    got = _matcher(adf, 16, bs, 0, P1, P2, ur, ctype=ctype, k=k).compute(left, right)
    err = ref_error_level(gt, got)
    print("census %s %d block %d P1 %d P2 %d uniqueness %d: error %.2f %%" % ("dense" if ctype == DENSE else "sparse", k, bs, P1, P2, ur, err))
    assert err <= 10.0                                                    # test_block_matching.cpp:231


def test_reference_fixture_bar_bites(adf):
    left, right, gt = load_tsukuba()
    got = _matcher(adf, 16, 3, 0, 10, 100, 1, ctype=DENSE, k=7).compute(right, left)
    err = ref_error_level(gt, got)
    print("census dense 7 block 3, views swapped: error %.2f %%" % err)
    assert err > 30.0


# ------------------------------------------------------------------------------------------------
# the Birchfield-Tomasi cost is untouched
# ------------------------------------------------------------------------------------------------
def test_new_handle_reports_bt(adf):
    from addingdisparityfiltering_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.adf_sgbm_create(C.byref(h), 0, 16, 3))
    try:
        cost, size = C.c_int(-1), C.c_int(-1)
        _lib.check(L.adf_sgbm_get_cost(h, C.byref(cost), C.byref(size)))
        assert cost.value == adf.SGBM_COST_BT == 0
        _lib.check(L.adf_sgbm_set_cost(h, SPARSE, 9))
        _lib.check(L.adf_sgbm_get_cost(h, C.byref(cost), C.byref(size)))
        assert (cost.value, size.value) == (SPARSE, 9)
        assert L.adf_sgbm_set_cost(h, DENSE, 9) == EBADARG               # refused: the handle keeps its cost
        _lib.check(L.adf_sgbm_get_cost(h, C.byref(cost), C.byref(size)))
        assert (cost.value, size.value) == (SPARSE, 9)
    finally:
        L.adf_sgbm_destroy(h)
    assert adf.StereoSGBM.create(0, 16, 3).getCostType() == adf.SGBM_COST_BT


def test_one_handle_switches_cost_between_calls(adf, oracle):
    """Census, Birchfield-Tomasi, census on ONE handle: the workspace layout follows the cost (8 against 12 bytes per
    pixel and plane), the BT call is the oracle's bit for bit, both census calls the direct statement's."""
    a, b = _pair(77, 37, 140, shift=6)
    exp_census = _expected(a, b, 32, 3, P1=72, P2=288, k=7)
    exp_bt = oracle.sgbm_compute(a, b, 32, 3, 0, 72, 288, 63, 0)
    m = _matcher(adf, 32, 3, P1=72, P2=288, k=7); m.setPreFilterCap(63)
    first = m.compute(a, b)
    handle = m._h.value
    m.setCostType(adf.SGBM_COST_BT)
    assert np.array_equal(m.compute(a, b), exp_bt)
    m.setCostType(adf.SGBM_COST_CENSUS_DENSE)
    again = m.compute(a, b)
    assert m._h.value == handle
    assert np.array_equal(first, exp_census) and np.array_equal(again, exp_census)
    assert not np.array_equal(exp_census, exp_bt)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _refused(adf, fn):
    with pytest.raises(adf.AdfError) as e:
        fn()
    assert e.value.code == EBADARG and len(str(e.value)) > len("adf error 1: ")
    return str(e.value)


def test_refusals(adf):
    import torch
    from addingdisparityfiltering_amd import _lib
    a, b = _pair(3, 20, 60)
    c3 = np.ascontiguousarray(np.stack([a, a, a], 2))
    assert "CV_8UC1" in _refused(adf, lambda: _matcher(adf, 16, 3).compute(c3, c3))        # census with 3-channel views
    for ctype, k in ((DENSE, 9), (SPARSE, 13), (DENSE, 4), (SPARSE, 6), (SPARSE, 3), (3, 5), (-1, 5)):
        _refused(adf, lambda: _matcher(adf, 16, 3, ctype=ctype, k=k).compute(a, b))
        _refused(adf, lambda: adf.censusTransform(a, k, ctype))
    _refused(adf, lambda: adf.censusTransform(a, 5, adf.SGBM_COST_BT))                     # not a descriptor
    # a mis-aligned dst, straight on the C-ABI (the mirror only makes aligned ones)
    L = _lib.lib()
    src = torch.from_numpy(a).cuda()
    dst = torch.zeros((2 * 20 * 60 + 2,), dtype=torch.int64, device="cuda")
    args = (1, src.data_ptr(), 60, 0, 60, 20, DENSE, 5)
    assert L.adf_census_transform_device(*args, dst.data_ptr() + 4, 60 * 8, 0, None) == EBADARG
    assert b"8-byte" in L.adf_last_error()
    assert L.adf_census_transform_device(*args, dst.data_ptr(), 60 * 8 + 4, 0, None) == EBADARG
    assert L.adf_census_transform_device(2, *args[1:], dst.data_ptr(), 60 * 8, 20 * 60 * 8 + 4, None) == EBADARG
    torch.cuda.synchronize()
    assert (dst == 0).all()                                                                 # nothing was written
    assert L.adf_census_transform_device(*args, dst.data_ptr(), 60 * 8, 0, None) == 0       # the same call, aligned
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dst[:1200]).reshape(20, 60), census_transform(a, 5, False))


# ------------------------------------------------------------------------------------------------
# views -> filtered disparity
# ------------------------------------------------------------------------------------------------
def test_views_to_filtered_disparity_with_the_census_matcher(adf, oracle):
    """A 96 x 160 crop of the Tsukuba pair: the census matcher for both views (the right one from createRightMatcher,
    which carries the cost over), then the filter set up from the matcher, every stage on the device, against the direct
    statement for both views followed by the oracle's filter."""
    import torch
    left, right, _ = load_tsukuba()
    left = np.ascontiguousarray(left[100:196, 120:280]); right = np.ascontiguousarray(right[100:196, 120:280])
    nd, bs = 16, 3
    lm = adf.StereoSGBM.create(0, nd, bs)
    lm.setP1(10); lm.setP2(100); lm.setMode(adf.StereoSGBM.MODE_SGBM_3WAY)
    lm.setCostType(adf.SGBM_COST_CENSUS_DENSE); lm.setCensusSize(7)
    wls = adf.createDisparityWLSFilter(lm)
    rm = adf.createRightMatcher(lm)
    assert (rm.getCostType(), rm.getCensusSize(), rm.getMinDisparity()) == (adf.SGBM_COST_CENSUS_DENSE, 7, -nd + 1)
    wls.setLambda(8000.0); wls.setSigmaColor(1.5); wls.setSolver(adf.SOLVER_EXACT)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    dl = lm.compute(tl, tr); dr = rm.compute(tr, tl)
    out = wls.filter(dl, tl, None, dr)
    torch.cuda.synchronize()
    edl = _expected(left, right, nd, bs, k=7).astype(np.int16)
    edr = _expected(right, left, nd, bs, md=-nd + 1, k=7).astype(np.int16)
    assert np.array_equal(dl.cpu().numpy(), edl) and np.array_equal(dr.cpu().numpy(), edr)
    assert (edl[:, nd:] >= 0).mean() > 0.8                               # the crop really matches
    roi = wls.getROI()
    assert roi == (nd, 0, left.shape[1] - nd, left.shape[0])             # DF.cpp:407
    p = oracle.default_params(threads=4, use_confidence=1, disc_radius=2)
    p.lambda_ = 8000.0; p.sigma_color = 1.5
    exp, exp_conf = oracle.wls_filter(edl, left, edr, roi, p)
    assert np.array_equal(wls.getConfidenceMap().cpu().numpy(), exp_conf)
    assert np.array_equal(out.cpu().numpy(), exp)                        # the tolerance of the Birchfield-Tomasi pipeline test: none
