"""GPU tests of the modified census transform and the centre-symmetric census (csrc/census.h: the window-mean and the
mirrored-neighbour comparison rules) through the transform (csrc/census_kernels.hip), the block matcher's pack kernel
(csrc/bm_matcher.hip) and the semi-global matcher (csrc/sgbm_matcher.hip), on the C-ABI and through the Python mirror.

Integer work: every result is compared bit for bit with the direct statements tests/census_variants_ref.py (checked on
their own by tests/test_census_variants_ref.py).  There is no tolerance anywhere in this file."""
import ctypes as C
import functools

import numpy as np
import pytest

from census_variants_ref import CS, DENSE, MCT_DENSE, MCT_SPARSE, VARIANTS, bm_variant, sgbm_variant, transform
from test_oracle_sgbm import _pair, naive_median3

pytestmark = pytest.mark.gpu

BT, SAD, EBADARG = 0, 0, 1


def _image(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _bits(t):
    """The uint64 bit pattern an int64 tensor carries."""
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------
# transform
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype,k", VARIANTS)
def test_transform_every_descriptor_device_and_host(adf, ctype, k):
    """(1, 1) and (2, 3) are smaller than every window (all clamped), (17, 65) is one past a tile edge in both directions,
    (40, 130) has several workgroups with partial ones at the edges."""
    import torch
    for H, W in ((1, 1), (2, 3), (17, 65), (40, 130)):
        img = _image(H * W + k, H, W)
        exp = transform(img, ctype, k)
        host = adf.censusTransform(img, k, ctype)
        assert host.dtype == np.uint64 and np.array_equal(host, exp), (H, W)
        t = torch.from_numpy(img).cuda()
        dev = adf.censusTransform(t, k, ctype)
        again = adf.censusTransform(t, k, ctype)
        assert dev.dtype == torch.int64 and dev.is_cuda
        assert np.array_equal(_bits(dev), exp), (H, W)
        assert torch.equal(dev, again)                                   # a second call gives the same bits


def test_transform_window_mean_decides_on_one_grey_level(adf):
    """255s with one 254 and the reverse at k = 11: 121 * p against the window sum has no rounding to hide behind."""
    for fill, odd in ((255, 254), (254, 255)):
        img = np.full((20, 70), fill, np.uint8); img[9, 33] = odd; img[0, 0] = odd; img[19, 66] = odd
        assert np.array_equal(adf.censusTransform(img, 11, MCT_SPARSE), transform(img, MCT_SPARSE, 11))
        assert np.array_equal(adf.censusTransform(img, 7, MCT_DENSE), transform(img, MCT_DENSE, 7))


@pytest.mark.parametrize("ctype,k", [(CS, 9), (MCT_SPARSE, 11)])
def test_transform_batch_with_strided_rows_into_dst(adf, ctype, k):
    import torch
    N, H, W = 3, 19, 70
    imgs = np.stack([_image(50 + i, H, W) for i in range(N)])
    exp = np.stack([transform(im, ctype, k) for im in imgs])
    src = np.zeros((N, H + 2, W + 5), np.uint8); src[:, :H, :W] = imgs    # rows and images further apart than they need be
    dst = np.full((N, H + 1, W + 3), 77, np.uint64)
    res = adf.censusTransform(src[:, :H, :W], k, ctype, dst[:, :H, :W])
    assert res.base is dst and np.array_equal(dst[:, :H, :W], exp)
    assert (dst[:, H:] == 77).all() and (dst[:, :, W:] == 77).all()
    tsrc = torch.from_numpy(src).cuda()
    tdst = torch.full((N, H + 1, W + 3), 77, dtype=torch.int64, device="cuda")
    adf.censusTransform(tsrc[:, :H, :W], k, ctype, tdst[:, :H, :W])
    assert np.array_equal(_bits(tdst[:, :H, :W].contiguous()), exp)
    assert (tdst[:, H:] == 77).all() and (tdst[:, :, W:] == 77).all()


# ------------------------------------------------------------------------------------------------
# block matcher
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _views(seed, H, W, shift=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W + 96), dtype=np.uint8)
    base = (base // 2 + np.roll(base, 1, 1) // 4 + np.roll(base, 1, 0) // 4).astype(np.uint8)
    base[H // 4:H // 2, 60:60 + W // 4] = 90                                        # a flat patch: nothing but ties
    base[H // 2:, 50:50 + W // 3] = (40 + 150 * ((np.arange(W // 3) // 3) % 2)).astype(np.uint8)   # a repetitive one
    left = np.ascontiguousarray(base[:, 40:40 + W]); right = np.ascontiguousarray(np.roll(base, -shift, 1)[:, 40:40 + W])
    left.setflags(write=False); right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def _bm_expected(key, swap, nd, bs, md, uniq, ctype, k):
    """The statement's map of the pair _views(*key), computed once per configuration, shared and left unchanged."""
    a, b = _views(*key)
    if swap:
        a, b = b, a
    out = bm_variant(a, b, nd, bs, md, uniq, ctype, k)
    out.setflags(write=False)
    return out


def _bm(adf, nd, bs, md=0, uniq=0, ctype=CS, k=7):
    bm = adf.StereoBM.create(nd, bs)
    bm.setMinDisparity(md); bm.setTextureThreshold(0); bm.setUniquenessRatio(uniq)
    bm.setCostType(ctype); bm.setCensusSize(k)
    return bm


@pytest.mark.parametrize("ctype,k", VARIANTS)
def test_bm_every_descriptor_compute_and_compute_both(adf, ctype, k):
    """30 x 80, 16 disparities, block 9: the left map of compute and of computeBoth against the statement, the right map
    against the statement with the views swapped and minDisparity = -(min + num) + 1."""
    import torch
    key, nd, bs = (1, 30, 80, 5), 16, 9
    left, right = _views(*key)
    exp_l = _bm_expected(key, False, nd, bs, 0, 0, ctype, k)
    exp_r = _bm_expected(key, True, nd, bs, -nd + 1, 0, ctype, k)
    bm = _bm(adf, nd, bs, ctype=ctype, k=k)
    assert np.array_equal(bm.compute(left, right), exp_l)
    dl, dr = bm.computeBoth(torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda())
    assert np.array_equal(dl.cpu().numpy(), exp_l) and np.array_equal(dr.cpu().numpy(), exp_r)
    inner = exp_l[4:-4, 19:-4].astype(np.int64)
    assert (inner != -16).all() and (np.abs(inner - 5 * 16) <= 8).mean() > 0.5      # the pair really matches: most pixels find the shift


@pytest.mark.parametrize("H,W,nd,bs,md,uniq,ctype,k", [
    (30, 80, 16, 9, 2, 0, MCT_SPARSE, 9),                # positive minimum disparity
    (30, 80, 16, 9, 0, 15, MCT_DENSE, 5),                # the uniqueness test
    (50, 90, 16, 21, 0, 0, CS, 3),                       # the widest window on the narrowest descriptor (4 bits, one plane)
    (30, 80, 16, 9, 0, 15, CS, 5),                       # 12 bits: the second plane is half empty
])
def test_bm_parameter_corners(adf, H, W, nd, bs, md, uniq, ctype, k):
    key = (H + bs, H, W, 5)
    left, right = _views(*key)
    got = _bm(adf, nd, bs, md, uniq, ctype, k).compute(left, right)
    exp = _bm_expected(key, False, nd, bs, md, uniq, ctype, k)
    assert np.array_equal(got, exp)
    w2 = bs // 2
    inner = exp[w2:H - w2, md + nd - 1 + w2:W - w2]
    assert (inner != (md - 1) * 16).any()
    if uniq:
        assert (inner == (md - 1) * 16).any()                                       # the test rejects some, not all


# ------------------------------------------------------------------------------------------------
# semi-global matcher
# ------------------------------------------------------------------------------------------------
SG = dict(nd=32, bs=3, P1=72, P2=288)


@functools.lru_cache(maxsize=None)
def _sg_pair(seed=77):
    a, b = _pair(seed, 37, 140, shift=6)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _sg_expected(seed, ctype, k, mode=2, disp12=1000000):
    a, b = _sg_pair(seed)
    out = naive_median3(sgbm_variant(a, b, SG["nd"], SG["bs"], 0, SG["P1"], SG["P2"], 0, mode, disp12, ctype, k))
    out.setflags(write=False)
    return out


def _sgbm(adf, ctype, k, mode=2, disp12=1000000):
    m = adf.StereoSGBM.create(0, SG["nd"], SG["bs"])
    m.setP1(SG["P1"]); m.setP2(SG["P2"]); m.setUniquenessRatio(0); m.setMode(mode)
    m.setDisp12MaxDiff(disp12); m.setSpeckleWindowSize(0)
    m.setCostType(ctype); m.setCensusSize(k)
    return m


@pytest.mark.parametrize("ctype,k", [(MCT_DENSE, 5), (MCT_SPARSE, 9), (CS, 3), (CS, 9)])
def test_sgbm_descriptors_bit_exact(adf, ctype, k):
    """37 x 140, 32 disparities, block 3, P1 72, P2 288, 3-way."""
    a, b = _sg_pair()
    got = _sgbm(adf, ctype, k).compute(a, b)
    exp = _sg_expected(77, ctype, k)
    assert np.array_equal(got, exp)
    assert (np.abs(exp[:, 40:-8].astype(np.int64) - 6 * 16) <= 8).mean() > 0.5      # the pair really matches at its shift


def test_sgbm_mode_hh_with_the_left_right_check(adf):
    a, b = _sg_pair()
    got = _sgbm(adf, CS, 9, mode=1, disp12=1).compute(a, b)
    assert np.array_equal(got, _sg_expected(77, CS, 9, 1, 1))


def test_sgbm_batch_of_two(adf):
    import torch
    pairs = [_sg_pair(77), _sg_pair(78)]
    left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda(); right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    got = _sgbm(adf, MCT_SPARSE, 9).compute(left, right).cpu().numpy()
    assert got.shape == (2, 37, 140)
    assert np.array_equal(got[0], _sg_expected(77, MCT_SPARSE, 9)) and np.array_equal(got[1], _sg_expected(78, MCT_SPARSE, 9))


def test_sgbm_one_handle_switches_cost_between_calls(adf, oracle):
    """Birchfield-Tomasi, centre-symmetric 7, census dense 7, modified census dense 7 on ONE handle: each result is its
    statement's (the first the oracle's), and no two of them are the same map."""
    a, b = _sg_pair()
    m = _sgbm(adf, BT, 7); m.setPreFilterCap(63)
    maps = [m.compute(a, b)]
    assert np.array_equal(maps[0], oracle.sgbm_compute(a, b, SG["nd"], SG["bs"], 0, SG["P1"], SG["P2"], 63, 0))
    handle = m._h.value
    for ctype in (CS, DENSE, MCT_DENSE):
        m.setCostType(ctype)
        maps.append(m.compute(a, b))
        assert np.array_equal(maps[-1], _sg_expected(77, ctype, 7)), ctype
        assert m._h.value == handle
    assert all(not np.array_equal(maps[i], maps[j]) for i in range(4) for j in range(i))


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
REFUSED = [(CS, 11), (CS, 4), (MCT_DENSE, 9), (MCT_SPARSE, 3), (3, 5), (7, 5)]


def test_refusals_on_the_c_abi_keep_the_cost(adf):
    from addingdisparityfiltering_amd import _lib
    L = _lib.lib()
    hb, hs = C.c_void_p(), C.c_void_p()
    _lib.check(L.adf_bm_create(C.byref(hb), 16, 9))
    _lib.check(L.adf_sgbm_create(C.byref(hs), 0, 16, 3))
    try:
        for h, setter, getter in ((hb, L.adf_bm_set_cost, L.adf_bm_get_cost), (hs, L.adf_sgbm_set_cost, L.adf_sgbm_get_cost)):
            def cost():
                c, s = C.c_int(-1), C.c_int(-1)
                _lib.check(getter(h, C.byref(c), C.byref(s)))
                return c.value, s.value

            for good in ((CS, 9), (MCT_SPARSE, 11), (MCT_DENSE, 3), (CS, 3)):
                _lib.check(setter(h, *good))
                assert cost() == good
            for bad in REFUSED:
                assert setter(h, *bad) == EBADARG and len(L.adf_last_error()) > 0, bad
                assert cost() == (CS, 3)                                            # the handle keeps its cost
        src = np.zeros((8, 8), np.uint8); dst = np.zeros((8, 8), np.uint64)
        for bad in REFUSED:
            assert L.adf_census_transform_host(1, src.ctypes.data, 8, 0, 8, 8, bad[0], bad[1], dst.ctypes.data, 64, 0) == EBADARG
            assert len(L.adf_last_error()) > 0
        assert L.adf_census_transform_host(1, src.ctypes.data, 8, 0, 8, 8, CS, 9, dst.ctypes.data, 64, 0) == 0
    finally:
        L.adf_bm_destroy(hb); L.adf_sgbm_destroy(hs)


def _refused(adf, fn):
    with pytest.raises(adf.AdfError) as e:
        fn()
    assert e.value.code == EBADARG and len(str(e.value)) > len("adf error 1: ")
    return str(e.value)


def test_refusals_through_the_mirror(adf):
    a, b = _pair(3, 30, 80)
    for ctype, k in REFUSED:
        _refused(adf, lambda: adf.censusTransform(a, k, ctype))
        _refused(adf, lambda: _bm(adf, 16, 9, ctype=ctype, k=k).compute(a, b))
        _refused(adf, lambda: _sgbm(adf, ctype, k).compute(a, b))
    c3 = np.ascontiguousarray(np.stack([a, a, a], 2))
    for ctype, k in ((CS, 7), (MCT_DENSE, 5), (MCT_SPARSE, 9)):
        assert "CV_8UC1" in _refused(adf, lambda: _sgbm(adf, ctype, k).compute(c3, c3))   # a descriptor of 3-channel views
    # a matcher that was refused a pair goes on with the one it had
    bm = _bm(adf, 16, 9, ctype=CS, k=5)
    first = bm.compute(a, b)
    bm.setCensusSize(11)
    _refused(adf, lambda: bm.compute(a, b))
    bm.setCensusSize(5)
    assert np.array_equal(bm.compute(a, b), first)


# ------------------------------------------------------------------------------------------------
# matcher -> filter
# ------------------------------------------------------------------------------------------------
def test_cs7_block_matcher_into_the_wls_filter(adf):
    """A 60 x 120 synthetic pair: computeBoth with the centre-symmetric 7 cost gives the statement's two maps, and the
    filter gives from them what it gives from the statement's maps."""
    import torch
    nd, bs = 16, 9
    key = (9, 60, 120, 5)
    left, right = _views(*key)
    lm = adf.StereoBM.create(nd, bs)
    lm.setCostType(adf.BM_COST_CENSUS_CS); lm.setCensusSize(7)
    wls = adf.createDisparityWLSFilter(lm)                                          # forces textureThreshold = uniquenessRatio = 0
    assert (lm.getCostType(), lm.getCensusSize(), lm.getUniquenessRatio()) == (adf.BM_COST_CENSUS_CS, 7, 0)
    wls.setLambda(8000.0); wls.setSigmaColor(1.5)
    tl, tr = torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda()
    dl, dr = lm.computeBoth(tl, tr)
    out = wls.filter(dl, tl, None, dr).clone()
    conf = wls.getConfidenceMap().clone()
    edl = _bm_expected(key, False, nd, bs, 0, 0, CS, 7)
    edr = _bm_expected(key, True, nd, bs, -nd + 1, 0, CS, 7)
    assert np.array_equal(dl.cpu().numpy(), edl) and np.array_equal(dr.cpu().numpy(), edr)
    assert (edl[4:-4, nd + 3:-4] >= 0).mean() > 0.8                                 # the pair really matches
    ref = wls.filter(torch.from_numpy(edl.copy()).cuda(), tl, None, torch.from_numpy(edr.copy()).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(conf, wls.getConfidenceMap())
