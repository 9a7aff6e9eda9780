"""GPU tests of the block matcher's census / Hamming cost (csrc/bm_matcher.hip: bm_census_pack_kernel and the census
policy of bm_match_kernel; include/adf_wls.h: adf_bm_set_cost).

Integer work: every map is compared bit for bit with the direct statement tests/bm_census_ref.py.  The shapes are the
smallest at which the kernels can go wrong: every plane count, heights that are no multiple of a row group, matched
columns that cross a wave tile (256 - 2*w2 columns; 128 - 2*w2 with the uniqueness test and, for the census cost, at
window half-sizes 9 and 10), more than one workgroup of four row groups."""
import ctypes as C
import functools

import numpy as np
import pytest

from bm_census_ref import bm_census
from test_oracle_bm import error_level, load_tsukuba

pytestmark = pytest.mark.gpu

SAD, DENSE, SPARSE = 0, 1, 2
PAIRS = [(DENSE, 3), (DENSE, 5), (DENSE, 7), (SPARSE, 5), (SPARSE, 7), (SPARSE, 9), (SPARSE, 11)]   # 1, 3, 6, 1, 2, 3, 5 planes


@functools.lru_cache(maxsize=None)
def _views(seed, H, W, shift=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W + 96), dtype=np.uint8)
    base = (base // 2 + np.roll(base, 1, 1) // 4 + np.roll(base, 1, 0) // 4).astype(np.uint8)
    base[H // 4:H // 2, 60:60 + W // 4] = 90                                        # a flat patch: nothing but ties
    base[H // 2:, 50:50 + W // 3] = (40 + 150 * ((np.arange(W // 3) // 3) % 2)).astype(np.uint8)   # a repetitive one
    left = np.ascontiguousarray(base[:, 40:40 + W]); right = np.ascontiguousarray(np.roll(base, -shift, 1)[:, 40:40 + W])
    return left, right


@functools.lru_cache(maxsize=None)
def _expected_cached(seed, H, W, shift, swap, nd, bs, md, uniq, ctype, k):
    a, b = _views(seed, H, W, shift)
    if swap:
        a, b = b, a
    out = bm_census(a, b, nd, bs, md, uniq, k, ctype == SPARSE)
    out.setflags(write=False)
    return out


def _expected(view_key, nd, bs, md=0, uniq=0, ctype=DENSE, k=7, swap=False):
    """The statement's map of the pair _views(*view_key), computed once per configuration and shared."""
    seed, H, W, shift = view_key
    return _expected_cached(seed, H, W, shift, swap, nd, bs, md, uniq, ctype, k)


def _bm(adf, nd, bs, md=0, uniq=0, ctype=DENSE, k=7, cap=31, texthr=0):
    bm = adf.StereoBM.create(nd, bs)
    bm.setMinDisparity(md); bm.setPreFilterCap(cap); bm.setTextureThreshold(texthr); bm.setUniquenessRatio(uniq)
    bm.setCostType(ctype); bm.setCensusSize(k)
    return bm


# ------------------------------------------------------------------------------------------------
# every descriptor, tile and row-group boundaries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype,k", PAIRS)
def test_every_descriptor_bit_exact(adf, ctype, k):
    key = (1, 37, 83, 5)
    got = _bm(adf, 16, 9, ctype=ctype, k=k).compute(*_views(*key))
    exp = _expected(key, 16, 9, ctype=ctype, k=k)
    assert np.array_equal(got, exp)
    inner = exp[4:-4, 19:-4].astype(np.int64)
    assert (inner != -16).all() and (np.abs(inner - 5 * 16) <= 8).mean() > 0.5      # the pair really matches: most pixels find the shift


@pytest.mark.parametrize("ctype,k", PAIRS)
def test_image_narrower_than_a_tile_with_more_padding_than_image_rows(adf, ctype, k):
    """The shared tile load under the pack kernel's coordinates: 40 columns are less than one 64-column tile (every
    tile row ends in clamped columns), and 9 rows are three row groups between six padding groups (most of the tile's
    rows lie above or below the image and are clamped)."""
    key = (365, 9, 40, 3)
    got = _bm(adf, 16, 5, ctype=ctype, k=k).compute(*_views(*key))
    exp = _expected(key, 16, 5, ctype=ctype, k=k)
    assert np.array_equal(got, exp)
    inner = exp[2:-2, 17:-2].astype(np.int64)
    assert (inner != -16).all() and (np.abs(inner - 3 * 16) <= 8).mean() >= 0.5      # not vacuous: the pair matches at its shift


@pytest.mark.parametrize("ctype,k", [(DENSE, 3), (DENSE, 7)])                      # 1 and 6 planes
@pytest.mark.parametrize("H,W,bs", [(21, 330, 5), (22, 330, 21), (70, 150, 9)])
def test_tile_and_row_group_boundaries(adf, H, W, bs, ctype, k):
    """Columns: 330 wide, the matched columns cross the 256 - 2*2 tile at blockSize 5 and the 128 - 2*10 tile at
    blockSize 21.  Rows: 70 rows are 18 row groups, more than one workgroup of four.  (blockSize 21 takes 22 rows: the
    matcher refuses, as it always has, a block that is not smaller than the image -- asserted below at 21 rows.)"""
    key = (H * W + bs, H, W, 7)
    got = _bm(adf, 16, bs, ctype=ctype, k=k).compute(*_views(*key))
    assert np.array_equal(got, _expected(key, 16, bs, ctype=ctype, k=k))


def test_block_as_tall_as_the_image_is_refused_as_with_sad(adf):
    left, right = _views(3, 21, 330, 7)
    for ctype in (SAD, DENSE):
        with pytest.raises(adf.AdfError):
            _bm(adf, 16, 21, ctype=ctype, k=7).compute(left, right)


@pytest.mark.parametrize("bs", [5, 7, 11, 13, 15, 17, 19])
def test_the_other_window_sizes(adf, bs):
    """One instantiation per window half-size: the ones the cases above leave out, three planes."""
    key = (bs, 33, 300, 6)
    got = _bm(adf, 16, bs, ctype=SPARSE, k=9).compute(*_views(*key))
    assert np.array_equal(got, _expected(key, 16, bs, ctype=SPARSE, k=9))


@pytest.mark.parametrize("uniq", [15, 5])
@pytest.mark.parametrize("ctype,k", [(DENSE, 5), (SPARSE, 11)])
def test_uniqueness_instantiation(adf, ctype, k, uniq):
    """Two columns per lane, tile of 128: 200 columns are two tiles."""
    key = (25, 25, 200, 5)
    got = _bm(adf, 32, 9, uniq=uniq, ctype=ctype, k=k).compute(*_views(*key))
    exp = _expected(key, 32, 9, uniq=uniq, ctype=ctype, k=k)
    assert np.array_equal(got, exp)
    inner = exp[4:-4, 35:-4]
    assert (inner == -16).any() and (inner != -16).any()                           # the test rejects some, not all


@pytest.mark.parametrize("md,nd", [(-31, 32), (3, 16)])
def test_disparity_ranges(adf, md, nd):
    key = (7, 30, 140, 4)
    left, right = _views(*key)
    if md < 0:                                                                    # the right-view matcher's range (DF.cpp:424)
        got = _bm(adf, nd, 7, md, ctype=SPARSE, k=7).compute(right, left)
        assert np.array_equal(got, _expected(key, nd, 7, md, ctype=SPARSE, k=7, swap=True))
    else:
        got = _bm(adf, nd, 7, md, ctype=SPARSE, k=7).compute(left, right)
        assert np.array_equal(got, _expected(key, nd, 7, md, ctype=SPARSE, k=7))
    assert (got != (md - 1) * 16).any()


def test_range_that_leaves_no_matched_column(adf):
    left, right = _views(1, 30, 60)
    for md, nd in ((0, 64), (-80, 16)):
        got = _bm(adf, nd, 9, md, ctype=DENSE, k=5).compute(left, right)
        assert (got == (md - 1) * 16).all()
        assert np.array_equal(got, bm_census(left, right, nd, 9, md, 0, 5, False))


@pytest.mark.parametrize("bs", [9, 19])                                           # four and two columns per lane
def test_flat_image_every_pixel_is_a_tie(adf, bs):
    """Every cost is 0: the largest disparity wins everywhere in the valid rectangle, and with the uniqueness test on
    every pixel has a rival at the same cost and is rejected.  Ties are the rule with a Hamming cost."""
    H, W, nd, md = 26, 300, 16, 2
    flat = np.full((H, W), 131, np.uint8)
    w2 = bs // 2
    exp = np.full((H, W), (md - 1) * 16, np.int16)
    exp[w2:H - w2, md + nd - 1 + w2:W - w2] = (md + nd - 1) * 16
    for ctype, k in ((DENSE, 3), (DENSE, 7)):
        assert np.array_equal(_bm(adf, nd, bs, md, ctype=ctype, k=k).compute(flat, flat), exp)
        assert (_bm(adf, nd, bs, md, uniq=10, ctype=ctype, k=k).compute(flat, flat) == (md - 1) * 16).all()
    assert np.array_equal(exp, bm_census(flat, flat, nd, bs, md, 0, 3, False))


# ------------------------------------------------------------------------------------------------
# entries: batch, strides, both views, one handle, graph capture
# ------------------------------------------------------------------------------------------------
def test_batch_with_padded_rows_on_both_entries(adf):
    import torch
    N, H, W, nd, bs = 3, 30, 170, 16, 9
    keys = [(100 + i, H, W, 3 + i) for i in range(N)]
    exp = [_expected(key, nd, bs, ctype=SPARSE, k=7) for key in keys]
    hl = np.zeros((N, H, W + 13), np.uint8); hr = np.zeros((N, H, W + 5), np.uint8)
    for i, key in enumerate(keys):
        hl[i, :, :W], hr[i, :, :W] = _views(*key)
    bm = _bm(adf, nd, bs, ctype=SPARSE, k=7)
    # the device entry
    dl, dr = torch.from_numpy(hl).cuda(), torch.from_numpy(hr).cuda()
    out = torch.full((N, H, W + 6), 777, dtype=torch.int16, device="cuda")
    res = bm.compute(dl[:, :, :W], dr[:, :, :W], out[:, :, :W])
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and (out[:, :, W:] == 777).all()      # nothing written past the row
    for i in range(N):
        assert np.array_equal(out[i, :, :W].cpu().numpy(), exp[i])
    # the host entry
    hout = np.full((N, H, W + 3), 555, np.int16)
    bm.compute(hl[:, :, :W], hr[:, :, :W], hout[:, :, :W])
    assert (hout[:, :, W:] == 555).all()
    for i in range(N):
        assert np.array_equal(hout[i, :, :W], exp[i])


@pytest.mark.parametrize("cap", [31, 63])
def test_both_views_in_one_launch(adf, cap):
    """computeBoth == compute + createRightMatcher(...).compute, whatever preFilterCap is: with a census cost there is no
    prefilter, so the two views always share their descriptor planes and the single launch is always taken."""
    import torch
    key = (41, 45, 330, 6)
    nd, bs, md = 32, 9, 0
    left, right = _views(*key)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    lm = _bm(adf, nd, bs, md, ctype=DENSE, k=5, cap=cap)
    dl, dr = lm.computeBoth(tl, tr)
    assert getattr(lm, "_right", None) is None                                     # not the two-compute detour of a SAD matcher with another cap
    rm = adf.createRightMatcher(lm)
    assert (rm.getCostType(), rm.getCensusSize()) == (DENSE, 5)
    assert torch.equal(dl, lm.compute(tl, tr)) and torch.equal(dr, rm.compute(tr, tl))
    assert np.array_equal(dl.cpu().numpy(), _expected(key, nd, bs, md, ctype=DENSE, k=5))
    assert np.array_equal(dr.cpu().numpy(), _expected(key, nd, bs, -(md + nd) + 1, ctype=DENSE, k=5, swap=True))


def test_one_handle_switches_cost_between_calls(adf, oracle):
    """SAD, census, SAD on ONE handle: the view buffer is sized from the cost of each call (one dword against six per
    row group and column), the SAD maps are the oracle's before and after."""
    key = (77, 37, 140, 6)
    left, right = _views(*key)
    exp_sad = oracle.bm_compute(left, right, 16, 9, 0, 31, 0, 0)
    bm = _bm(adf, 16, 9, ctype=SAD)
    assert np.array_equal(bm.compute(left, right), exp_sad)
    handle = bm._h.value
    bm.setCostType(adf.BM_COST_CENSUS_DENSE); bm.setCensusSize(7)
    exp_census = _expected(key, 16, 9, ctype=DENSE, k=7)
    assert np.array_equal(bm.compute(left, right), exp_census)
    bm.setCostType(adf.BM_COST_SAD)
    assert np.array_equal(bm.compute(left, right), exp_sad)
    assert bm._h.value == handle and not np.array_equal(exp_sad, exp_census)


def test_second_call_is_capturable(adf):
    """Nothing is allocated or synchronised inside compute() once the view buffer exists: a captured call replays."""
    import torch
    key = (8, 30, 120, 6)
    left, right = _views(*key)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    bm = _bm(adf, 16, 7, ctype=SPARSE, k=9)
    eager = bm.compute(tl, tr).clone()
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                      # one linear graph
        bm.compute(tl, tr, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and np.array_equal(eager.cpu().numpy(), _expected(key, 16, 7, ctype=SPARSE, k=9))


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_keep_the_cost(adf):
    from addingdisparityfiltering_amd import _lib
    L = _lib.lib()
    left, right = _views(2, 30, 80)
    bm = _bm(adf, 16, 9, ctype=SPARSE, k=9)
    bm.compute(left, right)                                                        # makes the handle, pushes sparse 9

    def cost():
        c, s = C.c_int(-1), C.c_int(-1)
        _lib.check(L.adf_bm_get_cost(bm._h, C.byref(c), C.byref(s)))
        return c.value, s.value

    assert cost() == (SPARSE, 9)
    for ctype, k in ((DENSE, 9), (SPARSE, 3), (DENSE, 4), (7, 5)):
        assert L.adf_bm_set_cost(bm._h, ctype, k) == _lib.ADF_EBADARG and len(L.adf_last_error()) > 0
        assert cost() == (SPARSE, 9)
        bm.setCostType(ctype); bm.setCensusSize(k)
        with pytest.raises(adf.AdfError) as e:
            bm.compute(left, right)
        assert e.value.code == _lib.ADF_EBADARG
        assert cost() == (SPARSE, 9)
    # the semi-global matcher's constants are the same values and are accepted; SAD ignores the size and keeps it
    _lib.check(L.adf_bm_set_cost(bm._h, adf.SGBM_COST_CENSUS_DENSE, 5))
    assert cost() == (DENSE, 5)
    _lib.check(L.adf_bm_set_cost(bm._h, SAD, 4))
    assert cost() == (SAD, 5)
    h = C.c_void_p()
    _lib.check(L.adf_bm_create(C.byref(h), 16, 9))
    try:
        c, s = C.c_int(-1), C.c_int(-1)
        _lib.check(L.adf_bm_get_cost(h, C.byref(c), C.byref(s)))
        assert (c.value, s.value) == (adf.BM_COST_SAD, 7)                          # a new handle's
    finally:
        L.adf_bm_destroy(h)


def test_cap_and_texture_threshold_are_validated_and_not_used(adf):
    key = (1, 37, 83, 5)
    left, right = _views(*key)
    exp = _expected(key, 16, 9, ctype=DENSE, k=3)
    assert np.array_equal(_bm(adf, 16, 9, ctype=DENSE, k=3, cap=5, texthr=100000).compute(left, right), exp)
    with pytest.raises(adf.AdfError):
        _bm(adf, 16, 9, ctype=DENSE, k=3, cap=64).compute(left, right)
    with pytest.raises(adf.AdfError):
        _bm(adf, 16, 9, ctype=DENSE, k=3, texthr=-1).compute(left, right)


# ------------------------------------------------------------------------------------------------
# the reference's fixture, and the filter behind the matcher
# ------------------------------------------------------------------------------------------------
def test_tsukuba_on_the_device_equals_the_statement(adf):
    left, right, gt = load_tsukuba()
    got = _bm(adf, 16, 9, ctype=DENSE, k=7).compute(left, right)
    exp = bm_census(left, right, 16, 9, 0, 0, 7, False)
    assert np.array_equal(got, exp)
    err = error_level(gt, got)
    print("census dense 7 block 9 on the device: error %.2f %%" % err)
    assert err == error_level(gt, exp) and err <= 20.0                             # test_block_matching.cpp:148


def test_filter_run_on_census_maps(adf):
    """createDisparityWLSFilter(bm) on a 64 x 160 crop of the Tsukuba pair with the census maps of computeBoth: the maps
    are the statement's, and the filter's output is bit-equal to what it gives from the statement's maps -- the cost
    changes nothing downstream."""
    import torch
    left, right, _ = load_tsukuba()
    left = np.ascontiguousarray(left[100:164, 120:280]); right = np.ascontiguousarray(right[100:164, 120:280])
    nd, bs = 16, 9
    lm = adf.StereoBM.create(nd, bs)
    lm.setCostType(adf.BM_COST_CENSUS_SPARSE); lm.setCensusSize(9)
    wls = adf.createDisparityWLSFilter(lm)                                          # forces textureThreshold = uniquenessRatio = 0
    assert (lm.getCostType(), lm.getCensusSize(), lm.getUniquenessRatio()) == (adf.BM_COST_CENSUS_SPARSE, 9, 0)
    wls.setLambda(8000.0); wls.setSigmaColor(1.5)
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    dl, dr = lm.computeBoth(tl, tr)
    out = wls.filter(dl, tl, None, dr).clone()
    conf = wls.getConfidenceMap().clone()
    edl = bm_census(left, right, nd, bs, 0, 0, 9, True)
    edr = bm_census(right, left, nd, bs, -nd + 1, 0, 9, True)
    assert np.array_equal(dl.cpu().numpy(), edl) and np.array_equal(dr.cpu().numpy(), edr)
    assert (edl[4:-4, nd + 3:-4] >= 0).mean() > 0.8                                 # the crop really matches
    ref = wls.filter(torch.from_numpy(edl).cuda(), tl, None, torch.from_numpy(edr).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(conf, wls.getConfidenceMap())
    assert wls.getROI() == (nd + 4, 4, 160 - (nd + 4) - 4, 64 - 8)                  # DF.cpp:401: the SAD matcher's
