"""GPU tests of the block matcher's winning-cost plane (csrc/bm_matcher.hip: the cost store of bm_match_kernel and
bm_border_kernel; include/adf_wls.h: adf_bm_compute_cost_*) and of the chain built on it (StereoBM.computeFull).

Integer work: every plane is compared bit for bit with the direct statement tests/validate_ref.py.  Views 300 x 23 and
97 x 22: 300 matched columns cross the wave tile of both columns-per-lane layouts (256 - 2*w2 and 128 - 2*w2), 23 and 22
rows are six row groups with a partial last one and just admit blockSize 21."""
import functools

import numpy as np
import pytest

from test_oracle_bm import load_tsukuba
from test_speckle_ref import speckle_ref
from validate_ref import SAD, block_costs, bm_winner_cost, resolve, truncate16, validate_disparity

pytestmark = pytest.mark.gpu

DENSE, SPARSE, MCT_DENSE, CS = 1, 2, 4, 6
# (cost type, census size, preFilterCap)
COSTS = [(SAD, 7, 31), (SAD, 7, 63), (DENSE, 7, 31), (SPARSE, 5, 31), (MCT_DENSE, 5, 31), (CS, 9, 31)]
VIEWS = [(300, 23), (97, 22)]


def _dev():
    import torch

    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _views(W, H, shift=5):
    rng = np.random.default_rng(W * 100 + H)
    base = rng.integers(0, 256, (H, W + 96), dtype=np.uint8)
    base = (base // 2 + np.roll(base, 1, 1) // 4 + np.roll(base, 1, 0) // 4).astype(np.uint8)
    base[H // 4:H // 2 + 4, 60:60 + W // 4] = 90                                     # a flat patch: the texture test and ties
    rep = (40 + 150 * ((np.arange(W // 4) // 3) % 2)).astype(np.uint8)               # a repetitive patch: the uniqueness test
    base[H // 2:, 50 + W // 2:50 + W // 2 + W // 4] = rep
    left = np.ascontiguousarray(base[:, 40:40 + W])
    right = np.ascontiguousarray(np.roll(base, -shift, 1)[:, 40:40 + W])
    left.setflags(write=False); right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def _costs(W, H, nd, bs, md, cap, ctype, k):
    """block_costs of the pair, computed once per configuration and shared by its uniqueness and texture settings."""
    return block_costs(*_views(W, H), nd, bs, md, cap, ctype, k)


def _expected(W, H, nd, bs, md, cap, texthr, uniq, ctype, k):
    return resolve(_costs(W, H, nd, bs, md, cap, ctype, k), (H, W), nd, bs, md, 0 if ctype != SAD else texthr, uniq)


def _bm(adf, nd, bs, md=0, cap=31, texthr=0, uniq=0, ctype=SAD, k=7):
    bm = adf.StereoBM.create(nd, bs)
    bm.setMinDisparity(md); bm.setPreFilterCap(cap); bm.setTextureThreshold(texthr); bm.setUniquenessRatio(uniq)
    bm.setCostType(ctype); bm.setCensusSize(k)
    return bm


def _t(a):
    import torch

    return torch.from_numpy(np.array(a)).to(_dev())                 # (a copy: the cached views are read-only)


@pytest.mark.parametrize("ctype,k,cap", COSTS)
@pytest.mark.parametrize("md", [0, -5])
@pytest.mark.parametrize("bs", [5, 9, 21])
@pytest.mark.parametrize("nd", [16, 32])
@pytest.mark.parametrize("W,H", VIEWS)
def test_cost_plane_bit_exact(adf, W, H, nd, bs, md, ctype, k, cap):
    left, right = _views(W, H)
    tl, tr = _t(left), _t(right)
    seen_filtered = seen_kept = 0
    for uniq in (0, 15):
        for texthr in (0, 10):
            bm = _bm(adf, nd, bs, md, cap, texthr, uniq, ctype, k)
            plain = bm.compute(tl, tr).cpu().numpy()
            disp, cost = bm.computeWithCost(tl, tr)
            disp, cost = disp.cpu().numpy(), cost.cpu().numpy()
            assert disp.tobytes() == plain.tobytes(), "computeWithCost's map differs from compute()'s"
            exp_disp, cost32, cost16 = _expected(W, H, nd, bs, md, cap, texthr, uniq, ctype, k)
            assert np.array_equal(disp, exp_disp)
            inv = (md - 1) * 16
            kept = disp != inv
            assert np.array_equal(cost[kept], truncate16(cost32)[kept]), (uniq, texthr)
            assert (cost[~kept] == 0).all(), "a filtered pixel's cost is not 0"
            assert np.array_equal(cost, cost16)
            seen_filtered += int((~kept[bs // 2:H - bs // 2, max(md + nd - 1, 0) + bs // 2:W + min(md, 0) - bs // 2]).sum())
            seen_kept += int(kept.sum())
    assert seen_kept > 0
    if ctype == SAD and bs < 21:       # (a 21-row window covers the whole height of these views: no window lies in a patch)
        assert seen_filtered > 0, "no test rejected a pixel inside the valid rectangle"


@pytest.mark.parametrize("W,H", VIEWS)
def test_host_entry_and_batch_equal_the_device_entry(adf, W, H):
    left, right = _views(W, H)
    bm = _bm(adf, 16, 9, -5, 31, 10, 15)
    d0, c0 = bm.computeWithCost(_t(left), _t(right))
    dh, ch = bm.computeWithCost(left, right)
    assert isinstance(dh, np.ndarray) and np.array_equal(dh, d0.cpu().numpy()) and np.array_equal(ch, c0.cpu().numpy())
    # a batch of three (the pair, the pair swapped, the pair) into caller-provided planes with padded rows
    import torch

    L, R = np.stack([left, right, left]), np.stack([right, left, right])
    dfull = torch.full((3, H + 1, W + 6), 1234, dtype=torch.int16, device=_dev())
    cfull = torch.full((3, H + 2, W + 2), 4321, dtype=torch.int16, device=_dev())
    db, cb = bm.computeWithCost(_t(L), _t(R), dfull[:, :H, :W], cfull[:, :H, :W])
    assert db.data_ptr() == dfull.data_ptr() and cb.data_ptr() == cfull.data_ptr()
    d1, c1 = bm.computeWithCost(_t(right), _t(left))
    for i, (d, c) in enumerate(((d0, c0), (d1, c1), (d0, c0))):
        assert np.array_equal(dfull[i, :H, :W].cpu().numpy(), d.cpu().numpy()), i
        assert np.array_equal(cfull[i, :H, :W].cpu().numpy(), c.cpu().numpy()), i
    assert (dfull[:, H:, :] == 1234).all() and (dfull[:, :, W:] == 1234).all()
    assert (cfull[:, H:, :] == 4321).all() and (cfull[:, :, W:] == 4321).all(), "the cost plane's padding was written"


@pytest.mark.parametrize("ctype,k,cap", [(SAD, 7, 31), (SAD, 7, 63), (DENSE, 7, 31), (SPARSE, 5, 31)])
@pytest.mark.parametrize("bs,uniq", [(5, 0), (9, 15), (21, 0), (21, 15)])
@pytest.mark.parametrize("W,H", VIEWS)
def test_compute_both_with_cost_equals_the_two_separate_computes(adf, W, H, bs, uniq, ctype, k, cap):
    left, right = _views(W, H)
    tl, tr = _t(left), _t(right)
    for nd, md in ((16, 0), (32, -5)):
        bm = _bm(adf, nd, bs, md, cap, 10, uniq, ctype, k)
        dl, dr, cl, cr = (t.cpu().numpy() for t in bm.computeBothWithCost(tl, tr))
        el, ecl = (t.cpu().numpy() for t in bm.computeWithCost(tl, tr))
        er, ecr = (t.cpu().numpy() for t in adf.createRightMatcher(bm).computeWithCost(tr, tl))
        assert np.array_equal(dl, el) and np.array_equal(cl, ecl)
        assert np.array_equal(dr, er) and np.array_equal(cr, ecr)
        pl, pr = bm.computeBoth(tl, tr)
        assert np.array_equal(dl, pl.cpu().numpy()) and np.array_equal(dr, pr.cpu().numpy())
        # the right view against the statement: views swapped, minDisparity = -(md + nd) + 1, both tests off, cap 31
        # (createRightMatcher keeps cv::StereoBM's default cap)
        rcap = 31 if ctype == SAD else cap
        exp_r, _, exp_cr = bm_winner_cost(right, left, nd, bs, -(md + nd) + 1, rcap, 0, 0, ctype, k)
        assert np.array_equal(dr, exp_r) and np.array_equal(cr, exp_cr)
        assert (dr != (-(md + nd)) * 16).any()


def test_truncation_wraps_a_cost_above_32767(adf):
    """Left view a rising ramp, right view a falling one, 8 grey levels per column: the x-Sobel response is +-64,
    clipped to cap 63, so the prefiltered views hold 126 and 0 and a 21 x 21 SAD is 126 * 441 = 55566.  An 8-bit ramp that
    steep spans 32 columns, fewer than blockSize 21 plus 16 disparities need, so the ramp is a sawtooth of period 32; the two
    columns at each wrap hold the opposite extreme, which lowers the SAD of windows that contain them (every winner's: some
    disparity always reaches a wrap) to no less than 17 / 21 of the full value -- still above 32767 everywhere."""
    W, H, nd, bs = 97, 23, 16, 21
    ramp = ((8 * np.arange(W)) % 256).astype(np.uint8)
    left = np.tile(ramp, (H, 1))
    right = np.tile((248 - ramp).astype(np.uint8), (H, 1))
    exp_disp, cost32, cost16 = bm_winner_cost(left, right, nd, bs, 0, 63, 0, 0)
    kept = exp_disp != -16
    assert kept.any() and (cost32[kept] > 32767).all()
    assert block_costs(left, right, nd, bs, 0, 63)[0].max() == 126 * 441         # a window clear of the wraps
    assert cost32[kept].min() >= 126 * 441 * 17 // 21
    assert (cost16[kept] < 0).all()                                              # 55566 - 65536
    bm = _bm(adf, nd, bs, 0, 63, 0, 0)
    disp, cost = (t.cpu().numpy() for t in bm.computeWithCost(_t(left), _t(right)))
    assert np.array_equal(disp, exp_disp)
    assert np.array_equal(cost, cost16)
    assert np.array_equal(cost[kept].astype(np.int64) & 0xFFFF, cost32[kept].astype(np.int64) & 0xFFFF)


# ------------------------------------------------------------------------------------------------
# the chain on the stereo_* pair
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tsukuba_reference(nd, bs, maxdiff):
    left, right, gt = load_tsukuba()
    disp, _, cost16 = bm_winner_cost(left, right, nd, bs, 0, 31, 10, 15)
    valid, outside = validate_disparity(disp, cost16, 0, nd, maxdiff)
    assert outside == 0
    return left, right, gt, disp, cost16, valid


def bad_share(gt, disp16, inv=-16):
    """Share (%) of surviving pixels (map != inv, ground truth known) that are off by more than two disparity levels,
    on the 8-bit maps of disparity * 16 that test_oracle_bm.error_level compares."""
    alive = (disp16 != inv) & (gt != 0)
    out8 = np.clip(disp16, 0, 255).astype(np.int64)
    return 100.0 * ((np.abs(gt.astype(np.int64) - out8) > 2 * 16) & alive).sum() / alive.sum()


def test_validation_does_not_raise_the_bad_pixel_share():
    """The reference alone, on the CPU, StereoBM(16, 9) with cv's defaults: 4.45 % of 79086 surviving pixels are bad
    before validateDisparity at disp12MaxDiff = 1, 4.00 % of 78503 after.  The reference shows the
    share not rising, so the device map is gated on after <= before."""
    _, _, gt, disp, _, valid = _tsukuba_reference(16, 9, 1)
    before, after = bad_share(gt, disp), bad_share(gt, valid)
    print("bad-pixel share among surviving pixels: before %.2f %% of %d, after %.2f %% of %d"
          % (before, (disp != -16).sum(), after, (valid != -16).sum()))
    assert after <= before and (valid != disp).any()


def test_validated_device_map_is_no_worse_than_the_unvalidated_one(adf):
    left, right, gt, ref_disp, ref_cost, ref_valid = _tsukuba_reference(16, 9, 1)
    bm = adf.StereoBM.create(16, 9)
    disp, cost = bm.computeWithCost(_t(left), _t(right))
    raw = disp.cpu().numpy()
    assert np.array_equal(raw, ref_disp) and np.array_equal(cost.cpu().numpy(), ref_cost)
    adf.validateDisparity(disp, cost, 0, 16, 1)
    got = disp.cpu().numpy()
    assert np.array_equal(got, ref_valid)
    assert bad_share(gt, got) <= bad_share(gt, raw)


@pytest.mark.parametrize("maxdiff,window,srange", [(1, 100, 32), (-1, 100, 32), (1, 0, 0), (0, 50, 2), (1000000, 100, 32)])
def test_compute_full_equals_the_reference_chain(adf, maxdiff, window, srange):
    """The canonical sample's settings (disp12MaxDiff 1, speckleWindowSize 100, speckleRange 32) and each stage off."""
    left, right, _, ref_disp, ref_cost, _ = _tsukuba_reference(16, 9, 1)
    exp = ref_disp
    if maxdiff >= 0:
        exp, _ = validate_disparity(exp, ref_cost, 0, 16, maxdiff)
    if window > 0:
        exp = speckle_ref(exp, -16, window, srange)              # the range unscaled (stereo_binary_bm.cpp:416-417)
    bm = adf.StereoBM.create(16, 9)
    bm.setDisp12MaxDiff(maxdiff); bm.setSpeckleWindowSize(window); bm.setSpeckleRange(srange)
    assert bm.getSpeckleRange() == srange
    got = bm.computeFull(_t(left), _t(right))
    assert np.array_equal(got.cpu().numpy(), exp)
    assert np.array_equal(bm.computeFull(left, right), exp)       # host arrays: the host entries all the way
    if 0 <= maxdiff < 1000000 or window > 0:
        with pytest.raises(adf.AdfError):                        # compute() keeps refusing what computeFull runs
            bm.compute(_t(left), _t(right))


def test_sgbm_compute_full_is_compute_then_speckles(adf):
    left, right, _ = load_tsukuba()
    sg = adf.StereoSGBM.create(0, 16, 3, 24 * 9, 96 * 9, 1, 63, 10, 0, 0, adf.StereoSGBM.MODE_SGBM_3WAY)
    assert sg.getSpeckleRange() == 0
    raw = sg.compute(_t(left), _t(right)).cpu().numpy()
    assert np.array_equal(sg.computeFull(_t(left), _t(right)).cpu().numpy(), raw)   # speckleWindowSize 0: compute() alone
    sg.setSpeckleWindowSize(100); sg.setSpeckleRange(2)
    exp = speckle_ref(raw, -16, 100, 16 * 2)                     # 16 * speckleRange (stereo_binary_sgbm.cpp:716-718)
    got = sg.computeFull(_t(left), _t(right)).cpu().numpy()
    assert np.array_equal(got, exp) and (exp != raw).any()
    with pytest.raises(adf.AdfError):
        sg.compute(_t(left), _t(right))
