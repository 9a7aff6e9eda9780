"""StereoSGBM.computeBoth on the device (include/adf_wls.h: adf_sgbm_compute_both_*), bit for bit against the direct
statement tests/sgbm_both_ref.py.  Small images throughout: the statement is numpy over the whole volume, and these are
the shapes at which the winner pass's right-view part can go wrong -- every disparities-per-lane instantiation, rows
shorter than the prefetch ring, every shape of the disparity range, partial candidate ranges at both image borders."""
import numpy as np
import pytest

import sgbm_both_ref as ref
from test_gpu_real_guides import MAX_DIF, MAX_MEAN_DIF
from test_gpu_sgbm_full import tiled_pair
from test_oracle_sgbm import _pair, naive_median3

pytestmark = pytest.mark.gpu

OFF = 1000000


def _matcher(adf, nd, bs=3, md=0, P1=None, P2=None, cap=63, ur=0, mode=2, disp12=OFF, cost=0, k=7):
    m = adf.StereoSGBM.create(md, nd, bs)
    m.setP1(24 * bs * bs if P1 is None else P1); m.setP2(96 * bs * bs if P2 is None else P2)
    m.setPreFilterCap(cap); m.setUniquenessRatio(ur); m.setMode(mode); m.setDisp12MaxDiff(disp12)
    m.setCostType(cost); m.setCensusSize(k)
    return m


def _statement(oracle, a, b, nd, bs=3, md=0, P1=None, P2=None, cap=63, ur=0, mode=2, disp12=OFF, cost=0, k=7):
    return ref.both_maps(oracle, a, b, nd, bs, md, 24 * bs * bs if P1 is None else P1, 96 * bs * bs if P2 is None else P2,
                         cap, ur, mode, disp12, cost, k)[2:]


def _volume_case(adf, oracle, a, b, nd, **prm):
    """computeBoth(VOLUME) on device tensors: both maps against the statement, the left one against compute() too."""
    import torch
    m = _matcher(adf, nd, **prm)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dl, dr = m.computeBoth(ta, tb, rightSource=adf.SGBM_RIGHT_FROM_VOLUME)
    one = m.compute(ta, tb)
    torch.cuda.synchronize()
    el, er = _statement(oracle, a, b, nd, **prm)
    dl, dr = dl.cpu().numpy(), dr.cpu().numpy()
    assert np.array_equal(dl, one.cpu().numpy()), "the left map differs from compute()'s"
    assert np.array_equal(dl, el), "the left map differs from the statement"
    assert np.array_equal(dr, er), "the right map differs from the statement"
    return dl, dr


@pytest.mark.parametrize("nd", [16, 64, 128, 256, 512])
def test_every_disparities_per_lane_instantiation(adf, oracle, nd):
    """1, 2, 4 and 8 disparities per lane (16: lanes without disparities); 9 rows are no multiple of a workgroup's four."""
    a, b = _pair(nd, 9, nd + 37, shift=5)
    dl, dr = _volume_case(adf, oracle, a, b, nd)
    assert (dr[:, 1:] != -nd * 16).mean() > 0.9               # partial ranges count: columns 1 ... W-1 have winners


@pytest.mark.parametrize("nd", [48, 80, 272])
def test_disparity_counts_below_the_ring_size(adf, oracle, nd):
    """Counts that are no power of two: the ring of live right columns is larger than numDisparities."""
    a, b = _pair(nd + 1, 6, nd + 41, shift=7)
    _volume_case(adf, oracle, a, b, nd)


@pytest.mark.parametrize("w1", [1, 2, 5, 0, -3])
def test_rows_shorter_than_the_prefetch_ring(adf, oracle, w1):
    nd = 16
    a, b = _pair(30 + w1, 7, nd + w1, shift=2)
    dl, dr = _volume_case(adf, oracle, a, b, nd)
    if w1 <= 0:
        assert (dl == -16).all() and (dr == -nd * 16).all()   # both maps entirely invalid


@pytest.mark.parametrize("md", [0, -5, -31, 3])
def test_every_shape_of_the_disparity_range(adf, oracle, md):
    """0; a range straddling zero; the right matcher's own range 1 - nd; a positive minimum."""
    a, b = _pair(50 + md, 10, 80, shift=4)
    dl, dr = _volume_case(adf, oracle, a, b, 32, md=md)
    assert (dr <= -md * 16).all() and (dr >= -(md + 32) * 16).all()


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_every_mode(adf, oracle, mode):
    a, b = _pair(60 + mode, 11, 60, shift=3)
    _volume_case(adf, oracle, a, b, 16, mode=mode)


@pytest.mark.parametrize("bs", [1, 3, 7])
@pytest.mark.parametrize("cost,k,cn,P1,P2", [(0, 7, 1, None, None), (0, 7, 3, None, None), (1, 5, 1, 20, 80), (6, 7, 1, 20, 80)])
def test_every_cost_and_block_size(adf, oracle, cost, k, cn, P1, P2, bs):
    """Birchfield-Tomasi on one and three channels, census dense 5, centre-symmetric census 7."""
    a, b = _pair(70 + bs + cost + cn, 8, 55, cn, shift=4)
    _volume_case(adf, oracle, a, b, 16, bs=bs, cost=cost, k=k, P1=P1, P2=P2)


def test_flat_image_every_cost_ties(adf, oracle):
    """A census cost on a flat image: every cost is 0, every candidate ties, and the right map is each column's largest
    available k (no fit: it is nd-1, or its upper neighbour is no candidate)."""
    H, W, nd = 6, 50, 16
    a = np.full((H, W), 90, np.uint8)
    dl, dr = _volume_case(adf, oracle, a, a.copy(), nd, cost=1, k=5, P1=20, P2=80)
    raw = np.full((H, W), -nd * 16, np.int64)
    xr = np.arange(1, W)
    raw[:, 1:] = -16 * np.minimum(nd - 1, W - 1 - xr)
    assert np.array_equal(dr, naive_median3(raw))


@pytest.mark.parametrize("ur,disp12", [(15, OFF), (0, 1), (0, 0), (15, 1)])
def test_uniqueness_and_left_right_check_touch_the_left_map_only(adf, oracle, ur, disp12):
    import torch
    a, b = _pair(90, 12, 90, shift=6)
    dl, dr = _volume_case(adf, oracle, a, b, 32, ur=ur, disp12=disp12)
    plain = _matcher(adf, 32).computeBoth(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), rightSource=adf.SGBM_RIGHT_FROM_VOLUME)
    assert np.array_equal(dr, plain[1].cpu().numpy())         # the right map is unaffected by either


def _padded_batch(m, source, expect):
    """A batch of 3 with padded row and pair strides on all four planes; the bytes outside the maps stay untouched."""
    import torch
    N, H, W = 3, 12, 70
    pairs = [_pair(300 + i, H, W, shift=3 + i) for i in range(N)]
    bl = torch.zeros((N, H + 2, W + 5), dtype=torch.uint8, device="cuda"); br = torch.zeros((N, H + 1, W + 9), dtype=torch.uint8, device="cuda")
    for i, (l, r) in enumerate(pairs):
        bl[i, :H, :W] = torch.from_numpy(l).cuda(); br[i, :H, :W] = torch.from_numpy(r).cuda()
    ol = torch.full((N, H + 1, W + 3), 777, dtype=torch.int16, device="cuda")
    orr = torch.full((N, H + 3, W + 7), -555, dtype=torch.int16, device="cuda")
    rl, rr = m.computeBoth(bl[:, :H, :W], br[:, :H, :W], ol[:, :H, :W], orr[:, :H, :W], rightSource=source)
    torch.cuda.synchronize()
    assert rl.data_ptr() == ol.data_ptr() and rr.data_ptr() == orr.data_ptr()
    assert (ol[:, :, W:] == 777).all() and (ol[:, H:] == 777).all() and (orr[:, :, W:] == -555).all() and (orr[:, H:] == -555).all()
    for i, (l, r) in enumerate(pairs):
        el, er = expect(l, r)
        assert np.array_equal(ol[i, :H, :W].cpu().numpy(), el), i
        assert np.array_equal(orr[i, :H, :W].cpu().numpy(), er), i


def _matcher_maps(oracle, nd):
    return lambda l, r: (oracle.sgbm_compute(l, r, nd, 3, 0, 216, 864, 63, 0), oracle.sgbm_compute(r, l, nd, 3, 1 - nd, 216, 864, 63, 0))


def test_padded_batch(adf, oracle):
    nd = 16
    _padded_batch(_matcher(adf, nd), adf.SGBM_RIGHT_FROM_VOLUME, lambda l, r: _statement(oracle, l, r, nd))
    _padded_batch(_matcher(adf, nd), adf.SGBM_RIGHT_MATCHER, _matcher_maps(oracle, nd))


def test_padded_batch_in_chunks(adf, oracle, monkeypatch):
    """The same batch under a workspace limit that holds two images in flight and a half (ADF_WS_LIMIT_GB is read when
    the handle is created): chunks of 2 + 1."""
    nd, H, W = 16, 12, 70
    pad = lambda v: -(-v // 256) * 256
    per_image = 2 * pad(H * W * 12) + 3 * pad(H * (W - nd) * nd * 2) + 2 * pad(H * W * 2)      # include/adf_wls.h: workspace per image in flight
    monkeypatch.setenv("ADF_WS_LIMIT_GB", repr(2.5 * per_image / 2.0 ** 30))
    _padded_batch(_matcher(adf, nd), adf.SGBM_RIGHT_FROM_VOLUME, lambda l, r: _statement(oracle, l, r, nd))
    _padded_batch(_matcher(adf, nd), adf.SGBM_RIGHT_MATCHER, _matcher_maps(oracle, nd))


@pytest.mark.parametrize("md,ur,disp12,cost", [(0, 0, OFF, 0), (-4, 10, 1, 0), (2, 0, OFF, 1)])
def test_right_matcher_source_equals_the_two_computes(adf, md, ur, disp12, cost):
    import torch
    a, b = _pair(120 + md, 13, 85, shift=5)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = _matcher(adf, 32, md=md, ur=ur, disp12=disp12, cost=cost, k=5, P1=30, P2=120)
    dl, dr = m.computeBoth(ta, tb)                            # the default source is the matcher's
    el = m.compute(ta, tb)
    rm = adf.createRightMatcher(m)
    er = rm.compute(tb, ta)
    again = m.compute(ta, tb)                                 # the handle is the left matcher again
    torch.cuda.synchronize()
    assert (rm.getMinDisparity(), rm.getUniquenessRatio(), rm.getDisp12MaxDiff()) == (1 - md - 32, 0, OFF)
    assert torch.equal(dl, el) and torch.equal(dr, er) and torch.equal(again, el)
    assert not torch.equal(dr, m.computeBoth(ta, tb, rightSource=adf.SGBM_RIGHT_FROM_VOLUME)[1])   # a different map by definition


@pytest.mark.parametrize("source", [0, 1])
def test_host_entry_equals_the_device_entry(adf, source):
    import torch
    N, H, W, nd = 2, 10, 66, 16
    pairs = [_pair(140 + i, H, W, 3, shift=4) for i in range(N)]
    L = np.stack([p[0] for p in pairs]); R = np.stack([p[1] for p in pairs])
    m = _matcher(adf, nd, disp12=1)
    hl = np.full((N, H, W + 4), 99, np.int16); hr = np.full((N, H + 2, W), 98, np.int16)
    m.computeBoth(L, R, hl[:, :, :W], hr[:, :H], rightSource=source)
    dl, dr = m.computeBoth(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), rightSource=source)
    assert np.array_equal(hl[:, :, :W], dl.cpu().numpy()) and np.array_equal(hr[:, :H], dr.cpu().numpy())
    assert (hl[:, :, W:] == 99).all() and (hr[:, H:] == 98).all()
    one = m.computeBoth(L[1], R[1], rightSource=source)       # an unbatched colour pair on the host
    assert np.array_equal(one[0], hl[1, :, :W]) and np.array_equal(one[1], hr[1, :H])


def test_the_lds_limit_is_refused_and_the_widest_call_runs(adf, oracle):
    """include/adf_wls.h: 8576 columns, 4288 with the matcher's own left-right check.  One column more is ADF_ESIZE with
    the limits in the message and nothing launched; 4288 columns with the check on take 134.5 KiB of LDS and run."""
    import torch
    from addingdisparityfiltering_amd._lib import ADF_ESIZE
    msg = ("adf error %d: ADF_SGBM_RIGHT_FROM_VOLUME supports images up to 8576 columns (4288 with the matcher's own "
           "left-right check, disp12MaxDiff)" % ADF_ESIZE)
    for W, disp12 in ((4289, 1), (8577, OFF)):
        v = torch.zeros((2, W), dtype=torch.uint8, device="cuda")
        ol = torch.full((2, W), 777, dtype=torch.int16, device="cuda"); orr = torch.full((2, W), -555, dtype=torch.int16, device="cuda")
        m = _matcher(adf, 16, disp12=disp12)
        with pytest.raises(adf.AdfError) as e:
            m.computeBoth(v, v, ol, orr, rightSource=adf.SGBM_RIGHT_FROM_VOLUME)
        assert e.value.code == ADF_ESIZE and str(e.value) == msg
        torch.cuda.synchronize()
        assert (ol == 777).all() and (orr == -555).all()
        m.computeBoth(v, v, ol, orr)                          # the matcher's map has no such limit
        torch.cuda.synchronize()
        assert (ol != 777).all() and (orr != -555).all()
    a, b = _pair(160, 5, 4288, shift=8)
    _volume_case(adf, oracle, a, b, 16, disp12=1)


def test_overlapping_maps_and_a_missing_map_are_refused(adf):
    import torch
    from addingdisparityfiltering_amd import _lib
    H, W = 6, 40
    v = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    buf = torch.zeros((2 * H, W), dtype=torch.int16, device="cuda")
    m = _matcher(adf, 16)
    for source in (0, 1):
        with pytest.raises(adf.AdfError) as e:
            m.computeBoth(v, v, buf[:H], buf[H - 1:2 * H - 1], rightSource=source)
        assert e.value.code == _lib.ADF_EBADARG and str(e.value) == "adf error %d: the two disparity maps must not overlap" % _lib.ADF_EBADARG
        m.computeBoth(v, v, buf[:H], buf[H:], rightSource=source)         # adjacent is fine
    lib = _lib.lib()
    args = (m._h, 1, v.data_ptr(), W, 0, v.data_ptr(), W, 0, 1, W, H, buf.data_ptr(), 2 * W, 0)
    assert lib.adf_sgbm_compute_both_device(*args, None, 2 * W, 0, 1, None) == _lib.ADF_EBADARG
    assert lib.adf_last_error() == b"views and disparity must be non-NULL, n_pairs positive"
    assert lib.adf_sgbm_compute_both_device(*args, buf[H:].data_ptr(), 2 * W, 0, 2, None) == _lib.ADF_EBADARG     # unknown source
    assert lib.adf_last_error() == b"right_source must be ADF_SGBM_RIGHT_MATCHER or ADF_SGBM_RIGHT_FROM_VOLUME"
    assert lib.adf_sgbm_compute_both_device(*args, buf[H:].data_ptr() + 1, 2 * W, 0, 1, None) == _lib.ADF_ESIZE
    assert lib.adf_sgbm_compute_both_device(*args, buf[H:].data_ptr(), 2 * W - 2, 0, 1, None) == _lib.ADF_ESIZE
    assert lib.adf_sgbm_compute_both_device(*args, buf[H:].data_ptr(), 2 * W, 0, 1, None) == _lib.ADF_OK
    torch.cuda.synchronize()


def test_640x480_through_the_filter(adf, oracle):
    """BASELINE config 1's shape on the KITTI-shaped fixture, tiled: computeBoth(VOLUME) against the statement, then its
    two maps through the filter set up from the matcher, on both solvers, against the oracle's filter fed with the
    statement's maps."""
    import torch
    H, W, nd = 480, 640, 64
    L, R = tiled_pair(H, W)
    lm = _matcher(adf, nd, disp12=0)
    wls = adf.createDisparityWLSFilter(lm)                    # (switches the matcher's own left-right check off)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    dl, dr = lm.computeBoth(tl, tr, rightSource=adf.SGBM_RIGHT_FROM_VOLUME)
    torch.cuda.synchronize()
    el, er = _statement(oracle, L, R, nd)
    assert np.array_equal(dl.cpu().numpy(), el) and np.array_equal(dr.cpu().numpy(), er)
    assert (el[:, nd:] >= 0).mean() > 0.8 and (er[:, 1:W - nd] > -nd * 16).mean() > 0.8      # the pair really matches; the right map is no map of invalid values
    wls.setLambda(8000.0); wls.setSigmaColor(1.5)
    p = oracle.default_params(threads=8, use_confidence=1, disc_radius=2, sigma_color=1.5)
    p.lambda_ = 8000.0
    roi = (nd, 0, W - nd, H)
    exp, exp_conf = oracle.wls_filter(el, L, er, roi, p)
    for solver in (adf.SOLVER_EXACT, adf.SOLVER_WAVE):
        wls.setSolver(solver)
        out = wls.filter(dl, tl, None, dr)
        torch.cuda.synchronize()
        assert wls.getROI() == roi and wls.getLastSolver() == solver
        assert np.array_equal(wls.getConfidenceMap().cpu().numpy(), exp_conf)
        d = np.abs(out.cpu().numpy().astype(np.int64) - exp.astype(np.int64))
        if solver == adf.SOLVER_EXACT:
            assert d.max() == 0
        else:
            assert d.max() <= MAX_DIF and d.mean() <= MAX_MEAN_DIF, (d.max(), d.mean())
    assert (exp_conf > 0).mean() > 0.2 and (exp[:, nd:] != el[:, nd:]).mean() > 0.3      # the filter had work to do
