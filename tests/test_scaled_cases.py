"""CPU checks of the inputs in tests/scaled_cases.py, on the oracle alone: the plateau maps are not a vacuous probe
at any case (confidence positive where the values are extreme, and the second saturate_cast of DF.cpp:273 at work on a
good share of those pixels, with unclamped values beside them), every fuzz seed is a call the oracle accepts, and the
directed case for the float product of DF.cpp:318 tells the two products apart."""
import numpy as np
import pytest

import scaled_cases as sc


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_plateau_maps_are_not_vacuous(oracle, c):
    view, dl, dr = sc.case_inputs(c)
    p = oracle.default_params(sigma_color=1.5, threads=4, disc_radius=c.radius)
    out, conf = oracle.wls_filter_scaled(dl, view, dr, c.roi, p)
    roi = sc.inside(conf.shape, sc.hi_roi(c.roi, c.view, c.maps))
    pos = (conf > 0) & roi
    share = pos.sum() / roi.sum()
    assert share >= 0.4, "confidence > 0 on %.2f of the ROI" % share                      # condition 1
    assert np.all(out[~roi] == -16)
    if c.maps[0] < c.view[0]:                                                            # condition 2
        # the first saturate_cast's result times x_ratio, before the second one
        r = oracle.resize_linear(dl, c.view).astype(np.float64) * float(sc.x_ratio(c.view, c.maps))
        sat = (np.abs(r) > 32767.5)[pos].mean()
        assert 0.2 <= sat <= 0.8, "saturating share %.3f" % sat
        hi = oracle.resize_linear(dl, c.view, post_scale=float(sc.x_ratio(c.view, c.maps)))
        assert (hi[pos] == 32767).any() and (hi[pos] == -32768).any()                   # both clamp directions
    else:
        r = oracle.resize_linear(dl, c.view).astype(np.float64) * float(sc.x_ratio(c.view, c.maps))
        assert np.abs(r).max() <= 32767.5                                                # a reduction cannot saturate


def test_limit_maps_hit_every_value():
    dl = sc.limits(np.random.default_rng(0), 24, 32)
    assert set(np.unique(dl)) == set(sc.LIMITS.tolist())


def test_no_fuzz_seed_is_rejected(oracle):
    for seed in sc.FUZZ_SEEDS:
        f = sc.fuzz_case(seed)
        assert 40 <= f["W"] <= 699 and 24 <= f["H"] <= 259 and f["mw"] >= 12 and f["mh"] >= 8
        assert 1 <= f["radius"] <= 8 and 1 <= f["thresh"] <= 63
        x, y, w, h = f["roi"]
        assert x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= f["mw"] and y + h <= f["mh"]
        p = oracle.default_params(sigma_color=1.5, threads=4, disc_radius=f["radius"], lrc_thresh=f["thresh"])
        out, conf = oracle.wls_filter_scaled(f["dl"], f["view"], f["dr"], f["roi"], p)      # raises where the oracle refuses
        roi = sc.inside(conf.shape, sc.hi_roi(f["roi"], (f["W"], f["H"]), (f["mw"], f["mh"])))
        assert (conf[roi] > 0).mean() > 0.1, seed
    # the geometry is spread over the path's forms: scale factors on both sides of the staging buffer's reach (0.6),
    # reductions, both channel counts
    cases = [sc.fuzz_case(s) for s in sc.FUZZ_SEEDS]
    sx = np.array([c["mw"] / c["W"] for c in cases])
    assert (sx <= 0.6).sum() >= 10 and ((sx > 0.65) & (sx < 1)).sum() >= 5 and (sx > 1).sum() >= 2
    assert {c["ch"] for c in cases} == {1, 3}


def test_float_product_of_the_lrc_threshold(oracle):
    """(int)(resize_factor * LRC_thresh), DF.cpp:318, is a float32 product.  No fuzz seed and no threshold at 107 / 320
    separates it from a double product; the directed case does, and the threshold's last unit changes the map."""
    for seed in sc.FUZZ_SEEDS:
        f = sc.fuzz_case(seed)
        a, b = sc.lrc_thresholds(f["mw"], f["W"], f["thresh"])
        assert a == b
    assert all(len(set(sc.lrc_thresholds(107, 320, t))) == 1 for t in range(1, 64))
    c = sc.LRC_CASE
    (W, H), (mw, mh) = c["view"], c["maps"]
    assert sc.lrc_thresholds(mw, W, c["thresh"]) == (14, 13)
    _, dl, dr, roi = sc.synthetic.make_artificial_example(mw, mh, 1, seed=c["seed"])
    rf = float(np.float32(mw) / np.float32(W))
    c14 = oracle.confidence(dl, dr, roi, radius=5, lrc_thresh=c["thresh"], resize_factor=rf)
    c13 = oracle.confidence(dl, dr, roi, radius=5, lrc_thresh=c["thresh"] - 1, resize_factor=rf)   # 0.7 * 19 = 13.3
    assert sc.lrc_thresholds(mw, W, c["thresh"] - 1) == (13, 13)
    assert (c14 != c13).mean() > 0.01                               # pixels whose left-right difference is exactly 13
