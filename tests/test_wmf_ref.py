"""CPU tests of the weighted median filter's definition (include/adf_wls.h): the library's host weight table against
float64 NumPy, hand cases on the direct statement tests/wmf_ref.py, and the usefulness gate on the Tsukuba pair."""
import numpy as np
import pytest

from test_oracle_bm import load_tsukuba
from wmf_ref import weighted_median

LEVELS = 3 * 256 * 256
ONE = 65536


def _numpy_table(sigma):
    return np.rint(np.exp(-np.arange(LEVELS, dtype=np.float64) / (2.0 * sigma * sigma)) * 65536.0).astype(np.int64)


@pytest.mark.parametrize("sigma", [0.5, 1.0, 10.0, 25.5, 1000.0])
def test_weight_table_against_numpy(adf, sigma):
    t = adf.wmfWeightTable(sigma)
    assert t.dtype == np.uint32 and t.shape == (LEVELS,)
    t = t.astype(np.int64)
    # the host libm's last bit may flip a rounding: every entry within +-1
    assert np.abs(t - _numpy_table(sigma)).max() <= 1
    assert t[0] == ONE
    assert (np.diff(t) <= 0).all()


def test_weight_table_off_is_all_ones(adf):
    assert (adf.wmfWeightTable(25.5, adf.WMF_OFF) == ONE).all()
    assert (adf.wmfWeightTable(0.001, adf.WMF_OFF) == ONE).all()


def _ones():
    return np.full(LEVELS, ONE, np.uint32)


def test_unused_centre_is_filled():
    src = np.full((5, 5), 48, np.int16)
    src[2, 2] = -16
    joint = np.zeros((5, 5), np.uint8)
    assert weighted_median(joint, src, 1, _ones(), ignore_value=-16)[2, 2] == 48
    mask = np.ones((5, 5), np.uint8)
    mask[2, 2] = 0
    assert weighted_median(joint, src, 1, _ones(), mask=mask)[2, 2] == 48
    assert weighted_median(joint, src, 1, _ones())[2, 2] == 48          # (a plain median removes the outlier too)
    assert weighted_median(joint, src, 1, _ones(), ignore_value=48)[2, 2] == -16 and \
        weighted_median(joint, src, 1, _ones(), ignore_value=48)[0, 0] == 48   # no tap used at (0, 0): src stays


def test_all_unused_window_keeps_src():
    rng = np.random.default_rng(1)
    src = rng.integers(-100, 100, (6, 7)).astype(np.int16)
    joint = rng.integers(0, 256, (6, 7), dtype=np.uint8)
    out = weighted_median(joint, src, 2, _ones(), mask=np.zeros((6, 7), np.uint8))
    assert np.array_equal(out, src)
    # every used tap of weight 0: a table that is 0 everywhere but at distance 0, a joint without two equal neighbours
    t = np.zeros(LEVELS, np.uint32)
    t[0] = ONE
    joint = (np.arange(42, dtype=np.uint8) * 3).reshape(6, 7)
    src[2, 3] = -16
    out = weighted_median(joint, src, 1, t, ignore_value=-16)
    assert out[2, 3] == -16 and np.array_equal(out, src)


def test_huge_sigma_equals_off_equals_lower_median(adf):
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (9, 11), dtype=np.uint8)
    joint = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    # at sigma = 1e6 every entry rounds to 65536: exp(-195075 / 2e12) * 65536 = 65536 - 0.0064
    t = adf.wmfWeightTable(1e6)
    assert (t == ONE).all()
    a = weighted_median(joint, src, 1, t)
    b = weighted_median(joint, src, 1, adf.wmfWeightTable(1.0, adf.WMF_OFF))
    assert np.array_equal(a, b)
    # interior windows hold 9 taps: np.median of an odd count is an element, the lower (and only) median
    for y in range(1, 8):
        for x in range(1, 10):
            assert a[y, x] == np.median(src[y - 1:y + 2, x - 1:x + 2])
    # corner windows hold 4 taps: the lower median is the second smallest
    assert a[0, 0] == np.sort(src[:2, :2].ravel())[1]


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_result_is_always_a_tap_value(adf, dtype):
    rng = np.random.default_rng(3)
    H, W, r = 12, 17, 2
    if dtype == np.float32:
        src = rng.standard_normal((H, W)).astype(np.float32)
        src[rng.random((H, W)) < 0.1] = np.nan
        src[0, 0], src[5, 5], src[6, 6], src[7, 7] = np.inf, -np.inf, 0.0, -0.0
    else:
        info = np.iinfo(dtype)
        src = rng.integers(info.min, info.max + 1, (H, W)).astype(dtype)
    joint = rng.integers(0, 256, (H, W), dtype=np.uint8)
    mask = (rng.random((H, W)) < 0.8).astype(np.uint8)
    out = weighted_median(joint, src, r, adf.wmfWeightTable(10.0), mask=mask)
    bits = {np.uint8: np.uint8, np.int16: np.uint16, np.float32: np.uint32}[dtype]
    for y in range(H):
        for x in range(W):
            win = src[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1]
            assert out[y:y + 1, x:x + 1].view(bits)[0, 0] in set(win.view(bits).ravel().tolist()) | {src[y:y + 1, x:x + 1].view(bits)[0, 0]}


def test_usefulness_gate_on_tsukuba(adf, oracle):
    """The oracle's block matcher (16 disparities, window 7) on the Tsukuba pair, the WLS factory's ROI, gray left view as
    joint, ignore value -16, the library's own table: r = 7, sigma = 10 must give MSE <= 1.30 and bad pixels <= 7.0 %
    inside the ROI (measured with a float64 NumPy table: 1.178 and 6.42 %, against a raw 3.510 and 11.48 %; the arithmetic
    is integer, the margin covers only +-1 table entries)."""
    left, right, gt = load_tsukuba()
    gt = gt.astype(np.int16)
    gt[gt == 0] = 16320                                                  # the fixture's 0 is "unknown": UNKNOWN_DISPARITY (DF.cpp:460)
    roi = (19, 3, 362, 282)
    raw = oracle.bm_compute(left, right, 16, 7)
    out = weighted_median(left, raw, 7, adf.wmfWeightTable(10.0), ignore_value=-16)
    mse, bad = oracle.compute_mse(gt, out, roi), oracle.bad_pixel_percent(gt, out, roi)
    raw_mse, raw_bad = oracle.compute_mse(gt, raw, roi), oracle.bad_pixel_percent(gt, raw, roi)
    print("raw MSE %.3f bad %.2f %%; weighted median r = 7, sigma = 10: MSE %.3f bad %.2f %%" % (raw_mse, raw_bad, mse, bad))
    assert mse <= 1.30 and bad <= 7.0
    assert mse < raw_mse and bad < raw_bad
