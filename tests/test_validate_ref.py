"""The direct statements of tests/validate_ref.py themselves (CPU): the SAD cost restatement describes the matcher the
oracle states, and the sequential validateDisparity does what include/adf_wls.h says on hand-worked rows."""
import numpy as np
import pytest

from validate_ref import INT_MAX, bm_winner_cost, validate_disparity


def _pair(seed, H, W, shift=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W + 64), dtype=np.uint8)
    base = (base // 2 + np.roll(base, 1, 1) // 4 + np.roll(base, 1, 0) // 4).astype(np.uint8)
    base[H // 3:H // 2, 30:30 + W // 4] = 77                                 # a flat patch: the texture test bites
    return np.ascontiguousarray(base[:, 20:20 + W]), np.ascontiguousarray(np.roll(base, -shift, 1)[:, 20:20 + W])


@pytest.mark.parametrize("seed,H,W,nd,bs,md,cap,texthr,uniq", [
    (1, 31, 90, 16, 9, 0, 31, 10, 15),
    (2, 23, 120, 32, 21, -5, 63, 0, 0),
    (3, 40, 75, 16, 5, 3, 20, 40, 5),
])
def test_sad_restatement_reproduces_the_oracle(oracle, seed, H, W, nd, bs, md, cap, texthr, uniq):
    left, right = _pair(seed, H, W)
    disp, cost32, cost16 = bm_winner_cost(left, right, nd, bs, md, cap, texthr, uniq)
    exp = oracle.bm_compute(left, right, nd, bs, md, cap, texthr, uniq)
    assert np.array_equal(disp, exp)
    inv = (md - 1) * 16
    assert (exp != inv).any() and (cost16[exp == inv] == 0).all()
    assert np.array_equal(cost16[exp != inv].astype(np.int64) & 0xFFFF, cost32[exp != inv].astype(np.int64) & 0xFFFF)
    assert cost32.max() <= 2 * cap * bs * bs


def _row(W, inv, pixels):
    """A one-row map of INV and a cost plane of zeros with `pixels` = {x: (d, c)} put in."""
    disp = np.full((1, W), inv, np.int16)
    cost = np.zeros((1, W), np.int32)
    for x, (d, c) in pixels.items():
        disp[0, x], cost[0, x] = d, c
    return disp, cost


def test_constant_disparity_is_untouched_at_maxdiff_0():
    disp = np.full((3, 60), 5 * 16, np.int16)
    cost = np.arange(180, dtype=np.int32).reshape(3, 60) % 7
    out, outside = validate_disparity(disp, cost, 0, 16, 0)
    assert np.array_equal(out, disp) and outside == 0


def test_two_votes_on_one_column_the_dearer_one_is_invalidated():
    # x = 30 with d = 4 and x = 34 with d = 8 both match column 26; 4 * 16 > 16 * 1
    disp, cost = _row(60, -16, {30: (64, 10), 34: (128, 20)})
    out, _ = validate_disparity(disp, cost, 0, 16, 1)
    assert out[0, 30] == 64 and out[0, 34] == -16
    assert (out[0] == -16).sum() == 59
    out, _ = validate_disparity(disp, cost, 0, 16, 4)                    # |64 - 128| = 16 * 4 is not MORE than the tolerance
    assert np.array_equal(out, disp)
    disp, cost = _row(60, -16, {30: (64, 20), 34: (128, 10)})           # the other way round
    out, _ = validate_disparity(disp, cost, 0, 16, 1)
    assert out[0, 30] == -16 and out[0, 34] == 128


def test_equal_costs_the_smaller_x_wins():
    disp, cost = _row(60, -16, {30: (64, 10), 34: (128, 10)})
    out, _ = validate_disparity(disp, cost, 0, 16, 1)
    assert out[0, 30] == 64 and out[0, 34] == -16


def test_an_int_max_cost_never_wins():
    disp, cost = _row(60, -16, {30: (64, INT_MAX), 34: (128, INT_MAX)})
    out, _ = validate_disparity(disp, cost, 0, 16, 0)
    assert np.array_equal(out, disp)                                     # disp2[26] stays empty: both pixels are kept
    disp, cost = _row(60, -16, {30: (64, INT_MAX), 34: (128, INT_MAX - 1)})
    out, _ = validate_disparity(disp, cost, 0, 16, 0)
    assert out[0, 30] == -16 and out[0, 34] == 128


def test_a_pixel_whose_candidates_are_outside_the_row_is_kept():
    # d = 40 at x = 20 (outside the matcher's range [0, 16) on purpose): x - d0 = x - d1 = -20, and so is its vote
    disp, cost = _row(60, -16, {20: (40 * 16, 1), 30: (64, 5)})
    out, outside = validate_disparity(disp, cost, 0, 16, 0)
    assert np.array_equal(out, disp) and outside == 1


def test_columns_outside_the_search_range_are_not_looked_at():
    disp = np.full((2, 40), 3 * 16, np.int16)                            # odd x: d = 3; even x: d = 8, the same columns
    disp[:, ::2] = 8 * 16
    cost = np.ones((2, 40), np.int16)
    out, _ = validate_disparity(disp, cost, -4, 16, 0)                   # X0 = 12, X1 = 36
    assert np.array_equal(out[:, :12], disp[:, :12]) and np.array_equal(out[:, 36:], disp[:, 36:])
    assert (out[:, 12:36] != disp[:, 12:36]).any()
