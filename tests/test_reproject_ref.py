"""CPU tests of the direct statement of the reprojection to 3-D (tests/reproject_ref.py), which the device code is held to
bit for bit (tests/test_gpu_reproject.py): against a per-pixel loop in Python floats, against the pinhole formula, and the
rules for missing values and for the order of the point list."""
import math
import struct

import numpy as np

import reproject_ref as ref

# nothing here is a power of two or a short binary fraction: every product and sum rounds
Q_FULL = np.array([[0.7, -0.013, 0.31, -301.3],
                   [0.017, 1.1, -0.23, 177.7],
                   [0.0031, -0.0007, 0.9, 517.1],
                   [0.00011, 0.00013, 0.37, 1.9]])


def rectified_q(f=721.5377, cx=609.5593, cy=172.854, baseline=0.5371, cx2=None):
    """Q of stereoRectify: Z = f * B / d when both principal points agree."""
    cx2 = cx if cx2 is None else cx2
    return np.array([[1.0, 0, 0, -cx], [0, 1.0, 0, -cy], [0, 0, 0, f], [0, 0, 1.0 / baseline, (cx - cx2) / baseline]])


def _f32(v):
    """Round a Python float (binary64) to float32 the way a C cast does: nearest, overflow to infinity."""
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def _loop(disp, Q, scale):
    """The definition, pixel by pixel: Python floats are binary64, every operator rounds once."""
    H, W = disp.shape
    out = np.empty((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            d = float(disp[y, x]) * scale
            r = [((float(Q[i][0]) * x + float(Q[i][1]) * y) + float(Q[i][3])) + float(Q[i][2]) * d for i in range(4)]
            iw = 1.0 / r[3]
            out[y, x] = [_f32(r[0] * iw), _f32(r[1] * iw), _f32(r[2] * iw)]
    return out


def test_statement_equals_a_per_pixel_loop_bit_for_bit():
    rng = np.random.default_rng(5)
    for disp in (rng.integers(-300, 3000, (5, 7)).astype(np.int16), (rng.random((5, 7)) * 97.3 + 0.1).astype(np.float32)):
        for scale in (1.0, 1.0 / 16, 0.1):
            got = ref.reproject(disp, Q_FULL, scale)
            assert got.dtype == np.float32 and got.shape == (5, 7, 3)
            assert np.array_equal(got.view(np.uint32), _loop(disp, Q_FULL, scale).view(np.uint32))


def test_pinhole_depth():
    f, B = 721.5377, 0.5371
    disp = (np.arange(1, 36, dtype=np.float32).reshape(5, 7) * 1.37).astype(np.float32)
    z = ref.reproject(disp, rectified_q(f, baseline=B))[..., 2]
    expect = f * B / disp.astype(np.float64)
    # Z = f * (1 / (d / B)): three roundings in double, then one to float
    assert np.all(np.abs(z.astype(np.float64) - expect) <= np.abs(expect) * (2.0 ** -24 + 4 * 2.0 ** -53))
    fixed = np.round(disp * 16).astype(np.int16)                        # the filters' units, disparity * 16
    z16 = ref.reproject(fixed, rectified_q(f, baseline=B), 1.0 / 16)[..., 2]
    expect16 = f * B / (fixed.astype(np.float64) / 16)
    assert np.all(np.abs(z16.astype(np.float64) - expect16) <= np.abs(expect16) * (2.0 ** -24 + 4 * 2.0 ** -53))
    x = ref.reproject(disp, rectified_q(f, cx=3.0, cy=2.0, baseline=B))[..., 0]
    assert np.all(x[:, 3] == 0) and np.all(x[:, 4] > 0) and np.all(x[:, 2] < 0)     # the principal point's column


def test_division_by_zero_is_not_sanitised():
    disp = np.array([[0, 16], [32, 0]], np.int16)
    out = ref.reproject(disp, rectified_q(cx=0.5, cy=0.5))                # r_3 = d / B: zero where d == 0
    assert np.isinf(out[0, 0]).all() and np.isinf(out[1, 1]).all() and np.isfinite(out[0, 1]).all()
    Q = rectified_q(cx=1.0)
    Q[3] = 0                                                             # iw = 1 / 0 everywhere
    out = ref.reproject(disp, Q)
    assert not np.isfinite(out).any()
    assert np.isnan(out[:, 1, 0]).all() and np.isinf(out[:, 0, 0]).all()  # 0 * inf in the principal point's column


def test_missing_values_three_modes():
    disp = np.array([[-16, 5, 80], [80, -16, 7]], np.int16)
    Q = rectified_q()
    plain = ref.reproject(disp, Q)
    assert np.array_equal(plain, ref.reproject(disp, Q, mode=ref.MISSING_NONE))
    assert not (plain[..., 2] == 10000).any()
    low = ref.reproject(disp, Q, mode=ref.MISSING_MIN)
    assert np.array_equal(low[..., 2] == 10000, disp == -16)
    assert np.array_equal(low[..., :2].view(np.uint32), plain[..., :2].view(np.uint32))      # X and Y stay as computed
    assert np.array_equal(low[..., 2][disp != -16], plain[..., 2][disp != -16])
    named = ref.reproject(disp, Q, mode=ref.MISSING_VALUE, missing_value=80)
    assert np.array_equal(named[..., 2] == 10000, disp == 80)
    assert not (ref.reproject(disp, Q, mode=ref.MISSING_VALUE, missing_value=81)[..., 2] == 10000).any()
    # the test is on raw values, within FLT_EPSILON: below it a float neighbour of the minimum is missing too
    eps = np.float32(ref.FLT_EPSILON)
    f = np.array([[0.0, eps, 2 * eps, np.nan, -0.0, 1.0]], np.float32)
    assert list(ref.missing_mask(f, ref.MISSING_MIN)[0]) == [True, True, False, False, True, False]
    assert ref.map_minimum(f) == 0.0
    assert math.isnan(ref.map_minimum(np.full((2, 2), np.nan, np.float32)))
    assert not ref.missing_mask(np.full((2, 2), np.nan, np.float32), ref.MISSING_MIN).any()
    assert not ref.missing_mask(np.array([[-np.inf, 1.0]], np.float32), ref.MISSING_MIN).any()   # inf - inf is NaN


def test_each_map_of_a_batch_has_its_own_minimum():
    batch = np.array([[[3, 9, 3]], [[9, 12, 40]], [[-7, 3, 9]]], np.int16)
    z = ref.reproject(batch, rectified_q(), mode=ref.MISSING_MIN)[..., 2]
    assert np.array_equal(z == 10000, [[[True, False, True]], [[True, False, False]], [[True, False, False]]])


def test_point_list_is_in_raster_order():
    rng = np.random.default_rng(11)
    disp = rng.integers(1, 200, (6, 9)).astype(np.int16)
    disp[rng.random((6, 9)) < 0.3] = -16
    view = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    Q = rectified_q()
    pts, col, idx = ref.point_cloud(disp, Q, view, mode=ref.MISSING_VALUE, missing_value=-16)
    xyz = ref.reproject(disp, Q)
    expect = [(y, x) for y in range(6) for x in range(9) if disp[y, x] != -16]
    assert len(pts) == len(expect) and list(idx) == [y * 9 + x for y, x in expect]
    assert all(np.array_equal(pts[k], xyz[y, x]) and np.array_equal(col[k], view[y, x]) for k, (y, x) in enumerate(expect))
    # ROI and z range cut the set without reordering it
    pts2, _, idx2 = ref.point_cloud(disp, Q, None, roi=(1, 2, 5, 3), z_range=(0.0, 40.0), mode=ref.MISSING_VALUE, missing_value=-16)
    keep = [k for k, (y, x) in enumerate(expect) if 2 <= y < 5 and 1 <= x < 6 and 0.0 <= float(xyz[y, x, 2]) <= 40.0]
    assert 0 < len(keep) < len(expect) and list(idx2) == [int(idx[k]) for k in keep] and np.array_equal(pts2, pts[keep])
    # a pixel whose point is not finite is not in the list
    disp0 = disp.copy()
    disp0[0, 0] = 0
    assert 0 not in ref.point_cloud(disp0, Q)[2]
