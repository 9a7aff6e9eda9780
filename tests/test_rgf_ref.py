"""CPU tests of the rolling guidance filter's NumPy statement tests/rgf_ref.py (include/adf_wls.h: "rolling guidance
filter"): the vectorised statement against a per-pixel loop, uint8 against the joint bilateral statement applied
num_iter times, what every depth must return unchanged, and the host tables: their lengths and the interpolated float
weight against the Gaussian it stands for."""
import math

import numpy as np
import pytest

import jbf_ref
import rgf_ref

DEPTHS = [np.uint8, np.int16, np.float32]
BORDERS = [rgf_ref.BORDER_REPLICATE, rgf_ref.BORDER_REFLECT, rgf_ref.BORDER_REFLECT_101]
BITS = {np.dtype(np.uint8): np.uint8, np.dtype(np.int16): np.uint16, np.dtype(np.float32): np.uint32}


def _map(rng, shape, dtype):
    if dtype == np.float32:
        return (rng.choice(np.array([-2.5, 0.0, 16.25, 60.0], np.float32), shape) + rng.standard_normal(shape).astype(np.float32) * 3).astype(np.float32)
    if dtype == np.int16:
        return (rng.choice(np.array([16, 480, 2000, -16]), shape) + rng.integers(-20, 21, shape)).astype(np.int16)
    return np.clip(rng.choice(np.array([0, 7, 128, 250]), shape) + rng.integers(-9, 10, shape), 0, 255).astype(np.uint8)


def _same_bits(a, b):
    v = BITS[a.dtype]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


@pytest.mark.parametrize("dtype", DEPTHS)
@pytest.mark.parametrize("shape,r,border", [((5, 7), 1, BORDERS[2]), ((4, 6), 2, BORDERS[1]), ((3, 2), 3, BORDERS[0]), ((1, 5), 2, BORDERS[2])])
def test_statement_equals_the_per_pixel_loop(dtype, shape, r, border):
    rng = np.random.default_rng(shape[0] * 10 + r)
    src = _map(rng, shape, dtype)
    colour, space, r_, scale = rgf_ref.tables(dtype, 2 * r + 1, 12.0, 1.5)
    assert r_ == r
    for n in (1, 3):
        assert _same_bits(rgf_ref.rgf(src, r, colour, space, scale, n, border), rgf_ref.naive(src, r, colour, space, scale, n, border))


@pytest.mark.parametrize("sc", [3.0, 25.0, 1000.0])
def test_uint8_is_the_joint_bilateral_statement_iterated(sc):
    rng = np.random.default_rng(int(sc))
    src = _map(rng, (11, 17), np.uint8)
    src[2:5, 3:9] = rng.integers(0, 256, (3, 6), dtype=np.uint8)
    C, S, r = jbf_ref.tables(7, sc, 2.0, 1)
    colour, space, r_, scale = rgf_ref.tables(np.uint8, 7, sc, 2.0)
    assert r == r_ and scale == 1.0 and np.array_equal(space, S)
    assert np.array_equal(colour, C[:len(colour)]) and (C[len(colour):] == 0).all()         # C cut after its first zero
    joint = src
    for n in range(1, 4):
        joint = jbf_ref.jbf(joint, src, r, C, S, rgf_ref.BORDER_REFLECT, np.uint8)
        assert np.array_equal(rgf_ref.rgf(src, r, colour, space, scale, n, rgf_ref.BORDER_REFLECT), joint)


@pytest.mark.parametrize("dtype", DEPTHS)
def test_constant_maps_and_zero_iterations(dtype):
    rng = np.random.default_rng(3)
    colour, space, r, scale = rgf_ref.tables(dtype, 7, 25.0, 3.0)
    # float32: every w * c is exact when c is zero or a power of two, so sum = c * wsum and the quotient is c exactly; any
    # other constant comes back within the roundings of the two chains (49 taps: a few ulps), which is NOT "exactly".
    values = {np.uint8: (0, 255, 77), np.int16: (-32768, 32767, -16), np.float32: (0.0, -4.0, 0.5, 2.0 ** 100)}[dtype]
    for v in values:
        flat = np.full((6, 9), v, dtype)
        assert _same_bits(rgf_ref.rgf(flat, r, colour, space, scale, 3), flat)
    if dtype == np.float32:
        flat = np.full((6, 9), -2.5, dtype)
        assert np.abs(rgf_ref.rgf(flat, r, colour, space, scale, 3) / flat - 1).max() <= 49 * 2.0 ** -23
    src = _map(rng, (2, 6, 9), dtype)
    out = rgf_ref.rgf(src, r, colour, space, scale, 0)
    assert _same_bits(out, src) and out is not src
    assert not _same_bits(rgf_ref.rgf(src, r, colour, space, scale, 2), src)                # (the filter does something)


@pytest.mark.parametrize("sc,T", [(1.0, 16), (25.0, 362), (5000.0, 65536)])
def test_table_lengths(adf, sc, T):
    n = 1                                                                                    # a Python loop over math.exp
    while n < 65536 and np.float32(math.exp(float(n) * float(n) * (-0.5 / (sc * sc)))) != 0:
        n += 1
    n = min(n + 1, 65536)
    assert n == T
    colour, space, r, scale = adf.rgfTables(np.int16, -1, sc, 3.0)
    assert colour.shape == (T,) and colour.dtype == np.float32 and colour[0] == 1.0 and scale == 1.0 and r == 4
    assert (np.diff(colour) <= 0).all() and (colour[:-1] > 0).all() and (T == 65536 or colour[-1] == 0)
    assert len(rgf_ref.colour_table(np.int16, sc)) == T
    c8 = adf.rgfTables(np.uint8, -1, sc, 3.0)[0]
    assert np.array_equal(c8, colour[:256]) and len(c8) == min(T, 256)
    assert np.array_equal(c8, adf.jbfTables(-1, sc, 3.0, 1)[0][:len(c8)])                    # the joint bilateral filter's C


def test_float_grid(adf):
    G, space, r, scale = adf.rgfTables(np.float32, 9, 25.0, 3.0)
    assert G.shape == (rgf_ref.GRID_ENTRIES,) and G.dtype == np.float32 and r == 4 and scale == np.float32(256.0 / 25.0)
    assert G[0] == 1.0 and (G[:3692] > 0).all() and (G[3692:] == 0).all() and (np.diff(G) <= 0).all()
    for sc in (0.5, 1000.0):                                                                 # a constant: no parameter moves it
        assert np.array_equal(adf.rgfTables(np.float32, 3, sc, 1.0)[0], G)
    ref = rgf_ref.colour_table(np.float32, 25.0)
    assert np.abs(G.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max() <= 1
    assert adf.rgfTables(np.float32, 9, 0.0, 3.0)[3] == np.float32(256.0)                    # sigma_color <= 0 -> 1


@pytest.mark.parametrize("sigma", [0.05, 25.0, 3000.0])
def test_interpolated_float_weight_against_the_gaussian(adf, sigma):
    """Linear interpolation of exp(-t*t/2) on a grid of h = 1/256 errs by at most h*h/8 * max|f''| = 1.9e-6 (|f''| <= 1, at
    t = 0); the float32 roundings of a, f, the table and the three operations add a few 1e-7.  The bound is 3e-6."""
    G, _, _, scale = adf.rgfTables(np.float32, 9, sigma, 3.0)
    rng = np.random.default_rng(7)
    L = (rng.random(200000) * 16.0 * sigma).astype(np.float32)
    L[:4] = (0.0, sigma, 4 * sigma, np.float32(16.0 * sigma * 0.999999))
    w = rgf_ref.range_weight(L, np.zeros_like(L), G, scale)
    exact = np.exp(-0.5 * (L.astype(np.float64) / sigma) ** 2)
    err = np.abs(w.astype(np.float64) - exact).max()
    print("sigma %g: max |interpolated - exact| = %.3g" % (sigma, err))
    assert err <= 3e-6
    far = np.array([16.0 * sigma * 1.0001, 1e30, np.inf, np.nan], np.float32)                # beyond 16 sigma: exactly 0
    assert (rgf_ref.range_weight(far, np.zeros_like(far), G, scale) == 0).all()
    assert rgf_ref.range_weight(np.float32([5.0]), np.float32([5.0]), G, scale)[0] == 1.0    # the centre tap
