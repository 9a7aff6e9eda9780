"""CPU pins on the statement of the joint bilateral filter (tests/jbf_ref.py; include/adf_wls.h): the vectorised
statement against a naive per-pixel loop, constant maps, the border rule against hand-written expectations, the radius
rule, and the distance of the float32 statement to the same statement in float64.  Run with -s to see the measured
figures."""
import numpy as np
import pytest

import jbf_ref
from jbf_ref import BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE

BORDERS = [BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101]


def _joint(rng, H, W, ch):
    """Smooth regions with edges, a little noise, and a flat patch."""
    base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
    g = np.clip(base[..., None] + rng.integers(-6, 7, (H, W, ch)), 0, 255).astype(np.uint8)
    g[H // 2:, W // 2:, :] = 90
    return g if ch == 3 else g[..., 0]


def _src16(rng, H, W):
    """Plateaus, noise over the whole range and both ends of it."""
    s = rng.choice(np.array([16, 480, 2000, -16], np.int16), (H, W))
    noisy = rng.random((H, W)) < 0.3
    s[noisy] = rng.integers(-32768, 32768, int(noisy.sum())).astype(np.int16)
    s[0, 0], s[-1, -1], s[H // 2, W // 2] = 32767, -32768, -32767
    return s


def _cv_border(p, n, border):
    """cv::borderInterpolate as OpenCV writes it: reflect step by step until the coordinate is inside."""
    if 0 <= p < n:
        return p
    if border == BORDER_REPLICATE:
        return 0 if p < 0 else n - 1
    if n == 1:
        return 0
    delta = 1 if border == BORDER_REFLECT_101 else 0
    while not 0 <= p < n:
        p = -p - 1 + delta if p < 0 else n - 1 - (p - n) - delta
    return p


def _naive(joint, src, r, C, S, border):
    """Per pixel, per tap, scalar float32 arithmetic in the stated order."""
    H, W = src.shape
    g = joint.reshape(H, W, -1).astype(int)
    out = np.empty((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            total, wsum = np.float32(0), np.float32(0)
            for i in range(-r, r + 1):
                for j in range(-r, r + 1):
                    if i * i + j * j > r * r:
                        continue
                    qy, qx = _cv_border(y + i, H, border), _cv_border(x + j, W, border)
                    L = int(np.abs(g[y, x] - g[qy, qx]).sum())
                    w = np.float32(S[i * i + j * j]) * np.float32(C[L])
                    total = total + w * np.float32(src[qy, qx])
                    wsum = wsum + w
            out[y, x] = total / wsum
    return out


@pytest.mark.parametrize("H,W,ch,d,border", [(5, 7, 3, 5, BORDER_REFLECT_101), (3, 2, 1, 11, BORDER_REFLECT),
                                             (4, 6, 1, 7, BORDER_REPLICATE)])
def test_the_statement_against_a_naive_loop(H, W, ch, d, border):
    rng = np.random.default_rng(H * 100 + W)
    joint, src = _joint(rng, H, W, ch), _src16(rng, H, W)
    C, S, r = jbf_ref.tables(d, 20.0, 2.5, ch)
    assert r == d // 2 and len(jbf_ref.taps(r)) > (2 * r + 1) ** 2 // 2
    got = jbf_ref.jbf(joint, src, r, C, S, border, np.float32)
    want = _naive(joint, src, r, C, S, border)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, src.astype(np.float32))


def test_constant_maps_come_back_exactly():
    """With an integer output every constant comes back: the quotient is the constant to a few ulp, far inside the half
    that rint forgives.  As float32 the quotient itself is exact where every product w * v is, i.e. for 0 and powers of
    two; other floats come back to within the bound of test_float32_against_float64."""
    rng = np.random.default_rng(1)
    for ch in (1, 3):
        joint = rng.integers(0, 256, (13, 17, ch), dtype=np.uint8)
        joint = joint if ch == 3 else joint[..., 0]
        for d, sc, ss in ((5, 25.0, 3.0), (-1, 3.0, 2.0), (15, 1000.0, 0.5)):
            C, S, r = jbf_ref.tables(d, sc, ss, ch)
            for border in BORDERS:
                for v, dtype in ((-32768, np.int16), (32767, np.int16), (-1234, np.int16), (255, np.uint8), (77, np.uint8),
                                 (0.0, np.float32), (-0.25, np.float32), (4096.0, np.float32)):
                    src = np.full((13, 17), v, dtype)
                    out = jbf_ref.jbf(joint, src, r, C, S, border)
                    assert out.dtype == src.dtype and np.array_equal(out, src)


def test_border_index():
    p = np.arange(-7, 12)
    #                    -7 -6 -5 -4 -3 -2 -1 | 0  1  2  3 | 4  5  6  7  8  9 10 11
    want = {BORDER_REPLICATE:   [0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3],
            BORDER_REFLECT:     [1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3],
            BORDER_REFLECT_101: [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1]}
    for border in BORDERS:
        assert jbf_ref.border_index(p, 4, border).tolist() == want[border]
        assert jbf_ref.border_index(np.arange(-9, 10), 1, border).tolist() == [0] * 19          # n = 1
        for n in (1, 2, 3, 5):                                                                # |offset| > 2n, step by step
            q = np.arange(-3 * n - 31, 4 * n + 32)
            assert jbf_ref.border_index(q, n, border).tolist() == [_cv_border(int(v), n, border) for v in q]
    assert jbf_ref.border_index(np.array([-3, -2, -1, 0, 1, 2, 3, 4]), 2, BORDER_REFLECT_101).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    assert jbf_ref.border_index(np.array([-3, -2, -1, 0, 1, 2, 3, 4]), 2, BORDER_REFLECT).tolist() == [1, 1, 0, 0, 1, 1, 0, 0]
    for bad in (0, 3, 5, 16):
        with pytest.raises(ValueError):
            jbf_ref.border_index(p, 4, bad)


def test_radius_rule():
    # d > 0: d / 2, raised to 1
    for d, r in ((1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (9, 4), (63, 31)):
        assert jbf_ref.clamped(d, 10.0, 7.0)[2] == r
    # d <= 0: cvRound(1.5 sigmaSpace); 1.0 and 3.0 make exact halves in double, decided by half-to-even alone
    for ss, r in ((1.0, 2), (3.0, 4), (2.0, 3), (8.0, 12), (0.1, 1), (0.0, 2), (-5.0, 2)):
        assert jbf_ref.clamped(0, 10.0, ss)[2] == r and jbf_ref.clamped(-7, 10.0, ss)[2] == r
    assert jbf_ref.clamped(5, 0.0, -1.0)[:2] == (1.0, 1.0) and jbf_ref.clamped(5, 2.5, 0.5)[:2] == (2.5, 0.5)
    for d, sc, ss, ch in ((5, 25.0, 3.0, 1), (-1, 3.0, 8.0, 3)):
        C, S, r = jbf_ref.tables(d, sc, ss, ch)
        assert C.dtype == S.dtype == np.float32 and C.shape == (255 * ch + 1,) and S.shape == (r * r + 1,)
        assert C[0] == 1.0 and S[0] == 1.0 and (np.diff(C) <= 0).all() and (np.diff(S) <= 0).all()
    assert len(jbf_ref.taps(1)) == 5 and len(jbf_ref.taps(2)) == 13 and jbf_ref.taps(1) == [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]


FRACTIONS = []


@pytest.mark.parametrize("ch,d,sc,ss,kind", [(3, 63, 25.0, 20.0, "s16"), (1, 63, 1000.0, 100.0, "s16"), (3, 17, 3.0, 3.0, "s16"),
                                             (1, 5, 25.0, 0.5, "u8"), (3, 17, 25.0, 3.0, "f32"), (1, -1, 40.0, 8.0, "f32")])
def test_float32_against_float64(ch, d, sc, ss, kind):
    """Each of the two chains carries one rounding per tap for the product and one for the sum, and the quotient one
    more: to first order |y32 - y64| <= 2 (taps + 2) 2^-24 max|src|.  Worst observed over these cases: 0.135 of the
    bound (r = 2, sigmaSpace 0.5, uint8 data: few taps, so the roundings cancel least); at r = 31 on int16 data 0.021
    absolute, 0.002 of the bound."""
    rng = np.random.default_rng(ch * 1000 + abs(d))
    H, W = 21, 45
    joint = _joint(rng, H, W, ch)
    src = {"s16": lambda: _src16(rng, H, W), "u8": lambda: rng.integers(0, 256, (H, W), dtype=np.uint8),
           "f32": lambda: (rng.random((H, W), np.float32) * 4000 - 2000).astype(np.float32)}[kind]()
    C, S, r = jbf_ref.tables(d, sc, ss, ch)
    y32 = jbf_ref.weighted_mean(joint, src, r, C, S, BORDER_REFLECT_101, np.float32)
    y64 = jbf_ref.weighted_mean(joint, src, r, C, S, BORDER_REFLECT_101, np.float64)
    assert y32.dtype == np.float32 and y64.dtype == np.float64
    bound = 2 * (len(jbf_ref.taps(r)) + 2) * 2.0 ** -24 * float(np.abs(src.astype(np.float64)).max())
    err = float(np.abs(y32.astype(np.float64) - y64).max())
    FRACTIONS.append(err / bound)
    print("r %2d ch %d %s: |y32 - y64| <= %.3g, bound %.3g, fraction %.4f (worst so far %.4f)" % (r, ch, kind, err, bound, err / bound, max(FRACTIONS)))
    assert err <= bound
