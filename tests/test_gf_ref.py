"""CPU tests that pin the guided filter's NumPy statement tests/gf_ref.py (include/adf_wls.h, "guided filter"): its fixed
points, the relation between its float and integer paths, its border rule, and its distance to an independent float64
textbook guided filter -- window means from a summed-area table over numpy.pad(mode="symmetric"), numpy.linalg.solve per
pixel -- under a bound derived from that comparator's own coefficients."""
import numpy as np
import pytest

from gf_ref import convert, guided_filter, guided_filter_q, reflect, window_sum

SIZES = [(1, 5), (5, 1), (9, 13), (40, 70)]                              # H, W
RADII = [0, 1, 4, 31]
EPS = [0.01, 1.0, 100.0]


def _guide(rng, H, W, ch):
    """Smooth regions with edges and a little noise; a flat patch, where the covariances vanish."""
    base = (np.add.outer(np.arange(H) // 3 * 9, np.arange(W) // 5 * 14) % 256).astype(np.int64)
    g = np.clip(base[..., None] + rng.integers(-6, 7, (H, W, ch)), 0, 255).astype(np.uint8)
    g[H // 2:, W // 2:] = 90
    return g if ch == 3 else g[..., 0]


def _src16(rng, H, W):
    """int16 disparities: steps, noise, and the ends of the range next to each other."""
    s = rng.choice(np.array([16, 480, 2000, -16], np.int16), (H, W))
    noisy = rng.random((H, W)) < 0.3
    s[noisy] = rng.integers(-32768, 32768, int(noisy.sum())).astype(np.int16)
    ends = rng.random((H, W)) < 0.1
    s[ends] = rng.choice(np.array([32767, -32767, -32768], np.int16), int(ends.sum()))
    return s


def _box_mean(v, r):
    """Window means of a float64 / int64 plane: a summed-area table over the symmetric padding."""
    p = np.pad(v, r, mode="symmetric")
    sat = np.zeros((p.shape[0] + 1, p.shape[1] + 1), p.dtype)
    sat[1:, 1:] = p.cumsum(0).cumsum(1)
    n = 2 * r + 1
    H, W = v.shape
    s = sat[n:n + H, n:n + W] - sat[0:H, n:n + W] - sat[n:n + H, 0:W] + sat[0:H, 0:W]
    return s.astype(np.float64) / (n * n)


def _textbook(guide, src, r, eps):
    """He et al.'s guided filter in float64: q, and the window mean of |b| + 255 sum |a_c| that the bound is made of."""
    g = (guide[..., None] if guide.ndim == 2 else guide).astype(np.int64)
    ch = g.shape[2]
    p = src.astype(np.int64)                                             # integer planes: exact sums
    mI = np.stack([_box_mean(g[..., c], r) for c in range(ch)], -1)
    mp = _box_mean(p, r)
    cov_Ip = np.stack([_box_mean(g[..., c] * p, r) for c in range(ch)], -1) - mI * mp[..., None]
    sigma = np.empty(src.shape + (ch, ch))
    for c in range(ch):
        for d in range(ch):
            sigma[..., c, d] = _box_mean(g[..., c] * g[..., d], r) - mI[..., c] * mI[..., d] + (eps if c == d else 0.0)
    a = np.linalg.solve(sigma, cov_Ip[..., None])[..., 0]
    b = mp - (a * mI).sum(-1)
    q = _box_mean(b, r) + sum(_box_mean(a[..., c], r) * g[..., c] for c in range(ch))
    scale = _box_mean(np.abs(b) + 255.0 * np.abs(a).sum(-1), r)
    return q, scale


def test_a_constant_source_returns_the_constant():
    rng = np.random.default_rng(1)
    for ch in (1, 3):
        guide = _guide(rng, 9, 13, ch)
        for dtype, value in ((np.uint8, 201), (np.int16, -32768), (np.int16, 32767), (np.int16, 77), (np.float32, -3.25)):
            for r in (0, 2, 31):
                src = np.full((9, 13), value, dtype)
                out = guided_filter(guide, src, r, 0.5)
                assert out.dtype == src.dtype and np.array_equal(out, src), (ch, dtype, value, r)
                # the float output too wherever the float32 sums of b are exact: N * 32767 at r = 31 needs 27 bits
                if abs(value) * 4 * (2 * r + 1) ** 2 < 2 ** 24 or value == -32768:
                    assert np.array_equal(guided_filter(guide, src, r, 0.5, np.float32), src.astype(np.float32))


def test_an_integer_valued_float_source_gives_the_int16_source_s_bits():
    rng = np.random.default_rng(2)
    for ch in (1, 3):
        for (H, W), r in (((9, 13), 1), ((9, 13), 4), ((40, 70), 31), ((1, 5), 2)):
            guide, src = _guide(rng, H, W, ch), _src16(rng, H, W)
            for eps in (0.01, 100.0):
                qi = guided_filter_q(guide, src, r, eps)
                qf = guided_filter_q(guide, src.astype(np.float32), r, eps)
                assert np.array_equal(qi.view(np.uint64), qf.view(np.uint64))
                for d in (np.uint8, np.int16, np.float32):
                    assert np.array_equal(convert(qi, d), guided_filter(guide, src.astype(np.float32), r, eps, d))


def test_radius_zero_is_the_identity_of_the_model():
    """N = 1: every covariance is 0, so a = 0, b = p and q = p."""
    rng = np.random.default_rng(3)
    src = _src16(rng, 9, 13)
    for ch in (1, 3):
        assert np.array_equal(guided_filter(_guide(rng, 9, 13, ch), src, 0, 1.0), src)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (3, 4), (9, 13)])
@pytest.mark.parametrize("r", [0, 1, 4, 13, 31])
def test_the_border_is_numpy_s_symmetric_padding(H, W, r):
    rng = np.random.default_rng(H * 100 + W + r)
    v = rng.integers(-1000, 1000, (H, W)).astype(np.int64)
    for n in (H, W):
        assert np.array_equal(reflect(np.arange(-r, n + r), n), np.pad(np.arange(n), r, mode="symmetric"))
    p = np.pad(v, r, mode="symmetric")
    direct = np.array([[p[y:y + 2 * r + 1, x:x + 2 * r + 1].sum() for x in range(W)] for y in range(H)])
    assert np.array_equal(window_sum(v, r), direct)


def test_the_float32_sums_follow_the_stated_order():
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((6, 7)) * 1e3).astype(np.float32)
    r = 2
    p = np.pad(v, r, mode="symmetric")
    exp = np.empty_like(v)
    for y in range(6):
        for x in range(7):
            cols = []
            for dx in range(2 * r + 1):
                c = p[y, x + dx]
                for dy in range(1, 2 * r + 1):
                    c = np.float32(c + p[y + dy, x + dx])
                cols.append(c)
            s = cols[0]
            for c in cols[1:]:
                s = np.float32(s + c)
            exp[y, x] = s
    assert np.array_equal(window_sum(v, r).view(np.uint32), exp.view(np.uint32))


def test_conversion_rounds_half_to_even_and_saturates():
    q = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 254.5, 255.5, 300.0, -7.0, 32767.5, -32768.5, 1e9, -1e9, np.nan])
    assert convert(q, np.uint8).tolist() == [0, 2, 2, 0, 0, 254, 255, 255, 0, 255, 0, 255, 0, 0]
    assert convert(q, np.int16).tolist() == [0, 2, 2, 0, -2, 254, 256, 300, -7, 32767, -32768, 32767, -32768, -32768]
    assert convert(np.array([0.1]), np.float32)[0] == np.float32(0.1)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_distance_to_a_float64_textbook_guided_filter(ch, H, W):
    """|q - q64| <= 2 (4r + 4) 2^-24 mean_window(|b64| + 255 sum_c |a64_c|): one float32 rounding per coefficient plus two
    sequential float32 sums of 2r + 1 terms, to first order, doubled for the higher-order terms."""
    rng = np.random.default_rng(ch * 1000 + H * 10 + W)
    worst = 0.0
    for r in RADII:
        for eps in EPS:
            guide, src = _guide(rng, H, W, ch), _src16(rng, H, W)
            q = guided_filter_q(guide, src, r, eps)
            q64, scale = _textbook(guide, src, r, eps)
            bound = 2.0 * (4 * r + 4) * 2.0 ** -24 * scale
            ratio = float((np.abs(q - q64) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (r, eps, ratio)
    print("worst error / bound: %.3f" % worst)
