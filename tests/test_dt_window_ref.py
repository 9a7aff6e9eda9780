"""CPU pins on the statement of the domain transform filter's normalized-convolution mode (tests/dt_window_ref.py;
include/adf_wls.h): a written-out scalar loop, the order of the passes, its invariants and degenerate shapes, the tie at a
window's ends, the library's radii against NumPy's doubles, the distance to a float64 evaluation over the same windows
(bound derived in DESIGN.md, section 26) and the measured distance to the reference's own arithmetic (DT.inl:211-221,
277-321, 477-494: float32 running distances, a float32 running integral).  Run with -s to see the measured figures."""
import functools

import numpy as np

import dt_ref
import dt_window_ref as ref

SIZES = [(5, 300), (37, 41), (130, 129)]                                # (H, W): test_dt_ref.py's
ITERS = [1, 3, 5]
SIGMAS = [(10.0, 30.0), (40.0, 10.0), (3.0, 255.0), (80.0, 50.0)]       # (sigmaSpatial, sigmaColor)
TIE = 4.618802070617676                                                  # float32(8 / sqrt(3)): r_1 = 8.0 at one iteration


def _guide(rng, H, W, ch):
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


def _filter(guide, src, ss, sr, N, dst_dtype=None):
    return ref.dt_window_filter(guide, src, ss, sr, ref.radii(ss, N), dst_dtype)


def _scalar_pass(x, L, r, k):
    """One pass along the rows of x, pixel by pixel, as include/adf_wls.h words it.  L[y][j]: the step between j and j + 1."""
    H, n = x.shape
    out = np.empty_like(x)
    for y in range(H):
        for j in range(n):
            lb = j
            while lb > 0:
                S = int(sum(L[y][lb - 1:j]))
                if not np.float32(j - lb + 1) + np.float32(k * np.float32(S)) <= r:
                    break
                lb -= 1
            rb = j
            while rb < n - 1:
                S = int(sum(L[y][j:rb + 1]))
                if not np.float32(rb + 1 - j) + np.float32(k * np.float32(S)) < r:
                    break
                rb += 1
            acc = x[y, lb]
            for p in range(lb + 1, rb + 1):
                acc = np.float32(acc + x[y, p])
            out[y, j] = acc / np.float32(rb - lb + 1)
    return out


def test_a_written_out_scalar_loop_and_the_order_of_the_passes():
    rng = np.random.default_rng(4)
    g, s = _guide(rng, 9, 11, 1), _src16(rng, 9, 11)
    radii, k = ref.radii(4.0, 2), ref.factor(4.0, 30.0)
    assert k.dtype == np.float32 and radii.dtype == np.float32
    Lh, Lv = dt_ref.l1_steps(g)
    x = s.astype(np.float32)
    for r in radii:                                                      # rows come before columns in each iteration
        x = _scalar_pass(x, Lh, r, k)
        x = _scalar_pass(np.ascontiguousarray(x.T), np.ascontiguousarray(Lv.T), r, k).T
    got = ref.iterations(g, s, radii, k)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(x).view(np.uint32))
    # ... and the other order is another filter
    y = s.astype(np.float32)
    for r in radii:
        y = _scalar_pass(np.ascontiguousarray(y.T), np.ascontiguousarray(Lv.T), r, k).T
        y = _scalar_pass(np.ascontiguousarray(y), Lh, r, k)
    assert not np.array_equal(x, y)


def test_an_integer_valued_constant_map_comes_back_exactly():
    rng = np.random.default_rng(1)
    for ch in (1, 3):
        guide = rng.integers(0, 256, (23, 31, ch), dtype=np.uint8)
        guide = guide if ch == 3 else guide[..., 0]
        for ss, sr, N in ((10, 30, 3), (0.5, 0.0, 8), (80, 50, 3), (3, 255, 5)):
            for v, dtype in ((-32768, np.int16), (32767, np.int16), (255, np.uint8), (123456.0, np.float32)):
                src = np.full((23, 31), v, dtype)
                out = _filter(guide, src, ss, sr, N)
                assert out.dtype == src.dtype and np.array_equal(out, src)


def test_a_flat_guide_gives_the_same_result_whatever_its_value():
    rng = np.random.default_rng(2)
    src = _src16(rng, 19, 27)
    for ch in (1, 3):
        shape = (19, 27, 3) if ch == 3 else (19, 27)
        outs = [_filter(np.full(shape, v, np.uint8), src, 8, 20, 3, np.float32) for v in (0, 90, 255)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        assert not np.array_equal(outs[0], src.astype(np.float32))       # and it does smooth


def test_degenerate_shapes():
    rng = np.random.default_rng(3)
    one = np.array([[-1234]], np.int16)
    assert np.array_equal(_filter(np.array([[7]], np.uint8), one, 10, 30, 3), one)
    # W = 1: the rows are left alone, the column is filtered as a 1 x H row would be, and the other way round
    g, s = rng.integers(0, 256, (1, 40), dtype=np.uint8), _src16(rng, 1, 40)
    row = _filter(g, s, 10, 30, 3, np.float32)
    col = _filter(g.T.copy(), s.T.copy(), 10, 30, 3, np.float32)
    assert np.array_equal(row, col.T) and not np.array_equal(row, s.astype(np.float32))
    # ... which is the one-dimensional pass, three times
    x, L = s.astype(np.float32), dt_ref.l1_steps(g)[0]
    for r in ref.radii(10, 3):
        x = _scalar_pass(x, L, r, ref.factor(10, 30))
    assert np.array_equal(row, x)
    # a radius below 1 is an identity pass
    assert np.array_equal(ref.window_pass(x, L, np.float32(0.76), ref.factor(10, 30)), x)


def test_the_tie_at_the_ends_of_a_window(adf):
    radii = adf.dtNcRadii(TIE, 1)
    assert radii.dtype == np.float32 and radii.shape == (1,) and radii[0] == 8.0
    assert ref.radii(TIE, 1)[0] == 8.0
    # a flat guide: D is the pixel distance, an interior window is [j - 8, j + 7] -- the left end included, the right excluded
    L = np.zeros((1, 39), np.int64)
    left, right = ref.windows(L, radii[0], ref.factor(TIE, TIE))
    assert ref.factor(TIE, TIE) == 1.0
    assert (left[0, 8:] == 8).all() and (left[0, :8] == np.arange(8)).all()
    assert (right[0, :32] == 7).all() and (right[0, 32:] == np.arange(7, -1, -1)).all()
    x = np.arange(40, dtype=np.float32)[None] ** 2
    y = ref.window_pass(x, L, radii[0], np.float32(1.0))
    assert y[0, 20] == np.float32(sum(float(v) ** 2 for v in range(12, 28)) / 16)   # 16 taps, exact in float32


def test_library_radii_against_numpy(adf):
    for N in (1, 2, 3, 5, 8):
        for ss in (0.5, 1.0, 3.0, 10.0, 40.0, 80.0, TIE, 1000.0, 12.345678):
            lib, own = adf.dtNcRadii(ss, N), ref.radii(ss, N)
            assert lib.dtype == np.float32 and lib.shape == (N,)
            assert np.array_equal(lib.view(np.uint32), own.view(np.uint32)), (ss, N)   # 0 ulp apart
            assert (np.diff(lib) < 0).all() or N == 1                    # the first iteration has the widest window
    assert adf.dtNcRadii(10, 0).shape == (1,) and adf.dtNcRadii(10, -4).shape == (1,)
    assert np.array_equal(adf.dtNcRadii(0.25, 3), adf.dtNcRadii(1.0, 3))                # the clamp
    assert int(adf.dtNcRadii(80, 3)[0]) == 120 and int(adf.dtNcRadii(10, 3)[0]) == 15


def _cases():
    k = 0
    for ch in (1, 3):
        for H, W in SIZES:
            for N in ITERS:
                for ss, sr in SIGMAS:
                    k += 1
                    yield k, ch, H, W, N, ss, sr


def _reference_pass(x, L, r, k):
    """One pass of the reference's arithmetic along the rows of x (DT.inl:477-494, 211-221, 277-321): float32 running
    distances idist[], a float32 running integral of the row, the bounds found on idist[], the integral differenced."""
    H, n = x.shape
    out = np.empty((H, n), np.float32)
    step = (np.float32(1.0) + (k * L.astype(np.float32)).astype(np.float32)).astype(np.float32)
    for y in range(H):
        idist = np.empty(n + 1, np.float32)
        idist[0] = 0
        idist[1:n] = np.cumsum(step[y], dtype=np.float32)                # sequential float32 adds
        idist[n] = np.finfo(np.float32).max
        integral = np.zeros(n + 1, np.float32)
        integral[1:] = np.cumsum(x[y], dtype=np.float32)
        cur = idist[:n]
        lb = np.searchsorted(idist[:n], cur - r, side="left")            # the first idist >= cur - r
        rb = np.searchsorted(idist, cur + r, side="left") - 1            # the last idist < cur + r
        assert (lb <= np.arange(n)).all() and (rb >= np.arange(n)).all() and (rb <= n - 1).all()
        out[y] = (integral[rb + 1] - integral[lb]) / (rb + 1 - lb).astype(np.float32)
    return out


def _reference_filter(guide, src, ss, sr, N):
    ss, sr, N = dt_ref.clamped(ss, sr, N)
    k = ss / sr
    Lh, Lv = dt_ref.l1_steps(guide)
    x = src.astype(np.float32)
    for i in range(1, N + 1):
        r = np.float32(3.0 * dt_ref.sigma_h(ss, N, i))
        x = _reference_pass(x, Lh, r, k)
        x = np.ascontiguousarray(_reference_pass(np.ascontiguousarray(x.T), np.ascontiguousarray(Lv.T), r, k).T)
    return dt_ref.convert(x, np.int16)


def test_sequential_cumsum_is_what_numpy_gives():
    """_reference_pass leans on np.cumsum adding left to right in float32."""
    v = np.random.default_rng(0).random(1000).astype(np.float32) * 1000
    acc, seq = np.float32(0), []
    for e in v:
        acc = np.float32(acc + e)
        seq.append(acc)
    assert np.array_equal(np.cumsum(v, dtype=np.float32), np.array(seq, np.float32))


@functools.lru_cache(maxsize=None)
def _measured():
    """Per case: (error / bound against float64 sums over the same windows, max and mean |difference| in int16 LSB and the
    share of pixels that differ against the reference's arithmetic, the widest window, N)."""
    out = []
    for c, ch, H, W, N, ss, sr in _cases():
        rng = np.random.default_rng(2000 + c)
        guide, src = _guide(rng, H, W, ch), _src16(rng, H, W)
        radii, k = ref.radii(ss, N), ref.factor(ss, sr)
        x32 = ref.iterations(guide, src, radii, k, np.float32)
        x64 = ref.iterations(guide, src, radii, k, np.float64)
        bound = sum(2 * (2 * int(np.floor(r)) + 1) for r in radii) * 2.0 ** -24 * float(np.abs(src.astype(np.float64)).max())
        err = float(np.abs(x32.astype(np.float64) - x64).max())
        ours = dt_ref.convert(x32, np.int16).astype(np.int64)
        theirs = _reference_filter(guide, src, ss, sr, N).astype(np.int64)
        delta = np.abs(ours - theirs)
        Lh, Lv = dt_ref.l1_steps(guide)
        widest = max(int((l + r + 1).max()) for l, r in (ref.windows(Lh, radii[0], k), ref.windows(Lv.T, radii[0], k)))
        out.append((err / bound, int(delta.max()), float(delta.mean()), float((delta > 0).mean()), widest, N))
    return tuple(out)


def test_distance_to_float64_within_the_derived_bound():
    m = _measured()
    ratios = [c[0] for c in m]
    print("\nfloat32 statement against float64 sums over the same windows, %d cases: worst error / bound %.5f" % (len(m), max(ratios)))
    assert max(ratios) <= 1.0


def test_distance_to_the_reference_arithmetic():
    m = _measured()
    low = [c for c in m if c[5] <= 3]
    print("\nagainst the reference's arithmetic, int16 LSB: max |d| %d, mean |d| %.5f, differing at most %.4f %% over all cases; "
          "N <= 3: max %d, mean %.5f, differing at most %.4f %%; widest window %d pixels"
          % (max(c[1] for c in m), float(np.mean([c[2] for c in m])), 100 * max(c[3] for c in m),
             max(c[1] for c in low), float(np.mean([c[2] for c in low])), 100 * max(c[3] for c in low), max(c[4] for c in m)))
    assert max(c[1] for c in low) <= 1
