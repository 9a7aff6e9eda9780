"""CPU pins on the statement of the domain transform filter's recursive mode (tests/dt_ref.py; include/adf_wls.h): its
invariants, its degenerate shapes, the layout of the feedback table, the library's host table against NumPy's exp, the
distance to a float64 evaluation of the same recurrence (bound derived in DESIGN.md, section 22) and the measured distance
to the reference's own table arithmetic (DT.inl:401-405, 539-561).  Run with -s to see the measured figures."""
import functools

import numpy as np
import pytest

import dt_ref

SIZES = [(5, 300), (37, 41), (130, 129)]                                # (H, W)
ITERS = [1, 3, 5]
SIGMAS = [(10.0, 30.0), (40.0, 10.0), (3.0, 255.0), (1000.0, 0.01)]     # (sigmaSpatial, sigmaColor)


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


def _cases():
    k = 0
    for ch in (1, 3):
        for H, W in SIZES:
            for N in ITERS:
                for ss, sr in SIGMAS:
                    k += 1
                    yield k, ch, H, W, N, ss, sr


def test_a_constant_map_comes_back_exactly():
    rng = np.random.default_rng(1)
    for ch in (1, 3):
        guide = rng.integers(0, 256, (23, 31, ch), dtype=np.uint8)
        guide = guide if ch == 3 else guide[..., 0]
        for ss, sr, N in ((10, 30, 3), (0.5, 0.0, 8), (1000, 0.01, 1), (3, 255, 5)):
            table = dt_ref.rf_table(ss, sr, N, ch)
            for v, dtype in ((-32768, np.int16), (32767, np.int16), (255, np.uint8), (123456.789, np.float32), (-0.1, np.float32)):
                src = np.full((23, 31), v, dtype)
                out = dt_ref.dt_filter(guide, src, table)
                assert out.dtype == src.dtype and np.array_equal(out, src)


def test_a_flat_guide_gives_the_same_result_whatever_its_value():
    rng = np.random.default_rng(2)
    src = _src16(rng, 19, 27)
    for ch in (1, 3):
        table = dt_ref.rf_table(8, 20, 3, ch)
        shape = (19, 27, 3) if ch == 3 else (19, 27)
        outs = [dt_ref.dt_filter(np.full(shape, v, np.uint8), src, table, np.float32) for v in (0, 90, 255)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        assert not np.array_equal(outs[0], src.astype(np.float32))       # and it does smooth
        # only A[0] was read
        other = table.copy()
        other[:, 1:] = 0.5
        assert np.array_equal(dt_ref.dt_filter(np.full(shape, 7, np.uint8), src, other, np.float32), outs[0])


def test_degenerate_shapes():
    rng = np.random.default_rng(3)
    table = dt_ref.rf_table(10, 30, 3, 1)
    one = np.array([[-1234]], np.int16)
    assert np.array_equal(dt_ref.dt_filter(np.array([[7]], np.uint8), one, table), one)
    # W = 1: the rows are left alone, the column is filtered as a 1 x H row would be, and the other way round
    g, s = rng.integers(0, 256, (1, 40), dtype=np.uint8), _src16(rng, 1, 40)
    row = dt_ref.dt_filter(g, s, table, np.float32)
    col = dt_ref.dt_filter(g.T.copy(), s.T.copy(), table, np.float32)
    assert np.array_equal(row, col.T) and not np.array_equal(row, s.astype(np.float32))
    # ... which is the one-dimensional recurrence written out
    x, a = s[0].astype(np.float32), table[:, np.abs(np.diff(g[0].astype(np.int64)))]
    for i in range(3):
        for j in range(1, 40):
            x[j] = x[j] + a[i, j - 1] * (x[j - 1] - x[j])
        for j in range(38, -1, -1):
            x[j] = x[j] + a[i, j] * (x[j + 1] - x[j])
    assert np.array_equal(row[0], x)


def test_the_order_is_rows_first_then_columns_per_iteration():
    rng = np.random.default_rng(4)
    g, s = _guide(rng, 9, 11, 1), _src16(rng, 9, 11)
    table = dt_ref.rf_table(10, 30, 2, 1)
    x = s.astype(np.float32)
    Lh, Lv = dt_ref.l1_steps(g)
    for i in range(2):
        for y in range(9):
            for j in range(1, 11):
                x[y, j] = x[y, j] + table[i, Lh[y, j - 1]] * (x[y, j - 1] - x[y, j])
            for j in range(9, -1, -1):
                x[y, j] = x[y, j] + table[i, Lh[y, j]] * (x[y, j + 1] - x[y, j])
        for c in range(11):
            for y in range(1, 9):
                x[y, c] = x[y, c] + table[i, Lv[y - 1, c]] * (x[y - 1, c] - x[y, c])
            for y in range(7, -1, -1):
                x[y, c] = x[y, c] + table[i, Lv[y, c]] * (x[y + 1, c] - x[y, c])
    assert np.array_equal(dt_ref.dt_filter(g, s, table, np.float32), x)


def test_table_layout_and_distances():
    for ch in (1, 3):
        t = dt_ref.rf_table(10, 30, 3, ch)
        assert t.shape == (3, 255 * ch + 1) and t.dtype == np.float32
        assert (t[0] >= t[1]).all() and (t[1] >= t[2]).all() and t[0, 0] > t[2, 0]   # row 0 = iteration 1, the widest sigmaH
        assert (np.diff(t.astype(np.float64), axis=1) <= 0).all()                      # falls with the guide difference
    ss, sr, N = dt_ref.clamped(10, 30, 3)
    d = dt_ref.distances(ss, sr, 3)
    k = np.float32(10) / np.float32(30)
    assert d[0] == np.float32(1.0) and d[765] == np.float32(1.0) + np.float32(k * np.float32(765))
    assert d.dtype == np.float32
    # A_1[0] = exp(-sqrt(2/3) / sigmaH_1), sigmaH_1 = ss 2^(N-1) / sqrt(4^N - 1)
    assert dt_ref.rf_table(10, 30, 3, 1)[0, 0] == np.float32(np.exp(-np.sqrt(2.0 / 3.0) / (10.0 * 4.0 / np.sqrt(63.0))))
    # the clamps
    assert dt_ref.clamped(0.5, 0.0, 0) == (np.float32(1.0), np.float32(0.01), 1)
    assert np.array_equal(dt_ref.rf_table(0.5, 0.0, 0, 1), dt_ref.rf_table(1.0, 0.01, 1, 1))


def _ulp_apart(a, b):
    """|a - b| in units of the last place of float32, for non-negative finite floats."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_library_table_against_numpy(adf):
    worst = 0
    for ch in (1, 3):
        for N in (1, 3, 5, 8):
            for ss, sr in SIGMAS + [(0.5, 0.0), (1.0, 1.0), (255.0, 3.0)]:
                lib, ref = adf.dtRfTable(ss, sr, N, ch), dt_ref.rf_table(ss, sr, N, ch)
                assert lib.shape == ref.shape and lib.dtype == np.float32
                assert (lib >= 0).all() and (lib <= 1).all()
                worst = max(worst, int(_ulp_apart(lib, ref).max()))
    print("\ndtRfTable against NumPy's exp: worst difference %d ulp" % worst)
    assert worst <= 1


def _reference_table(ss, sr, N, ch):
    """The feedback the reference's arithmetic arrives at (DT.hpp:130-133, DT.inl:401-405, 539-561), as a table: alpha and
    log(alpha) rounded to float, one float exp, and the float plane squared in place for every later iteration."""
    ss, sr, N = dt_ref.clamped(ss, sr, N)
    alpha = np.float32(np.exp(-np.sqrt(2.0 / 3.0) / dt_ref.sigma_h(ss, N, 1)))
    lna = np.log(alpha)
    assert lna.dtype == np.float32
    rows = [np.exp((lna * dt_ref.distances(ss, sr, ch)).astype(np.float32))]
    assert rows[0].dtype == np.float32
    for _ in range(1, N):
        rows.append(rows[-1] * rows[-1])
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _measured():
    """Per case: (error / bound against float64, share of int16 outputs that differ from the float64 ones, max and mean
    |difference| in int16 LSB against the reference's table arithmetic, N)."""
    out = []
    for k, ch, H, W, N, ss, sr in _cases():
        rng = np.random.default_rng(1000 + k)
        guide, src = _guide(rng, H, W, ch), _src16(rng, H, W)
        table = dt_ref.rf_table(ss, sr, N, ch)
        x32 = dt_ref.recurrence(guide, src, table, np.float32)
        x64 = dt_ref.recurrence(guide, src, table, np.float64)
        bound = 12.0 * N * max(W, H) * 2.0 ** -24 * float(np.abs(src.astype(np.float64)).max())
        err = float(np.abs(x32.astype(np.float64) - x64).max())
        differ = float((dt_ref.convert(x32, np.int16) != dt_ref.convert(x64, np.int16)).mean())
        ours = dt_ref.convert(x32, np.int16).astype(np.int64)
        theirs = dt_ref.dt_filter(guide, src, _reference_table(ss, sr, N, ch), np.int16).astype(np.int64)
        delta = np.abs(ours - theirs)
        out.append((err / bound, differ, int(delta.max()), float(delta.mean()), N))
    return tuple(out)


def test_distance_to_float64_within_the_derived_bound():
    m = _measured()
    ratios = [c[0] for c in m]
    print("\nfloat32 statement against float64, %d cases: worst error / bound %.5f; int16 outputs that differ: at most %.4f %%"
          % (len(m), max(ratios), 100 * max(c[1] for c in m)))
    assert max(ratios) <= 1.0


def test_distance_to_the_reference_arithmetic():
    m = _measured()
    print("\nagainst the reference's table arithmetic, int16 LSB: max |d| %d, mean |d| %.5f over all cases; N <= 3: max %d, mean %.5f"
          % (max(c[2] for c in m), float(np.mean([c[3] for c in m])),
             max(c[2] for c in m if c[4] <= 3), float(np.mean([c[3] for c in m if c[4] <= 3]))))
    assert max(c[2] for c in m if c[4] <= 3) <= 1
