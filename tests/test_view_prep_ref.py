"""CPU side of the matcher's view preparation (half-size resize + BGR2GRAY, csrc/view_prep_kernels.hip): the exported
symbols and adf_half_size, the refusals of the C-ABI and of the Python mirror that come before any device work, and the
NumPy reference `view_prep_ref` -- the checker of the device kernels -- against tutorial_replay's half_size / bgr2gray
on the tutorial's pair and against hand-worked images for the odd-size tail."""
import ctypes as C

import numpy as np
import pytest

import tutorial_replay as tr


def half_of(n):
    """cvRound(n * 0.5), round half to even."""
    k = n // 2
    return k + (n & 1 & k)


def _round_half_even_div(s, n):
    """cvRound(s / n) for n in (1, 2, 4) on non-negative integer arrays, half to even."""
    q, r = s // n, s % n
    up = (2 * r > n) | ((2 * r == n) & (q % 2 == 1))
    return q + up


def view_prep_ref(img, half, gray):
    """(H,W) / (H,W,3) uint8 image, or a batch (N,H,W) / (N,H,W,3) when img.ndim says so through `batch_ref`.
    half: the 2x2 mean (a+b+c+d+2) >> 2 onto (half_of(H), half_of(W)); a last column / row with a single source
    column / row is the mean over the pixels that exist, cvRound(sum / count) half to even.  gray: 14-bit BGR2GRAY on
    the (rounded) 8-bit channels."""
    a = img.astype(np.int64)
    if half:
        H, W = a.shape[:2]
        h, w = half_of(H), half_of(W)
        out = np.empty((h, w) + a.shape[2:], np.int64)
        for y in range(h):
            ys = [r for r in (2 * y, 2 * y + 1) if r < H]
            rows = a[ys].sum(axis=0)                                        # (W[,3])
            wf = min(w, W // 2)                                             # whole cells
            cells = rows[0:2 * wf:2] + rows[1:2 * wf:2]
            n = 2 * len(ys)
            out[y, :wf] = (cells + 2) >> 2 if n == 4 else _round_half_even_div(cells, n)
            if wf < w:                                                      # one source column left
                out[y, wf] = _round_half_even_div(rows[2 * wf], len(ys))
        a = out
    if gray:
        a = (a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + (1 << 13)) >> 14
    return a.astype(np.uint8)


def batch_ref(imgs, half, gray):
    return np.stack([view_prep_ref(i, half, gray) for i in imgs])


# ---- 1. symbols and adf_half_size ----
def test_symbols_are_exported():
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for name in ("adf_prepare_views_device", "adf_prepare_views_host", "adf_half_size"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("n,exp", [(0, 0), (1, 0), (2, 1), (3, 2), (5, 2), (375, 188), (1242, 621), (1243, 622)])
def test_half_size_rounds_half_to_even(n, exp):
    import addingdisparityfiltering_amd as adf
    from addingdisparityfiltering_amd import _lib

    v = C.c_int(-1)
    assert _lib.lib().adf_half_size(n, C.byref(v)) == _lib.ADF_OK
    assert v.value == exp == half_of(n) == int(np.round(n * 0.5))          # numpy rounds half to even too
    assert adf.halfSize(n) == exp


def test_half_size_refusals():
    from addingdisparityfiltering_amd import _lib

    v = C.c_int(7)
    assert _lib.lib().adf_half_size(-1, C.byref(v)) == _lib.ADF_EBADARG
    assert _lib.lib().adf_half_size(4, None) == _lib.ADF_EBADARG
    assert v.value == 7


# ---- 2. refusals, before any device is touched (this suite runs without a GPU) ----
def _call(entry, n, src, sstride, simage, W, H, sc, dst, dstride, dimage, dW, dH, dc):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    sp = C.c_void_p(src.ctypes.data) if src is not None else None
    dp = C.c_void_p(dst.ctypes.data) if dst is not None else None
    args = [n, sp, sstride, simage, W, H, sc, dp, dstride, dimage, dW, dH, dc]
    rc = L.adf_prepare_views_device(*args, None) if entry == "device" else L.adf_prepare_views_host(*args)
    return rc, L.adf_last_error()


@pytest.mark.parametrize("entry", ["device", "host"])
def test_c_abi_refusals(entry):
    from addingdisparityfiltering_amd import _lib

    src = np.zeros((8, 8, 3), np.uint8)
    dst = np.full((8, 8, 3), 0x5A, np.uint8)
    bad = [
        # W, H -> dW, dH that are neither the same size nor half of it
        dict(dW=2, dH=2),                                   # a quarter
        dict(dW=8, dH=4),                                   # half in one direction only
        dict(dW=16, dH=16),                                 # twice
        dict(dW=5, dH=4), dict(dW=4, dH=3), dict(dW=3, dH=4),   # half size off by one
        dict(dW=8, dH=8, dc=3),                             # same size, same channels: not a case
        dict(sc=1, dc=3),                                   # 1 -> 3 channels
        dict(sc=4, dc=1), dict(sc=4, dc=4), dict(sc=3, dc=4), dict(sc=2, dc=1), dict(sc=3, dc=2),
        dict(n=0), dict(n=-3),
        dict(src=None), dict(dst=None),
        dict(sstride=23),                                   # a source row is 24 bytes
        dict(dstride=3),                                    # a destination row is 4 bytes
        dict(sstride=-24),
        dict(W=0), dict(H=0),
    ]
    for kw in bad:
        a = dict(n=1, src=src, sstride=24, simage=192, W=8, H=8, sc=3, dst=dst, dstride=24, dimage=192, dW=4, dH=4, dc=1)
        a.update(kw)
        rc, msg = _call(entry, **a)
        assert rc == _lib.ADF_EBADARG, (kw, rc, msg)
        assert msg, kw
    # odd sizes: the half size is cvRound, so 7 -> 4 and 5 -> 2, not the floor / the ceiling
    for W, dW_ok, dW_bad in ((7, 4, 3), (5, 2, 3)):
        a = dict(n=1, src=src, sstride=24, simage=192, W=W, H=8, sc=3, dst=dst, dstride=24, dimage=192, dW=dW_bad, dH=4, dc=1)
        rc, msg = _call(entry, **a)
        assert rc == _lib.ADF_EBADARG and msg, (W, dW_bad)
    # overlapping destination images of a batch
    rc, msg = _call(entry, n=2, src=src, sstride=24, simage=0, W=8, H=4, sc=3, dst=dst, dstride=24, dimage=2, dW=4, dH=2, dc=1)
    assert rc == _lib.ADF_EBADARG and b"overlap" in msg
    assert np.all(dst == 0x5A), "a refused call wrote to dst"


def test_python_refusals():
    import addingdisparityfiltering_amd as adf

    img = np.zeros((8, 8, 3), np.uint8)
    gray = np.zeros((8, 8), np.uint8)
    for kw in (dict(fx=0.25, fy=0.25), dict(fx=0.5, fy=0.25), dict(fx=1.0, fy=1.0), dict(), dict(fx=2, fy=2),
               dict(dsize=(2, 2)), dict(dsize=(4, 3)), dict(dsize=(8, 8)), dict(fx=0.5, fy=0.5, interpolation=0)):
        with pytest.raises(adf.AdfError) as e:
            adf.resize(img, **kw)
        assert e.value.code == 1, kw
    for code in (7, 0, 10, None):                           # (7 = COLOR_RGB2GRAY)
        with pytest.raises(adf.AdfError) as e:
            adf.cvtColor(img, code)
        assert e.value.code == 1
    with pytest.raises(adf.AdfError):
        adf.cvtColor(gray, adf.COLOR_BGR2GRAY)             # needs three channels
    with pytest.raises(adf.AdfError):
        adf.resize(np.zeros((2, 8, 8, 4), np.uint8), fx=0.5, fy=0.5)       # four channels
    with pytest.raises(adf.AdfError):
        adf.resize(np.zeros((8, 8, 3), np.int16), fx=0.5, fy=0.5)          # 8-bit only
    with pytest.raises(adf.AdfError):
        adf.resize(np.zeros((1, 1), np.uint8), fx=0.5, fy=0.5)             # the half-size image is empty
    with pytest.raises(adf.AdfError):
        adf.matcherViews(img, scale=0.25)
    with pytest.raises(adf.AdfError):
        adf.matcherViews(gray, scale=1.0)                  # nothing to do
    with pytest.raises(adf.AdfError):
        adf.matcherViews(img, scale=0.5, dst=np.zeros((4, 5), np.uint8))   # dst of the wrong size
    assert adf.COLOR_BGR2GRAY == 6 and adf.INTER_LINEAR == 1


# ---- 3. the NumPy reference ----
def test_reference_equals_the_replay_on_the_tutorial_pair():
    left, right, _, _ = tr.load_fixtures()
    assert left.shape == (436, 1024, 3)
    for v in (left, right):
        assert np.array_equal(view_prep_ref(v, True, False), tr.half_size(v))
        assert np.array_equal(view_prep_ref(v, False, True), tr.bgr2gray(v))
        assert np.array_equal(view_prep_ref(v, True, True), tr.bgr2gray(tr.half_size(v)))
        assert np.array_equal(view_prep_ref(v[:, :, 1], True, False), tr.half_size(v[:, :, 1]))
    gl, gr, _ = tr.matcher_views(left, right)
    assert np.array_equal(batch_ref([left, right], True, True), np.stack([gl, gr]))


def test_reference_equals_the_replay_on_random_even_sizes():
    rng = np.random.default_rng(5)
    for H, W in ((2, 2), (4, 6), (64, 64), (10, 1024)):
        v = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(view_prep_ref(v, True, False), tr.half_size(v))
        assert np.array_equal(view_prep_ref(v, True, True), tr.bgr2gray(tr.half_size(v)))


def test_hand_worked_3x3():
    # 3 x 3 -> 2 x 2: one whole cell, a single-column cell (2 px), a single-row cell (2 px), a corner (1 px)
    img = np.array([[1, 2, 9],
                    [3, 4, 10],
                    [5, 8, 7]], np.uint8)
    # (1+2+3+4+2)>>2 = 3   (10/4 = 2.5: the whole cell rounds half UP)
    # (9+10)/2 = 9.5 -> 10 (half to even)         (5+8)/2 = 6.5 -> 6 (half to even)        7
    assert np.array_equal(view_prep_ref(img, True, False), np.array([[3, 10], [6, 7]], np.uint8))
    img2 = np.array([[0, 2, 0],
                     [0, 0, 1],
                     [2, 1, 255]], np.uint8)
    # (2+2)>>2 = 1 (0.5 rounds up in a whole cell)   (0+1)/2 = 0.5 -> 0   (2+1)/2 = 1.5 -> 2   255
    assert np.array_equal(view_prep_ref(img2, True, False), np.array([[1, 0], [2, 255]], np.uint8))


def test_hand_worked_5x2():
    # W = 5, H = 2 -> 2 x 1 (cvRound(2.5) = 2): the fifth column is dropped, both cells are whole
    img = np.array([[10, 20, 1, 1, 200],
                    [30, 41, 1, 2, 200]], np.uint8)
    # (10+20+30+41+2)>>2 = 103>>2 = 25       (1+1+1+2+2)>>2 = 7>>2 = 1
    assert np.array_equal(view_prep_ref(img, True, False), np.array([[25, 1]], np.uint8))
    # W = 2, H = 5 -> 1 x 2 likewise
    assert np.array_equal(view_prep_ref(np.ascontiguousarray(img.T), True, False), np.array([[25], [1]], np.uint8))
    # W = 7 -> 4: three whole cells and column 6 alone
    row = np.array([[1, 2, 3, 4, 5, 6, 9], [1, 2, 3, 4, 5, 7, 12]], np.uint8)
    # (1+2+1+2+2)>>2 = 2, (3+4+3+4+2)>>2 = 4, (5+6+5+7+2)>>2 = 6, (9+12)/2 = 10.5 -> 10
    assert np.array_equal(view_prep_ref(row, True, False), np.array([[2, 4, 6, 10]], np.uint8))


def test_hand_worked_gray_and_fused():
    px = np.array([[[255, 255, 255], [0, 0, 0]],
                   [[255, 0, 0], [0, 0, 255]]], np.uint8)
    # white: (1868+9617+4899)*255 + 8192 = 16384*255 + 8192 -> 255;  blue 255: (476340+8192)>>14 = 29;  red: (1249245+8192)>>14 = 76
    assert np.array_equal(view_prep_ref(px, False, True), np.array([[255, 0], [29, 76]], np.uint8))
    # fused: channels first (B: (255+0+255+0+2)>>2 = 128, G: (255+2)>>2 = 64, R: (255+0+0+255+2)>>2 = 128), then gray
    g = (128 * 1868 + 64 * 9617 + 128 * 4899 + 8192) >> 14
    assert np.array_equal(view_prep_ref(px, True, True), np.array([[g]], np.uint8))
    assert np.array_equal(view_prep_ref(px, True, True), view_prep_ref(view_prep_ref(px, True, False), False, True))
