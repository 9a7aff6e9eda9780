"""CPU side of the speckle filter (cv::filterSpeckles): the C restatement tests/speckle_ref.c -- the checker of the
device kernels -- against the Python restatement tutorial_replay.remove_speckles and a hand-worked map, and the
argument checks of the Python mirror and the C-ABI that run before any device work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tutorial_replay as tr

HERE = os.path.dirname(os.path.abspath(__file__))
_REF = None


def ref_lib():
    """tests/speckle_ref.c built with gcc into a temporary directory, loaded with ctypes."""
    global _REF
    if _REF is None:
        out = os.path.join(tempfile.mkdtemp(prefix="speckle_ref_"), "libspeckle_ref.so")
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC", os.path.join(HERE, "speckle_ref.c"), "-o", out], check=True)
        L = C.CDLL(out)
        L.speckle_ref.restype = None
        L.speckle_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _REF = L
    return _REF


def speckle_ref(disp, new_val, max_size, max_diff):
    """Filtered copy of a CV_16SC1 map (H,W) or batch (N,H,W) by the C restatement."""
    d = np.array(disp, dtype=np.int16, copy=True, order="C")
    if d.ndim == 3:
        for k in range(d.shape[0]):
            d[k] = speckle_ref(d[k], new_val, max_size, max_diff)
        return d
    H, W = d.shape
    label = np.empty(H * W, np.int32)
    lst = np.empty(H * W, np.int32)
    ref_lib().speckle_ref(d.ctypes.data, W, H, W, int(new_val), int(max_size), int(max_diff),
                          label.ctypes.data, lst.ctypes.data)
    return d


def test_c_reference_equals_python_restatement():
    rng = np.random.default_rng(2024)
    for it in range(200):
        H, W = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        kind = it % 4
        if kind == 0:       # few levels: large components and exact ties
            d = rng.integers(-2, 3, (H, W)) * 16
        elif kind == 1:     # graded values: maxDiff decides
            d = np.cumsum(rng.integers(-3, 4, (H, W)), axis=1) * 8
        elif kind == 2:     # int16 extremes (differ by 65535: int32 arithmetic)
            d = rng.choice(np.array([-32768, -32767, 0, 32766, 32767]), (H, W))
        else:
            d = rng.integers(-40, 40, (H, W))
        d = d.astype(np.int16)
        new_val = int(rng.choice([-16, 0, int(d.flat[0]), -32768, 32767]))     # often a value that occurs in the map
        max_size = int(rng.choice([-1, 0, 1, 2, 3, 5, 8, H * W, H * W + 1]))
        max_diff = int(rng.choice([-1, 0, 1, 2, 16, 32, 65535]))
        exp = tr.remove_speckles(d, new_val, max_size, max_diff)
        got = speckle_ref(d, new_val, max_size, max_diff)
        assert np.array_equal(got, exp), (it, d, new_val, max_size, max_diff)


# 8 x 8 hand-worked map, newVal -16, maxSpeckleSize 4:
#   5-ring 12 px | 9-block 4 px (= max) | 7s 5 px (= max + 1) | 1s 4 px | 3s 3 px | row 4 all newVal |
#   2s split by newVal into 5 px (left) and 4 px (right) | 8s 3 px | 4s of row 7 plus (6,7) 9 px
HAND = np.array([[5, 5, 5, 5, -16, 7, 7, 7],
                 [5, 9, 9, 5, -16, 7, 1, 1],
                 [5, 9, 9, 5, -16, 7, 1, 1],
                 [5, 5, 5, 5, -16, 3, 3, 3],
                 [-16] * 8,
                 [2, 2, 2, -16, 2, 2, 8, 8],
                 [2, 2, -16, -16, 2, 2, 8, 4],
                 [4, 4, 4, 4, 4, 4, 4, 4]], np.int16)


def _removed(*cells):
    m = np.zeros(HAND.shape, bool)
    for y, x in cells:
        m[y, x] = True
    return m


NINE = [(1, 1), (1, 2), (2, 1), (2, 2)]
ONES = [(1, 6), (1, 7), (2, 6), (2, 7)]
THREES = [(3, 5), (3, 6), (3, 7)]
TWOS_RIGHT = [(5, 4), (5, 5), (6, 4), (6, 5)]
EIGHTS = [(5, 6), (5, 7), (6, 6)]


@pytest.mark.parametrize("max_size,max_diff,removed", [
    # maxDiff 0: components of exactly max go, max + 1 stay; the newVal column splits the 2s into 5 + 4
    (4, 0, _removed(*NINE, *ONES, *THREES, *TWOS_RIGHT, *EIGHTS)),
    # maxDiff 2: 1s and 3s join (7 px), 2s join the 4s (row 7) into one large component; 9-block and 8s still go
    (4, 2, _removed(*NINE, *EIGHTS)),
    # negative maxDiff: every pixel is its own component
    (1, -1, HAND != -16),
    (0, -1, np.zeros(HAND.shape, bool)),
    # maxSpeckleSize 0 changes nothing whatever maxDiff is
    (0, 0, np.zeros(HAND.shape, bool)),
])
def test_hand_worked_map(max_size, max_diff, removed):
    exp = np.where(removed, np.int16(-16), HAND)
    assert np.array_equal(speckle_ref(HAND, -16, max_size, max_diff), exp)
    assert np.array_equal(tr.remove_speckles(HAND, -16, max_size, max_diff), exp)


# ---- argument checks of the Python mirror (raised before any device work) ----
def test_filter_speckles_rejects_wrong_dtype():
    import addingdisparityfiltering_amd as adf

    with pytest.raises(adf.AdfError):
        adf.filterSpeckles(np.zeros((4, 4), np.float32), -16, 10, 16)
    with pytest.raises(adf.AdfError):
        adf.filterSpeckles(np.zeros((4, 4), np.int32), -16, 10, 16)


def test_filter_speckles_rejects_8u():
    import addingdisparityfiltering_amd as adf

    with pytest.raises(adf.AdfError) as e:
        adf.filterSpeckles(np.zeros((4, 4), np.uint8), 0, 10, 16)
    assert e.value.code == 1


@pytest.mark.parametrize("nv", [32768, -32769, 1e6, float("nan")])
def test_filter_speckles_rejects_new_val_outside_int16(nv):
    import addingdisparityfiltering_amd as adf

    img = np.zeros((4, 4), np.int16)
    with pytest.raises(adf.AdfError):
        adf.filterSpeckles(img, nv, 10, 16)
    assert not img.any()


def test_filter_speckles_rejects_bad_shapes():
    import addingdisparityfiltering_amd as adf

    for a in (np.zeros(5, np.int16), np.zeros((2, 2, 2, 2), np.int16), np.zeros((0, 4), np.int16)):
        with pytest.raises(adf.AdfError):
            adf.filterSpeckles(a, -16, 10, 16)


# ---- the C-ABI: sizes and the checks that precede any device work ----
def test_c_abi_workspace_and_argument_checks():
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    assert L.adf_filter_speckles_workspace_bytes(1, 3840, 2160) == 8 * 3840 * 2160
    assert L.adf_filter_speckles_workspace_bytes(16, 7, 5) == 16 * 8 * 35
    assert L.adf_filter_speckles_workspace_bytes(0, 7, 5) == 0
    img = np.zeros((4, 4), np.int16)
    p = C.c_void_p(img.ctypes.data)
    # newVal outside int16, empty map, misaligned stride, row stride too small, int32 label range
    assert L.adf_filter_speckles_device(1, p, 8, 32, 4, 4, 40000, 10, 16, None, 0, None) == _lib.ADF_EBADARG
    assert L.adf_filter_speckles_host(1, p, 8, 32, 4, 4, -40000, 10, 16) == _lib.ADF_EBADARG
    assert L.adf_filter_speckles_device(1, p, 8, 32, 0, 4, -16, 10, 16, None, 0, None) == _lib.ADF_EBADARG
    assert L.adf_filter_speckles_device(1, p, 9, 36, 4, 4, -16, 10, 16, None, 0, None) == _lib.ADF_EBADARG
    assert L.adf_filter_speckles_device(1, p, 6, 32, 4, 4, -16, 10, 16, None, 0, None) == _lib.ADF_ESIZE
    assert L.adf_filter_speckles_device(1, p, 2 * 65536, 0, 65536, 32768, -16, 10, 16, None, 0, None) == _lib.ADF_ESIZE
    assert b"2^31" in L.adf_last_error()
    # maps of a batch must not overlap; a caller workspace must be large enough
    assert L.adf_filter_speckles_device(2, p, 8, 16, 4, 4, -16, 10, 16, None, 0, None) == _lib.ADF_ESIZE
    assert L.adf_filter_speckles_device(1, p, 8, 32, 4, 4, -16, 10, 16, p, 127, None) == _lib.ADF_ESIZE
    assert not img.any()
