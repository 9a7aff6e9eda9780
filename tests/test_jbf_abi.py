"""CPU tests of the joint bilateral filter's refusals (include/adf_wls.h): every one returns its status before a device is
touched -- this file runs without a GPU, through both entry kinds -- with the status the guided filter gives for the same
cause, and the Python wrapper raises the same ones; the table entry point against the NumPy statement; the symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import jbf_ref

EBADARG, ESIZE = 1, 2
U8, S16, S32, F32 = 0, 3, 4, 5
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
H, W = 6, 8


def _good():
    """The arguments of a call that would be accepted, by name."""
    return dict(n=1, joint=np.zeros((H, W), np.uint8), jch=1, src=np.zeros((H, W), np.int16), sdepth=S16,
                dst=np.zeros((H, W), np.int16), ddepth=S16, W=W, H=H, d=5, sc=25.0, ss=3.0, border=REFLECT_101,
                strides={}, offsets={})


def _status(adf, kind, **change):
    from addingdisparityfiltering_amd import _lib

    a = _good()
    a.update(change)
    L = _lib.lib()

    def img(name):
        arr = a[name]
        if arr is None:
            return (None, 0, 0)
        if isinstance(arr, int):
            return (arr, a["strides"].get(name, W * 4), 0)
        return (arr.ctypes.data + a["offsets"].get(name, 0), a["strides"].get(name, arr.strides[0]), a["strides"].get(name + "_map", 0))

    j, s, d = img("joint"), img("src"), img("dst")
    args = (a["n"], j[0], j[1], j[2], a["jch"], s[0], s[1], s[2], a["sdepth"], d[0], d[1], d[2], a["ddepth"], a["W"], a["H"],
            a["d"], a["sc"], a["ss"], a["border"])
    if kind == "device":
        return L.adf_joint_bilateral_filter_device(*args, None)
    return L.adf_joint_bilateral_filter_host(*args)


def _last_error():
    from addingdisparityfiltering_amd import _lib

    return _lib.lib().adf_last_error()


KINDS = ["host", "device"]


def test_symbols_and_constants(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for name in ("adf_joint_bilateral_filter_device", "adf_joint_bilateral_filter_host", "adf_jbf_tables_host"):
        assert hasattr(L, name)
    assert not hasattr(L, "adf_joint_bilateral_filter_workspace_bytes")                     # there is no workspace
    assert (adf.BORDER_CONSTANT, adf.BORDER_REPLICATE, adf.BORDER_REFLECT, adf.BORDER_WRAP, adf.BORDER_REFLECT_101) == (0, 1, 2, 3, 4)
    assert adf.BORDER_DEFAULT == adf.BORDER_REFLECT_101 and adf.JBF_MAX_RADIUS == 31        # cv's enum values
    assert callable(adf.jointBilateralFilter) and callable(adf.jbfTables)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "adf_wls.h")).read()
    for line in ("#define ADF_JBF_MAX_RADIUS 31", "#define ADF_BORDER_REPLICATE 1", "#define ADF_BORDER_REFLECT 2", "#define ADF_BORDER_REFLECT_101 4"):
        assert line in header


@pytest.mark.parametrize("kind", KINDS)
def test_border_types(adf, kind):
    for border, name in ((CONSTANT, b"BORDER_CONSTANT"), (WRAP, b"BORDER_WRAP")):
        assert _status(adf, kind, border=border) == EBADARG
        assert b"not built" in _last_error() and name in _last_error()
    for border in (-1, 5, 16, 100):                                                         # (16 is cv's BORDER_ISOLATED)
        assert _status(adf, kind, border=border) == EBADARG
        assert b"not built" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_parameters(adf, kind):
    for bad in (float("nan"), float("inf"), float("-inf"), 1e300, -1e300):   # (1e300 is not finite as float32)
        assert _status(adf, kind, sc=bad) == EBADARG
        assert _status(adf, kind, ss=bad) == EBADARG
    for d in (64, 65, 1000, (1 << 31) - 1):                                  # r = d / 2 above 31
        assert _status(adf, kind, d=d) == EBADARG
        assert b"radius" in _last_error()
    for d in (0, -1):                                                        # r = cvRound(1.5 sigmaSpace) above 31: 31.5 -> 32
        assert _status(adf, kind, d=d, ss=21.0) == EBADARG
        assert _status(adf, kind, d=d, ss=1e30) == EBADARG
        assert b"radius" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_depths_and_channels(adf, kind):
    for depth in (S32, 1, 2, 6, -1):
        assert _status(adf, kind, sdepth=depth) == EBADARG
        assert _status(adf, kind, ddepth=depth) == EBADARG
    for jch in (0, 2, 4, -1):
        assert _status(adf, kind, jch=jch) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
def test_null_empty_and_joint_is_src(adf, kind):
    for name in ("joint", "src", "dst"):
        assert _status(adf, kind, **{name: None}) == EBADARG
    for k in ("n", "W", "H"):
        assert _status(adf, kind, **{k: 0}) == EBADARG
        assert _status(adf, kind, **{k: -3}) == EBADARG
    same = np.zeros((H, W), np.uint8)
    assert _status(adf, kind, joint=same, src=same, sdepth=U8) == EBADARG
    assert b"not built" in _last_error() and b"bilateralFilter" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_misalignment(adf, kind):
    big16 = np.zeros((H + 1, W + 4), np.int16)
    for name in ("src", "dst"):
        assert _status(adf, kind, **{name: big16}, offsets={name: 1}) == EBADARG           # base
        assert _status(adf, kind, **{name: big16}, strides={name: 2 * W + 1}) == EBADARG    # row stride
        assert _status(adf, kind, **{name: big16}, strides={name + "_map": 1001}) == EBADARG
    big32 = np.zeros((H + 1, W + 4), np.float32)
    for name, depth in (("src", "sdepth"), ("dst", "ddepth")):                              # each aligned to its OWN depth
        for off in (1, 2):
            assert _status(adf, kind, **{name: big32, depth: F32}, offsets={name: off}) == EBADARG
        assert _status(adf, kind, **{name: big32, depth: F32}, strides={name: 4 * W + 2}) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
def test_overlap(adf, kind):
    buf = np.zeros((2 * H, W), np.int16)
    assert _status(adf, kind, src=buf[:H], dst=buf[:H]) == EBADARG                          # in place
    assert _status(adf, kind, src=buf[:H], dst=buf[H - 1:2 * H - 1]) == EBADARG             # one row shared
    b8 = np.zeros((2 * H, 2 * W), np.uint8)
    assert _status(adf, kind, joint=b8[:H], dst=b8[:H].view(np.int16), strides={"joint": 2 * W}) == EBADARG
    assert _status(adf, kind, joint=b8[:H], dst=b8[:H], ddepth=U8, strides={"joint": 2 * W, "dst": 2 * W}) == EBADARG
    # maps of a batch: the destination's must not overlap each other
    two = np.zeros((2, H, W), np.int16)
    assert _status(adf, kind, n=2, src=two, dst=np.zeros((2, H, W), np.int16),
                   strides={"src_map": two.strides[0], "dst_map": two.strides[0] - 2, "joint_map": 0}) == ESIZE


@pytest.mark.parametrize("kind", KINDS)
def test_sizes(adf, kind):
    assert _status(adf, kind, W=65536, H=32768, joint=1 << 20, src=1 << 21, dst=1 << 22,
                   strides={"joint": 65536, "src": 131072, "dst": 131072}) == ESIZE          # W*H = 2^31
    for name, short in (("src", 2 * W - 2), ("dst", 2 * W - 2), ("joint", W - 1)):
        assert _status(adf, kind, strides={name: short}) == ESIZE
    assert _status(adf, kind, jch=3, joint=np.zeros((H, W, 3), np.uint8), strides={"joint": 3 * W - 1}) == ESIZE
    # a destination row is measured in the DESTINATION's depth
    assert _status(adf, kind, ddepth=F32, dst=np.zeros((H, W), np.float32), strides={"dst": 4 * W - 4}) == ESIZE
    assert _status(adf, kind, ddepth=U8, dst=np.zeros((H, W), np.uint8), strides={"dst": W - 1}) == ESIZE


def _ulps(a, b):
    """The distance of two float32 arrays of one sign in units of the last place, on the bits (denormals and zeros too)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_tables_entry_point(adf):
    """Both sides round a double exp that is faithful to under one double ulp to float32: the two roundings can differ by
    one step of the last place and no more."""
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for d, sc, ss, ch in ((5, 25.0, 3.0, 1), (9, 3.0, 0.5, 3), (-1, 1000.0, 8.0, 3), (0, 0.0, -2.0, 1), (63, 40.0, 100.0, 1),
                          (-1, 0.37, 20.9, 3), (17, 255.0, 1e-3, 1)):
        colour, space, r = adf.jbfTables(d, sc, ss, ch)
        C_, S_, r_ = jbf_ref.tables(d, sc, ss, ch)
        assert r == r_ and colour.dtype == space.dtype == np.float32
        assert colour.shape == (255 * ch + 1,) and space.shape == (r * r + 1,)
        assert colour[0] == 1.0 and space[0] == 1.0
        assert (colour >= 0).all() and (space >= 0).all() and (np.diff(colour) <= 0).all() and (np.diff(space) <= 0).all()
        assert _ulps(colour, C_).max() <= 1 and _ulps(space, S_).max() <= 1
    # exactly the stated lengths are written, and the radius alone may be asked for
    c = np.full(766 + 1, -7.0, np.float32)
    s = np.full(16 + 1 + 1, -7.0, np.float32)
    r = C.c_int(-1)
    assert L.adf_jbf_tables_host(9, 25.0, 3.0, 3, c.ctypes.data, s.ctypes.data, C.byref(r)) == 0
    assert r.value == 4 and c[-1] == -7.0 and s[-1] == -7.0 and (c[:-1] >= 0).all() and (s[:-1] > 0).all()
    assert np.array_equal(c[:-1], adf.jbfTables(9, 25.0, 3.0, 3)[0]) and np.array_equal(s[:-1], adf.jbfTables(9, 25.0, 3.0, 3)[1])
    r = C.c_int(-1)
    assert L.adf_jbf_tables_host(-1, 25.0, 3.0, 1, None, None, C.byref(r)) == 0 and r.value == 4      # cvRound(4.5) = 4
    assert L.adf_jbf_tables_host(-1, 25.0, 1.0, 1, None, None, C.byref(r)) == 0 and r.value == 2      # cvRound(1.5) = 2
    assert L.adf_jbf_tables_host(9, 25.0, 3.0, 3, c.ctypes.data, None, C.byref(r)) == EBADARG
    assert L.adf_jbf_tables_host(9, 25.0, 3.0, 3, c.ctypes.data, s.ctypes.data, None) == 0
    # the clamps: the calls and the tables agree on them
    for a, b in (((5, 0.0, -1.0, 1), (5, 1.0, 1.0, 1)), ((1, 9.0, 2.0, 3), (3, 9.0, 2.0, 3)), ((0, 9.0, 2.0, 1), (6, 9.0, 2.0, 1))):
        ta, tb = adf.jbfTables(*a), adf.jbfTables(*b)
        assert ta[2] == tb[2] and np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    for bad in ((5, float("nan"), 3.0, 1), (5, 25.0, float("inf"), 1), (5, 25.0, 3.0, 2), (64, 25.0, 3.0, 1), (0, 25.0, 21.0, 1)):
        assert L.adf_jbf_tables_host(*bad, c.ctypes.data, s.ctypes.data, C.byref(r)) == EBADARG
        with pytest.raises(adf.AdfError):
            adf.jbfTables(*bad)


def test_python_wrapper_refuses(adf):
    joint, src = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16)

    def code(*args, **kw):
        with pytest.raises(adf.AdfError) as e:
            adf.jointBilateralFilter(*args, **kw)
        return e.value.code, str(e.value)

    for border, name in ((adf.BORDER_CONSTANT, "BORDER_CONSTANT"), (adf.BORDER_WRAP, "BORDER_WRAP")):
        c, msg = code(joint, src, 5, 25, 3, border)
        assert c == EBADARG and "not built" in msg and name in msg
    for border in (7, 16, None):
        assert code(joint, src, 5, 25, 3, border)[0] == EBADARG
    c, msg = code(joint.astype(np.float32), src, 5, 25, 3)                                  # 32-bit joints
    assert c == EBADARG and "not built" in msg
    assert code(joint.astype(np.int32), src, 5, 25, 3)[0] == EBADARG
    assert code(joint.astype(np.int16), src, 5, 25, 3)[0] == EBADARG
    c, msg = code(np.zeros((2, H, W), np.uint8), np.zeros((2, H, W, 3), np.int16), 5, 25, 3)   # multi-channel sources
    assert c == EBADARG and "not built" in msg
    same = np.zeros((H, W), np.uint8)
    c, msg = code(same, same, 5, 25, 3)                                                     # joint is src
    assert c == EBADARG and "not built" in msg
    c, msg = code(None, src, 5, 25, 3)                                                      # an empty joint
    assert c == EBADARG and "not built" in msg
    assert code(joint, None, 5, 25, 3)[0] == EBADARG
    for bad in (float("nan"), float("inf")):
        assert code(joint, src, 5, bad, 3)[0] == EBADARG and code(joint, src, 5, 25, bad)[0] == EBADARG
    assert code(joint, src, 64, 25, 3)[0] == EBADARG and code(joint, src, -1, 25, 21.0)[0] == EBADARG
    assert code(joint, src.astype(np.int32), 5, 25, 3)[0] == EBADARG                        # depth
    assert code(joint, src.astype(np.float64), 5, 25, 3)[0] == EBADARG
    assert code(joint, src, 5, 25, 3, dDepth=4)[0] == EBADARG                               # CV_32S
    assert code(np.zeros((H, W, 2), np.uint8), src, 5, 25, 3)[0] == EBADARG                 # channel count
    assert code(joint, src, 5, 25, 3, dst=src)[0] == EBADARG                                # overlap
    assert code(joint, src, 5, 25, 3, dst=np.zeros((H, W), np.float32))[0] == EBADARG       # dst of another depth than dDepth
    assert code(np.zeros((H, W + 1), np.uint8), src, 5, 25, 3)[0] == ESIZE
    assert code(joint, src, 5, 25, 3, dst=np.zeros((H + 1, W), np.int16))[0] == ESIZE
    # the defaults: cv's BORDER_DEFAULT, src's depth
    import inspect

    sig = inspect.signature(adf.jointBilateralFilter).parameters
    assert sig["borderType"].default == adf.BORDER_REFLECT_101 == 4 and sig["dDepth"].default == -1
    assert list(sig)[:6] == ["joint", "src", "d", "sigmaColor", "sigmaSpace", "borderType"]
