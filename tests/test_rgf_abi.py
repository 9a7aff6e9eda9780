"""CPU tests of the rolling guidance filter's refusals (include/adf_wls.h: "rolling guidance filter"): every one returns
its status before a device is touched -- this file runs without a GPU, through both entry kinds -- with a non-empty last
error; the workspace size; the table entry point's sizes; the Python wrapper's refusals and its defaults."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

EBADARG, ESIZE = 1, 2
U8, S16, S32, F32 = 0, 3, 4, 5
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
H, W = 6, 8
KINDS = ["host", "device"]


def _good():
    """The arguments of a call that would be accepted, by name."""
    return dict(n=1, src=np.zeros((H, W), np.int16), dst=np.zeros((H, W), np.int16), depth=S16, W=W, H=H, d=5, sc=25.0, ss=3.0,
                iters=4, border=REFLECT_101, strides={}, offsets={}, ws=None, ws_bytes=0)


def _status(kind, **change):
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

    s, d = img("src"), img("dst")
    args = (a["n"], s[0], s[1], s[2], d[0], d[1], d[2], a["depth"], a["W"], a["H"], a["d"], a["sc"], a["ss"], a["iters"], a["border"])
    if kind == "device":
        ws = a["ws"]
        rc = L.adf_rolling_guidance_filter_device(*args, ws if ws is None or isinstance(ws, int) else ws.ctypes.data, a["ws_bytes"], None)
    else:
        rc = L.adf_rolling_guidance_filter_host(*args)
    assert rc == 0 or len(L.adf_last_error()) > 0
    return rc


def _last_error():
    from addingdisparityfiltering_amd import _lib

    return _lib.lib().adf_last_error()


def test_symbols_and_constants(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for name in ("adf_rolling_guidance_filter_device", "adf_rolling_guidance_filter_host", "adf_rgf_tables_host",
                 "adf_rolling_guidance_workspace_bytes"):
        assert hasattr(L, name)
    assert adf.RGF_MAX_ITERS == 16
    assert callable(adf.rollingGuidanceFilter) and callable(adf.rgfTables) and callable(adf.rollingGuidanceWorkspaceBytes)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "adf_wls.h")).read()
    assert "#define ADF_RGF_MAX_ITERS 16" in header


@pytest.mark.parametrize("kind", KINDS)
def test_num_iter(adf, kind):
    for n in (-1, 17, -100, 1 << 30):
        assert _status(kind, iters=n) == EBADARG
        assert b"numOfIter" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_scale_not_finite(adf, kind):
    f = np.zeros((H, W), np.float32)
    assert _status(kind, src=f, dst=f.copy(), depth=F32, sc=1e-37) == EBADARG
    assert b"sigmaColor" in _last_error()
    assert _status(kind, sc=1e-37, iters=-1) == EBADARG and b"numOfIter" in _last_error()    # (an integer depth has no scale)


@pytest.mark.parametrize("kind", KINDS)
def test_border_types(adf, kind):
    for border, name in ((CONSTANT, b"BORDER_CONSTANT"), (WRAP, b"BORDER_WRAP")):
        assert _status(kind, border=border) == EBADARG
        assert b"not built" in _last_error() and name in _last_error()
    for border in (-1, 5, 16, 100):
        assert _status(kind, border=border) == EBADARG
        assert b"not built" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_parameters(adf, kind):
    for bad in (float("nan"), float("inf"), float("-inf"), 1e300, -1e300):   # (1e300 is not finite as float32)
        assert _status(kind, sc=bad) == EBADARG
        assert _status(kind, ss=bad) == EBADARG
    for d in (64, 65, 1000, (1 << 31) - 1):                                  # r = d / 2 above 31
        assert _status(kind, d=d) == EBADARG
        assert b"radius" in _last_error()
    for d in (0, -1):                                                        # r = cvRound(1.5 sigmaSpace) above 31: 31.5 -> 32
        assert _status(kind, d=d, ss=21.0) == EBADARG
        assert b"radius" in _last_error()
    for depth in (S32, 1, 2, 6, -1):
        assert _status(kind, depth=depth) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
def test_null_and_empty(adf, kind):
    for name in ("src", "dst"):
        assert _status(kind, **{name: None}) == EBADARG
    for k in ("n", "W", "H"):
        assert _status(kind, **{k: 0}) == EBADARG
        assert _status(kind, **{k: -3}) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
def test_misalignment(adf, kind):
    big16 = np.zeros((H + 1, W + 4), np.int16)
    for name in ("src", "dst"):
        assert _status(kind, **{name: big16}, offsets={name: 1}) == EBADARG                 # base
        assert _status(kind, **{name: big16}, strides={name: 2 * W + 1}) == EBADARG          # row stride
        assert _status(kind, **{name: big16}, strides={name + "_map": 1001}) == EBADARG
    big32 = np.zeros((H + 1, W + 4), np.float32)
    for name in ("src", "dst"):
        other = {"src": "dst", "dst": "src"}[name]
        for off in (1, 2):
            assert _status(kind, **{name: big32, other: np.zeros((H, W), np.float32)}, depth=F32, offsets={name: off}) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
def test_overlap_and_sizes(adf, kind):
    buf = np.zeros((2 * H, W), np.int16)
    assert _status(kind, src=buf[:H], dst=buf[:H]) == EBADARG                               # in place
    assert b"in-place" in _last_error()
    assert _status(kind, src=buf[:H], dst=buf[H - 1:2 * H - 1]) == EBADARG                  # one row shared
    two = np.zeros((2, H, W), np.int16)
    assert _status(kind, n=2, src=two, dst=np.zeros((2, H, W), np.int16),
                   strides={"src_map": two.strides[0], "dst_map": two.strides[0] - 2}) == ESIZE
    assert _status(kind, W=65536, H=32768, src=1 << 21, dst=1 << 33, strides={"src": 131072, "dst": 131072}) == ESIZE   # W*H = 2^31
    for name in ("src", "dst"):
        assert _status(kind, strides={name: 2 * W - 2}) == ESIZE


def test_workspace(adf):
    from addingdisparityfiltering_amd import _lib

    size = _lib.lib().adf_rolling_guidance_workspace_bytes
    for depth, es in ((U8, 1), (S16, 2), (F32, 4)):
        for n in (1, 3):
            assert size(n, W, H, depth, 0) == 0 and size(n, W, H, depth, 1) == 0
            for iters in (2, 3, 16):
                assert size(n, W, H, depth, iters) == n * W * H * es                        # one plane per map
    for bad in ((0, W, H, S16, 4), (1, 0, H, S16, 4), (1, W, -1, S16, 4), (1, W, H, S32, 4), (1, W, H, S16, -1), (1, W, H, S16, 17),
                (1, 65536, 32768, S16, 4)):
        assert size(*bad) == 0                                                               # what the calls refuse
    assert adf.rollingGuidanceWorkspaceBytes(3, H, W, np.int16, 4) == 3 * H * W * 2
    assert adf.rollingGuidanceWorkspaceBytes(3, H, W, adf.CV_32F, 2) == 3 * H * W * 4
    assert adf.rollingGuidanceWorkspaceBytes(3, H, W, np.uint8, 1) == 0
    # a caller's workspace that is too small, misaligned, or on top of an image: refused before a device is touched
    ws = np.zeros(W * H + 2, np.int16)
    assert _status("device", ws=ws, ws_bytes=2 * W * H - 1) == ESIZE
    assert b"workspace" in _last_error()
    assert _status("device", ws=ws.ctypes.data + 2, ws_bytes=2 * W * H) == EBADARG
    src = np.zeros((H, W), np.int16)
    assert _status("device", src=src, ws=src, ws_bytes=2 * W * H) == EBADARG
    assert b"workspace" in _last_error()


def test_tables_entry_point(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    r, n, k = C.c_int(-1), C.c_int(-1), C.c_float(-1)
    assert L.adf_rgf_tables_host(S16, -1, 25.0, 3.0, None, None, C.byref(r), C.byref(n), C.byref(k)) == 0     # the sizes alone
    assert (r.value, n.value, k.value) == (4, 362, 1.0)
    c, s = np.full(362 + 1, -7.0, np.float32), np.full(16 + 1 + 1, -7.0, np.float32)
    assert L.adf_rgf_tables_host(S16, -1, 25.0, 3.0, c.ctypes.data, s.ctypes.data, None, None, None) == 0
    assert c[-1] == -7.0 and s[-1] == -7.0 and c[-2] == 0.0 and (c[:-2] > 0).all() and (s[:-1] > 0).all()     # exactly T and r*r + 1 entries
    colour, space, radius, scale = adf.rgfTables(np.int16, -1, 25.0, 3.0)
    assert np.array_equal(c[:-1], colour) and np.array_equal(s[:-1], space) and radius == 4 and scale == 1.0
    assert np.array_equal(space, adf.jbfTables(-1, 25.0, 3.0, 1)[1])                          # S is the joint bilateral filter's
    assert L.adf_rgf_tables_host(F32, 9, 25.0, 3.0, None, None, C.byref(r), C.byref(n), C.byref(k)) == 0
    assert (r.value, n.value) == (4, 4098) and np.float32(k.value) == np.float32(256.0 / 25.0)
    assert L.adf_rgf_tables_host(S16, 9, 25.0, 3.0, c.ctypes.data, None, None, None, None) == EBADARG
    for depth_or_dtype in (adf.CV_16S, np.int16, np.dtype(np.int16), "int16"):
        assert np.array_equal(adf.rgfTables(depth_or_dtype, -1, 25.0, 3.0)[0], colour)
    for bad in ((S16, 5, float("nan"), 3.0), (S16, 5, 25.0, float("inf")), (S16, 64, 25.0, 3.0), (S32, 5, 25.0, 3.0), (F32, 5, 1e-37, 3.0)):
        assert L.adf_rgf_tables_host(*bad, None, None, C.byref(r), C.byref(n), C.byref(k)) == EBADARG
        assert len(L.adf_last_error()) > 0
    for bad in ((np.int32, 5, 25.0, 3.0), (np.float64, 5, 25.0, 3.0), (4, 5, 25.0, 3.0), (np.float32, 5, 1e-37, 3.0)):
        with pytest.raises(adf.AdfError):
            adf.rgfTables(*bad)


def test_python_wrapper_refuses_and_defaults(adf):
    src = np.zeros((H, W), np.int16)

    def code(*args, **kw):
        with pytest.raises(adf.AdfError) as e:
            adf.rollingGuidanceFilter(*args, **kw)
        return e.value.code, str(e.value)

    for border, name in ((adf.BORDER_CONSTANT, "BORDER_CONSTANT"), (adf.BORDER_WRAP, "BORDER_WRAP")):
        c, msg = code(src, borderType=border)
        assert c == EBADARG and "not built" in msg and name in msg
    assert code(src, borderType=None)[0] == EBADARG
    for n in (-1, 17):
        c, msg = code(src, numOfIter=n)
        assert c == EBADARG and "numOfIter" in msg
    c, msg = code(np.zeros((H, W), np.float32), sigmaColor=1e-37)
    assert c == EBADARG and "sigmaColor" in msg
    assert code(None)[0] == EBADARG
    assert code(src.astype(np.int32))[0] == EBADARG and code(src.astype(np.float64))[0] == EBADARG
    c, msg = code(np.zeros((2, H, W, 3), np.int16))                                          # multi-channel sources
    assert c == EBADARG and "not built" in msg
    assert code(src, dst=src)[0] == EBADARG                                                   # no in-place call
    assert code(src, dst=np.zeros((H, W), np.float32))[0] == EBADARG                          # dst has the source's depth
    assert code(src, dst=np.zeros((H + 1, W), np.int16))[0] == ESIZE
    assert code(src, 64)[0] == EBADARG and code(src, -1, 25, 21.0)[0] == EBADARG
    assert code(src, workspace=np.zeros(4 * H * W, np.uint8))[0] == EBADARG                   # a workspace goes with CUDA tensors
    # the reference's defaults (EF.hpp:350): d = -1, sigmaColor = 25, sigmaSpace = 3, numOfIter = 4, BORDER_DEFAULT
    sig = inspect.signature(adf.rollingGuidanceFilter).parameters
    assert list(sig) == ["src", "d", "sigmaColor", "sigmaSpace", "numOfIter", "borderType", "dst", "workspace"]
    assert [sig[k].default for k in ("d", "sigmaColor", "sigmaSpace", "numOfIter", "borderType", "dst", "workspace")] == \
        [-1, 25, 3, 4, adf.BORDER_REFLECT_101, None, None]
