"""CPU tests of the refusals of the domain transform filter's normalized-convolution mode (include/adf_wls.h:
adf_dt_window_filter_*): every one returns its status before a device is touched -- this file runs without a GPU, through
both entry kinds -- with the status adf_dt_filter_* gives for the same cause, and the Python wrapper raises the same ones;
the modes, the radius limit, the workspace size formula; the radii entry point; the symbols."""
import numpy as np
import pytest

EBADARG, ESIZE, ENODEV = 1, 2, 5
U8, S16, S32, F32 = 0, 3, 4, 5
NC, IC, RF = 0, 1, 2
H, W = 6, 8


def _good():
    """The arguments of a call that would be accepted, by name."""
    return dict(n=1, guide=np.zeros((H, W), np.uint8), gch=1, src=np.zeros((H, W), np.int16), sdepth=S16,
                dst=np.zeros((H, W), np.int16), ddepth=S16, W=W, H=H, ss=10.0, sr=30.0, mode=NC, iters=3,
                ws=None, ws_bytes=0, strides={}, offsets={})


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

    g, s, d = img("guide"), img("src"), img("dst")
    args = (a["n"], g[0], g[1], g[2], a["gch"], s[0], s[1], s[2], a["sdepth"], d[0], d[1], d[2], a["ddepth"], a["W"], a["H"],
            a["ss"], a["sr"], a["mode"], a["iters"])
    if kind == "device":
        return L.adf_dt_window_filter_device(*args, a["ws"], a["ws_bytes"], None)
    return L.adf_dt_window_filter_host(*args)


def _last_error():
    from addingdisparityfiltering_amd import _lib

    return _lib.lib().adf_last_error()


def _passes_the_checks(adf, kind, **change):
    """The call gets past every check of its arguments.  The device entry is handed a workspace one byte short, which is
    refused last and before anything is launched (its pointers are host memory here); the host entry goes on to run, or
    to fail for want of a device."""
    if kind == "device":
        a = _good()
        a.update(change)
        rc = _status(adf, kind, ws=1 << 20, ws_bytes=2 * 4 * a["W"] * a["H"] * a["n"] - 1, **change)
        return rc == ESIZE and b"adf_dt_window_filter_workspace_bytes" in _last_error()
    return _status(adf, kind, **change) not in (EBADARG, ESIZE)


KINDS = ["host", "device"]


def test_symbols_and_constants(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for name in ("adf_dt_window_filter_workspace_bytes", "adf_dt_window_filter_device", "adf_dt_window_filter_host", "adf_dt_nc_radii_host"):
        assert hasattr(L, name)
    assert adf.DT_NC_MAX_RADIUS == 127 and (adf.DTF_NC, adf.DTF_IC, adf.DTF_RF) == (0, 1, 2)
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "adf_wls.h")).read()
    assert "#define ADF_DT_NC_MAX_RADIUS 127\n" in header


def test_workspace_size(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    assert L.adf_dt_window_filter_workspace_bytes(1, 3840, 2160) == 2 * 4 * 3840 * 2160     # two float planes per map
    assert L.adf_dt_window_filter_workspace_bytes(16, 7, 5) == 16 * 2 * 4 * 35
    assert L.adf_dt_window_filter_workspace_bytes(3, 65536, 32767) == 3 * 2 * 4 * 65536 * 32767   # past 32 bits
    for bad in ((0, 7, 5), (1, 0, 5), (1, 7, 0), (-1, 7, 5), (1, 65536, 32768)):
        assert L.adf_dt_window_filter_workspace_bytes(*bad) == 0
    assert adf.dtWindowFilterWorkspaceBytes(2, 5, 7) == 2 * 2 * 4 * 35                      # (n, H, W)
    assert adf.dtWindowFilterWorkspaceBytes(2, 5, 7) == 2 * adf.dtFilterWorkspaceBytes(2, 5, 7)


@pytest.mark.parametrize("kind", KINDS)
def test_modes(adf, kind):
    assert _passes_the_checks(adf, kind, mode=NC)
    assert _status(adf, kind, mode=IC) == EBADARG
    assert b"not built" in _last_error()
    assert _status(adf, kind, mode=RF) == EBADARG
    assert b"adf_dt_filter_" in _last_error() and b"not built" not in _last_error()
    for mode in (-1, 3, 100):
        assert _status(adf, kind, mode=mode) == EBADARG
        assert b"unknown mode" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_the_radius_limit(adf, kind):
    assert _passes_the_checks(adf, kind, ss=80.0, iters=3)               # r_1 = 120.9: the reference's perf configuration
    assert _passes_the_checks(adf, kind, ss=84.0, iters=3)               # r_1 = 126.996
    for ss, iters in ((80.0, 1), (1000.0, 3), (85.0, 3), (74.0, 1)):     # r_1 = 138.6, 1511.9, 128.5, 128.2
        assert _status(adf, kind, ss=ss, iters=iters) == EBADARG
        assert b"127" in _last_error()
    assert _passes_the_checks(adf, kind, ss=73.0, iters=1)               # r_1 = 126.4


@pytest.mark.parametrize("kind", KINDS)
def test_parameters(adf, kind):
    for bad in (float("nan"), float("inf"), float("-inf"), 1e300):       # (1e300 is not finite as the float32 the filter uses)
        assert _status(adf, kind, ss=bad) == EBADARG
        assert _status(adf, kind, sr=bad) == EBADARG
    for iters in (9, 1 << 20):
        assert _status(adf, kind, iters=iters) == EBADARG
        assert b"numIters" in _last_error()
    for ss, sr, iters in ((0.5, 30.0, 3), (10.0, 0.0, 3), (-3.0, -1.0, 0), (10.0, 30.0, -2), (10.0, 30.0, 8)):   # clamped, not refused
        assert _passes_the_checks(adf, kind, ss=ss, sr=sr, iters=iters)


@pytest.mark.parametrize("kind", KINDS)
def test_depths_and_channels(adf, kind):
    for depth in (S32, 1, 2, 6, -1):
        assert _status(adf, kind, sdepth=depth) == EBADARG
        assert _status(adf, kind, ddepth=depth) == EBADARG
    for gch in (0, 2, 4, -1):
        assert _status(adf, kind, gch=gch) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
def test_null_and_empty(adf, kind):
    for name in ("guide", "src", "dst"):
        assert _status(adf, kind, **{name: None}) == EBADARG
    for k in ("n", "W", "H"):
        assert _status(adf, kind, **{k: 0}) == EBADARG
        assert _status(adf, kind, **{k: -3}) == EBADARG


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
    assert _status(adf, kind, guide=b8[:H], dst=b8[:H].view(np.int16), strides={"guide": 2 * W}) == EBADARG
    assert _status(adf, kind, guide=b8[:H], dst=b8[:H], ddepth=U8, strides={"guide": 2 * W, "dst": 2 * W}) == EBADARG
    # maps of a batch: the destination's must not overlap each other
    two = np.zeros((2, H, W), np.int16)
    assert _status(adf, kind, n=2, src=two, dst=np.zeros((2, H, W), np.int16),
                   strides={"src_map": two.strides[0], "dst_map": two.strides[0] - 2, "guide_map": 0}) == ESIZE


@pytest.mark.parametrize("kind", KINDS)
def test_sizes(adf, kind):
    assert _status(adf, kind, W=65536, H=32768, guide=1 << 20, src=1 << 21, dst=1 << 22,
                   strides={"guide": 65536, "src": 131072, "dst": 131072}) == ESIZE          # W*H = 2^31
    for name, short in (("src", 2 * W - 2), ("dst", 2 * W - 2), ("guide", W - 1)):
        assert _status(adf, kind, strides={name: short}) == ESIZE
    assert _status(adf, kind, gch=3, guide=np.zeros((H, W, 3), np.uint8), strides={"guide": 3 * W - 1}) == ESIZE
    # a destination row is measured in the DESTINATION's depth
    assert _status(adf, kind, ddepth=F32, dst=np.zeros((H, W), np.float32), strides={"dst": 4 * W - 4}) == ESIZE
    assert _status(adf, kind, ddepth=U8, dst=np.zeros((H, W), np.uint8), strides={"dst": W - 1}) == ESIZE


def test_workspace_too_small_or_misaligned(adf):
    need = 2 * 4 * W * H
    assert _status(adf, "device", ws=1 << 20, ws_bytes=need - 1) == ESIZE                   # (never dereferenced)
    assert b"adf_dt_window_filter_workspace_bytes" in _last_error()
    assert _status(adf, "device", ws=(1 << 20) + 2, ws_bytes=need) == EBADARG


@pytest.mark.parametrize("change", [dict(mode=IC), dict(mode=RF), dict(mode=7), dict(ss=80.0, iters=1), dict(ss=float("nan")),
                                    dict(iters=9), dict(sdepth=S32), dict(gch=2), dict(src=None), dict(W=0),
                                    dict(strides={"src": 2 * W - 2})])
def test_host_and_device_entries_answer_alike(adf, change):
    rc_h = _status(adf, "host", **change)
    text_h = _last_error()
    rc_d = _status(adf, "device", **change)
    assert rc_h == rc_d and rc_h in (EBADARG, ESIZE) and text_h == _last_error()


def test_the_old_names_still_refuse_the_mode(adf):
    from addingdisparityfiltering_amd import _lib

    g, s, d = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16), np.zeros((H, W), np.int16)
    rc = _lib.lib().adf_dt_filter_host(1, g.ctypes.data, W, 0, 1, s.ctypes.data, 2 * W, 0, S16, d.ctypes.data, 2 * W, 0, S16, W, H,
                                       10.0, 30.0, NC, 3)
    assert rc == EBADARG and b"not built" in _last_error()
    with pytest.raises(adf.AdfError) as e:
        adf.dtFilter(g, s, 10, 30, adf.DTF_NC)
    assert "not built" in str(e.value)


def test_radii_entry_point(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    r = np.full(4, -7.0, np.float32)
    assert L.adf_dt_nc_radii_host(10.0, 3, r.ctypes.data) == 0
    assert r[3] == -7.0 and r[0] > r[1] > r[2] > 0                                          # N floats, no more
    assert np.array_equal(r[:3], adf.dtNcRadii(10.0, 3))
    assert np.float32(3.0 * 10.0 * 4.0 / np.sqrt(63.0)) == r[0]
    assert L.adf_dt_nc_radii_host(1000.0, 1, r.ctypes.data) == 0                            # it reports; the calls judge
    assert L.adf_dt_nc_radii_host(10.0, 3, None) == EBADARG
    for bad in ((float("nan"), 3), (float("inf"), 3), (1e300, 3), (10.0, 9)):
        assert L.adf_dt_nc_radii_host(*bad, r.ctypes.data) == EBADARG
    with pytest.raises(adf.AdfError):
        adf.dtNcRadii(10.0, 9)
    with pytest.raises(adf.AdfError):
        adf.dtNcRadii(float("nan"), 3)


def test_python_wrapper_refuses(adf):
    guide, src = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16)

    def code(*args, **kw):
        with pytest.raises(adf.AdfError) as e:
            adf.dtWindowFilter(*args, **kw)
        return e.value.code

    for mode in (adf.DTF_RF, adf.DTF_IC, 7, None):
        assert code(guide, src, 10, 30, mode) == EBADARG
        with pytest.raises(adf.AdfError):
            adf.createDTWindowFilter(guide, 10, 30, mode)
    with pytest.raises(adf.AdfError) as e:
        adf.dtWindowFilter(guide, src, 10, 30, adf.DTF_IC)
    assert "not built" in str(e.value)
    with pytest.raises(adf.AdfError) as e:
        adf.dtWindowFilter(guide, src, 10, 30, adf.DTF_RF)
    assert "dtFilter" in str(e.value) and "not built" not in str(e.value)
    for bad in (float("nan"), float("inf")):
        assert code(guide, src, bad, 30) == EBADARG and code(guide, src, 10, bad) == EBADARG
        with pytest.raises(adf.AdfError):
            adf.createDTWindowFilter(guide, bad, 30)
    assert code(guide, src, 10, 30, numIters=9) == EBADARG
    with pytest.raises(adf.AdfError):
        adf.createDTWindowFilter(guide, 10, 30, numIters=9)
    assert code(guide, src, 80, 50, numIters=1) == EBADARG and code(guide, src, 1000, 30) == EBADARG    # the radius limit
    with pytest.raises(adf.AdfError):
        adf.createDTWindowFilter(guide, 80, 50, numIters=1)
    assert isinstance(adf.createDTWindowFilter(guide, 80, 50), adf.DTWindowFilter)          # 3 iterations: r_1 = 120.9
    assert code(guide, src.astype(np.int32), 10, 30) == EBADARG                             # depth
    assert code(guide, src.astype(np.float64), 10, 30) == EBADARG
    assert code(guide, src, 10, 30, dDepth=4) == EBADARG                                    # CV_32S
    assert code(np.zeros((H, W, 2), np.uint8), src, 10, 30) == EBADARG                      # channel count
    assert code(guide.astype(np.int16), src, 10, 30) == EBADARG
    assert code(guide, src, 10, 30, dst=src) == EBADARG                                     # overlap
    assert code(guide, src, 10, 30, dst=np.zeros((H, W), np.float32)) == EBADARG            # dst of another depth than dDepth
    assert code(np.zeros((H, W + 1), np.uint8), src, 10, 30) == ESIZE
    assert code(guide, src, 10, 30, dst=np.zeros((H + 1, W), np.int16)) == ESIZE
    assert code(guide, np.zeros((2, 3, H, W), np.int16), 10, 30) == EBADARG
    assert code(None, src, 10, 30) == EBADARG
    assert code(guide, src, 10, 30, workspace=np.zeros(4096, np.uint8)) == EBADARG          # a workspace goes with tensors
    # the defaults are the reference's: DTF_NC, three iterations, src's depth
    import inspect

    sig = inspect.signature(adf.dtWindowFilter).parameters
    assert sig["mode"].default == adf.DTF_NC and sig["numIters"].default == 3 and sig["dDepth"].default == -1
    assert inspect.signature(adf.createDTWindowFilter).parameters["mode"].default == adf.DTF_NC
