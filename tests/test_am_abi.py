"""CPU tests of the adaptive manifold filter's host side (include/adf_wls.h: adf_am_filter_*): every refusal returns its
status before a device is touched -- this file runs without a GPU, through both entry kinds and the Python mirror -- and
leaves the outputs alone; the defaults and signatures of the reference's interface; the workspace size."""
import inspect

import numpy as np
import pytest

EBADARG, ESIZE = 1, 2
U8, S16, S32, F32 = 0, 3, 4, 5
H, W = 6, 8
SENTINEL = 12345


def _good():
    """The arguments of a call that would be accepted, by name."""
    return dict(n=1, joint=np.zeros((H, W), np.uint8), jch=1, src=np.zeros((H, W), np.int16), sdepth=S16,
                dst=np.full((H, W), SENTINEL, np.int16), ddepth=S16, W=W, H=H, ss=4.0, sr=0.2, height=-1, adjust=0,
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

    j, s, d = img("joint"), img("src"), img("dst")
    args = (a["n"], j[0], j[1], j[2], a["jch"], s[0], s[1], s[2], a["sdepth"], d[0], d[1], d[2], a["ddepth"], a["W"], a["H"],
            a["ss"], a["sr"], a["height"], a["adjust"])
    rc = L.adf_am_filter_device(*args, a["ws"], a["ws_bytes"], None) if kind == "device" else L.adf_am_filter_host(*args)
    if isinstance(a["dst"], np.ndarray) and rc in (EBADARG, ESIZE):
        assert (a["dst"] == (SENTINEL if a["dst"].dtype != np.uint8 else 0)).all(), "a refused call wrote its output"
    return rc


def _last_error():
    from addingdisparityfiltering_amd import _lib

    return _lib.lib().adf_last_error()


def _passes_the_checks(adf, kind, **change):
    """The call gets past every check of its arguments.  The device entry is handed a workspace one byte short, which is
    refused last and before anything is launched (its pointers are host memory here); the host entry goes on to run, or to
    fail for want of a device."""
    if kind == "device":
        from addingdisparityfiltering_amd import _lib

        a = _good()
        a.update(change)
        need = _lib.lib().adf_am_filter_workspace_bytes(a["n"], a["W"], a["H"], a["jch"], a["ss"], a["sr"], a["height"])
        assert need > 0
        rc = _status(adf, kind, ws=1 << 20, ws_bytes=need - 1, **change)
        return rc == ESIZE and b"adf_am_filter_workspace_bytes" in _last_error()
    return _status(adf, kind, **change) not in (EBADARG, ESIZE)


KINDS = ["host", "device"]


def test_symbols_and_constants(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for name in ("adf_am_filter_workspace_bytes", "adf_am_filter_device", "adf_am_filter_host", "adf_am_plan_host", "adf_am_exp_host"):
        assert hasattr(L, name)
    assert adf.AM_MAX_TREE_HEIGHT == 8
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "adf_wls.h")).read()
    assert "#define ADF_AM_MAX_TREE_HEIGHT 8 " in header


@pytest.mark.parametrize("kind", KINDS)
def test_sigmas(adf, kind):
    for ss in (0.999, 0.0, -4.0, float("nan"), float("inf")):
        assert _status(adf, kind, ss=ss) == EBADARG
        assert b"sigma_s" in _last_error()
    for sr in (0.0, -0.2, 1.0001, 5.0, float("nan"), float("inf")):
        assert _status(adf, kind, sr=sr) == EBADARG
        assert b"sigma_r" in _last_error()
    for ss, sr in ((1.0, 1.0), (4.0, 0.01), (16.0, 0.2), (8.0, 1.0)):
        assert _passes_the_checks(adf, kind, ss=ss, sr=sr)


@pytest.mark.parametrize("kind", KINDS)
def test_tree_height(adf, kind):
    for height in (0, -2, -100, 9, 1 << 20):
        assert _status(adf, kind, height=height) == EBADARG
        assert b"tree_height" in _last_error()
    for height in (-1, 1, 2, 8):
        assert _passes_the_checks(adf, kind, height=height)
    # an automatic height above the limit: floor(log2 2^20) - 1 = 19 levels at sigma_r -> 0
    big = dict(W=1 << 12, H=1 << 12, joint=1 << 20, src=1 << 26, dst=1 << 28, strides={"joint": 1 << 12, "src": 1 << 13, "dst": 1 << 13})
    assert _status(adf, kind, ss=float(1 << 20), sr=0.01, **big) == EBADARG
    assert b"automatic tree height" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_small_plane(adf, kind):
    # df = 4 at (16, 0.2): W = 2 gives cvRound(0.5) = 0 columns, W = 3 gives 1
    for bad in (dict(W=2), dict(H=2), dict(W=1, H=1)):
        assert _status(adf, kind, ss=16.0, **bad) == EBADARG
        assert b"small plane" in _last_error()
    assert _passes_the_checks(adf, kind, ss=16.0, W=3, H=3)


@pytest.mark.parametrize("kind", KINDS)
def test_null_empty_depths_and_channels(adf, kind):
    assert _status(adf, kind, joint=None) == EBADARG
    assert b"not built" in _last_error()
    for name in ("src", "dst"):
        assert _status(adf, kind, **{name: None}) == EBADARG
    for k in ("n", "W", "H"):
        assert _status(adf, kind, **{k: 0}) == EBADARG
        assert _status(adf, kind, **{k: -3}) == EBADARG
    for depth in (S32, 1, 2, 6, -1):
        assert _status(adf, kind, sdepth=depth) == EBADARG
        assert _status(adf, kind, ddepth=depth) == EBADARG
    for jch in (0, 2, 4, -1):
        assert _status(adf, kind, jch=jch) == EBADARG
        assert b"1 or 3 channels" in _last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_geometry(adf, kind):
    big16 = np.full((H + 1, W + 4), SENTINEL, np.int16)
    for name in ("src", "dst"):
        assert _status(adf, kind, **{name: big16}, offsets={name: 1}) == EBADARG            # base
        assert _status(adf, kind, **{name: big16}, strides={name: 2 * W + 1}) == EBADARG     # row stride
    buf = np.full((2 * H, W), SENTINEL, np.int16)
    assert _status(adf, kind, src=buf[:H], dst=buf[:H]) == EBADARG                           # in place
    assert b"src or joint" in _last_error()
    b8 = np.zeros((2 * H, 2 * W), np.uint8)
    assert _status(adf, kind, joint=b8[:H], dst=b8[:H], ddepth=U8, strides={"joint": 2 * W, "dst": 2 * W}) == EBADARG
    assert _status(adf, kind, W=65536, H=32768, joint=1 << 20, src=1 << 21, dst=1 << 22,
                   strides={"joint": 65536, "src": 131072, "dst": 131072}) == ESIZE           # W*H = 2^31
    for name, short in (("src", 2 * W - 2), ("dst", 2 * W - 2), ("joint", W - 1)):
        assert _status(adf, kind, strides={name: short}) == ESIZE
    two = np.zeros((2, H, W), np.int16)
    assert _status(adf, kind, n=2, src=two, dst=np.full((2, H, W), SENTINEL, np.int16),
                   strides={"src_map": two.strides[0], "dst_map": two.strides[0] - 2, "joint_map": 0}) == ESIZE


@pytest.mark.parametrize("change", [dict(ss=0.5), dict(sr=1.5), dict(sr=float("nan")), dict(height=0), dict(height=9), dict(ss=16.0, W=2),
                                    dict(joint=None), dict(jch=2), dict(sdepth=S32), dict(src=None), dict(W=0), dict(strides={"src": 2 * W - 2})])
def test_host_and_device_entries_answer_alike(adf, change):
    rc_h = _status(adf, "host", **change)
    text_h = _last_error()
    rc_d = _status(adf, "device", **change)
    assert rc_h == rc_d and rc_h in (EBADARG, ESIZE) and text_h == _last_error()


def test_workspace(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    need = L.adf_am_filter_workspace_bytes(1, W, H, 1, 4.0, 0.2, -1)
    assert need > 4 * 4 * W * H                                                             # num, den, mind and the root manifold
    assert _status(adf, "device", ws=1 << 20, ws_bytes=need - 1) == ESIZE                    # (never dereferenced)
    assert b"adf_am_filter_workspace_bytes" in _last_error()
    assert _status(adf, "device", ws=(1 << 20) + 2, ws_bytes=need) == EBADARG
    assert L.adf_am_filter_workspace_bytes(2, W, H, 1, 4.0, 0.2, -1) > need
    assert L.adf_am_filter_workspace_bytes(1, W, H, 3, 4.0, 0.2, -1) > need
    assert L.adf_am_filter_workspace_bytes(1, W, H, 1, 4.0, 0.2, 8) > need
    assert L.adf_am_filter_workspace_bytes(4, 65536, 32767, 3, 16.0, 0.2, -1) > 1 << 35      # past 32 bits
    for bad in ((0, W, H, 1, 4.0, 0.2, -1), (1, 0, H, 1, 4.0, 0.2, -1), (1, W, 0, 1, 4.0, 0.2, -1), (1, 65536, 32768, 1, 4.0, 0.2, -1),
                (1, W, H, 2, 4.0, 0.2, -1), (1, W, H, 1, 0.5, 0.2, -1), (1, W, H, 1, 4.0, 0.0, -1), (1, W, H, 1, 4.0, 1.5, -1),
                (1, W, H, 1, 4.0, 0.2, 0), (1, W, H, 1, 4.0, 0.2, 9), (1, 2, H, 1, 16.0, 0.2, -1), (1, W, H, 1, float("nan"), 0.2, -1)):
        assert L.adf_am_filter_workspace_bytes(*bad) == 0
    assert adf.amFilterWorkspaceBytes(2, H, W, 3, 4.0, 0.2) == L.adf_am_filter_workspace_bytes(2, W, H, 3, 4.0, 0.2, -1)   # (n, H, W)
    assert adf.amFilterWorkspaceBytes(1, H, W, 1, 4.0, 1.5) == 0
    assert adf.amFilterWorkspaceBytes(1, H, W, 1, 4.0, 0.2, 0) == 0


def test_plan_entry_point(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    p = _lib.AmPlan()
    p.df = -7
    jtab = np.full(257, -7.0, np.float32)
    assert L.adf_am_plan_host(16.0, 0.2, -1, 130, 200, p, jtab.ctypes.data) == 0
    assert (p.df, p.height, p.sh, p.sw, p.manifolds) == (4, 3, 50, 32, 7)
    assert jtab[256] == -7.0 and jtab[0] == 0.0 and jtab[255] == 1.0                        # 256 floats, no more
    assert L.adf_am_plan_host(16.0, 0.2, -1, 130, 200, p, None) == 0                        # the table is optional
    assert L.adf_am_plan_host(16.0, 0.2, -1, 130, 200, None, None) == EBADARG
    p.df = -7
    for bad in ((0.5, 0.2, -1, 8, 8), (16.0, 0.0, -1, 8, 8), (16.0, 0.2, 0, 8, 8), (16.0, 0.2, 9, 8, 8), (16.0, 0.2, -1, 2, 8), (16.0, 0.2, -1, 0, 8)):
        assert L.adf_am_plan_host(*bad, p, None) == EBADARG
        assert p.df == -7                                                                   # a refused call leaves the plan alone
    with pytest.raises(adf.AdfError):
        adf.amPlan(16.0, 1.5, -1, 8, 8)


def test_python_mirror_refuses_and_leaves_dst_alone(adf):
    joint, src = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16)

    def code(*args, **kw):
        dst = kw.get("dst")
        before = None if dst is None else dst.copy()
        with pytest.raises(adf.AdfError) as e:
            adf.amFilter(*args, **kw)
        assert dst is None or np.array_equal(dst, before)
        return e.value.code

    out = np.full((H, W), SENTINEL, np.int16)
    for ss, sr in ((0.5, 0.2), (float("nan"), 0.2), (4.0, 0.0), (4.0, 1.5), (4.0, float("inf"))):
        assert code(joint, src, ss, sr, dst=out) == EBADARG
    assert code(None, src, 4.0, 0.2, dst=out) == EBADARG
    assert code(joint, None, 4.0, 0.2) == EBADARG
    assert code(joint, src.astype(np.int32), 4.0, 0.2) == EBADARG                            # depth
    assert code(joint, src, 4.0, 0.2, dDepth=4) == EBADARG                                   # CV_32S
    assert code(np.zeros((H, W, 2), np.uint8), src, 4.0, 0.2) == EBADARG                     # channel count
    assert code(joint.astype(np.int16), src, 4.0, 0.2) == EBADARG
    assert code(joint, src, 4.0, 0.2, dst=src) == EBADARG                                    # overlap
    assert code(joint, np.zeros((2, 3, H, W), np.int16), 4.0, 0.2) == EBADARG
    assert code(np.zeros((H, W + 1), np.uint8), src, 4.0, 0.2) == ESIZE
    assert code(joint, src, 16.0, 0.2, dst=np.full((2, W), SENTINEL, np.int16)) == ESIZE
    assert code(joint[:2], src[:2], 16.0, 0.2) == EBADARG                                    # the small plane would be empty
    assert code(joint, src, 4.0, 0.2, workspace=np.zeros(4096, np.uint8)) == EBADARG         # a workspace goes with tensors
    f = adf.createAMFilter(4.0, 0.2)
    for height in (0, -2, 9):
        f.setTreeHeight(height)
        with pytest.raises(adf.AdfError) as e:
            f.filter(src, out, joint)
        assert e.value.code == EBADARG and (out == SENTINEL).all()
    with pytest.raises(adf.AdfError) as e:
        adf.createAMFilter(4.0, 0.2).filter(src)                                             # no joint
    assert e.value.code == EBADARG and "not built" in str(e.value)


def test_defaults_and_signatures(adf):
    f = adf.AdaptiveManifoldFilter.create()
    assert isinstance(f, adf.AdaptiveManifoldFilter)
    assert (f.getSigmaS(), f.getSigmaR(), f.getTreeHeight(), f.getPCAIterations(), f.getAdjustOutliers(), f.getUseRNG()) == \
        (16.0, 0.2, -1, 1, False, False)
    f.setSigmaS(40)
    f.setSigmaR(0.1)
    f.setTreeHeight(5)
    f.setPCAIterations(4)
    f.setAdjustOutliers(True)
    f.setUseRNG(False)
    assert (f.getSigmaS(), f.getSigmaR(), f.getTreeHeight(), f.getPCAIterations(), f.getAdjustOutliers(), f.getUseRNG()) == \
        (40.0, 0.1, 5, 4, True, False)
    f.setPCAIterations(0)
    assert f.getPCAIterations() == 1                                                         # clamped
    with pytest.raises(adf.AdfError) as e:
        f.setUseRNG(True)
    assert e.value.code == EBADARG and "not built" in str(e.value)
    assert f.collectGarbage() is None
    g = adf.createAMFilter(8.0, 0.3)
    assert (g.getSigmaS(), g.getSigmaR(), g.getAdjustOutliers(), g.getTreeHeight()) == (8.0, 0.3, False, -1)
    assert adf.createAMFilter(8.0, 0.3, True).getAdjustOutliers() is True
    sig = inspect.signature(adf.amFilter).parameters
    assert list(sig)[:5] == ["joint", "src", "sigma_s", "sigma_r", "adjust_outliers"]
    assert sig["adjust_outliers"].default is False and sig["dDepth"].default == -1 and sig["dst"].default is None and sig["workspace"].default is None
    assert inspect.signature(adf.createAMFilter).parameters["adjust_outliers"].default is False
    assert list(inspect.signature(adf.AdaptiveManifoldFilter.filter).parameters)[:4] == ["self", "src", "dst", "joint"]
