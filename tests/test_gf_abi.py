"""CPU tests of the guided filter's refusals (include/adf_wls.h): every one returns its status before a device is touched
-- this file runs without a GPU, through both entry kinds -- and the Python wrapper raises the same ones; the workspace
size formula; the symbols."""
import numpy as np
import pytest

EBADARG, ESIZE = 1, 2
U8, S16, S32, F32 = 0, 3, 4, 5
H, W = 6, 8


def _good():
    """The arguments of a call that would be accepted, by name."""
    return dict(n=1, guide=np.zeros((H, W), np.uint8), gch=1, src=np.zeros((H, W), np.int16), sdepth=S16,
                dst=np.zeros((H, W), np.int16), ddepth=S16, W=W, H=H, r=2, eps=1.0, strides={}, offsets={})


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
            a["r"], a["eps"])
    if kind == "device":
        return L.adf_guided_filter_device(*args, None, 0, None)
    return L.adf_guided_filter_host(*args)


KINDS = ["host", "device"]


def test_symbols_and_constants(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    for name in ("adf_guided_filter_workspace_bytes", "adf_guided_filter_device", "adf_guided_filter_host"):
        assert hasattr(L, name)
    assert adf.GF_MAX_RADIUS == 31 and (adf.CV_8U, adf.CV_16S, adf.CV_32F) == (0, 3, 5)


def test_workspace_size(adf):
    from addingdisparityfiltering_amd import _lib

    L = _lib.lib()
    assert L.adf_guided_filter_workspace_bytes(1, 3840, 2160, 1) == 2 * 4 * 3840 * 2160     # (channels + 1) float planes
    assert L.adf_guided_filter_workspace_bytes(16, 7, 5, 3) == 16 * 4 * 4 * 35
    assert L.adf_guided_filter_workspace_bytes(3, 65536, 32767, 3) == 3 * 4 * 4 * 65536 * 32767   # past 32 bits
    for bad in ((0, 7, 5, 1), (1, 0, 5, 1), (1, 7, 0, 3), (1, 7, 5, 2), (1, 7, 5, 0), (1, 7, 5, 4)):
        assert L.adf_guided_filter_workspace_bytes(*bad) == 0
    assert adf.guidedFilterWorkspaceBytes(2, 5, 7, 3) == 2 * 4 * 4 * 35                       # (n, H, W, channels)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("eps", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_eps(adf, kind, eps):
    assert _status(adf, kind, eps=eps) == EBADARG


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", [-1, 32, 1 << 20])
def test_radius(adf, kind, r):
    assert _status(adf, kind, r=r) == EBADARG
    from addingdisparityfiltering_amd import _lib
    assert b"r must" in _lib.lib().adf_last_error()


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
    # a float source on a 2-byte boundary is refused although the int16 destination would be fine there
    assert _status(adf, kind, src=big32, sdepth=F32, offsets={"src": 2}) == EBADARG
    # 8-bit maps need no alignment: the call goes on to the next refusal
    b8 = np.zeros((H + 1, W + 4), np.uint8)
    assert _status(adf, kind, src=b8, sdepth=U8, offsets={"src": 1}, r=40) == EBADARG
    from addingdisparityfiltering_amd import _lib
    assert b"r must" in _lib.lib().adf_last_error()


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


def test_python_wrapper_refuses(adf):
    guide, src = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16)

    def code(*args, **kw):
        with pytest.raises(adf.AdfError) as e:
            adf.guidedFilter(*args, **kw)
        return e.value.code

    assert code(guide, src, -1, 1.0) == EBADARG and code(guide, src, 32, 1.0) == EBADARG
    for eps in (0.0, -2.0, float("nan"), float("inf")):
        assert code(guide, src, 2, eps) == EBADARG
        with pytest.raises(adf.AdfError):
            adf.createGuidedFilter(guide, 2, eps)
    with pytest.raises(adf.AdfError):
        adf.createGuidedFilter(guide, 32, 1.0)
    assert code(guide, src.astype(np.int32), 2, 1.0) == EBADARG                             # depth
    assert code(guide, src.astype(np.float64), 2, 1.0) == EBADARG
    assert code(guide, src, 2, 1.0, dDepth=4) == EBADARG                                    # CV_32S
    assert code(guide, src, 2, 1.0, dDepth=6) == EBADARG
    assert code(np.zeros((H, W, 2), np.uint8), src, 2, 1.0) == EBADARG                      # channel count
    assert code(guide.astype(np.int16), src, 2, 1.0) == EBADARG
    assert code(guide, src, 2, 1.0, dst=src) == EBADARG                                     # overlap
    assert code(guide, src, 2, 1.0, dst=np.zeros((H, W), np.float32)) == EBADARG            # dst of another depth than dDepth
    assert code(guide, src, 2, 1.0, dDepth=adf.CV_32F, dst=np.zeros((H, W), np.int16)) == EBADARG
    assert code(np.zeros((H, W + 1), np.uint8), src, 2, 1.0) == ESIZE
    assert code(guide, src, 2, 1.0, dst=np.zeros((H + 1, W), np.int16)) == ESIZE
    assert code(guide, np.zeros((2, 3, H, W), np.int16), 2, 1.0) == EBADARG
    assert code(None, src, 2, 1.0) == EBADARG
    assert code(guide, src, 2, 1.0, workspace=np.zeros(4096, np.uint8)) == EBADARG          # a workspace goes with tensors
    odd = np.zeros((H, 2 * W + 1), np.uint8)[:, 1:].view(np.int16)                          # an int16 map on an odd address
    assert code(guide, odd, 2, 1.0) == EBADARG
