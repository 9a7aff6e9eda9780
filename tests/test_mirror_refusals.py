"""What the Python mirror (ximgproc.py) refuses, with which code and which words, and what its host and device twins
must keep agreeing on.  The CPU part creates no handle (every refusal comes before the library is asked for one); the
GPU part uses 16 x 24 maps."""
import numpy as np
import pytest

from addingdisparityfiltering_amd import _lib
from addingdisparityfiltering_amd import ximgproc as xi
from addingdisparityfiltering_amd._lib import ADF_EBADARG, ADF_ESIZE, AdfError

H, W = 8, 12
SAME_SIZE = "All the images must have the same size"
NO_SPECKLES = "speckle filtering is not implemented inside compute(); use filterSpeckles on the result"


def _refused(code, msg, fn, *args, **kw):
    with pytest.raises(AdfError) as e:
        fn(*args, **kw)
    assert e.value.code == code and str(e.value) == "adf error %d: %s" % (code, msg)


def _views(h=H, w=W):
    return np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)


@pytest.fixture
def no_library(monkeypatch):
    """Asking for the library fails the test: the refusal under test has to come first."""
    def lib():
        raise AssertionError("the library was asked for before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", lib)


# ---- StereoBM.compute / StereoSGBM.compute / computeBoth ----
@pytest.mark.parametrize("make,name", [(lambda: xi.StereoBM.create(16, 5), "BM"), (lambda: xi.StereoSGBM.create(0, 16, 3), "SGBM")])
def test_matcher_compute_refusals(no_library, make, name):
    left, right = _views()
    m = make()
    _refused(ADF_ESIZE, SAME_SIZE, m.compute, left, right[:, :10])
    _refused(ADF_ESIZE, SAME_SIZE, m.compute, left, right[:6])
    _refused(ADF_EBADARG, "left must have dtype uint8 (got float32)", m.compute, left.astype(np.float32), right)
    _refused(ADF_EBADARG, "right must have dtype uint8 (got int16)", m.compute, left, right.astype(np.int16))
    _refused(ADF_ESIZE, "disparity must match the views", m.compute, left, right, np.zeros((H, W - 2), np.int16))
    _refused(ADF_EBADARG, "disparity must have dtype int16 (got float32)", m.compute, left, right, np.zeros((H, W), np.float32))
    m.setSpeckleWindowSize(50)
    _refused(ADF_EBADARG, NO_SPECKLES, m.compute, left, right)
    _refused(ADF_EBADARG, NO_SPECKLES, m.compute, left, right[:, :10])        # the matcher's own state is looked at first
    assert m._h is None


def test_bm_refuses_its_own_left_right_check(no_library):
    left, right = _views()
    m = xi.StereoBM.create(16, 5)
    for v in (0, 1, 999999):
        m.setDisp12MaxDiff(v)
        _refused(ADF_EBADARG, "disp12MaxDiff (left-right check inside the matcher) is not implemented", m.compute, left, right)
    m.setSpeckleWindowSize(50)                                                # both apply: the left-right check wins
    _refused(ADF_EBADARG, "disp12MaxDiff (left-right check inside the matcher) is not implemented", m.compute, left, right)
    m.setSpeckleWindowSize(0)
    for v in (-1, 1000000):                                                   # off: the next refusal is the size's
        m.setDisp12MaxDiff(v)
        _refused(ADF_ESIZE, SAME_SIZE, m.compute, left, right[:, :10])
    assert m._h is None


def test_sgbm_refuses_a_bad_mode_and_mismatched_channels(no_library):
    left, right = _views()
    m = xi.StereoSGBM.create(0, 16, 3)
    for v in (3, -1):
        m.setMode(v)
        _refused(ADF_EBADARG, "mode must be StereoSGBM.MODE_SGBM, MODE_HH or MODE_SGBM_3WAY", m.compute, left, right)
    m.setSpeckleWindowSize(50)                                                # both apply: the mode wins
    _refused(ADF_EBADARG, "mode must be StereoSGBM.MODE_SGBM, MODE_HH or MODE_SGBM_3WAY", m.compute, left, right)
    m.setSpeckleWindowSize(0)
    m.setMode(xi.StereoSGBM.MODE_SGBM_3WAY)
    _refused(ADF_ESIZE, SAME_SIZE, m.compute, np.zeros((H, W, 3), np.uint8), right)      # colour against gray
    assert m._h is None


def test_bm_takes_gray_views_only(no_library):
    batch = np.zeros((2, H, W, 3), np.uint8)
    _refused(ADF_EBADARG, "left has an unsupported shape (2, 8, 12, 3)", xi.StereoBM.create(16, 5).compute, batch, batch)


def test_compute_both_refuses_host_arrays(no_library):
    left, right = _views()
    m = xi.StereoBM.create(16, 5)
    msg = "computeBoth takes device tensors; use two compute() calls on the host"
    _refused(ADF_EBADARG, msg, m.computeBoth, left, right)
    _refused(ADF_EBADARG, msg, m.computeBoth, left, right[:, :10])            # before the sizes are compared
    m.setPreFilterCap(63)                                                     # ... and before the two-compute fallback
    _refused(ADF_EBADARG, msg, m.computeBoth, left, right)
    _refused(ADF_EBADARG, "left must have dtype uint8 (got int16)", m.computeBoth, left.astype(np.int16), right)
    assert m._h is None


# ---- FastGlobalSmootherFilter(...) ----
@pytest.mark.parametrize("guide,msg", [
    (None, "guide is empty"),
    (np.zeros((0, 0), np.uint8), "guide is empty"),
    (np.zeros((H, 0, 3), np.uint8), "guide is empty"),
    (np.zeros((H, W), np.uint16), "guide must be CV_8UC1 or CV_8UC3"),
    (np.zeros((H, W, 2), np.uint8), "guide must be CV_8UC1 or CV_8UC3"),
    (np.zeros((H, W, 4), np.uint8), "guide must be CV_8UC1 or CV_8UC3"),
    (np.zeros((2, H, W, 3), np.uint8), "guide must be CV_8UC1 or CV_8UC3"),
    (np.zeros((W,), np.uint8), "guide must be CV_8UC1 or CV_8UC3"),
])
def test_fgs_guide_refusals(no_library, guide, msg):
    _refused(ADF_EBADARG, msg, xi.FastGlobalSmootherFilter, guide, 8000.0, 1.5)
    _refused(ADF_EBADARG, msg, xi.createFastGlobalSmootherFilter, guide, 8000.0, 1.5)
    _refused(ADF_EBADARG, msg, xi.fastGlobalSmootherFilter, guide, np.zeros((H, W), np.uint8), 8000.0, 1.5)


# ---- filterSpeckles ----
def test_filter_speckles_refusals(no_library):
    img = np.zeros((H, W), np.int16)
    _refused(ADF_EBADARG, "img is empty", xi.filterSpeckles, None, 0, 10, 16)
    _refused(ADF_EBADARG, "filterSpeckles supports CV_16SC1 only (CV_8UC1 is not supported)",
             xi.filterSpeckles, np.zeros((H, W), np.uint8), 0, 10, 16)
    _refused(ADF_EBADARG, "img must be (H,W) or a batch (N,H,W)", xi.filterSpeckles, np.zeros((2, 2, H, W), np.int16), 0, 10, 16)
    _refused(ADF_EBADARG, "img must have dtype int16 (got float32)", xi.filterSpeckles, np.zeros((H, W), np.float32), 0, 10, 16)
    for v in (float("nan"), float("inf"), -float("inf")):
        _refused(ADF_EBADARG, "newVal must be finite", xi.filterSpeckles, img, v, 10, 16)
    _refused(ADF_EBADARG, "maxDiff must be finite", xi.filterSpeckles, img, 0, 10, float("nan"))
    _refused(ADF_EBADARG, "newVal 40000 is outside the CV_16S range", xi.filterSpeckles, img, 40000, 10, 16)
    _refused(ADF_EBADARG, "newVal -32768.6 is outside the CV_16S range", xi.filterSpeckles, img, -32768.6, 10, 16)


# ---- resize / cvtColor / matcherViews ----
def test_view_preparation_refusals(no_library):
    gray, bgr = np.zeros((H, W), np.uint8), np.zeros((H, W, 3), np.uint8)
    _refused(ADF_EBADARG, "resize supports fx == fy == 0.5 only (got fx=0.25, fy=0.25)", xi.resize, bgr, None, 0.25, 0.25)
    _refused(ADF_EBADARG, "resize supports fx == fy == 0.5 only (got fx=0.5, fy=1.0)", xi.resize, bgr, (0, 0), 0.5, 1.0)
    _refused(ADF_EBADARG, "resize supports fx == fy == 0.5 only (got fx=0, fy=0)", xi.resize, gray)
    _refused(ADF_EBADARG, "resize supports INTER_LINEAR at a scale of exactly 0.5 only", xi.resize, bgr, None, 0.5, 0.5, 0)
    _refused(ADF_EBADARG, "src is empty", xi.resize, None, None, 0.5, 0.5)
    _refused(ADF_EBADARG, "src must be (H,W[,3]) or a batch (N,H,W[,3])", xi.resize, np.zeros((W,), np.uint8), None, 0.5, 0.5)
    _refused(ADF_EBADARG, "src has 2 channels; CV_8UC1 and CV_8UC3 are supported", xi.resize, np.zeros((2, H, W, 2), np.uint8), None, 0.5, 0.5)
    _refused(ADF_EBADARG, "cvtColor supports COLOR_BGR2GRAY only (got code 7)", xi.cvtColor, bgr, 7)
    _refused(ADF_EBADARG, "cvtColor(COLOR_BGR2GRAY) needs a 3-channel image", xi.cvtColor, gray, xi.COLOR_BGR2GRAY)
    _refused(ADF_EBADARG, "matcherViews supports scale 0.5 and 1.0 only (got 0.25)", xi.matcherViews, bgr, 0.25)
    _refused(ADF_EBADARG, "matcherViews: scale 1.0 without a colour conversion leaves nothing to do", xi.matcherViews, gray, 1.0)
    _refused(ADF_EBADARG, "matcherViews: scale 1.0 without a colour conversion leaves nothing to do", xi.matcherViews, bgr, 1.0, False)


def test_resize_refuses_another_dsize():
    """(the half size comes from the library: adf_half_size, host arithmetic)"""
    bgr = np.zeros((H, W + 1, 3), np.uint8)
    assert (xi.halfSize(W + 1), xi.halfSize(H)) == (6, 4)
    _refused(ADF_EBADARG, "resize supports half size only: dsize must be (6, 4) for a 13 x 8 image", xi.resize, bgr, (7, 4))
    _refused(ADF_ESIZE, "resize: dst must have shape (4, 6, 3)", xi.resize, bgr, (6, 4), 0, 0, xi.INTER_LINEAR, np.zeros((4, 7, 3), np.uint8))


# ---- evaluation utilities ----
def test_evaluation_refusals(no_library):
    a = np.zeros((H, W), np.int16)
    for fn in (xi.computeMSE, xi.computeBadPixelPercent):
        _refused(ADF_ESIZE, "GT and src differ in size", fn, a, a[:, :10])
        _refused(ADF_EBADARG, "src must have dtype int16 (got uint8)", fn, a, a.astype(np.uint8))
    _refused(ADF_ESIZE, "dst has the wrong size or placement", xi.getDisparityVis, a, np.zeros((H, W - 1), np.uint8))
    _refused(ADF_EBADARG, "dst must have dtype uint8 (got int16)", xi.getDisparityVis, a, a.copy())


# ---- accessors and the two factories that go through them ----
_COMMON = ["MinDisparity", "NumDisparities", "BlockSize", "Disp12MaxDiff", "SpeckleWindowSize", "UniquenessRatio"]
_ACCESSORS = [(xi.StereoBM, _COMMON + ["TextureThreshold", "PreFilterCap"]),
              (xi.StereoSGBM, _COMMON + ["P1", "P2", "Mode", "PreFilterCap"])]
_ATTR = {"P1": "P1", "P2": "P2"}                             # every other parameter's attribute starts in lower case


@pytest.mark.parametrize("cls,names", _ACCESSORS)
def test_every_accessor_pair_round_trips(cls, names):
    m = cls.create()
    for k, name in enumerate(names):
        getter, setter = getattr(cls, "get" + name), getattr(cls, "set" + name)      # real attributes of the class
        assert callable(getter) and callable(setter)
        assert setter(m, 100 + k) is None
        assert getter(m) == 100 + k
        assert getattr(m, _ATTR.get(name, name[0].lower() + name[1:])) == 100 + k   # computeBoth copies these by name
    for k, name in enumerate(names):                         # no pair writes another pair's value
        assert getattr(m, "get" + name)() == 100 + k


def test_matcher_defaults():
    bm = xi.StereoBM.create()
    assert [bm.getMinDisparity(), bm.getNumDisparities(), bm.getBlockSize(), bm.getDisp12MaxDiff(), bm.getSpeckleWindowSize(),
            bm.getUniquenessRatio(), bm.getTextureThreshold(), bm.getPreFilterCap()] == [0, 64, 21, -1, 0, 15, 10, 31]
    assert xi.StereoBM(48, 9).getNumDisparities() == 48 and bm._h is None
    sg = xi.StereoSGBM.create()
    assert [sg.getMinDisparity(), sg.getNumDisparities(), sg.getBlockSize(), sg.getDisp12MaxDiff(), sg.getSpeckleWindowSize(),
            sg.getUniquenessRatio(), sg.getP1(), sg.getP2(), sg.getMode(), sg.getPreFilterCap()] == [0, 16, 3, 0, 0, 0, 0, 0, 0, 0]
    sg = xi.StereoSGBM.create(1, 32, 5, 8, 32, 2, 63, 7, 9, 0, xi.StereoSGBM.MODE_HH)
    assert [sg.getMinDisparity(), sg.getNumDisparities(), sg.getBlockSize(), sg.getDisp12MaxDiff(), sg.getSpeckleWindowSize(),
            sg.getUniquenessRatio(), sg.getP1(), sg.getP2(), sg.getMode(), sg.getPreFilterCap()] == [1, 32, 5, 2, 9, 7, 8, 32, 1, 63]
    assert sg._h is None


def _bm_state(m):
    return [m.getMinDisparity(), m.getNumDisparities(), m.getBlockSize(), m.getTextureThreshold(), m.getUniquenessRatio(),
            m.getPreFilterCap(), m.getDisp12MaxDiff(), m.getSpeckleWindowSize()]


def _sgbm_state(m):
    return [m.getMinDisparity(), m.getNumDisparities(), m.getBlockSize(), m.getP1(), m.getP2(), m.getMode(),
            m.getPreFilterCap(), m.getUniquenessRatio(), m.getDisp12MaxDiff(), m.getSpeckleWindowSize()]


def test_create_right_matcher(no_library):
    bm = xi.StereoBM.create(32, 9)
    bm.setMinDisparity(4); bm.setTextureThreshold(7); bm.setUniquenessRatio(5); bm.setPreFilterCap(63); bm.setSpeckleWindowSize(20)
    before = _bm_state(bm)
    r = xi.createRightMatcher(bm)
    assert isinstance(r, xi.StereoBM) and r._h is None
    assert _bm_state(r) == [-(4 + 32) + 1, 32, 9, 0, 0, 31, 1000000, 0]      # the cap stays cv::StereoBM's default (DF.cpp:421-431)
    assert _bm_state(bm) == before                                            # the left matcher is only read
    sg = xi.StereoSGBM.create(2, 48, 5, 200, 800, 1, 63, 10, 100, 2, xi.StereoSGBM.MODE_SGBM_3WAY)
    before = _sgbm_state(sg)
    r = xi.createRightMatcher(sg)
    assert isinstance(r, xi.StereoSGBM) and r._h is None
    assert _sgbm_state(r) == [-(2 + 48) + 1, 48, 5, 200, 800, xi.StereoSGBM.MODE_SGBM_3WAY, 63, 0, 1000000, 0]
    assert _sgbm_state(sg) == before
    _refused(ADF_EBADARG, "createRightMatcher supports only StereoBM and StereoSGBM", xi.createRightMatcher, xi.StereoMatcher())


def test_create_filter_refuses_another_matcher(no_library):
    m = xi.StereoMatcher(0, 16, 3)
    m.setSpeckleWindowSize(9)
    _refused(ADF_EBADARG, "DisparityWLSFilter natively supports only StereoBM and StereoSGBM", xi.createDisparityWLSFilter, m)
    assert (m.getDisp12MaxDiff(), m.getSpeckleWindowSize()) == (1000000, 0)  # (mutated first, like DF.cpp:389-390)


# =============================================================================================
# GPU part: 16 x 24 maps
# =============================================================================================
GH, GW = 16, 24


def _pair(seed=3, color=True):
    rng = np.random.default_rng(seed)
    view = rng.integers(0, 256, (GH, GW, 3) if color else (GH, GW), dtype=np.uint8)
    dl = (rng.integers(0, 6, (GH, GW)) * 16).astype(np.int16)
    dr = (-dl).astype(np.int16)
    return view, dl, dr


@pytest.mark.gpu
def test_create_filter_from_a_matcher(adf):
    bm = xi.StereoBM.create(32, 9)
    bm.setMinDisparity(4); bm.setTextureThreshold(7); bm.setUniquenessRatio(5); bm.setPreFilterCap(63); bm.setSpeckleWindowSize(20)
    f = xi.createDisparityWLSFilter(bm)
    assert _bm_state(bm) == [4, 32, 9, 0, 0, 63, 1000000, 0]
    assert f.getDepthDiscontinuityRadius() == 3 and f._use_confidence      # ceil(0.33 * 9)
    sg = xi.StereoSGBM.create(2, 48, 5, 200, 800, 1, 63, 10, 100, 2, xi.StereoSGBM.MODE_HH)
    f = xi.createDisparityWLSFilter(sg)
    assert _sgbm_state(sg) == [2, 48, 5, 200, 800, xi.StereoSGBM.MODE_HH, 63, 0, 1000000, 0]
    assert f.getDepthDiscontinuityRadius() == 3 and f._use_confidence      # ceil(0.5 * 5)
    assert (f.getLambda(), f.getSigmaColor(), f.getLRCthresh()) == (8000.0, 1.0, 24)


@pytest.mark.gpu
def test_wls_filter_refusals(adf):
    import torch

    dev = torch.device("cuda", 0)
    view, dl, dr = _pair()
    f = xi.createDisparityWLSFilterGeneric(True)
    for to in (lambda a: a, lambda a: torch.from_numpy(a).to(dev)):
        v, l, r = to(view), to(dl), to(dr)
        _refused(ADF_EBADARG, "disparity_map_right is required with use_confidence", f.filter, l, v)
        _refused(ADF_ESIZE, "left and right disparity maps differ in size", f.filter, l, v, None, r[:, :20])
        _refused(ADF_ESIZE, "filtered_disparity_map has the wrong size or placement", f.filter, l, v, to(np.zeros((GH, GW - 1), np.int16)), r)
        _refused(ADF_EBADARG, "disparity_map_left is empty", f.filter, None, v, None, r)
        _refused(ADF_EBADARG, "left_view is empty", f.filter, l, None, None, r)
    tv, tl, tr = (torch.from_numpy(a).to(dev) for a in (view, dl, dr))
    mixed = "inputs must all be numpy arrays or all be CUDA tensors"
    _refused(ADF_EBADARG, mixed, f.filter, dl, tv, None, dr)
    _refused(ADF_EBADARG, mixed, f.filter, tl, view, None, tr)
    _refused(ADF_EBADARG, mixed, f.filter, tl, tv, None, dr)
    _refused(ADF_ESIZE, "filtered_disparity_map has the wrong size or placement", f.filter, tl, tv, np.zeros((GH, GW), np.int16), tr)
    _refused(ADF_ESIZE, "filtered_disparity_map has the wrong size or placement", f.filter, dl, view, torch.zeros((GH, GW), dtype=torch.int16, device=dev), dr)
    _refused(ADF_EBADARG, "disparity_map_left must have dtype torch.int16", f.filter, tl.float(), tv, None, tr)
    assert f.getConfidenceMap().shape == (0, 0)                              # nothing was filtered


@pytest.mark.gpu
def test_fgs_filter_refusals_host_and_device(adf):
    import torch

    dev = torch.device("cuda", 0)
    guide = _pair()[0]
    src = np.zeros((GH, GW, 3), np.float32)
    size = "Size of the filtered image must be equal to the size of the guide image"
    for to, dst_code, dst_msg in ((lambda a: a, ADF_ESIZE, "dst must be a C-contiguous ndarray with src's shape and dtype"),
                                  (lambda a: torch.from_numpy(a).to(dev), ADF_EBADARG, "dst must be a contiguous CUDA tensor shaped like src")):
        f = xi.createFastGlobalSmootherFilter(to(guide), 8000.0, 1.5)
        s = to(src)
        _refused(ADF_ESIZE, size, f.filter, s[:, :20])
        _refused(ADF_ESIZE, size, f.filter, s[:12])
        _refused(ADF_EBADARG, "src must have at most 4 channels", f.filter, to(np.zeros((GH, GW, 5), np.float32)))
        _refused(ADF_EBADARG, "src depth must be CV_8U, CV_16S or CV_32F", f.filter, to(src.astype(np.float64)))
        _refused(ADF_EBADARG, "src depth must be CV_8U, CV_16S or CV_32F", f.filter, to(np.zeros((2, GH, GW, 3), np.float32)))
        _refused(dst_code, dst_msg, f.filter, s, to(np.zeros((GH, 2 * GW, 3), np.float32))[:, ::2])       # not contiguous
        _refused(dst_code, dst_msg, f.filter, s, to(np.zeros((GH, GW, 3), np.int16)))                       # another dtype
        _refused(dst_code, dst_msg, f.filter, s, to(np.zeros((GH, GW), np.float32)))                        # another shape
        out = to(np.zeros((GH, GW, 3), np.float32))
        assert f.filter(s, out) is out
        assert f.filter(to(np.ascontiguousarray(np.zeros((2 * GH, GW, 3), np.float32)))[::2]).shape == s.shape   # strided input: copied, accepted
    # the other side's array as dst
    f = xi.createFastGlobalSmootherFilter(guide, 8000.0, 1.5)
    _refused(ADF_ESIZE, "dst must be a C-contiguous ndarray with src's shape and dtype", f.filter, src, torch.zeros((GH, GW, 3), device=dev))
    f = xi.createFastGlobalSmootherFilter(torch.from_numpy(guide).to(dev), 8000.0, 1.5)
    _refused(ADF_EBADARG, "dst must be a contiguous CUDA tensor shaped like src", f.filter, torch.from_numpy(src).to(dev), np.zeros((GH, GW, 3), np.float32))
    _refused(ADF_EBADARG, "guide is empty", xi.createFastGlobalSmootherFilter, torch.zeros((0, 0), dtype=torch.uint8, device=dev), 8000.0, 1.5)
    _refused(ADF_EBADARG, "guide must be CV_8UC1 or CV_8UC3", xi.createFastGlobalSmootherFilter, torch.zeros((GH, GW, 2), dtype=torch.uint8, device=dev), 8000.0, 1.5)
    _refused(ADF_EBADARG, "guide must be CV_8UC1 or CV_8UC3", xi.createFastGlobalSmootherFilter, torch.zeros((GH, GW), dtype=torch.int16, device=dev), 8000.0, 1.5)


@pytest.mark.gpu
def test_a_side_stream_gives_the_default_streams_bytes(adf):
    """The mirror hands torch's CURRENT stream to the library: the filter, the smoother's creation (its guide upload) and
    its filter call on a side stream give the bytes they give on the default stream.  On the side stream the inputs are
    written behind a few milliseconds of spinning, so work queued on any other stream would read zeros instead."""
    import torch

    dev = torch.device("cuda", 0)
    view, dl, dr = _pair()
    src = (np.random.default_rng(9).random((GH, GW, 3), dtype=np.float32) * 255).astype(np.float32)
    inputs = [torch.from_numpy(a).to(dev) for a in (view, dl, dr, src)]

    def run(tv, tl, tr, ts):
        f = xi.createDisparityWLSFilterGeneric(True)
        f.setSigmaColor(1.5)
        out = f.filter(tl, tv, None, tr)
        conf = f.getConfidenceMap()
        g = xi.createFastGlobalSmootherFilter(tv, 8000.0, 1.5)
        sm = g.filter(ts)
        sm2 = xi.fastGlobalSmootherFilter(tv[:, :, 0], tl, 500.0, 3.0, solver=xi.SOLVER_EXACT)
        return out, conf, sm, sm2

    expect = run(*inputs)
    late = [torch.zeros_like(t) for t in inputs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)                          # (some 10 ms of device time)
        for z, t in zip(late, inputs):
            z.copy_(t)
        got = run(*late)
    side.synchronize()
    torch.cuda.synchronize()
    for e, g in zip(expect, got):
        assert e.dtype == g.dtype and torch.equal(e, g)
    assert float(expect[0].float().abs().sum()) > 0 and float(expect[2].abs().sum()) > 0


@pytest.mark.gpu
def test_fgs_takes_a_one_element_channel_axis_of_any_stride(adf):
    """(H,W,1) made by a new axis or by permuting (1,H,W): dense for numpy and torch alike, whatever stride the
    one-element axis reports; the pitch comes from the shape.  Same bytes as the (H,W) form, host and device."""
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    guide = rng.integers(0, 256, (GH, GW), dtype=np.uint8)
    src = rng.integers(-500, 500, (GH, GW)).astype(np.int16)
    for to, back in ((lambda a: a, lambda a: a), (lambda a: torch.from_numpy(a).to(dev), lambda a: a.cpu().numpy())):
        g, s = to(guide), to(src)
        expect = back(xi.createFastGlobalSmootherFilter(g, 800.0, 4.0).filter(s))
        axis = lambda a: a[:, :, None]
        permuted = lambda a: (a[None].permute(1, 2, 0) if xi._is_torch(a) else a[None].transpose(1, 2, 0))
        for shape_g in (axis, permuted):
            f = xi.createFastGlobalSmootherFilter(shape_g(g), 800.0, 4.0)
            for shape_s in (axis, permuted):
                got = f.filter(shape_s(s))
                assert tuple(got.shape) == (GH, GW, 1) and np.array_equal(back(got)[:, :, 0], expect)
    f = xi.createFastGlobalSmootherFilter(guide, 800.0, 4.0)
    _refused(ADF_EBADARG, "src depth must be CV_8U, CV_16S or CV_32F", f.filter, src.astype(">i2"))
    _refused(ADF_EBADARG, "src depth must be CV_8U, CV_16S or CV_32F", f.filter, src.astype(np.uint16))


@pytest.mark.gpu
def test_confidence_map_host_and_device_agree(adf):
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    views = rng.integers(0, 256, (2, GH, GW, 3), dtype=np.uint8)
    dls = (rng.integers(0, 5, (2, GH, GW)) * 16).astype(np.int16)
    drs = (-dls + (rng.integers(0, 3, (2, GH, GW)) * 16)).astype(np.int16)       # some pixels fail the left-right check
    fh, fd = xi.createDisparityWLSFilterGeneric(True), xi.createDisparityWLSFilterGeneric(True)
    for batched in (False, True):
        sel = (lambda a: a) if batched else (lambda a: a[0])
        oh = fh.filter(sel(dls), sel(views), None, sel(drs))
        od = fd.filter(*(torch.from_numpy(sel(a)).to(dev) for a in (dls, views)), None, torch.from_numpy(sel(drs)).to(dev))
        ch, cd = fh.getConfidenceMap(), fd.getConfidenceMap()
        assert isinstance(ch, np.ndarray) and ch.dtype == np.float32 and cd.dtype == torch.float32 and cd.is_cuda
        assert ch.shape == tuple(cd.shape) == ((2, GH, GW) if batched else (GH, GW))
        assert np.array_equal(ch.view(np.uint32), cd.cpu().numpy().view(np.uint32))
        assert np.array_equal(oh, od.cpu().numpy())
        assert 0.0 <= float(ch.min()) < float(ch.max()) <= 255.0                # (DF.cpp's scale) not one constant
        if batched:
            assert np.array_equal(fh.getConfidenceMap(1), ch[1]) and torch.equal(fd.getConfidenceMap(1), cd[1])
    assert xi.createDisparityWLSFilterGeneric(False).getConfidenceMap().shape == (0, 0)
