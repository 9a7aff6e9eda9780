"""Host-side mirror of the reference's operator interface for the disparity-filter path.

Same names, argument meaning and error behaviour as cv::ximgproc in
modules/ximgproc/include/opencv2/ximgproc/disparity_filter.hpp (DF.hpp) and
edge_filter.hpp (EF.hpp), over the C-ABI in include/adf_wls.h:

    createDisparityWLSFilter(matcher_left)          DF.hpp:131  / DF.cpp:386-414
    createRightMatcher(matcher_left)                DF.hpp:139  / DF.cpp:417-449
    createDisparityWLSFilterGeneric(use_confidence) DF.hpp:149  / DF.cpp:452-455
    DisparityWLSFilter.filter(...)                  DF.hpp:75   / DF.cpp:219-298
    DisparityWLSFilter.get*/set*                    DF.hpp:90-122
    createFastGlobalSmootherFilter(...)             EF.hpp:393
    fastGlobalSmootherFilter(...)                   EF.hpp:413
    filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, buf)   calib3d (outside the reference tree)
    validateDisparity(disparity, cost, minDisparity, numberOfDisparities, disp12MaxDiff)   calib3d (outside the reference tree)
    StereoBM.computeWithCost / computeBothWithCost / computeFull, StereoSGBM.computeFull   what calib3d's compute does with the matcher's own settings (extension names)
    StereoSGBM.computeBoth(left, right, ..., rightSource)   both views' maps from one call (extension; include/adf_wls.h: adf_sgbm_compute_both_*)
    censusTransform(image, kernelSize, type)        modules/stereo descriptor.hpp:428 / descriptor.cpp:77-98
    StereoBM.setCostType(BM_COST_CENSUS_*) / setCensusSize(k)   the cost of modules/stereo stereo_binary_bm.cpp:367-408 (extension)
    resize(src, dsize, fx, fy) at half size, cvtColor(src, COLOR_BGR2GRAY)   imgproc (outside the reference tree)
    reprojectImageTo3D(disparity, Q, handleMissingValues, ddepth), pointCloud(...)   calib3d (outside the reference tree)
    initUndistortRectifyMap(K, dist, R, P, size), remap(src, map1, map2), rectifyViews(...)   calib3d / imgproc (outside the reference tree)
    weightedMedianFilter(joint, src, r, sigma, weightType, mask, ignoreValue)   weighted_median_filter.hpp:64-90 (the library's own integer definition)
    guidedFilter(guide, src, radius, eps, dDepth)   EF.hpp:180  / guided_filter.cpp (the library's own exact definition)
    createGuidedFilter(guide, radius, eps) -> GuidedFilter.filter(src, dst, dDepth)   EF.hpp:158, 143
    dtFilter(guide, src, sigmaSpatial, sigmaColor, mode, numIters)   EF.hpp:120  / dtfilter_cpu.hpp (DTF_RF only; the library's own exact definition)
    createDTFilter(guide, sigmaSpatial, sigmaColor, mode, numIters) -> DTFilter.filter(src, dst, dDepth)   EF.hpp:100, 80
    dtWindowFilter(guide, src, sigmaSpatial, sigmaColor, mode, numIters)   the same call in mode DTF_NC, the reference's default (the library's own exact definition)
    createDTWindowFilter(guide, sigmaSpatial, sigmaColor, mode, numIters) -> DTWindowFilter.filter(src, dst, dDepth)
    jointBilateralFilter(joint, src, d, sigmaColor, sigmaSpace, borderType, dDepth)   EF.hpp:317 / joint_bilateral_filter.cpp (8-bit joints; the library's own exact definition)
    rollingGuidanceFilter(src, d, sigmaColor, sigmaSpace, numOfIter, borderType)   EF.hpp:350 / rolling_guidance_filter.cpp (one channel; the library's own exact definition)

Images are numpy arrays (host path: copied to the GPU and back) or torch CUDA
tensors (device path: zero-copy, asynchronous on torch's current stream).  A
leading batch dimension filters N independent, equally sized pairs in one call.
All compute runs in the HIP library; there is no CPU fallback.
"""
import ctypes as C
import functools
import math

import numpy as np

from . import _lib
from ._lib import SGBM_COST_BT, SGBM_COST_CENSUS_DENSE, SGBM_COST_CENSUS_SPARSE  # noqa: F401  (re-exported)
from ._lib import BM_COST_SAD, BM_COST_CENSUS_DENSE, BM_COST_CENSUS_SPARSE  # noqa: F401  (re-exported)
from ._lib import SGBM_COST_MCT_DENSE, SGBM_COST_MCT_SPARSE, SGBM_COST_CENSUS_CS  # noqa: F401  (re-exported)
from ._lib import BM_COST_MCT_DENSE, BM_COST_MCT_SPARSE, BM_COST_CENSUS_CS  # noqa: F401  (re-exported)
from ._lib import SGBM_RIGHT_MATCHER, SGBM_RIGHT_FROM_VOLUME  # noqa: F401  (re-exported)
from ._lib import WMF_EXP, WMF_IV1, WMF_IV2, WMF_COS, WMF_JAC, WMF_OFF  # noqa: F401  (cv's WMFWeightType; EXP and OFF are built)
from ._lib import GF_MAX_RADIUS  # noqa: F401  (re-exported)
from ._lib import DTF_NC, DTF_IC, DTF_RF, DT_MAX_ITERS, DT_NC_MAX_RADIUS  # noqa: F401  (cv's EdgeAwareFiltersList; DTF_RF and, under dtWindowFilter, DTF_NC are built)
from ._lib import RGF_MAX_ITERS, AM_MAX_TREE_HEIGHT  # noqa: F401  (re-exported)
from ._lib import JBF_MAX_RADIUS, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101  # noqa: F401  (cv's BorderTypes; 1, 2 and 4 are built)
from ._lib import AdfError, HANDOFF_IMAGE, HANDOFF_IMAGE_PAIR_TAIL, HANDOFF_PAIR_PLANE, PATH_CONF_BAND, PATH_FUSED_FIRST_PASS, PATH_MERGED_PREP, PATH_ROW_WEIGHTS_GUIDE, PATH_SCALED_FUSED, PATH_SCALED_HALF, Rect, SOLVER_EXACT, SOLVER_WAVE  # noqa: F401  (re-exported)

try:  # torch is optional plumbing: device memory and streams only
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_torch(a):
    return torch is not None and isinstance(a, torch.Tensor)


def _as_rect(roi):
    if roi is None:
        return None
    if isinstance(roi, Rect):
        return roi
    x, y, w, h = roi
    return Rect(int(x), int(y), int(w), int(h))


_ITEMSIZE = {np.int16: 2, np.uint8: 1, np.float32: 4, np.uint64: 8, np.int32: 4}
# (torch has no unsigned 64-bit type that every build can index: a descriptor plane is an int64 tensor carrying the bit pattern)
_TORCH_DTYPE = {np.int16: torch.int16, np.uint8: torch.uint8, np.float32: torch.float32, np.uint64: torch.int64, np.int32: torch.int32} if torch is not None else {}
_raw_stream = getattr(getattr(torch, "_C", None), "_cuda_getCurrentRawStream", None) if torch is not None else None


class _Image:
    """Pointer + strides of a (N,)H,W(,C) image held by numpy or torch."""

    def __init__(self, arr, dtype_np, what, batched, allow_channels=(1,)):
        self.keep = arr
        if _is_torch(arr):
            if not arr.is_cuda:
                arr = arr.cpu().numpy()
            else:
                if arr.dtype != _TORCH_DTYPE[dtype_np]:
                    raise AdfError(_lib.ADF_EBADARG, "%s must have dtype %s" % (what, _TORCH_DTYPE[dtype_np]))
                self.device = True
                isz = _ITEMSIZE[dtype_np]
                self.ptr = arr.data_ptr()
                self._finish(arr.shape, [q * isz for q in arr.stride()], isz, what, batched, allow_channels)
                return
        a = np.asarray(arr)
        if a.dtype != np.dtype(dtype_np):
            raise AdfError(_lib.ADF_EBADARG, "%s must have dtype %s (got %s)" % (what, np.dtype(dtype_np), a.dtype))
        self.device = False
        self.keep = a
        self.ptr = a.ctypes.data
        self._finish(a.shape, a.strides, a.itemsize, what, batched, allow_channels)

    def _finish(self, shape, strides, itemsize, what, batched, allow_channels):
        # (this runs four times per filter call: no list surgery)
        nd = len(shape)
        k = 1 if batched else 0
        if nd - k == 2:
            self.c, sc, sx = 1, itemsize, strides[k + 1]
        elif nd - k == 3:
            self.c, sc, sx = shape[k + 2], strides[k + 2], strides[k + 1]
        else:
            raise AdfError(_lib.ADF_EBADARG, "%s has an unsupported shape %s" % (what, tuple(shape)))
        self.n, self.pair_stride = (shape[0], strides[0]) if batched else (1, 0)
        self.h, self.w, self.stride = shape[k], shape[k + 1], strides[k]
        if self.n < 1 or self.h < 1 or self.w < 1:
            raise AdfError(_lib.ADF_EBADARG, "%s is empty" % what)
        if self.c not in allow_channels:
            raise AdfError(_lib.ADF_EBADARG, "%s must have %s channel(s)" % (what, " or ".join(map(str, allow_channels))))
        if sc != itemsize or sx != itemsize * self.c:
            raise AdfError(_lib.ADF_ESIZE, "%s rows must be dense (channel-interleaved, unit pixel stride)" % what)


def _empty(img, shape, dtype_np):
    """An uninitialised array where `img` lives: a tensor on its device, or a numpy array."""
    if img.device:
        return torch.empty(shape, dtype=_TORCH_DTYPE[dtype_np], device=img.keep.device)
    return np.empty(shape, dtype_np)


def _out_like(img, batched, dtype_np):
    return _empty(img, (img.n, img.h, img.w) if batched else (img.h, img.w), dtype_np)


def _stream_of(img):
    if img.device:
        dev = img.keep.device
        if _raw_stream is not None and dev.index is not None:      # the raw handle of torch's current stream, without a Stream object
            return _raw_stream(dev.index)
        return torch.cuda.current_stream(dev).cuda_stream
    return None


def _read(fn, ctype, *args):
    """What a C getter writes through its last argument (an int* or a double*)."""
    v = ctype()
    _lib.check(fn(*args, C.byref(v)))
    return v.value


_entries = {}   # base name -> (host function, device function), resolved on first use


def _call(name, img, args):
    """THE host/device fork: `name`_device(*args, stream) for an image held by a CUDA tensor (torch's current stream on
    its device), `name`_host(*args) otherwise.  Pointers go as plain integers (None = null): the prototypes in _lib.py
    say void*, so no ctypes object is built per argument.  A device-only entry has no host function: host arrays are
    refused (its caller words the refusal first)."""
    pair = _entries.get(name)
    if pair is None:
        pair = _entries[name] = (getattr(_lib.lib(), name + "_host", None), getattr(_lib.lib(), name + "_device"))
    if img.device:
        _lib.check(pair[1](*args, _stream_of(img)))
    elif pair[0] is None:
        raise AdfError(_lib.ADF_EBADARG, "%s takes device tensors only" % name)
    else:
        _lib.check(pair[0](*args))


class _Handle:
    """Owns `_h`, the library's handle of a filter or a matcher: a subclass names its destroy function, and the handle
    goes with the object."""
    _h, _destroy = None, None

    def __del__(self):
        h, self._h = self._h, None
        if h:
            try:
                getattr(_lib.lib(), self._destroy)(h)
            except Exception:
                pass


def _check_device(dev, imgs, what):
    """A handle's workspace lives on the device that was current when it was created (include/adf_wls.h), `dev`:
    tensors of another GPU would pair it with foreign pointers and a foreign stream."""
    for im in imgs:
        if im is not None and im.device and im.keep.device.index != dev:
            raise AdfError(_lib.ADF_EBADARG, "%s lives on cuda:%d; tensors on cuda:%s cannot be passed to it "
                                             "(create one handle per GPU)" % (what, dev, im.keep.device.index))


def _map_dtype(m, exactly=None):
    """np.float32 for a float32 disparity map (numpy or torch), np.int16 for everything else -- which _Image then holds
    to int16, so that any other dtype is refused with ADF_EBADARG.  With `exactly`: that dtype if the map has it, else None."""
    dt = getattr(m, "dtype", None)
    want = np.float32 if exactly is None else exactly
    if _is_torch(m):
        has = dt is _TORCH_DTYPE[want]
    else:
        has = dt is not None and np.dtype(dt) == np.dtype(want)
    return want if has else (np.int16 if exactly is None else None)


class DisparityFilter:
    """Main interface for all disparity map filters (DF.hpp:52-76)."""

    def filter(self, disparity_map_left, left_view, filtered_disparity_map=None,
               disparity_map_right=None, ROI=None, right_view=None):
        raise NotImplementedError


class DisparityWLSFilter(_Handle, DisparityFilter):
    """Disparity map filter based on the Weighted Least Squares filter (DF.hpp:82-122)."""
    _destroy = "adf_wls_destroy"

    def __init__(self, use_confidence, left_offset=0, right_offset=0, top_offset=0, bottom_offset=0,
                 min_disp=0):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().adf_wls_create(C.byref(self._h), int(bool(use_confidence)), left_offset,
                                             right_offset, top_offset, bottom_offset, min_disp))
        self._use_confidence = bool(use_confidence)
        self._last = None  # (batched, device, example image) of the last filter call
        self._dev = _read(_lib.lib().adf_wls_get_device, C.c_int, self._h)   # fixed at creation

    # ---- parameters (DF.hpp:90-122) ----
    def getLambda(self):
        return _read(_lib.lib().adf_wls_get_lambda, C.c_double, self._h)

    def setLambda(self, _lambda):
        _lib.check(_lib.lib().adf_wls_set_lambda(self._h, float(_lambda)))

    def getSigmaColor(self):
        return _read(_lib.lib().adf_wls_get_sigma_color, C.c_double, self._h)

    def setSigmaColor(self, _sigma_color):
        _lib.check(_lib.lib().adf_wls_set_sigma_color(self._h, float(_sigma_color)))

    def getLRCthresh(self):
        return _read(_lib.lib().adf_wls_get_lrc_thresh, C.c_int, self._h)

    def setLRCthresh(self, _LRC_thresh):
        _lib.check(_lib.lib().adf_wls_set_lrc_thresh(self._h, int(_LRC_thresh)))

    def getDepthDiscontinuityRadius(self):
        return _read(_lib.lib().adf_wls_get_depth_discontinuity_radius, C.c_int, self._h)

    def setDepthDiscontinuityRadius(self, _disc_radius):
        _lib.check(_lib.lib().adf_wls_set_depth_discontinuity_radius(self._h, int(_disc_radius)))

    # extensions of this implementation (no counterpart in DF.hpp)
    def setFGSParams(self, lambda_attenuation=0.25, num_iter=3):
        _lib.check(_lib.lib().adf_wls_set_fgs_params(self._h, float(lambda_attenuation), int(num_iter)))

    def setSolver(self, solver):
        _lib.check(_lib.lib().adf_wls_set_solver(self._h, int(solver)))

    def getSolver(self):
        return _read(_lib.lib().adf_wls_get_solver, C.c_int, self._h)

    def getLastSolver(self):
        return _read(_lib.lib().adf_wls_get_last_solver, C.c_int, self._h)

    def getLastPath(self):
        """PATH_* bits of the last filter call: which kernels its confidence stage took (introspection only)."""
        return _read(_lib.lib().adf_wls_get_last_path, C.c_int, self._h)

    def getLastSolverPath(self):
        """... and which its solve passes took (PATH_ROW_WEIGHTS_GUIDE): a word of its own."""
        return _read(_lib.lib().adf_wls_get_last_solver_path, C.c_int, self._h)

    def getLastHandoff(self):
        """HANDOFF_IMAGE where the last row pass of the last call stored the last column pass's register image."""
        return _read(_lib.lib().adf_wls_get_last_handoff, C.c_int, self._h)

    def getInnerHandoffs(self):
        """(full, tail): how many hand-offs before the last one took the register image in the last call's full chunks
        and in its shorter last chunk."""
        full, tail = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().adf_wls_get_inner_handoffs(self._h, C.byref(full), C.byref(tail)))
        return full.value, tail.value

    def enableProfiling(self, on=True):
        """Bracket every kernel launch with HIP events on the caller's stream (measurement hook)."""
        _lib.check(_lib.lib().adf_wls_profile_enable(self._h, int(bool(on))))

    def readProfile(self):
        """{kernel class: dict(launches, total_ms, alg_bytes, moved_bytes)} since enableProfiling()."""
        buf = (_lib.KernelTime * 16)()
        n = C.c_int()
        _lib.check(_lib.lib().adf_wls_profile_read(self._h, buf, 16, C.byref(n)))
        return {buf[k].name.decode(): dict(launches=buf[k].launches, total_ms=buf[k].total_ms,
                                           alg_bytes=buf[k].alg_bytes, moved_bytes=buf[k].moved_bytes)
                for k in range(n.value)}

    def workspaceBytes(self):
        return int(_lib.lib().adf_wls_workspace_bytes(self._h))

    # ---- DisparityFilter::filter (DF.hpp:75) ----
    def filter(self, disparity_map_left, left_view, filtered_disparity_map=None,
               disparity_map_right=None, ROI=None, right_view=None):
        """disparity maps: int16 (CV_16SC1) or float32 (CV_32FC1, the same units: disparity * 16 -- include/adf_wls.h,
        adf_wls_filter_typed_*); the left map's dtype selects the depth and the right map must have it too."""
        return self._filter("adf_wls_filter_scaled", np.int16, disparity_map_left, left_view, filtered_disparity_map,
                            disparity_map_right, ROI)

    def filterFloat(self, disparity_map_left, left_view, filtered_disparity_map=None,
                    disparity_map_right=None, ROI=None):
        """Extension (adf_wls_filter*_f32_*, include/adf_wls.h): filter() with a float32 filtered map that keeps what the
        rounding to 1/16 pixel throws away.  Same inputs and rules; the map is in the int16 map's units (disparity * 16),
        -16.0 outside the ROI, never NaN or inf, and rounding it (half to even, saturated to int16) gives filter()'s map
        bit for bit."""
        return self._filter("adf_wls_filter_scaled_f32", np.float32, disparity_map_left, left_view, filtered_disparity_map,
                            disparity_map_right, ROI)

    def _filter(self, entry, out_dtype, disparity_map_left, left_view, filtered_disparity_map, disparity_map_right, ROI):
        if disparity_map_left is None:
            raise AdfError(_lib.ADF_EBADARG, "disparity_map_left is empty")
        if left_view is None:
            raise AdfError(_lib.ADF_EBADARG, "left_view is empty")
        batched = len(disparity_map_left.shape) == 3
        # the left map's dtype selects the maps' depth: int16, or float32 through the typed entry (refused here, before
        # the library is asked: float64, float16, and a right map of another dtype)
        mdt = _map_dtype(disparity_map_left)
        if mdt is np.float32 and disparity_map_right is not None and _map_dtype(disparity_map_right, np.int16) is np.int16:
            mdt = np.int16   # a pair has ONE depth: beside an int16 right map the float32 left map is the one refused
        dl = _Image(disparity_map_left, mdt, "disparity_map_left", batched)
        gv = _Image(left_view, np.uint8, "left_view", batched, allow_channels=(1, 3))
        if gv.n != dl.n:
            raise AdfError(_lib.ADF_ESIZE, "batch sizes of disparity maps and views differ")
        # a disparity map of another resolution is resized to the view (DF.cpp:224-227, 239-247, 268-277)
        dr = None
        if disparity_map_right is not None and getattr(disparity_map_right, "size", 1) != 0:
            dr = _Image(disparity_map_right, mdt, "disparity_map_right", batched)
            if (dr.n, dr.h, dr.w) != (dl.n, dl.h, dl.w):
                raise AdfError(_lib.ADF_ESIZE, "left and right disparity maps differ in size")  # DF.cpp:263-264
        elif self._use_confidence:
            raise AdfError(_lib.ADF_EBADARG, "disparity_map_right is required with use_confidence")  # DF.cpp:262
        if gv.device != dl.device or (dr is not None and dr.device != dl.device):
            raise AdfError(_lib.ADF_EBADARG, "inputs must all be numpy arrays or all be CUDA tensors")
        if filtered_disparity_map is None:
            filtered_disparity_map = _out_like(gv, batched, out_dtype)
        out = _Image(filtered_disparity_map, out_dtype, "filtered_disparity_map", batched)
        if (out.n, out.h, out.w) != (gv.n, gv.h, gv.w) or out.device != dl.device:               # DF.cpp:252,282
            raise AdfError(_lib.ADF_ESIZE, "filtered_disparity_map has the wrong size or placement")
        if dl.device:
            _check_device(self._dev, (dl, gv, dr, out), "this DisparityWLSFilter")
        roi = _as_rect(ROI)
        args = (self._h, dl.n,
                dl.ptr, dl.stride, dl.pair_stride, dl.w, dl.h,
                gv.ptr, gv.stride, gv.pair_stride, gv.c, gv.w, gv.h,
                out.ptr, out.stride, out.pair_stride,
                dr.ptr if dr else None, dr.stride if dr else 0, dr.pair_stride if dr else 0,
                C.byref(roi) if roi is not None else None)
        if mdt is np.float32:   # (int16 maps stay on their entry, argument for argument)
            entry = "adf_wls_filter_typed"
            args = args[:5] + (_lib.DEPTH_32F,) + args[5:16] + (_DEPTH[out_dtype],) + args[16:]
        # (the one fork written out instead of going through _call: this call's host time is counted in microseconds)
        if dl.device:
            _lib.check(getattr(_lib.lib(), entry + "_device")(*args, _stream_of(dl)))
        else:
            _lib.check(getattr(_lib.lib(), entry + "_host")(*args))
        self._last = (batched, dl.device, gv)
        return filtered_disparity_map

    def getConfidenceMap(self, pair=None):
        """CV_32F confidence map(s) of the last filter call (DF.hpp:117, DF.cpp:138)."""
        if self._last is None or not self._use_confidence:
            return np.zeros((0, 0), np.float32)  # the reference returns an empty Mat
        batched, device, ex = self._last
        pairs = range(ex.n) if pair is None else [pair]
        outs = []
        for k in pairs:
            o = _empty(ex, (ex.h, ex.w), np.float32)
            _call("adf_wls_get_confidence", ex, (self._h, k, o.data_ptr() if device else o.ctypes.data, ex.w * 4))
            outs.append(o)
        if pair is not None or not batched:
            return outs[0]
        return torch.stack(outs) if device else np.stack(outs)

    def getROI(self):
        r = Rect()
        _lib.check(_lib.lib().adf_wls_get_roi(self._h, C.byref(r)))
        return (r.x, r.y, r.width, r.height)

    def sync(self, stream=None):
        _lib.check(_lib.lib().adf_wls_sync(self._h, stream))


# ---------------------------------------------------------------------------------------------
# Matchers.  cv::StereoBM / cv::StereoSGBM live in OpenCV's calib3d, which is outside the reference tree;
# the factories below only need the parameter accessors.  StereoBM additionally carries compute(), the
# published block-matching algorithm on the device (csrc/bm_matcher.hip; parity unpinned
# at the calib3d boundary, bit-exact against oracle/adf_oracle_bm.c); StereoSGBM.compute() is the semi-global matcher in
# the sample's mode (csrc/sgbm_matcher.hip, bit-exact against oracle/adf_oracle_sgbm.c).
# ---------------------------------------------------------------------------------------------
def _accessors(*names):
    """Class decorator: cv::StereoMatcher's getX() / setX(v) pair for every attribute x in `names`."""
    def pair(name):
        return (lambda self: getattr(self, name)), (lambda self, v: setattr(self, name, v))

    def add(cls):
        for name in names:
            for prefix, fn in zip(("get", "set"), pair(name)):
                fn.__name__ = prefix + name[0].upper() + name[1:]
                setattr(cls, fn.__name__, fn)
        return cls
    return add


def _triple(X):
    """A plane's three arguments of a C entry: pointer, row stride, pair stride."""
    return X.ptr, X.stride, X.pair_stride


@_accessors("minDisparity", "numDisparities", "blockSize", "disp12MaxDiff", "speckleWindowSize", "speckleRange", "uniquenessRatio")
class StereoMatcher(_Handle):
    """The parameters every matcher has, and the part of compute() both have in common.  A subclass names its C entry
    point (`_entry`) and the channels a view may have (`_channels`), and supplies `_refuse()` (its own settings it cannot
    run), `_prepare(imgs)` (make the handle if absent, check the device, push the parameters) and `_args(L, R, D)`."""
    _channels = (1,)

    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3):
        self.minDisparity, self.numDisparities, self.blockSize = minDisparity, numDisparities, blockSize
        self.disp12MaxDiff, self.speckleWindowSize, self.uniquenessRatio = -1, 0, 10
        self.speckleRange = 0       # read by computeFull only: compute() runs no speckle filter

    def compute(self, left, right, disparity=None):
        """StereoMatcher::compute: 8-bit views (H,W) or a batch (N,H,W) -> CV_16SC1 disparity*16, rejected pixels
        (minDisparity-1)*16.  torch CUDA tensors are matched where they are, asynchronously on torch's current stream;
        numpy arrays take the host entry point.  The speckle filter is not built into either matcher: the filter
        factory switches it off (DF.cpp:390)."""
        self._refuse()
        if self.speckleWindowSize > 0:
            raise AdfError(_lib.ADF_EBADARG, "speckle filtering is not implemented inside compute(); "
                                             "use filterSpeckles on the result")
        return self._match(left, right, disparity)

    def _views(self, left, right, device_only=None):
        """(L, R, batched): both views described, equal in size and on the same side; `device_only`: the refusal of host arrays."""
        nd = len(left.shape)
        color = 3 in self._channels and nd in (3, 4) and left.shape[-1] == 3   # (H,W,3) / (N,H,W,3); a batch of 3-pixel-wide gray images is not a case
        batched = nd == (4 if color else 3)
        L = _Image(left, np.uint8, "left", batched, self._channels)
        R = _Image(right, np.uint8, "right", batched, self._channels)
        if device_only and not (L.device and R.device):
            raise AdfError(_lib.ADF_EBADARG, device_only)
        if (L.n, L.h, L.w, L.c) != (R.n, R.h, R.w, R.c):
            raise AdfError(_lib.ADF_ESIZE, "All the images must have the same size")
        if L.device != R.device:
            raise AdfError(_lib.ADF_EBADARG, "left and right must live on the same side (host or device)")
        return L, R, batched

    def _run(self, entry, views, planes, mismatch, instead=None, tail=()):
        """A compute call past its views (_views): the output planes {name: the caller's or None for a new one} of the
        views' size and on their side, the handle prepared, `entry` through _call -- or, where the matcher cannot use
        `entry`, `instead(*planes)`.  `tail`: the entry's arguments past its planes.  Returns the planes."""
        L, R, batched = views
        maps = [_out_like(L, batched, np.int16) if m is None else m for m in planes.values()]
        descs = [_Image(m, np.int16, what, batched) for m, what in zip(maps, planes)]
        for D in descs:
            if (D.n, D.h, D.w) != (L.n, L.h, L.w) or D.device != L.device:
                raise AdfError(_lib.ADF_ESIZE, mismatch)
        if instead is not None:
            instead(*maps)
            return tuple(maps)
        self._prepare((L, R, *descs))
        args = self._args(L, R, descs[0])
        for D in descs[1:]:
            args += _triple(D)
        _call(entry, L, args + tail)
        return tuple(maps)

    def _match(self, left, right, disparity):
        """compute() past its refusals: the match alone, whatever the speckle settings say (computeFull runs them)."""
        return self._run(self._entry, self._views(left, right), {"disparity": disparity}, "disparity must match the views")[0]


@_accessors("textureThreshold", "preFilterCap", "costType", "censusSize")
class StereoBM(StereoMatcher):
    """cv::StereoBM's accessors plus compute() on the device (csrc/bm_matcher.hip): CV_8UC1 views.  compute() runs neither
    the left-right check nor the speckle filter of cv::StereoBM and refuses settings that ask for them: the filter factory
    switches both off (DF.cpp:389-390).  computeFull() is the whole calib3d chain -- computeWithCost(), validateDisparity(),
    filterSpeckles() -- with the matcher's own disp12MaxDiff, speckleWindowSize and speckleRange.

    Extension: setCostType(BM_COST_CENSUS_DENSE / _SPARSE) + setCensusSize(k) match census descriptors with a Hamming
    distance, the cost of the reference's own cv::stereo::StereoBinaryBM (include/adf_wls.h: adf_bm_set_cost), which
    ignores gain and exposure differences between the cameras.  preFilterCap and textureThreshold are validated as
    with SAD and NOT USED with a census cost: there is no prefiltered image whose texture could be summed.  Bit-exact
    against the direct statement tests/bm_census_ref.py.  The library checks the pair (type, size) when compute()
    pushes it.  Descriptors: BM_COST_CENSUS_DENSE (k 3, 5, 7), BM_COST_CENSUS_SPARSE (5, 7, 9, 11), the modified census
    BM_COST_MCT_DENSE (3, 5, 7) / BM_COST_MCT_SPARSE (5, 7, 9, 11: neighbours against the window mean) and the
    centre-symmetric BM_COST_CENSUS_CS (3, 5, 7, 9: 4 / 12 / 24 / 40 bits, neighbours against their mirror image); see
    censusTransform.  The matcher's time follows the descriptor's byte planes, ceil(bits / 8)."""
    _destroy, _entry = "adf_bm_destroy", "adf_bm_compute"

    def __init__(self, numDisparities=0, blockSize=21):
        super().__init__(0, numDisparities if numDisparities > 0 else 64, blockSize)   # cv::StereoBM: 0 -> 64
        self.textureThreshold, self.uniquenessRatio, self.preFilterCap = 10, 15, 31
        self.costType, self.censusSize = BM_COST_SAD, 7     # a new adf_bm handle's

    @staticmethod
    def create(numDisparities=0, blockSize=21):
        return StereoBM(numDisparities, blockSize)

    def _left_right_check_on(self):
        return 0 <= self.disp12MaxDiff < 1000000

    def _refuse(self):
        if self._left_right_check_on():
            raise AdfError(_lib.ADF_EBADARG, "disp12MaxDiff (left-right check inside the matcher) is not implemented")

    def _prepare(self, imgs):
        lib = _lib.lib()
        if self._h is None:
            h = C.c_void_p()
            _lib.check(lib.adf_bm_create(C.byref(h), int(self.numDisparities), int(self.blockSize)))
            self._h = h
        _check_device(_read(lib.adf_bm_get_device, C.c_int, self._h), imgs, "this StereoBM")
        _lib.check(lib.adf_bm_set_params(self._h, int(self.minDisparity), int(self.numDisparities), int(self.blockSize),
                                         int(self.preFilterCap), int(self.textureThreshold), int(self.uniquenessRatio)))
        _lib.check(lib.adf_bm_set_cost(self._h, int(self.costType), int(self.censusSize)))

    def _args(self, L, R, D):
        return (self._h, L.n, L.ptr, L.stride, L.pair_stride, R.ptr, R.stride, R.pair_stride, L.w, L.h,
                D.ptr, D.stride, D.pair_stride)     # (spelled out: this runs once per call)

    def computeWithCost(self, left, right, disparity=None, cost=None):
        """Extension: compute()'s map AND the CV_16S plane of the winning disparity's aggregated cost, the pair calib3d's
        StereoBM hands to validateDisparity (include/adf_wls.h: adf_bm_compute_cost_*).  The map is compute()'s byte for
        byte; the plane holds (int16)cost where the map holds a disparity and 0 where it holds (minDisparity-1)*16.  The
        match alone: disp12MaxDiff and the speckle settings are not applied here (computeFull does).  Host arrays take the
        host entry; device tensors run on torch's current stream.  Returns (disparity, cost)."""
        return self._run("adf_bm_compute_cost", self._views(left, right), {"disparity": disparity, "cost": cost},
                         "disparity and cost must match the views")

    def computeBothWithCost(self, left, right, disparity_left=None, disparity_right=None, cost_left=None, cost_right=None):
        """Extension: computeBoth's two maps and the cost plane of each search, identical to `self.computeWithCost(left,
        right)` and `createRightMatcher(self).computeWithCost(right, left)`.  Device tensors only; the same fallback to
        two separate computes as computeBoth when a SAD matcher's preFilterCap is not 31.  Returns (disparity_left,
        disparity_right, cost_left, cost_right)."""
        views = self._views(left, right, "computeBothWithCost takes device tensors; use two computeWithCost() calls on the host")
        rm = self._unshared_right_matcher()
        return self._run("adf_bm_compute_both_cost", views,
                         {"disparity_left": disparity_left, "disparity_right": disparity_right, "cost_left": cost_left, "cost_right": cost_right},
                         "disparity maps and cost planes must match the views",
                         rm and (lambda dl, dr, kl, kr: (rm.computeWithCost(right, left, dr, kr), self.computeWithCost(left, right, dl, kl))))

    def computeFull(self, left, right, disparity=None):
        """Extension: what calib3d's StereoBM::compute does with the matcher's own settings, under a new name so that
        compute() stays what the filter factory expects: the match with its cost; validateDisparity when
        0 <= disp12MaxDiff; filterSpeckles((minDisparity-1)*16, speckleWindowSize, speckleRange) when speckleWindowSize > 0
        -- the range unscaled, the call-site convention of modules/stereo/src/stereo_binary_bm.cpp:416-417."""
        disparity, cost = self.computeWithCost(left, right, disparity)
        if self.disp12MaxDiff >= 0:      # (past 2^26 no two CV_16S values differ by more: the clamp changes nothing)
            validateDisparity(disparity, cost, self.minDisparity, self.numDisparities, min(int(self.disp12MaxDiff), 1 << 26))
        if self.speckleWindowSize > 0:
            filterSpeckles(disparity, (int(self.minDisparity) - 1) * 16, self.speckleWindowSize, self.speckleRange)
        return disparity

    def _unshared_right_matcher(self):
        """None where one launch serves both views (computeBoth's docstring); for a SAD matcher whose preFilterCap is not
        31, createRightMatcher(self) on a matcher (and handle) this one keeps for the two-launch fallback."""
        if self.preFilterCap == 31 or self.costType != BM_COST_SAD:
            return None
        if getattr(self, "_right", None) is None:
            self._right = StereoBM(1, 5)
        rm = createRightMatcher(self)
        for k in ("minDisparity", "numDisparities", "blockSize", "textureThreshold", "uniquenessRatio",
                  "preFilterCap", "disp12MaxDiff", "speckleWindowSize", "costType", "censusSize"):
            setattr(self._right, k, getattr(rm, k))
        return self._right

    def computeBoth(self, left, right, disparity_left=None, disparity_right=None):
        """Extension: this matcher's map AND the map of createRightMatcher(self) (DF.cpp:417-431) from one launch --
        identical to `self.compute(left, right)` and `createRightMatcher(self).compute(right, left)`, with the views
        prefiltered once and both searches in one grid (worth it for one pair per call).  Device tensors only.

        The reference's right matcher keeps cv::StereoBM's default preFilterCap of 31 (DF.cpp:421-431 copy every
        parameter BUT the cap), so one shared prefilter is only the same computation when this matcher's cap is 31
        too; with any other cap the two maps are produced by the two separate computes (same results, two launches).
        With a census cost there is no prefilter: the views share their descriptor planes whatever the cap is, and the
        single launch is always taken."""
        views = self._views(left, right, "computeBoth takes device tensors; use two compute() calls on the host")
        if self._left_right_check_on() or self.speckleWindowSize > 0:
            raise AdfError(_lib.ADF_EBADARG, "the matcher's own left-right check and speckle filter are not implemented")
        rm = self._unshared_right_matcher()
        return self._run("adf_bm_compute_both", views, {"disparity_left": disparity_left, "disparity_right": disparity_right},
                         "disparity maps must match the views",
                         rm and (lambda dl, dr: (self.compute(left, right, dl), rm.compute(right, left, dr))))


@_accessors("P1", "P2", "mode", "preFilterCap", "costType", "censusSize")
class StereoSGBM(StereoMatcher):
    """cv::StereoSGBM's accessors plus compute() on the device (csrc/sgbm_matcher.hip): the published semi-global
    algorithm with three paths (MODE_SGBM_3WAY, the mode the reference's sample selects:
    samples/disparity_filtering.cpp:166-176), five (MODE_SGBM) or eight (MODE_HH), bit-exact against
    oracle/adf_oracle_sgbm.c; parity unpinned at calib3d.  compute() takes CV_8UC1 / CV_8UC3 views (H,W[,3]) or a batch
    (N,H,W[,3]) and runs the matcher's own left-right check (disp12MaxDiff; create's default 0 reads as 1, the filter
    factory switches it off with 1000000, DF.cpp:389); compute() runs no speckle filter (DF.cpp:390 sets it to 0) and
    refuses speckleWindowSize > 0; computeFull() is compute() followed by filterSpeckles with the matcher's settings.

    Extension: setCostType(SGBM_COST_CENSUS_DENSE / _SPARSE) + setCensusSize(k) match on census descriptors with a Hamming
    distance, the cost of the reference's own cv::stereo::StereoBinarySGBM (its setBinaryKernelType / kernelSize;
    include/adf_wls.h: adf_sgbm_set_cost).  CV_8UC1 views only; preFilterCap is ignored; bit-exact against the direct
    statement tests/census_ref.py.  The library checks the pair (type, size) when compute() pushes it.  Descriptors:
    SGBM_COST_CENSUS_DENSE (k 3, 5, 7), SGBM_COST_CENSUS_SPARSE (5, 7, 9, 11), the modified census SGBM_COST_MCT_DENSE
    (3, 5, 7) / SGBM_COST_MCT_SPARSE (5, 7, 9, 11: neighbours against the window mean) and the centre-symmetric
    SGBM_COST_CENSUS_CS (3, 5, 7, 9: neighbours against their mirror image); see censusTransform."""
    MODE_SGBM, MODE_HH, MODE_SGBM_3WAY = 0, 1, 2
    _destroy, _entry, _channels = "adf_sgbm_destroy", "adf_sgbm_compute", (1, 3)

    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, mode=0, preFilterCap=0):
        super().__init__(minDisparity, numDisparities, blockSize)
        self.P1, self.P2, self.mode, self.preFilterCap = P1, P2, mode, preFilterCap
        self.disp12MaxDiff, self.uniquenessRatio = 0, 0     # cv::StereoSGBM::create's defaults (the filter factory raises disp12MaxDiff to 1000000)
        self.costType, self.censusSize = SGBM_COST_BT, 7    # a new adf_sgbm handle's

    @staticmethod
    def create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
               uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=0):
        m = StereoSGBM(minDisparity, numDisparities, blockSize, P1, P2, mode, preFilterCap)
        m.disp12MaxDiff, m.uniquenessRatio, m.speckleWindowSize = disp12MaxDiff, uniquenessRatio, speckleWindowSize
        m.speckleRange = speckleRange
        return m

    def computeFull(self, left, right, disparity=None):
        """Extension: what calib3d's StereoSGBM::compute does with the matcher's own settings, under a new name so that
        compute() stays what the filter factory expects: compute(), whose own left-right check already runs, then
        filterSpeckles((minDisparity-1)*16, speckleWindowSize, 16*speckleRange) when speckleWindowSize > 0
        (modules/stereo/src/stereo_binary_sgbm.cpp:716-718)."""
        self._refuse()
        disparity = self._match(left, right, disparity)
        if self.speckleWindowSize > 0:
            filterSpeckles(disparity, (int(self.minDisparity) - 1) * 16, self.speckleWindowSize, 16 * int(self.speckleRange))
        return disparity

    def _refuse(self):
        if self.mode not in (StereoSGBM.MODE_SGBM, StereoSGBM.MODE_HH, StereoSGBM.MODE_SGBM_3WAY):
            raise AdfError(_lib.ADF_EBADARG, "mode must be StereoSGBM.MODE_SGBM, MODE_HH or MODE_SGBM_3WAY")

    def _prepare(self, imgs):
        lib = _lib.lib()
        if self._h is None:
            h = C.c_void_p()
            _lib.check(lib.adf_sgbm_create(C.byref(h), int(self.minDisparity), int(self.numDisparities), int(self.blockSize)))
            self._h = h
        _check_device(_read(lib.adf_sgbm_get_device, C.c_int, self._h), imgs, "this StereoSGBM")
        _lib.check(lib.adf_sgbm_set_params(self._h, int(self.minDisparity), int(self.numDisparities), int(self.blockSize),
                                           int(self.P1), int(self.P2), int(self.preFilterCap), int(self.uniquenessRatio),
                                           int(self.mode)))
        _lib.check(lib.adf_sgbm_set_disp12_max_diff(self._h, int(self.disp12MaxDiff)))
        _lib.check(lib.adf_sgbm_set_cost(self._h, int(self.costType), int(self.censusSize)))

    def _args(self, L, R, D):
        return (self._h, L.n, L.ptr, L.stride, L.pair_stride, R.ptr, R.stride, R.pair_stride, L.c, L.w, L.h,
                D.ptr, D.stride, D.pair_stride)     # (spelled out: this runs once per call)

    def computeBoth(self, left, right, disparity_left=None, disparity_right=None, rightSource=SGBM_RIGHT_MATCHER):
        """Extension: this matcher's map AND a right-view map from one call, the pair DisparityWLSFilter.filter takes
        (include/adf_wls.h: adf_sgbm_compute_both_*).  The left map is compute()'s byte for byte.  Host arrays take the
        host entry; device tensors run on torch's current stream.  compute()'s refusals apply (speckleWindowSize > 0
        included).  Returns (disparity_left, disparity_right).

        rightSource=SGBM_RIGHT_MATCHER (default): the map of createRightMatcher(self).compute(right, left), as a second
        run inside the call -- identical to the two separate computes, and as expensive.
        rightSource=SGBM_RIGHT_FROM_VOLUME: a speed-for-fidelity option.  The right map is read from this view's
        aggregated volume along its diagonals inside the winner pass (no second cost volume, no second set of path
        passes).  It is NOT the right matcher's map -- the paths ran along the left image -- and has its own definition
        in include/adf_wls.h, bit-exact against tests/sgbm_both_ref.py; on the Tsukuba fixture (a CPU measurement) 93-96 %
        of its columns lie within 1 px of the right matcher's, and the filter improves the raw map a little less with it."""
        self._refuse()
        if self.speckleWindowSize > 0:
            raise AdfError(_lib.ADF_EBADARG, "speckle filtering is not implemented inside computeBoth(); "
                                             "use filterSpeckles on the result")
        if rightSource not in (SGBM_RIGHT_MATCHER, SGBM_RIGHT_FROM_VOLUME):
            raise AdfError(_lib.ADF_EBADARG, "rightSource must be SGBM_RIGHT_MATCHER or SGBM_RIGHT_FROM_VOLUME")
        return self._run("adf_sgbm_compute_both", self._views(left, right),
                         {"disparity_left": disparity_left, "disparity_right": disparity_right}, "disparity maps must match the views",
                         tail=(int(rightSource),))


_INT32_MAX = 2 ** 31 - 1


def _round_half_even(v, what):
    """cvRound of a double argument (round half to even), as an int32 for the C-ABI."""
    v = float(v)
    if not math.isfinite(v):
        raise AdfError(_lib.ADF_EBADARG, "%s must be finite" % what)
    return int(round(v))


def filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, buf=None):
    """cv::filterSpeckles (calib3d; in-tree call site modules/stereo/src/stereo_binary_sgbm.cpp:716-718): 4-connected
    components of pixels != newVal whose neighbours differ by at most maxDiff; every component of at most
    maxSpeckleSize pixels is set to newVal.  `img` is a CV_16SC1 map (H,W) or a batch (N,H,W), modified IN PLACE:
    a torch CUDA tensor runs on the device, asynchronously on torch's current stream; a numpy array takes the host
    entry point.  newVal and maxDiff are rounded half-to-even like cv's doubles (cvRound).  `buf` (device path only):
    a CUDA tensor of at least speckleWorkspaceBytes(...) bytes used as the workspace -- the call then allocates
    nothing and may be captured into a CUDA graph; None = the library's cached scratch.  Returns (img, buf) like
    cv2.filterSpeckles.  Parity with calib3d is unpinned (include/adf_wls.h)."""
    if img is None:
        raise AdfError(_lib.ADF_EBADARG, "img is empty")
    dt = img.dtype if _is_torch(img) else np.asarray(img).dtype
    if dt == np.uint8 or (torch is not None and dt == torch.uint8):
        raise AdfError(_lib.ADF_EBADARG, "filterSpeckles supports CV_16SC1 only (CV_8UC1 is not supported)")
    nd = len(img.shape)
    if nd not in (2, 3):
        raise AdfError(_lib.ADF_EBADARG, "img must be (H,W) or a batch (N,H,W)")
    im = _Image(img, np.int16, "img", nd == 3)
    nv = _round_half_even(newVal, "newVal")
    if not -32768 <= nv <= 32767:
        raise AdfError(_lib.ADF_EBADARG, "newVal %r is outside the CV_16S range" % (newVal,))
    md = max(-_INT32_MAX, min(_INT32_MAX, _round_half_even(maxDiff, "maxDiff")))   # (|diff| <= 65535 either way)
    ms = max(-_INT32_MAX, min(_INT32_MAX, int(maxSpeckleSize)))                     # (W*H < 2^31 either way)
    args = (im.n, im.ptr, im.stride, im.pair_stride, im.w, im.h, nv, ms, md)
    if not im.device:
        _call("adf_filter_speckles", im, args)
        return img, buf
    ws, ws_bytes = None, 0
    if buf is not None:
        if not (_is_torch(buf) and buf.is_cuda and buf.is_contiguous()):
            raise AdfError(_lib.ADF_EBADARG, "buf must be a contiguous CUDA tensor (or None)")
        if buf.device != img.device:
            raise AdfError(_lib.ADF_EBADARG, "buf lives on %s, img on %s" % (buf.device, img.device))
        ws, ws_bytes = buf.data_ptr(), buf.numel() * buf.element_size()
        if ws_bytes < speckleWorkspaceBytes(im.n, im.h, im.w):
            raise AdfError(_lib.ADF_ESIZE, "buf holds %d bytes; %d needed" % (ws_bytes, speckleWorkspaceBytes(im.n, im.h, im.w)))
    with torch.cuda.device(img.device):
        _call("adf_filter_speckles", im, args + (ws, ws_bytes))
    return img, buf


def validateDisparity(disparity, cost, minDisparity, numberOfDisparities, disp12MaxDiff=1):
    """calib3d's validateDisparity(disparity, cost, minDisparity, numberOfDisparities, disp12MaxDiff): the block matcher's
    own left-right check on its map and on the aggregated cost of each winning disparity (StereoBM.computeWithCost).  Per
    row every pixel votes, with its cost, for the column it matched in the other view; a pixel is set to
    (minDisparity-1)*16 when both columns it may have matched hold a winner that differs from it by more than
    16*disp12MaxDiff (the full statement, the refusals and the deviation for votes outside the row: include/adf_wls.h).
    `disparity`: CV_16SC1 (H,W) or a batch (N,H,W), modified IN PLACE and returned; `cost`: int16 or int32, same shape and
    side.  A torch CUDA tensor runs on the device, asynchronously on torch's current stream; a numpy array takes the host
    entry point.  Parity with calib3d is unpinned."""
    if disparity is None or cost is None:
        raise AdfError(_lib.ADF_EBADARG, "disparity and cost must not be empty")
    nd = len(disparity.shape)
    if nd not in (2, 3):
        raise AdfError(_lib.ADF_EBADARG, "disparity must be (H,W) or a batch (N,H,W)")
    D = _Image(disparity, np.int16, "disparity", nd == 3)
    cdt = cost.dtype if _is_torch(cost) else np.asarray(cost).dtype
    if cdt == np.int16 or (torch is not None and cdt == torch.int16):
        ctype, code = np.int16, _lib.DEPTH_16S
    elif cdt == np.int32 or (torch is not None and cdt == torch.int32):
        ctype, code = np.int32, _lib.DEPTH_32S
    else:
        raise AdfError(_lib.ADF_EBADARG, "cost must be int16 (CV_16S) or int32 (CV_32S), got %s" % (cdt,))
    if len(cost.shape) != nd:
        raise AdfError(_lib.ADF_ESIZE, "cost must have the disparity map's shape")
    K = _Image(cost, ctype, "cost", nd == 3)
    if (K.n, K.h, K.w) != (D.n, D.h, D.w) or K.device != D.device:
        raise AdfError(_lib.ADF_ESIZE, "cost must have the disparity map's shape on its side (host or device)")
    ints = []
    for v, what in ((minDisparity, "minDisparity"), (numberOfDisparities, "numberOfDisparities"), (disp12MaxDiff, "disp12MaxDiff")):
        v = int(v)
        if not -_INT32_MAX <= v <= _INT32_MAX:
            raise AdfError(_lib.ADF_EBADARG, "%s does not fit an int" % what)
        ints.append(v)
    args = (D.n, D.ptr, D.stride, D.pair_stride, K.ptr, K.stride, K.pair_stride, code, D.w, D.h) + tuple(ints)
    if not D.device:
        _call("adf_validate_disparity", D, args)
        return disparity
    if cost.device != disparity.device:
        raise AdfError(_lib.ADF_EBADARG, "cost lives on %s, disparity on %s" % (cost.device, disparity.device))
    with torch.cuda.device(disparity.device):
        _call("adf_validate_disparity", D, args)
    return disparity


def censusTransform(image, kernelSize, type, dst=None):
    """cv::stereo::censusTransform(image, kernelSize, dist, type) (descriptor.hpp:428, descriptor.cpp:77-98): the census
    descriptor of every pixel of a CV_8UC1 image (H,W) or a batch (N,H,W), `type` SGBM_COST_CENSUS_DENSE (kernelSize 3, 5,
    7: 8 / 24 / 48 bits) or SGBM_COST_CENSUS_SPARSE (5, 7, 9, 11: 8 / 16 / 24 / 36 bits); SGBM_COST_MCT_DENSE /
    SGBM_COST_MCT_SPARSE, the modified census transform (same grids, sizes and bit counts; a bit is
    k*k*neighbour > sum of the whole clamped k x k window, centre included); or SGBM_COST_CENSUS_CS, the centre-symmetric
    census (3, 5, 7, 9: 4 / 12 / 24 / 40 bits; the offsets before (0, 0) in raster order, a bit is neighbour > its
    mirror image through the centre).  The BM_COST_* twins have the same values.  The definition (replicated
    edge, bit order) is the library's own: include/adf_wls.h.  A numpy image gives an np.uint64 array through the host
    entry; a torch CUDA tensor gives an int64 tensor carrying the same bit pattern, on the device and asynchronously on
    torch's current stream.  `dst`: an output of that type and shape to write into."""
    if image is None:
        raise AdfError(_lib.ADF_EBADARG, "image is empty")
    nd = len(image.shape)
    if nd not in (2, 3):
        raise AdfError(_lib.ADF_EBADARG, "image must be (H,W) or a batch (N,H,W) of CV_8UC1 images")
    im = _Image(image, np.uint8, "image", nd == 3)
    if dst is None:
        dst = _out_like(im, nd == 3, np.uint64)
    D = _Image(dst, np.uint64, "dst", nd == 3)
    if (D.n, D.h, D.w) != (im.n, im.h, im.w) or D.device != im.device:
        raise AdfError(_lib.ADF_ESIZE, "dst must have the image's shape on its side (host or device)")
    args = (im.n, im.ptr, im.stride, im.pair_stride, im.w, im.h, int(type), int(kernelSize), D.ptr, D.stride, D.pair_stride)
    if not im.device:
        _call("adf_census_transform", im, args)
        return dst
    if dst.device != im.keep.device:
        raise AdfError(_lib.ADF_EBADARG, "dst lives on %s, image on %s" % (dst.device, im.keep.device))
    with torch.cuda.device(im.keep.device):
        _call("adf_census_transform", im, args)
    return dst


def speckleWorkspaceBytes(n, H, W):
    """Bytes of device workspace filterSpeckles needs for n maps of H x W (8 per pixel)."""
    return int(_lib.lib().adf_filter_speckles_workspace_bytes(int(n), int(W), int(H)))


# ---------------------------------------------------------------------------------------------
# The matcher's views: the two imgproc calls of the sample's default pipeline (samples/disparity_filtering.cpp:130-141)
# on the device (csrc/view_prep_kernels.hip; arithmetic and the unpinned odd-size tail: include/adf_wls.h).
# ---------------------------------------------------------------------------------------------
COLOR_BGR2GRAY = 6      # cv::COLOR_BGR2GRAY
INTER_LINEAR = 1        # cv::INTER_LINEAR


def halfSize(n):
    """cvRound(n * 0.5), half to even (adf_half_size): the size cv::resize(.., 0.5, 0.5) gives an axis of n pixels."""
    return _read(_lib.lib().adf_half_size, C.c_int, int(n))


def _view_image(src, what):
    """(_Image, batched, colour) of an 8-bit view (H,W), (H,W,3), (N,H,W) or (N,H,W,3); a three-dimensional shape that
    ends in 3 is one colour image, so a batch of 3-pixel-wide gray images is passed as (N,H,W,1)."""
    if src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s is empty" % what)
    nd = len(src.shape)
    if nd not in (2, 3, 4):
        raise AdfError(_lib.ADF_EBADARG, "%s must be (H,W[,3]) or a batch (N,H,W[,3])" % what)
    if nd == 4 and src.shape[-1] not in (1, 3):
        raise AdfError(_lib.ADF_EBADARG, "%s has %d channels; CV_8UC1 and CV_8UC3 are supported" % (what, src.shape[-1]))
    color = src.shape[-1] == 3 and nd in (3, 4)
    batched = nd == 4 or (nd == 3 and not color)
    if nd == 4 and not color:
        src = src[..., 0]                                        # (the stride of a one-element axis means nothing)
    im = _Image(src, np.uint8, what, batched, allow_channels=(3,) if color else (1,))
    im.unit_axis = nd == 4 and not color
    return im, batched, color


def _prepare_views(im, batched, half, dst_channels, dst, what):
    w, h = (halfSize(im.w), halfSize(im.h)) if half else (im.w, im.h)
    if w < 1 or h < 1:
        raise AdfError(_lib.ADF_EBADARG, "%s: the half-size image of %d x %d is empty" % (what, im.w, im.h))
    unit = im.unit_axis and dst_channels == 1                    # (N,H,W,1) in, (N,h,w,1) out
    shape = ((im.n,) if batched else ()) + (h, w) + ((3,) if dst_channels == 3 else (1,) if unit else ())
    if dst is None:
        dst = _empty(im, shape, np.uint8)
    if tuple(dst.shape) != shape:
        raise AdfError(_lib.ADF_ESIZE, "%s: dst must have shape %s" % (what, shape))
    D = _Image(dst[..., 0] if unit else dst, np.uint8, "dst", batched, allow_channels=(dst_channels,))
    if (D.n, D.h, D.w) != (im.n, h, w) or D.device != im.device:
        raise AdfError(_lib.ADF_ESIZE, "%s: dst must have shape %s on the side (host or device) of src" % (what, shape))
    args = (im.n, im.ptr, im.stride, im.pair_stride, im.w, im.h, im.c, D.ptr, D.stride, D.pair_stride, w, h, dst_channels)
    if not im.device:
        _call("adf_prepare_views", im, args)
        return dst
    if dst.device != im.keep.device:
        raise AdfError(_lib.ADF_EBADARG, "dst lives on %s, src on %s" % (dst.device, im.keep.device))
    with torch.cuda.device(im.keep.device):
        _call("adf_prepare_views", im, args)
    return dst


def resize(src, dsize=None, fx=0, fy=0, interpolation=INTER_LINEAR, dst=None):
    """cv::resize(src, dst, dsize, fx, fy, INTER_LINEAR) for the one scale the sample uses (SAMPLE:137-138):
    fx == fy == 0.5, or the `dsize` (width, height) that scale gives, (halfSize(W), halfSize(H)).  The 2x2 mean
    (a + b + c + d + 2) >> 2 per channel, bit-exact; odd sizes: include/adf_wls.h (parity unpinned).  `src` is a CV_8UC1 /
    CV_8UC3 image (H,W[,3]) or a batch (N,H,W[,3]) -- a batch of 3-pixel-wide gray images goes as (N,H,W,1) -- ; a torch
    CUDA tensor is resized on the device, asynchronously on torch's current stream (row strides of a sliced view are
    honoured), a numpy array takes the host entry point.  `dst`: an output of the right shape to write into (with it the
    device call allocates nothing and may be captured into a CUDA graph)."""
    if interpolation != INTER_LINEAR:
        raise AdfError(_lib.ADF_EBADARG, "resize supports INTER_LINEAR at a scale of exactly 0.5 only")
    im, batched, color = _view_image(src, "src")
    if dsize is not None and tuple(dsize) != (0, 0):
        if tuple(int(v) for v in dsize) != (halfSize(im.w), halfSize(im.h)):
            raise AdfError(_lib.ADF_EBADARG, "resize supports half size only: dsize must be (%d, %d) for a %d x %d image"
                           % (halfSize(im.w), halfSize(im.h), im.w, im.h))
    elif not (fx == 0.5 and fy == 0.5):
        raise AdfError(_lib.ADF_EBADARG, "resize supports fx == fy == 0.5 only (got fx=%r, fy=%r)" % (fx, fy))
    return _prepare_views(im, batched, True, im.c, dst, "resize")


def cvtColor(src, code, dst=None):
    """cv::cvtColor(src, dst, COLOR_BGR2GRAY) (SAMPLE:155-156): (B*1868 + G*9617 + R*4899 + 8192) >> 14, bit-exact.
    `src` is a CV_8UC3 image (H,W,3) or a batch (N,H,W,3), numpy (host entry) or torch CUDA (device, current stream)."""
    if code != COLOR_BGR2GRAY:
        raise AdfError(_lib.ADF_EBADARG, "cvtColor supports COLOR_BGR2GRAY only (got code %r)" % (code,))
    im, batched, color = _view_image(src, "src")
    if not color:
        raise AdfError(_lib.ADF_EBADARG, "cvtColor(COLOR_BGR2GRAY) needs a 3-channel image")
    return _prepare_views(im, batched, False, 1, dst, "cvtColor")


def matcherViews(view, scale=0.5, gray=True, dst=None):
    """Extension: what the sample feeds its matcher, from a full-size view, in ONE launch -- resize(view, 0.5, 0.5) then
    cvtColor(BGR2GRAY) without the half-size colour image ever being written (identical, bit for bit, to the two calls).
    scale 0.5 or 1.0; gray=False keeps the channels (StereoSGBM takes colour views: that is resize()).  `view` may
    hold all left and all right views of a batch in one tensor."""
    if scale not in (0.5, 1.0, 1):
        raise AdfError(_lib.ADF_EBADARG, "matcherViews supports scale 0.5 and 1.0 only (got %r)" % (scale,))
    im, batched, color = _view_image(view, "view")
    half = scale == 0.5
    to_gray = bool(gray) and color
    if not half and not to_gray:
        raise AdfError(_lib.ADF_EBADARG, "matcherViews: scale 1.0 without a colour conversion leaves nothing to do")
    return _prepare_views(im, batched, half, 1 if to_gray else im.c, dst, "matcherViews")


# ---------------------------------------------------------------------------------------------
# Reprojection to 3-D (cv::reprojectImageTo3D of calib3d, outside the reference tree) and the point list, on the device
# (csrc/reproject_kernels.hip; definition, missing values and the unpinned parity: include/adf_wls.h).
# ---------------------------------------------------------------------------------------------
CV_32F = 5              # cv's depth code, the one `ddepth` reprojectImageTo3D builds
_RP, _PC = "reprojectImageTo3D", "pointCloud"


def _reproject_source(who, disparity):
    """(_Image, batched, depth code) of a CV_16SC1 / CV_32FC1 map (H,W) or batch (N,H,W)."""
    if disparity is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: the disparity map is empty" % who)
    dt = _NUMPY_DTYPE.get(disparity.dtype if _is_torch(disparity) else np.asarray(disparity).dtype)
    if dt not in (np.int16, np.float32):
        raise AdfError(_lib.ADF_EBADARG, "%s: disparity must be CV_16SC1 or CV_32FC1" % who)
    nd = len(disparity.shape)
    if nd not in (2, 3):
        raise AdfError(_lib.ADF_EBADARG, "%s: disparity must be (H,W) or a batch (N,H,W)" % who)
    im = _Image(disparity, dt, "disparity", nd == 3)
    if im.w * im.h >= 2 ** 31:
        raise AdfError(_lib.ADF_ESIZE, "%s: W*H must be below 2^31" % who)
    return im, nd == 3, _DEPTH[dt]


def _reproject_params(who, Q, dispScale, handleMissingValues, missingValue):
    """adf_reproject_params from cv's arguments: missingValue (when given) selects ADF_MISSING_VALUE, else
    handleMissingValues selects ADF_MISSING_MIN."""
    if _is_torch(Q):
        Q = Q.detach().cpu().numpy()
    try:
        q = np.asarray(Q, dtype=np.float64)
    except (TypeError, ValueError):
        q = np.zeros(0)
    if q.shape != (4, 4):
        raise AdfError(_lib.ADF_EBADARG, "%s: Q must be a 4x4 matrix" % who)
    prm = _lib.ReprojectParams()
    prm.Q[:] = [float(v) for v in q.ravel()]
    prm.disp_scale = float(dispScale)
    if not math.isfinite(prm.disp_scale):
        raise AdfError(_lib.ADF_EBADARG, "%s: disp_scale must be finite" % who)
    prm.missing_mode, prm.missing_value = _lib.MISSING_MIN if handleMissingValues else _lib.MISSING_NONE, 0.0
    if missingValue is not None:
        prm.missing_mode, prm.missing_value = _lib.MISSING_VALUE, float(missingValue)
        if not math.isfinite(prm.missing_value):
            raise AdfError(_lib.ADF_EBADARG, "%s: missing_value must be finite" % who)
    return prm


def reprojectWorkspaceBytes(n):
    """Bytes of device workspace reprojectImageTo3D needs for n maps (4 per map; read with handleMissingValues only)."""
    return int(_lib.lib().adf_reproject_workspace_bytes(int(n)))


def pointCloudWorkspaceBytes(n, H, W):
    """Bytes of device workspace the point list of n maps of H x W needs (adf_point_cloud_workspace_bytes)."""
    return int(_lib.lib().adf_point_cloud_workspace_bytes(int(n), int(W), int(H)))


def reprojectImageTo3D(disparity, Q, handleMissingValues=False, ddepth=-1, dst=None, dispScale=1.0, missingValue=None,
                       zOnly=False, buf=None):
    """cv::reprojectImageTo3D(disparity, _3dImage, Q, handleMissingValues, ddepth) (calib3d): the CV_32FC3 image of
    (X, Y, Z) = Q * (x, y, d, 1) / W for a CV_16SC1 / CV_32FC1 map (H,W) or a batch (N,H,W) -> (H,W,3) / (N,H,W,3), every
    step one binary64 operation in the order include/adf_wls.h states (bit-exact against tests/reproject_ref.py; parity
    with calib3d is unpinned).  A numpy map takes the host entry; a torch CUDA tensor runs on the device, asynchronously
    on torch's current stream (row strides of a sliced view are honoured).  `Q`: any 4x4 array-like.  `ddepth`: -1 or
    CV_32F.  handleMissingValues: pixels at the map's minimum get Z = 10000 (each map of a batch has its own minimum).
    Extensions: `dispScale` multiplies the raw value first (1/16 turns the filters' fixed-point units into pixels; cv
    itself never divides), `missingValue` names the missing value instead of reducing for the minimum (-16 for filterFloat
    output), `zOnly` gives the Z plane (H,W) alone, `dst` an output to write into, `buf` (device path with
    handleMissingValues) a CUDA tensor of at least reprojectWorkspaceBytes(N) bytes: with it, or without
    handleMissingValues, the call allocates nothing and may be captured into a CUDA graph."""
    if ddepth not in (-1, CV_32F):
        raise AdfError(_lib.ADF_EBADARG, "%s: ddepth must be -1 or CV_32F (CV_16SC3 and CV_32SC3 are not built)" % _RP)
    im, batched, depth = _reproject_source(_RP, disparity)
    prm = _reproject_params(_RP, Q, dispScale, handleMissingValues, missingValue)
    ch = 1 if zOnly else 3
    shape = ((im.n,) if batched else ()) + (im.h, im.w) + (() if zOnly else (3,))
    if dst is None:
        dst = _empty(im, shape, np.float32)
    if tuple(dst.shape) != shape:
        raise AdfError(_lib.ADF_ESIZE, "%s: dst must have shape %s" % (_RP, shape))
    D = _Image(dst, np.float32, "dst", batched, allow_channels=(ch,))
    if D.device != im.device:
        raise AdfError(_lib.ADF_ESIZE, "%s: dst must have shape %s on the side (host or device) of disparity" % (_RP, shape))
    args = (im.n, im.ptr, depth, im.stride, im.pair_stride, im.w, im.h, C.byref(prm), D.ptr, D.stride, D.pair_stride, ch)
    if not im.device:
        _call("adf_reproject_to_3d", im, args)
        return dst
    if dst.device != im.keep.device:
        raise AdfError(_lib.ADF_EBADARG, "dst lives on %s, disparity on %s" % (dst.device, im.keep.device))
    ws, ws_bytes = None, 0
    if buf is not None:
        if not (_is_torch(buf) and buf.is_cuda and buf.is_contiguous()):
            raise AdfError(_lib.ADF_EBADARG, "buf must be a contiguous CUDA tensor (or None)")
        if buf.device != im.keep.device:
            raise AdfError(_lib.ADF_EBADARG, "buf lives on %s, disparity on %s" % (buf.device, im.keep.device))
        ws, ws_bytes = buf.data_ptr(), buf.numel() * buf.element_size()
        if prm.missing_mode == _lib.MISSING_MIN and ws_bytes < reprojectWorkspaceBytes(im.n):
            raise AdfError(_lib.ADF_ESIZE, "buf holds %d bytes; %d needed" % (ws_bytes, reprojectWorkspaceBytes(im.n)))
    with torch.cuda.device(im.keep.device):
        _call("adf_reproject_to_3d", im, args + (ws, ws_bytes))
    return dst


def pointCloud(disparity, Q, view=None, ROI=None, zRange=None, handleMissingValues=False, missingValue=None, dispScale=1.0,
               capacity=None, withIndex=False):
    """Extension: the compact list of the valid points of a map, without the (H,W,3) image ever being written.  A pixel
    is valid when it lies inside `ROI` ((x, y, w, h); None = the whole map), is not missing (handleMissingValues /
    missingValue as in reprojectImageTo3D), its X, Y, Z are finite and zRange[0] <= Z <= zRange[1] (`zRange` None = no
    range).  Returns (points, colours, index, count): points (count,3) float32 in raster order with the bits
    reprojectImageTo3D gives, colours (count,C) uint8 from `view` ((H,W) or (H,W,C), C 1 or 3; None without a view), index
    (count,) int32 = y*W + x with withIndex (else None), count = the number of valid pixels.  `capacity` bounds the entries
    written (default: the ROI's area); count is the full number even then, and the outputs are trimmed to
    min(count, capacity).  THE TRIM COSTS ONE HOST READ OF THE COUNT: on the device path the call synchronises torch's
    current stream once (callers that must not wait use adf_point_cloud_device).  A batch (N,H,W) gives four lists."""
    im, batched, depth = _reproject_source(_PC, disparity)
    prm = _reproject_params(_PC, Q, dispScale, handleMissingValues, missingValue)
    roi = _as_rect(ROI) or Rect(0, 0, im.w, im.h)
    if roi.x < 0 or roi.y < 0 or roi.width < 1 or roi.height < 1 or roi.x > im.w - roi.width or roi.y > im.h - roi.height:
        raise AdfError(_lib.ADF_ESIZE, "%s: ROI does not fit the map" % _PC)
    z_min, z_max = (-math.inf, math.inf) if zRange is None else (float(zRange[0]), float(zRange[1]))
    if math.isnan(z_min) or math.isnan(z_max):
        raise AdfError(_lib.ADF_EBADARG, "%s: z_min and z_max must not be NaN" % _PC)
    area = roi.width * roi.height
    if capacity is None:
        capacity = area
    capacity = int(capacity)
    if capacity < 0:
        raise AdfError(_lib.ADF_EBADARG, "%s: capacity must not be negative" % _PC)
    capacity = min(capacity, _INT32_MAX)
    V, vch = None, 0
    if view is not None:
        nd = len(disparity.shape)
        extra = len(view.shape) - nd
        if extra not in (0, 1) or tuple(view.shape[:nd]) != tuple(disparity.shape):
            raise AdfError(_lib.ADF_ESIZE, "%s: view must have the disparity map's size" % _PC)
        vch = view.shape[-1] if extra else 1
        if vch not in (1, 3):
            raise AdfError(_lib.ADF_EBADARG, "%s: view_channels must be 1 or 3" % _PC)
        V = _Image(view[..., 0] if extra and vch == 1 else view, np.uint8, "view", batched, allow_channels=(vch,))
        if V.device != im.device:
            raise AdfError(_lib.ADF_EBADARG, "inputs must all be numpy arrays or all be CUDA tensors")
    rows = max(1, min(capacity, area))                           # (an empty tensor has no pointer to pass)
    if im.device:
        dev = im.keep.device
        if V is not None and V.keep.device != dev:
            raise AdfError(_lib.ADF_EBADARG, "view lives on %s, disparity on %s" % (V.keep.device, dev))
        points = torch.empty((im.n, rows, 3), dtype=torch.float32, device=dev)
        colours = torch.empty((im.n, rows, vch), dtype=torch.uint8, device=dev) if V is not None else None
        index = torch.empty((im.n, rows), dtype=torch.int32, device=dev) if withIndex else None
        counts = torch.empty((im.n,), dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
    else:
        points = np.empty((im.n, rows, 3), np.float32)
        colours = np.empty((im.n, rows, vch), np.uint8) if V is not None else None
        index = np.empty((im.n, rows), np.int32) if withIndex else None
        counts = np.zeros((im.n,), np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data
    args = (im.n, im.ptr, depth, im.stride, im.pair_stride, im.w, im.h, C.byref(prm), C.byref(roi), z_min, z_max,
            None if V is None else V.ptr, 0 if V is None else V.stride, 0 if V is None else V.pair_stride, vch,
            ptr(points), rows * 12, ptr(colours), rows * vch, ptr(index), rows * 4, capacity, ptr(counts))
    if im.device:
        with torch.cuda.device(im.keep.device):
            _call("adf_point_cloud", im, args + (None, 0))
        got = [int(c) for c in counts.cpu().tolist()]            # the one host read (synchronises the current stream)
    else:
        _call("adf_point_cloud", im, args)
        got = [int(c) for c in counts]
    keep = [min(c, capacity) for c in got]
    cut = lambda a: [None] * im.n if a is None else [a[k, :keep[k]] for k in range(im.n)]
    P, Cl, I = cut(points), cut(colours), cut(index)
    if batched:
        return P, Cl, I, got
    return P[0], Cl[0], I[0], got[0]


# ---------------------------------------------------------------------------------------------
# Rectification (cv::initUndistortRectifyMap of calib3d, cv::remap of imgproc, outside the reference tree) on the device
# (csrc/rectify_kernels.hip; definition, limits and the unpinned parity: include/adf_wls.h, "rectification").
# ---------------------------------------------------------------------------------------------
CV_32FC1 = 5            # cv's type code of the one map form that is built
BORDER_CONSTANT = 0     # cv::BORDER_CONSTANT
_IM, _RM, _RV = "initUndistortRectifyMap", "remap", "rectifyViews"


def _matrix(who, name, m, shapes):
    """A host float64 matrix of one of `shapes` from any array-like (a tensor is read back)."""
    if _is_torch(m):
        m = m.detach().cpu().numpy()
    try:
        a = np.ascontiguousarray(m, dtype=np.float64)
    except (TypeError, ValueError):
        a = np.zeros(0)
    if a.shape not in shapes:
        raise AdfError(_lib.ADF_EBADARG, "%s: %s must be a %s matrix" % (who, name, " or ".join("%dx%d" % s for s in shapes)))
    return a


def rectifyParams(cameraMatrix, distCoeffs=None, R=None, newCameraMatrix=None, who="rectifyParams"):
    """adf_rectify_params from cv's arguments, through adf_rectify_params_init (the one inverse every layer shares).
    distCoeffs: None or 0, 4, 5 or 8 numbers in cv's order; R: None (identity) or 3x3; newCameraMatrix: 3x3 or 3x4 (P1 / P2
    of stereoRectify), None = cameraMatrix."""
    K = _matrix(who, "cameraMatrix", cameraMatrix, ((3, 3),))
    P = K if newCameraMatrix is None else _matrix(who, "newCameraMatrix", newCameraMatrix, ((3, 3), (3, 4)))
    Rm = None if R is None else _matrix(who, "R", R, ((3, 3),))
    if _is_torch(distCoeffs):
        distCoeffs = distCoeffs.detach().cpu().numpy()
    d = np.zeros(0) if distCoeffs is None else np.ascontiguousarray(distCoeffs, dtype=np.float64).ravel()
    prm = _lib.RectifyParams()
    _lib.check(_lib.lib().adf_rectify_params_init(K.ctypes.data, d.ctypes.data if d.size else None, int(d.size),
                                                  None if Rm is None else Rm.ctypes.data, P.ctypes.data, P.shape[1], C.byref(prm)))
    return prm


def _border(who, borderValue, ch):
    """The three bytes of border_value from a scalar or a 3-tuple (cv::Scalar: a scalar sets the first channel only in
    cv; here a scalar means every channel, which is what a gray fill wants)."""
    try:
        vals = [float(v) for v in borderValue] if hasattr(borderValue, "__len__") else [float(borderValue)] * 3
    except (TypeError, ValueError):
        vals = []
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) not in (3, 4) or any(not (0 <= v <= 255) or v != int(v) for v in vals[:3]):
        raise AdfError(_lib.ADF_EBADARG, "%s: borderValue must be an integer in [0, 255] or three of them" % who)
    return (C.c_uint8 * 3)(*[int(v) for v in vals[:3]])


def _on_device(im, fn):
    if not im.device:
        return fn()
    with torch.cuda.device(im.keep.device):
        return fn()


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type=CV_32FC1, device=None):
    """cv::initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, CV_32FC1) -> (map1, map2): the two
    float planes (H,W) of source coordinates for `size` = (width, height), every step one binary64 operation in the order
    include/adf_wls.h states (bit-exact against tests/rectify_ref.py; parity with calib3d is unpinned).  Only m1type
    CV_32FC1 is built (no CV_16SC2 pair, no convertMaps).  `device`: None gives numpy arrays through the host entry; a
    torch device (or "cuda") gives CUDA tensors computed on it, asynchronously on torch's current stream."""
    if m1type != CV_32FC1:
        raise AdfError(_lib.ADF_EBADARG, "%s: m1type must be CV_32FC1 (the CV_16SC2 pair is not built)" % _IM)
    prm = rectifyParams(cameraMatrix, distCoeffs, R, newCameraMatrix, _IM)
    try:
        W, H = int(size[0]), int(size[1])
    except (TypeError, ValueError, IndexError):
        raise AdfError(_lib.ADF_EBADARG, "%s: size must be (width, height)" % _IM)
    if W < 1 or H < 1:
        raise AdfError(_lib.ADF_EBADARG, "%s: the size is empty" % _IM)
    if W * H >= 2 ** 31:
        raise AdfError(_lib.ADF_ESIZE, "%s: W*H must be below 2^31" % _IM)
    if device is None:
        m1, m2 = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
    else:
        if torch is None:
            raise AdfError(_lib.ADF_EBADARG, "%s: device maps need torch" % _IM)
        m1 = torch.empty((H, W), dtype=torch.float32, device=device)
        m2 = torch.empty_like(m1)
        if not m1.is_cuda:
            raise AdfError(_lib.ADF_EBADARG, "%s: device must be a CUDA device (None gives numpy arrays)" % _IM)
    X, Y = _Image(m1, np.float32, "map1", False), _Image(m2, np.float32, "map2", False)
    _on_device(X, lambda: _call("adf_init_undistort_rectify_map", X, (C.byref(prm), W, H, X.ptr, X.stride, Y.ptr, Y.stride)))
    return m1, m2


def _sample(who, src, maps, prm, W, H, borderValue, dst):
    """The common part of remap and rectifyViews: `maps` = (X, Y) _Images or None, `prm` = RectifyParams or None."""
    im, batched, color = _view_image(src, "src")
    if im.w > 32767 or im.h > 32767:
        raise AdfError(_lib.ADF_ESIZE, "%s: srcW and srcH must not exceed 32767" % who)
    if W * H >= 2 ** 31:
        raise AdfError(_lib.ADF_ESIZE, "%s: W*H must be below 2^31" % who)
    border = _border(who, borderValue, im.c)
    shape = ((im.n,) if batched else ()) + (H, W) + ((3,) if color else (1,) if im.unit_axis else ())
    if dst is None:
        dst = _empty(im, shape, np.uint8)
    if tuple(dst.shape) != shape:
        raise AdfError(_lib.ADF_ESIZE, "%s: dst must have shape %s" % (who, shape))
    D = _Image(dst[..., 0] if im.unit_axis else dst, np.uint8, "dst", batched, allow_channels=(im.c,))
    if D.device != im.device or (im.device and dst.device != im.keep.device):
        raise AdfError(_lib.ADF_ESIZE, "%s: dst must have shape %s where src lives (host, or the same device)" % (who, shape))
    head = (im.n, im.ptr, im.stride, im.pair_stride, im.w, im.h, im.c)
    tail = (D.ptr, D.stride, D.pair_stride, W, H, INTER_LINEAR, BORDER_CONSTANT, border)
    if maps is not None:
        X, Y = maps
        for m in maps:
            if m.device != im.device or (im.device and m.keep.device != im.keep.device):
                raise AdfError(_lib.ADF_EBADARG, "%s: the maps must live where src lives (host, or the same device)" % who)
        _on_device(im, lambda: _call("adf_remap", im, head + (X.ptr, X.stride, Y.ptr, Y.stride) + tail))
    else:
        _on_device(im, lambda: _call("adf_rectify_views", im, head + (C.byref(prm),) + tail))
    return dst


def remap(src, map1, map2, interpolation=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0, dst=None):
    """cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, borderValue) with a CV_32FC1 map pair (H,W): bilinear
    with 5 fractional bits, the integer form include/adf_wls.h states (bit-exact against tests/rectify_ref.py).  `src` is a
    CV_8UC1 / CV_8UC3 image (h,w[,3]) of any size up to 32767 x 32767 or a batch (N,h,w[,3]); one map pair serves the whole
    batch.  numpy arrays take the host entry, torch CUDA tensors run on the device on torch's current stream (with `dst`
    given nothing is allocated: capturable).  Other interpolations and border modes are refused.  `borderValue`: an integer
    for every channel, or three."""
    if interpolation != INTER_LINEAR or borderMode != BORDER_CONSTANT:
        raise AdfError(_lib.ADF_EBADARG, "%s: INTER_LINEAR with BORDER_CONSTANT only" % _RM)
    if map1 is None or map2 is None or len(map1.shape) != 2 or tuple(map1.shape) != tuple(map2.shape):
        raise AdfError(_lib.ADF_EBADARG, "%s: map1 and map2 must be two CV_32FC1 planes (H,W) of one size" % _RM)
    X, Y = _Image(map1, np.float32, "map1", False), _Image(map2, np.float32, "map2", False)
    return _sample(_RM, src, (X, Y), None, X.w, X.h, borderValue, dst)


def rectifyViews(src, cameraMatrix, distCoeffs, R, newCameraMatrix, size=None, borderValue=0, dst=None):
    """Extension: remap(src, *initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size)) in ONE launch,
    bit for bit, without the maps ever being written: the per-frame call (one read of the source, one write of the
    destination).  `size` = (width, height) of the rectified view, None = the source's.  `src` may hold every view of one
    camera in a batch; the two cameras of a rig have different parameters and take two calls."""
    im, _, _ = _view_image(src, "src")
    try:
        W, H = (im.w, im.h) if size is None else (int(size[0]), int(size[1]))
    except (TypeError, ValueError, IndexError):
        raise AdfError(_lib.ADF_EBADARG, "%s: size must be (width, height)" % _RV)
    if W < 1 or H < 1:
        raise AdfError(_lib.ADF_EBADARG, "%s: the size is empty" % _RV)
    prm = rectifyParams(cameraMatrix, distCoeffs, R, newCameraMatrix, _RV)
    return _sample(_RV, src, None, prm, W, H, borderValue, dst)


# ---------------------------------------------------------------------------------------------
# Weighted median filter: cv::ximgproc::weightedMedianFilter (weighted_median_filter.hpp:64-90) in the library's own
# integer definition (include/adf_wls.h; csrc/wmf_kernels.hip; the direct statement is tests/wmf_ref.py).
# ---------------------------------------------------------------------------------------------
_WMF = "weightedMedianFilter"
_WMF_NOT_BUILT = {WMF_IV1: "WMF_IV1", WMF_IV2: "WMF_IV2", WMF_COS: "WMF_COS", WMF_JAC: "WMF_JAC"}


def _choice(who, value, accepted, not_built, must, are, unknown=None):
    """int(value) when it is one of `accepted`.  A value of cv's that this build leaves out is refused by its name in
    `not_built` -- any other integer too, worded by `unknown`, where the filter has such a text -- with what IS built
    (`are`); everything else with what the parameter must be (`must`)."""
    try:
        v = int(value)
    except (TypeError, ValueError):
        raise AdfError(_lib.ADF_EBADARG, "%s: %s" % (who, must))
    if v in accepted:
        return v
    name = not_built.get(v) or (unknown and unknown % v)
    if name:
        raise AdfError(_lib.ADF_EBADARG, "%s: %s is not built; %s" % (who, name, are))
    raise AdfError(_lib.ADF_EBADARG, "%s: %s" % (who, must))


_wmf_weight_type = functools.partial(_choice, accepted=(WMF_EXP, WMF_OFF), not_built=_WMF_NOT_BUILT,   # (who, weightType)
                                     must="weightType must be WMF_EXP or WMF_OFF", are="WMF_EXP and WMF_OFF are")


CV_8U, CV_16S = 0, 3    # cv's depth codes (CV_32F is above): what dDepth takes
_GF_DTYPE = {CV_8U: np.uint8, CV_16S: np.int16, CV_32F: np.float32}


def _filter_images(who, src, dst, dDepth=-1, guide=None, role="guide", mask=None, suffix="", float_guide=None, in_place=None):
    """What the five edge-aware filters ask of their images, in the one order they all report it -> (S, G, M, D, dst,
    dt, ddt): the _Images of src, of the guide or joint (`role` names it; None: the filter has none), of the mask (None:
    none) and of dst -- made here, of dtype ddt, when None --, src's dtype and dst's.  A filter without a dDepth leaves
    it at -1: dst has src's dtype.  `suffix` ends the refusal of a src that is no map or batch; `float_guide` and
    `in_place` word one filter's own refusal (a float32 joint; dst is src) at its place in that order."""
    nd = len(src.shape)
    if nd not in (2, 3):
        raise AdfError(_lib.ADF_EBADARG, "%s: src must be (H,W) or a batch (N,H,W) of one-channel maps%s" % (who, suffix))
    batched = nd == 3
    for dt in (np.uint8, np.int16, np.float32):
        if _map_dtype(src, dt) is not None:
            break
    else:
        raise AdfError(_lib.ADF_EBADARG, "%s: src must be uint8 (CV_8U), int16 (CV_16S) or float32 (CV_32F)" % who)
    if float_guide and _map_dtype(guide, np.float32) is not None:
        raise AdfError(_lib.ADF_EBADARG, "%s: %s" % (who, float_guide))
    if dDepth != -1 and dDepth not in _GF_DTYPE:
        raise AdfError(_lib.ADF_EBADARG, "%s: dDepth must be -1, CV_8U, CV_16S or CV_32F" % who)
    ddt = dt if dDepth == -1 else _GF_DTYPE[dDepth]
    S = _Image(src, dt, "src", batched)
    G = None if guide is None else _Image(guide, np.uint8, role, batched, allow_channels=(1, 3))
    M = None if mask is None else _Image(mask, np.uint8, "mask", batched)
    if in_place and dst is src:
        raise AdfError(_lib.ADF_EBADARG, "%s: %s" % (who, in_place))
    if dst is None:
        dst = _out_like(S, batched, ddt)
    D = _Image(dst, ddt, "dst", batched)
    for im, what in ((G, role), (M, "mask"), (D, "dst")):
        if im is None:
            continue
        if (im.n, im.h, im.w) != (S.n, S.h, S.w) or im.device != S.device:
            raise AdfError(_lib.ADF_ESIZE, "%s: %s must have src's size on its side (host or device)" % (who, what))
        if S.device and im.keep.device != S.keep.device:
            raise AdfError(_lib.ADF_EBADARG, "%s: %s lives on %s, src on %s" % (who, what, im.keep.device, S.keep.device))
    return S, G, M, D, dst, dt, ddt


def _workspace(who, S, workspace):
    """(pointer, bytes) of a caller's workspace for a call on S's device: a contiguous CUDA tensor there; (None, 0) for None."""
    if workspace is None:
        return None, 0
    if not S.device:
        raise AdfError(_lib.ADF_EBADARG, "%s: a workspace goes with CUDA tensors only" % who)
    if not (_is_torch(workspace) and workspace.is_cuda and workspace.is_contiguous()):
        raise AdfError(_lib.ADF_EBADARG, "%s: workspace must be a contiguous CUDA tensor (or None)" % who)
    if workspace.device != S.keep.device:
        raise AdfError(_lib.ADF_EBADARG, "%s: workspace lives on %s, src on %s" % (who, workspace.device, S.keep.device))
    return workspace.data_ptr(), workspace.numel() * workspace.element_size()


def _filter_call(name, S, args, ws=None):
    """The entry `name` on S's side, on S's device when it has one; `ws` (the device entry alone takes one) follows args."""
    if not S.device:
        _call(name, S, args)
        return
    with torch.cuda.device(S.keep.device):     # (spelled out, not _on_device: this runs once per filter call)
        _call(name, S, args + ws if ws else args)


def wmfWeightTable(sigma, weightType=WMF_EXP):
    """The weight table T of weightedMedianFilter exactly as its calls build it (adf_wmf_weight_table_host): 3*256*256
    uint32 entries indexed by the squared joint distance, lrint(exp(-i / (2 sigma^2)) * 65536) for WMF_EXP, all 65536 for
    WMF_OFF.  Host only: no device is touched."""
    wt = _wmf_weight_type("wmfWeightTable", weightType)
    table = np.empty(_lib.WMF_TABLE_LEVELS, np.uint32)
    _lib.check(_lib.lib().adf_wmf_weight_table_host(float(sigma), wt, table.ctypes.data, table.size))
    return table


def weightedMedianFilter(joint, src, r, sigma=25.5, weightType=WMF_EXP, mask=None, ignoreValue=None, dst=None):
    """cv::ximgproc::weightedMedianFilter(joint, src, dst, r, sigma, weightType, mask) in the library's own integer
    definition (include/adf_wls.h): per pixel the weighted median of the used pixels of the (2r+1)^2 window clipped at the
    border, with weights T[squared joint distance] -- the smallest window value v whose weight at or below it reaches half
    the total.  `src`: uint8, int16 or float32, (H,W) or a batch (N,H,W), one channel; `joint`: uint8 of that size with 1
    or 3 channels; `mask`: uint8, 0 = ignored.  Extension: `ignoreValue` -- pixels holding it are ignored too, and get a
    value from their neighbours: (minDisparity-1)*16 fills the holes validateDisparity and filterSpeckles leave.  A pixel
    whose window has no used pixel of positive weight keeps its value.  1 <= r <= 31; weightType WMF_EXP or WMF_OFF (the
    plain median); WMF_IV1, WMF_IV2, WMF_COS, WMF_JAC and multi-channel sources are not built.  Torch CUDA tensors run on
    the device, asynchronously on torch's current stream (the first call with a new sigma uploads its table
    synchronously and cannot be captured into a graph; later ones can); numpy arrays take the host entry point.
    Returns dst, which must not overlap the inputs."""
    if joint is None or src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: joint and src must not be empty" % _WMF)
    wt = _wmf_weight_type(_WMF, weightType)
    S, J, M, D, dst, dt, _ = _filter_images(_WMF, src, dst, -1, joint, "joint", mask)
    args = (S.n, J.ptr, J.stride, J.pair_stride, J.c, S.ptr, S.stride, S.pair_stride, _DEPTH[dt], D.ptr, D.stride, D.pair_stride,
            S.w, S.h, int(r), float(sigma), wt, M.ptr if M else None, M.stride if M else 0, M.pair_stride if M else 0,
            0 if ignoreValue is None else 1, 0.0 if ignoreValue is None else float(ignoreValue))
    _filter_call("adf_weighted_median_filter", S, args)
    return dst

# ---------------------------------------------------------------------------------------------
# cv::ximgproc::guidedFilter / createGuidedFilter / GuidedFilter (EF.hpp:143-180, guided_filter.cpp) in the library's own
# exact definition (include/adf_wls.h; csrc/guided_filter_kernels.hip; the direct statement is tests/gf_ref.py).
# ---------------------------------------------------------------------------------------------
_GF = "guidedFilter"


def guidedFilterWorkspaceBytes(n, H, W, channels):
    """Bytes of device workspace guidedFilter needs for n maps of H x W under a guide of `channels` channels
    (adf_guided_filter_workspace_bytes): the channels + 1 float coefficient planes between its two launches."""
    return int(_lib.lib().adf_guided_filter_workspace_bytes(int(n), int(W), int(H), int(channels)))


def guidedFilter(guide, src, radius, eps, dDepth=-1, dst=None, workspace=None):
    """cv::ximgproc::guidedFilter(guide, src, dst, radius, eps, dDepth) in the library's own definition (include/adf_wls.h):
    per (2 radius + 1)^2 window, BORDER_REFLECT, the linear model q = a . guide + b of the source with regulariser eps (in
    squared grey levels of the 0..255 guide), the models covering a pixel averaged -- exact integer statistics, one stated
    operation order, bit-exact against tests/gf_ref.py.

        guide    uint8, (H,W) or (H,W,3); with a batch (N,H,W) or (N,H,W,3)
        src      uint8, int16 or float32, (H,W) or a batch (N,H,W), one channel
        radius   0 .. 31 (GF_MAX_RADIUS)
        eps      finite, > 0
        dDepth   -1 = src's depth, or CV_8U, CV_16S, CV_32F: integer outputs are rounded half to even and saturated
        dst      None, or an array / tensor of that depth and src's shape that overlaps neither input

    The filter is not blind to a matcher's invalid value (minDisparity-1)*16: fill the holes first (weightedMedianFilter
    with ignoreValue).  Multi-channel sources are not built: split them.  Torch CUDA tensors run on the device,
    asynchronously on torch's current stream; `workspace` (device path only): a CUDA tensor of at least
    guidedFilterWorkspaceBytes(...) bytes -- the call then allocates nothing and may be captured into a CUDA graph; None =
    the library's cached scratch.  Numpy arrays take the host entry point.  Returns dst."""
    if guide is None or src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: guide and src must not be empty" % _GF)
    S, G, _, D, dst, dt, ddt = _filter_images(_GF, src, dst, dDepth, guide)
    args = (S.n, G.ptr, G.stride, G.pair_stride, G.c, S.ptr, S.stride, S.pair_stride, _DEPTH[dt], D.ptr, D.stride, D.pair_stride,
            _DEPTH[ddt], S.w, S.h, int(radius), float(eps))
    _filter_call("adf_guided_filter", S, args, _workspace(_GF, S, workspace))
    return dst


class GuidedFilter:
    """cv::ximgproc::GuidedFilter (EF.hpp:130-144): holds the guide, radius and eps; filter(src) is
    guidedFilter(guide, src, radius, eps).  The guide's statistics are recomputed per call (they ride along in the
    coefficient kernel), so the object saves no work: it is the reference's interface."""

    def __init__(self, guide, radius, eps):
        if guide is None:
            raise AdfError(_lib.ADF_EBADARG, "%s: guide must not be empty" % _GF)
        if not (0 <= int(radius) <= GF_MAX_RADIUS):
            raise AdfError(_lib.ADF_EBADARG, "%s: radius must lie in [0, %d]" % (_GF, GF_MAX_RADIUS))
        if not (math.isfinite(float(eps)) and float(eps) > 0):
            raise AdfError(_lib.ADF_EBADARG, "%s: eps must be finite and > 0" % _GF)
        self._guide, self._radius, self._eps = guide, int(radius), float(eps)

    def filter(self, src, dst=None, dDepth=-1, workspace=None):
        return guidedFilter(self._guide, src, self._radius, self._eps, dDepth, dst, workspace)


def createGuidedFilter(guide, radius, eps):
    """EF.hpp:158: a GuidedFilter on `guide` (held by reference, not copied)."""
    return GuidedFilter(guide, radius, eps)


# ---------------------------------------------------------------------------------------------
# cv::ximgproc::dtFilter / createDTFilter / DTFilter (EF.hpp:66-121, dtfilter_cpu.hpp) in mode DTF_RF, in the library's own
# exact definition (include/adf_wls.h; csrc/dt_filter_kernels.hip; the direct statement is tests/dt_ref.py).
# ---------------------------------------------------------------------------------------------
_DT = "dtFilter"
_DT_NOT_BUILT = {DTF_NC: "DTF_NC", DTF_IC: "DTF_IC"}


_dt_mode = functools.partial(_choice, accepted=(DTF_RF,), not_built=_DT_NOT_BUILT, must="mode must be DTF_RF", are="DTF_RF is")   # (who, mode)


def dtRfTable(sigmaSpatial, sigmaColor, numIters=3, channels=1):
    """The feedback table of dtFilter's DTF_RF mode exactly as its calls build it (adf_dt_rf_table_host): float32,
    (max(1, numIters), 255 * channels + 1); row i - 1 holds A_i[L] for the L1 guide difference L.  Host only: no device is
    touched."""
    n = max(1, int(numIters))
    if n > DT_MAX_ITERS or int(channels) not in (1, 3):     # (the library refuses them too; the array is sized first)
        raise AdfError(_lib.ADF_EBADARG, "dtRfTable: numIters must not exceed %d, channels must be 1 or 3" % DT_MAX_ITERS)
    table = np.empty((n, 255 * int(channels) + 1), np.float32)
    _lib.check(_lib.lib().adf_dt_rf_table_host(float(sigmaSpatial), float(sigmaColor), int(numIters), int(channels), table.ctypes.data))
    return table


def dtFilterWorkspaceBytes(n, H, W):
    """Bytes of device workspace dtFilter needs for n maps of H x W (adf_dt_filter_workspace_bytes): one float plane per
    map, which holds the map between the passes."""
    return int(_lib.lib().adf_dt_filter_workspace_bytes(int(n), int(W), int(H)))


def dtFilter(guide, src, sigmaSpatial, sigmaColor, mode=DTF_RF, numIters=3, dDepth=-1, dst=None, workspace=None):
    """cv::ximgproc::dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters) in mode DTF_RF, in the library's
    own definition (include/adf_wls.h): numIters times, a recursive sweep along every row there and back, then along every
    column, x[j] += A[L] (x[j-1] - x[j]) with the feedback A falling with the guide's L1 difference L between the two
    pixels -- one stated operation order, bit-exact against tests/dt_ref.py fed with dtRfTable.

        guide         uint8, (H,W) or (H,W,3); with a batch (N,H,W) or (N,H,W,3)
        src           uint8, int16 or float32, (H,W) or a batch (N,H,W), one channel
        sigmaSpatial  clamped to >= 1;  sigmaColor  clamped to >= 0.01 (in grey levels of the 0..255 guide); both finite
        mode          DTF_RF.  The reference's default is DTF_NC, which this call refuses, as it does DTF_IC: the default
                      HERE is DTF_RF.  DTF_NC is dtWindowFilter
        numIters      clamped to >= 1, at most 8 (DT_MAX_ITERS)
        dDepth        -1 = src's depth, or CV_8U, CV_16S, CV_32F: integer outputs are rounded half to even and saturated
        dst           None, or an array / tensor of that depth and src's shape that overlaps neither input

    The filter is not blind to a matcher's invalid value (minDisparity-1)*16: fill the holes first (weightedMedianFilter
    with ignoreValue).  Multi-channel sources are not built: split them.  Torch CUDA tensors run on the device,
    asynchronously on torch's current stream; `workspace` (device path only): a CUDA tensor of at least
    dtFilterWorkspaceBytes(...) bytes -- the call then allocates nothing and may be captured into a CUDA graph; None =
    the library's cached scratch.  Numpy arrays take the host entry point.  Returns dst."""
    if guide is None or src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: guide and src must not be empty" % _DT)
    m = _dt_mode(_DT, mode)
    S, G, _, D, dst, dt, ddt = _filter_images(_DT, src, dst, dDepth, guide)
    args = (S.n, G.ptr, G.stride, G.pair_stride, G.c, S.ptr, S.stride, S.pair_stride, _DEPTH[dt], D.ptr, D.stride, D.pair_stride,
            _DEPTH[ddt], S.w, S.h, float(sigmaSpatial), float(sigmaColor), m, int(numIters))
    _filter_call("adf_dt_filter", S, args, _workspace(_DT, S, workspace))
    return dst


class DTFilter:
    """cv::ximgproc::DTFilter (EF.hpp:66-84): holds the guide and the parameters; filter(src) is dtFilter(guide, src, ...).
    There is no init stage -- the weights are one table read per step, recomputed from the guide in every sweep -- so the
    object saves no work: it is the reference's interface.  As with dtFilter, the default mode is DTF_RF (the reference's
    DTF_NC is not built)."""

    def __init__(self, guide, sigmaSpatial, sigmaColor, mode=DTF_RF, numIters=3):
        if guide is None:
            raise AdfError(_lib.ADF_EBADARG, "%s: guide must not be empty" % _DT)
        m = _dt_mode(_DT, mode)
        if not (math.isfinite(float(sigmaSpatial)) and math.isfinite(float(sigmaColor))):
            raise AdfError(_lib.ADF_EBADARG, "%s: sigmaSpatial and sigmaColor must be finite" % _DT)
        if int(numIters) > DT_MAX_ITERS:
            raise AdfError(_lib.ADF_EBADARG, "%s: numIters must not exceed %d" % (_DT, DT_MAX_ITERS))
        self._guide, self._ss, self._sr, self._mode, self._iters = guide, float(sigmaSpatial), float(sigmaColor), m, int(numIters)

    def filter(self, src, dst=None, dDepth=-1, workspace=None):
        return dtFilter(self._guide, src, self._ss, self._sr, self._mode, self._iters, dDepth, dst, workspace)


def createDTFilter(guide, sigmaSpatial, sigmaColor, mode=DTF_RF, numIters=3):
    """EF.hpp:100: a DTFilter on `guide` (held by reference, not copied).  The default mode is DTF_RF, not the reference's
    DTF_NC, which is not built."""
    return DTFilter(guide, sigmaSpatial, sigmaColor, mode, numIters)


# ---------------------------------------------------------------------------------------------
# cv::ximgproc::dtFilter / createDTFilter / DTFilter in mode DTF_NC, the reference's default, under names of their own
# (dtFilter above is pinned to refuse DTF_NC), in the library's own exact definition (include/adf_wls.h;
# csrc/dt_window_kernels.hip; the direct statement is tests/dt_window_ref.py).
# ---------------------------------------------------------------------------------------------
_DTW = "dtWindowFilter"


def _dtw_mode(who, mode):
    """DTF_NC; DTF_RF is sent to dtFilter, DTF_IC refused as not built."""
    if isinstance(mode, int) and mode == DTF_RF:
        raise AdfError(_lib.ADF_EBADARG, "%s: DTF_RF is dtFilter's mode; mode must be DTF_NC" % who)
    return _choice(who, mode, accepted=(DTF_NC,), not_built={DTF_IC: "DTF_IC"}, must="mode must be DTF_NC", are="DTF_NC is")


def dtNcRadii(sigmaSpatial, numIters=3):
    """The radii r_1 .. r_N of dtWindowFilter's iterations exactly as its calls form them (adf_dt_nc_radii_host):
    float32, (max(1, numIters),); iteration i averages over the pixels within r_i of each pixel in the transformed domain,
    at most floor(r_i) to either side.  Host only: no device is touched."""
    n = max(1, int(numIters))
    if n > DT_MAX_ITERS:     # (the library refuses it too; the array is sized first)
        raise AdfError(_lib.ADF_EBADARG, "dtNcRadii: numIters must not exceed %d" % DT_MAX_ITERS)
    radii = np.empty(n, np.float32)
    _lib.check(_lib.lib().adf_dt_nc_radii_host(float(sigmaSpatial), int(numIters), radii.ctypes.data))
    return radii


def dtWindowFilterWorkspaceBytes(n, H, W):
    """Bytes of device workspace dtWindowFilter needs for n maps of H x W (adf_dt_window_filter_workspace_bytes): two
    float planes per map, between which the passes carry the map."""
    return int(_lib.lib().adf_dt_window_filter_workspace_bytes(int(n), int(W), int(H)))


def dtWindowFilter(guide, src, sigmaSpatial, sigmaColor, mode=DTF_NC, numIters=3, dDepth=-1, dst=None, workspace=None):
    """cv::ximgproc::dtFilter(guide, src, dst, sigmaSpatial, sigmaColor, mode, numIters) in mode DTF_NC -- the
    reference's default --, in the library's own definition (include/adf_wls.h): numIters times, every pixel becomes the
    mean of the map over a window along its row, then along its column; the window holds the pixels whose distance in the
    transformed domain -- pixel steps plus sigmaSpatial / sigmaColor times the guide's L1 differences walked over -- stays
    within the iteration's radius (dtNcRadii).  Bit-exact against tests/dt_window_ref.py fed with dtNcRadii.

        guide, src, sigmaColor, numIters, dDepth, dst   as dtFilter's
        sigmaSpatial  clamped to >= 1, finite, and small enough for the first radius to stay within 127 pixels
                      (DT_NC_MAX_RADIUS): up to 84 at numIters 3
        mode          DTF_NC.  DTF_RF is dtFilter's; DTF_IC is not built

    Everything else -- invalid values, multi-channel sources, tensors and streams, `workspace` (here at least
    dtWindowFilterWorkspaceBytes(...) bytes), host arrays -- is as with dtFilter.  Returns dst."""
    if guide is None or src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: guide and src must not be empty" % _DTW)
    m = _dtw_mode(_DTW, mode)
    S, G, _, D, dst, dt, ddt = _filter_images(_DTW, src, dst, dDepth, guide)
    args = (S.n, G.ptr, G.stride, G.pair_stride, G.c, S.ptr, S.stride, S.pair_stride, _DEPTH[dt], D.ptr, D.stride, D.pair_stride,
            _DEPTH[ddt], S.w, S.h, float(sigmaSpatial), float(sigmaColor), m, int(numIters))
    _filter_call("adf_dt_window_filter", S, args, _workspace(_DTW, S, workspace))
    return dst


class DTWindowFilter:
    """cv::ximgproc::DTFilter (EF.hpp:66-84) in mode DTF_NC: holds the guide and the parameters; filter(src) is
    dtWindowFilter(guide, src, ...).  There is no init stage -- the distances are summed from the guide in every pass -- so
    the object saves no work: it is the reference's interface, with the reference's default mode."""

    def __init__(self, guide, sigmaSpatial, sigmaColor, mode=DTF_NC, numIters=3):
        if guide is None:
            raise AdfError(_lib.ADF_EBADARG, "%s: guide must not be empty" % _DTW)
        m = _dtw_mode(_DTW, mode)
        if not (math.isfinite(float(sigmaSpatial)) and math.isfinite(float(sigmaColor))):
            raise AdfError(_lib.ADF_EBADARG, "%s: sigmaSpatial and sigmaColor must be finite" % _DTW)
        if int(numIters) > DT_MAX_ITERS:
            raise AdfError(_lib.ADF_EBADARG, "%s: numIters must not exceed %d" % (_DTW, DT_MAX_ITERS))
        if not dtNcRadii(sigmaSpatial, numIters)[0] < DT_NC_MAX_RADIUS + 1:
            raise AdfError(_lib.ADF_EBADARG, "%s: the first iteration's radius exceeds %d pixels" % (_DTW, DT_NC_MAX_RADIUS))
        self._guide, self._ss, self._sr, self._mode, self._iters = guide, float(sigmaSpatial), float(sigmaColor), m, int(numIters)

    def filter(self, src, dst=None, dDepth=-1, workspace=None):
        return dtWindowFilter(self._guide, src, self._ss, self._sr, self._mode, self._iters, dDepth, dst, workspace)


def createDTWindowFilter(guide, sigmaSpatial, sigmaColor, mode=DTF_NC, numIters=3):
    """EF.hpp:100 with the reference's default mode: a DTWindowFilter on `guide` (held by reference, not copied)."""
    return DTWindowFilter(guide, sigmaSpatial, sigmaColor, mode, numIters)


# ---------------------------------------------------------------------------------------------
# cv::ximgproc::jointBilateralFilter (EF.hpp:317, joint_bilateral_filter.cpp) in the library's own exact definition
# (include/adf_wls.h; csrc/joint_bilateral_kernels.hip; the direct statement is tests/jbf_ref.py).
# ---------------------------------------------------------------------------------------------
_JBF = "jointBilateralFilter"
BORDER_DEFAULT = BORDER_REFLECT_101     # cv::BORDER_DEFAULT
_JBF_NOT_BUILT = {BORDER_CONSTANT: "BORDER_CONSTANT", BORDER_WRAP: "BORDER_WRAP"}


_jbf_border = functools.partial(_choice, accepted=(BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101), not_built=_JBF_NOT_BUILT,   # (who, borderType)
                                must="borderType must be BORDER_REPLICATE, BORDER_REFLECT or BORDER_REFLECT_101",
                                are="BORDER_REPLICATE, BORDER_REFLECT and BORDER_REFLECT_101 are", unknown="borderType %d")


def jbfTables(d, sigmaColor, sigmaSpace, channels=1):
    """The tables of jointBilateralFilter exactly as its calls use them (adf_jbf_tables_host): (C, S, r) with C float32 of
    255 * channels + 1 entries indexed by the joint's L1 difference, S float32 of r * r + 1 entries indexed by the squared
    distance, and the radius r the clamps give.  Host only: no device is touched."""
    r = C.c_int(0)
    fn = _lib.lib().adf_jbf_tables_host
    _lib.check(fn(int(d), float(sigmaColor), float(sigmaSpace), int(channels), None, None, C.byref(r)))   # (sizes S)
    colour, space = np.empty(255 * int(channels) + 1, np.float32), np.empty(r.value * r.value + 1, np.float32)
    _lib.check(fn(int(d), float(sigmaColor), float(sigmaSpace), int(channels), colour.ctypes.data, space.ctypes.data, C.byref(r)))
    return colour, space, r.value


def jointBilateralFilter(joint, src, d, sigmaColor, sigmaSpace, borderType=BORDER_REFLECT_101, dDepth=-1, dst=None):
    """cv::ximgproc::jointBilateralFilter(joint, src, dst, d, sigmaColor, sigmaSpace, borderType) in the library's own
    definition (include/adf_wls.h): the mean of the source over the disc of radius r, a tap weighted by
    S[squared distance] * C[L1 difference of the joint's pixels], float32 sums in one stated order -- bit-exact against
    tests/jbf_ref.py fed with jbfTables.

        joint       uint8, (H,W) or (H,W,3); with a batch (N,H,W) or (N,H,W,3); not src itself
        src         uint8, int16 or float32, (H,W) or a batch (N,H,W), one channel
        d           the diameter: r = d // 2; d <= 0: r = round-half-even(1.5 sigmaSpace); r is raised to 1 and must not
                    exceed 31 (JBF_MAX_RADIUS)
        sigmaColor  in grey levels of the 0..255 joint; sigmaSpace in pixels; both finite, <= 0 means 1
        borderType  BORDER_REPLICATE, BORDER_REFLECT or BORDER_REFLECT_101 (cv's default, the default here);
                    BORDER_CONSTANT and BORDER_WRAP are not built
        dDepth      -1 = src's depth, or CV_8U, CV_16S, CV_32F: integer outputs are rounded half to even and saturated
        dst         None, or an array / tensor of that depth and src's shape that overlaps neither input

    The filter is not blind to a matcher's invalid value (minDisparity-1)*16: fill the holes first (weightedMedianFilter
    with ignoreValue).  Float (CV_32F) joints, multi-channel sources and the fall-back to cv::bilateralFilter for an empty
    joint or joint is src are not built.  Torch CUDA tensors run on the device, asynchronously on torch's current stream:
    one launch, no workspace, and once a (sigmaColor, sigmaSpace, r, channels) has been used the call allocates nothing
    and may be captured into a CUDA graph.  Numpy arrays take the host entry point.  Returns dst."""
    if joint is None or src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: joint and src must not be empty (an empty joint is cv::bilateralFilter, which is not built)" % _JBF)
    if joint is src:
        raise AdfError(_lib.ADF_EBADARG, "%s: joint is src is cv::bilateralFilter, which is not built" % _JBF)
    b = _jbf_border(_JBF, borderType)
    S, J, _, D, dst, dt, ddt = _filter_images(_JBF, src, dst, dDepth, joint, "joint", suffix="; multi-channel sources are not built",
                                              float_guide="a float32 (CV_32F) joint is not built; the joint must be uint8")
    args = (S.n, J.ptr, J.stride, J.pair_stride, J.c, S.ptr, S.stride, S.pair_stride, _DEPTH[dt], D.ptr, D.stride, D.pair_stride,
            _DEPTH[ddt], S.w, S.h, int(d), float(sigmaColor), float(sigmaSpace), b)
    _filter_call("adf_joint_bilateral_filter", S, args)
    return dst


# ---------------------------------------------------------------------------------------------
# cv::ximgproc::rollingGuidanceFilter (EF.hpp:350, rolling_guidance_filter.cpp) in the library's own exact definition
# (include/adf_wls.h; csrc/rolling_guidance_kernels.hip; the direct statement is tests/rgf_ref.py).
# ---------------------------------------------------------------------------------------------
_RGF = "rollingGuidanceFilter"


def _rgf_depth(who, depth_or_dtype):
    """The ADF depth code of a depth code (CV_8U, CV_16S, CV_32F) or of a numpy / torch dtype; anything else is refused."""
    if isinstance(depth_or_dtype, int) and depth_or_dtype in _GF_DTYPE:
        return _DEPTH[_GF_DTYPE[depth_or_dtype]]
    for dt in (np.uint8, np.int16, np.float32):
        if torch is not None and isinstance(depth_or_dtype, torch.dtype):
            if depth_or_dtype is _TORCH_DTYPE[dt]:
                return _DEPTH[dt]
            continue
        try:
            if np.dtype(depth_or_dtype) == np.dtype(dt):
                return _DEPTH[dt]
        except TypeError:
            break
    raise AdfError(_lib.ADF_EBADARG, "%s: the depth must be uint8 (CV_8U), int16 (CV_16S) or float32 (CV_32F)" % who)


def rgfTables(depth_or_dtype, d, sigmaColor, sigmaSpace):
    """The tables of rollingGuidanceFilter exactly as its calls use them (adf_rgf_tables_host): (colour, space, r, scale).
    For uint8 / int16 `colour` is C, float32 of T entries indexed by min(|J(p) - J(q)|, T - 1) -- the range table cut after
    its first zero entry, T <= 256 or 65536 -- and scale is 1.0; for float32 it is the constant grid G of 4098 entries that
    |J(p) - J(q)| * scale is interpolated in, scale = float32(256 / sigmaColor).  `space` is S, float32 of r * r + 1
    entries indexed by the squared distance, and r the radius the clamps give.  Host only: no device is touched."""
    depth = _rgf_depth("rgfTables", depth_or_dtype)
    r, n, k = C.c_int(0), C.c_int(0), C.c_float(0)
    fn = _lib.lib().adf_rgf_tables_host
    args = (depth, int(d), float(sigmaColor), float(sigmaSpace))
    _lib.check(fn(*args, None, None, C.byref(r), C.byref(n), C.byref(k)))   # (the sizes)
    colour, space = np.empty(n.value, np.float32), np.empty(r.value * r.value + 1, np.float32)
    _lib.check(fn(*args, colour.ctypes.data, space.ctypes.data, C.byref(r), C.byref(n), C.byref(k)))
    return colour, space, r.value, np.float32(k.value)


def rollingGuidanceWorkspaceBytes(n, H, W, dtype, numOfIter):
    """Bytes of device workspace rollingGuidanceFilter needs for n maps of H x W of `dtype` (or depth code) and numOfIter
    iterations (adf_rolling_guidance_workspace_bytes): one plane of that depth per map, which takes every other
    iteration's result; 0 for numOfIter <= 1."""
    return int(_lib.lib().adf_rolling_guidance_workspace_bytes(int(n), int(W), int(H), _rgf_depth("rollingGuidanceWorkspaceBytes", dtype), int(numOfIter)))


def rollingGuidanceFilter(src, d=-1, sigmaColor=25, sigmaSpace=3, numOfIter=4, borderType=BORDER_DEFAULT, dst=None, workspace=None):
    """cv::ximgproc::rollingGuidanceFilter(src, dst, d, sigmaColor, sigmaSpace, numOfIter, borderType) in the library's own
    definition (include/adf_wls.h): J_0 = src; numOfIter times J_{k+1} = the joint bilateral filter of src with the joint
    J_k, stored in src's depth; dst = the last J.  Structures below the spatial scale vanish in the first iteration, the
    later ones restore the large edges -- with no colour view.  Bit-exact against tests/rgf_ref.py fed with rgfTables.

        src         uint8, int16 or float32, (H,W) or a batch (N,H,W), one channel
        d           the diameter: r = d // 2; d <= 0: r = round-half-even(1.5 sigmaSpace); r is raised to 1 and must not
                    exceed 31 (JBF_MAX_RADIUS)
        sigmaColor  in the map's own units (1/16 pixel for a matcher's int16 map); sigmaSpace in pixels; finite, <= 0 means 1
        numOfIter   0 .. 16 (RGF_MAX_ITERS); 0 copies src
        borderType  BORDER_REPLICATE, BORDER_REFLECT or BORDER_REFLECT_101 (cv's default, the default here)
        dst         None, or an array / tensor of src's dtype and shape that does not overlap it (no in-place call)

    The range weight of uint8 / int16 maps is a host-built table of the integer difference; float32 maps interpolate a
    constant 4096-bin grid laid over 16 sigmaColor (not, as the reference, over the joint's min-max range), and a uniform
    map takes no Gaussian shortcut.  The filter is not blind to a matcher's invalid value: fill the holes first
    (weightedMedianFilter with ignoreValue).  Torch CUDA tensors run on the device, asynchronously on torch's current
    stream; `workspace` (device path only): a CUDA tensor of at least rollingGuidanceWorkspaceBytes(...) bytes -- once a
    (dtype, sigmaColor, sigmaSpace, r) has been used the call then allocates nothing and may be captured into a CUDA
    graph; None = the library's cached scratch.  Numpy arrays take the host entry point.  Returns dst."""
    if src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: src must not be empty" % _RGF)
    b = _jbf_border(_RGF, borderType)
    S, _, _, D, dst, dt, _ = _filter_images(_RGF, src, dst, suffix="; multi-channel sources are not built",
                                            in_place="dst is src: there is no in-place call")
    args = (S.n, S.ptr, S.stride, S.pair_stride, D.ptr, D.stride, D.pair_stride, _DEPTH[dt], S.w, S.h, int(d), float(sigmaColor),
            float(sigmaSpace), int(numOfIter), b)
    _filter_call("adf_rolling_guidance_filter", S, args, _workspace(_RGF, S, workspace))
    return dst


# ---------------------------------------------------------------------------------------------
# cv::ximgproc::amFilter / createAMFilter / AdaptiveManifoldFilter (EF.hpp:203-280, adaptive_manifold_filter_n.cpp) in
# the library's own exact definition (include/adf_wls.h; csrc/am_filter_kernels.hip; the direct statement is
# tests/am_ref.py).
# ---------------------------------------------------------------------------------------------
_AM = "amFilter"


def amPlan(sigma_s, sigma_r, tree_height=-1, W=1, H=1):
    """What amFilter's host side derives from its parameters and the map's size, exactly as its calls form it
    (adf_am_plan_host): a dict with df, height, sh, sw, manifolds (ints), the float32 scalars a_root, a_child, sr2, argW,
    ss, ratio, lnA, argOut, and jtab, the 256 float32 levels of the joint.  Host only: no device is touched."""
    p = _lib.AmPlan()
    jtab = np.empty(256, np.float32)
    _lib.check(_lib.lib().adf_am_plan_host(float(sigma_s), float(sigma_r), int(tree_height), int(W), int(H), C.byref(p), jtab.ctypes.data))
    out = {k: int(getattr(p, k)) for k in ("df", "height", "sh", "sw", "manifolds")}
    out.update({k: np.float32(getattr(p, f)) for k, f in (("a_root", "a_root"), ("a_child", "a_child"), ("sr2", "sr2"), ("argW", "arg_w"),
                                                          ("ss", "ss"), ("ratio", "ratio"), ("lnA", "ln_a"), ("argOut", "arg_out"))})
    out["jtab"] = jtab
    return out


def amFilterWorkspaceBytes(n, H, W, channels, sigma_s, sigma_r, tree_height=-1):
    """Bytes of device workspace amFilter needs for n maps of H x W with a joint of `channels` channels
    (adf_am_filter_workspace_bytes); 0 for arguments the calls refuse."""
    return int(_lib.lib().adf_am_filter_workspace_bytes(int(n), int(W), int(H), int(channels), float(sigma_s), float(sigma_r), int(tree_height)))


def _am_filter(joint, src, sigma_s, sigma_r, tree_height, adjust_outliers, dst, dDepth, workspace):
    if joint is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: joint must not be empty (filtering src by itself is not built)" % _AM)
    if src is None:
        raise AdfError(_lib.ADF_EBADARG, "%s: src must not be empty" % _AM)
    S, G, _, D, dst, dt, ddt = _filter_images(_AM, src, dst, dDepth, joint, role="joint")
    args = (S.n, G.ptr, G.stride, G.pair_stride, G.c, S.ptr, S.stride, S.pair_stride, _DEPTH[dt], D.ptr, D.stride, D.pair_stride,
            _DEPTH[ddt], S.w, S.h, float(sigma_s), float(sigma_r), int(tree_height), int(bool(adjust_outliers)))
    _filter_call("adf_am_filter", S, args, _workspace(_AM, S, workspace))
    return dst


def amFilter(joint, src, sigma_s, sigma_r, adjust_outliers=False, dst=None, dDepth=-1, workspace=None):
    """cv::ximgproc::amFilter(joint, src, dst, sigma_s, sigma_r, adjust_outliers): the adaptive manifold filter, a
    high-dimensional bilateral filter of a map through a gray or BGR view for large kernels, in the library's own
    definition (include/adf_wls.h).  Bit-exact against tests/am_ref.py fed with amPlan.

        joint    (H,W) or (H,W,3) uint8, or a batch (N,H,W[,3]); must not be None
        src      (H,W) or (N,H,W) uint8, int16 or float32, one channel
        sigma_s  >= 1: the spatial scale in pixels; the small plane is 1/df of the map, df = amPlan(...)["df"]
        sigma_r  in (0, 1]: the range scale, the joint taken as 0 .. 1
        adjust_outliers  pull pixels far from every manifold back to src
        dDepth   -1 (src's depth, as the reference), CV_8U, CV_16S or CV_32F
        dst      must not overlap src or joint

    The tree height is automatic (AdaptiveManifoldFilter sets it).  Tensors, streams, `workspace` (at least
    amFilterWorkspaceBytes(...) bytes) and host arrays are as with dtFilter.  Returns dst."""
    return _am_filter(joint, src, sigma_s, sigma_r, -1, adjust_outliers, dst, dDepth, workspace)


class AdaptiveManifoldFilter:
    """cv::ximgproc::AdaptiveManifoldFilter (EF.hpp:203-245): the parameters as properties, filter(src, dst, joint).
    UseRNG is False and cannot be switched on (the reference's random start vector is not built; its default is True);
    PCAIterations is stored, clamped to >= 1, and does not change the result (include/adf_wls.h)."""

    def __init__(self, sigma_s=16.0, sigma_r=0.2, adjust_outliers=False):
        self._sigma_s, self._sigma_r, self._tree_height, self._pca, self._adjust = float(sigma_s), float(sigma_r), -1, 1, bool(adjust_outliers)

    @staticmethod
    def create():
        return AdaptiveManifoldFilter()

    def getSigmaS(self):
        return self._sigma_s

    def setSigmaS(self, val):
        self._sigma_s = float(val)

    def getSigmaR(self):
        return self._sigma_r

    def setSigmaR(self, val):
        self._sigma_r = float(val)

    def getTreeHeight(self):
        return self._tree_height

    def setTreeHeight(self, val):
        self._tree_height = int(val)

    def getPCAIterations(self):
        return self._pca

    def setPCAIterations(self, val):
        self._pca = max(1, int(val))

    def getAdjustOutliers(self):
        return self._adjust

    def setAdjustOutliers(self, val):
        self._adjust = bool(val)

    def getUseRNG(self):
        return False

    def setUseRNG(self, val):
        if val:
            raise AdfError(_lib.ADF_EBADARG, "%s: UseRNG is not built; the start vector is (0.5, -0.5, 0.5)" % _AM)

    def filter(self, src, dst=None, joint=None, dDepth=-1, workspace=None):
        return _am_filter(joint, src, self._sigma_s, self._sigma_r, self._tree_height, self._adjust, dst, dDepth, workspace)

    def collectGarbage(self):
        """Nothing to collect: the object holds no device memory."""


def createAMFilter(sigma_s, sigma_r, adjust_outliers=False):
    """EF.hpp:259: an AdaptiveManifoldFilter with these parameters."""
    return AdaptiveManifoldFilter(sigma_s, sigma_r, adjust_outliers)


def createDisparityWLSFilter(matcher_left):
    """DF.hpp:131, DF.cpp:386-414: set the filter up from the matcher (and mutate the matcher).  A matcher's cost type
    and census size are not among the mutated parameters: createRightMatcher(matcher_left) carries them to the right view."""
    matcher_left.setDisp12MaxDiff(1000000)
    matcher_left.setSpeckleWindowSize(0)
    min_disp = matcher_left.getMinDisparity()
    num_disp = matcher_left.getNumDisparities()
    wsize = matcher_left.getBlockSize()
    wsize2 = wsize // 2
    if isinstance(matcher_left, StereoBM):
        matcher_left.setTextureThreshold(0)
        matcher_left.setUniquenessRatio(0)
        wls = DisparityWLSFilter(True, max(0, min_disp + num_disp) + wsize2, max(0, -min_disp) + wsize2,
                                 wsize2, wsize2, min_disp)
        wls.setDepthDiscontinuityRadius(int(math.ceil(0.33 * wsize)))
    elif isinstance(matcher_left, StereoSGBM):
        matcher_left.setUniquenessRatio(0)
        wls = DisparityWLSFilter(True, max(0, min_disp + num_disp), max(0, -min_disp), 0, 0, min_disp)
        wls.setDepthDiscontinuityRadius(int(math.ceil(0.5 * wsize)))
    else:
        raise AdfError(_lib.ADF_EBADARG, "DisparityWLSFilter natively supports only StereoBM and StereoSGBM")
    return wls


def createRightMatcher(matcher_left):
    """DF.hpp:139, DF.cpp:417-449."""
    min_disp = matcher_left.getMinDisparity()
    num_disp = matcher_left.getNumDisparities()
    wsize = matcher_left.getBlockSize()
    if isinstance(matcher_left, StereoBM):
        right = StereoBM.create(num_disp, wsize)
        right.setMinDisparity(-(min_disp + num_disp) + 1)
        right.setTextureThreshold(0)
        right.setUniquenessRatio(0)
        right.setCostType(matcher_left.getCostType())         # (a different cost on the right view would wreck the LRC confidence)
        right.setCensusSize(matcher_left.getCensusSize())
        right.setDisp12MaxDiff(1000000)
        right.setSpeckleWindowSize(0)
        return right
    if isinstance(matcher_left, StereoSGBM):
        right = StereoSGBM.create(-(min_disp + num_disp) + 1, num_disp, wsize)
        right.setUniquenessRatio(0)
        right.setP1(matcher_left.getP1())
        right.setP2(matcher_left.getP2())
        right.setMode(matcher_left.getMode())
        right.setPreFilterCap(matcher_left.getPreFilterCap())
        right.setCostType(matcher_left.getCostType())         # (a different cost on the right view would wreck the LRC confidence)
        right.setCensusSize(matcher_left.getCensusSize())
        right.setDisp12MaxDiff(1000000)
        right.setSpeckleWindowSize(0)
        return right
    raise AdfError(_lib.ADF_EBADARG, "createRightMatcher supports only StereoBM and StereoSGBM")


def createDisparityWLSFilterGeneric(use_confidence):
    """DF.hpp:149, DF.cpp:452-455."""
    return DisparityWLSFilter(use_confidence)


# ---------------------------------------------------------------------------------------------
# Fast Global Smoother (EF.hpp:361-413)
# ---------------------------------------------------------------------------------------------
_DEPTH = {np.uint8: _lib.DEPTH_8U, np.int16: _lib.DEPTH_16S, np.float32: _lib.DEPTH_32F}
_NUMPY_DTYPE = {**{t: n for n, t in _TORCH_DTYPE.items()}, **{np.dtype(n): n for n in _ITEMSIZE}}


class _Dense:
    """An array the smoother makes dense itself, as _call, _check_device and _stream_of see an image: `device`, `keep`
    and `ptr`, plus `dtype`, the numpy type of its elements (None: none the library takes).  A CUDA tensor stays where it
    is, anything else becomes a numpy array; a strided one is copied.  Rows are then shape[1] * channels elements apart
    whatever stride a one-element axis reports, so the pitch comes from the shape and no stride is read."""

    def __init__(self, a):
        self.device = _is_torch(a) and a.is_cuda
        self.keep = a = a.contiguous() if self.device else np.ascontiguousarray(a)
        self.ptr = a.data_ptr() if self.device else a.ctypes.data
        self.dtype = _NUMPY_DTYPE.get(a.dtype)


class FastGlobalSmootherFilter(_Handle):
    _destroy = "adf_fgs_destroy"

    def __init__(self, guide, lambda_, sigma_color, lambda_attenuation=0.25, num_iter=3, solver=SOLVER_WAVE):
        self._h = C.c_void_p()
        device = _is_torch(guide) and guide.is_cuda
        if guide is None or (guide.numel() if device else getattr(guide, "size", 0)) == 0:
            raise AdfError(_lib.ADF_EBADARG, "guide is empty")  # FGS.cpp:143
        im = _Dense(guide)
        g = im.keep
        if im.dtype is not np.uint8 or len(g.shape) not in (2, 3) or (len(g.shape) == 3 and g.shape[2] not in (1, 3)):
            raise AdfError(_lib.ADF_EBADARG, "guide must be CV_8UC1 or CV_8UC3")  # FGS.cpp:144
        ch = 1 if len(g.shape) == 2 else g.shape[2]
        self._shape = tuple(g.shape[:2])
        args = (C.byref(self._h), im.ptr, g.shape[1] * ch, ch, g.shape[1], g.shape[0], float(lambda_), float(sigma_color),
                float(lambda_attenuation), int(num_iter), int(solver))
        if device:
            # the guide already lives in HBM (a device pipeline, e.g. sparse_match_interpolators.cpp:202-203):
            # adf_fgs_create_device, asynchronous on torch's current stream, nothing crosses PCIe
            with torch.cuda.device(g.device):
                _lib.check(_lib.lib().adf_fgs_create_device(*args, _stream_of(im)))
            self._guide_keep = g       # the copy into the handle is queued on the stream: keep the source alive
        else:
            _lib.check(_lib.lib().adf_fgs_create(*args))

    def getSolver(self):
        """The solver this filter runs: SOLVER_WAVE only if it was asked for and the guide fits it (library extension)."""
        return _read(_lib.lib().adf_fgs_get_solver, C.c_int, self._h)

    def filter(self, src, dst=None):
        """EF.hpp:370, FGS.cpp:182-233.  A torch CUDA tensor is filtered where it is (asynchronously on
        torch's current stream) and a CUDA tensor is returned; anything else takes the host path."""
        S = _Dense(src)
        s, dtype, device = S.keep, S.dtype, S.device
        if dtype not in _DEPTH or len(s.shape) not in (2, 3):
            raise AdfError(_lib.ADF_EBADARG, "src depth must be CV_8U, CV_16S or CV_32F")  # FGS.cpp:184
        cn = 1 if len(s.shape) == 2 else s.shape[2]
        if cn > 4:
            raise AdfError(_lib.ADF_EBADARG, "src must have at most 4 channels")
        if tuple(s.shape[:2]) != self._shape:
            raise AdfError(_lib.ADF_ESIZE,
                           "Size of the filtered image must be equal to the size of the guide image")  # FGS.cpp:187
        if dst is None:
            dst = torch.empty_like(s) if device else np.empty_like(s)
        else:
            # the library writes h rows of w*cn elements at a dense stride: anything else would be overrun
            dense = (_is_torch(dst) and dst.is_cuda and dst.is_contiguous()) if device else \
                    (isinstance(dst, np.ndarray) and dst.flags["C_CONTIGUOUS"])
            if not (dense and dst.shape == s.shape and dst.dtype == s.dtype):
                if device:
                    raise AdfError(_lib.ADF_EBADARG, "dst must be a contiguous CUDA tensor shaped like src")
                raise AdfError(_lib.ADF_ESIZE, "dst must be a C-contiguous ndarray with src's shape and dtype")
        D, rowb = _Dense(dst), s.shape[1] * cn * _ITEMSIZE[dtype]
        if device:
            _check_device(_read(_lib.lib().adf_fgs_get_device, C.c_int, self._h), (S, D), "this FastGlobalSmootherFilter")
        _call("adf_fgs_filter", S, (self._h, S.ptr, rowb, D.ptr, rowb, _DEPTH[dtype], cn))
        return dst


def createFastGlobalSmootherFilter(guide, lambda_, sigma_color, lambda_attenuation=0.25, num_iter=3, solver=SOLVER_WAVE):
    """EF.hpp:393 (`solver` is this library's extension: SOLVER_WAVE or the bit-exact SOLVER_EXACT)."""
    return FastGlobalSmootherFilter(guide, lambda_, sigma_color, lambda_attenuation, num_iter, solver)


def fastGlobalSmootherFilter(guide, src, lambda_, sigma_color, lambda_attenuation=0.25, num_iter=3, dst=None,
                             solver=SOLVER_WAVE):
    """EF.hpp:413, FGS.cpp:687-691."""
    return createFastGlobalSmootherFilter(guide, lambda_, sigma_color, lambda_attenuation, num_iter, solver).filter(src, dst)


def releaseCachedMemory():
    """Returns the device blocks of destroyed filters and the weight tables the library keeps for the next filter
    (include/adf_wls.h: adf_release_cached_memory) to the driver."""
    _lib.lib().adf_release_cached_memory()


# ---------------------------------------------------------------------------------------------
# Evaluation utilities (DF.hpp:163-204, DF.cpp:460-556)
# ---------------------------------------------------------------------------------------------
UNKNOWN_DISPARITY = 16320  # DF.cpp:460


def readGT(src_path):
    """DF.hpp:163 / DF.cpp:462-495: ground-truth disparity (x16) from a Middlebury (8-bit gray: value*16,
    0 -> unknown) or MPI-Sintel (8-bit colour: 64*R + G/4) image.  Returns (status, map); status 0 = ok,
    1 = unsupported image, like the reference.  Decoding uses Pillow (the reference uses cv::imread)."""
    try:
        from PIL import Image

        im = Image.open(src_path)
        im.load()
    except Exception:
        return 1, np.zeros((0, 0), np.int16)
    if im.mode == "RGB":
        a = np.asarray(im, np.int32)                       # PIL is RGB; the reference indexes BGR val[2]=R, val[1]=G
        return 0, (64 * a[:, :, 0] + a[:, :, 1] // 4).astype(np.int16)
    if im.mode == "L":
        a = np.asarray(im, np.int32)
        return 0, np.where(a == 0, UNKNOWN_DISPARITY, 16 * a).astype(np.int16)
    return 1, np.zeros((im.size[1], im.size[0]), np.int16)


def _evaluate(name, GT, src, ROI, *thresh):
    """One of the two error measures: `name`_host / _device(GT, src, size, ROI, [thresh,] &result)."""
    g = _Image(GT, np.int16, "GT", False)
    s = _Image(src, np.int16, "src", False)
    if (g.h, g.w) != (s.h, s.w):
        raise AdfError(_lib.ADF_ESIZE, "GT and src differ in size")   # DF.cpp:501
    if g.device != s.device:
        raise AdfError(_lib.ADF_EBADARG, "GT and src must both be numpy arrays or both be CUDA tensors")
    roi, out = _as_rect(ROI), C.c_double()
    _call(name, g, (g.ptr, g.stride, s.ptr, s.stride, g.w, g.h, C.byref(roi) if roi is not None else None, *[int(t) for t in thresh], C.byref(out)))
    return out.value


def computeMSE(GT, src, ROI=None):
    """DF.hpp:176, DF.cpp:497-517."""
    return _evaluate("adf_compute_mse", GT, src, ROI)


def computeBadPixelPercent(GT, src, ROI=None, thresh=24):
    """DF.hpp:190, DF.cpp:519-539."""
    return _evaluate("adf_compute_bad_pixel_percent", GT, src, ROI, thresh)


def getDisparityVis(src, dst=None, scale=1.0):
    """DF.hpp:202, DF.cpp:541-556."""
    s = _Image(src, np.int16, "src", False)
    if dst is None:
        dst = _empty(s, (s.h, s.w), np.uint8)
    d = _Image(dst, np.uint8, "dst", False)
    if (d.h, d.w) != (s.h, s.w) or d.device != s.device:
        raise AdfError(_lib.ADF_ESIZE, "dst has the wrong size or placement")
    _call("adf_get_disparity_vis", s, (s.ptr, s.stride, d.ptr, d.stride, s.w, s.h, float(scale)))
    return dst
