"""The C-ABI of the rectification (include/adf_wls.h): the seven symbols and their prototypes, adf_rectify_params_init
bit-equal to the NumPy statement's inverse, and every refusal -- through the library and through the Python mirror --
with its code.  Refusals come before any device is touched, so all of this runs on a machine without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rectify_ref as ref
from addingdisparityfiltering_amd import _lib
from addingdisparityfiltering_amd import ximgproc as xi
from addingdisparityfiltering_amd._lib import ADF_EBADARG, ADF_ESIZE, ADF_OK, AdfError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["adf_rectify_params_init", "adf_init_undistort_rectify_map_device", "adf_init_undistort_rectify_map_host",
         "adf_remap_device", "adf_remap_host", "adf_rectify_views_device", "adf_rectify_views_host"]
P_KITTI = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
K_KITTI = np.array([[984.2439, 0.0, 690.0], [0.0, 980.8141, 233.1966], [0.0, 0.0, 1.0]])
DIST = [-0.3728755, 0.2037299, 0.002219027, 0.001383707, -0.07233722]


def _header():
    return open(os.path.join(ROOT, "include", "adf_wls.h")).read()


def _init(K, dist, R, P, p_cols=None, n_dist=None):
    prm = _lib.RectifyParams()
    K = np.ascontiguousarray(K, np.float64)
    P = np.ascontiguousarray(P, np.float64)
    d = np.ascontiguousarray([] if dist is None else dist, np.float64)
    Rm = None if R is None else np.ascontiguousarray(R, np.float64)
    rc = _lib.lib().adf_rectify_params_init(K.ctypes.data, d.ctypes.data if d.size else None, d.size if n_dist is None else n_dist,
                                            None if Rm is None else Rm.ctypes.data, P.ctypes.data,
                                            P.shape[1] if p_cols is None else p_cols, C.byref(prm))
    return rc, prm


def test_symbols_are_exported_and_bound_with_the_headers_prototypes():
    L = C.CDLL(_lib.LIB_PATH)
    bound = {s[0]: s for s in _lib.SYMBOLS}
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    scalar = {"int": C.c_int, "double": C.c_double, "ptrdiff_t": C.c_ssize_t, "size_t": C.c_size_t}
    for name in NAMES:
        assert hasattr(L, name), name
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, code).groups()
        _, restype, argtypes = bound[name]
        assert restype is scalar[ret]
        params = [p.strip() for p in params.split(",")]
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            if "*" in p or "[" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p)
                if "adf_rectify_params" in p:
                    assert t is C.POINTER(_lib.RectifyParams)
            else:
                assert t is scalar[p.split()[0]], (name, p)
    S = _lib.RectifyParams
    assert (S.fx.offset, S.fy.offset, S.cx.offset, S.cy.offset, S.dist.offset, S.ir.offset, C.sizeof(S)) == (0, 8, 16, 24, 32, 96, 168)
    assert re.search(r"typedef struct adf_rectify_params \{ double fx, fy, cx, cy; double dist\[8\]; double ir\[9\]; \}", code)
    assert re.search(r"#define ADF_INTER_LINEAR 1\b", code) and re.search(r"#define ADF_BORDER_CONSTANT 0\b", code)
    assert (xi.INTER_LINEAR, xi.BORDER_CONSTANT, xi.CV_32FC1) == (1, 0, 5)


def test_header_states_the_contract():
    text = _header()
    for words in ("rectification (cv::initUndistortRectifyMap, cv::remap)", "UNPINNED", "no fused multiply-add",
                  "X = (ir0*u + ir1*v) + ir2", "kr = (1.0 + ((k3*r2 + k2)*r2 + k1)*r2) / (1.0 + ((k6*r2 + k5)*r2 + k4)*r2)",
                  "cv accumulates ir0, ir3, ir6 along u", "cv's SIMD builds fuse", "convertMaps", "sx = (int)rintf(tx) (half to even)",
                  "+ 512) >> 10", "c00 = a11*a22 - a12*a21", "det = (a00*c00 + a01*c01) + a02*c02", "one division per entry",
                  "srcW, srcH <= 32767", "W*H < 2^31", "A tap outside the source", "is never loaded"):
        assert words in text, words


@pytest.mark.parametrize("R", [None, "rot"])
@pytest.mark.parametrize("P", [P_KITTI, P_KITTI[:, :3], K_KITTI])
@pytest.mark.parametrize("dist", [None, DIST[:4], DIST, DIST + [0.01, -0.03, 0.002]])
def test_params_init_equals_the_statement_bit_for_bit(R, P, dist):
    a = np.deg2rad(2.0)
    Rm = None if R is None else ref.rot(a, -a, a)
    rc, prm = _init(K_KITTI, dist, Rm, P)
    assert rc == ADF_OK
    (fx, fy, cx, cy), d, ir = ref.params(K_KITTI, dist, Rm, P)
    assert (prm.fx, prm.fy, prm.cx, prm.cy) == (fx, fy, cx, cy)
    assert np.array_equal(np.array(prm.dist[:]).view(np.uint64), d.view(np.uint64))
    assert np.array_equal(np.array(prm.ir[:]).view(np.uint64), ir.view(np.uint64))
    mirror = xi.rectifyParams(K_KITTI, dist, Rm, P)                  # the Python layer takes the same inverse
    assert bytes(mirror) == bytes(prm)


def test_params_init_ignores_the_skew_and_the_fourth_column():
    K = K_KITTI.copy()
    K[0, 1] = 3.5
    P2 = P_KITTI.copy()
    P2[:, 3] = [1e6, -1e6, 7.0]
    rc, a = _init(K, DIST, None, P2)
    rc2, b = _init(K_KITTI, DIST, None, P_KITTI)
    assert rc == ADF_OK and rc2 == ADF_OK and bytes(a) == bytes(b)


def test_params_init_refusals():
    lib = _lib.lib()
    for n in (12, 14, 1, 3, 6, -1):
        rc, _ = _init(K_KITTI, [0.0] * 14, None, P_KITTI, n_dist=n)
        assert rc == ADF_EBADARG, n
        assert b"n_dist" in lib.adf_last_error()
    rc, _ = _init(K_KITTI, None, None, np.ones((3, 3)))
    assert rc == ADF_EBADARG and b"singular" in lib.adf_last_error()
    rc, _ = _init(K_KITTI, None, np.zeros((3, 3)), P_KITTI)
    assert rc == ADF_EBADARG
    rc, _ = _init(K_KITTI, None, None, np.full((3, 3), np.inf))
    assert rc == ADF_EBADARG
    for cols in (5, 2, 0):
        rc, _ = _init(K_KITTI, None, None, P_KITTI, p_cols=cols)
        assert rc == ADF_EBADARG and b"p_cols" in lib.adf_last_error()
    prm = _lib.RectifyParams()
    assert lib.adf_rectify_params_init(None, None, 0, None, None, 3, C.byref(prm)) == ADF_EBADARG
    rc = lib.adf_rectify_params_init(K_KITTI.ctypes.data, None, 5, None, K_KITTI.ctypes.data, 3, C.byref(prm))
    assert rc == ADF_EBADARG                                         # coefficients announced, none given


def _ptr(a):
    return a.ctypes.data


def test_map_and_sampling_refusals_need_no_device():
    lib = _lib.lib()
    _, prm = _init(K_KITTI, DIST, None, P_KITTI)
    mx, my = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32)
    src, dst = np.zeros((6, 10, 3), np.uint8), np.zeros((4, 8, 3), np.uint8)
    m = lib.adf_init_undistort_rectify_map_host
    assert m(None, 8, 4, _ptr(mx), 32, _ptr(my), 32) == ADF_EBADARG
    assert m(C.byref(prm), 0, 4, _ptr(mx), 32, _ptr(my), 32) == ADF_EBADARG
    assert m(C.byref(prm), 8, 4, None, 32, _ptr(my), 32) == ADF_EBADARG
    assert m(C.byref(prm), 8, 4, _ptr(mx), 30, _ptr(my), 32) == ADF_EBADARG          # stride not a multiple of 4
    assert m(C.byref(prm), 8, 4, _ptr(mx), 28, _ptr(my), 32) == ADF_ESIZE
    assert m(C.byref(prm), 1 << 16, 1 << 15, _ptr(mx), 1 << 18, _ptr(my), 1 << 18) == ADF_ESIZE

    def remap(n=1, s=_ptr(src), ss=30, si=180, sw=10, sh=6, ch=3, x=_ptr(mx), xs=32, y=_ptr(my), ys=32, d=_ptr(dst), ds=24, di=96,
              w=8, h=4, interp=1, border=0):
        return lib.adf_remap_host(n, s, ss, si, sw, sh, ch, x, xs, y, ys, d, ds, di, w, h, interp, border, None)

    def views(n=1, s=_ptr(src), ss=30, si=180, sw=10, sh=6, ch=3, p=C.byref(prm), d=_ptr(dst), ds=24, di=96, w=8, h=4, interp=1, border=0):
        return lib.adf_rectify_views_host(n, s, ss, si, sw, sh, ch, p, d, ds, di, w, h, interp, border, None)

    for call in (remap, views):
        assert call(n=0) == ADF_EBADARG
        assert call(s=None) == ADF_EBADARG and call(d=None) == ADF_EBADARG
        assert call(sw=0) == ADF_EBADARG and call(h=0) == ADF_EBADARG
        assert call(ch=2) == ADF_EBADARG and call(ch=4) == ADF_EBADARG
        assert call(interp=0) == ADF_EBADARG and call(interp=2) == ADF_EBADARG       # INTER_NEAREST, INTER_CUBIC
        assert call(border=1) == ADF_EBADARG and call(border=4) == ADF_EBADARG       # BORDER_REPLICATE, BORDER_REFLECT_101
        assert call(sw=32768, ss=3 * 32768) == ADF_ESIZE and call(sh=32768) == ADF_ESIZE
        assert call(w=1 << 16, h=1 << 15, ds=3 << 16) == ADF_ESIZE
        assert call(ss=29) == ADF_ESIZE and call(ds=23) == ADF_ESIZE
        assert call(n=2, di=95) == ADF_EBADARG                                       # destination images overlap
        assert call(n=2, si=-180) == ADF_EBADARG
    assert remap(x=None) == ADF_EBADARG and remap(y=None) == ADF_EBADARG
    assert remap(xs=30) == ADF_EBADARG and remap(ys=28) == ADF_ESIZE
    assert views(p=None) == ADF_EBADARG


def test_mirror_refusals():
    K, src = K_KITTI, np.zeros((6, 10, 3), np.uint8)
    maps = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32)

    def code(fn):
        with pytest.raises(AdfError) as e:
            fn()
        return e.value.code

    assert code(lambda: xi.initUndistortRectifyMap(K, None, None, K, (8, 4), m1type=11)) == ADF_EBADARG      # CV_16SC2
    assert code(lambda: xi.initUndistortRectifyMap(K, [0.0] * 12, None, K, (8, 4))) == ADF_EBADARG
    assert code(lambda: xi.initUndistortRectifyMap(K[:2], None, None, K, (8, 4))) == ADF_EBADARG
    assert code(lambda: xi.initUndistortRectifyMap(K, None, np.eye(4), K, (8, 4))) == ADF_EBADARG
    assert code(lambda: xi.initUndistortRectifyMap(K, None, None, np.ones((3, 3)), (8, 4))) == ADF_EBADARG
    assert code(lambda: xi.initUndistortRectifyMap(K, None, None, K, (0, 4))) == ADF_EBADARG
    assert code(lambda: xi.initUndistortRectifyMap(K, None, None, K, 8)) == ADF_EBADARG
    assert code(lambda: xi.remap(src, *maps, interpolation=0)) == ADF_EBADARG
    assert code(lambda: xi.remap(src, *maps, borderMode=1)) == ADF_EBADARG
    assert code(lambda: xi.remap(src, maps[0], maps[1][:3])) == ADF_EBADARG
    assert code(lambda: xi.remap(src, maps[0].astype(np.float64), maps[1].astype(np.float64))) == ADF_EBADARG
    assert code(lambda: xi.remap(src, *maps, borderValue=256)) == ADF_EBADARG
    assert code(lambda: xi.remap(src, *maps, borderValue=(1, 2))) == ADF_EBADARG
    assert code(lambda: xi.remap(src, *maps, dst=np.zeros((4, 8), np.uint8))) == ADF_ESIZE
    assert code(lambda: xi.remap(np.zeros((2, 6, 10, 2), np.uint8), *maps)) == ADF_EBADARG
    assert code(lambda: xi.rectifyViews(src, K, None, None, K, size=(0, 0))) == ADF_EBADARG
    assert code(lambda: xi.rectifyViews(src, K, [0.0] * 14, None, K)) == ADF_EBADARG
    assert code(lambda: xi.rectifyViews(src.astype(np.int16), K, None, None, K)) == ADF_EBADARG
