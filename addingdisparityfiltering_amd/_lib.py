"""ctypes binding of libadf_wls.so (the C-ABI of include/adf_wls.h).

The product path has no CPU fallback: if the HIP library is missing or fails to
load, importing the filter API raises.  Nothing here touches oracle/.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ADF_WLS_LIB selects another build of the same library (A/B timing or output comparison against an older build)
LIB_PATH = os.environ.get("ADF_WLS_LIB") or os.path.join(_HERE, "libadf_wls.so")

ADF_OK, ADF_EBADARG, ADF_ESIZE, ADF_EHIP, ADF_ENOMEM, ADF_ENODEV = range(6)
SOLVER_EXACT, SOLVER_WAVE = 0, 1
PATH_CONF_BAND, PATH_FUSED_FIRST_PASS, PATH_MERGED_PREP, PATH_SCALED_FUSED, PATH_SCALED_HALF = 1, 2, 4, 8, 16    # adf_wls_get_last_path bits (include/adf_wls.h)
PATH_ROW_WEIGHTS_GUIDE = 32    # adf_wls_get_last_solver_path bit
HANDOFF_PAIR_PLANE, HANDOFF_IMAGE, HANDOFF_IMAGE_PAIR_TAIL = 0, 1, 2   # adf_wls_get_last_handoff
DEPTH_8U, DEPTH_16S, DEPTH_32S, DEPTH_32F = 0, 3, 4, 5
SGBM_COST_BT, SGBM_COST_CENSUS_DENSE, SGBM_COST_CENSUS_SPARSE = 0, 1, 2    # adf_sgbm_set_cost (include/adf_wls.h)
BM_COST_SAD, BM_COST_CENSUS_DENSE, BM_COST_CENSUS_SPARSE = 0, 1, 2    # adf_bm_set_cost (the census values equal SGBM_COST_CENSUS_*)
# modified census (window mean) on the dense / the sparse grid, centre-symmetric census; 3 and 7 stay unassigned (include/adf_wls.h)
SGBM_COST_MCT_DENSE, SGBM_COST_MCT_SPARSE, SGBM_COST_CENSUS_CS = 4, 5, 6
BM_COST_MCT_DENSE, BM_COST_MCT_SPARSE, BM_COST_CENSUS_CS = 4, 5, 6
SGBM_RIGHT_MATCHER, SGBM_RIGHT_FROM_VOLUME = 0, 1    # adf_sgbm_compute_both_*'s right_source (include/adf_wls.h)
MISSING_NONE, MISSING_MIN, MISSING_VALUE = 0, 1, 2    # adf_reproject_params.missing_mode (include/adf_wls.h)
WMF_EXP, WMF_IV1, WMF_IV2, WMF_COS, WMF_JAC, WMF_OFF = range(6)    # cv::ximgproc::WMFWeightType; EXP and OFF are built (ADF_WMF_*)
WMF_WEIGHT_ONE, WMF_TABLE_LEVELS, WMF_MAX_RADIUS = 65536, 3 * 256 * 256, 31
GF_MAX_RADIUS = 31    # ADF_GF_MAX_RADIUS
DTF_NC, DTF_IC, DTF_RF, DT_MAX_ITERS = 0, 1, 2, 8    # ADF_DTF_*, ADF_DT_MAX_ITERS
DT_NC_MAX_RADIUS = 127    # ADF_DT_NC_MAX_RADIUS
JBF_MAX_RADIUS = 31    # ADF_JBF_MAX_RADIUS
BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = 1, 2, 3, 4    # cv::BorderTypes; 1, 2 and 4 are built (ADF_BORDER_*)
RGF_MAX_ITERS = 16    # ADF_RGF_MAX_ITERS
AM_MAX_TREE_HEIGHT = 8    # ADF_AM_MAX_TREE_HEIGHT


class AdfError(RuntimeError):
    """Counterpart of cv::Exception raised by CV_Assert / CV_Error on the reference path."""

    def __init__(self, code, msg):
        super().__init__("adf error %d: %s" % (code, msg))
        self.code = code


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int), ("total_ms", C.c_double),
                ("alg_bytes", C.c_double), ("moved_bytes", C.c_double)]


class Rect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class ReprojectParams(C.Structure):
    """adf_reproject_params: Q row-major, disp_scale, missing_mode, missing_value."""
    _fields_ = [("Q", C.c_double * 16), ("disp_scale", C.c_double), ("missing_mode", C.c_int), ("missing_value", C.c_double)]


class RectifyParams(C.Structure):
    """adf_rectify_params: fx, fy, cx, cy, dist (k1 k2 p1 p2 k3 k4 k5 k6), ir = inverse(P[:, :3] * R) row-major."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("dist", C.c_double * 8), ("ir", C.c_double * 9)]


class AmPlan(C.Structure):
    """adf_am_plan: what amFilter's host side derives from (sigma_s, sigma_r, tree_height, W, H)."""
    _fields_ = [(k, C.c_int) for k in ("df", "height", "sh", "sw", "manifolds")] + \
               [(k, C.c_float) for k in ("a_root", "a_child", "sr2", "arg_w", "ss", "ratio", "ln_a", "arg_out")]


# every symbol include/adf_wls.h declares: (name, restype, argtypes)
_vp, _i, _d, _pd, _sz = C.c_void_p, C.c_int, C.c_double, C.c_ssize_t, C.c_size_t
_FILTER_DEV = [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd,
               C.POINTER(Rect), _vp]
_REPROJECT_DEV = [_i, _vp, _i, _pd, _pd, _i, _i, C.POINTER(ReprojectParams), _vp, _pd, _pd, _i, _vp, _sz, _vp]
_POINT_CLOUD_DEV = [_i, _vp, _i, _pd, _pd, _i, _i, C.POINTER(ReprojectParams), C.POINTER(Rect), _d, _d, _vp, _pd, _pd, _i,
                    _vp, _pd, _vp, _pd, _vp, _pd, _i, _vp, _vp, _sz, _vp]
_RECTIFY_MAP_DEV = [C.POINTER(RectifyParams), _i, _i, _vp, _pd, _vp, _pd, _vp]
_REMAP_DEV = [_i, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _vp, _pd, _vp, _pd, _pd, _i, _i, _i, _i, _vp, _vp]
_RECTIFY_VIEWS_DEV = [_i, _vp, _pd, _pd, _i, _i, _i, C.POINTER(RectifyParams), _vp, _pd, _pd, _i, _i, _i, _i, _vp, _vp]
_WMF_DEV = [_i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _i, _i, _d, _i, _vp, _pd, _pd, _i, _d, _vp]
_GF_DEV = [_i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _i, _i, _i, _d, _vp, _sz, _vp]
_DT_DEV = [_i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _i, _i, _d, _d, _i, _i, _vp, _sz, _vp]
_JBF_DEV = [_i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _i, _i, _i, _d, _d, _i, _vp]
_AM_DEV = [_i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _vp, _pd, _pd, _i, _i, _i, _d, _d, _i, _i, _vp, _sz, _vp]
_RGF_DEV = [_i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _i, _d, _d, _i, _i, _vp, _sz, _vp]
_FILTER_SCALED_DEV = [_vp, _i, _vp, _pd, _pd, _i, _i, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd,
                      C.POINTER(Rect), _vp]
# adf_wls_filter_typed_*: the scaled call with a depth behind the left map's strides and one behind the output's
_FILTER_TYPED_DEV = _FILTER_SCALED_DEV[:5] + [_i] + _FILTER_SCALED_DEV[5:16] + [_i] + _FILTER_SCALED_DEV[16:]
SYMBOLS = [
    ("adf_version", _i, []),
    ("adf_last_error", C.c_char_p, []),
    ("adf_device_count", _i, []),
    ("adf_device_pci_bus_id", _i, [_i, C.c_char_p, _i]),
    ("adf_wls_create", _i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i]),
    ("adf_wls_destroy", None, [_vp]),
    ("adf_wls_set_lambda", _i, [_vp, _d]),
    ("adf_wls_get_lambda", _i, [_vp, C.POINTER(_d)]),
    ("adf_wls_set_sigma_color", _i, [_vp, _d]),
    ("adf_wls_get_sigma_color", _i, [_vp, C.POINTER(_d)]),
    ("adf_wls_set_lrc_thresh", _i, [_vp, _i]),
    ("adf_wls_get_lrc_thresh", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_set_depth_discontinuity_radius", _i, [_vp, _i]),
    ("adf_wls_get_depth_discontinuity_radius", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_set_fgs_params", _i, [_vp, _d, _i]),
    ("adf_wls_set_solver", _i, [_vp, _i]),
    ("adf_wls_get_solver", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_get_last_solver", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_get_last_path", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_get_last_solver_path", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_get_last_handoff", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_get_inner_handoffs", _i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    ("adf_wls_filter_device", _i, _FILTER_DEV),
    ("adf_wls_filter_host", _i, _FILTER_DEV[:-1]),
    ("adf_wls_filter_scaled_device", _i, _FILTER_SCALED_DEV),
    ("adf_wls_filter_scaled_host", _i, _FILTER_SCALED_DEV[:-1]),
    ("adf_wls_filter_f32_device", _i, _FILTER_DEV),
    ("adf_wls_filter_f32_host", _i, _FILTER_DEV[:-1]),
    ("adf_wls_filter_scaled_f32_device", _i, _FILTER_SCALED_DEV),
    ("adf_wls_filter_scaled_f32_host", _i, _FILTER_SCALED_DEV[:-1]),
    ("adf_wls_filter_typed_device", _i, _FILTER_TYPED_DEV),
    ("adf_wls_filter_typed_host", _i, _FILTER_TYPED_DEV[:-1]),
    ("adf_wls_get_confidence_device", _i, [_vp, _i, _vp, _pd, _vp]),
    ("adf_wls_get_confidence_host", _i, [_vp, _i, _vp, _pd]),
    ("adf_wls_get_device", _i, [_vp, C.POINTER(_i)]),
    ("adf_wls_get_roi", _i, [_vp, C.POINTER(Rect)]),
    ("adf_wls_sync", _i, [_vp, _vp]),
    ("adf_wls_workspace_bytes", _sz, [_vp]),
    ("adf_wls_profile_enable", _i, [_vp, _i]),
    ("adf_wls_profile_read", _i, [_vp, _vp, _i, C.POINTER(_i)]),
    ("adf_fgs_create", _i, [C.POINTER(_vp), _vp, _pd, _i, _i, _i, _d, _d, _d, _i, _i]),
    ("adf_fgs_create_device", _i, [C.POINTER(_vp), _vp, _pd, _i, _i, _i, _d, _d, _d, _i, _i, _vp]),
    ("adf_fgs_destroy", None, [_vp]),
    ("adf_release_cached_memory", None, []),
    ("adf_weight_table_host", _i, [C.c_float, _vp, _i]),
    ("adf_fgs_get_device", _i, [_vp, C.POINTER(_i)]),
    ("adf_fgs_get_solver", _i, [_vp, C.POINTER(_i)]),
    ("adf_fgs_filter_host", _i, [_vp, _vp, _pd, _vp, _pd, _i, _i]),
    ("adf_fgs_filter_device", _i, [_vp, _vp, _pd, _vp, _pd, _i, _i, _vp]),
    ("adf_compute_mse_host", _i, [_vp, _pd, _vp, _pd, _i, _i, C.POINTER(Rect), C.POINTER(_d)]),
    ("adf_compute_mse_device", _i, [_vp, _pd, _vp, _pd, _i, _i, C.POINTER(Rect), C.POINTER(_d), _vp]),
    ("adf_compute_bad_pixel_percent_host", _i, [_vp, _pd, _vp, _pd, _i, _i, C.POINTER(Rect), _i, C.POINTER(_d)]),
    ("adf_compute_bad_pixel_percent_device", _i, [_vp, _pd, _vp, _pd, _i, _i, C.POINTER(Rect), _i, C.POINTER(_d), _vp]),
    ("adf_get_disparity_vis_host", _i, [_vp, _pd, _vp, _pd, _i, _i, _d]),
    ("adf_get_disparity_vis_device", _i, [_vp, _pd, _vp, _pd, _i, _i, _d, _vp]),
    ("adf_bm_create", _i, [C.POINTER(_vp), _i, _i]),
    ("adf_bm_destroy", None, [_vp]),
    ("adf_bm_set_params", _i, [_vp, _i, _i, _i, _i, _i, _i]),
    ("adf_bm_get_device", _i, [_vp, C.POINTER(_i)]),
    ("adf_bm_get_params", _i, [_vp] + [C.POINTER(_i)] * 6),
    ("adf_bm_set_cost", _i, [_vp, _i, _i]),
    ("adf_bm_get_cost", _i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    ("adf_bm_compute_device", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _vp, _pd, _pd, _vp]),
    ("adf_bm_compute_both_device", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd, _vp]),
    ("adf_bm_compute_host", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _vp, _pd, _pd]),
    ("adf_bm_compute_cost_device", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd, _vp]),
    ("adf_bm_compute_cost_host", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd]),
    ("adf_bm_compute_both_cost_device", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i] + [_vp, _pd, _pd] * 4 + [_vp]),
    ("adf_sgbm_create", _i, [C.POINTER(_vp), _i, _i, _i]),
    ("adf_sgbm_destroy", None, [_vp]),
    ("adf_sgbm_get_device", _i, [_vp, C.POINTER(_i)]),
    ("adf_sgbm_set_params", _i, [_vp] + [_i] * 8),
    ("adf_sgbm_get_params", _i, [_vp] + [C.POINTER(_i)] * 8),
    ("adf_sgbm_set_disp12_max_diff", _i, [_vp, _i]),
    ("adf_sgbm_get_disp12_max_diff", _i, [_vp, C.POINTER(_i)]),
    ("adf_sgbm_set_cost", _i, [_vp, _i, _i]),
    ("adf_sgbm_get_cost", _i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    ("adf_sgbm_compute_device", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _vp]),
    ("adf_sgbm_compute_host", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd]),
    ("adf_sgbm_compute_both_device", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _vp]),
    ("adf_sgbm_compute_both_host", _i, [_vp, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _vp, _pd, _pd, _i]),
    ("adf_census_transform_device", _i, [_i, _vp, _pd, _pd, _i, _i, _i, _i, _vp, _pd, _pd, _vp]),
    ("adf_census_transform_host", _i, [_i, _vp, _pd, _pd, _i, _i, _i, _i, _vp, _pd, _pd]),
    ("adf_filter_speckles_workspace_bytes", _sz, [_i, _i, _i]),
    ("adf_filter_speckles_device", _i, [_i, _vp, _pd, _pd, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    ("adf_filter_speckles_host", _i, [_i, _vp, _pd, _pd, _i, _i, _i, _i, _i]),
    ("adf_validate_disparity_device", _i, [_i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _i, _i, _i, _vp]),
    ("adf_validate_disparity_host", _i, [_i, _vp, _pd, _pd, _vp, _pd, _pd, _i, _i, _i, _i, _i, _i]),
    ("adf_half_size", _i, [_i, C.POINTER(_i)]),
    ("adf_prepare_views_device", _i, [_i, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _i, _i, _i, _vp]),
    ("adf_prepare_views_host", _i, [_i, _vp, _pd, _pd, _i, _i, _i, _vp, _pd, _pd, _i, _i, _i]),
    ("adf_reproject_workspace_bytes", _sz, [_i]),
    ("adf_reproject_to_3d_device", _i, _REPROJECT_DEV),
    ("adf_reproject_to_3d_host", _i, _REPROJECT_DEV[:-3]),
    ("adf_point_cloud_workspace_bytes", _sz, [_i, _i, _i]),
    ("adf_point_cloud_device", _i, _POINT_CLOUD_DEV),
    ("adf_point_cloud_host", _i, _POINT_CLOUD_DEV[:-3]),
    ("adf_rectify_params_init", _i, [_vp, _vp, _i, _vp, _vp, _i, C.POINTER(RectifyParams)]),
    ("adf_init_undistort_rectify_map_device", _i, _RECTIFY_MAP_DEV),
    ("adf_init_undistort_rectify_map_host", _i, _RECTIFY_MAP_DEV[:-1]),
    ("adf_remap_device", _i, _REMAP_DEV),
    ("adf_remap_host", _i, _REMAP_DEV[:-1]),
    ("adf_rectify_views_device", _i, _RECTIFY_VIEWS_DEV),
    ("adf_rectify_views_host", _i, _RECTIFY_VIEWS_DEV[:-1]),
    ("adf_wmf_weight_table_host", _i, [_d, _i, _vp, _i]),
    ("adf_weighted_median_filter_device", _i, _WMF_DEV),
    ("adf_weighted_median_filter_host", _i, _WMF_DEV[:-1]),
    ("adf_guided_filter_workspace_bytes", _sz, [_i, _i, _i, _i]),
    ("adf_guided_filter_device", _i, _GF_DEV),
    ("adf_guided_filter_host", _i, _GF_DEV[:-3]),
    ("adf_dt_filter_workspace_bytes", _sz, [_i, _i, _i]),
    ("adf_dt_rf_table_host", _i, [_d, _d, _i, _i, _vp]),
    ("adf_dt_filter_device", _i, _DT_DEV),
    ("adf_dt_filter_host", _i, _DT_DEV[:-3]),
    ("adf_dt_window_filter_workspace_bytes", _sz, [_i, _i, _i]),
    ("adf_dt_nc_radii_host", _i, [_d, _i, _vp]),
    ("adf_dt_window_filter_device", _i, _DT_DEV),
    ("adf_dt_window_filter_host", _i, _DT_DEV[:-3]),
    ("adf_jbf_tables_host", _i, [_i, _d, _d, _i, _vp, _vp, C.POINTER(_i)]),
    ("adf_joint_bilateral_filter_device", _i, _JBF_DEV),
    ("adf_joint_bilateral_filter_host", _i, _JBF_DEV[:-1]),
    ("adf_rolling_guidance_workspace_bytes", _sz, [_i, _i, _i, _i, _i]),
    ("adf_rgf_tables_host", _i, [_i, _i, _d, _d, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_float)]),
    ("adf_rolling_guidance_filter_device", _i, _RGF_DEV),
    ("adf_rolling_guidance_filter_host", _i, _RGF_DEV[:-3]),
    ("adf_am_plan_host", _i, [_d, _d, _i, _i, _i, C.POINTER(AmPlan), _vp]),
    ("adf_am_exp_host", _i, [_vp, _vp, _sz]),
    ("adf_am_filter_workspace_bytes", _sz, [_i, _i, _i, _i, _d, _d, _i]),
    ("adf_am_filter_device", _i, _AM_DEV),
    ("adf_am_filter_host", _i, _AM_DEV[:-3]),
]

_lib = None


def lib():
    """Load the HIP library; raise loudly if it is not built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            try:
                fn = getattr(L, name)
            except AttributeError:
                if os.environ.get("ADF_WLS_LIB"):     # an A/B build of older sources may lack the newest entry points
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != ADF_OK:
        raise AdfError(rc, lib().adf_last_error().decode("utf-8", "replace"))


def device_pci_bus_id(device):
    """PCI bus id string of HIP device `device` (adf_device_pci_bus_id)."""
    buf = C.create_string_buffer(64)
    check(lib().adf_device_pci_bus_id(int(device), buf, 64))
    return buf.value.decode()
