"""ctypes binding of librover_fe.so (include/rover_fe.h).  The HIP library is the product's only
compute path: importing this module raises ImportError when the library has not been built, and
`Context()` raises RuntimeError when no gfx950 device can be opened -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RFE_LIBRARY selects another build of the same ABI (tools/ use the -DRFE_TUNING build for A/B measurements)
LIB_PATH = os.environ.get("RFE_LIBRARY") or os.path.join(_HERE, "librover_fe.so")

KIND_SUPERPOINT, KIND_LIGHTGLUE = 1, 2
OPT_LG_FOLD_WO = 1
OPT_LG_FP16X2 = 2    # LightGlue Linears + attention as split products on the f16 matrix pipe (default off)
OPT_HOST_GRAPH = 3   # host entries replay a captured hipGraph per repeated call shape (default off; helps fixed-capacity callers only)

EXPORTS = [
    "rfe_init", "rfe_destroy", "rfe_last_error", "rfe_version", "rfe_load_weights", "rfe_load_onnx", "rfe_set_weights",
    "rfe_weight_count", "rfe_weights_id", "rfe_get_hparams", "rfe_set_hparams", "rfe_set_option", "rfe_get_option", "rfe_set_stream", "rfe_synchronize", "rfe_malloc", "rfe_free", "rfe_host_malloc", "rfe_host_free", "rfe_workspace_bytes", "rfe_memcpy_h2d",
    "rfe_memcpy_d2h", "rfe_extract_u8", "rfe_extract_u8_dev", "rfe_extract_f32", "rfe_extract_f32_dev", "rfe_extract_u8_bin", "rfe_extract_u8_bin_dev",
    "rfe_pyramid_geometry", "rfe_extract_pyramid_u8", "rfe_extract_pyramid_u8_dev", "rfe_match", "rfe_match_dev", "rfe_match_fused",
    "rfe_extract_match_stream_dev", "rfe_stereo_match", "rfe_stereo_match_dev", "rfe_stereo_frame_dev", "rfe_stereo_match_pyramid", "rfe_stereo_match_pyramid_dev", "rfe_stereo_frame_pyramid_dev",
    "rfe_l2_distance_matrix", "rfe_binarize_descriptors",
    "rfe_search_candidates", "rfe_distinctive_descriptors",
    "rfe_l2_distance_matrix_dev", "rfe_binarize_descriptors_dev", "rfe_search_candidates_dev", "rfe_distinctive_descriptors_dev",
    "rfe_search_by_projection", "rfe_search_by_projection_dev", "rfe_search_by_projection_sim3", "rfe_search_by_projection_sim3_dev",
    "rfe_search_local_points", "rfe_search_local_points_dev", "rfe_triangulate_neighbours", "rfe_triangulate_neighbours_dev",
    "rfe_pose_optimization", "rfe_pose_optimization_dev", "rfe_pose_inertial_optimization", "rfe_pose_inertial_optimization_dev", "rfe_sim3_ransac", "rfe_sim3_ransac_dev", "rfe_sim3_ransac_iterations", "rfe_optimize_sim3", "rfe_optimize_sim3_dev", "rfe_local_ba", "rfe_local_ba_dev", "rfe_essential_graph", "rfe_essential_graph_dev", "rfe_global_ba", "rfe_global_ba_dev",
    "rfe_two_view", "rfe_two_view_dev", "rfe_k_two_view_check", "rfe_k_two_view_check_rt", "rfe_k_pose_inertial_classify",
    "rfe_bow_vocab_create", "rfe_bow_vocab_load", "rfe_bow_vocab_destroy", "rfe_bow_vocab_info", "rfe_bow_transform", "rfe_bow_transform_dev",
    "rfe_bow_db_create", "rfe_bow_db_destroy", "rfe_bow_db_add", "rfe_bow_db_add_dev", "rfe_bow_db_erase", "rfe_bow_db_clear", "rfe_bow_db_size",
    "rfe_bow_db_query", "rfe_bow_db_query_dev",
    "rfe_pool_create", "rfe_pool_destroy", "rfe_pool_last_error", "rfe_pool_size", "rfe_pool_ctx", "rfe_pool_has_rccl", "rfe_pool_set_weights",
    "rfe_pool_load_weights", "rfe_pool_set_option", "rfe_pool_set_hparams", "rfe_pool_shard", "rfe_pool_extract_match_stream",
    "rfe_profile_enable", "rfe_profile_filter", "rfe_profile_reset", "rfe_profile_read",
    "rfe_k_conv3x3", "rfe_k_linear", "rfe_k_scoremap", "rfe_k_sparse_desc", "rfe_k_select", "rfe_k_select_keys", "rfe_k_lightglue_taps", "rfe_k_set_lightglue_tap", "rfe_k_global_ba_stop_after", "rfe_k_lightglue_ffn", "rfe_k_attention", "rfe_k_cross_attention", "rfe_k_lightglue_self_attention", "rfe_k_lightglue_assign", "rfe_k_pool_inject_gather_failure", "rfe_k_onnx_convert", "rfe_k_bow_vocab_read",
]

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(rover-slam_amd/csrc/Makefile). There is no CPU fallback.")

lib = C.CDLL(LIB_PATH)

_vp, _fp, _ip, _u8p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p  # raw addresses (host or device)
lib.rfe_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
lib.rfe_destroy.argtypes = [C.c_void_p]
lib.rfe_destroy.restype = None
lib.rfe_last_error.argtypes = [C.c_void_p]
lib.rfe_last_error.restype = C.c_char_p
lib.rfe_version.restype = C.c_char_p
lib.rfe_load_weights.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
lib.rfe_set_weights.argtypes = [C.c_void_p, C.c_int, _fp, C.c_int64]
lib.rfe_weight_count.argtypes = [C.c_int]
lib.rfe_weight_count.restype = C.c_int64
lib.rfe_weights_id.restype = C.c_uint64
lib.rfe_weights_id.argtypes = [C.c_void_p, C.c_int]


class HParams(C.Structure):
    """include/rover_fe.h: rfe_hparams -- the constants baked into the reference's two .onnx graphs (RFEW v2 header)."""
    _fields_ = [("sp_max_keypoints", C.c_int32), ("sp_detection_threshold", C.c_float), ("sp_nms_radius", C.c_int32),
                ("sp_remove_borders", C.c_int32), ("sp_topk_always", C.c_int32), ("lg_layers", C.c_int32), ("lg_heads", C.c_int32), ("lg_filter_threshold", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


lib.rfe_get_hparams.argtypes = [C.c_void_p, C.POINTER(HParams)]
lib.rfe_set_hparams.argtypes = [C.c_void_p, C.POINTER(HParams)]
lib.rfe_pool_set_hparams.argtypes = [C.c_void_p, C.POINTER(HParams)]
lib.rfe_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
lib.rfe_get_option.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
lib.rfe_set_stream.argtypes = [C.c_void_p, C.c_void_p]
lib.rfe_synchronize.argtypes = [C.c_void_p]
lib.rfe_malloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
lib.rfe_free.argtypes = [C.c_void_p, C.c_void_p]
lib.rfe_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
lib.rfe_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
_ext = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _ip, _ip, _fp, _fp]
lib.rfe_extract_u8.argtypes = _ext
lib.rfe_extract_f32.argtypes = _ext
lib.rfe_extract_f32_dev.argtypes = _ext
lib.rfe_extract_u8_dev.argtypes = _ext
lib.rfe_extract_u8_bin.argtypes = _ext + [_u8p]
lib.rfe_extract_u8_bin_dev.argtypes = _ext + [_u8p]
lib.rfe_pyramid_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, _ip, _ip, _fp]
_pyr = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _ip, C.c_float, _ip, _ip, _fp, _ip, _fp, _fp, _u8p]
lib.rfe_extract_pyramid_u8.argtypes = _pyr
lib.rfe_extract_pyramid_u8_dev.argtypes = _pyr
_mt = [C.c_void_p, _fp, _fp, _fp, _fp, _ip, _ip, C.c_int, C.c_int, C.c_int, C.c_float, _ip, _ip, _fp]
lib.rfe_match.argtypes = _mt
lib.rfe_match_dev.argtypes = _mt
lib.rfe_match_fused.argtypes = [C.c_void_p, _fp, C.c_int, _fp, C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_float,
                                C.c_float, _ip]
lib.rfe_extract_match_stream_dev.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_float, _ip, _ip, _fp, _fp, _ip, _ip, _fp]
_st = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp, C.c_float, C.c_float, _fp, _fp]
lib.rfe_stereo_match.argtypes = _st
lib.rfe_stereo_match_dev.argtypes = _st
lib.rfe_stereo_frame_dev.argtypes = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_int, _ip, _ip, _fp, _fp, _fp, _fp, _ip, _ip, _fp]
_stp = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_float, _fp, _ip, C.c_int, _fp, _ip, C.c_int, _fp, _fp, C.c_float, C.c_float,
        C.c_int, _fp, _fp]
lib.rfe_stereo_match_pyramid.argtypes = _stp
lib.rfe_stereo_match_pyramid_dev.argtypes = _stp
lib.rfe_stereo_frame_pyramid_dev.argtypes = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _ip, C.c_float, C.c_float,
                                             C.c_float, C.c_float, C.c_int, C.c_int, _ip, _ip, _fp, _ip, _fp, _fp, _fp, _fp, _ip, _ip, _fp]
lib.rfe_l2_distance_matrix.argtypes = [C.c_void_p, _fp, C.c_int, _fp, C.c_int, _fp]
lib.rfe_binarize_descriptors.argtypes = [C.c_void_p, _fp, C.c_int, _u8p]
lib.rfe_search_candidates.argtypes = [C.c_void_p, _fp, C.c_int, _fp, C.c_int, _ip, _ip, _u8p, _ip, _fp, _fp]
lib.rfe_distinctive_descriptors.argtypes = [C.c_void_p, _fp, _ip, C.c_int, _ip, _fp]
lib.rfe_l2_distance_matrix_dev.argtypes = [C.c_void_p, _fp, C.c_int, _fp, C.c_int, _fp]
lib.rfe_binarize_descriptors_dev.argtypes = [C.c_void_p, _fp, C.c_int, _u8p]
lib.rfe_search_candidates_dev.argtypes = [C.c_void_p, _fp, C.c_int, _fp, C.c_int, _ip, _ip, _u8p, _ip, _fp, _fp]
lib.rfe_distinctive_descriptors_dev.argtypes = [C.c_void_p, _fp, _ip, C.c_int, C.c_int, C.c_int, _ip, _fp]
_psq = [C.c_void_p, _fp, _fp, _fp, _ip, _u8p, C.c_int, _fp, _fp, _ip, _ip, _u8p, C.c_int]
_psb = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]
lib.rfe_search_by_projection.argtypes = _psq + _psb + [_ip, _ip, _fp, _fp, _ip]
lib.rfe_search_by_projection_dev.argtypes = _psq + [_ip] + _psb + [C.c_int, _ip, _ip, _fp, _fp, _ip]


MAX_LEVELS = 16                                                   # RFE_MAX_LEVELS
PROJ_INVZ, PROJ_DIV = 0, 1                                        # RFE_PROJ_*
DIST_FLOAT, DIST_TRUNC = 0, 1                                     # RFE_DIST_*


class Sim3Params(C.Structure):
    """include/rover_fe.h: rfe_sim3_params -- pose, intrinsics, bounds and scale pyramid of one Sim3 SearchByProjection call."""
    _fields_ = [("quat", C.c_float * 4), ("t", C.c_float * 3), ("ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float), ("th", C.c_int32),
                ("nlevels", C.c_int32), ("log_scale_factor", C.c_float), ("scale_factors", C.c_float * MAX_LEVELS),
                ("proj_mode", C.c_int32), ("dist_mode", C.c_int32)]


def sim3_params(quat, t, ow, intrinsics, bounds, th, scale_factors=(1.0,), log_scale_factor=0.0, proj_mode=PROJ_INVZ, dist_mode=DIST_FLOAT,
                nlevels=None):
    """rfe_sim3_params from plain values: quat (x, y, z, w), intrinsics (fx, fy, cx, cy), bounds (min_x, min_y, max_x, max_y)"""
    p = Sim3Params()
    p.quat[:] = [float(v) for v in quat]; p.t[:] = [float(v) for v in t]; p.ow[:] = [float(v) for v in ow]
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in intrinsics)
    p.min_x, p.min_y, p.max_x, p.max_y = (float(v) for v in bounds)
    p.th, p.nlevels, p.log_scale_factor = int(th), len(scale_factors) if nlevels is None else int(nlevels), float(log_scale_factor)
    for l, v in enumerate(list(scale_factors)[:MAX_LEVELS]):
        p.scale_factors[l] = float(v)
    p.proj_mode, p.dist_mode = int(proj_mode), int(dist_mode)
    return p


_s3q = [C.c_void_p, C.POINTER(Sim3Params), _fp, _fp, _fp, _fp, _fp, _fp, _u8p, C.c_int, _fp, _fp, _ip, _u8p, C.c_int]
_s3o = [_ip, _ip, _fp, _fp, _fp, _fp, _ip, _ip, _ip]
lib.rfe_search_by_projection_sim3.argtypes = _s3q + [C.c_float] + _s3o
lib.rfe_search_by_projection_sim3_dev.argtypes = _s3q + [_ip, C.c_float, C.c_int] + _s3o

LEVEL_ZERO, LEVEL_PREDICTED = 0, 1                                # RFE_LEVEL_*


class FrustumParams(C.Structure):
    """include/rover_fe.h: rfe_frustum_params -- pose, intrinsics, bounds, gates and scale pyramid of one SearchLocalPoints call."""
    _fields_ = [("rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("mbf", C.c_float), ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("view_cos_limit", C.c_float), ("th", C.c_float), ("far_points", C.c_int32), ("th_far", C.c_float), ("nlevels", C.c_int32),
                ("log_scale_factor", C.c_float), ("scale_factors", C.c_float * MAX_LEVELS), ("level_mode", C.c_int32)]


def frustum_params(rcw, tcw, ow, intrinsics, mbf, bounds, th, far_points=False, th_far=0.0, scale_factors=(1.0,), log_scale_factor=0.0,
                   level_mode=LEVEL_ZERO, view_cos_limit=0.5, nlevels=None):
    """rfe_frustum_params from plain values: rcw [3,3] row-major, intrinsics (fx, fy, cx, cy), bounds (min_x, min_y, max_x, max_y)"""
    p = FrustumParams()
    p.rcw[:] = [float(v) for v in np.asarray(rcw, np.float32).reshape(-1)]
    p.tcw[:] = [float(v) for v in tcw]; p.ow[:] = [float(v) for v in ow]
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in intrinsics)
    p.mbf = float(mbf)
    p.min_x, p.min_y, p.max_x, p.max_y = (float(v) for v in bounds)
    p.view_cos_limit, p.th, p.far_points, p.th_far = float(view_cos_limit), float(th), int(bool(far_points)), float(th_far)
    p.nlevels, p.log_scale_factor = len(scale_factors) if nlevels is None else int(nlevels), float(log_scale_factor)
    for l, v in enumerate(list(scale_factors)[:MAX_LEVELS]):
        p.scale_factors[l] = float(v)
    p.level_mode = int(level_mode)
    return p


_lpq = [C.c_void_p, C.POINTER(FrustumParams), _fp, _fp, _fp, _fp, _fp, _fp, _u8p, _u8p, C.c_int, _fp, _fp, _ip, _ip, _u8p, C.c_int]
_lpo = [_ip, _ip, _fp, _fp, _fp, _fp, _fp, _fp, _ip, _ip, _ip]
lib.rfe_search_local_points.argtypes = _lpq + [C.c_float] + _lpo
lib.rfe_search_local_points_dev.argtypes = _lpq + [_ip, C.c_float, C.c_int] + _lpo
class TriParams(C.Structure):
    """include/rover_fe.h: rfe_tri_params -- the switches, gates and scale pyramid of one CreateNewMapPoints call."""
    _fields_ = [("inertial", C.c_int32), ("far_points", C.c_int32), ("th_far", C.c_float), ("ratio_factor", C.c_float), ("nlevels", C.c_int32),
                ("scale_factors", C.c_float * MAX_LEVELS), ("level_sigma2", C.c_float * MAX_LEVELS)]


class TriView(C.Structure):
    """include/rover_fe.h: rfe_tri_view -- pose, camera centre, intrinsics and stereo baseline of one keyframe."""
    _fields_ = [("rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float)]


def tri_params(inertial, far_points, th_far, ratio_factor, scale_factors, level_sigma2, nlevels=None):
    """rfe_tri_params from plain values (ratio_factor = 1.5f * mfScaleFactor)"""
    p = TriParams()
    p.inertial, p.far_points, p.th_far, p.ratio_factor = int(bool(inertial)), int(bool(far_points)), float(th_far), float(ratio_factor)
    p.nlevels = len(scale_factors) if nlevels is None else int(nlevels)
    for l, v in enumerate(list(scale_factors)[:MAX_LEVELS]):
        p.scale_factors[l] = float(v)
    for l, v in enumerate(list(level_sigma2)[:MAX_LEVELS]):
        p.level_sigma2[l] = float(v)
    return p


def tri_view(rcw, tcw, ow, fx, fy, cx, cy, invfx, invfy, mb, mbf):
    """rfe_tri_view from plain values: rcw [3,3] row-major"""
    v = TriView()
    v.rcw[:] = [float(x) for x in np.asarray(rcw, np.float32).reshape(-1)]
    v.tcw[:] = [float(x) for x in tcw]; v.ow[:] = [float(x) for x in ow]
    v.fx, v.fy, v.cx, v.cy, v.invfx, v.invfy, v.mb, v.mbf = (float(x) for x in (fx, fy, cx, cy, invfx, invfy, mb, mbf))
    return v


TRI_OUTPUTS = ("code", "x3d", "point_stereo", "out_n", "out_idx1", "out_idx2", "out_x3d", "out_stereo", "matches")
_tri = [C.c_void_p, C.POINTER(TriParams), C.POINTER(TriView), _fp, _fp, _ip, _fp, _fp, _u8p, C.c_int, C.c_void_p, _fp, _fp, _ip, _fp, _fp, _u8p, _ip,
        _u8p, C.c_int, C.c_int, _ip, _ip, C.c_int, _ip, _fp, _u8p, _ip, _ip, _ip, _fp, _u8p, _ip, _ip]
lib.rfe_triangulate_neighbours.argtypes = _tri
lib.rfe_triangulate_neighbours_dev.argtypes = _tri


class PoseParams(C.Structure):
    """include/rover_fe.h: rfe_pose_params -- intrinsics, mbf, mvInvLevelSigma2 and the LM schedule of one PoseOptimization call."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("nlevels", C.c_int32),
                ("inv_level_sigma2", C.c_float * MAX_LEVELS), ("iterations", C.c_int32 * 4), ("max_trials", C.c_int32)]


def pose_params(fx, fy, cx, cy, bf, inv_level_sigma2=(1.0,), iterations=(0, 0, 0, 0), max_trials=0, nlevels=None):
    """rfe_pose_params from plain values (iterations / max_trials 0 = the reference's 10)"""
    p = PoseParams()
    p.fx, p.fy, p.cx, p.cy, p.bf = (float(v) for v in (fx, fy, cx, cy, bf))
    p.nlevels = len(inv_level_sigma2) if nlevels is None else int(nlevels)
    for l, v in enumerate(list(inv_level_sigma2)[:MAX_LEVELS]):
        p.inv_level_sigma2[l] = float(v)
    p.iterations[:] = [int(v) for v in iterations]
    p.max_trials = int(max_trials)
    return p


POSE_OUTPUTS = ("pose_f32", "chi2", "trace")
_pose = [C.c_void_p, C.POINTER(PoseParams), _fp, _fp, _ip, _fp, _fp, _u8p, _ip, C.c_int, C.c_int, _vp, _fp, _u8p, _fp, _vp, _ip]
lib.rfe_pose_optimization.argtypes = _pose
lib.rfe_pose_optimization_dev.argtypes = _pose


class PoseInertialParams(C.Structure):
    """include/rover_fe.h: rfe_pose_inertial_params -- intrinsics, mbf and mvInvLevelSigma2 of one PoseInertialOptimization call."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("nlevels", C.c_int32),
                ("inv_level_sigma2", C.c_float * MAX_LEVELS)]


def pose_inertial_params(fx, fy, cx, cy, bf, inv_level_sigma2=(1.0,), nlevels=None):
    """rfe_pose_inertial_params from plain values"""
    p = PoseInertialParams()
    p.fx, p.fy, p.cx, p.cy, p.bf = (float(v) for v in (fx, fy, cx, cy, bf))
    p.nlevels = len(inv_level_sigma2) if nlevels is None else int(nlevels)
    for l, v in enumerate(list(inv_level_sigma2)[:MAX_LEVELS]):
        p.inv_level_sigma2[l] = float(v)
    return p


PIO_LAST_KEYFRAME, PIO_LAST_FRAME = 0, 1
PIO_CAM_FLOATS, PIO_STATE_FLOATS, PIO_PREINT_FLOATS, PIO_COV_RW_FLOATS, PIO_PRIOR_DOUBLES = 36, 21, 148, 18, 246
PIO_OUTPUTS = ("state_f32", "chi2", "prior_out", "trace")
_pio = [C.c_void_p, C.POINTER(PoseInertialParams), _ip, _ip, _fp, _fp, _fp, _fp, _fp, _vp, _fp, _ip, _fp, _fp, _u8p, _fp, _ip, C.c_int, C.c_int,
        _vp, _fp, _u8p, _fp, _vp, _vp, _ip]
lib.rfe_pose_inertial_optimization.argtypes = _pio
lib.rfe_pose_inertial_optimization_dev.argtypes = _pio
lib.rfe_k_pose_inertial_classify.argtypes = [C.c_void_p, C.POINTER(PoseInertialParams), C.c_int, C.c_int, _vp, _fp, _ip, _fp, _fp, _fp, _u8p, _fp,
                                             C.c_int, _u8p, _fp]


class Sim3SolverParams(C.Structure):
    """include/rover_fe.h: rfe_sim3_solver_params -- both keyframes' poses and cameras, fix_scale, min_inliers, its and n of one Sim3Solver
    problem."""
    _fields_ = [("rcw1", C.c_float * 9), ("tcw1", C.c_float * 3), ("rcw2", C.c_float * 9), ("tcw2", C.c_float * 3),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("fix_scale", C.c_int32), ("min_inliers", C.c_int32), ("its", C.c_int32), ("n", C.c_int32)]


def sim3_solver_params(problems):
    """an rfe_sim3_solver_params array from dicts with rcw1, tcw1, rcw2, tcw2, cam1 / cam2 = (fx, fy, cx, cy), fix_scale, min_inliers, its, n"""
    arr = (Sim3SolverParams * max(len(problems), 1))()
    for p, d in zip(arr, problems):
        for k in ("rcw1", "tcw1", "rcw2", "tcw2"):
            getattr(p, k)[:] = [float(v) for v in np.asarray(d[k], np.float32).reshape(-1)]
        p.fx1, p.fy1, p.cx1, p.cy1 = (float(v) for v in d["cam1"])
        p.fx2, p.fy2, p.cx2, p.cy2 = (float(v) for v in d["cam2"])
        p.fix_scale, p.min_inliers, p.its, p.n = int(d["fix_scale"]), int(d["min_inliers"]), int(d["its"]), int(d["n"])
    return arr


SIM3_RANSAC_OUTPUTS = ("R", "t", "s", "inliers", "best_inliers", "counts", "hyps")
_s3 = [C.c_void_p, C.c_void_p, _fp, _fp, _fp, _fp, _ip, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _u8p, _u8p, _ip, _fp, _ip]
lib.rfe_sim3_ransac.argtypes = _s3
lib.rfe_sim3_ransac_dev.argtypes = _s3
lib.rfe_sim3_ransac_iterations.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int]


def sim3_ransac_iterations(probability, min_inliers, n, max_its):
    """SetRansacParameters' mRansacMaxIts (rfe_sim3_ransac_iterations; needs no device)"""
    return int(lib.rfe_sim3_ransac_iterations(float(probability), int(min_inliers), int(n), int(max_its)))


class TwoViewParams(C.Structure):
    """include/rover_fe.h: rfe_two_view_params -- camera, sigma, rh_threshold, min_parallax, min_triangulated, its, n1, n2 of one
    TwoViewReconstruction problem (0 = the reference's default, for every field behind cy but n1 / n2)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("sigma", C.c_float), ("rh_threshold", C.c_float),
                ("min_parallax", C.c_float), ("min_triangulated", C.c_int32), ("its", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32)]


def two_view_params(problems):
    """an rfe_two_view_params array from dicts with the structure's field names (missing fields are 0)"""
    arr = (TwoViewParams * max(len(problems), 1))()
    for p, d in zip(arr, problems):
        for k, t in TwoViewParams._fields_:
            setattr(p, k, (float if t is C.c_float else int)(d.get(k, 0)))
    return arr


TWO_VIEW_OUTPUTS = ("p3d", "triangulated", "inliers_h", "inliers_f", "scores", "models", "cand")
_tv = [C.c_void_p, C.c_void_p, _fp, _fp, _ip, _ip, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _u8p, _u8p, _u8p, _fp, _fp,
       _fp, _ip]
lib.rfe_two_view.argtypes = _tv
lib.rfe_two_view_dev.argtypes = _tv
lib.rfe_k_two_view_check.argtypes = [C.c_void_p, C.c_int, _fp, C.c_float, _fp, C.c_int, _fp, _u8p]
lib.rfe_k_two_view_check_rt.argtypes = [C.c_void_p, _fp, _fp, C.c_float, _fp, C.c_int, _u8p, _fp, _fp]
class OptimizeSim3Params(C.Structure):
    """include/rover_fe.h: rfe_optimize_sim3_params -- both keyframes' poses, cameras and level tables, th2, the flags, n / n2 and the LM
    schedule of one OptimizeSim3 problem."""
    _fields_ = [("rcw1", C.c_float * 9), ("tcw1", C.c_float * 3), ("rcw2", C.c_float * 9), ("tcw2", C.c_float * 3),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("nlevels1", C.c_int32), ("inv_level_sigma2_1", C.c_float * MAX_LEVELS),
                ("nlevels2", C.c_int32), ("inv_level_sigma2_2", C.c_float * MAX_LEVELS), ("th2", C.c_float),
                ("fix_scale", C.c_int32), ("all_points", C.c_int32), ("n", C.c_int32), ("n2", C.c_int32),
                ("iterations", C.c_int32 * 3), ("max_trials", C.c_int32)]


def optimize_sim3_params(problems):
    """an rfe_optimize_sim3_params array from dicts with rcw1, tcw1, rcw2, tcw2, cam1 / cam2 = (fx, fy, cx, cy), inv1 / inv2
    (mvInvLevelSigma2 of each keyframe), th2, fix_scale, all_points, n, n2 and optionally iterations (3), max_trials, nlevels1, nlevels2"""
    arr = (OptimizeSim3Params * max(len(problems), 1))()
    for p, d in zip(arr, problems):
        for k in ("rcw1", "tcw1", "rcw2", "tcw2"):
            getattr(p, k)[:] = [float(v) for v in np.asarray(d[k], np.float32).reshape(-1)]
        p.fx1, p.fy1, p.cx1, p.cy1 = (float(v) for v in d["cam1"])
        p.fx2, p.fy2, p.cx2, p.cy2 = (float(v) for v in d["cam2"])
        for side in ("1", "2"):
            inv = list(np.asarray(d["inv" + side], np.float32).reshape(-1))
            setattr(p, "nlevels" + side, int(d.get("nlevels" + side, len(inv))))
            for l, v in enumerate(inv[:MAX_LEVELS]):
                getattr(p, "inv_level_sigma2_" + side)[l] = float(v)
        p.th2 = float(d["th2"])
        p.fix_scale, p.all_points, p.n, p.n2 = int(d["fix_scale"]), int(d["all_points"]), int(d["n"]), int(d["n2"])
        p.iterations[:] = [int(v) for v in d.get("iterations", (0, 0, 0))]
        p.max_trials = int(d.get("max_trials", 0))
    return arr


OPTIMIZE_SIM3_OUTPUTS = ("s12_f32", "chi2", "trace")
_os3 = [C.c_void_p, C.c_void_p, _vp, _fp, _fp, _u8p, _fp, _ip, _ip, _fp, _ip, C.c_int, C.c_int, C.c_int, _vp, _fp, _u8p, _vp, _vp, _ip]
lib.rfe_optimize_sim3.argtypes = _os3
lib.rfe_optimize_sim3_dev.argtypes = _os3


class LocalBaParams(C.Structure):
    """include/rover_fe.h: rfe_local_ba_params, passed BY VALUE -- the LM schedule of one LocalBundleAdjustment, the two chi2 thresholds and
    the host address of pbStopFlag (0 = none)."""
    _fields_ = [("iterations", C.c_int32), ("max_trials", C.c_int32), ("user_lambda_init", C.c_double), ("th2_mono", C.c_double),
                ("th2_stereo", C.c_double), ("stop", C.c_void_p)]


def local_ba_params(iterations=10, max_trials=0, user_lambda_init=0.0, th2_mono=5.991, th2_stereo=7.815, stop=None):
    """stop: None, or a numpy uint8 array of one element that the caller keeps alive (pbStopFlag)"""
    return LocalBaParams(int(iterations), int(max_trials), float(user_lambda_init), float(th2_mono), float(th2_stereo),
                         None if stop is None else stop.ctypes.data)


LOCAL_BA_OUTPUTS = ("pose_f32", "point_f32", "chi2", "trace")
LBA_MAX_FREE, LBA_MAX_KF, LBA_MAX_POINTS, LBA_MAX_EDGES, LBA_MAX_ITERATIONS = 64, 256, 16384, 131072, 64
_lba = [C.c_void_p, LocalBaParams, _fp, _fp, _ip, _fp, _ip, _fp, _ip, _fp, _fp, _ip, _ip, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
        _vp, _fp, _vp, _fp, _u8p, _vp, _vp, _ip]
lib.rfe_local_ba.argtypes = _lba
lib.rfe_local_ba_dev.argtypes = _lba


class EssentialGraphParams(C.Structure):
    """include/rover_fe.h: rfe_essential_graph_params, passed BY VALUE -- the LM schedule of one OptimizeEssentialGraph and bFixScale."""
    _fields_ = [("iterations", C.c_int32), ("max_trials", C.c_int32), ("user_lambda_init", C.c_double), ("fix_scale", C.c_int32),
                ("reserved", C.c_int32)]


def essential_graph_params(iterations=20, max_trials=0, user_lambda_init=1e-16, fix_scale=False):
    return EssentialGraphParams(int(iterations), int(max_trials), float(user_lambda_init), 1 if fix_scale else 0, 0)


ESSENTIAL_GRAPH_OUTPUTS = ("tiw_f32", "swi", "chi2", "trace")
EG_MAX_KF, EG_MAX_EDGES, EG_MAX_POINTS, EG_MAX_ITERATIONS, EG_TILE_V = 1024, 16384, 1 << 20, 64, 4
_eg = [C.c_void_p, EssentialGraphParams, _vp, _vp, _u8p, _ip, _ip, _u8p, _fp, _ip, C.c_int, C.c_int, C.c_int, _vp, _fp, _vp, _fp, _vp, _vp, _ip]
lib.rfe_essential_graph.argtypes = _eg
lib.rfe_essential_graph_dev.argtypes = _eg


class GlobalBaParams(C.Structure):
    """include/rover_fe.h: rfe_global_ba_params, passed BY VALUE -- the LM schedule of one GlobalBundleAdjustemnt, bRobust with the two Huber
    thresholds and the host address of pbStopFlag (0 = none)."""
    _fields_ = [("iterations", C.c_int32), ("max_trials", C.c_int32), ("user_lambda_init", C.c_double), ("robust", C.c_int32),
                ("reserved", C.c_int32), ("huber2_mono", C.c_double), ("huber2_stereo", C.c_double), ("stop", C.c_void_p)]


def global_ba_params(iterations=10, max_trials=0, user_lambda_init=0.0, robust=False, huber2_mono=5.99, huber2_stereo=7.815, stop=None):
    """stop: None, or a numpy uint8 array of one element that the caller keeps alive (pbStopFlag)"""
    return GlobalBaParams(int(iterations), int(max_trials), float(user_lambda_init), 1 if robust else 0, 0, float(huber2_mono),
                          float(huber2_stereo), None if stop is None else stop.ctypes.data)


GLOBAL_BA_OUTPUTS = ("pose_f32", "point_f32", "chi2", "trace")
GBA_MAX_KF, GBA_MAX_POINTS, GBA_MAX_EDGES, GBA_MAX_ITERATIONS, GBA_MAX_PAIRS, GBA_TILE_V = 1024, 1 << 18, 1 << 21, 64, 1 << 25, 4
_gba = [C.c_void_p, GlobalBaParams, _fp, _fp, _ip, _fp, _ip, _u8p, _fp, _ip, _fp, _fp, _ip, _ip, _ip, C.c_int, C.c_int, C.c_int, C.c_int,
        _vp, _fp, _vp, _fp, _u8p, _vp, _vp, _ip]
lib.rfe_global_ba.argtypes = _gba
lib.rfe_global_ba_dev.argtypes = _gba
lib.rfe_k_global_ba_stop_after.argtypes = [C.c_void_p, C.c_int]


BOW_TF_IDF, BOW_TF, BOW_IDF, BOW_BINARY = 0, 1, 2, 3
BOW_L1_NORM = 0
BOW_MAX_N = 4096


class BowVocabDesc(C.Structure):
    """include/rover_fe.h: rfe_bow_vocab_desc -- a DBoW3 vocabulary tree in flat host arrays."""
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32), ("n_nodes", C.c_int32), ("D", C.c_int32),
                ("parent", C.c_void_p), ("child_offsets", C.c_void_p), ("children", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p),
                ("word_id", C.c_void_p)]


BOW_VOCAB_ARRAYS = (("parent", np.int32), ("child_offsets", np.int32), ("children", np.int32), ("desc", np.uint8), ("weight", np.float64),
                    ("word_id", np.int32))
lib.rfe_bow_vocab_create.argtypes = [C.c_void_p, C.POINTER(BowVocabDesc), C.POINTER(C.c_void_p)]
lib.rfe_bow_vocab_load.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
lib.rfe_bow_vocab_destroy.argtypes = [C.c_void_p]
lib.rfe_bow_vocab_destroy.restype = None
lib.rfe_bow_vocab_info.argtypes = [C.c_void_p, _ip]
_bowt = [C.c_void_p, C.c_void_p, _fp, _u8p, C.c_int, C.c_int, _ip, _ip, _vp, _ip, _ip, _vp, _ip, _ip, _ip, _ip]
lib.rfe_bow_transform.argtypes = _bowt
lib.rfe_bow_transform_dev.argtypes = _bowt
lib.rfe_bow_db_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.rfe_bow_db_destroy.argtypes = [C.c_void_p]
lib.rfe_bow_db_destroy.restype = None
lib.rfe_bow_db_add.argtypes = [C.c_void_p, _ip, _vp, C.c_int, C.POINTER(C.c_int32)]
lib.rfe_bow_db_add_dev.argtypes = lib.rfe_bow_db_add.argtypes
lib.rfe_bow_db_erase.argtypes = [C.c_void_p, C.c_int32]
lib.rfe_bow_db_clear.argtypes = [C.c_void_p]
lib.rfe_bow_db_size.argtypes = [C.c_void_p]
_bowq = [C.c_void_p, _ip, _vp, C.c_int, _u8p, _ip, _u8p, _vp, _ip]
lib.rfe_bow_db_query.argtypes = _bowq
lib.rfe_bow_db_query_dev.argtypes = _bowq
lib.rfe_k_bow_vocab_read.argtypes = [C.c_char_p, _ip, _ip, _ip, _ip, _u8p, _vp, _ip, C.c_char_p, C.c_int]
lib.rfe_profile_enable.argtypes = [C.c_void_p, C.c_int]
lib.rfe_profile_filter.argtypes = [C.c_void_p, C.c_char_p]
lib.rfe_profile_reset.argtypes = [C.c_void_p]
lib.rfe_profile_read.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
lib.rfe_k_conv3x3.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp]
lib.rfe_k_linear.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, _fp, _fp, C.c_int, C.c_int, _fp]
lib.rfe_k_scoremap.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]
lib.rfe_k_sparse_desc.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int, _ip, _ip, _fp, _fp]
lib.rfe_k_select.argtypes = [C.c_void_p, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _ip, _ip, _fp]
lib.rfe_k_select_keys.argtypes = lib.rfe_k_select.argtypes
lib.rfe_k_lightglue_taps.argtypes = [C.c_void_p, _fp, _fp, _fp, _fp, C.c_int, C.c_int, _fp, _fp, _fp]
lib.rfe_k_set_lightglue_tap.argtypes = [C.c_void_p, C.c_int, _fp, _fp, _fp]
lib.rfe_k_lightglue_ffn.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _fp]
lib.rfe_k_lightglue_self_attention.argtypes = [C.c_void_p, C.c_int, _fp, _fp, C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.POINTER(C.c_int32)]
lib.rfe_k_lightglue_assign.argtypes = [C.c_void_p, _fp, _fp, _fp, _fp, _ip, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int32,
                                       _fp, _fp, _fp, _fp, _ip, _ip, _ip, _ip, _fp, _fp]
lib.rfe_k_attention.argtypes = [C.c_void_p, _fp, _fp, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _fp]
lib.rfe_k_cross_attention.argtypes = [C.c_void_p, _fp, C.c_int, _fp, C.c_int, C.c_int, _ip, C.c_int]


POOL_AUTO, POOL_RCCL, POOL_COPY = 0, 1, 2
lib.rfe_pool_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
lib.rfe_pool_destroy.argtypes = [C.c_void_p]
lib.rfe_pool_destroy.restype = None
lib.rfe_pool_last_error.argtypes = [C.c_void_p]
lib.rfe_pool_last_error.restype = C.c_char_p
lib.rfe_pool_size.argtypes = [C.c_void_p]
lib.rfe_pool_ctx.argtypes = [C.c_void_p, C.c_int]
lib.rfe_pool_ctx.restype = C.c_void_p
lib.rfe_pool_has_rccl.argtypes = [C.c_void_p]
lib.rfe_k_pool_inject_gather_failure.argtypes = [C.c_void_p, C.c_int]
lib.rfe_load_onnx.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
lib.rfe_k_onnx_convert.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_char_p, C.c_int]
lib.rfe_host_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
lib.rfe_host_free.argtypes = [C.c_void_p]
lib.rfe_host_free.restype = None
lib.rfe_workspace_bytes.argtypes = [C.c_void_p]
lib.rfe_workspace_bytes.restype = C.c_int64
lib.rfe_pool_set_weights.argtypes = [C.c_void_p, C.c_int, _fp, C.c_int64]
lib.rfe_pool_load_weights.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
lib.rfe_pool_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
lib.rfe_pool_shard.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.rfe_pool_extract_match_stream.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                              _ip, _ip, _fp, _fp, _ip, _ip, _fp]


class RfeError(RuntimeError):
    pass


def _addr(a):
    """address of a numpy array (host) / int (device pointer) / object with data_ptr() (torch)."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    raise TypeError(type(a))


class DevBuf:
    """Device allocation owned by a Context (rfe_malloc / rfe_free)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        ctx._chk(lib.rfe_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(lib.rfe_memcpy_h2d(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._chk(lib.rfe_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib.rfe_free(self.ctx.h, self.ptr)
            self.ptr = None


def _dev(x):
    """address of a DevBuf / raw device address / torch tensor: what the _dev wrappers take for every array."""
    return x.ptr if isinstance(x, DevBuf) else _addr(x)


def _f32_rows(a, w):
    """a as contiguous float32 rows of w."""
    return np.ascontiguousarray(a, np.float32).reshape(-1, w)


def _opt(a, dt):
    """an optional array: None, or a flat and contiguous as dt."""
    return None if a is None else np.ascontiguousarray(a, dt).reshape(-1)


# per-map-point outputs of the projection-search fronts as the host wrappers preset them (n = max(Np, 1))
_PS_POINT_OUT = {"proj": lambda n: np.zeros((n, 2), np.float32), "radius": lambda n: np.zeros((n,), np.float32),
                 "proj_xr": lambda n: np.zeros((n,), np.float32), "depth": lambda n: np.zeros((n,), np.float32),
                 "view_cos": lambda n: np.zeros((n,), np.float32), "level": lambda n: np.full((n,), -1, np.int32),
                 "reject": lambda n: np.ones((n,), np.int32)}


def _ps_outputs(first, Np, Nf, front=()):
    """output arrays of a projection-search host wrapper in the order the C entry takes them: `first` [Nf] (assign / matched), best_idx /
    best_dist / second_dist [Np], then the front's (keys of _PS_POINT_OUT)."""
    n1, f1 = max(Np, 1), max(Nf, 1)
    o = {first: np.full((f1,), -1, np.int32), "best_idx": np.full((n1,), -1, np.int32), "best_dist": np.full((n1,), 256, np.float32),
         "second_dist": np.full((n1,), 256, np.float32)}
    o.update((k, _PS_POINT_OUT[k](n1)) for k in front)
    return o


def _ps_result(o, first, Np, Nf, nmatches, stats):
    """the dict a projection-search host wrapper returns: the arrays of _ps_outputs cut to their counts, nmatches, stats."""
    out = {k: (v[:Nf] if k == first else v[:Np]) for k, v in o.items()}
    out.update(nmatches=nmatches, stats=stats)
    return out


def read_bow_vocab(path):
    """The library's reader of DBoW3's uncompressed binary vocabulary stream, without a device (rfe_k_bow_vocab_read): a dict with k, L,
    weighting, scoring, n_nodes, D and the arrays of rfe_bow_vocab_desc.  RfeError with the reader's reason when it refuses the file."""
    hdr = np.zeros((6,), np.int32)
    err = C.create_string_buffer(512)
    rc = lib.rfe_k_bow_vocab_read(path.encode(), hdr.ctypes.data, None, None, None, None, None, None, err, 512)
    if rc != 0:
        raise RfeError(f"librover_fe error {rc}: {err.value.decode()}")
    k, L, weighting, scoring, n, D = (int(v) for v in hdr)
    v = {"k": k, "L": L, "weighting": weighting, "scoring": scoring, "n_nodes": n, "D": D,
         "parent": np.zeros((n,), np.int32), "child_offsets": np.zeros((n + 1,), np.int32), "children": np.zeros((max(n - 1, 1),), np.int32),
         "desc": np.zeros((n, D), np.uint8), "weight": np.zeros((n,), np.float64), "word_id": np.zeros((n,), np.int32)}
    rc = lib.rfe_k_bow_vocab_read(path.encode(), hdr.ctypes.data, *[v[name].ctypes.data for name, _ in BOW_VOCAB_ARRAYS], err, 512)
    if rc != 0:
        raise RfeError(f"librover_fe error {rc}: {err.value.decode()}")
    v["children"] = v["children"][:n - 1]
    return v


class BowVocab:
    """A DBoW3 vocabulary on the device of `ctx` (rfe_bow_vocab_create / rfe_bow_vocab_load).  tree: a dict with k, L,
    weighting, scoring, D and the arrays of rfe_bow_vocab_desc (n_nodes = len(weight)); path: an uncompressed DBoW3 binary stream."""

    def __init__(self, ctx, tree=None, path=None):
        assert (tree is None) != (path is None)
        self.ctx, h = ctx, C.c_void_p()
        if path is not None:
            ctx._chk(lib.rfe_bow_vocab_load(ctx.h, path.encode(), C.byref(h)))
        else:
            a = {name: np.ascontiguousarray(tree[name], dt) for name, dt in BOW_VOCAB_ARRAYS}
            d = BowVocabDesc(int(tree["k"]), int(tree["L"]), int(tree["weighting"]), int(tree["scoring"]),
                             int(tree.get("n_nodes", len(a["weight"]))), int(tree["D"]), *[a[name].ctypes.data for name, _ in BOW_VOCAB_ARRAYS])
            ctx._chk(lib.rfe_bow_vocab_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h
        info = np.zeros((8,), np.int32)
        lib.rfe_bow_vocab_info(self.h, info.ctypes.data)
        self.k, self.L, self.n_nodes, self.n_words, self.D, self.weighting, self.scoring, self.depth = (int(v) for v in info)

    def close(self):
        if self.h:
            lib.rfe_bow_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BowDatabase:
    """The keyframe database's BoW vectors on the device (rfe_bow_db_*): add / erase / clear, and query = common-word counts,
    the 0.8 max gate and the L1 scores of KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates."""

    def __init__(self, ctx):
        self.ctx, h = ctx, C.c_void_p()
        ctx._chk(lib.rfe_bow_db_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib.rfe_bow_db_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.ctx._chk(lib.rfe_bow_db_size(self.h))

    def add(self, word, value):
        w, v = np.ascontiguousarray(word, np.int32).reshape(-1), np.ascontiguousarray(value, np.float64).reshape(-1)
        assert len(w) == len(v)
        e = C.c_int32(-1)
        self.ctx._chk(lib.rfe_bow_db_add(self.h, w.ctypes.data, v.ctypes.data, len(w), C.byref(e)))
        return e.value

    def add_dev(self, word, value, n):
        a = _dev
        e = C.c_int32(-1)
        self.ctx._chk(lib.rfe_bow_db_add_dev(self.h, a(word), a(value), int(n), C.byref(e)))
        return e.value

    def erase(self, entry):
        self.ctx._chk(lib.rfe_bow_db_erase(self.h, int(entry)))

    def clear(self):
        self.ctx._chk(lib.rfe_bow_db_clear(self.h))

    def query(self, word, value, exclude=None, score=None):
        """Host arrays.  score: the array the scores are written into (float64 [len(self)]; zeros when None) -- entries that are not scored
        keep what it held.  Returns a dict: common, scored, score, stats [4] = max_common, min_common, n_sharing, n_scored."""
        E = len(self)
        w, v = np.ascontiguousarray(word, np.int32).reshape(-1), np.ascontiguousarray(value, np.float64).reshape(-1)
        assert len(w) == len(v)
        ex = None if exclude is None else np.ascontiguousarray(exclude, np.uint8).reshape(-1)
        assert ex is None or len(ex) == E
        common, scored = np.zeros((max(E, 1),), np.int32), np.zeros((max(E, 1),), np.uint8)
        sc = np.zeros((max(E, 1),), np.float64)
        if score is not None:
            sc[:E] = score
        st = np.zeros((4,), np.int32)
        self.ctx._chk(lib.rfe_bow_db_query(self.h, w.ctypes.data, v.ctypes.data, len(w), _addr(ex), common.ctypes.data, scored.ctypes.data,
                                           sc.ctypes.data, st.ctypes.data))
        return {"common": common[:E], "scored": scored[:E], "score": sc[:E], "stats": st}

    def query_dev(self, word, value, nq, common, scored, score, stats, exclude=None):
        """rfe_bow_db_query_dev: every array a DevBuf (or a raw device address / torch tensor); asynchronous on the ctx stream."""
        a = _dev
        self.ctx._chk(lib.rfe_bow_db_query_dev(self.h, a(word), a(value), int(nq), a(exclude), a(common), a(scored), a(score), a(stats)))


def split_levels(flat, level_h, level_w):
    """[B, sum_l H_l*W_l] level buffer of rfe_extract_pyramid_u8 -> list of [B,H_l,W_l] views, level 0 first."""
    out, off = [], 0
    for h, w in zip(level_h, level_w):
        out.append(flat[:, off:off + int(h) * int(w)].reshape(flat.shape[0], int(h), int(w)))
        off += int(h) * int(w)
    return out


class StereoStream:
    """Device-resident stereo stream (rfe_stereo_frame_dev): owns the output buffers, push() enqueues one stereo frame
    (device image pointers) without any host synchronisation, results() downloads the last frame's outputs."""

    def __init__(self, ctx, H, W, kmax=1024, mb=0.11, mbf=0.11 * 435.0, thr=0.0005, filter_thr=0.1):
        self.ctx, self.H, self.W, self.K = ctx, H, W, kmax
        self.mb, self.mbf, self.thr, self.filter_thr = mb, mbf, thr, filter_thr
        K = kmax
        self._spec = [("n", np.int32, (2,)), ("kxy", np.int32, (2, K, 2)), ("score", np.float32, (2, K)), ("desc", np.float32, (2, K, 256)),
                      ("u_right", np.float32, (K,)), ("depth", np.float32, (K,)), ("S", np.int32, (1,)), ("pairs", np.int32, (K, 2)),
                      ("ms", np.float32, (K,))]
        self.bufs = {name: ctx.alloc(int(np.prod(shape)) * np.dtype(dt).itemsize) for name, dt, shape in self._spec}
        self.first = True

    def push(self, img_l_dev, img_r_dev, stride=None, reset=False):
        b = self.bufs
        self.ctx._chk(lib.rfe_stereo_frame_dev(self.ctx.h, _addr(img_l_dev), _addr(img_r_dev), self.H, self.W, stride or self.W, self.K,
                                               self.thr, self.filter_thr, self.mb, self.mbf, int(reset or self.first), b["n"].ptr,
                                               b["kxy"].ptr, b["score"].ptr, b["desc"].ptr, b["u_right"].ptr, b["depth"].ptr,
                                               b["S"].ptr, b["pairs"].ptr, b["ms"].ptr))
        self.first = False

    def results(self):
        self.ctx.synchronize()
        out = {name: self.bufs[name].download(shape, dt) for name, dt, shape in self._spec}
        out["S"] = int(out["S"][0])
        return out

    def close(self):
        for b in self.bufs.values():
            b.free()
        self.bufs = {}


STEREO_SAD_LEVEL, STEREO_SAD_LEVEL0 = 0, 1   # include/rover_fe.h: RFE_STEREO_SAD_*


class StereoPyramidStream:
    """StereoStream for scale pyramids (rfe_stereo_frame_pyramid_dev): kmax is one budget per level (or an int for every level)."""

    def __init__(self, ctx, H, W, nlevels=8, scale_factor=1.2, kmax=128, mb=0.11, mbf=0.11 * 435.0, thr=0.0005, filter_thr=0.1,
                 sad_source=STEREO_SAD_LEVEL):
        self.ctx, self.H, self.W, self.L, self.sf = ctx, H, W, int(nlevels), scale_factor
        self.kmax = np.full((max(self.L, 1),), int(kmax), np.int32) if np.isscalar(kmax) else np.ascontiguousarray(kmax, np.int32)
        self.mb, self.mbf, self.thr, self.filter_thr, self.sad_source = mb, mbf, thr, filter_thr, sad_source
        K = self.K = int(self.kmax.sum())
        self._spec = [("n", np.int32, (2,)), ("level_n", np.int32, (2, max(self.L, 1))), ("kpts", np.float32, (2, K, 2)),
                      ("octave", np.int32, (2, K)), ("score", np.float32, (2, K)), ("desc", np.float32, (2, K, 256)),
                      ("u_right", np.float32, (K,)), ("depth", np.float32, (K,)), ("S", np.int32, (1,)), ("pairs", np.int32, (K, 2)),
                      ("ms", np.float32, (K,))]
        self.bufs = {name: ctx.alloc(max(int(np.prod(shape)), 1) * np.dtype(dt).itemsize) for name, dt, shape in self._spec}
        self.first = True

    def push(self, img_l_dev, img_r_dev, stride=None, reset=False):
        b = self.bufs
        self.ctx._chk(lib.rfe_stereo_frame_pyramid_dev(self.ctx.h, _addr(img_l_dev), _addr(img_r_dev), self.H, self.W, stride or self.W, self.L,
                                                       self.sf, self.kmax.ctypes.data, self.thr, self.filter_thr, self.mb, self.mbf,
                                                       self.sad_source, int(reset or self.first), b["n"].ptr, b["level_n"].ptr, b["kpts"].ptr,
                                                       b["octave"].ptr, b["score"].ptr, b["desc"].ptr, b["u_right"].ptr, b["depth"].ptr,
                                                       b["S"].ptr, b["pairs"].ptr, b["ms"].ptr))
        self.first = False

    def results(self):
        self.ctx.synchronize()
        out = {name: self.bufs[name].download(shape, dt) for name, dt, shape in self._spec}
        out["S"] = int(out["S"][0])
        return out

    def close(self):
        for b in self.bufs.values():
            b.free()
        self.bufs = {}


MAX_LEVELS = 16


def pyramid_geometry(H, W, nlevels, scale_factor):
    """rfe_pyramid_geometry: (level_h, level_w, level_scale) of the scale pyramid (pure function, no device).  Raises RfeError for
    arguments rfe_extract_pyramid_u8 refuses, a level that rounds to zero pixels included."""
    L = max(int(nlevels), 1)
    h, w, s = np.zeros((L,), np.int32), np.zeros((L,), np.int32), np.zeros((L,), np.float32)
    rc = lib.rfe_pyramid_geometry(H, W, nlevels, scale_factor, h.ctypes.data, w.ctypes.data, s.ctypes.data)
    if rc < 0:
        raise RfeError(f"rfe_pyramid_geometry({H}, {W}, {nlevels}, {scale_factor}) failed ({rc})")
    return h, w, s


def pool_shard(F, n, member):
    """rfe_pool_shard: (first_frame, frames, pairs) of `member` among n for an F-frame stream (pure function, no device)."""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.rfe_pool_shard(F, n, member, C.byref(a), C.byref(b), C.byref(c))
    if rc < 0:
        raise RfeError(f"rfe_pool_shard({F}, {n}, {member}) failed ({rc})")
    return a.value, b.value, c.value


class Pool:
    """rfe_pool: one ctx + host thread per member device; a stream of F frames sharded with one overlap frame, results
    gathered into member 0's device (RCCL or copies) and returned as host arrays in global order."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = lib.rfe_pool_create(devs, len(devices), C.byref(h))
        if rc != 0:
            raise RfeError(f"rfe_pool_create failed ({rc}): {lib.rfe_pool_last_error(None).decode()}")
        self.h = h

    def close(self):
        if self.h:
            lib.rfe_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise RfeError(f"librover_fe pool error {rc}: {lib.rfe_pool_last_error(self.h).decode()}")
        return rc

    @property
    def size(self):
        return lib.rfe_pool_size(self.h)

    @property
    def has_rccl(self):
        return bool(lib.rfe_pool_has_rccl(self.h))

    def set_weights(self, kind, blob):
        blob = np.ascontiguousarray(blob, np.float32)
        self._chk(lib.rfe_pool_set_weights(self.h, kind, blob.ctypes.data, blob.size))

    def set_option(self, option, value):
        self._chk(lib.rfe_pool_set_option(self.h, option, int(value)))

    def set_hparams(self, **kw):
        """Change some graph hyper-parameters (keys of rfe_hparams) on EVERY member; the others keep member 0's current values."""
        h = HParams()
        rc = lib.rfe_get_hparams(lib.rfe_pool_ctx(self.h, 0), C.byref(h))
        if rc < 0:
            raise RfeError(f"rfe_get_hparams on pool member 0 failed ({rc})")
        for k, v in kw.items():
            if not hasattr(h, k):
                raise KeyError(k)
            setattr(h, k, v)
        self._chk(lib.rfe_pool_set_hparams(self.h, C.byref(h)))

    def extract_match_stream(self, frames_u8, kmax=1024, thr=0.0005, filter_thr=0.1, transport=POOL_AUTO, with_desc=True):
        """frames_u8: host [F,H,W] uint8.  Returns dict n [F], kxy [F,K,2], score / desc (with_desc), S [F-1], pairs [F-1,K,2], ms [F-1,K]."""
        img = np.ascontiguousarray(frames_u8, np.uint8)
        F, H, W = img.shape
        P = max(F - 1, 1)
        out = {"n": np.zeros((F,), np.int32), "kxy": np.zeros((F, kmax, 2), np.int32), "S": np.zeros((P,), np.int32),
               "pairs": np.zeros((P, kmax, 2), np.int32), "ms": np.zeros((P, kmax), np.float32)}
        if with_desc:
            out["score"] = np.zeros((F, kmax), np.float32)
            out["desc"] = np.zeros((F, kmax, 256), np.float32)
        self._chk(lib.rfe_pool_extract_match_stream(self.h, img.ctypes.data, H, W, W, F, kmax, thr, filter_thr, transport, out["n"].ctypes.data,
                                                    out["kxy"].ctypes.data, out["score"].ctypes.data if with_desc else None,
                                                    out["desc"].ctypes.data if with_desc else None, out["S"].ctypes.data,
                                                    out["pairs"].ctypes.data, out["ms"].ctypes.data))
        return out


class Context:
    """One rfe_ctx (own HIP stream + workspaces).  Single caller, like one ORT session of the reference."""

    def __init__(self, device=0):
        h = C.c_void_p()
        rc = lib.rfe_init(device, C.byref(h))
        if rc != 0:
            raise RfeError(f"rfe_init failed ({rc}): {lib.rfe_last_error(None).decode()}")
        self.h = h

    def close(self):
        if self.h:
            lib.rfe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise RfeError(f"librover_fe error {rc}: {lib.rfe_last_error(self.h).decode()}")
        return rc

    # ---- weights
    def set_weights(self, kind, blob):
        blob = np.ascontiguousarray(blob, np.float32)
        self._chk(lib.rfe_set_weights(self.h, kind, blob.ctypes.data, blob.size))

    def load_weights(self, sp_path=None, lg_path=None):
        self._chk(lib.rfe_load_weights(self.h, sp_path.encode() if sp_path else None, lg_path.encode() if lg_path else None))

    def get_hparams(self):
        h = HParams()
        self._chk(lib.rfe_get_hparams(self.h, C.byref(h)))
        return h.as_dict()

    def set_hparams(self, **kw):
        """Change some of the graph hyper-parameters (keys of rfe_hparams); the others keep their current values."""
        h = HParams()
        self._chk(lib.rfe_get_hparams(self.h, C.byref(h)))
        for k, v in kw.items():
            if not hasattr(h, k):
                raise KeyError(k)
            setattr(h, k, v)
        self._chk(lib.rfe_set_hparams(self.h, C.byref(h)))

    def set_option(self, option, value):
        self._chk(lib.rfe_set_option(self.h, option, int(value)))

    def get_option(self, option):
        v = C.c_int()
        self._chk(lib.rfe_get_option(self.h, option, C.byref(v)))
        return v.value

    def set_stream(self, stream_ptr):
        self._chk(lib.rfe_set_stream(self.h, stream_ptr))

    def workspace_bytes(self):
        return int(lib.rfe_workspace_bytes(self.h))

    def synchronize(self):
        self._chk(lib.rfe_synchronize(self.h))

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    # ---- host-buffer entry points
    def extract(self, img_u8, kmax=1024, thr=0.0005, pad_cols=0, binarized=False):
        """img_u8: [B,H,W] or [H,W] uint8 (host).  Returns n[B], kxy[B,Kmax,2], score[B,Kmax], desc[B,Kmax,256]
        (+ desc_bin u8 [B,Kmax,256] when binarized=True: Frame::binarize_descriptors written by the sampling kernel).
        pad_cols > 0 passes the frames with a row stride of W + pad_cols bytes (like a cv::Mat ROI)."""
        img = np.ascontiguousarray(img_u8, np.uint8)
        if img.ndim == 2:
            img = img[None]
        B, H, W = img.shape
        stride = W + pad_cols
        if pad_cols:
            wide = np.full((B, H, stride), 255, np.uint8)
            wide[:, :, :W] = img
            img = wide
        n = np.zeros((B,), np.int32)
        kxy = np.zeros((B, kmax, 2), np.int32)
        score = np.zeros((B, kmax), np.float32)
        desc = np.zeros((B, kmax, 256), np.float32)
        if binarized:
            dbin = np.zeros((B, kmax, 256), np.uint8)
            self._chk(lib.rfe_extract_u8_bin(self.h, img.ctypes.data, H, W, stride, B, kmax, thr, n.ctypes.data, kxy.ctypes.data,
                                             score.ctypes.data, desc.ctypes.data, dbin.ctypes.data))
            return n, kxy, score, desc, dbin
        self._chk(lib.rfe_extract_u8(self.h, img.ctypes.data, H, W, stride, B, kmax, thr, n.ctypes.data, kxy.ctypes.data,
                                     score.ctypes.data, desc.ctypes.data))
        return n, kxy, score, desc

    def extract_pyramid(self, frames_u8, nlevels=8, scale_factor=1.2, kmax=1024, thr=0.0005, with_levels=False, pad_cols=0):
        """SuperPoint on a scale pyramid (rfe_extract_pyramid_u8).  frames_u8: [B,H,W] or [H,W] uint8 (host); kmax: an int (every level)
        or one budget per level.  Returns a dict: n [B], level_n [B,L], kpts [B,Ktot,2] f32 level-0 pixels, octave [B,Ktot], score [B,Ktot],
        desc [B,Ktot,256] (Ktot = sum of the budgets) and, with_levels, levels: a list of L arrays [B,H_l,W_l] u8."""
        img = np.ascontiguousarray(frames_u8, np.uint8)
        if img.ndim == 2:
            img = img[None]
        B, H, W = img.shape
        stride = W + pad_cols
        if pad_cols:
            wide = np.full((B, H, stride), 255, np.uint8)
            wide[:, :, :W] = img
            img = wide
        L = int(nlevels)
        km = np.full((max(L, 1),), int(kmax), np.int32) if np.isscalar(kmax) else np.ascontiguousarray(kmax, np.int32)
        K = int(km.sum())
        out = {"n": np.zeros((B,), np.int32), "level_n": np.zeros((B, max(L, 1)), np.int32), "kpts": np.zeros((B, K, 2), np.float32),
               "octave": np.zeros((B, K), np.int32), "score": np.zeros((B, K), np.float32), "desc": np.zeros((B, K, 256), np.float32)}
        lv = None
        if with_levels:
            lh, lw, _ = pyramid_geometry(H, W, L, scale_factor)
            lv = np.zeros((B, int((lh.astype(np.int64) * lw).sum())), np.uint8)
        self._chk(lib.rfe_extract_pyramid_u8(self.h, img.ctypes.data, H, W, stride, B, L, scale_factor, km.ctypes.data, thr,
                                             out["n"].ctypes.data, out["level_n"].ctypes.data, out["kpts"].ctypes.data,
                                             out["octave"].ctypes.data, out["score"].ctypes.data, out["desc"].ctypes.data,
                                             None if lv is None else lv.ctypes.data))
        if with_levels:
            out["levels"] = split_levels(lv, lh, lw)
        return out

    def extract_f32(self, img_f32, kmax=1024, thr=0.0005):
        """The float entry: img_f32 [B,H,W] or [H,W] float32, already normalised (what the reference's Extractor_Inference is handed).
        Same outputs as extract()."""
        img = np.ascontiguousarray(img_f32, np.float32)
        if img.ndim == 2:
            img = img[None]
        B, H, W = img.shape
        n = np.zeros((B,), np.int32)
        kxy = np.zeros((B, kmax, 2), np.int32)
        score = np.zeros((B, kmax), np.float32)
        desc = np.zeros((B, kmax, 256), np.float32)
        self._chk(lib.rfe_extract_f32(self.h, img.ctypes.data, H, W, W, B, kmax, thr, n.ctypes.data, kxy.ctypes.data,
                                      score.ctypes.data, desc.ctypes.data))
        return n, kxy, score, desc

    def match(self, k0n, k1n, d0, d1, m, n, filter_thr=0.1):
        """Batched pairs, host arrays: k0n [P,Mmax,2], d0 [P,Mmax,256], m [P] ...  Returns S[P], pairs, ms."""
        k0n = np.ascontiguousarray(k0n, np.float32); k1n = np.ascontiguousarray(k1n, np.float32)
        d0 = np.ascontiguousarray(d0, np.float32); d1 = np.ascontiguousarray(d1, np.float32)
        m = np.ascontiguousarray(m, np.int32); n = np.ascontiguousarray(n, np.int32)
        P, Mmax = k0n.shape[0], k0n.shape[1]
        Nmax = k1n.shape[1]
        cap = min(Mmax, Nmax)
        S = np.zeros((P,), np.int32)
        pairs = np.zeros((P, cap, 2), np.int32)
        ms = np.zeros((P, cap), np.float32)
        self._chk(lib.rfe_match(self.h, k0n.ctypes.data, k1n.ctypes.data, d0.ctypes.data, d1.ctypes.data, m.ctypes.data,
                                n.ctypes.data, P, Mmax, Nmax, filter_thr, S.ctypes.data, pairs.ctypes.data, ms.ctypes.data))
        return S, pairs, ms

    def match_fused(self, kpts0, kpts1, desc0, desc1, rows, cols, filter_thr=0.1, match_thresh=0.0):
        kpts0 = np.ascontiguousarray(kpts0, np.float32).reshape(-1, 2)
        kpts1 = np.ascontiguousarray(kpts1, np.float32).reshape(-1, 2)
        desc0 = np.ascontiguousarray(desc0, np.float32); desc1 = np.ascontiguousarray(desc1, np.float32)
        M, N = kpts0.shape[0], kpts1.shape[0]
        vn = np.full((max(M, 1),), -1, np.int32)
        size = self._chk(lib.rfe_match_fused(self.h, kpts0.ctypes.data, M, kpts1.ctypes.data, N, desc0.ctypes.data,
                                             desc1.ctypes.data, rows, cols, filter_thr, match_thresh, vn.ctypes.data))
        return size, vn[:M]

    def stereo_match(self, img_l, img_r, k_l, k_r, d_l, d_r, mb, mbf):
        """Frame::ComputeStereoMatches on host arrays; returns (uRight[N], depth[N])."""
        il = np.ascontiguousarray(img_l, np.uint8); ir = np.ascontiguousarray(img_r, np.uint8)
        kl = np.ascontiguousarray(k_l, np.float32).reshape(-1, 2); kr = np.ascontiguousarray(k_r, np.float32).reshape(-1, 2)
        dl = np.ascontiguousarray(d_l, np.float32); dr = np.ascontiguousarray(d_r, np.float32)
        H, W = il.shape
        N, Nr = kl.shape[0], kr.shape[0]
        u = np.full((max(N, 1),), -1, np.float32); z = np.full((max(N, 1),), -1, np.float32)
        self._chk(lib.rfe_stereo_match(self.h, il.ctypes.data, ir.ctypes.data, H, W, W, kl.ctypes.data, N, kr.ctypes.data, Nr,
                                       dl.ctypes.data, dr.ctypes.data, mb, mbf, u.ctypes.data, z.ctypes.data))
        return u[:N], z[:N]

    def stereo_match_pyramid(self, levels_l, levels_r, H, W, nlevels, scale_factor, k_l, oct_l, k_r, oct_r, d_l, d_r, mb, mbf, sad_source=0):
        """Octave-aware Frame::ComputeStereoMatches (rfe_stereo_match_pyramid) on host arrays.  levels_l / levels_r: one view's level
        images, either the flat [sum_l H_l*W_l] u8 buffer or a list of [H_l,W_l] arrays, level 0 first; returns (uRight[N], depth[N])."""
        def flat(lv):
            if isinstance(lv, (list, tuple)):
                return np.concatenate([np.ascontiguousarray(a, np.uint8).reshape(-1) for a in lv])
            return np.ascontiguousarray(lv, np.uint8).reshape(-1)
        vl, vr = flat(levels_l), flat(levels_r)
        lh, lw, _ = pyramid_geometry(H, W, nlevels, scale_factor)
        need = int((lh.astype(np.int64) * lw).sum())
        if vl.size != need or vr.size != need:
            raise RfeError(f"stereo_match_pyramid: level buffers hold {vl.size} / {vr.size} bytes, the geometry needs {need}")
        kl = np.ascontiguousarray(k_l, np.float32).reshape(-1, 2); kr = np.ascontiguousarray(k_r, np.float32).reshape(-1, 2)
        ol = np.ascontiguousarray(oct_l, np.int32).reshape(-1); orr = np.ascontiguousarray(oct_r, np.int32).reshape(-1)
        dl = np.ascontiguousarray(d_l, np.float32).reshape(-1, 256); dr = np.ascontiguousarray(d_r, np.float32).reshape(-1, 256)
        N, Nr = kl.shape[0], kr.shape[0]
        assert ol.shape[0] == N and orr.shape[0] == Nr and dl.shape[0] == N and dr.shape[0] == Nr
        u = np.full((max(N, 1),), -1, np.float32); z = np.full((max(N, 1),), -1, np.float32)
        self._chk(lib.rfe_stereo_match_pyramid(self.h, vl.ctypes.data, vr.ctypes.data, H, W, nlevels, scale_factor, kl.ctypes.data,
                                               ol.ctypes.data, N, kr.ctypes.data, orr.ctypes.data, Nr, dl.ctypes.data, dr.ctypes.data,
                                               mb, mbf, sad_source, u.ctypes.data, z.ctypes.data))
        return u[:N], z[:N]

    def search_candidates(self, q, f, offsets, cand, skip=None):
        """Best / second-best scan of SearchByProjection1 (SPmatcher.cc:1218-1248) over CSR candidate lists."""
        qa = np.ascontiguousarray(q, np.float32).reshape(-1, 256); fa = np.ascontiguousarray(f, np.float32).reshape(-1, 256)
        off = np.ascontiguousarray(offsets, np.int32); cd = np.ascontiguousarray(cand, np.int32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        Nq = qa.shape[0]
        bi = np.empty((max(Nq, 1),), np.int32); bd = np.empty((max(Nq, 1),), np.float32); sd = np.empty((max(Nq, 1),), np.float32)
        self._chk(lib.rfe_search_candidates(self.h, qa.ctypes.data, Nq, fa.ctypes.data, fa.shape[0], off.ctypes.data,
                                            cd.ctypes.data, None if sk is None else sk.ctypes.data, bi.ctypes.data,
                                            bd.ctypes.data, sd.ctypes.data))
        return bi[:Nq], bd[:Nq], sd[:Nq]

    def search_by_projection(self, q, proj, radius, f, bounds, kpts=None, kxy=None, pred_level=None, observed=None, octave=None, skip=None,
                             th_high=1.4):
        """SPmatcher::SearchByProjection1 as one call (rfe_search_by_projection, host arrays).  bounds = (min_x, min_y, max_x, max_y);
        exactly one of kpts [Nf,2] f32 and kxy [Nf,2] i32.  Returns a dict: assign [Nf], best_idx / best_dist / second_dist [Nq],
        nmatches, stats [4] (nmatches, candidates, rounds, overflow)."""
        qa, fa, pa, ra = _f32_rows(q, 256), _f32_rows(f, 256), _f32_rows(proj, 2), np.ascontiguousarray(radius, np.float32).reshape(-1)
        Nq, Nf = qa.shape[0], fa.shape[0]
        assert pa.shape[0] == Nq and ra.shape[0] == Nq
        ka, xa, lv, ob = _opt(kpts, np.float32), _opt(kxy, np.int32), _opt(pred_level, np.int32), _opt(observed, np.uint8)
        oc, sk = _opt(octave, np.int32), _opt(skip, np.uint8)
        o, st = _ps_outputs("assign", Nq, Nf), np.zeros((4,), np.int32)
        n = self._chk(lib.rfe_search_by_projection(self.h, qa.ctypes.data, pa.ctypes.data, ra.ctypes.data, _addr(lv), _addr(ob), Nq,
                                                   fa.ctypes.data, _addr(ka), _addr(xa), _addr(oc), _addr(sk), Nf, *[float(b) for b in bounds],
                                                   th_high, *[o[k].ctypes.data for k in o], st.ctypes.data))
        return _ps_result(o, "assign", Nq, Nf, n, st)

    def search_by_projection_dev(self, q, proj, radius, Nq, f, Nf, bounds, cand_cap, assign, stats, kpts=None, kxy=None, pred_level=None,
                                 observed=None, octave=None, skip=None, nf_dev=None, th_high=1.4, best_idx=None, best_dist=None,
                                 second_dist=None):
        """rfe_search_by_projection_dev: every array a DevBuf (or a raw device address / torch tensor); asynchronous on the ctx stream,
        outputs land in assign [Nf], stats [4] and the optional best_idx / best_dist / second_dist [Nq]."""
        a = _dev
        self._chk(lib.rfe_search_by_projection_dev(self.h, a(q), a(proj), a(radius), a(pred_level), a(observed), Nq, a(f), a(kpts), a(kxy),
                                                   a(octave), a(skip), Nf, a(nf_dev), *[float(b) for b in bounds], th_high, cand_cap,
                                                   a(assign), a(best_idx), a(best_dist), a(second_dist), a(stats)))

    def search_by_projection_sim3(self, params, q, pw, normal, min_dist, max_dist, scale_dist, f, th_accept, valid=None, kpts=None, kxy=None,
                                  matched_in=None):
        """The Sim3 SearchByProjection overloads of loop closing as one call (rfe_search_by_projection_sim3, host arrays).
        params: a Sim3Params (sim3_params()); scale_dist [Np] is the bare mfMaxDistance of PredictScale; exactly one of kpts [Nf,2] f32 and kxy [Nf,2] i32.  Returns a dict: matched [Nf], best_idx /
        best_dist / second_dist / radius / level / reject [Np], proj [Np,2], nmatches, stats [8]."""
        qa, fa, pa, na = _f32_rows(q, 256), _f32_rows(f, 256), _f32_rows(pw, 3), _f32_rows(normal, 3)
        mn, mx, sc = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (min_dist, max_dist, scale_dist))
        Np, Nf = qa.shape[0], fa.shape[0]
        assert pa.shape[0] == Np and na.shape[0] == Np and mn.shape[0] == Np and mx.shape[0] == Np and sc.shape[0] == Np
        va, ka, xa, mi = _opt(valid, np.uint8), _opt(kpts, np.float32), _opt(kxy, np.int32), _opt(matched_in, np.uint8)
        o, st = _ps_outputs("matched", Np, Nf, ("proj", "radius", "level", "reject")), np.zeros((8,), np.int32)
        n = self._chk(lib.rfe_search_by_projection_sim3(self.h, C.byref(params), qa.ctypes.data, pa.ctypes.data, na.ctypes.data, mn.ctypes.data,
                                                        mx.ctypes.data, sc.ctypes.data, _addr(va), Np, fa.ctypes.data, _addr(ka), _addr(xa), _addr(mi), Nf,
                                                        float(th_accept), *[o[k].ctypes.data for k in o], st.ctypes.data))
        return _ps_result(o, "matched", Np, Nf, n, st)

    def search_by_projection_sim3_dev(self, params, q, pw, normal, min_dist, max_dist, scale_dist, Np, f, Nf, th_accept, cand_cap, matched, stats,
                                      valid=None, kpts=None, kxy=None, matched_in=None, nf_dev=None, best_idx=None, best_dist=None,
                                      second_dist=None, proj=None, radius=None, level=None, reject=None):
        """rfe_search_by_projection_sim3_dev: every array a DevBuf (or a raw device address / torch tensor); asynchronous on the ctx stream,
        outputs land in matched [Nf], stats [8] and the optional per-map-point arrays."""
        a = _dev
        self._chk(lib.rfe_search_by_projection_sim3_dev(self.h, C.byref(params), a(q), a(pw), a(normal), a(min_dist), a(max_dist), a(scale_dist), a(valid), Np,
                                                        a(f), a(kpts), a(kxy), a(matched_in), Nf, a(nf_dev), float(th_accept), cand_cap,
                                                        a(matched), a(best_idx), a(best_dist), a(second_dist), a(proj), a(radius), a(level),
                                                        a(reject), a(stats)))

    def search_local_points(self, params, q, pw, normal, min_dist, max_dist, scale_dist, f, valid=None, observed=None, kpts=None, kxy=None,
                            octave=None, skip=None, th_high=1.4):
        """Steps 2 and 3 of Tracking::SearchLocalPoints as one call (rfe_search_local_points, host arrays).  params: a
        FrustumParams (frustum_params()); scale_dist [Np] is the bare mfMaxDistance of PredictScale; exactly one of kpts [Nf,2] f32 and kxy
        [Nf,2] i32.  Returns a dict: assign [Nf], best_idx / best_dist / second_dist / proj_xr / depth / view_cos / level / reject [Np],
        proj [Np,2], nmatches, stats [8]."""
        qa, fa, pa, na = _f32_rows(q, 256), _f32_rows(f, 256), _f32_rows(pw, 3), _f32_rows(normal, 3)
        mn, mx, sc = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (min_dist, max_dist, scale_dist))
        Np, Nf = qa.shape[0], fa.shape[0]
        assert pa.shape[0] == Np and na.shape[0] == Np and mn.shape[0] == Np and mx.shape[0] == Np and sc.shape[0] == Np
        va, ob, ka, xa = _opt(valid, np.uint8), _opt(observed, np.uint8), _opt(kpts, np.float32), _opt(kxy, np.int32)
        oc, sk = _opt(octave, np.int32), _opt(skip, np.uint8)
        o = _ps_outputs("assign", Np, Nf, ("proj", "proj_xr", "depth", "view_cos", "level", "reject"))
        st = np.zeros((8,), np.int32)
        n = self._chk(lib.rfe_search_local_points(self.h, C.byref(params), qa.ctypes.data, pa.ctypes.data, na.ctypes.data, mn.ctypes.data,
                                                  mx.ctypes.data, sc.ctypes.data, _addr(va), _addr(ob), Np, fa.ctypes.data, _addr(ka), _addr(xa),
                                                  _addr(oc), _addr(sk), Nf, float(th_high), *[o[k].ctypes.data for k in o], st.ctypes.data))
        return _ps_result(o, "assign", Np, Nf, n, st)

    def search_local_points_dev(self, params, q, pw, normal, min_dist, max_dist, scale_dist, Np, f, Nf, cand_cap, assign, stats, valid=None,
                                observed=None, kpts=None, kxy=None, octave=None, skip=None, nf_dev=None, th_high=1.4, best_idx=None,
                                best_dist=None, second_dist=None, proj=None, proj_xr=None, depth=None, view_cos=None, level=None, reject=None):
        """rfe_search_local_points_dev: every array a DevBuf (or a raw device address / torch tensor); asynchronous on the ctx stream,
        outputs land in assign [Nf], stats [8] and the optional per-map-point arrays."""
        a = _dev
        self._chk(lib.rfe_search_local_points_dev(self.h, C.byref(params), a(q), a(pw), a(normal), a(min_dist), a(max_dist), a(scale_dist), a(valid),
                                                  a(observed), Np, a(f), a(kpts), a(kxy), a(octave), a(skip), Nf, a(nf_dev), float(th_high),
                                                  cand_cap, a(assign), a(best_idx), a(best_dist), a(second_dist), a(proj), a(proj_xr), a(depth),
                                                  a(view_cos), a(level), a(reject), a(stats)))

    def triangulate_neighbours(self, params, view1, kpts1, octave1, uright1, depth1, has_mp1, views2, kpts2, octave2, uright2, depth2, has_mp2,
                               n2, S, pairs, kpts1_raw=None, kpts2_raw=None, neighbour_valid=None, outputs=TRI_OUTPUTS):
        """LocalMapping::CreateNewMapPoints behind the matcher for all neighbours (rfe_triangulate_neighbours, host arrays).
        params: a TriParams (tri_params()); view1: a TriView, views2: a sequence of Nn of them; kpts2 [Nn,N2max,2] and the other neighbour
        arrays [Nn,N2max]; S [Nn], pairs [Nn,Kmax,2] as rfe_match_dev writes them.  outputs: the arrays to ask for (the others are passed
        as NULL).  Returns a dict: code [Nn,Kmax], x3d [Nn,Kmax,3], point_stereo [Nn,Kmax], the created points in creation order (out_n,
        out_idx1, out_idx2, out_x3d [created,3], out_stereo), matches [Nn], created, stats [8]."""
        pr = np.ascontiguousarray(pairs, np.int32)
        Nn, Kmax = pr.shape[0], pr.shape[1]
        k1 = np.ascontiguousarray(kpts1, np.float32).reshape(-1, 2)
        N1 = k1.shape[0]
        k2 = np.ascontiguousarray(kpts2, np.float32).reshape(Nn, -1, 2) if Nn else np.zeros((0, 0, 2), np.float32)
        N2max = k2.shape[1]
        v2 = (TriView * max(Nn, 1))(*views2)
        flat = lambda a, dt, n: np.ascontiguousarray(a, dt).reshape(-1)[:n] if n else np.zeros((0,), dt)   # noqa: E731
        o1, u1, d1, m1 = flat(octave1, np.int32, N1), flat(uright1, np.float32, N1), flat(depth1, np.float32, N1), flat(has_mp1, np.uint8, N1)
        f2 = Nn * N2max
        o2, u2, d2, m2 = flat(octave2, np.int32, f2), flat(uright2, np.float32, f2), flat(depth2, np.float32, f2), flat(has_mp2, np.uint8, f2)
        assert len(o1) == N1 and len(m1) == N1 and len(o2) == f2 and len(m2) == f2
        nn2, Sa = flat(n2, np.int32, Nn), flat(S, np.int32, Nn)
        r1, r2 = _opt(kpts1_raw, np.float32), _opt(kpts2_raw, np.float32)
        nv = None if neighbour_valid is None else np.ascontiguousarray(neighbour_valid, np.uint8).reshape(-1)
        n1, s1 = max(N1, 1), max(Nn * Kmax, 1)
        o = {"code": np.full((s1,), -1, np.int32), "x3d": np.zeros((s1, 3), np.float32), "point_stereo": np.zeros((s1,), np.uint8),
             "out_n": np.zeros((n1,), np.int32), "out_idx1": np.zeros((n1,), np.int32), "out_idx2": np.zeros((n1,), np.int32),
             "out_x3d": np.zeros((n1, 3), np.float32), "out_stereo": np.zeros((n1,), np.uint8), "matches": np.zeros((max(Nn, 1),), np.int32)}
        assert tuple(o) == TRI_OUTPUTS
        st = np.zeros((8,), np.int32)
        n = self._chk(lib.rfe_triangulate_neighbours(self.h, C.byref(params), C.byref(view1), _addr(k1), _addr(r1), _addr(o1), _addr(u1), _addr(d1),
                                                     _addr(m1), N1, C.cast(v2, C.c_void_p), _addr(k2), _addr(r2), _addr(o2), _addr(u2), _addr(d2),
                                                     _addr(m2), _addr(nn2), _addr(nv), Nn, N2max, _addr(Sa), _addr(pr), Kmax,
                                                     *[o[k].ctypes.data if k in outputs else None for k in o], st.ctypes.data))
        out = {"code": o["code"][:Nn * Kmax].reshape(Nn, Kmax), "x3d": o["x3d"][:Nn * Kmax].reshape(Nn, Kmax, 3),
               "point_stereo": o["point_stereo"][:Nn * Kmax].reshape(Nn, Kmax), "matches": o["matches"][:Nn]}
        out.update({k: o[k][:n] for k in ("out_n", "out_idx1", "out_idx2", "out_x3d", "out_stereo")})
        out = {k: v for k, v in out.items() if k in outputs}
        out.update(created=n, stats=st)
        return out

    def triangulate_neighbours_dev(self, params, view1, kpts1, octave1, uright1, depth1, has_mp1, N1, views2, kpts2, octave2, uright2, depth2,
                                   has_mp2, n2, Nn, N2max, S, pairs, Kmax, stats, kpts1_raw=None, kpts2_raw=None, neighbour_valid=None, code=None,
                                   x3d=None, point_stereo=None, out_n=None, out_idx1=None, out_idx2=None, out_x3d=None, out_stereo=None,
                                   matches=None):
        """rfe_triangulate_neighbours_dev: params and view1 are host structures, every array (views2 [Nn] included) a DevBuf (or a raw
        device address / torch tensor); asynchronous on the ctx stream.  The out_* arrays need room for N1 entries."""
        a = _dev
        self._chk(lib.rfe_triangulate_neighbours_dev(self.h, C.byref(params), C.byref(view1), a(kpts1), a(kpts1_raw), a(octave1), a(uright1),
                                                     a(depth1), a(has_mp1), N1, a(views2), a(kpts2), a(kpts2_raw), a(octave2), a(uright2),
                                                     a(depth2), a(has_mp2), a(n2), a(neighbour_valid), Nn, N2max, a(S), a(pairs), Kmax, a(code),
                                                     a(x3d), a(point_stereo), a(out_n), a(out_idx1), a(out_idx2), a(out_x3d), a(out_stereo),
                                                     a(matches), a(stats)))

    def pose_optimization(self, params, pose0, kpts_un, xw, has_mp, octave=None, uright=None, n=None, outlier=None, chi2=None,
                          outputs=POSE_OUTPUTS):
        """Optimizer::PoseOptimization for B problems (rfe_pose_optimization, host arrays).  params: a PoseParams
        (pose_params()); pose0 [B,7] qx qy qz qw tx ty tz; kpts_un [B,N,2], xw [B,N,3], has_mp / octave / uright [B,N], n [B] or None.
        outlier / chi2: what those arrays hold where the call does not write (default 0).  outputs: the optional arrays to ask for (the
        others are passed as NULL).  Returns a dict: pose [B,7] float64, outlier [B,N], stats [B,8], ret, and pose_f32 / chi2 / trace
        [B,4,8] as asked."""
        p0 = np.ascontiguousarray(pose0, np.float32).reshape(-1, 7)
        B = p0.shape[0]
        k = np.ascontiguousarray(kpts_un, np.float32)
        N = k.size // (2 * B) if B else 0
        k = k.reshape(B, N, 2)
        f = B * N
        x, m = _opt(xw, np.float32), _opt(has_mp, np.uint8)
        o, u, nn = _opt(octave, np.int32), _opt(uright, np.float32), _opt(n, np.int32)
        assert len(x) == f * 3 and len(m) == f and (o is None or len(o) == f) and (u is None or len(u) == f) and (nn is None or len(nn) == B)
        b1, f1 = max(B, 1), max(f, 1)
        out = np.zeros((f1,), np.uint8)
        c2 = np.zeros((f1,), np.float32)
        if outlier is not None:
            out[:f] = np.asarray(outlier, np.uint8).reshape(-1)
        if chi2 is not None:
            c2[:f] = np.asarray(chi2, np.float32).reshape(-1)
        pose, pf = np.zeros((b1, 7), np.float64), np.zeros((b1, 7), np.float32)
        tr, st = np.zeros((b1, 4, 8), np.float64), np.zeros((b1, 8), np.int32)
        opt = {"pose_f32": pf, "chi2": c2, "trace": tr}
        ret = self._chk(lib.rfe_pose_optimization(self.h, C.byref(params), _addr(p0), _addr(k), _addr(o), _addr(u), _addr(x), _addr(m), _addr(nn),
                                                  B, N, pose.ctypes.data, pf.ctypes.data if "pose_f32" in outputs else None, out.ctypes.data,
                                                  c2.ctypes.data if "chi2" in outputs else None, tr.ctypes.data if "trace" in outputs else None,
                                                  st.ctypes.data))
        r = {"pose": pose[:B], "outlier": out[:f].reshape(B, N), "stats": st[:B], "ret": ret}
        r.update({key: (a[:f].reshape(B, N) if key == "chi2" else a[:B]) for key, a in opt.items() if key in outputs})
        return r

    def pose_optimization_dev(self, params, pose0, kpts_un, xw, has_mp, B, N, pose, outlier, stats, octave=None, uright=None, n=None,
                              pose_f32=None, chi2=None, trace=None):
        """rfe_pose_optimization_dev: params is a host structure, every array a DevBuf (or a raw device address / torch tensor);
        asynchronous on the ctx stream."""
        a = _dev
        self._chk(lib.rfe_pose_optimization_dev(self.h, C.byref(params), a(pose0), a(kpts_un), a(octave), a(uright), a(xw), a(has_mp), a(n),
                                                int(B), int(N), a(pose), a(pose_f32), a(outlier), a(chi2), a(trace), a(stats)))

    def pose_inertial_optimization(self, params, mode, cam, state, prev_state, preint, cov_rw, kpts_un, xw, has_mp, track_depth, prior_in=None,
                                   rec_init=None, octave=None, uright=None, n=None, outlier=None, chi2=None, outputs=PIO_OUTPUTS):
        """Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame for B problems (rfe_pose_inertial_optimization, host arrays; DESIGN.md
        6p).  params: a PoseInertialParams (pose_inertial_params()); mode [B] PIO_LAST_KEYFRAME / PIO_LAST_FRAME; cam [B,36], state /
        prev_state [B,21], preint [B,148], cov_rw [B,18] float32; prior_in [B,246] float64 or None; kpts_un [B,N,2], xw [B,N,3], has_mp /
        track_depth / octave / uright [B,N]; rec_init / n [B] or None.  outlier / chi2: what those arrays hold where the call does not write
        (default 0).  outputs: the optional arrays to ask for (the others are passed as NULL).  Returns a dict: state [B,21] float64,
        outlier [B,N], stats [B,16], ret, and state_f32 / chi2 / prior_out [B,246] / trace [B,4,8] as asked."""
        md = np.ascontiguousarray(mode, np.int32).reshape(-1)
        B = md.size
        k = np.ascontiguousarray(kpts_un, np.float32)
        N = k.size // (2 * B) if B else 0
        f = B * N
        cm, st, ps, pr, cv = (_opt(v, np.float32) for v in (cam, state, prev_state, preint, cov_rw))
        assert len(cm) == B * PIO_CAM_FLOATS and len(st) == len(ps) == B * PIO_STATE_FLOATS and len(pr) == B * PIO_PREINT_FLOATS
        assert len(cv) == B * PIO_COV_RW_FLOATS
        pin, rc = _opt(prior_in, np.float64), _opt(rec_init, np.int32)
        x, m, td = _opt(xw, np.float32), _opt(has_mp, np.uint8), _opt(track_depth, np.float32)
        o, u, nn = _opt(octave, np.int32), _opt(uright, np.float32), _opt(n, np.int32)
        assert len(x) == f * 3 and len(m) == f and len(td) == f and (o is None or len(o) == f) and (u is None or len(u) == f)
        assert (nn is None or len(nn) == B) and (rc is None or len(rc) == B) and (pin is None or len(pin) == B * PIO_PRIOR_DOUBLES)
        b1, f1 = max(B, 1), max(f, 1)
        out = np.zeros((f1,), np.uint8)
        c2 = np.zeros((f1,), np.float32)
        if outlier is not None:
            out[:f] = np.asarray(outlier, np.uint8).reshape(-1)
        if chi2 is not None:
            c2[:f] = np.asarray(chi2, np.float32).reshape(-1)
        so, sf = np.zeros((b1, PIO_STATE_FLOATS), np.float64), np.zeros((b1, PIO_STATE_FLOATS), np.float32)
        po, tr, sts = np.zeros((b1, PIO_PRIOR_DOUBLES), np.float64), np.zeros((b1, 4, 8), np.float64), np.zeros((b1, 16), np.int32)
        opt = {"state_f32": sf, "chi2": c2, "prior_out": po, "trace": tr}
        want = {key: (a.ctypes.data if key in outputs else None) for key, a in opt.items()}
        ret = self._chk(lib.rfe_pose_inertial_optimization(self.h, C.byref(params), _addr(md), _addr(rc), _addr(cm), _addr(st), _addr(ps), _addr(pr),
                                                           _addr(cv), _addr(pin), _addr(k), _addr(o), _addr(u), _addr(x), _addr(m), _addr(td),
                                                           _addr(nn), B, N, so.ctypes.data, want["state_f32"], out.ctypes.data, want["chi2"],
                                                           want["prior_out"], want["trace"], sts.ctypes.data))
        r = {"state": so[:B], "outlier": out[:f].reshape(B, N), "stats": sts[:B], "ret": ret}
        r.update({key: (a[:f].reshape(B, N) if key == "chi2" else a[:B]) for key, a in opt.items() if key in outputs})
        return r

    def pose_inertial_optimization_dev(self, params, mode, cam, state, prev_state, preint, cov_rw, kpts_un, xw, has_mp, track_depth, B, N,
                                       state_out, outlier, stats, prior_in=None, rec_init=None, octave=None, uright=None, n=None,
                                       state_f32=None, chi2=None, prior_out=None, trace=None):
        """rfe_pose_inertial_optimization_dev: params is a host structure, every array a DevBuf (or a raw device address / torch tensor);
        asynchronous on the ctx stream."""
        a = _dev
        self._chk(lib.rfe_pose_inertial_optimization_dev(self.h, C.byref(params), a(mode), a(rec_init), a(cam), a(state), a(prev_state),
                                                         a(preint), a(cov_rw), a(prior_in), a(kpts_un), a(octave), a(uright), a(xw), a(has_mp),
                                                         a(track_depth), a(n), int(B), int(N), a(state_out), a(state_f32), a(outlier), a(chi2),
                                                         a(prior_out), a(trace), a(stats)))

    def k_pose_inertial_classify(self, params, mode, rnd, view, kpts_un, xw, track_depth, outlier_in, chi2_in, octave=None, uright=None):
        """rfe_k_pose_inertial_classify: the float classification behind round rnd (0..3) or the recovery pass (4) of n edges at the camera
        pose view [12] -> code [n], chi2 [n]"""
        v = np.ascontiguousarray(view, np.float64).reshape(12)
        k, x, td = (_opt(a, np.float32) for a in (kpts_un, xw, track_depth))
        oi, ci = _opt(outlier_in, np.uint8), _opt(chi2_in, np.float32)
        o, u = _opt(octave, np.int32), _opt(uright, np.float32)
        n = len(td)
        code, c2 = np.zeros(n, np.uint8), np.zeros(n, np.float32)
        self._chk(lib.rfe_k_pose_inertial_classify(self.h, C.byref(params), int(mode), int(rnd), v.ctypes.data, _addr(k), _addr(o), _addr(u), _addr(x),
                                                   _addr(td), _addr(oi), _addr(ci), n, code.ctypes.data, c2.ctypes.data))
        return code, c2

    def sim3_ransac(self, problems, xw1, xw2, sigma2_1, sigma2_2, draws, fill=None, outputs=SIM3_RANSAC_OUTPUTS):
        """Sim3Solver's RANSAC for B problems (rfe_sim3_ransac, host arrays).  problems: B dicts (sim3_solver_params()) or the
        ctypes array; xw1 / xw2 [B,N,3], sigma2_1 / sigma2_2 [B,N], draws [B,H,3].  fill: what inliers / best_inliers [B,N], counts [B,H] and
        hyps [B,H,32] hold where the call does not write (default 0).  outputs: the optional arrays to ask for.  Returns a dict: T12 [B,16],
        stats [B,8], ret and the optional arrays."""
        P = problems if isinstance(problems, C.Array) else sim3_solver_params(problems)
        B = len(problems)
        d = np.ascontiguousarray(draws, np.int32)
        H = d.size // (3 * B) if B else 1
        x1, x2 = np.ascontiguousarray(xw1, np.float32), np.ascontiguousarray(xw2, np.float32)
        N = x1.size // (3 * B) if B else 0
        g1, g2 = np.ascontiguousarray(sigma2_1, np.float32), np.ascontiguousarray(sigma2_2, np.float32)
        assert x2.size == x1.size == B * N * 3 and g1.size == g2.size == B * N and d.size == B * H * 3
        b1 = max(B, 1)
        shape = {"T12": (b1, 16), "R": (b1, 9), "t": (b1, 3), "s": (b1,), "inliers": (b1, max(N, 1)), "best_inliers": (b1, max(N, 1)),
                 "counts": (b1, H), "hyps": (b1, H, 32), "stats": (b1, 8)}
        dt = {"inliers": np.uint8, "best_inliers": np.uint8, "counts": np.int32, "stats": np.int32}
        o = {k: np.zeros(shape[k], dt.get(k, np.float32)) for k in shape}
        for k, v in (fill or {}).items():
            o[k][:B, :np.asarray(v).shape[1]] = v
        arg = lambda k: o[k].ctypes.data if k in outputs else None   # noqa: E731
        ret = self._chk(lib.rfe_sim3_ransac(self.h, C.addressof(P), _addr(x1), _addr(x2), _addr(g1), _addr(g2), _addr(d), B, N, H,
                                            o["T12"].ctypes.data, arg("R"), arg("t"), arg("s"), arg("inliers"), arg("best_inliers"), arg("counts"),
                                            arg("hyps"), o["stats"].ctypes.data))
        r = {k: (o[k][:B, :N] if k in ("inliers", "best_inliers") else o[k][:B]) for k in ("T12", "stats") + tuple(outputs)}
        r["ret"] = ret
        return r

    def sim3_ransac_dev(self, problems, xw1, xw2, sigma2_1, sigma2_2, draws, B, N, H, T12, stats, R=None, t=None, s=None, inliers=None,
                        best_inliers=None, counts=None, hyps=None):
        """rfe_sim3_ransac_dev: problems is a HOST array (sim3_solver_params()), every other array a DevBuf (or a raw device address / torch
        tensor); asynchronous on the ctx stream."""
        a = _dev
        P = problems if isinstance(problems, C.Array) else sim3_solver_params(problems)
        self._chk(lib.rfe_sim3_ransac_dev(self.h, C.addressof(P), a(xw1), a(xw2), a(sigma2_1), a(sigma2_2), a(draws), int(B), int(N), int(H),
                                          a(T12), a(R), a(t), a(s), a(inliers), a(best_inliers), a(counts), a(hyps), a(stats)))

    def two_view(self, problems, kpts1, kpts2, S, pairs, draws, fill=None, outputs=TWO_VIEW_OUTPUTS):
        """TwoViewReconstruction for B problems (rfe_two_view, host arrays).  problems: B dicts (two_view_params()) or the
        ctypes array with B given by S; kpts1 [B,N1max,2], kpts2 [B,N2max,2], S [B], pairs [B,Kmax,2], draws [B,H,8].  fill: what the
        optional arrays hold where the call does not write (default 0).  outputs: the optional arrays to ask for (the others are passed
        as NULL).  Returns a dict: R21 [B,9], t21 [B,3], stats [B,16], ret and the optional arrays."""
        s = np.ascontiguousarray(S, np.int32).reshape(-1)
        B = len(s)
        P = problems if isinstance(problems, C.Array) else two_view_params(problems)
        assert len(P) >= B
        k1, k2 = np.ascontiguousarray(kpts1, np.float32), np.ascontiguousarray(kpts2, np.float32)
        pr, d = np.ascontiguousarray(pairs, np.int32), np.ascontiguousarray(draws, np.int32)
        N1, N2, K = (a.size // (2 * B) if B else 0 for a in (k1, k2, pr))
        H = d.size // (8 * B) if B else 1
        assert k1.size == B * N1 * 2 and k2.size == B * N2 * 2 and pr.size == B * K * 2 and d.size == B * H * 8
        b1 = max(B, 1)
        shape = {"R21": (b1, 9), "t21": (b1, 3), "p3d": (b1, max(N1, 1), 3), "triangulated": (b1, max(N1, 1)), "inliers_h": (b1, max(K, 1)),
                 "inliers_f": (b1, max(K, 1)), "scores": (b1, H, 2), "models": (b1, 2, 9), "cand": (b1, 8, 16), "stats": (b1, 16)}
        dt = {"triangulated": np.uint8, "inliers_h": np.uint8, "inliers_f": np.uint8, "stats": np.int32}
        o = {k: np.zeros(shape[k], dt.get(k, np.float32)) for k in shape}
        for k, v in (fill or {}).items():
            v = np.asarray(v)
            o[k][:B, :v.shape[1]] = v
        arg = lambda k: o[k].ctypes.data if k in outputs else None   # noqa: E731
        ret = self._chk(lib.rfe_two_view(self.h, C.addressof(P), _addr(k1), _addr(k2), _addr(s), _addr(pr), _addr(d), B, N1, N2, K, H,
                                         o["R21"].ctypes.data, o["t21"].ctypes.data, *(arg(k) for k in TWO_VIEW_OUTPUTS), o["stats"].ctypes.data))
        cut = {"p3d": N1, "triangulated": N1, "inliers_h": K, "inliers_f": K}
        r = {k: (o[k][:B, :cut[k]] if k in cut else o[k][:B]) for k in ("R21", "t21", "stats") + tuple(outputs)}
        r["ret"] = ret
        return r

    def two_view_dev(self, problems, kpts1, kpts2, S, pairs, draws, B, N1max, N2max, Kmax, H, R21, t21, stats, p3d=None, triangulated=None,
                     inliers_h=None, inliers_f=None, scores=None, models=None, cand=None):
        """rfe_two_view_dev: problems is a HOST array (two_view_params()), every other array a DevBuf (or a raw device address / torch
        tensor); asynchronous on the ctx stream."""
        a = _dev
        P = problems if isinstance(problems, C.Array) else two_view_params(problems)
        self._chk(lib.rfe_two_view_dev(self.h, C.addressof(P), a(kpts1), a(kpts2), a(S), a(pairs), a(draws), int(B), int(N1max), int(N2max),
                                       int(Kmax), int(H), a(R21), a(t21), a(p3d), a(triangulated), a(inliers_h), a(inliers_f), a(scores),
                                       a(models), a(cand), a(stats)))

    def k_two_view_check(self, model, M, pts, sigma=1.0):
        """rfe_k_two_view_check: CheckHomography (model 0) / CheckFundamental (1) of ONE model M [9] over pts [n,4] -> contrib [n], inl [n]"""
        M, pts = np.ascontiguousarray(M, np.float32).reshape(9), np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        n = len(pts)
        contrib, inl = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint8)
        self._chk(lib.rfe_k_two_view_check(self.h, int(model), _addr(M), float(sigma), _addr(pts), n, contrib.ctypes.data, inl.ctypes.data))
        return contrib[:n], inl[:n]

    def k_two_view_check_rt(self, R, t, K4, th2, pts):
        """rfe_k_two_view_check_rt: CheckRT of ONE (R, t) over pts [n,4] -> code [n], cosParallax [n], p3d [n,3]"""
        Rt = np.concatenate([np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3)])
        K4, pts = np.ascontiguousarray(K4, np.float32).reshape(4), np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        n = len(pts)
        code, cosp, p3d = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 3), np.float32)
        self._chk(lib.rfe_k_two_view_check_rt(self.h, _addr(Rt), _addr(K4), float(th2), _addr(pts), n, code.ctypes.data, cosp.ctypes.data,
                                              p3d.ctypes.data))
        return code[:n], cosp[:n], p3d[:n]

    def optimize_sim3(self, problems, s12_0, xw1, xw2, valid, kpts1, idx2, kpts2, octave1=None, octave2=None, keep=None, chi2=None,
                      outputs=OPTIMIZE_SIM3_OUTPUTS):
        """Optimizer::OptimizeSim3 for B problems (rfe_optimize_sim3, host arrays).  problems: B dicts
        (optimize_sim3_params()) or the ctypes array; s12_0 [B,8] float64 qx qy qz qw tx ty tz s; xw1 / xw2 [B,N,3], valid / octave1 / idx2
        [B,N], kpts1 [B,N,2], kpts2 [B,N2,2], octave2 [B,N2].  keep / chi2: what those arrays hold where the call does not write (default 1 /
        0).  outputs: the optional arrays to ask for (the others are passed as NULL).  Returns a dict: s12 [B,8] float64, keep [B,N], stats
        [B,8], ret, and s12_f32 / chi2 [B,N,2] / trace [B,2,8] as asked."""
        P = problems if isinstance(problems, C.Array) else optimize_sim3_params(problems)
        s0 = np.ascontiguousarray(s12_0, np.float64).reshape(-1, 8)
        B = s0.shape[0]                            # not len(problems): a prepared array of no problems still has one element
        assert len(P) >= B
        v = np.ascontiguousarray(valid, np.uint8)
        N = v.size // B if B else 0
        k2 = np.ascontiguousarray(kpts2, np.float32)
        N2 = k2.size // (2 * B) if B else 0
        f, g = B * N, B * N2
        x1, x2, k1, i2 = _opt(xw1, np.float32), _opt(xw2, np.float32), _opt(kpts1, np.float32), _opt(idx2, np.int32)
        o1, o2 = _opt(octave1, np.int32), _opt(octave2, np.int32)
        assert len(x1) == len(x2) == f * 3 and len(k1) == f * 2 and len(i2) == f
        assert (o1 is None or len(o1) == f) and (o2 is None or len(o2) == g)
        b1, f1 = max(B, 1), max(f, 1)
        kp = np.ones((f1,), np.uint8)
        c2 = np.zeros((f1, 2), np.float64)
        if keep is not None:
            kp[:f] = np.asarray(keep, np.uint8).reshape(-1)
        if chi2 is not None:
            c2[:f] = np.asarray(chi2, np.float64).reshape(-1, 2)
        s12, sf = np.zeros((b1, 8), np.float64), np.zeros((b1, 8), np.float32)
        tr, st = np.zeros((b1, 2, 8), np.float64), np.zeros((b1, 8), np.int32)
        opt = {"s12_f32": sf, "chi2": c2, "trace": tr}
        ret = self._chk(lib.rfe_optimize_sim3(self.h, C.addressof(P), s0.ctypes.data, _addr(x1), _addr(x2), _addr(v.reshape(-1)), _addr(k1),
                                              _addr(o1), _addr(i2), _addr(k2.reshape(-1)) if g else None, _addr(o2), B, N, N2, s12.ctypes.data,
                                              sf.ctypes.data if "s12_f32" in outputs else None, kp.ctypes.data,
                                              c2.ctypes.data if "chi2" in outputs else None, tr.ctypes.data if "trace" in outputs else None,
                                              st.ctypes.data))
        r = {"s12": s12[:B], "keep": kp[:f].reshape(B, N), "stats": st[:B], "ret": ret}
        r.update({key: (a[:f].reshape(B, N, 2) if key == "chi2" else a[:B]) for key, a in opt.items() if key in outputs})
        return r

    def optimize_sim3_dev(self, problems, s12_0, xw1, xw2, valid, kpts1, idx2, kpts2, B, N, N2, s12, keep, stats, octave1=None, octave2=None,
                          s12_f32=None, chi2=None, trace=None):
        """rfe_optimize_sim3_dev: problems is a HOST array (optimize_sim3_params()), every other array a DevBuf (or a raw device address /
        torch tensor); asynchronous on the ctx stream."""
        a = _dev
        P = problems if isinstance(problems, C.Array) else optimize_sim3_params(problems)
        self._chk(lib.rfe_optimize_sim3_dev(self.h, C.addressof(P), a(s12_0), a(xw1), a(xw2), a(valid), a(kpts1), a(octave1), a(idx2), a(kpts2),
                                            a(octave2), int(B), int(N), int(N2), a(s12), a(s12_f32), a(keep), a(chi2), a(trace), a(stats)))

    def local_ba(self, params, P, F, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, kpts, xw, edge_point, edge_kf, edge_feat, octave=None,
                 uright=None, outputs=LOCAL_BA_OUTPUTS, shape=None):
        """Optimizer::LocalBundleAdjustment for one problem (rfe_local_ba, host arrays).  params: local_ba_params(); P free
        keyframes first, then F fixed; kf_pose [K,7], kf_cam [K,5], kf_nlevels [K], kf_sigma2 [K,16], kf_feat_off [K+1]; kpts [Nf,2], octave /
        uright [Nf]; xw [L,3]; edge_point / edge_kf / edge_feat [E].  shape: (L, E, Nf) when the arrays are longer than the problem (what
        lies behind is not read).  outputs: the optional arrays to ask for.  Returns a dict: pose [P,7] and point [L,3] float64, erase [E],
        stats [8], ret, and pose_f32 / point_f32 / chi2 [E] / trace [iterations,4] as asked."""
        kp, kc, ks = _opt(kf_pose, np.float32), _opt(kf_cam, np.float32), _opt(kf_sigma2, np.float32)
        nl, fo = _opt(kf_nlevels, np.int32), _opt(kf_feat_off, np.int32)
        k, x = _opt(kpts, np.float32), _opt(xw, np.float32)
        ep, ek, ef = _opt(edge_point, np.int32), _opt(edge_kf, np.int32), _opt(edge_feat, np.int32)
        oc, ur = _opt(octave, np.int32), _opt(uright, np.float32)
        L, E, Nf = (len(x) // 3, len(ep), len(k) // 2) if shape is None else shape
        its = max(int(params.iterations), 0)
        o = {"pose": np.zeros((max(P, 1), 7), np.float64), "pose_f32": np.zeros((max(P, 1), 7), np.float32),
             "point": np.zeros((max(L, 1), 3), np.float64), "point_f32": np.zeros((max(L, 1), 3), np.float32),
             "erase": np.zeros((max(E, 1),), np.uint8), "chi2": np.zeros((max(E, 1),), np.float64),
             "trace": np.zeros((max(its, 1), 4), np.float64), "stats": np.zeros((8,), np.int32)}
        ad = [o[n].ctypes.data if (n not in LOCAL_BA_OUTPUTS or n in outputs) else None for n in o]
        ret = self._chk(lib.rfe_local_ba(self.h, params, _addr(kp), _addr(kc), _addr(nl), _addr(ks), _addr(fo), _addr(k), _addr(oc), _addr(ur),
                                         _addr(x), _addr(ep), _addr(ek), _addr(ef), int(P), int(F), int(L), int(E), int(Nf), *ad))
        n = {"pose": P, "pose_f32": P, "point": L, "point_f32": L, "erase": E, "chi2": E, "trace": its, "stats": 8}
        r = {key: a[:n[key]] for key, a in o.items() if key not in LOCAL_BA_OUTPUTS or key in outputs}
        r["ret"] = ret
        return r

    def local_ba_dev(self, params, P, F, L, E, Nf, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, kpts, xw, edge_point, edge_kf, edge_feat,
                     pose, point, erase, stats, octave=None, uright=None, pose_f32=None, point_f32=None, chi2=None, trace=None):
        """rfe_local_ba_dev: every array a DevBuf (or a raw device address / torch tensor).  SYNCHRONOUS: returns the number of erased
        edges when the optimisation has finished."""
        a = _dev
        return self._chk(lib.rfe_local_ba_dev(self.h, params, a(kf_pose), a(kf_cam), a(kf_nlevels), a(kf_sigma2), a(kf_feat_off), a(kpts), a(octave),
                                              a(uright), a(xw), a(edge_point), a(edge_kf), a(edge_feat), int(P), int(F), int(L), int(E), int(Nf),
                                              a(pose), a(pose_f32), a(point), a(point_f32), a(erase), a(chi2), a(trace), a(stats)))

    def essential_graph(self, params, s_est, s_meas, fixed, edge_i, edge_j, edge_from_est, xw=None, point_ref=None,
                        outputs=ESSENTIAL_GRAPH_OUTPUTS, shape=None):
        """Optimizer::OptimizeEssentialGraph for one pose graph (rfe_essential_graph, host arrays).  params:
        essential_graph_params(); s_est / s_meas [N,8] float64 (q xyzw, t, s), fixed [N]; edge_i / edge_j / edge_from_est [E] in ascending
        (i, j); xw [L,3] float32 with point_ref [L].  shape: (N, E, L) when the arrays are longer than the problem (what lies behind is
        not read).  Returns a dict: siw [N,8], xw_out [L,3], stats [8], ret (LM iterations run), and tiw_f32 [N,7] / swi [N,8] / chi2 [E] /
        trace [iterations,4] as asked."""
        se, sm, fx = _opt(s_est, np.float64), _opt(s_meas, np.float64), _opt(fixed, np.uint8)
        ei, ej, es = _opt(edge_i, np.int32), _opt(edge_j, np.int32), _opt(edge_from_est, np.uint8)
        x, pr = _opt(xw, np.float32), _opt(point_ref, np.int32)
        N, E, L = (len(fx), len(ei), 0 if pr is None else len(pr)) if shape is None else shape
        its = max(int(params.iterations), 0)
        o = {"siw": np.zeros((max(N, 1), 8), np.float64), "tiw_f32": np.zeros((max(N, 1), 7), np.float32),
             "swi": np.zeros((max(N, 1), 8), np.float64), "xw_out": np.zeros((max(L, 1), 3), np.float32),
             "chi2": np.zeros((max(E, 1),), np.float64), "trace": np.zeros((max(its, 1), 4), np.float64), "stats": np.zeros((8,), np.int32)}
        ad = [o[n].ctypes.data if (n not in ESSENTIAL_GRAPH_OUTPUTS or n in outputs) else None for n in o]
        ret = self._chk(lib.rfe_essential_graph(self.h, params, _addr(se), _addr(sm), _addr(fx), _addr(ei), _addr(ej), _addr(es), _addr(x),
                                                _addr(pr), int(N), int(E), int(L), *ad))
        n = {"siw": N, "tiw_f32": N, "swi": N, "xw_out": L, "chi2": E, "trace": its, "stats": 8}
        r = {key: a[:n[key]] for key, a in o.items() if key not in ESSENTIAL_GRAPH_OUTPUTS or key in outputs}
        r["ret"] = ret
        return r

    def essential_graph_dev(self, params, N, E, L, s_est, s_meas, fixed, edge_i, edge_j, edge_from_est, xw, point_ref, siw, xw_out, stats,
                            tiw_f32=None, swi=None, chi2=None, trace=None):
        """rfe_essential_graph_dev: every array a DevBuf (or a raw device address / torch tensor).  SYNCHRONOUS: returns the number of LM
        iterations run when the optimisation has finished."""
        a = _dev
        return self._chk(lib.rfe_essential_graph_dev(self.h, params, a(s_est), a(s_meas), a(fixed), a(edge_i), a(edge_j), a(edge_from_est),
                                                     a(xw), a(point_ref), int(N), int(E), int(L), a(siw), a(tiw_f32), a(swi), a(xw_out),
                                                     a(chi2), a(trace), a(stats)))

    def global_ba(self, params, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, fixed, kpts, xw, edge_point, edge_kf, edge_feat, octave=None,
                  uright=None, outputs=GLOBAL_BA_OUTPUTS, shape=None):
        """Optimizer::GlobalBundleAdjustemnt for one problem (rfe_global_ba, host arrays).  params: global_ba_params();
        kf_pose [K,7], kf_cam [K,5], kf_nlevels [K], kf_sigma2 [K,16], kf_feat_off [K+1], fixed [K]; kpts [Nf,2], octave / uright [Nf];
        xw [L,3]; edge_point / edge_kf / edge_feat [E].  shape: (L, E, Nf) when the arrays are longer than the problem (what lies behind is
        not read).  outputs: the optional arrays to ask for.  Returns a dict: pose [K,7] and point [L,3] float64, included [L], stats [8],
        ret (LM iterations run), and pose_f32 / point_f32 / chi2 [E] / trace [iterations,4] as asked."""
        kp, kc, ks = _opt(kf_pose, np.float32), _opt(kf_cam, np.float32), _opt(kf_sigma2, np.float32)
        nl, fo, fx = _opt(kf_nlevels, np.int32), _opt(kf_feat_off, np.int32), _opt(fixed, np.uint8)
        k, x = _opt(kpts, np.float32), _opt(xw, np.float32)
        ep, ek, ef = _opt(edge_point, np.int32), _opt(edge_kf, np.int32), _opt(edge_feat, np.int32)
        oc, ur = _opt(octave, np.int32), _opt(uright, np.float32)
        K = 0 if fx is None else len(fx)
        L, E, Nf = (len(x) // 3, len(ep), len(k) // 2) if shape is None else shape
        its = max(int(params.iterations), 0)
        o = {"pose": np.zeros((max(K, 1), 7), np.float64), "pose_f32": np.zeros((max(K, 1), 7), np.float32),
             "point": np.zeros((max(L, 1), 3), np.float64), "point_f32": np.zeros((max(L, 1), 3), np.float32),
             "included": np.zeros((max(L, 1),), np.uint8), "chi2": np.zeros((max(E, 1),), np.float64),
             "trace": np.zeros((max(its, 1), 4), np.float64), "stats": np.zeros((8,), np.int32)}
        ad = [o[n].ctypes.data if (n not in GLOBAL_BA_OUTPUTS or n in outputs) else None for n in o]
        ret = self._chk(lib.rfe_global_ba(self.h, params, _addr(kp), _addr(kc), _addr(nl), _addr(ks), _addr(fo), _addr(fx), _addr(k), _addr(oc),
                                          _addr(ur), _addr(x), _addr(ep), _addr(ek), _addr(ef), int(K), int(L), int(E), int(Nf), *ad))
        n = {"pose": K, "pose_f32": K, "point": L, "point_f32": L, "included": L, "chi2": E, "trace": its, "stats": 8}
        r = {key: a[:n[key]] for key, a in o.items() if key not in GLOBAL_BA_OUTPUTS or key in outputs}
        r["ret"] = ret
        return r

    def global_ba_dev(self, params, K, L, E, Nf, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, fixed, kpts, xw, edge_point, edge_kf,
                      edge_feat, pose, point, included, stats, octave=None, uright=None, pose_f32=None, point_f32=None, chi2=None, trace=None):
        """rfe_global_ba_dev: every array a DevBuf (or a raw device address / torch tensor).  SYNCHRONOUS: returns the number of LM
        iterations run when the optimisation has finished."""
        a = _dev
        return self._chk(lib.rfe_global_ba_dev(self.h, params, a(kf_pose), a(kf_cam), a(kf_nlevels), a(kf_sigma2), a(kf_feat_off), a(fixed), a(kpts),
                                               a(octave), a(uright), a(xw), a(edge_point), a(edge_kf), a(edge_feat), int(K), int(L), int(E), int(Nf),
                                               a(pose), a(pose_f32), a(point), a(point_f32), a(included), a(chi2), a(trace), a(stats)))

    def bow_transform(self, vocab, desc, levelsup=0):
        """Frame::ComputeBoW3 behind binarize_descriptors (rfe_bow_transform, host arrays).  desc: float32 [N,256] SuperPoint
        descriptors (binarised by the call) or uint8 [N,D] bytes.  Returns a dict: word / node / weight [N] per feature, bow_word / bow_value
        [bow_n], fv_node [fv_n], fv_offsets [fv_n + 1], fv_feat [fv_offsets[-1]]."""
        d = np.asarray(desc)
        assert d.dtype in (np.float32, np.uint8) and d.ndim == 2
        d = np.ascontiguousarray(d)
        N, n1 = d.shape[0], max(d.shape[0], 1)
        f32 = d.ctypes.data if d.dtype == np.float32 else None
        u8 = d.ctypes.data if d.dtype == np.uint8 else None
        o = {"word": np.zeros((n1,), np.int32), "node": np.zeros((n1,), np.int32), "weight": np.zeros((n1,), np.float64),
             "bow_n": np.zeros((1,), np.int32), "bow_word": np.zeros((n1,), np.int32), "bow_value": np.zeros((n1,), np.float64),
             "fv_n": np.zeros((1,), np.int32), "fv_node": np.zeros((n1,), np.int32), "fv_offsets": np.zeros((n1 + 1,), np.int32),
             "fv_feat": np.zeros((n1,), np.int32)}
        self._chk(lib.rfe_bow_transform(self.h, vocab.h, f32, u8, N, int(levelsup), *[a.ctypes.data for a in o.values()]))
        nb, nf = int(o["bow_n"][0]), int(o["fv_n"][0])
        return {"word": o["word"][:N], "node": o["node"][:N], "weight": o["weight"][:N], "bow_word": o["bow_word"][:nb],
                "bow_value": o["bow_value"][:nb], "fv_node": o["fv_node"][:nf], "fv_offsets": o["fv_offsets"][:nf + 1],
                "fv_feat": o["fv_feat"][:int(o["fv_offsets"][nf])]}

    def bow_transform_dev(self, vocab, N, levelsup, bow_n, bow_word, bow_value, fv_n, fv_node, fv_offsets, fv_feat, desc_f32=None, desc_u8=None,
                          word=None, node=None, weight=None):
        """rfe_bow_transform_dev: every array a DevBuf (or a raw device address / torch tensor); asynchronous on the ctx stream."""
        a = _dev
        self._chk(lib.rfe_bow_transform_dev(self.h, vocab.h, a(desc_f32), a(desc_u8), int(N), int(levelsup), a(word), a(node), a(weight), a(bow_n),
                                            a(bow_word), a(bow_value), a(fv_n), a(fv_node), a(fv_offsets), a(fv_feat)))

    def distinctive_descriptors(self, desc, offsets):
        """MapPoint::ComputeDistinctiveDescriptors for many map points (MapPoint.cc:438-530)."""
        da = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
        off = np.ascontiguousarray(offsets, np.int32)
        Np = off.shape[0] - 1
        b = np.empty((max(Np, 1),), np.int32); m = np.empty((max(Np, 1),), np.float32)
        self._chk(lib.rfe_distinctive_descriptors(self.h, da.ctypes.data, off.ctypes.data, Np, b.ctypes.data, m.ctypes.data))
        return b[:Np], m[:Np]

    # ---- profiling
    def profile(self, on=True):
        self._chk(lib.rfe_profile_enable(self.h, int(on)))

    def profile_filter(self, stage=None):
        """Record events for one stage only (None = all stages)."""
        self._chk(lib.rfe_profile_filter(self.h, stage.encode() if stage else None))

    def profile_reset(self):
        self._chk(lib.rfe_profile_reset(self.h))

    def profile_read(self):
        names = C.create_string_buffer(4096)
        ms = (C.c_double * 64)()
        calls = (C.c_int64 * 64)()
        k = self._chk(lib.rfe_profile_read(self.h, names, 4096, ms, calls, 64))
        nm = names.value.decode().split(";") if k else []
        return {nm[i]: (ms[i], calls[i]) for i in range(k)}
