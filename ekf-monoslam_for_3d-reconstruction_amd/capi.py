"""ctypes binding of include/ekf_monoslam.h (one prototype per declared entry point)."""
from __future__ import annotations

import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EKF_LIB_PATH") or os.path.join(HERE, "lib", "libekfslam_hip.so")   # (EKF_LIB_PATH: an A/B build, tools/ only)
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "ekf_monoslam.h")

EKF_F32, EKF_F64 = 0, 1
EKF_OPT_PROPAGATE_STREAMING, EKF_OPT_USE_MFMA, EKF_OPT_PROFILE, EKF_OPT_PIPELINE = 0, 1, 2, 3
EKF_OPT_SPLIT_BF16, EKF_OPT_FEATURE_NOISE, EKF_OPT_FUSED_LAUNCHES, EKF_OPT_W_RECOMPUTE = 4, 5, 6, 7
EKF_KF_NONE, EKF_KF_CANDIDATE, EKF_KF_EMIT_CURRENT, EKF_KF_EMIT_CANDIDATE, EKF_KF_EMIT_FIRST = 0, 1, 2, 3, 4
EKF_KF_OPT_KEEP_CURRENT_PROJECTIONS = 0
STATUS_NAMES = {0: "EKF_OK", 1: "EKF_ERR_ARG", 2: "EKF_ERR_CAPACITY", 3: "EKF_ERR_DEVICE",
                4: "EKF_ERR_STATE", 5: "EKF_ERR_NUMERIC", 6: "EKF_ERR_UNSUPPORTED"}


class EkfError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class EkfConfig(C.Structure):
    """struct ekf_config (ConfigVSLAM.h:23-48 + camModel.hpp:9-11 + frame size)."""
    _fields_ = [
        ("sigma_vx", C.c_float), ("sigma_vy", C.c_float), ("sigma_vz", C.c_float),
        ("sigma_wx", C.c_float), ("sigma_wy", C.c_float), ("sigma_wz", C.c_float),
        ("rho_0", C.c_float), ("sigma_rho_0", C.c_float),
        ("window_size", C.c_int), ("sigma_pixel", C.c_int), ("kernel_size", C.c_int),
        ("sigma_size", C.c_int), ("scale", C.c_int),
        ("T_camera", C.c_float),
        ("nInitFeatures", C.c_int), ("min_features", C.c_int), ("max_features", C.c_int),
        ("forsePlane", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("u0", C.c_float), ("v0", C.c_float),
        ("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float), ("p1", C.c_float), ("p2", C.c_float),
        ("image_width", C.c_int), ("image_height", C.c_int),
    ]


class EkfSbaCamera(C.Structure):
    """ekf_sba_camera: the pinhole K = (fx, fy, cx, cy)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


def declared_symbols(header_path: str = HEADER_PATH):
    """Names of every function the header declares (used by the ABI export test)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ekf_[a-z0-9_]+)\s*\(", text)))


_P = C.c_void_p
_PROTOS = {
    "ekf_config_default": (None, [C.POINTER(EkfConfig)]),
    "ekf_abi_version": (C.c_int, []),
    "ekf_create": (C.c_int, [C.POINTER(EkfConfig), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "ekf_destroy": (None, [_P]),
    "ekf_last_error": (C.c_char_p, [_P]),
    "ekf_set_dt": (C.c_int, [_P, C.c_double]),
    "ekf_get_dt": (C.c_double, [_P]),
    "ekf_set_stream": (C.c_int, [_P, _P]),
    "ekf_set_option": (C.c_int, [_P, C.c_int, C.c_int]),
    "ekf_synchronize": (C.c_int, [_P]),
    "ekf_add_feature": (C.c_int, [_P, C.c_double, C.c_double]),
    "ekf_remove_feature": (C.c_int, [_P, C.c_int]),
    "ekf_remove_features": (C.c_int, [_P, _P, C.c_int]),
    "ekf_predict": (C.c_int, [_P, _P, _P, C.c_int]),
    "ekf_measure": (C.c_int, [_P]),
    "ekf_get_motion_jacobian": (C.c_int, [_P, _P, _P]),
    "ekf_get_predictions": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "ekf_update": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "ekf_update_device": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "ekf_rescue_high_innovation": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_double, _P]),
    "ekf_set_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "ekf_set_frame_raw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ekf_set_frame_raw_device": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ekf_get_frame": (C.c_int, [_P, _P, C.c_int]),
    "ekf_set_patch": (C.c_int, [_P, C.c_int, _P]),
    "ekf_get_patch": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ekf_get_blur_predictions": (C.c_int, [_P, _P]),
    "ekf_find_matches": (C.c_int, [_P, C.c_double, _P, _P, _P]),
    "ekf_export_points": (C.c_int, [_P, _P, C.c_int]),
    "ekf_export_points_table": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "ekf_get_feature_ids": (C.c_int, [_P, _P, _P]),
    "ekf_set_feature_meta": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "ekf_num_archived": (C.c_int, [_P]),
    "ekf_get_feature_track": (C.c_int, [_P, _P, _P, _P, _P]),
    "ekf_set_feature_track": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "ekf_find_new_features": (C.c_int, [_P, C.c_int, C.c_double, C.c_double, C.c_int, _P, C.POINTER(C.c_int)]),
    "ekf_end_update": (C.c_int, [_P, C.c_float, C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_int)]),
    "ekf_get_search_ellipses": (C.c_int, [_P, C.c_int, _P]),
    "ekf_ransac_1point": (C.c_int, [_P, _P, _P, C.c_int, C.c_double, _P, _P, C.POINTER(C.c_int)]),
    "ekf_update_two_stage": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_uint, C.c_double, C.c_double, _P, _P,
                                       C.POINTER(C.c_int)]),
    "ekf_innovation_covariance": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "ekf_get_gain": (C.c_int, [_P, _P]),
    "ekf_last_measurement_rows": (C.c_int, [_P]),
    "ekf_convert_xyz_if_linear": (C.c_int, [_P, C.c_int]),
    "ekf_convert_xyz_if_linear_all": (C.c_int, [_P]),
    "ekf_num_features": (C.c_int, [_P]),
    "ekf_state_dim": (C.c_int, [_P]),
    "ekf_get_feature_layout": (C.c_int, [_P, _P, _P]),
    "ekf_get_state": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ekf_set_state": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ekf_get_sigma_block": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ekf_peek_workspace": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ekf_set_sigma_block": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ekf_covariance_parameter": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "ekf_feature_xyz": (C.c_int, [_P, C.c_int, _P, _P]),
    "ekf_check_invariants": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ekf_profile_kernels": (C.c_int, []),
    "ekf_profile_kernel_name": (C.c_char_p, [C.c_int]),
    "ekf_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "ekf_profile_reset": (C.c_int, [_P]),
    "ekf_profile_work": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "ekf_get_chunk_plan": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ekf_launch_kinds": (C.c_int, []),
    "ekf_launch_kind_name": (C.c_char_p, [C.c_int]),
    "ekf_launch_count": (C.c_int, [_P, C.c_int, C.POINTER(C.c_longlong)]),
    "ekf_shard_configure": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "ekf_shard_get_info": (C.c_int, [_P, _P]),
    "ekf_shard_update": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "ekf_shard_rebalance": (C.c_int, [_P]),
    "ekf_device_mu": (_P, [_P]),
    "ekf_device_sigma": (_P, [_P, C.POINTER(C.c_int)]),
    "ekf_sba_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "ekf_sba_create_solver": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "ekf_sba_get_solver": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "ekf_sba_set_cg": (C.c_int, [_P, C.c_double, C.c_int]),
    "ekf_sba_get_cg": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "ekf_sba_get_cg_log": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_int)]),
    "ekf_sba_destroy": (None, [_P]),
    "ekf_sba_last_error": (C.c_char_p, [_P]),
    "ekf_sba_add_nodes": (C.c_int, [_P, C.c_int, _P]),
    "ekf_sba_add_points": (C.c_int, [_P, C.c_int, _P]),
    "ekf_sba_add_projections": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_int)]),
    "ekf_sba_counts": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ekf_sba_run": (C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_int)]),
    "ekf_sba_cost": (C.c_int, [_P, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ekf_sba_set_huber": (C.c_int, [_P, C.c_double]),
    "ekf_sba_get_huber": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "ekf_sba_count_bad": (C.c_int, [_P, C.c_double, C.POINTER(C.c_int)]),
    "ekf_sba_remove_bad": (C.c_int, [_P, C.c_double, C.POINTER(C.c_int)]),
    "ekf_sba_reduce_tracks": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "ekf_sba_num_bad_points": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "ekf_sba_avg_error": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "ekf_sba_get_projections": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_int)]),
    "ekf_sba_get_nodes": (C.c_int, [_P, _P]),
    "ekf_sba_get_points": (C.c_int, [_P, _P]),
    "ekf_sba_get_log": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int)]),
    "ekf_sba_profile": (C.c_int, [_P, C.c_int]),
    "ekf_sba_get_profile": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "ekf_keyframe_create": (C.c_int, [_P, C.c_float, C.POINTER(_P)]),
    "ekf_keyframe_create_raw": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "ekf_keyframe_destroy": (None, [_P]),
    "ekf_keyframe_last_error": (C.c_char_p, [_P]),
    "ekf_keyframe_set_option": (C.c_int, [_P, C.c_int, C.c_int]),
    "ekf_keyframe_observe": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ekf_keyframe_get_emitted": (C.c_int, [_P, C.POINTER(C.c_int), _P, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "ekf_keyframe_get_image": (C.c_int, [_P, _P, C.c_int]),
    "ekf_keyframe_get_raw_image": (C.c_int, [_P, _P, C.c_int]),
    "ekf_keyframe_get_state": (C.c_int, [_P, _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "ekf_keyframe_reset": (C.c_int, [_P]),
    "ekf_rectified_camera": (C.c_int, [_P, C.c_int, _P]),
    "ekf_get_frame_rectified": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "ekf_undistort_pixels": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "ekf_keyframe_get_image_rectified": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "ekf_keyframe_get_emitted_rectified": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(C.c_int)]),
    "ekf_dense_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "ekf_dense_destroy": (None, [_P]),
    "ekf_dense_last_error": (C.c_char_p, [_P]),
    "ekf_dense_set_view": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "ekf_dense_set_view_device": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "ekf_dense_set_view_from_keyframe": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "ekf_dense_set_pose": (C.c_int, [_P, C.c_int, _P]),
    "ekf_dense_get_view": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "ekf_dense_sweep": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]),
    "ekf_dense_filter": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_int]),
    "ekf_dense_get_depth": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "ekf_dense_get_points": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ekf_dense_profile": (C.c_int, [_P, C.c_int]),
    "ekf_dense_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_fusion_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_double, C.c_double, C.c_int, C.POINTER(_P)]),
    "ekf_fusion_destroy": (None, [_P]),
    "ekf_fusion_last_error": (C.c_char_p, [_P]),
    "ekf_fusion_integrate": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ekf_fusion_integrate_host": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ekf_fusion_reset": (C.c_int, [_P]),
    "ekf_fusion_get_volume": (C.c_int, [_P, _P, _P, _P, _P]),
    "ekf_fusion_set_volume": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "ekf_fusion_extract": (C.c_int, [_P, C.c_int, C.POINTER(C.c_ulonglong)]),
    "ekf_fusion_get_mesh": (C.c_int, [_P, _P, _P, _P, C.c_ulonglong]),
    "ekf_fusion_profile": (C.c_int, [_P, C.c_int]),
    "ekf_fusion_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_raycast_render": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_double, C.c_double, C.c_double, C.c_int]),
    "ekf_raycast_render_view": (C.c_int, [_P, _P, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]),
    "ekf_raycast_get": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "ekf_raycast_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_dense_set_view_colour": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "ekf_dense_set_view_colour_device": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "ekf_dense_set_view_colour_from_keyframe": (C.c_int, [_P, C.c_int, _P, _P]),
    "ekf_dense_get_view_colour": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "ekf_dense_sweep_sgm": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int]),
    "ekf_dense_get_volume": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ekf_dense_get_sgm_profile": (C.c_int, [_P, _P, _P]),
    "ekf_dense_sweep_census": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]),
    "ekf_dense_sweep_sgm_census": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int]),
    "ekf_dense_get_census": (C.c_int, [_P, C.c_int, _P]),
    "ekf_dense_get_census_profile": (C.c_int, [_P, _P, _P]),
    "ekf_dense_sweep_best": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int]),
    "ekf_dense_get_best_profile": (C.c_int, [_P, _P, _P]),
    "ekf_dense_keep_runner_up": (C.c_int, [_P, C.c_int]),
    "ekf_dense_get_runner_up": (C.c_int, [_P, C.c_int, _P]),
    "ekf_dense_filter_unique": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_int, C.c_int]),
    "ekf_dense_get_unique_profile": (C.c_int, [_P, _P, _P]),
    "ekf_dense_filter_speckle": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "ekf_dense_get_segments": (C.c_int, [_P, C.c_int, _P, _P]),
    "ekf_dense_speckle_host": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "ekf_dense_get_speckle_profile": (C.c_int, [_P, _P, _P]),
    "ekf_colour_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_double, C.c_double, C.c_int, C.POINTER(_P)]),
    "ekf_colour_has": (C.c_int, [_P]),
    "ekf_colour_integrate_host": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ekf_colour_get_volume": (C.c_int, [_P, _P]),
    "ekf_colour_set_volume": (C.c_int, [_P, _P]),
    "ekf_colour_get_mesh": (C.c_int, [_P, _P, C.c_ulonglong]),
    "ekf_colour_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_colour_get_render": (C.c_int, [_P, _P]),
    "ekf_mesh_weld": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "ekf_mesh_get": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_ulonglong, C.c_ulonglong]),
    "ekf_mesh_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_components_find": (C.c_int, [_P, C.POINTER(C.c_ulonglong)]),
    "ekf_components_get": (C.c_int, [_P, _P, _P, C.c_ulonglong]),
    "ekf_components_prune": (C.c_int, [_P, C.c_uint, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "ekf_components_get_pruned": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_ulonglong, C.c_ulonglong]),
    "ekf_components_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_smooth_run": (C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_ulonglong),
                                 C.POINTER(C.c_ulonglong)]),
    "ekf_smooth_get": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_ulonglong, C.c_ulonglong]),
    "ekf_smooth_get_adjacency": (C.c_int, [_P, _P, _P, _P, C.c_ulonglong]),
    "ekf_smooth_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_simplify_run": (C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                   C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "ekf_simplify_get": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_ulonglong, C.c_ulonglong]),
    "ekf_simplify_get_map": (C.c_int, [_P, _P, C.c_ulonglong]),
    "ekf_simplify_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_texture_begin": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ekf_texture_add_view": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_ulonglong)]),
    "ekf_texture_add_view_host": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_double, C.c_double,
                                            C.POINTER(C.c_ulonglong)]),
    "ekf_texture_finish": (C.c_int, [_P, C.POINTER(C.c_ulonglong)]),
    "ekf_texture_get": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_ulonglong]),
    "ekf_texture_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_raster_set_mesh": (C.c_int, [_P, _P, _P, _P, _P, C.c_ulonglong, C.c_ulonglong]),
    "ekf_raster_render": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_double, C.c_int, C.c_int, C.c_int]),
    "ekf_raster_render_view": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]),
    "ekf_raster_get": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ekf_raster_set_small_limit": (C.c_int, [_P, C.c_int]),
    "ekf_raster_get_profile": (C.c_int, [_P, _P, _P]),
    "ekf_distance_set_mesh": (C.c_int, [_P, _P, _P, C.c_ulonglong, C.c_ulonglong]),
    "ekf_distance_run": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]),
    "ekf_distance_run_points": (C.c_int, [_P, C.c_int, _P, C.c_ulonglong]),
    "ekf_distance_get": (C.c_int, [_P, _P, _P, _P, _P, C.c_ulonglong]),
    "ekf_distance_get_stats": (C.c_int, [_P, C.c_double, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_double),
                                         C.POINTER(C.c_ulonglong), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]),
    "ekf_distance_set_grid": (C.c_int, [_P, C.c_int]),
    "ekf_distance_get_grid": (C.c_int, [_P, _P, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]),
    "ekf_distance_get_profile": (C.c_int, [_P, _P, _P]),
}

_lib = None


def ptr(a):
    """The data of a numpy array as void*; None stays NULL."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Handle:
    """Base of the wrapper classes: one handle of the family ``_family`` (``ekf``, ``ekf_sba``, ``ekf_keyframe``, ``ekf_dense``
    or ``ekf_fusion``), which names its ``<family>_destroy`` and ``<family>_last_error``.  ``close`` may be called twice, and
    an object whose constructor raised is deleted without harm."""
    _family = "ekf"

    def _create(self, create, *args):
        """``<create>(*args, &handle)``; raises with the message the library keeps for a failed create."""
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = getattr(self._lib, create)(*args, C.byref(self._h))
        if rc != 0:
            msg = getattr(self._lib, self._family + "_last_error")(None)
            raise EkfError(rc, msg.decode() if msg else create + " failed")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(self._lib, self._family + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = getattr(self._lib, self._family + "_last_error")(self._h)
            raise EkfError(rc, msg.decode() if msg else "")


def load_library(path: str = LIB_PATH):
    """dlopen the HIP library and attach prototypes.  Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise EkfError(3, f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)            # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
