"""ctypes binding of include/se2gpu.h (libse2gpu.so).

This is harness plumbing for tests/ and bench.py: the product is the C-ABI library and the C++
adapters in include/se2lam_amd/.  There is NO fallback: if the shared library is missing this
module raises, and if no GPU is visible every compute call raises `Se2GpuError`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libse2gpu.so")

OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_STATE = -1, -2, -3, -4, -5


class Se2GpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"se2gpu error {code}: {msg}")
        self.code = code


class Keypoint(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("class_id", C.c_int32)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28 == C.sizeof(Keypoint)


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("score_type", C.c_int32), ("fast_th", C.c_int32), ("max_rows", C.c_int32),
                ("max_cols", C.c_int32), ("max_batch", C.c_int32)]


class FrameBounds(C.Structure):
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float)]


class Camera(C.Structure):
    """se2gpu_camera: fx, fy, cx, cy, d[8] (OpenCV order k1 k2 p1 p2 [k3 [k4 k5 k6]]), nd in {4, 5, 8}"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("d", C.c_float * 8),
                ("nd", C.c_int32)]

    @classmethod
    def from_KD(cls, K, D):
        K = np.asarray(K, np.float32).reshape(3, 3)
        D = np.asarray(D, np.float32).ravel()
        c = cls(K[0, 0], K[1, 1], K[0, 2], K[1, 2], (C.c_float * 8)(), len(D))
        for i, v in enumerate(D[:8]):
            c.d[i] = v
        return c


class LocalGraph(C.Structure):
    _fields_ = [("n_local_kf", C.c_int32), ("n_ref_kf", C.c_int32), ("n_mp", C.c_int32), ("n_obs", C.c_int32),
                ("kf_id", C.c_void_p), ("kf_Twb", C.c_void_p), ("kf_Rcw", C.c_void_p),
                ("odo_to", C.c_void_p), ("odo_meas", C.c_void_p), ("odo_cov", C.c_void_p),
                ("mp_pos", C.c_void_p), ("obs_mp", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_uv", C.c_void_p),
                ("obs_lc", C.c_void_p), ("obs_sigma2", C.c_void_p),
                ("fx", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("Rbc", C.c_double * 9), ("tbc", C.c_double * 3),
                ("huber_delta", C.c_float), ("xrot_info", C.c_float), ("z_info", C.c_float)]


class MapView(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_mp", C.c_int32), ("kf_id", C.c_void_p), ("covis_ptr", C.c_void_p),
                ("covis_idx", C.c_void_p), ("kf_mp_ptr", C.c_void_p), ("kf_mp_idx", C.c_void_p), ("mp_id", C.c_void_p),
                ("mp_kf_ptr", C.c_void_p), ("mp_kf_idx", C.c_void_p)]


class VocTrainParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("max_iters", C.c_int32),
                ("seed", C.c_uint64)]


class VocTrainStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nodes", "words", "kmeans_nodes", "trivial_nodes", "lloyd_iters_total", "lloyd_iters_max",
                                         "short_seeded_nodes", "empty_clusters", "capped_nodes", "zero_weight_words")]


class BaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("terminated", C.c_int32),
                ("stopped", C.c_int32), ("chi2_init", C.c_double), ("chi2_final", C.c_double),
                ("lambda_final", C.c_double), ("chi2_hist", C.c_double * 64), ("lambda_hist", C.c_double * 64),
                ("trials_hist", C.c_int32 * 64)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)

# every symbol declared in include/se2gpu.h: name -> (restype, argtypes)
_VP, _I, _D, _F, _SZ = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_size_t
_PD, _PI32, _PU8, _PF = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
_PKP = C.POINTER(Keypoint)
SYMBOLS = {
    "se2gpu_last_error": (C.c_char_p, []),
    "se2gpu_device_count": (_I, []),
    "se2gpu_version": (C.c_char_p, []),
    # ORB extractor
    "se2gpu_orb_create": (_I, [C.POINTER(OrbParams), C.POINTER(_VP)]),
    "se2gpu_orb_destroy": (None, [_VP]),
    "se2gpu_orb_levels": (_I, [_VP]),
    "se2gpu_orb_scale_factor": (_F, [_VP]),
    "se2gpu_orb_extract": (_I, [_VP, _VP, _I, _I, _SZ, _VP, _VP, _VP, _I, C.POINTER(_I)]),
    "se2gpu_orb_extract_batch_device": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _I]),
    "se2gpu_orb_sync": (_I, [_VP]),
    "se2gpu_orb_set_stream": (_I, [_VP, _VP]),
    "se2gpu_orb_debug_level": (_I, [_VP, _I, _I, _I, _VP, _SZ, C.POINTER(_I), C.POINTER(_I)]),
    "se2gpu_orb_debug_score": (_I, [_VP, _I, _I, _VP, _SZ, C.POINTER(_I), C.POINTER(_I)]),
    "se2gpu_orb_debug_nth_element": (_I, [_VP, _I, _I, _I]),
    "se2gpu_orb_stream": (_VP, [_VP]),
    "se2gpu_undistort_map": (_I, [C.POINTER(Camera), _I, _I, _VP, _VP]),
    "se2gpu_undistort_points": (_I, [C.POINTER(Camera), _VP, _I, _VP]),
    "se2gpu_frame_bounds_un": (_I, [C.POINTER(Camera), _I, _I, C.POINTER(FrameBounds)]),
    "se2gpu_orb_set_camera": (_I, [_VP, C.POINTER(Camera)]),
    "se2gpu_orb_score_kernel": (_I, [_VP, _VP]),
    "se2gpu_orb_profile": (_I, [_VP, _I]),
    "se2gpu_orb_profile_get": (_I, [_VP, _I, C.POINTER(C.c_char_p), _PD, C.POINTER(C.c_int64)]),
    # matcher
    "se2gpu_hamming": (_I, [_VP, _VP]),
    "se2gpu_three_maxima": (_I, [_VP, _I, _VP, _VP, _VP]),
    "se2gpu_matcher_create": (_I, [_I, _I, C.POINTER(_VP)]),
    "se2gpu_matcher_destroy": (None, [_VP]),
    "se2gpu_matcher_set_stream": (_I, [_VP, _VP]),
    "se2gpu_matcher_sync": (_I, [_VP]),
    "se2gpu_matcher_spill_calls": (_I, [_VP, _VP]),
    "se2gpu_matcher_stream": (_VP, [_VP]),
    "se2gpu_match_window": (_I, [_VP, C.POINTER(FrameBounds), _VP, _VP, _I, _VP, _VP, _I, _VP, _I, _I, _I, _I, _F,
                                 _VP, C.POINTER(_I)]),
    "se2gpu_match_window_batch_device": (_I, [_VP, C.POINTER(FrameBounds), _VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I,
                                              _I, _I, _F, _VP, _VP]),
    "se2gpu_search_by_bow": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP, _I, _F, _I,
                                  _VP, C.POINTER(_I)]),
    "se2gpu_search_by_bow_batch_device": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _F, _I,
                                               _VP, _VP]),
    "se2gpu_match_projection": (_I, [_VP, C.POINTER(FrameBounds), _VP, _VP, _VP, _VP, _I, _VP, _F, _F, _F, _F,
                                     _VP, _VP, _VP, _I, _I, _I, _F, _VP, C.POINTER(_I)]),
    "se2gpu_match_projection_device": (_I, [_VP, C.POINTER(FrameBounds), _VP, _VP, _VP, _VP, _I, _VP, _F, _F, _F, _F,
                                            _VP, _VP, _VP, _I, _I, _I, _F, _VP, _VP]),
    "se2gpu_mappoint_main_batch_device": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _I, _VP,
                                               _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_mappoint_parallax_batch_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP,
                                                   _F, _F, _F, _VP, _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_kf_correspd_batch_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                             _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _F, _F, _F, _I, _VP, _VP, _VP, _VP, _VP,
                                             _VP, _VP, _VP]),
    "se2gpu_map_apply_ws_bytes": (C.c_longlong, [_I, _I, _I, _I]),
    "se2gpu_map_apply_batch_device": (_I, [_VP, _VP, _I, _I, _VP] + [_VP] * 5 + [_VP, _I, _I, _VP, _VP, _I] + [_VP] * 8 +
                                      [_I, _VP] + [_VP] * 16 + [_VP, C.c_longlong]),
    "se2gpu_covis_bits_words": (C.c_longlong, [_I, _I]),
    "se2gpu_covis_build_device": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP]),
    "se2gpu_covis_pairs_device": (_I, [_VP, _VP, _I, _I, _VP, _VP, _I, _F, _D, _VP, _VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _I]),
    "se2gpu_covis_refset_device": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _I, _I, _I, _D, _VP, _VP]),
    "se2gpu_covis_adj_words": (C.c_longlong, [_I]),
    "se2gpu_covis_connect_device": (_I, [_VP, _VP, _I, _VP, _VP, _I, _VP, _I]),
    "se2gpu_covis_disconnect_device": (_I, [_VP, _VP, _I, _VP, _I]),
    "se2gpu_local_window_batch_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I,
                                              _VP, _I]),
    "se2gpu_local_ba_ws_bytes": (C.c_longlong, [_I, _I, _I, _I, _I]),
    "se2gpu_local_ba_ws_layout": (_I, [_I, _I, _I, _I, _I, _VP, _VP, _I]),
    "se2gpu_local_ba_batch_device": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                          _VP, _VP, _I, _VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _I, _F, _F, _F, _VP, _D, _D, _D,
                                          _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_localizer_ba_ws_bytes": (C.c_longlong, [_I, _I]),
    "se2gpu_localizer_ba_ws_layout": (_I, [_I, _I, _VP, _VP, _I]),
    "se2gpu_localizer_ba_batch_device": (_I, [_VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I,
                                              _F, _F, _F, _VP, _D, _D, _D, _D, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    # BA
    "se2gpu_ba_create": (_I, [C.POINTER(_VP)]),
    "se2gpu_ba_reserve": (_I, [_I, _I, _I]),
    "se2gpu_ba_destroy": (None, [_VP]),
    "se2gpu_ba_clear": (_I, [_VP]),
    "se2gpu_ba_set_stream": (_I, [_VP, _VP]),
    "se2gpu_ba_stream": (_VP, [_VP]),
    "se2gpu_ba_add_cam": (_I, [_VP, _D, _D, _D]),
    "se2gpu_ba_set_Tbc": (_I, [_VP, _PD, _PD]),
    "se2gpu_ba_add_vertex_se2": (_I, [_VP, _I, _D, _D, _D, _I]),
    "se2gpu_ba_add_vertex_xyz": (_I, [_VP, _I, _PD, _I, _I]),
    "se2gpu_ba_add_edge_se2xyz": (_I, [_VP, _I, _I, _PD, _PD, _D]),
    "se2gpu_ba_add_edge_se2": (_I, [_VP, _I, _I, _PD, _PD]),
    "se2gpu_ba_load": (_I, [_VP, _I, _I, _I, _I, _PD, _PU8, _PD, _PI32, _PI32, _PD, _PD, _PI32, _PI32, _PD, _PD, _D]),
    "se2gpu_ba_load_local_graph": (_I, [_VP, C.POINTER(LocalGraph)]),
    "se2gpu_ba_add_vertex_se3": (_I, [_VP, _I, _PD, _I]),
    "se2gpu_ba_add_vertex_iso3": (_I, [_VP, _I, _PD, _I]),
    "se2gpu_plane_motion_prior_iso3": (_I, [_VP, _VP, _D, _D, _D, _VP, _VP]),
    "se2gpu_ba_add_prior_se3": (_I, [_VP, _I, _PD, _PD]),
    "se2gpu_ba_add_edge_se3": (_I, [_VP, _I, _I, _PD, _PD]),
    "se2gpu_ba_add_edge_xyz2uv": (_I, [_VP, _I, _I, _PD, _D, _D]),
    "se2gpu_ba_get_se3": (_I, [_VP, _I, _PD]),
    "se2gpu_ba_edge_chi2": (_I, [_VP, _PD, _I]),
    "se2gpu_map_update_local_graph": (_I, [C.POINTER(MapView), _I, _I, _VP, C.POINTER(_I), _VP, C.POINTER(_I), _VP, C.POINTER(_I)]),
    "se2gpu_sparsify_se3xyz": (_I, [_I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_feat_edge_batch": (_I, [_I, _I, _I, _I, _VP, _VP, _D, _D, _D, _VP, _VP, _VP, _VP, _D, _D, _VP, _VP, _VP, _VP, _VP,
                                    _VP, _VP, _VP]),
    "se2gpu_feat_edge_ws_bytes": (C.c_longlong, [_I, _I]),
    "se2gpu_feat_edge_ws_layout": (_I, [_I, _I, _VP, _I]),
    "se2gpu_feat_edge_batch_device": (_I, [_VP, _I, _I, _I, _D, _D, _VP, _D, _D, _D, _VP, _VP, _I, _I, _VP, _VP, _I, _I,
                                           _VP, _VP, _I, _VP, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP,
                                           _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_ba_initialize": (_I, [_VP]),
    "se2gpu_ba_set_edge_level": (_I, [_VP, _I, _I]),
    "se2gpu_ba_reset_estimates": (_I, [_VP]),
    "se2gpu_ba_reset_estimates_batch": (_I, [_VP, _I]),
    "se2gpu_ba_optimize": (_I, [_VP, _I, _I, _PU8, _I, C.POINTER(BaStats)]),
    "se2gpu_ba_optimize_batch": (_I, [C.POINTER(_VP), _I, _I, _I, _PU8, C.POINTER(BaStats)]),
    "se2gpu_ba_last_batch_path": (_I, []),
    "se2gpu_ba_get_se2": (_I, [_VP, _I, _PD]),
    "se2gpu_ba_get_xyz": (_I, [_VP, _I, _PD]),
    "se2gpu_ba_get_all": (_I, [_VP, _PD, _PD]),
    "se2gpu_ba_chi2": (_D, [_VP]),
    "se2gpu_ba_debug_reduced_system": (_I, [_VP, _D, _PD, _PD]),
    "se2gpu_ba_debug_solve": (_I, [_VP, _D, _PD, C.POINTER(C.c_int)]),
    "se2gpu_ba_debug_solver_path": (_I, [_VP]),
    "se2gpu_ba_debug_linearize_counts": (_I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "se2gpu_ba_debug_chol_verify": (_I, [_VP, _VP, _VP, _I]),
    "se2gpu_ba_debug_pool_sizes": (_I, [_VP]),
    "se2gpu_ba_debug_solve_plan": (_I, [_I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _I]),
    "se2gpu_ba_debug_solve_plan_tile": (_I, [_I, _I, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _I]),
    "se2gpu_ba_debug_solve_plan_neager": (_I, [_I, _I, _VP, _I, _I, _VP, _I]),
    "se2gpu_ba_debug_plan_neager": (_I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _VP, _I]),
    "se2gpu_ba_debug_flat_records_host": (_I, [_I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_ba_debug_flat_records": (_I, [_VP, _VP, _VP, _I, C.POINTER(C.c_int)]),
    "se2gpu_ba_debug_reduce_grid": (_I, [_VP, _VP]),
    "se2gpu_ba_debug_plan_host": (_I, [_I, _I, _I, _VP, _VP, _VP, _I, _VP, _VP, _I, _I, _VP, _I, _VP]),
    "se2gpu_debug_se3": (_I, [_I, _I, _VP, _VP]),
    "se2gpu_debug_wave_int": (_I, [_I, _I, _I, _VP, _VP]),
    "se2gpu_triangulate": (_I, [_I, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _I, _VP, _VP,
                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "se2gpu_track_create": (_I, [C.POINTER(_VP)]),
    "se2gpu_track_destroy": (None, [_VP]),
    "se2gpu_track_fundamental_mask": (_I, [_VP, _VP, _VP, _I, _VP, C.POINTER(C.c_int)]),
    "se2gpu_track_remove_outliers": (_I, [_VP, _VP, _I, _VP, _I, _VP, C.POINTER(C.c_int)]),
    "se2gpu_track_last_ransac": (_I, [_VP, _VP]),
    "se2gpu_track_set_stream": (_I, [_VP, _VP]),
    "se2gpu_track_stream": (_VP, [_VP]),
    "se2gpu_track_sync": (_I, [_VP]),
    "se2gpu_track_loop_verify_batch_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "se2gpu_track_frames_batch_device": (_I, [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, C.c_float,
                                              C.c_float, _I, _VP, _VP, _VP, _VP]),
    "se2gpu_plane_motion_prior": (_I, [_VP, _VP, _D, _D, _D, _VP, _VP]),
    "se2gpu_track_pose_ba": (_I, [_VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _D, _D, _D, _D, _I, _VP, C.POINTER(BaStats)]),
    "se2gpu_track_triangulate": (_I, [_VP, _I, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _I, _VP, _VP,
                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "se2gpu_ba_reduce_buffer_doubles": (_SZ, [_VP, _I]),
    "se2gpu_ba_exchange_doubles": (_SZ, [_I]),
    "se2gpu_ba_exchange_doubles_h": (_SZ, [_VP]),
    "se2gpu_ba_exchange_row": (_I, [_I, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "se2gpu_ba_set_allreduce": (_I, [_VP, ALLREDUCE_FN, _VP, _VP]),
    "se2gpu_ba_set_shard": (_I, [_VP, _I, _I]),
    "se2gpu_comm_unique_id": (_I, [_VP]),
    "se2gpu_comm_create": (_I, [_VP, _I, _I, C.POINTER(_VP)]),
    "se2gpu_comm_destroy": (None, [_VP]),
    "se2gpu_comm_count": (_I, [_VP, C.POINTER(_I)]),
    "se2gpu_comm_allreduce_sum_f64": (_I, [_VP, _VP, _SZ, _VP]),
    "se2gpu_ba_set_comm": (_I, [_VP, _VP]),
    "se2gpu_ba_shard_landmarks": (_I, [_I, _I, _PI32, _PI32, _I, _PI32]),
    "se2gpu_ba_edge_information": (_I, [_I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _F, _F, _F, _VP]),
    "se2gpu_ba_profile": (_I, [_VP, _I]),
    "se2gpu_ba_profile_get": (_I, [_VP, _I, C.POINTER(C.c_char_p), _PD, C.POINTER(C.c_int64)]),
    # DBoW2 vocabulary
    "se2gpu_voc_create": (_I, [_I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, C.POINTER(_VP)]),
    "se2gpu_voc_load": (_I, [C.c_char_p, C.POINTER(_VP)]),
    "se2gpu_voc_destroy": (None, [_VP]),
    "se2gpu_voc_words": (_I, [_VP]),
    "se2gpu_voc_nodes": (_I, [_VP]),
    "se2gpu_voc_k": (_I, [_VP]),
    "se2gpu_voc_L": (_I, [_VP]),
    "se2gpu_voc_scoring": (_I, [_VP]),
    "se2gpu_voc_weighting": (_I, [_VP]),
    "se2gpu_voc_export": (_I, [_VP, _I, _VP, _VP, _VP, _VP]),
    "se2gpu_voc_save": (_I, [_VP, C.c_char_p]),
    "se2gpu_voc_train": (_I, [_VP, _VP, _VP, _I, _I, _I, C.POINTER(_VP), _VP]),
    "se2gpu_voc_train_profile": (_I, [_I]),
    "se2gpu_voc_train_profile_get": (_I, [_I, C.POINTER(C.c_char_p), _PD, C.POINTER(C.c_int64)]),
    "se2gpu_bow_create": (_I, [_VP, _I, _I, C.POINTER(_VP)]),
    "se2gpu_bow_destroy": (None, [_VP]),
    "se2gpu_bow_set_stream": (_I, [_VP, _VP]),
    "se2gpu_bow_sync": (_I, [_VP]),
    "se2gpu_bow_stream": (_VP, [_VP]),
    "se2gpu_bow_transform_batch_device": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "se2gpu_bow_transform": (_I, [_VP, _VP, _I, _I, _VP, _VP, C.POINTER(_I), _VP, _VP, _VP, C.POINTER(_I)]),
    "se2gpu_bowdb_create": (_I, [_VP, C.POINTER(_VP)]),
    "se2gpu_bowdb_destroy": (None, [_VP]),
    "se2gpu_bowdb_add": (_I, [_VP, _I, _VP, _VP, _I]),
    "se2gpu_bowdb_add_device": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _I]),
    "se2gpu_bowdb_remove": (_I, [_VP, _I]),
    "se2gpu_bowdb_size": (_I, [_VP]),
    "se2gpu_bowdb_query": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, C.POINTER(_I), C.POINTER(_I), _PD]),
    # timers / memory
    "se2gpu_timer_create": (_I, [C.POINTER(_VP)]),
    "se2gpu_timer_destroy": (None, [_VP]),
    "se2gpu_timer_start": (_I, [_VP, _VP]),
    "se2gpu_timer_stop": (_I, [_VP, _VP]),
    "se2gpu_timer_elapsed_ms": (_I, [_VP, C.POINTER(C.c_float)]),
    "se2gpu_malloc": (_I, [C.POINTER(_VP), _SZ]),
    "se2gpu_free": (_I, [_VP]),
    "se2gpu_memcpy_h2d": (_I, [_VP, _VP, _SZ]),
    "se2gpu_memcpy_d2h": (_I, [_VP, _VP, _SZ]),
    "se2gpu_host_alloc": (_I, [C.POINTER(_VP), _SZ]),
    "se2gpu_host_free": (_I, [_VP]),
    "se2gpu_memcpy_h2d_async": (_I, [_VP, _VP, _SZ, _VP]),
    "se2gpu_memcpy_d2h_async": (_I, [_VP, _VP, _SZ, _VP]),
    "se2gpu_stream_create": (_I, [C.POINTER(_VP)]),
    "se2gpu_stream_destroy": (_I, [_VP]),
    "se2gpu_stream_synchronize": (_I, [_VP]),
    "se2gpu_timer_stream_wait": (_I, [_VP, _VP]),
    "se2gpu_device_synchronize": (_I, []),
    "se2gpu_set_device": (_I, [_I]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libse2gpu.so (fails loudly when it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing - run `python -m se2lam_amd.build` (or __graft_entry__.build()). "
                "se2lam_amd has no CPU / eager fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int):
    if rc != OK:
        raise Se2GpuError(rc, lib().se2gpu_last_error().decode(errors="replace"))


def device_count() -> int:
    return int(lib().se2gpu_device_count())


def vp(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def pd(a: np.ndarray):
    return a.ctypes.data_as(_PD)


class DeviceArray:
    """A raw device allocation (se2gpu_malloc) with numpy round-trips; for tests and bench."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(lib().se2gpu_malloc(C.byref(self.ptr), self.nbytes))

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceArray":
        a = np.ascontiguousarray(a)
        d = cls(a.nbytes)
        if a.nbytes:
            check(lib().se2gpu_memcpy_h2d(d.ptr, vp(a), a.nbytes))
        return d

    def to_numpy(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        if out.nbytes:
            check(lib().se2gpu_memcpy_d2h(vp(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().se2gpu_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def dev_ptr(d):
    """a DeviceArray, a raw device pointer or None -> what ctypes passes for a pointer argument"""
    return None if d is None else (d.ptr if isinstance(d, DeviceArray) else d)


def upload(a, dtype=None) -> DeviceArray:
    """a host array in device memory; an empty one gets one element (an allocation of 0 bytes has no address)"""
    a = np.ascontiguousarray(a, dtype)
    return DeviceArray.from_numpy(a if a.size else np.zeros(1, a.dtype))


SENT, ISENT = -7.0, -9   # float / integer outputs start from these: the calls leave alone what they do not compute
SENTINEL_FRAME, SENTINEL_OCTAVE, SENTINEL_DIST, SENTINEL_DESC = -55, -77, -1.0, 0xAB   # the main-key-frame call's own


def csr(lists):
    """[(frames, features), ...] per point, in container order -> mp_ptr (m + 1), obs_frame, obs_ftr (int32) of obs_table.h"""
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(f) for f, _ in lists])
    cat = lambda j: np.concatenate([np.asarray(l[j], np.int32).ravel() for l in lists] + [np.zeros(0, np.int32)])
    return ptr, cat(0), cat(1)


class PinnedArray:
    """Pinned host allocation (se2gpu_host_alloc) viewed as a numpy array; for the streaming bench."""

    def __init__(self, shape, dtype):
        self.ptr = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        check(lib().se2gpu_host_alloc(C.byref(self.ptr), n))
        buf = (C.c_uint8 * n).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def __del__(self):
        try:
            if self.ptr:
                self.array = None
                lib().se2gpu_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


class Stream:
    def __init__(self):
        self.h = C.c_void_p()
        check(lib().se2gpu_stream_create(C.byref(self.h)))

    def sync(self):
        check(lib().se2gpu_stream_synchronize(self.h))

    def __del__(self):
        try:
            if self.h:
                lib().se2gpu_stream_destroy(self.h)
        except Exception:
            pass


class Timer:
    def __init__(self):
        self.h = C.c_void_p()
        check(lib().se2gpu_timer_create(C.byref(self.h)))

    def start(self, stream):
        check(lib().se2gpu_timer_start(self.h, stream))

    def stop(self, stream):
        check(lib().se2gpu_timer_stop(self.h, stream))

    def make_wait(self, stream):
        """`stream` waits for this timer's stop event (cross-stream ordering without a host sync)"""
        check(lib().se2gpu_timer_stream_wait(self.h, stream))

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        check(lib().se2gpu_timer_elapsed_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            if self.h:
                lib().se2gpu_timer_destroy(self.h)
        except Exception:
            pass


# ops of se2gpu_debug_se3 (include/se2gpu.h), with the doubles each reads and writes per item
SE3_OPS = {"exp": (0, 6, 12), "log": (1, 12, 6), "mul": (2, 24, 12), "normalize": (3, 9, 9), "quat_of": (4, 9, 4),
           "to_mqt": (5, 12, 6), "from_mqt": (6, 6, 12), "adj": (7, 12, 36), "jac_right": (8, 12, 36),
           "jac_left_inv": (9, 24, 36), "log_exp": (10, 6, 6)}


def debug_se3(op: str, x) -> np.ndarray:
    """se2gpu_debug_se3: function `op` of csrc/se3_math.h on the device for every row of x (n, doubles the op reads) -> (n, doubles
    it writes), one launch"""
    code, nin, nout = SE3_OPS[op]
    x = np.ascontiguousarray(x, np.float64).reshape(-1, nin)
    n = x.shape[0]
    buf = np.zeros((n, 24))
    buf[:, :nin] = x
    out = np.zeros((n, 36))
    check(lib().se2gpu_debug_se3(code, n, vp(buf), vp(out)))
    return out[:, :nout].copy()


# ops of se2gpu_debug_wave_int (include/se2gpu.h); the workgroup scans write one more word, the sum of all
WAVE_INT_OPS = {"sum": 0, "min": 1, "max": 2, "scan_i32": 3, "scan_i64": 4, "rank": 5, "block_scan_i32": 6, "block_scan_i64": 7,
                "fresh_scan_i32": 8, "fresh_scan_i64": 9}


def debug_wave_int(op: str, block: int, x) -> np.ndarray:
    """se2gpu_debug_wave_int: function `op` of csrc/wave_int.h by one workgroup of `block` threads over the int64 values x -> int64
    (len(x), or len(x) + 1 for the workgroup scans)"""
    code = WAVE_INT_OPS[op]
    x = np.ascontiguousarray(x, np.int64).reshape(-1)
    out = np.zeros(len(x) + (1 if code >= 6 else 0), np.int64)
    check(lib().se2gpu_debug_wave_int(code, int(block), len(x), vp(x), vp(out)))
    return out
