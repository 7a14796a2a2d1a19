"""ctypes binding of the C ABI in include/osfm_hip.h (libosfm_hip.so).

There is no fallback: if the HIP library is not built the import of this
module raises, and every compute entry point raises OsfmError when the
library reports an error (e.g. no gfx950 device).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# OSFM_HIP_LIBRARY: another build of the same library (kernel experiments)
LIB_PATH = os.environ.get("OSFM_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libosfm_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). orthosfm_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH)
# The HIP runtime the library is bound to, taken now: a torch imported later brings a second copy
# of the runtime (same soname, another file), and a later CDLL("libamdhip64.so") returns that copy,
# whose hipHostMalloc then reports no device.
_hip = C.CDLL("libamdhip64.so")


class OsfmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"osfm status {status}: {msg}")
        self.status = status


OK, E_ARG, E_DEVICE, E_RANGE, E_CAPACITY, E_STATE, E_NUMERIC, E_IO = 0, -1, -2, -3, -4, -5, -6, -7
MATCHER_EXHAUSTIVE, MATCHER_CASCADE_HASHING = 0, 1
RANSAC_FUNDAMENTAL, RANSAC_AFFINE = 0, 1
PAIR_MATCHED, PAIR_REJECTED_LOWRES, PAIR_REJECTED_COUNT, PAIR_SKIPPED_EMPTY, PAIR_REJECTED_INLIERS = 0, 1, 2, 3, 4


class MatchOptions(C.Structure):
    _fields_ = [("sift_lowe_ratio", C.c_float), ("sift_distance_threshold", C.c_float),
                ("surf_lowe_ratio", C.c_float), ("surf_distance_threshold", C.c_float),
                ("use_lowres_matching", C.c_int32), ("num_lowres_features", C.c_int32),
                ("min_lowres_matches", C.c_int32), ("min_feature_matches", C.c_int32),
                ("pairs_per_batch", C.c_int32),
                ("geometric_verification", C.c_int32), ("ransac_max_iterations", C.c_int32),
                ("ransac_threshold", C.c_double), ("min_matching_inliers", C.c_int32),
                ("matcher_type", C.c_int32), ("ransac_seed", C.c_uint64),
                ("cascade_keep_empty_blocks", C.c_int32), ("special_kernel_max", C.c_int32),
                ("ransac_model", C.c_int32), ("ransac_refit", C.c_int32)]


class RansacOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved", C.c_int32),
                ("threshold", C.c_double), ("seed", C.c_uint64)]


class RansacAffineOptions(C.Structure):
    """osfm_ransac_affine_options"""
    _fields_ = [("max_iterations", C.c_int32), ("refit", C.c_int32),
                ("threshold", C.c_double), ("seed", C.c_uint64)]


class RansacAffineResult(C.Structure):
    """osfm_ransac_affine_result"""
    _fields_ = [("best_iteration", C.c_int32), ("ransac_inliers", C.c_int32),
                ("refit_ran", C.c_int32), ("refit_accepted", C.c_int32)]


class GuidedOptions(C.Structure):
    """osfm_guided_options"""
    _fields_ = [("threshold", C.c_double), ("sift_lowe_ratio", C.c_float), ("surf_lowe_ratio", C.c_float),
                ("cap_from_seeds", C.c_int32), ("reserved", C.c_int32)]


class GuidedResult(C.Structure):
    """osfm_guided_result"""
    _fields_ = [("status", C.c_int32), ("num_seeds", C.c_int32), ("num_added", C.c_int32),
                ("max_candidates", C.c_int32), ("offset", C.c_int64)]


GUIDED_OK, GUIDED_TOO_FEW, GUIDED_DEGENERATE = 0, 1, 2


class Pair(C.Structure):
    _fields_ = [("view_1", C.c_int32), ("view_2", C.c_int32)]


class PairResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("lowres_matches", C.c_int32),
                ("num_matches", C.c_int32), ("num_inliers", C.c_int32), ("offset", C.c_int64)]


class MatchStats(C.Structure):
    _fields_ = [("tile_kernel_ms", C.c_double), ("tile_kernel_launches", C.c_int32),
                ("exact_scan_queries", C.c_int32), ("mac_count", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("lowres_kernel_ms", C.c_double),
                ("lowres_kernel_launches", C.c_int32), ("tile_workgroups", C.c_int32),
                ("lowres_mac_count", C.c_int64), ("cashash_kernel_ms", C.c_double),
                ("cashash_kernel_launches", C.c_int32), ("special_kernel_launches", C.c_int32),
                ("special_kernel_ms", C.c_double), ("tile_shader_cycles", C.c_double), ("tile_refclk_ticks", C.c_double),
                ("surf_tile_kernel_ms", C.c_double), ("surf_tile_kernel_launches", C.c_int32), ("reserved2", C.c_int32),
                ("surf_mac_count", C.c_int64)]


class MemoryReport(C.Structure):
    _fields_ = [("device_buffer_bytes", C.c_int64), ("pool_live_bytes", C.c_int64), ("pool_cached_bytes", C.c_int64),
                ("pinned_host_bytes", C.c_int64), ("live_matchers", C.c_int32), ("live_streams", C.c_int32),
                ("live_events", C.c_int32), ("reserved", C.c_int32)]


class BaProblem(C.Structure):
    _fields_ = [("model", C.c_int32), ("num_cameras", C.c_int32), ("num_points", C.c_int32),
                ("num_observations", C.c_int32),
                ("cam_params", C.c_void_p), ("cam_const", C.c_void_p),
                ("img_width", C.c_void_p), ("img_height", C.c_void_p),
                ("points", C.c_void_p), ("obs_xy", C.c_void_p),
                ("obs_camera", C.c_void_p), ("obs_point", C.c_void_p)]


class BaOptions(C.Structure):
    _fields_ = [("huber_delta", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("max_num_iterations", C.c_int32), ("optimize_points", C.c_int32),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("jacobi_scaling", C.c_int32), ("max_consecutive_invalid_steps", C.c_int32),
                ("device", C.c_int32), ("verbose", C.c_int32),
                ("retriangulate_points", C.c_int32), ("small_form", C.c_int32)]


class TracksSummary(C.Structure):
    _fields_ = [("num_tracks", C.c_int32), ("num_invalid_tracks", C.c_int32), ("num_features", C.c_int64)]


class OutlierStats(C.Structure):
    _fields_ = [("mean", C.c_double), ("sigma", C.c_double),
                ("num_with_point", C.c_int32), ("num_kept", C.c_int32)]


class BaSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("num_iterations", C.c_int32), ("num_successful_steps", C.c_int32),
                ("num_unsuccessful_steps", C.c_int32), ("termination", C.c_int32),
                ("mean_point_change", C.c_double), ("max_point_change", C.c_double),
                ("solve_ms", C.c_double), ("point_pass_ms", C.c_double),
                ("pair_pass_ms", C.c_double), ("cholesky_ms", C.c_double),
                ("back_pass_ms", C.c_double),
                ("linearizations", C.c_int32), ("num_pair_entries", C.c_int32),
                ("lm_loop_ms", C.c_double),
                ("flow_fallbacks", C.c_int32), ("order_arcs", C.c_int32),
                ("chain_blocks_natural", C.c_int32), ("chain_blocks", C.c_int32)]


class TkOptions(C.Structure):
    """osfm_tk_options"""
    _fields_ = [("sample_size", C.c_int32), ("max_iterations", C.c_int32), ("probability", C.c_double),
                ("inlier_ratio", C.c_double), ("min_consensus", C.c_int32), ("device", C.c_int32),
                ("max_error_px", C.c_double), ("seed", C.c_uint64)]


class TkResult(C.Structure):
    """osfm_tk_result"""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("usable_models", C.c_int32),
                ("supported_models", C.c_int32), ("best_iteration", C.c_int32), ("num_inliers", C.c_int32),
                ("mean_error_px", C.c_double), ("score_kernel_ms", C.c_double)]


TK_RANSAC, TK_FALLBACK, TK_TOO_FEW, TK_DEGENERATE = 0, 1, 2, 3


class ResectOptions(C.Structure):
    """osfm_resect_options"""
    _fields_ = [("max_iterations", C.c_int32), ("min_consensus", C.c_int32), ("probability", C.c_double),
                ("inlier_ratio", C.c_double), ("max_error_px", C.c_double), ("min_pivot", C.c_double),
                ("min_axis_ratio", C.c_double), ("estimate_scale", C.c_int32), ("device", C.c_int32),
                ("scale", C.c_double), ("seed", C.c_uint64)]


class ResectResult(C.Structure):
    """osfm_resect_result"""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("usable_models", C.c_int32),
                ("supported_models", C.c_int32), ("best_iteration", C.c_int32), ("ransac_inliers", C.c_int32),
                ("num_inliers", C.c_int32), ("refit_used", C.c_int32), ("mean_error_px", C.c_double),
                ("score_kernel_ms", C.c_double)]


RESECT_OK, RESECT_TOO_FEW, RESECT_NO_MODEL = 0, 1, 2

SIFT_MAX_OCTAVES = 16


class SiftOptions(C.Structure):
    """osfm_sift_options"""
    _fields_ = [("num_samples_per_octave", C.c_int32), ("min_octave", C.c_int32), ("max_octave", C.c_int32),
                ("contrast_threshold", C.c_float), ("edge_ratio_threshold", C.c_float),
                ("base_blur_sigma", C.c_float), ("inherent_blur_sigma", C.c_float), ("max_keypoints", C.c_int32)]


class SiftSummary(C.Structure):
    """osfm_sift_summary"""
    _fields_ = [("num_candidates", C.c_int32), ("num_keypoints", C.c_int32), ("num_descriptors", C.c_int32),
                ("num_octaves", C.c_int32),
                ("keypoints_per_octave", C.c_int32 * SIFT_MAX_OCTAVES),
                ("descriptors_per_octave", C.c_int32 * SIFT_MAX_OCTAVES)] + \
               [(n, C.c_double) for n in ("scale_space_ms", "extrema_ms", "localisation_ms", "orientation_ms",
                                          "descriptor_ms", "total_ms")]


SURF_OCTAVES = 4


class SurfOptions(C.Structure):
    """osfm_surf_options"""
    _fields_ = [("contrast_threshold", C.c_float), ("use_upright_descriptor", C.c_int32), ("max_keypoints", C.c_int32)]


class SurfSummary(C.Structure):
    """osfm_surf_summary"""
    _fields_ = [("num_candidates", C.c_int32), ("num_keypoints", C.c_int32), ("num_descriptors", C.c_int32),
                ("num_guarded", C.c_int32),
                ("keypoints_per_octave", C.c_int32 * SURF_OCTAVES),
                ("descriptors_per_octave", C.c_int32 * SURF_OCTAVES)] + \
               [(n, C.c_double) for n in ("sat_ms", "response_ms", "extrema_ms", "localisation_ms", "orientation_ms",
                                          "descriptor_ms", "total_ms")]


FEATURE_SIFT, FEATURE_SURF, FEATURE_ALL = 1, 2, 3


class ViewOptions(C.Structure):
    """osfm_view_options"""
    _fields_ = [("downscale_factor", C.c_int32), ("max_image_size", C.c_int32), ("feature_types", C.c_int32)]


class ViewSummary(C.Structure):
    """osfm_view_summary"""
    _fields_ = [(n, C.c_int32) for n in ("import_width", "import_height", "feature_width", "feature_height", "num_halvings",
                                         "num_sift", "num_surf", "reserved")] + \
               [("sift", SiftSummary), ("surf", SurfSummary)] + \
               [(n, C.c_double) for n in ("halving_ms", "view_ms", "total_ms")]


MARK_TRACKS, MARK_FEATURES = 0, 1
CLAMP_REFERENCE, CLAMP_IMAGE = 0, 1
MARK_IN, MARK_OUTSIDE = 1, 2


class ViewMarkOptions(C.Structure):
    """osfm_view_mark_options"""
    _fields_ = [(n, C.c_int32) for n in ("mode", "clamp", "threshold", "pixel_width")]


class ViewMarkSummary(C.Structure):
    """osfm_view_mark_summary"""
    _fields_ = [(n, C.c_int32) for n in ("masked_out_sift", "masked_out_surf", "outside", "kept_sift", "kept_surf", "has_mask",
                                         "pixel_width", "reserved")]


class ViewBank(C.Structure):
    """osfm_view_bank (test hook osfm_match_debug_view_bank)."""
    COUNTS = ("n_sift", "n_surf", "n_sift_pad", "n_surf_pad", "n_special", "n_special_pad", "surf_norm2_max", "n_positions")
    ARRAYS = ("sift", "sift_raw", "special", "surf", "sift_corr", "sift_raw_corr", "special_corr", "special_map", "special_slot",
              "surf_corr", "positions")
    _fields_ = [(n, C.c_int32) for n in COUNTS] + [(n, C.c_void_p) for n in ARRAYS]


class BaLinCapture(C.Structure):
    """osfm_ba_lin_capture (test hook osfm_ba_debug_linearization)."""
    ARRAYS = ("scale_c", "diag_c", "S", "rhs", "scale_p", "diag_p", "vinv", "ge", "y_c", "cand_cams", "cand_points")
    _fields_ = [(n, C.c_void_p) for n in ARRAYS] + [("nc", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.c_double) for n in ("initial_cost", "grad_max", "radius", "model_cost_change", "cand_cost",
                                          "relative_decrease")] + \
               [(n, C.c_int32) for n in ("stopped", "accepted", "flow_aborted", "num_pad")] + \
               [(n, C.c_double) for n in ("pad_diag_min", "pad_diag_max", "pad_off_max")] + \
               [(n, C.c_int32) for n in ("win_num", "win_over", "small_lists", "dense", "dense_splits", "num_pairs", "pair_chunk",
                                         "max_chunks", "multi_chunk_pairs", "order_arcs", "span", "N", "small_solve",
                                         "one_launch", "post_fused", "back_fused")]


class BaCovOptions(C.Structure):
    """osfm_ba_cov_options."""
    _fields_ = [("huber_delta", C.c_double), ("min_pivot_ratio", C.c_double), ("optimize_points", C.c_int32),
                ("depth_gauge", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32)]


class BaCovResult(C.Structure):
    """osfm_ba_cov_result: the caller's arrays (any may be None), then what the call fills in."""
    ARRAYS = ("cam_cov", "cam_ldim", "cam_cov_full", "point_cov", "point_valid")
    _fields_ = [(n, C.c_void_p) for n in ARRAYS] + [("nc", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.c_double) for n in ("cost", "variance_factor", "min_pivot_seen")] + \
               [(n, C.c_int32) for n in ("num_residuals", "num_unknowns", "num_camera_unknowns", "num_valid_points",
                                         "gauge_camera", "gauge_axis", "rank_deficient", "dense_schur")] + \
               [(n, C.c_double) for n in ("linearize_ms", "factor_ms", "inverse_ms", "point_ms", "total_ms")]


BA_COV_MAX_UNKNOWNS = 8192


class ConsensusOptions(C.Structure):
    """osfm_consensus_options."""
    _fields_ = [("max_error", C.c_double), ("min_support", C.c_int32), ("max_sample", C.c_int32),
                ("refit_rounds", C.c_int32), ("device", C.c_int32)]


class ConsensusLimits(C.Structure):
    """osfm_consensus_limits."""
    _fields_ = [(n, C.c_int32) for n in ("short_length", "short_tracks", "long_tracks", "max_sample")]


class ConsensusStats(C.Structure):
    """osfm_consensus_stats."""
    COUNTERS = ("tracks_tested", "tracks_clean", "tracks_repaired", "tracks_unsupported", "tracks_degenerate",
                "tracks_unsettled", "obs_tested", "obs_dropped", "hypotheses_scored")
    _fields_ = [(n, C.c_int64) for n in COUNTERS] + [("device_ms", C.c_double)]

    def counters(self) -> dict:
        return {n: int(getattr(self, n)) for n in self.COUNTERS}


CONSENSUS_UNTESTED, CONSENSUS_CLEAN, CONSENSUS_REPAIRED, CONSENSUS_UNSUPPORTED, CONSENSUS_DEGENERATE = 0, 1, 2, 3, 4
CONSENSUS_MAX_REFIT_ROUNDS = 16

class RefineOptions(C.Structure):
    """osfm_refine_options."""
    _fields_ = [("radius", C.c_int32), ("max_iterations", C.c_int32)] + \
               [(n, C.c_double) for n in ("step", "eps", "min_contrast", "max_shift", "max_deform", "min_score", "min_pivot")]


REFINE_STATUS = ("untested", "reference", "refined", "outside", "flat", "ill_conditioned", "not_converged", "reject_shift",
                 "reject_deform", "reject_score")
(REFINE_UNTESTED, REFINE_REFERENCE, REFINE_REFINED, REFINE_OUTSIDE, REFINE_FLAT, REFINE_ILL_CONDITIONED, REFINE_NOT_CONVERGED,
 REFINE_REJECT_SHIFT, REFINE_REJECT_DEFORM, REFINE_REJECT_SCORE) = range(10)


class RefineStats(C.Structure):
    """osfm_refine_stats."""
    _fields_ = [("status_count", C.c_int64 * len(REFINE_STATUS)), ("iterations", C.c_int64), ("device_ms", C.c_double)]

    def counters(self) -> dict:
        d = {n: int(self.status_count[i]) for i, n in enumerate(REFINE_STATUS)}
        d["iterations"] = int(self.iterations)
        return d


class DenseOptions(C.Structure):
    """osfm_dense_options."""
    _fields_ = [(n, C.c_int32) for n in ("radius", "min_sources", "min_consistent", "reserved")] + \
               [(n, C.c_double) for n in ("min_contrast", "min_score", "consistency_tol")]


DENSE_STATUS = ("ok", "border", "flat", "no_sources", "low_score", "range_edge", "inconsistent", "duplicate")
(DENSE_OK, DENSE_BORDER, DENSE_FLAT, DENSE_NO_SOURCES, DENSE_LOW_SCORE, DENSE_RANGE_EDGE, DENSE_INCONSISTENT,
 DENSE_DUPLICATE) = range(8)


class DenseStats(C.Structure):
    """osfm_dense_stats."""
    _fields_ = [("status_count", C.c_int64 * len(DENSE_STATUS)), ("samples", C.c_int64), ("device_ms", C.c_double)]

    def counters(self) -> dict:
        return {n: int(self.status_count[i]) for i, n in enumerate(DENSE_STATUS)}


class DenseMeshOptions(C.Structure):
    """osfm_dense_mesh_options."""
    _fields_ = [("dd_factor", C.c_double)] + [(n, C.c_int32) for n in ("confidence_iterations", "min_island", "use_fused", "refined_normals")]


MESH_VERTEX_SIMPLE, MESH_VERTEX_BORDER, MESH_VERTEX_COMPLEX = range(3)
MESH_STAGES = ("label", "triangles", "vertices", "confidence", "emit")


class DenseMeshStats(C.Structure):
    """osfm_dense_mesh_stats."""
    _fields_ = [(n, C.c_int64) for n in ("pixels_solid", "pixels_island", "components", "triangles_dropped", "vertices_simple",
                                         "vertices_border", "vertices_complex")] + \
               [("threshold_steps", C.c_double), ("device_ms", C.c_double), ("stage_ms", C.c_double * len(MESH_STAGES))]

    def counters(self) -> dict:
        return {n: int(getattr(self, n)) for n, t in self._fields_ if t is C.c_int64}


class DenseRefineOptions(C.Structure):
    """osfm_dense_refine_options."""
    _fields_ = [(n, C.c_int32) for n in ("radius", "min_sources", "max_iterations", "reserved")] + \
               [(n, C.c_double) for n in ("eps", "max_shift", "max_deform", "min_score", "min_pivot")]


DENSE_REFINE_STATUS = ("not_ok", "refined", "outside", "ill_conditioned", "not_converged", "reject_shift", "reject_slope", "reject_score")
(DENSE_REFINE_NOT_OK, DENSE_REFINE_REFINED, DENSE_REFINE_OUTSIDE, DENSE_REFINE_ILL_CONDITIONED, DENSE_REFINE_NOT_CONVERGED,
 DENSE_REFINE_REJECT_SHIFT, DENSE_REFINE_REJECT_SLOPE, DENSE_REFINE_REJECT_SCORE) = range(8)


class DenseRefineStats(C.Structure):
    """osfm_dense_refine_stats."""
    _fields_ = [("status_count", C.c_int64 * len(DENSE_REFINE_STATUS)), ("iterations", C.c_int64), ("samples", C.c_int64),
                ("device_ms", C.c_double)]

    def counters(self) -> dict:
        d = {n: int(self.status_count[i]) for i, n in enumerate(DENSE_REFINE_STATUS)}
        d["iterations"] = int(self.iterations)
        return d


# every symbol include/osfm_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "osfm_last_error", "osfm_version", "osfm_device_count", "osfm_device_memory", "osfm_library_memory", "osfm_trim_device_memory", "osfm_ransac_selfcheck", "osfm_ba_debug_chol_trace", "osfm_ba_debug_flow_spin_limit", "osfm_ba_debug_order",
    "osfm_ba_debug_cholesky_solve", "osfm_ba_debug_linearization",
    "osfm_match_options_default", "osfm_match_create", "osfm_match_create_multi", "osfm_match_get_devices", "osfm_match_destroy",
    "osfm_quantize_sift", "osfm_quantize_surf",
    "osfm_match_set_view", "osfm_match_set_view_float", "osfm_match_view_size", "osfm_match_expect_pairs", "osfm_match_set_positions",
    "osfm_ransac_options_default", "osfm_ransac_fundamental", "osfm_ransac_affine_options_default", "osfm_ransac_affine",
    "osfm_guided_options_default", "osfm_guided_limits", "osfm_match_guided",
    "osfm_match_pair", "osfm_match_pair_lowres", "osfm_match_twoway", "osfm_match_all",
    "osfm_pair_from_index", "osfm_match_get_stats", "osfm_match_get_shard_stats", "osfm_match_get_cascade_hashes",
    "osfm_ba_options_default", "osfm_ba_small_limits", "osfm_ba_solve", "osfm_ba_reprojection_errors",
    "osfm_ba_triangulate", "osfm_ba_cov_options_default", "osfm_ba_covariance", "osfm_scene_covariance",
    "osfm_nn_distances", "osfm_filter_outlier_tracks", "osfm_filter_reprojection",
    "osfm_consensus_options_default", "osfm_consensus_get_limits", "osfm_ba_consensus", "osfm_scene_filter_consensus",
    "osfm_scene_create", "osfm_scene_destroy", "osfm_scene_set_flags", "osfm_scene_align_views", "osfm_scene_set_cameras", "osfm_scene_get_cameras",
    "osfm_scene_triangulate", "osfm_scene_filter_reprojection", "osfm_scene_local_adjustment", "osfm_scene_global_adjustment",
    "osfm_scene_filter_outliers", "osfm_scene_download",
    "osfm_tk_options_default", "osfm_tk_align", "osfm_tk_resolve_ambiguity", "osfm_scene_tk_align",
    "osfm_resect_options_default", "osfm_resect_limits", "osfm_resect_view", "osfm_scene_resect_view",
    "osfm_tracks_compute", "osfm_tracks_compute_ranges", "osfm_build_groups",
    "osfm_tracks_builder_create", "osfm_tracks_builder_feed", "osfm_tracks_builder_finish", "osfm_tracks_builder_destroy",
    "osfm_tracks_select_observations",
    "osfm_tracks_feature_table",
    "osfm_tracks_file_write", "osfm_tracks_file_read", "osfm_tracks_pairwise_files_write",
    "osfm_tracks_from_mve", "osfm_cameras_file_write", "osfm_cameras_file_read",
    "osfm_sparse_cloud_write", "osfm_time_measurements_write", "osfm_time_measurements_read",
    "osfm_sift_options_default", "osfm_sift_create", "osfm_sift_destroy", "osfm_sift_extract", "osfm_sift_download",
    "osfm_sift_debug_image", "osfm_sift_debug_keypoints",
    "osfm_surf_options_default", "osfm_surf_create", "osfm_surf_destroy", "osfm_surf_extract", "osfm_surf_download",
    "osfm_surf_debug_image", "osfm_surf_debug_keypoints", "osfm_surf_debug_describe",
    "osfm_view_options_default", "osfm_view_front_create", "osfm_view_front_destroy", "osfm_view_front_load",
    "osfm_view_front_download", "osfm_view_front_debug_image", "osfm_match_set_view_from_front",
    "osfm_match_debug_view_bank", "osfm_match_debug_set_view_device",
    "osfm_view_mark_options_default", "osfm_view_front_load_marked", "osfm_view_front_download_marks", "osfm_view_debug_mark_rows",
    "osfm_tracks_filter_marked",
    "osfm_refine_options_default", "osfm_refine_create", "osfm_refine_destroy", "osfm_refine_set_image",
    "osfm_refine_set_image_from_front", "osfm_refine_tracks",
    "osfm_dense_options_default", "osfm_dense_limits", "osfm_dense_debug_ablation", "osfm_dense_create", "osfm_dense_destroy", "osfm_dense_set_image",
    "osfm_dense_set_image_from_front", "osfm_dense_set_cameras", "osfm_dense_sweep", "osfm_dense_fuse",
    "osfm_dense_download_status", "osfm_dense_download_cloud", "osfm_dense_cloud_write",
    "osfm_dense_set_map", "osfm_dense_mesh_options_default", "osfm_dense_mesh_limits", "osfm_dense_mesh_view",
    "osfm_dense_download_mesh", "osfm_dense_mesh_write",
    "osfm_dense_refine_options_default", "osfm_dense_refine_view", "osfm_dense_download_refined",
]

# osfm_track_feature as a numpy record (32 bytes, no padding)
TRACK_FEATURE = np.dtype([("view_id", "<u4"), ("local_feature_id", "<u4"), ("global_feature_id", "<u4"),
                          ("x", "<f4"), ("y", "<f4"), ("r", "<u4"), ("g", "<u4"), ("b", "<u4")])

lib.osfm_last_error.restype = C.c_char_p
lib.osfm_version.restype = C.c_int
# include/osfm_hip.h OSFM_ABI_VERSION: the structs below mirror THAT header, and the library writes them in full
ABI_VERSION = 102
# The header binds the entries that take an osfm_match_options to these symbols (the struct grew; the plain names keep
# the earlier layout for binaries built before that): this module and matching.py call them by these names.
for _name in ("osfm_match_options_default_v2", "osfm_match_create_v2", "osfm_match_create_multi_v2"):
    if not hasattr(lib, _name):
        raise ImportError(f"libosfm_hip.so lacks {_name} (rebuild: make -C orthosfm_amd/csrc)")
if lib.osfm_version() != ABI_VERSION and os.environ.get("OSFM_ALLOW_ABI_MISMATCH") != "1":
    raise ImportError(f"libosfm_hip.so reports ABI version {lib.osfm_version()}, orthosfm_amd/capi.py mirrors {ABI_VERSION} "
                      "(rebuild: make -C orthosfm_amd/csrc; experiments with an older build: OSFM_ALLOW_ABI_MISMATCH=1)")
lib.osfm_device_count.restype = C.c_int
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
lib.osfm_sift_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(SiftOptions), C.POINTER(C.c_void_p)]
lib.osfm_sift_destroy.argtypes = [C.c_void_p]
lib.osfm_sift_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SiftSummary)]
lib.osfm_sift_download.argtypes = [C.c_void_p] + [C.c_void_p] * 6
lib.osfm_sift_debug_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]
lib.osfm_sift_debug_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
lib.osfm_surf_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(SurfOptions), C.POINTER(C.c_void_p)]
lib.osfm_surf_destroy.argtypes = [C.c_void_p]
lib.osfm_surf_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(SurfSummary)]
lib.osfm_surf_download.argtypes = [C.c_void_p] + [C.c_void_p] * 6
lib.osfm_surf_debug_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
lib.osfm_surf_debug_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
lib.osfm_surf_debug_describe.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                         C.POINTER(C.c_int32)]
lib.osfm_view_front_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(ViewOptions), C.POINTER(SiftOptions),
                                       C.POINTER(SurfOptions), C.POINTER(C.c_void_p)]
lib.osfm_view_front_destroy.argtypes = [C.c_void_p]
lib.osfm_view_front_load.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ViewSummary)]
lib.osfm_view_front_download.argtypes = [C.c_void_p] + [C.c_void_p] * 7
lib.osfm_view_front_load_marked.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.POINTER(ViewMarkOptions), C.POINTER(ViewSummary), C.POINTER(ViewMarkSummary)]
lib.osfm_view_front_download_marks.argtypes = [C.c_void_p] + [C.c_void_p] * 3
lib.osfm_view_debug_mark_rows.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                          C.POINTER(ViewMarkOptions), C.c_void_p, C.c_void_p, C.c_void_p]
lib.osfm_tracks_filter_marked.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int64)]
lib.osfm_view_front_debug_image.argtypes = [C.c_void_p, C.c_void_p] + [C.POINTER(C.c_int32)] * 3
lib.osfm_match_set_view_from_front.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
lib.osfm_match_debug_view_bank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(ViewBank)]
lib.osfm_match_debug_set_view_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p]
lib.osfm_ba_small_limits.argtypes = [C.POINTER(C.c_int32)] * 3
lib.osfm_resect_limits.argtypes = [C.POINTER(C.c_int32)] * 2
lib.osfm_resect_view.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.osfm_scene_resect_view.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
lib.osfm_guided_limits.argtypes = [C.POINTER(C.c_int32)] * 3
lib.osfm_match_guided.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GuidedOptions),
                                  C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
lib.osfm_ba_cov_options_default.argtypes = [C.POINTER(BaCovOptions)]
lib.osfm_ba_covariance.argtypes = [C.c_void_p, C.POINTER(BaCovOptions), C.POINTER(BaCovResult)]
lib.osfm_scene_covariance.argtypes = [C.c_void_p, C.POINTER(BaCovOptions), C.POINTER(BaCovResult)]
lib.osfm_consensus_options_default.restype = None
lib.osfm_consensus_options_default.argtypes = [C.POINTER(ConsensusOptions)]
lib.osfm_consensus_get_limits.restype = None
lib.osfm_consensus_get_limits.argtypes = [C.POINTER(ConsensusLimits)]
lib.osfm_ba_consensus.argtypes = [C.c_void_p, C.POINTER(ConsensusOptions)] + [C.c_void_p] * 5 + [C.POINTER(ConsensusStats)]
lib.osfm_scene_filter_consensus.argtypes = [C.c_void_p, C.POINTER(ConsensusOptions), C.POINTER(ConsensusStats)]
lib.osfm_refine_options_default.argtypes = [C.POINTER(RefineOptions)]
lib.osfm_refine_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
lib.osfm_refine_destroy.argtypes = [C.c_void_p]
lib.osfm_refine_set_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
lib.osfm_refine_set_image_from_front.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
lib.osfm_refine_tracks.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.POINTER(RefineOptions)] + [C.c_void_p] * 5 + \
                                  [C.POINTER(RefineStats)]
lib.osfm_dense_options_default.argtypes = [C.POINTER(DenseOptions)]
lib.osfm_dense_limits.argtypes = [C.POINTER(C.c_int32)] * 5
lib.osfm_dense_debug_ablation.argtypes = [C.c_int]
lib.osfm_dense_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
lib.osfm_dense_destroy.argtypes = [C.c_void_p]
lib.osfm_dense_set_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
lib.osfm_dense_set_image_from_front.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
lib.osfm_dense_set_cameras.argtypes = [C.c_void_p, C.c_void_p]
lib.osfm_dense_sweep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, C.POINTER(DenseOptions),
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenseStats)]
lib.osfm_dense_fuse.argtypes = [C.c_void_p, C.POINTER(DenseOptions), C.POINTER(C.c_int64), C.POINTER(DenseStats)]
lib.osfm_dense_download_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
lib.osfm_dense_download_cloud.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
lib.osfm_dense_cloud_write.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p]
lib.osfm_dense_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
lib.osfm_dense_refine_options_default.argtypes = [C.POINTER(DenseRefineOptions)]
lib.osfm_dense_refine_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(DenseRefineOptions)] + [C.c_void_p] * 5 + \
                                      [C.POINTER(DenseRefineStats)]
lib.osfm_dense_download_refined.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
lib.osfm_dense_mesh_options_default.argtypes = [C.POINTER(DenseMeshOptions)]
lib.osfm_dense_mesh_limits.argtypes = [C.POINTER(C.c_int32)] * 3
lib.osfm_dense_mesh_view.argtypes = [C.c_void_p, C.c_int, C.POINTER(DenseMeshOptions), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(DenseMeshStats)]
lib.osfm_dense_download_mesh.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 7
lib.osfm_dense_mesh_write.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p]
lib.osfm_ba_debug_cholesky_solve.restype = C.c_int
lib.osfm_ba_debug_cholesky_solve.argtypes = [C.c_int, C.c_int, _f64p, _f64p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_int, C.c_int, C.c_int, _f64p, _i32p, _i32p]


def last_error() -> str:
    return lib.osfm_last_error().decode()


def check(status):
    if status != OK:
        raise OsfmError(status, last_error())


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None and a.size else None


def device_count() -> int:
    return lib.osfm_device_count()


def ransac_selfcheck(mode: int):
    """Sets the scoring mode of the RANSAC kernel (0 double, 1 pre-classified, 2 checked) and
    returns (wrong, undecided, tests) counted in mode 2 since the previous call."""
    c = (C.c_uint64 * 3)()
    check(lib.osfm_ransac_selfcheck(C.c_int(mode), c))
    return int(c[0]), int(c[1]), int(c[2])


_pinned_blocks = {}        # address -> the ctypes view that keeps the block reachable


def pinned_rows(rows: int):
    """A (rows, 2) int32 array in page-locked host memory (hipHostMalloc of the HIP runtime the
    library is linked against), e.g. as the result buffer of HipExhaustiveMatching.compute: the
    match lists then leave the device at full PCIe rate instead of through pageable staging.
    Lives until pinned_free (or as long as the process)."""
    p = C.c_void_p()
    nbytes = max(int(rows), 1) * 8
    rc = _hip.hipHostMalloc(C.byref(p), C.c_size_t(nbytes), C.c_uint(0))
    if rc != 0 or not p.value:
        raise OsfmError(E_DEVICE, f"hipHostMalloc({nbytes}) failed with {rc}")
    buf = (C.c_int32 * (max(int(rows), 1) * 2)).from_address(p.value)
    _pinned_blocks[p.value] = buf
    return np.frombuffer(buf, dtype=np.int32).reshape(-1, 2)[:rows]


def pinned_free(arr) -> bool:
    """Gives a pinned_rows block back (the caller drops its views of it); False when it is not one."""
    addr = int(arr.ctypes.data)
    if _pinned_blocks.pop(addr, None) is None:
        return False
    _hip.hipHostFree(C.c_void_p(addr))
    return True


def trim_device_memory(device: int = -1) -> int:
    """Hands the cached work-array memory back to the driver; returns the bytes released."""
    b = C.c_uint64()
    check(lib.osfm_trim_device_memory(C.c_int(device), C.byref(b)))
    return b.value


def device_memory(device: int = 0):
    """(free, total) bytes of the device's HBM."""
    f, t = C.c_uint64(), C.c_uint64()
    check(lib.osfm_device_memory(device, C.byref(f), C.byref(t)))
    return f.value, t.value


def library_memory() -> MemoryReport:
    """What the library itself holds in this process (osfm_library_memory)."""
    r = MemoryReport()
    check(lib.osfm_library_memory(C.byref(r)))
    return r


def default_match_options() -> MatchOptions:
    o = MatchOptions()
    check(lib.osfm_match_options_default_v2(C.byref(o)))      # the symbol the header binds: MatchOptions in full
    return o


def default_guided_options() -> GuidedOptions:
    o = GuidedOptions()
    check(lib.osfm_guided_options_default(C.byref(o)))
    return o


def guided_limits():
    """(queries_per_workgroup, positions_per_chunk, candidates_per_pass) of the guided matching kernel."""
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.osfm_guided_limits(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def default_consensus_options(**kw) -> ConsensusOptions:
    """osfm_consensus_options_default with the given fields replaced."""
    o = ConsensusOptions()
    lib.osfm_consensus_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"osfm_consensus_options has no field {k!r}")
        setattr(o, k, v)
    return o


def consensus_limits() -> ConsensusLimits:
    l = ConsensusLimits()
    lib.osfm_consensus_get_limits(C.byref(l))
    return l


def default_refine_options(**kw) -> RefineOptions:
    """osfm_refine_options_default with the given fields replaced."""
    o = RefineOptions()
    check(lib.osfm_refine_options_default(C.byref(o)))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"osfm_refine_options has no field {k!r}")
        setattr(o, k, v)
    return o


def default_dense_options(**kw) -> DenseOptions:
    """osfm_dense_options_default with the given fields replaced."""
    o = DenseOptions()
    check(lib.osfm_dense_options_default(C.byref(o)))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"osfm_dense_options has no field {k!r}")
        setattr(o, k, v)
    return o


def default_dense_mesh_options(**kw) -> DenseMeshOptions:
    """osfm_dense_mesh_options_default with the given fields replaced."""
    o = DenseMeshOptions()
    check(lib.osfm_dense_mesh_options_default(C.byref(o)))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"osfm_dense_mesh_options has no field {k!r}")
        setattr(o, k, v)
    return o


def default_dense_refine_options(**kw) -> DenseRefineOptions:
    """osfm_dense_refine_options_default with the given fields replaced."""
    o = DenseRefineOptions()
    check(lib.osfm_dense_refine_options_default(C.byref(o)))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"osfm_dense_refine_options has no field {k!r}")
        setattr(o, k, v)
    return o


def dense_mesh_limits():
    """(label_tile_w, label_tile_h, max_confidence_iterations) of the mesh kernels."""
    v = [C.c_int32() for _ in range(3)]
    check(lib.osfm_dense_mesh_limits(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def dense_limits():
    """(tile_w, tile_h, max_radius, max_sources, max_depths) of the plane-sweep kernel."""
    v = [C.c_int32() for _ in range(5)]
    check(lib.osfm_dense_limits(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def default_sift_options() -> SiftOptions:
    o = SiftOptions()
    check(lib.osfm_sift_options_default(C.byref(o)))
    return o


def default_surf_options() -> SurfOptions:
    o = SurfOptions()
    check(lib.osfm_surf_options_default(C.byref(o)))
    return o


def default_view_options() -> ViewOptions:
    o = ViewOptions()
    check(lib.osfm_view_options_default(C.byref(o)))
    return o


def default_view_mark_options() -> ViewMarkOptions:
    o = ViewMarkOptions()
    check(lib.osfm_view_mark_options_default(C.byref(o)))
    return o


def quantize_sift(f: np.ndarray) -> np.ndarray:
    f = np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 128)
    out = np.zeros(f.shape, dtype=np.uint16)
    check(lib.osfm_quantize_sift(_ptr(f, C.c_float), f.shape[0], _ptr(out, C.c_uint16)))
    return out


def quantize_surf(f: np.ndarray) -> np.ndarray:
    f = np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 64)
    out = np.zeros(f.shape, dtype=np.int16)
    check(lib.osfm_quantize_surf(_ptr(f, C.c_float), f.shape[0], _ptr(out, C.c_int16)))
    return out


def pair_from_index(i: int):
    a, b = C.c_int32(), C.c_int32()
    check(lib.osfm_pair_from_index(C.c_int64(i), C.byref(a), C.byref(b)))
    return a.value, b.value
