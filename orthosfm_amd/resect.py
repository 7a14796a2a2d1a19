"""Placing one view against triangulated points: the deterministic RANSAC over affine cameras of
include/osfm_hip.h (osfm_resect_view).  The scene form is Scene.resect_view
(orthosfm_amd/scene.py)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi

STATUS_NAMES = {capi.RESECT_OK: "ok", capi.RESECT_TOO_FEW: "too few", capi.RESECT_NO_MODEL: "no model"}


@dataclass
class Placement:
    rotation: np.ndarray        # (3, 3) local -> world: columns x, y, z axis of the camera
    scale: float
    offsets: np.ndarray         # (2,)
    inlier: np.ndarray          # (N,) bool: inliers of the final camera
    status: int
    iterations: int
    usable_models: int
    supported_models: int
    best_iteration: int
    ransac_inliers: int
    num_inliers: int
    mean_error_px: float
    refit_used: int
    score_kernel_ms: float
    num_points: int


def options(max_iterations=0, probability=0.999, inlier_ratio=0.5, min_consensus=8, max_error_px=3.0, min_pivot=None,
            min_axis_ratio=0.5, estimate_scale=0, scale=1.0, seed=0, device=0) -> capi.ResectOptions:
    """min_pivot None: the library's default."""
    o = capi.ResectOptions()
    capi.check(capi.lib.osfm_resect_options_default(C.byref(o)))
    o.max_iterations, o.probability, o.inlier_ratio, o.min_consensus = max_iterations, probability, inlier_ratio, min_consensus
    o.max_error_px, o.min_axis_ratio, o.estimate_scale, o.scale = max_error_px, min_axis_ratio, int(estimate_scale), scale
    o.seed, o.device = seed, device
    if min_pivot is not None:
        o.min_pivot = min_pivot
    return o


def limits():
    """osfm_resect_limits: (tile, chunk) of the scoring kernel as built."""
    t, k = C.c_int32(), C.c_int32()
    capi.check(capi.lib.osfm_resect_limits(C.byref(t), C.byref(k)))
    return t.value, k.value


def _placement(rot, scale, off, inl, r, n):
    return Placement(rot, scale.value, off, inl[:n].astype(bool), r.status, r.iterations, r.usable_models, r.supported_models,
                     r.best_iteration, r.ransac_inliers, r.num_inliers, r.mean_error_px, r.refit_used, r.score_kernel_ms, n)


def resect(points, xy, img_width, img_height, stream_id=0, **opts) -> Placement:
    """points (N, 3), xy (N, 2): N points and their pixel positions in the view; opts as options()."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or xy.shape != (points.shape[0], 2):
        raise ValueError("resect: points is (N, 3), xy (N, 2)")
    n = int(points.shape[0])
    o = options(**opts)
    rot, off, scale = np.zeros((3, 3)), np.zeros(2), C.c_double()
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    r = capi.ResectResult()
    capi.check(capi.lib.osfm_resect_view(points.ctypes.data, xy.ctypes.data, n, int(img_width), int(img_height), C.byref(o),
                                         C.c_uint64(stream_id), rot.ctypes.data, C.byref(scale), off.ctypes.data,
                                         inl.ctypes.data, C.byref(r)))
    return _placement(rot, scale, off, inl, r, n)


def placement_to_params(model, placement) -> np.ndarray:
    """The camera parameter vector (as osfm_ba_problem.cam_params) of a placement: its rotation (through
    pipeline._set_cam_rotation, as tk.bases_to_params), offsets and scale."""
    from . import ba as B
    from .pipeline import _set_cam_rotation
    p = np.zeros(7)
    _set_cam_rotation(model, p, np.asarray(placement.rotation, dtype=np.float64).reshape(3, 3))
    o = 4 if model == B.MODEL_QUATERNION else 3
    p[o:o + 2] = placement.offsets
    p[o + 2] = placement.scale
    return p
