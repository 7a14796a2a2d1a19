"""Initial alignment of a camera group (ReconstructionAlgorithm::calculateInitialAlignment,
src/sfm/reconstruct.cpp:205): the deterministic RANSAC over Tomasi-Kanade factorisations of
include/osfm_hip.h (osfm_tk_align, osfm_tk_resolve_ambiguity).
The scene form is Scene.tk_align (orthosfm_amd/scene.py)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi

STATUS_NAMES = {capi.TK_RANSAC: "ransac", capi.TK_FALLBACK: "fallback", capi.TK_TOO_FEW: "too few",
                capi.TK_DEGENERATE: "degenerate"}


@dataclass
class Alignment:
    basis_1: np.ndarray         # (C, 3, 3): one rotation per camera, camera 0 the identity; the scored solution
    basis_2: np.ndarray         # its mirror image T B T, T = diag(1, 1, -1)
    offsets: np.ndarray         # (C, 2)
    inlier: np.ndarray          # (N,) bool
    status: int
    iterations: int
    usable_models: int
    supported_models: int
    best_iteration: int
    num_inliers: int
    mean_error_px: float
    score_kernel_ms: float
    num_tracks: int


def options(sample_size=10, max_iterations=0, probability=0.999, inlier_ratio=0.7, min_consensus=25,
            max_error_px=3.0, seed=0, device=0) -> capi.TkOptions:
    o = capi.TkOptions()
    capi.check(capi.lib.osfm_tk_options_default(C.byref(o)))
    o.sample_size, o.max_iterations, o.probability, o.inlier_ratio = sample_size, max_iterations, probability, inlier_ratio
    o.min_consensus, o.max_error_px, o.seed, o.device = min_consensus, max_error_px, seed, device
    return o


def _alignment(b1, b2, off, inl, r, n):
    return Alignment(b1, b2, off, inl[:n].astype(bool), r.status, r.iterations, r.usable_models, r.supported_models,
                     r.best_iteration, r.num_inliers, r.mean_error_px, r.score_kernel_ms, n)


def align(xy, img_width, img_height, group_id=0, **opts) -> Alignment:
    """xy (N, C, 2): pixel positions of N tracks that all C cameras see (3 <= C <= 8); opts as options()."""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    if xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError("align: xy is (tracks, cameras, 2)")
    n, c = int(xy.shape[0]), int(xy.shape[1])
    o = options(**opts)
    b1, b2, off = np.zeros((max(c, 1), 3, 3)), np.zeros((max(c, 1), 3, 3)), np.zeros((max(c, 1), 2))
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    r = capi.TkResult()
    capi.check(capi.lib.osfm_tk_align(xy.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(n), C.c_int32(c),
                                      C.c_int32(img_width), C.c_int32(img_height), C.byref(o), C.c_uint64(group_id),
                                      capi._ptr(b1, C.c_double), capi._ptr(b2, C.c_double), capi._ptr(off, C.c_double),
                                      capi._ptr(inl, C.c_uint8), C.byref(r)))
    return _alignment(b1, b2, off, inl, r, n)


def resolve_ambiguity(basis_1, basis_2, global_rotation, has_global) -> int:
    """1 or 2: which of the two mirror solutions agrees with the global cameras (local -> world rotations
    global_rotation[c] of the views with has_global[c])."""
    b1 = np.ascontiguousarray(basis_1, dtype=np.float64).reshape(-1, 9)
    b2 = np.ascontiguousarray(basis_2, dtype=np.float64).reshape(-1, 9)
    g = np.ascontiguousarray(global_rotation, dtype=np.float64).reshape(-1, 9)
    hg = np.ascontiguousarray(has_global, dtype=np.uint8)
    if not (b1.shape == b2.shape == g.shape and hg.shape[0] == b1.shape[0]):
        raise ValueError("resolve_ambiguity: one matrix and one flag per camera")
    choice = C.c_int32()
    capi.check(capi.lib.osfm_tk_resolve_ambiguity(C.c_int32(b1.shape[0]), capi._ptr(b1, C.c_double), capi._ptr(b2, C.c_double),
                                                  capi._ptr(g, C.c_double), capi._ptr(hg, C.c_uint8), C.byref(choice)))
    return choice.value


def bases_to_params(model, bases) -> np.ndarray:
    """Camera parameter vectors (as osfm_ba_problem.cam_params) of the rotations `bases` (local -> world, as
    osfm_tk_align returns them), with offsets 0 and scale 1 as the reference's fresh cameras have
    (basisVectorToCameraVector, tomasi_kanade.cpp:169-191)."""
    from . import ba as B
    from .pipeline import _set_cam_rotation
    bases = np.asarray(bases, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros((bases.shape[0], 7))
    for p, R in zip(out, bases):
        _set_cam_rotation(model, p, R)
        p[6 if model == B.MODEL_QUATERNION else 5] = 1.0
    return out
