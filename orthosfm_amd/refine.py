"""Sub-pixel refinement of track observations by affine least-squares patch matching (include/osfm_hip.h,
"Sub-pixel refinement"; DESIGN.md "Observation refinement").  No counterpart in the reference."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi
from .features import _Handle, _image_arg


@dataclass
class RefineResult:
    xy: np.ndarray            # float64 [F, 2]: the input position of every observation that is not REFINED
    affine: np.ndarray        # float64 [F, 4]: the refined warp of REFINED observations, the initial one elsewhere
    score: np.ndarray         # float64 [F]
    status: np.ndarray        # int32 [F]: capi.REFINE_*
    iterations: np.ndarray    # int32 [F]
    stats: capi.RefineStats

    @property
    def refined(self):
        return self.status == capi.REFINE_REFINED


def relative_affine(offsets, scale, orientation, alive=None):
    """init_affine for refine(): (s_t / s_r) Rot(theta_t - theta_r) of every observation against the first alive one
    of its track, from the detectors' scale and orientation per observation; float64 [F, 4]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    F = int(offsets[-1]) if offsets.size else 0
    scale = np.asarray(scale, dtype=np.float64).reshape(F)
    theta = np.asarray(orientation, dtype=np.float64).reshape(F)
    live = np.ones(F, bool) if alive is None else np.asarray(alive).astype(bool).reshape(F)
    lengths = np.diff(offsets)
    track_of = np.repeat(np.arange(lengths.shape[0]), lengths)
    # the first alive observation of every track (a track without one keeps its first)
    first = offsets[:-1].copy()
    idx = np.flatnonzero(live)
    if idx.size:
        t, pos = np.unique(track_of[idx], return_index=True)
        first[t] = idx[pos]
    ref = first[track_of]
    s = scale / scale[ref]
    d = theta - theta[ref]
    c, sn = s * np.cos(d), s * np.sin(d)
    return np.ascontiguousarray(np.stack([c, -sn, sn, c], axis=1))


class Refiner(_Handle):
    """One osfm_refiner: a grey image per view on the device, and refine() over tracks."""
    _prefix = "refine"

    def __init__(self, device: int = 0, num_views: int = 1):
        self.num_views = int(num_views)
        self._h = C.c_void_p()
        capi.check(capi.lib.osfm_refine_create(int(device), self.num_views, C.byref(self._h)))

    def set_image(self, view: int, image):
        """uint8 [h, w] or [h, w, 3] from host memory."""
        image, channels = _image_arg("Refiner", image)
        capi.check(capi.lib.osfm_refine_set_image(self._h, int(view), image.ctypes.data, image.shape[1], image.shape[0], channels))

    def set_image_from_front(self, view: int, front):
        """The feature image of a features.ViewFrontEnd's last load, device to device."""
        capi.check(capi.lib.osfm_refine_set_image_from_front(self._h, int(view), front._h))

    def refine(self, offsets, view, xy, alive=None, init_affine=None, **options) -> RefineResult:
        """osfm_refine_tracks: tracks as CSR offsets [T + 1] over observations with view [F] and xy [F, 2] in pixels of
        the view's image (pixel centres at integers); options: the fields of osfm_refine_options."""
        o = capi.default_refine_options(**options)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or offsets.shape[0] < 1:
            raise ValueError("Refiner.refine: offsets [T + 1]")
        F = int(offsets[-1])
        view = np.ascontiguousarray(view, dtype=np.int32).reshape(-1)
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        if view.shape[0] != F or xy.shape[0] != F:
            raise ValueError(f"Refiner.refine: {F} observations by the offsets, {view.shape[0]} views, {xy.shape[0]} positions")
        if alive is not None:
            alive = np.ascontiguousarray(np.asarray(alive).astype(np.uint8)).reshape(-1)
            if alive.shape[0] != F:
                raise ValueError("Refiner.refine: alive [F]")
        if init_affine is not None:
            init_affine = np.ascontiguousarray(init_affine, dtype=np.float64).reshape(-1, 4)
            if init_affine.shape[0] != F:
                raise ValueError("Refiner.refine: init_affine [F, 4]")
        res = RefineResult(np.zeros((F, 2)), np.zeros((F, 4)), np.zeros(F), np.zeros(F, np.int32), np.zeros(F, np.int32),
                           capi.RefineStats())
        p = lambda a: a.ctypes.data if a is not None else None
        capi.check(capi.lib.osfm_refine_tracks(self._h, offsets.shape[0] - 1, p(offsets), p(view), p(xy), p(alive), p(init_affine),
                                               C.byref(o), p(res.xy), p(res.affine), p(res.score), p(res.status), p(res.iterations),
                                               C.byref(res.stats)))
        return res
