"""SIFT feature extraction on the device (include/osfm_hip.h, "SIFT feature extraction").

    ex = SiftExtractor(device=0, max_width=2048, max_height=2048)
    f = ex.extract(image)                 # uint8 [h, w] or [h, w, 3]
    matcher.set_view_features(0, f)

The result is FeatureSet::compute_sift's: sorted by scale, descending.  Reading image files and the halving of
images beyond a maximum size stay with the caller.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi


@dataclass
class Features:
    descriptors: np.ndarray     # float32 [n, 128]
    positions: np.ndarray       # float32 [n, 2], x, y in pixels of the input image
    normalized: np.ndarray      # float32 [n, 2], FeatureSet::normalize_feature_positions
    scale: np.ndarray           # float32 [n]
    orientation: np.ndarray     # float32 [n], radians in [0, 2 pi]
    colors: np.ndarray          # uint8 [n, 3]

    def __len__(self):
        return self.descriptors.shape[0]


class SiftExtractor:
    """One context (osfm_sift): the pyramid and work arrays for images up to max_width x max_height.  The keyword
    options are the fields of osfm_sift_options (Sift::Options and max_keypoints)."""

    def __init__(self, device: int = 0, max_width: int = 2048, max_height: int = 2048, **opts):
        o = capi.default_sift_options()
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"SiftExtractor: unknown option {k!r}")
            setattr(o, k, v)
        self.options = o
        self.summary = None
        self._h = C.c_void_p()
        capi.check(capi.lib.osfm_sift_create(device, int(max_width), int(max_height), C.byref(o), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.check(capi.lib.osfm_sift_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, image) -> capi.SiftSummary:
        """osfm_sift_extract alone: the summary (counts and stage times); the result stays in the context."""
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim not in (2, 3):
            raise TypeError("SiftExtractor: an uint8 image [h, w] or [h, w, channels] is expected")
        image = np.ascontiguousarray(image)
        channels = 1 if image.ndim == 2 else image.shape[2]
        s = capi.SiftSummary()
        capi.check(capi.lib.osfm_sift_extract(self._h, image.ctypes.data, image.shape[1], image.shape[0], channels, C.byref(s)))
        self.summary = s
        return s

    def download(self) -> Features:
        """osfm_sift_download of the last run()."""
        n = self.summary.num_descriptors
        f = Features(np.zeros((n, 128), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32),
                     np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.uint8))
        capi.check(capi.lib.osfm_sift_download(self._h, f.descriptors.ctypes.data, f.positions.ctypes.data, f.scale.ctypes.data,
                                               f.orientation.ctypes.data, f.colors.ctypes.data, f.normalized.ctypes.data))
        return f

    def extract(self, image) -> Features:
        self.run(image)
        return self.download()

    # --- test hooks ---------------------------------------------------------------------------------------------
    def debug_image(self, octave: int, kind: int, index: int) -> np.ndarray:
        w, h = C.c_int32(), C.c_int32()
        capi.check(capi.lib.osfm_sift_debug_image(self._h, octave, kind, index, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        capi.check(capi.lib.osfm_sift_debug_image(self._h, octave, kind, index, out.ctypes.data, None, None))
        return out

    def debug_keypoints(self, after_localisation: bool) -> np.ndarray:
        n = C.c_int32()
        capi.check(capi.lib.osfm_sift_debug_keypoints(self._h, int(after_localisation), None, C.byref(n)))
        out = np.zeros((n.value, 4), np.float32)
        capi.check(capi.lib.osfm_sift_debug_keypoints(self._h, int(after_localisation), out.ctypes.data, None))
        return out
