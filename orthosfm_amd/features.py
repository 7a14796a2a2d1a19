"""SIFT and SURF feature extraction on the device (include/osfm_hip.h, "SIFT feature extraction" and "SURF feature
extraction").

    ex = FeatureSetExtractor(device=0, max_width=2048, max_height=2048)
    fs = ex.extract(image)                # uint8 [h, w] or [h, w, 3]; fs.sift, fs.surf
    matcher.set_view_features(0, fs)

    f = SiftExtractor(0, 2048, 2048).extract(image)      # one detector alone; SurfExtractor likewise

    front = ViewFrontEnd(device=0, max_width=4096, max_height=4096)     # include/osfm_hip.h, "View front end"
    front.load(image)                     # one upload: halving chain, both detectors, colours and positions
    matcher.set_view_from_front(0, front) # the bank is made on the device; front.download() for the host's copy

A FeatureSet is the reference's with FEATURE_ALL: SIFT rows, then SURF rows, each sorted by scale, descending.
The extractors take the image as the detectors see it.  ViewFrontEnd is bundler::Features::compute from a decoded
image: it halves the image downscale_factor - 1 times and then while it holds more than max_image_size pixels, on
the device.  Reading image files stays with the caller.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi


@dataclass
class Features:
    descriptors: np.ndarray     # float32 [n, 128] (SIFT) or [n, 64] (SURF)
    positions: np.ndarray       # float32 [n, 2], x, y in pixels of the input image
    normalized: np.ndarray      # float32 [n, 2], FeatureSet::normalize_feature_positions
    scale: np.ndarray           # float32 [n]
    orientation: np.ndarray     # float32 [n], radians: SIFT in [0, 2 pi], SURF in [-pi, pi]
    colors: np.ndarray          # uint8 [n, 3]

    def __len__(self):
        return self.descriptors.shape[0]


def _image_arg(who, image):
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3):
        raise TypeError(f"{who}: an uint8 image [h, w] or [h, w, channels] is expected")
    image = np.ascontiguousarray(image)
    return image, 1 if image.ndim == 2 else image.shape[2]


class _Handle:
    """The life cycle of one C context, self._h: closed once, by hand, by `with` or with the object."""
    _prefix = None              # the C functions are osfm_<prefix>_*

    def _c(self, name):
        return getattr(capi.lib, f"osfm_{self._prefix}_{name}")

    def close(self):
        if self._h:
            capi.check(self._c("destroy")(self._h))
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


class _Detector(_Handle):
    """What SiftExtractor and SurfExtractor share: one context for images up to max_width x max_height, whose keyword
    options are the fields of the detector's options struct."""
    _options = _summary = _width = None     # the options factory, the summary type, floats per descriptor

    def __init__(self, device: int = 0, max_width: int = 2048, max_height: int = 2048, **opts):
        o = self._options()
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"{type(self).__name__}: unknown option {k!r}")
            setattr(o, k, v)
        self.options = o
        self.summary = None
        self._h = C.c_void_p()
        capi.check(self._c("create")(device, int(max_width), int(max_height), C.byref(o), C.byref(self._h)))

    def run(self, image):
        """osfm_*_extract alone: the summary (counts and stage times); the result stays in the context."""
        image, channels = _image_arg(type(self).__name__, image)
        s = self._summary()
        capi.check(self._c("extract")(self._h, image.ctypes.data, image.shape[1], image.shape[0], channels, C.byref(s)))
        self.summary = s
        return s

    def download(self) -> Features:
        """osfm_*_download of the last run()."""
        n = self.summary.num_descriptors
        f = Features(np.zeros((n, self._width), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32),
                     np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.uint8))
        capi.check(self._c("download")(self._h, f.descriptors.ctypes.data, f.positions.ctypes.data, f.scale.ctypes.data,
                                       f.orientation.ctypes.data, f.colors.ctypes.data, f.normalized.ctypes.data))
        return f

    def extract(self, image) -> Features:
        self.run(image)
        return self.download()

    def _debug_image(self, *plane) -> np.ndarray:
        w, h = C.c_int32(), C.c_int32()
        capi.check(self._c("debug_image")(self._h, *plane, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        capi.check(self._c("debug_image")(self._h, *plane, out.ctypes.data, None, None))
        return out

    def debug_keypoints(self, after_localisation: bool) -> np.ndarray:
        n = C.c_int32()
        capi.check(self._c("debug_keypoints")(self._h, int(after_localisation), None, C.byref(n)))
        out = np.zeros((n.value, 4), np.float32)
        capi.check(self._c("debug_keypoints")(self._h, int(after_localisation), out.ctypes.data, None))
        return out


class SiftExtractor(_Detector):
    """One context (osfm_sift): the pyramid and work arrays for images up to max_width x max_height.  The keyword
    options are the fields of osfm_sift_options (Sift::Options and max_keypoints)."""
    _prefix, _options, _summary, _width = "sift", staticmethod(capi.default_sift_options), capi.SiftSummary, 128

    def debug_image(self, octave: int, kind: int, index: int) -> np.ndarray:
        return self._debug_image(octave, kind, index)


class SurfExtractor(_Detector):
    """One context (osfm_surf): the summed-area table, the response maps and work arrays for images up to
    max_width x max_height.  The keyword options are the fields of osfm_surf_options (Surf::Options and
    max_keypoints)."""
    _prefix, _options, _summary, _width = "surf", staticmethod(capi.default_surf_options), capi.SurfSummary, 64

    def debug_image(self, octave: int, sample: int) -> np.ndarray:
        return self._debug_image(octave, sample)

    def debug_describe(self, x, y, scale, orientation, upright=False):
        """(descriptor [64], status) of one hand-placed descriptor on the last image: status 0 rejected, 1 ok,
        2 ok with taps outside the summed-area table read as zero (non-finite input only).  scale in [1, 65)."""
        out, status = np.zeros(64, np.float32), C.c_int32()
        capi.check(capi.lib.osfm_surf_debug_describe(self._h, float(x), float(y), float(scale), float(orientation), int(upright),
                                                     out.ctypes.data, C.byref(status)))
        return out, status.value


@dataclass
class FeatureSet:
    """FeatureSet::compute_features with FEATURE_ALL: both detectors' descriptors, and positions and colours of
    the SIFT rows followed by the SURF rows."""
    sift: Features
    surf: Features
    positions: np.ndarray       # float32 [n_sift + n_surf, 2]
    normalized: np.ndarray      # float32 [n_sift + n_surf, 2]
    colors: np.ndarray          # uint8 [n_sift + n_surf, 3]

    def __len__(self):
        return len(self.sift) + len(self.surf)


class FeatureSetExtractor:
    """A SIFT and a SURF context for images up to max_width x max_height; `sift` and `surf` are dictionaries of
    their options."""

    def __init__(self, device: int = 0, max_width: int = 2048, max_height: int = 2048, sift=None, surf=None):
        self.sift = SiftExtractor(device, max_width, max_height, **(sift or {}))
        try:
            self.surf = SurfExtractor(device, max_width, max_height, **(surf or {}))
        except Exception:
            self.sift.close()
            raise

    def close(self):
        self.sift.close()
        self.surf.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def extract(self, image) -> FeatureSet:
        a, b = self.sift.extract(image), self.surf.extract(image)
        return FeatureSet(a, b, np.concatenate([a.positions, b.positions]), np.concatenate([a.normalized, b.normalized]),
                          np.concatenate([a.colors, b.colors]))


@dataclass
class ViewFeatures(FeatureSet):
    """What ViewFrontEnd.download returns: the FeatureSet of the image the detectors saw, and the sizes the
    reference's pixel conversion needs."""
    import_width: int = 0       # after downscale_factor: calculateTracksUsingMVE's imageWidth
    import_height: int = 0
    feature_width: int = 0      # after the max_image_size loop: positions are in pixels of this image
    feature_height: int = 0


_MARK_MODES = {"tracks": capi.MARK_TRACKS, "features": capi.MARK_FEATURES}
_MARK_CLAMPS = {"reference": capi.CLAMP_REFERENCE, "image": capi.CLAMP_IMAGE}


def _mark_options(mode, clamp, threshold, pixel_width):
    if mode not in _MARK_MODES:
        raise ValueError(f"mask mode {mode!r}: 'tracks' or 'features'")
    if clamp not in _MARK_CLAMPS:
        raise ValueError(f"mask clamp {clamp!r}: 'reference' or 'image'")
    return capi.ViewMarkOptions(_MARK_MODES[mode], _MARK_CLAMPS[clamp], int(threshold), int(pixel_width))


def mark_rows_host(normalized, image, mask=None, clamp="reference", threshold=16, pixel_width=0):
    """Test hook osfm_view_debug_mark_rows: the row function of the marks kernel on host arrays, no device needed.
    Returns (pixel_xy, pixel_rgb, mark) for normalized [n, 2]; image is the import image."""
    image, channels = _image_arg("mark_rows_host", image)
    nrm = np.ascontiguousarray(normalized, dtype=np.float32).reshape(-1, 2)
    o = _mark_options("tracks", clamp, threshold, pixel_width)
    mw = mh = 0
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        mh, mw = mask.shape
    n = nrm.shape[0]
    xy, rgb, mark = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8)
    capi.check(capi.lib.osfm_view_debug_mark_rows(n, nrm.ctypes.data, image.ctypes.data, image.shape[1], image.shape[0], channels,
                                                  mask.ctypes.data if mask is not None else None, mw, mh, C.byref(o),
                                                  xy.ctypes.data, rgb.ctypes.data, mark.ctypes.data))
    return xy, rgb, mark


class ViewFrontEnd(_Handle):
    """One context (osfm_view_front) for images up to max_width x max_height: image in host memory -> halving
    chain -> SIFT and SURF from one upload -> colours and normalised positions, all on the device.  `sift` and
    `surf` are dictionaries of the detectors' options."""
    _prefix = "view_front"

    def __init__(self, device: int = 0, max_width: int = 2048, max_height: int = 2048, downscale_factor: int = 1,
                 max_image_size: int = 6_000_000, feature_types: int = capi.FEATURE_ALL, sift=None, surf=None):
        vo = capi.ViewOptions(int(downscale_factor), int(max_image_size), int(feature_types))
        so, uo = capi.default_sift_options(), capi.default_surf_options()
        for o, given, who in ((so, sift, "sift"), (uo, surf, "surf")):
            for k, v in (given or {}).items():
                if not hasattr(o, k):
                    raise TypeError(f"ViewFrontEnd: unknown {who} option {k!r}")
                setattr(o, k, v)
        self.options, self.summary, self.mark_summary = vo, None, None
        self._h = C.c_void_p()
        capi.check(capi.lib.osfm_view_front_create(device, int(max_width), int(max_height), C.byref(vo), C.byref(so), C.byref(uo),
                                                   C.byref(self._h)))

    def load(self, image) -> capi.ViewSummary:
        """osfm_view_front_load: the summary (sizes, counts, stage times); the result stays on the device for
        HipExhaustiveMatching.set_view_from_front and download()."""
        image, channels = _image_arg("ViewFrontEnd", image)
        self.summary = self.mark_summary = None
        s = capi.ViewSummary()
        capi.check(capi.lib.osfm_view_front_load(self._h, image.ctypes.data, image.shape[1], image.shape[0], channels, C.byref(s)))
        self.summary = s
        return s

    def load_marked(self, image, mask=None, mode="tracks", clamp="reference", threshold=16, pixel_width=0) -> capi.ViewSummary:
        """osfm_view_front_load_marked: load() with a mark, a pixel position and a pixel colour per row
        (filterTracksWithMasks and propagateColorsToTracks as lookups while the image is on the device).  mask: uint8
        [mh, mw] at whatever size the caller resized it to, or None for a view without one.  mode "tracks" leaves the
        result that of load(); "features" removes the masked-out rows from it.  clamp "reference" is the reference's
        swapped clamp, "image" the intended one.  mark_summary holds the counts; download_marks() the arrays."""
        image, channels = _image_arg("ViewFrontEnd", image)
        o = _mark_options(mode, clamp, threshold, pixel_width)
        mw = mh = 0
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 or mask.ndim != 2:
                raise TypeError("ViewFrontEnd: an uint8 mask [h, w] is expected")
            mask = np.ascontiguousarray(mask)
            mh, mw = mask.shape
        self.summary = self.mark_summary = None
        s, ms = capi.ViewSummary(), capi.ViewMarkSummary()
        capi.check(capi.lib.osfm_view_front_load_marked(self._h, image.ctypes.data, image.shape[1], image.shape[0], channels,
                                                        mask.ctypes.data if mask is not None else None, mw, mh, C.byref(o),
                                                        C.byref(s), C.byref(ms)))
        self.summary, self.mark_summary = s, ms
        return s

    def download_marks(self):
        """osfm_view_front_download_marks of the last load_marked(): (pixel_xy float32 [n, 2], pixel_rgb uint8 [n, 3],
        mark uint8 [n]) in download()'s row order."""
        if self.summary is None:
            raise capi.OsfmError(capi.E_STATE, "ViewFrontEnd.download_marks: no load to download")
        n = self.summary.num_sift + self.summary.num_surf
        xy, rgb, mark = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.uint8), np.zeros(n, np.uint8)
        capi.check(capi.lib.osfm_view_front_download_marks(self._h, xy.ctypes.data, rgb.ctypes.data, mark.ctypes.data))
        return xy, rgb, mark

    def download(self) -> ViewFeatures:
        """osfm_view_front_download of the last load()."""
        if self.summary is None:
            raise capi.OsfmError(capi.E_STATE, "ViewFrontEnd.download: no load to download")
        ns, nu = self.summary.num_sift, self.summary.num_surf
        n = ns + nu
        pos, nrm, col = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 3), np.uint8)
        scale, ori = np.zeros(n, np.float32), np.zeros(n, np.float32)
        ds, du = np.zeros((ns, 128), np.float32), np.zeros((nu, 64), np.float32)
        capi.check(capi.lib.osfm_view_front_download(self._h, pos.ctypes.data, nrm.ctypes.data, col.ctypes.data, scale.ctypes.data,
                                                     ori.ctypes.data, ds.ctypes.data, du.ctypes.data))
        part = lambda d, a, b: Features(d, pos[a:b], nrm[a:b], scale[a:b], ori[a:b], col[a:b])
        s = self.summary
        return ViewFeatures(part(ds, 0, ns), part(du, ns, n), pos, nrm, col, s.import_width, s.import_height, s.feature_width,
                            s.feature_height)

    def debug_image(self) -> np.ndarray:
        """Test hook: the image the detectors saw, [h, w] or [h, w, 3]."""
        w, h, c = C.c_int32(), C.c_int32(), C.c_int32()
        capi.check(capi.lib.osfm_view_front_debug_image(self._h, None, C.byref(w), C.byref(h), C.byref(c)))
        out = np.zeros((h.value, w.value) if c.value == 1 else (h.value, w.value, c.value), np.uint8)
        capi.check(capi.lib.osfm_view_front_debug_image(self._h, out.ctypes.data, None, None, None))
        return out
