"""ctypes mirror of the device-resident scene (include/osfm_hip.h, osfm_scene_*): the track table of the incremental
reconstruction uploaded once, every step of runPoseEstimation (src/sfm/reconstruct.cpp:193-281) a call that
selects its observations from the flags on the device.  Used by orthosfm_amd/pipeline.py; a C++ caller uses the
same entries (tests/host/scene_check.cc)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class Scene:
    def __init__(self, model: int, img_w, img_h, track_offsets, feat_view, feat_xy, device: int = 0):
        self.num_views = len(img_w)
        self._w = np.ascontiguousarray(img_w, dtype=np.int32)
        self._h = np.ascontiguousarray(img_h, dtype=np.int32)
        off = np.ascontiguousarray(track_offsets, dtype=np.int64)
        view = np.ascontiguousarray(feat_view, dtype=np.int32)
        xy = np.ascontiguousarray(feat_xy, dtype=np.float32).reshape(-1, 2)
        self.num_tracks = int(off.shape[0] - 1)
        self.num_features = int(view.shape[0])
        self._h_scene = C.c_void_p()
        capi.check(capi.lib.osfm_scene_create(C.c_int(device), C.c_int(model), C.c_int(self.num_views),
                                              capi._ptr(self._w, C.c_int32), capi._ptr(self._h, C.c_int32),
                                              C.c_int32(self.num_tracks), capi._ptr(off, C.c_int64),
                                              capi._ptr(view, C.c_int32), capi._ptr(xy, C.c_float), C.byref(self._h_scene)))

    def close(self):
        if self._h_scene:
            capi.lib.osfm_scene_destroy(self._h_scene)
            self._h_scene = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_flags(self, alive_track=None, alive_feature=None):
        at = None if alive_track is None else np.ascontiguousarray(alive_track, dtype=np.uint8)
        af = None if alive_feature is None else np.ascontiguousarray(alive_feature, dtype=np.uint8)
        capi.check(capi.lib.osfm_scene_set_flags(self._h_scene, None if at is None else capi._ptr(at, C.c_uint8),
                                                 None if af is None else capi._ptr(af, C.c_uint8)))

    def align_views(self, views, params, cam_const):
        v = np.ascontiguousarray(views, dtype=np.int32)
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 7)
        c = np.ascontiguousarray(cam_const, dtype=np.uint8).reshape(-1, 7)
        capi.check(capi.lib.osfm_scene_align_views(self._h_scene, C.c_int(v.shape[0]), capi._ptr(v, C.c_int32),
                                                   capi._ptr(p, C.c_double), capi._ptr(c, C.c_uint8)))

    def set_cameras(self, views, params):
        """Replaces the parameters of views that are aligned already (the next triangulation is a full pass)."""
        v = np.ascontiguousarray(views, dtype=np.int32)
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 7)
        capi.check(capi.lib.osfm_scene_set_cameras(self._h_scene, C.c_int(v.shape[0]), capi._ptr(v, C.c_int32),
                                                   capi._ptr(p, C.c_double)))

    def cameras(self):
        n = C.c_int32()
        capi.check(capi.lib.osfm_scene_get_cameras(self._h_scene, 0, None, None, C.byref(n)))
        views = np.zeros(max(n.value, 1), dtype=np.int32)
        params = np.zeros((max(n.value, 1), 7))
        capi.check(capi.lib.osfm_scene_get_cameras(self._h_scene, n.value, capi._ptr(views, C.c_int32),
                                                   capi._ptr(params, C.c_double), C.byref(n)))
        return views[:n.value], params[:n.value]

    def triangulate(self, new_views=None, check_full=False) -> int:
        """Returns the number of tracks on which the incremental pass differs from a full one (check_full)."""
        bad = C.c_int32()
        if new_views is None:
            capi.check(capi.lib.osfm_scene_triangulate(self._h_scene, 0, None, 0, C.byref(bad)))
        else:
            v = np.ascontiguousarray(new_views, dtype=np.int32)
            capi.check(capi.lib.osfm_scene_triangulate(self._h_scene, C.c_int(v.shape[0]), capi._ptr(v, C.c_int32),
                                                       C.c_int(1 if check_full else 0), C.byref(bad)))
        return bad.value

    def filter_reprojection(self, max_error: float):
        capi.check(capi.lib.osfm_scene_filter_reprojection(self._h_scene, C.c_double(max_error)))

    def filter_consensus(self, **opts):
        """osfm_scene_filter_consensus: the per-track consensus triangulation (filters.consensus) over the aligned
        cameras and every live track with two or more live features in aligned views, permanent.  opts: fields of
        osfm_consensus_options.  Returns the statistics (capi.ConsensusStats)."""
        o = capi.default_consensus_options(**opts)
        st = capi.ConsensusStats()
        capi.check(capi.lib.osfm_scene_filter_consensus(self._h_scene, C.byref(o), C.byref(st)))
        return st

    def local_adjustment(self, views, params, cam_const, max_error: float, options):
        """params is updated in place; returns (summary, points, observations)."""
        v = np.ascontiguousarray(views, dtype=np.int32)
        c = np.ascontiguousarray(cam_const, dtype=np.uint8).reshape(-1, 7)
        assert params.dtype == np.float64 and params.flags["C_CONTIGUOUS"]
        s = capi.BaSummary()
        m, o = C.c_int32(), C.c_int32()
        capi.check(capi.lib.osfm_scene_local_adjustment(self._h_scene, C.c_int(v.shape[0]), capi._ptr(v, C.c_int32),
                                                        capi._ptr(params, C.c_double), capi._ptr(c, C.c_uint8),
                                                        C.c_double(max_error), C.byref(options), C.byref(s),
                                                        C.byref(m), C.byref(o)))
        return s, m.value, o.value

    def tk_align(self, views, group_id=0, **opts):
        """osfm_scene_tk_align: the Tomasi-Kanade RANSAC (orthosfm_amd/tk.py) over the live tracks that all `views`
        see, selected and gathered on the device; cameras in the order of `views`."""
        from . import tk
        v = np.ascontiguousarray(views, dtype=np.int32)
        c = int(v.shape[0])
        o = tk.options(**opts)
        b1, b2, off = np.zeros((max(c, 1), 3, 3)), np.zeros((max(c, 1), 3, 3)), np.zeros((max(c, 1), 2))
        inl = np.zeros(max(self.num_tracks, 1), dtype=np.uint8)
        r, n = capi.TkResult(), C.c_int32()
        capi.check(capi.lib.osfm_scene_tk_align(self._h_scene, C.c_int(c), capi._ptr(v, C.c_int32), C.byref(o),
                                                C.c_uint64(group_id), capi._ptr(b1, C.c_double), capi._ptr(b2, C.c_double),
                                                capi._ptr(off, C.c_double), capi._ptr(inl, C.c_uint8),
                                                C.c_int32(inl.shape[0]), C.byref(r), C.byref(n)))
        return tk._alignment(b1, b2, off, inl, r, n.value)

    def resect_view(self, view, stream_id=0, **opts):
        """osfm_scene_resect_view: the affine-camera RANSAC (orthosfm_amd/resect.py) over the live features of `view`
        whose track has a point, selected and gathered on the device.  The view needs no camera; the scene is not
        changed."""
        from . import resect
        o = resect.options(**opts)
        rot, off, scale = np.zeros((3, 3)), np.zeros(2), C.c_double()
        inl = np.zeros(max(self.num_tracks, 1), dtype=np.uint8)        # a track holds at most one feature of a view
        r, n = capi.ResectResult(), C.c_int32()
        capi.check(capi.lib.osfm_scene_resect_view(self._h_scene, C.c_int32(view), C.byref(o), C.c_uint64(stream_id),
                                                   rot.ctypes.data, C.byref(scale), off.ctypes.data, inl.ctypes.data,
                                                   C.c_int32(inl.shape[0]), C.byref(r), C.byref(n)))
        return resect._placement(rot, scale, off, inl, r, n.value)

    def global_adjustment(self, options):
        s = capi.BaSummary()
        m, o = C.c_int32(), C.c_int32()
        capi.check(capi.lib.osfm_scene_global_adjustment(self._h_scene, C.byref(options), C.byref(s), C.byref(m), C.byref(o)))
        return s, m.value, o.value

    def covariance(self, options=None, full: bool = False, skip=(), fill=None, **kw):
        """osfm_scene_covariance: ba.covariance on the selection global_adjustment makes, bit for bit what the per-call
        entry gives on that problem; cameras in join order, points per scene track in the caller's numbering (a track
        outside the selection is invalid).  The scene is not changed.  Returns a ba.Covariance."""
        from . import ba
        o = options if options is not None else ba.cov_options(**kw)
        n = C.c_int32()
        capi.check(capi.lib.osfm_scene_get_cameras(self._h_scene, 0, None, None, C.byref(n)))
        return ba._covariance_call(lambda oo, r: capi.lib.osfm_scene_covariance(self._h_scene, C.byref(oo), C.byref(r)),
                                   n.value, self.num_tracks, 6 * n.value, o, full, skip, fill)

    def filter_outliers(self) -> int:
        k = C.c_int32()
        capi.check(capi.lib.osfm_scene_filter_outliers(self._h_scene, None, C.byref(k)))
        return k.value

    def download(self):
        """(alive_track, alive_feature, has_point, points) as the scene holds them."""
        at = np.zeros(max(self.num_tracks, 1), dtype=np.uint8)
        af = np.zeros(max(self.num_features, 1), dtype=np.uint8)
        hp = np.zeros(max(self.num_tracks, 1), dtype=np.uint8)
        pt = np.zeros((max(self.num_tracks, 1), 4))
        capi.check(capi.lib.osfm_scene_download(self._h_scene, capi._ptr(at, C.c_uint8), capi._ptr(af, C.c_uint8),
                                                capi._ptr(hp, C.c_uint8), capi._ptr(pt, C.c_double)))
        return (at[:self.num_tracks].astype(bool), af[:self.num_features].astype(bool),
                hp[:self.num_tracks].astype(bool), pt[:self.num_tracks])
