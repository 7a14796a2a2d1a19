"""The device-resident scene (orthosfm_amd/scene.py, csrc/scene_api.hip) as plain host state: a list of tracks, each a
list of features, flags and points per entry, the aligned cameras.  Same verbs as orthosfm_amd.scene.Scene.

Written track by track from the reference's text, not from the kernels' scans and scatters and not from
pipeline.py's vectorised per-call form: every selection is a Python loop over the features of a track.  The numbers
(intersections, reprojection errors, the outlier statistics) come from the CPU oracle through tests/oracle_lib.py;
nothing here calls the device.

What the reference does to a list of tracks, and what that is here, where "removed" is a cleared flag:

  live feature            alive_f[f] and alive_t[track of f]: a feature that is still in the reference's list.

  reprojection filter     filterTracksWithReprojectionError, outlier_filtering.cpp:127-192.
    judged                only a track with a live feature in EVERY camera of the set (:131, filterTracksToAvailable-
                          Cameras(cameras, tracks, true, true) keeps the tracks whose features inside the set number as
                          many as the cameras; a feature that a filter has removed is not in the track any more);
    re-triangulated       from those features (:134, triangulateTracks(cameras, fullSizeTracks, true));
    a feature of the set  stays iff its error against that point is < max_error (:160-165);
    a feature outside     the set always stays (:172-175);
    a judged track        stays iff what stays, inside plus outside, is more than one feature (:179-181);
    any other track       is untouched (:184-186).
    permanent form        (reconstruct.cpp:265) the dropped features and tracks lose their flags.  A feature of a judged
                          track that fails loses its flag whether its track stays or not.
    local form            (reconstruct.cpp:212-219) nothing changes; the adjustment behind it works on the tracks the
                          filter returns, cut to the cameras of the set and to those with two or more features there
                          (bundle_adjustment.cpp:72-75): the kept features of tracks that stay and keep more than one
                          feature inside the set -- for a track that is not judged, its live features inside the set.

  triangulation           triangulateOrthographicTracks(cameras, tracks, true), triangulation.cpp:44-93.
    full pass             every alive track: two or more live rays under the aligned cameras and a valid intersection
                          give it a point (:78-86), otherwise it loses the one it has (:89-91).  A dead track is not in
                          the reference's list: nothing about it changes.
    incremental pass      the same, for the alive tracks with a live feature in one of the new views only: the others
                          keep what they have (their rays have not changed).
    after set_cameras     the next pass is a full one whatever is asked for.

  global selection        runBundleAdjustment(alignedCameras, tracks, ...), bundle_adjustment.cpp:86-123: the alive
                          tracks with a point are the points, in track order (:88-99); their live features whose view has
                          a camera are the observations, in feature order (:101-121).

  outlier filter          filterOutlierTracks over the alive tracks in order (outlier_filtering.cpp:40-125); the dropped
                          ones lose their track flag, nothing else.

  download                always in the caller's numbering; there is no compaction here.

mutation: one of the planted errors of tests/test_scene_model_cpu.py (None: the model as described).
"""
import numpy as np

import oracle_lib

MUTATIONS = {
    "a": "a judged track stays with >= 1 feature left (> 1 is right)",
    "b": "features outside the camera set are not counted towards what is left",
    "c": "a track that a dead feature has made less than full is judged",
    "d": "a track seen by all cameras of the set but one is judged",
    "e": "every track with a feature in the set that has <= 1 feature left is killed, judged or not",
    "f": "the adjustment's selection takes tracks with one feature inside the set",
    "g": "the incremental triangulation clears the points of the tracks it does not touch",
}


class Flat:
    """The arrays of a flattened problem, named as oracle_lib.ba_problem_struct and ba.FlatProblem.from_scene read
    them, and the track of every point."""

    def __init__(self, model, cam_params, cam_const, img_w, img_h, points, obs_xy, obs_camera, obs_point, tracks):
        self.model = int(model)
        self.cam_params = np.array(cam_params, dtype=np.float64, order="C").reshape(-1, 7)
        self.cam_const = np.array(cam_const, dtype=np.uint8, order="C").reshape(-1, 7)
        self.img_w = np.array(img_w, dtype=np.int32, order="C").reshape(-1)
        self.img_h = np.array(img_h, dtype=np.int32, order="C").reshape(-1)
        self.points = np.array(points, dtype=np.float64, order="C").reshape(-1, 4)
        self.obs_xy = np.array(obs_xy, dtype=np.float64, order="C").reshape(-1, 2)
        self.obs_camera = np.array(obs_camera, dtype=np.int32, order="C").reshape(-1)
        self.obs_point = np.array(obs_point, dtype=np.int32, order="C").reshape(-1)
        self.tracks = list(tracks)

    @property
    def M(self):
        return self.points.shape[0]

    @property
    def O(self):
        return self.obs_camera.shape[0]

    def copy(self):
        return Flat(self.model, self.cam_params, self.cam_const, self.img_w, self.img_h, self.points, self.obs_xy,
                    self.obs_camera, self.obs_point, self.tracks)


class Verdict:
    """What the reprojection filter found for one judged track."""

    def __init__(self, track, inside, errors, kept, outside, stays):
        self.track, self.inside, self.errors, self.kept, self.outside, self.stays = track, inside, errors, kept, outside, stays


class SceneModel:
    def __init__(self, model, img_w, img_h, track_offsets, feat_view, feat_xy, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.model = int(model)
        self.mutation = mutation
        self.img_w = [int(v) for v in img_w]
        self.img_h = [int(v) for v in img_h]
        off = [int(v) for v in track_offsets]
        self.tracks = [list(range(off[t], off[t + 1])) for t in range(len(off) - 1)]
        self.view = [int(v) for v in feat_view]
        # Feature::x / y are floats (track.h:26-27): the double of each is what the residuals see
        xy = np.asarray(feat_xy, dtype=np.float32).reshape(-1, 2)
        self.xy = [(float(x), float(y)) for x, y in xy]
        T, F = len(self.tracks), len(self.view)
        self.alive_t = [True] * T
        self.alive_f = [True] * F
        self.has_point = [False] * T
        self.point = [[0.0, 0.0, 0.0, 0.0] for _ in range(T)]
        self.aligned = []                    # views in the order they joined
        self.cam = {}                        # view -> 7 parameters
        self.const = {}                      # view -> 7 constant flags
        self.cams_moved = False
        self.last_verdicts = []              # of the last filter (either form)

    # ---- state ------------------------------------------------------------------------------------------------
    @property
    def num_tracks(self):
        return len(self.tracks)

    @property
    def num_features(self):
        return len(self.view)

    def set_flags(self, alive_track=None, alive_feature=None):
        if alive_track is not None:
            assert len(alive_track) == len(self.alive_t)
            self.alive_t = [bool(v) for v in alive_track]
        if alive_feature is not None:
            assert len(alive_feature) == len(self.alive_f)
            self.alive_f = [bool(v) for v in alive_feature]

    def align_views(self, views, params, cam_const):
        params = np.asarray(params, dtype=np.float64).reshape(-1, 7)
        cam_const = np.asarray(cam_const, dtype=np.uint8).reshape(-1, 7)
        for i, v in enumerate(views):
            v = int(v)
            assert v not in self.cam, "the view has a camera already"
            self.aligned.append(v)
            self.cam[v] = params[i].copy()
            self.const[v] = cam_const[i].copy()

    def set_cameras(self, views, params):
        params = np.asarray(params, dtype=np.float64).reshape(-1, 7)
        for i, v in enumerate(views):
            assert int(v) in self.cam, "the view has no camera yet"
            self.cam[int(v)] = params[i].copy()
        if len(views):
            self.cams_moved = True

    def cameras(self):
        return list(self.aligned), np.array([self.cam[v] for v in self.aligned]).reshape(-1, 7)

    def download(self):
        return (np.array(self.alive_t, dtype=bool), np.array(self.alive_f, dtype=bool),
                np.array(self.has_point, dtype=bool), np.array(self.point, dtype=np.float64).reshape(-1, 4))

    # what a test that holds the device to this model takes over from the per-call entries, so that the next step of
    # both starts from the same bytes (the oracle's figures differ from the device's in the last bits)
    def adopt_points(self, tracks, points):
        for t, p in zip(tracks, points):
            assert self.has_point[t]
            self.point[t] = [float(v) for v in p]

    def adopt_cameras(self, params):
        params = np.asarray(params, dtype=np.float64).reshape(-1, 7)
        assert params.shape[0] == len(self.aligned)
        for v, p in zip(self.aligned, params):
            self.cam[v] = p.copy()

    # ---- helpers ----------------------------------------------------------------------------------------------
    def live(self, t):
        """The features of track t that are still in the reference's list."""
        if not self.alive_t[t]:
            return []
        return [f for f in self.tracks[t] if self.alive_f[f]]

    def _flatten(self, views, params, const, entries, start):
        """entries: (track, features) per point, in order; start: the points' start values."""
        slot = {int(v): i for i, v in enumerate(views)}
        xy, cam, pt, tr = [], [], [], []
        for j, (t, feats) in enumerate(entries):
            tr.append(t)
            for f in feats:
                xy.append(self.xy[f])
                cam.append(slot[self.view[f]])
                pt.append(j)
        return Flat(self.model, np.asarray(params, dtype=np.float64).reshape(-1, 7),
                    np.asarray(const, dtype=np.uint8).reshape(-1, 7), [self.img_w[int(v)] for v in views],
                    [self.img_h[int(v)] for v in views], np.asarray(start, dtype=np.float64).reshape(-1, 4),
                    np.asarray(xy, dtype=np.float64).reshape(-1, 2), cam, pt, tr)

    # ---- triangulation ----------------------------------------------------------------------------------------
    def triangulate(self, new_views=None):
        """Returns (problem, valid): the rays of the tracks the pass worked on, flattened as they were given to the
        oracle (points (0, 0, 0, 1) before, the intersections after), and which of them got a point."""
        full = new_views is None or self.cams_moved
        self.cams_moved = False
        new = set() if full else {int(v) for v in new_views}
        entries = []
        for t in range(len(self.tracks)):
            if not self.alive_t[t]:
                continue                                         # not in the reference's list
            live = self.live(t)
            if not full and not any(self.view[f] in new for f in live):
                if self.mutation == "g":
                    self.has_point[t] = False
                continue                                         # untouched: its rays are what they were
            rays = [f for f in live if self.view[f] in self.cam]            # triangulation.cpp:59-75
            self.has_point[t] = False                            # :89-91 (and :78-86 sets it again below)
            if rays:
                entries.append((t, rays))
        views = list(self.aligned)
        prob = self._flatten(views, [self.cam[v] for v in views], [self.const[v] for v in views], entries,
                             [[0.0, 0.0, 0.0, 1.0]] * len(entries))
        valid = oracle_lib.oracle_ba_triangulate(prob).astype(bool) if prob.M else np.zeros(0, dtype=bool)
        for j, (t, rays) in enumerate(entries):
            assert bool(valid[j]) == (len(rays) > 1)             # :78
            if valid[j]:
                self.has_point[t] = True
                self.point[t] = [float(v) for v in prob.points[j]]
        return prob, valid

    # ---- reprojection filter ----------------------------------------------------------------------------------
    def judge(self, views, params, const, max_error):
        views = [int(v) for v in views]
        n = len(views)
        inset = set(views)
        m = self.mutation
        judged = []
        for t in range(len(self.tracks)):
            if not self.alive_t[t]:
                continue
            inside = [f for f in self.live(t) if self.view[f] in inset]
            if m == "c":
                inside = [f for f in self.tracks[t] if self.view[f] in inset]          # dead features counted
            if len(inside) == n or (m == "d" and n > 1 and len(inside) == n - 1):      # :131
                judged.append((t, inside))
        # :134 -- the start value of a judged point is the track's own (it is overwritten: n >= 2 rays)
        prob = self._flatten(views, params, const, judged, [self.point[t] for t, _ in judged])
        err = np.zeros(0)
        if prob.M:
            valid = oracle_lib.oracle_ba_triangulate(prob)
            assert valid.all() or n < 2 or m == "d"
            _, err = oracle_lib.oracle_ba_residuals(prob)
        verdicts, k = [], 0
        for t, inside in judged:
            e = [float(err[k + i]) for i in range(len(inside))]
            k += len(inside)
            kept = [f for f, ef in zip(inside, e) if ef < max_error]                   # :160-165
            outside = [f for f in self.live(t) if self.view[f] not in inset]          # :172-175
            left = len(kept) + (0 if m == "b" else len(outside))
            stays = left >= 1 if m == "a" else left > 1                                # :179
            verdicts.append(Verdict(t, inside, e, kept, outside, stays))
        self.last_verdicts = verdicts
        return verdicts

    def filter_reprojection(self, max_error):
        """The permanent form over the aligned cameras.  Returns (tracks killed, features cleared)."""
        if not self.aligned or not self.tracks:
            return 0, 0
        views = list(self.aligned)
        verdicts = self.judge(views, [self.cam[v] for v in views], [self.const[v] for v in views], max_error)
        killed = cleared = 0
        for v in verdicts:
            for f in v.inside:
                if f not in v.kept and self.alive_f[f]:
                    self.alive_f[f] = False
                    cleared += 1
            if not v.stays:
                self.alive_t[v.track] = False
                killed += 1
        if self.mutation == "e":
            inset, judged = set(views), {v.track for v in verdicts}
            for t in range(len(self.tracks)):
                live = self.live(t)
                if t not in judged and any(self.view[f] in inset for f in live) and len(live) <= 1:
                    self.alive_t[t] = False
                    killed += 1
        return killed, cleared

    def local_selection(self, views, params, cam_const, max_error):
        """The local form: nothing changes.  Returns (features, M, O, problem): the features the adjustment works on in
        feature order, its numbers of points and observations, and the problem flattened with every point at
        (0, 0, 0, 1) -- the adjustment re-triangulates its copy first (runBundleAdjustment(..., true, true))."""
        views = [int(v) for v in views]
        inset = set(views)
        verdict_of = {v.track: v for v in self.judge(views, params, cam_const, max_error)}
        need = 1 if self.mutation == "f" else 2                  # bundle_adjustment.cpp:72-75
        entries = []
        for t in range(len(self.tracks)):
            if not self.alive_t[t]:
                continue
            v = verdict_of.get(t)
            if v is not None:
                if not v.stays:
                    continue
                feats = [f for f in v.kept if self.alive_f[f]]
            else:
                feats = [f for f in self.live(t) if self.view[f] in inset]
            if len(feats) >= need:
                entries.append((t, feats))
        prob = self._flatten(views, params, cam_const, entries, [[0.0, 0.0, 0.0, 1.0]] * len(entries))
        return [f for _, feats in entries for f in feats], prob.M, prob.O, prob

    # ---- global adjustment ------------------------------------------------------------------------------------
    def global_selection(self):
        """(M, O, problem): bundle_adjustment.cpp:86-123 over the aligned cameras, points from the tracks."""
        entries = []
        for t in range(len(self.tracks)):
            if self.alive_t[t] and self.has_point[t]:                                   # :88-99
                entries.append((t, [f for f in self.live(t) if self.view[f] in self.cam]))      # :101-121
        views = list(self.aligned)
        prob = self._flatten(views, [self.cam[v] for v in views], [self.const[v] for v in views], entries,
                             [self.point[t] for t, _ in entries])
        return prob.M, prob.O, prob

    def adopt_adjustment(self, prob):
        """The adjusted cameras and points of global_selection()'s problem, back into the state."""
        self.adopt_cameras(prob.cam_params)
        self.adopt_points(prob.tracks, prob.points)

    # ---- outlier filter ---------------------------------------------------------------------------------------
    def filter_outliers(self):
        alive = [t for t in range(len(self.tracks)) if self.alive_t[t]]
        if not alive:
            return 0
        keep, _, _ = oracle_lib.oracle_filter_outlier_tracks([self.point[t] for t in alive],
                                                             [self.has_point[t] for t in alive])
        killed = 0
        for t, k in zip(alive, keep):
            if not k:
                self.alive_t[t] = False
                killed += 1
        return killed
