"""Hostile track tables for the device-resident scene, and the sequences of steps that tests/test_scene_model_cpu.py
(model alone) and tests/test_scene_steps_gpu.py (device against model) run on them.

A table is built from synth.make_ba_scene(model, 6, N, min_len=6, max_len=6, noise_px=0.2): N points, each seen by
all 6 views, 0.2 px of noise, positions through float32.  Every track of the table takes one of those points, keeps
some of its 6 observations and shifts some of them.  The cameras of every step are the scene's ground-truth cameras,
so that a feature that was not shifted reprojects within its noise.

Classes.  A class is defined against a camera set S of n views: LOCAL = (3, 0, 4) for the local steps and for the
permanent filter of sequence C (only those three views are aligned there, so that views outside the set exist), and
ALL = all 6 views for the permanent filter of sequences A and F.  Against ALL there is no view outside the set and no
view without a camera: classes 4, 5 and 10 exist against LOCAL only.
   1  seen by all n, every feature consistent: stays whole
   2  seen by all n, one feature shifted by >= 4 px: loses that feature and stays
   3  seen by all n and by no other view, n - 1 features bad: dies
   4  as 3 with one or two features in views outside the set: stays alive, one feature inside (not in the
      adjustment's selection)
   5  seen by all n, all n features bad, two features outside: stays with nothing inside the set
   6  seen by n - 1 views of the set, every feature shifted by ~30 px: not judged, untouched
   7  would be full, but one of its features in the set has alive_f = 0 and another is shifted by ~30 px: not judged
      (judged, it would lose the shifted feature)
   8  alive_t = 0, features bad (every second one of them has a cleared feature flag as well): nothing changes
   9  empty tracks at the head, in the middle and at the tail of the table; tracks of length 1 (in a view of LOCAL)
  10  two features, both in views outside the set
The shifts of classes 2-5 are not random: with orthographic cameras of one scale the re-triangulated point is the
linear least-squares point of the pixel residuals, r = (I - A pinv(A)) (x - a) with A the stacked 2 x 3 projections.
The shifts of the bad features are taken from the null space of the block that maps them to the good features'
residuals (the good ones keep their noise residual), scaled until every bad feature is >= 5 px away from the point; for
class 2 (no such null space) the shift goes along the direction its own residual keeps most of, and the track is
taken only if the prediction gives > 2 px for it and < 1.45 px for the others (among three cameras a shifted feature
keeps at most 2/3 of its shift and hands 1/3 to each of the others: 4 px give 2.67 and 1.33).  classify() then checks
every planted track against the ORACLE's errors (tests/oracle_lib.py), not against this prediction.

Sizes.  Every scene kernel runs 256-thread blocks and the select / keep / flag kernels write one extra entry at
index F or T.  Tables f255, f256, f257 have that many features, t255, t256, t257 that many tracks, big has 1501
tracks; padding is done with tracks of length 1.  A table of 256 features cannot hold 8 tracks of every class against
both sets (8 of each against LOCAL alone are 234 features): f* hold 8 of each class against LOCAL and one track each of
classes 1, 2, 3 against ALL, so that the permanent filter over 6 cameras still kills a track and clears a feature.
"""
import functools

import numpy as np

from orthosfm_amd import synth
from scene_model import SceneModel

Q, E = synth.MODEL_QUATERNION, synth.MODEL_EULER
V = 6
ALL = (0, 1, 2, 3, 4, 5)
LOCAL = (3, 0, 4)
LOCAL2 = (1, 2, 5)
MAX_ERROR = 1.5
BORDERLINE = 1e-6
MIN_PER_CLASS = 8
SEED = synth.BASE_SEED
_ST = 0x5CE << 32

# name -> (classes against LOCAL, per class; classes against ALL, per class; target F or None; target T or None)
TABLES = {
    "f255": (8, 1, 255, None), "f256": (8, 1, 256, None), "f257": (8, 1, 257, None),
    "t255": (16, 12, None, 255), "t256": (16, 12, None, 256), "t257": (16, 12, None, 257),
    "big": (90, 80, None, 1501),
}
MODELS = (Q, E)
CASES = [(name, model) for name in TABLES for model in MODELS]
CLASSES_LOCAL = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
CLASSES_ALL = (1, 2, 3, 6, 7, 8)


def case_id(case):
    return f"{case[0]}-{'quat' if case[1] == Q else 'euler'}"


class Table:
    """offsets (T + 1) int64, view (F) int32, xy (F, 2) float32, the flags a sequence starts from, the planted label
    (set name, class) of every track, the cameras."""

    def __init__(self, name, model, offsets, view, xy, alive_t, alive_f, labels, cams, const, img_w, img_h):
        self.name, self.model = name, model
        self.offsets, self.view, self.xy = offsets, view, xy
        self.alive_t, self.alive_f, self.labels = alive_t, alive_f, labels
        self.cams, self.const, self.img_w, self.img_h = cams, const, img_w, img_h
        for a in (offsets, view, xy, alive_t, alive_f, cams, const, img_w, img_h):
            a.setflags(write=False)

    @property
    def T(self):
        return self.offsets.shape[0] - 1

    @property
    def F(self):
        return self.view.shape[0]

    def model_scene(self, mutation=None):
        return SceneModel(self.model, self.img_w, self.img_h, self.offsets, self.view, self.xy, mutation)

    def device_scene(self, device=0):
        from orthosfm_amd.scene import Scene
        return Scene(self.model, self.img_w, self.img_h, self.offsets, self.view, self.xy, device)

    def local_const(self, views):
        """The constant masks of a local step: the group's first camera fixed (reconstruct.cpp:215)."""
        c = self.const[list(views)].copy()
        c[0, :] = 1
        return c


# ---------------------------------------------------------------------------
# planting
# ---------------------------------------------------------------------------

def _projections(model, cams, w, h):
    """Per view (a, P): pixel position = a + P X (orthographic: exactly affine)."""
    out = []
    pts = np.vstack([np.zeros(3), np.eye(3)])
    for c in range(cams.shape[0]):
        p = synth._project(model, cams[c], pts, int(w[c]), int(h[c]))
        out.append((p[0].copy(), (p[1:] - p[0]).T.copy()))
    return out


def _residuals(proj, views, xy):
    """Pixel residual norms of the least-squares point of the features (views, xy)."""
    A = np.vstack([proj[v][1] for v in views])
    b = np.concatenate([xy[i] - proj[v][0] for i, v in enumerate(views)])
    X = np.linalg.lstsq(A, b, rcond=None)[0]
    return np.linalg.norm((A @ X - b).reshape(-1, 2), axis=1)


def _shift_for(proj, views, xy, bad, rnd):
    """Shifts (len(views), 2) that make the features `bad` (positions in views) fail and leave the others at their
    noise residual; None if the prediction does not give clear margins."""
    n = len(views)
    A = np.vstack([proj[v][1] for v in views])
    Mp = np.eye(2 * n) - A @ np.linalg.pinv(A)
    good = [i for i in range(n) if i not in bad]
    cols = [2 * i + k for i in bad for k in (0, 1)]
    rows = [2 * i + k for i in good for k in (0, 1)]
    single = False
    if good:
        _, s, vt = np.linalg.svd(Mp[np.ix_(rows, cols)])
        rank = int((s > 1e-9).sum())
        null = vt[rank:].T
        if null.shape[1] == 0:
            single = True
            i = bad[0]
            _, v_ = np.linalg.eigh(Mp[2 * i:2 * i + 2, 2 * i:2 * i + 2])
            d = v_[:, -1]
        else:
            d = null @ rnd[:null.shape[1]]
    else:
        d = rnd[:len(cols)].copy()
    d = d / np.linalg.norm(d)
    for scale in ([4.0, 4.1, 4.2, 4.5, 5.0] if single else [6.0 * 1.25 ** k for k in range(24)]):
        delta = np.zeros((n, 2))
        delta.reshape(-1)[cols] = scale * d
        moved = (xy + delta).astype(np.float32).astype(np.float64)
        r = _residuals(proj, views, moved)
        shifted_enough = all(np.linalg.norm(delta[i]) >= 4.0 for i in bad)
        if single:
            if shifted_enough and r[bad[0]] > 2.0 and all(r[i] < 1.45 for i in good):
                return delta
        elif shifted_enough and all(r[i] >= 5.0 for i in bad) and all(r[i] < 1.0 for i in good):
            return delta
    return None


class _Planter:
    def __init__(self, name, model, n_points):
        cfg = 0x300 + 16 * list(TABLES).index(name) + model
        self.sc = synth.make_ba_scene(model, V, n_points, config_id=cfg, min_len=V, max_len=V, noise_px=0.2)
        self.model = model
        self.proj = _projections(model, self.sc.gt_cams, self.sc.img_w, self.sc.img_h)
        self.next_point = 0
        self.stream = _ST | (cfg << 12)
        self.draws = 0
        self.tracks = []                     # (views, xy (float64, n x 2), dead feature positions, dead track, label)

    def _rnd(self, n):
        self.draws += 1
        return synth.normal(SEED, self.stream, n, offset=64 * self.draws)

    def _base(self, views):
        """The next unused point's observations in `views`, in the order the point's arc has them."""
        j = self.next_point
        self.next_point += 1
        assert j < self.sc.points.shape[0], "out of base points"
        k = np.arange(V * j, V * j + V)
        cam = self.sc.obs_camera[k]
        pick = [i for i in range(V) if int(cam[i]) in views]
        return [int(cam[i]) for i in pick], self.sc.obs_xy[k[pick]].copy()

    def plant(self, label, views, bad_views=(), gross_views=(), dead_views=(), dead_track=False):
        """bad_views: features that must fail against the set of the label while the rest of the set holds;
        gross_views: features shifted by ~30 px; dead_views: features with a cleared flag."""
        S = LOCAL if label[0] == "local" else ALL
        for _ in range(400):
            vs, xy = self._base(set(views))
            if bad_views:
                idx = [i for i, v in enumerate(vs) if v in S]
                sv = [vs[i] for i in idx]
                delta = _shift_for(self.proj, sv, xy[idx], [sv.index(v) for v in bad_views], self._rnd(2 * len(sv)))
                if delta is None:
                    continue
                xy[idx] += delta
            for v in gross_views:
                g = self._rnd(2)
                xy[vs.index(v)] += 30.0 * g / np.linalg.norm(g)
            self.tracks.append((vs, xy, [vs.index(v) for v in dead_views], dead_track, label))
            return
        raise AssertionError(f"no base point gives {label} clear margins")

    def empty(self):
        return ([], np.zeros((0, 2)), [], False, ("any", 9))


def _outside(S, k, i):
    out = [v for v in ALL if v not in S]
    return [out[(i + j) % len(out)] for j in range(k)] if out else []


def _plant_set(p, setname, S, count, classes):
    n = len(S)
    for i in range(count):
        rot = [S[(i + j) % n] for j in range(n)]                 # which features are the bad ones rotates
        extra = _outside(S, i % 3, i)                            # 0, 1 or 2 consistent features outside the set
        if 1 in classes:
            p.plant((setname, 1), list(S) + (extra if setname == "local" and count > MIN_PER_CLASS else []))
        if 2 in classes:
            p.plant((setname, 2), list(S) + (extra if count > MIN_PER_CLASS else []), bad_views=rot[:1])
        if 3 in classes:
            p.plant((setname, 3), list(S), bad_views=rot[:n - 1])
        if 4 in classes:
            p.plant((setname, 4), list(S) + _outside(S, 2 if i % 4 == 3 else 1, i), bad_views=rot[:n - 1])
        if 5 in classes:
            p.plant((setname, 5), list(S) + _outside(S, 2, i), bad_views=rot)
        if 6 in classes:
            p.plant((setname, 6), rot[:n - 1] + (extra[:1] if count > MIN_PER_CLASS else []), gross_views=rot[:n - 1])
        if 7 in classes:
            p.plant((setname, 7), list(S), gross_views=rot[:1], dead_views=rot[1:2])
        if 8 in classes:
            p.plant((setname, 8), list(S), gross_views=rot[:2], dead_views=rot[2:3] if i % 2 else (), dead_track=True)
        if 10 in classes:
            p.plant((setname, 10), _outside(S, 2, i))
        if 9 in classes:
            p.plant((setname, 9), [S[i % n]])


@functools.lru_cache(maxsize=None)
def table(name, model):
    n_local, n_all, target_f, target_t = TABLES[name]
    p = _Planter(name, model, 16 * (n_local * 10 + n_all * 6) + 512)
    _plant_set(p, "local", LOCAL, n_local, CLASSES_LOCAL)
    _plant_set(p, "all", ALL, n_all, (1, 2, 3) if target_f else CLASSES_ALL)
    # padding: tracks of length 1
    f_now = sum(len(t[0]) for t in p.tracks)
    pad = target_f - f_now if target_f else target_t - len(p.tracks) - 3
    assert pad >= 0, (name, pad)
    for i in range(pad):
        p.plant(("local", 9), [LOCAL[i % 3]])
    # a fixed shuffle, so that the classes are spread over the blocks; then the three empty tracks
    order = np.argsort(synth.uniform(SEED, p.stream | 0x7FF, len(p.tracks)), kind="stable")
    tracks = [p.tracks[i] for i in order]
    tracks.insert(len(tracks) // 2, p.empty())
    tracks.insert(0, p.empty())
    tracks.append(p.empty())
    ln = [len(t[0]) for t in tracks]
    offsets = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    view = np.array([v for t in tracks for v in t[0]], dtype=np.int32)
    xy = np.vstack([t[1] for t in tracks] + [np.zeros((0, 2))]).astype(np.float32)
    alive_t = np.array([not t[3] for t in tracks], dtype=np.uint8)
    alive_f = np.ones(view.shape[0], dtype=np.uint8)
    for j, t in enumerate(tracks):
        for i in t[2]:
            alive_f[offsets[j] + i] = 0
    tb = Table(name, model, offsets, view, xy, alive_t, alive_f, tuple(t[4] for t in tracks),
               p.sc.gt_cams.copy(), p.sc.cam_const.copy(), p.sc.img_w.copy(), p.sc.img_h.copy())
    if target_f:
        assert tb.F == target_f
    else:
        assert tb.T == target_t and tb.F % 256 != 0
    return tb


# ---------------------------------------------------------------------------
# what the oracle says about the planted tracks
# ---------------------------------------------------------------------------

def classify(tb, setname):
    """Per track of the table: the class it shows against the set under the ORACLE's errors with the table's start
    flags (0: none of the classes), and the smallest | error - MAX_ERROR | over the judged features."""
    S = LOCAL if setname == "local" else ALL
    m = tb.model_scene()
    m.set_flags(tb.alive_t, tb.alive_f)
    verdicts = {v.track: v for v in m.judge(list(S), tb.cams[list(S)], tb.const[list(S)], MAX_ERROR)}
    margin = min([abs(e - MAX_ERROR) for v in verdicts.values() for e in v.errors] + [np.inf])
    n = len(S)
    out = []
    for t in range(tb.T):
        feats = list(range(int(tb.offsets[t]), int(tb.offsets[t + 1])))
        inside = [f for f in feats if int(tb.view[f]) in S]
        live_in = [f for f in inside if tb.alive_f[f]]
        c = 0
        if len(feats) <= 1:
            c = 9
        elif not tb.alive_t[t]:
            c = 8
        elif not inside:
            c = 10
        elif t in verdicts:
            v = verdicts[t]
            k, o = len(v.kept), len(v.outside)
            if k == n:
                c = 1
            elif k == n - 1 and v.stays:
                c = 2
            elif k == 1 and o == 0 and not v.stays:
                c = 3
            elif k == 1 and o >= 1 and v.stays:
                c = 4
            elif k == 0 and o == 2 and v.stays:
                c = 5
        elif len(inside) == n and len(live_in) == n - 1:
            c = 7
        elif len(inside) == n - 1 and len(live_in) == n - 1:
            c = 6
        out.append(c)
    return out, margin


# ---------------------------------------------------------------------------
# sequences: lists of steps that both tests run
# ---------------------------------------------------------------------------
# ("flags", alive_t, alive_f) ("align", views) ("tri", new_views or None) ("filter",) ("local", views) ("global",)
# ("outliers",) ("move", view)  ("revive",): a set_flags call that must be refused

def moved(tb, view):
    p = tb.cams[view].copy()
    p[4 if tb.model == Q else 3] += 0.03                         # offsetX
    return p


def _clear_some(tb, at, af, views, every_t, every_f):
    """Clears every every_t-th track and every every_f-th feature among those in `views`."""
    at, af = at.copy(), af.copy()
    in_views = np.isin(tb.view, list(views))
    fs = np.flatnonzero(in_views)
    af[fs[::every_f]] = 0
    track_of = np.repeat(np.arange(tb.T), np.diff(tb.offsets))
    ts = np.unique(track_of[fs])
    at[ts[::every_t]] = 0
    return at, af


def sequences(tb):
    at0, af0 = np.array(tb.alive_t), np.array(tb.alive_f)
    start = ("flags", at0, af0)
    seq = {}
    seq["A"] = [start, ("align", ALL), ("tri", None), ("filter",), ("tri", None), ("global",)]
    seq["B"] = [start, ("align", ALL), ("tri", None), ("local", LOCAL), ("local", LOCAL2)]
    seq["C"] = [start, ("align", LOCAL), ("tri", None), ("filter",), ("global",)]
    af_d = af0.copy()
    af_d[np.isin(tb.view, [1, 2])] = 0
    seq["D"] = [("flags", at0, af_d), ("align", ALL), ("tri", None), ("local", LOCAL2)]
    at_e, af_e = _clear_some(tb, at0, af0, LOCAL2, 7, 5)
    seq["E"] = [start, ("align", LOCAL), ("tri", None), ("flags", at_e, af_e), ("align", LOCAL2),
                ("tri", LOCAL2), ("move", 0), ("tri", (5,))]
    return seq


def sequence_f(tb):
    """Sequence A with an outlier filter behind the filter, flags cleared by the caller and a second outlier filter:
    under OSFM_SCENE_COMPACT=2 two compactions in a row.  The ("flags*", every_t, every_f) steps clear every every_t-th of
    the tracks that are alive when they run and every every_f-th of the live features."""
    return [("flags", np.array(tb.alive_t), np.array(tb.alive_f)), ("align", ALL), ("tri", None), ("filter",),
            ("outliers",), ("flags*", 5, 7), ("outliers",), ("flags*", 9, 11), ("revive",), ("tri", None), ("global",)]


def run_model(tb, steps, mutation=None):
    """The model alone over a sequence.  Returns the trace: after every step the downloaded flags (as bytes) and, for
    the selections, M and O; and the statistics (killed, cleared) of every permanent filter, (M, O) of every
    selection, the smallest margin of a judged error."""
    m = tb.model_scene(mutation)
    trace, stats, margin = [], [], np.inf
    for st in steps:
        extra = None
        if st[0] == "flags":
            m.set_flags(st[1], st[2])
        elif st[0] == "flags*":
            at, af, _, _ = m.download()
            m.set_flags(*thin(at, af, np.repeat(np.arange(tb.T), np.diff(tb.offsets)), st[1], st[2]))
        elif st[0] == "align":
            vs = list(st[1])
            m.align_views(vs, tb.cams[vs], tb.const[vs])
        elif st[0] == "tri":
            m.triangulate(st[1])
        elif st[0] == "filter":
            extra = m.filter_reprojection(MAX_ERROR)
            stats.append(("filter",) + extra)
        elif st[0] == "local":
            vs = list(st[1])
            _, M, O, _ = m.local_selection(vs, tb.cams[vs], tb.local_const(vs), MAX_ERROR)
            extra = (M, O)
            stats.append(("local", M, O))
        elif st[0] == "global":
            M, O, _ = m.global_selection()
            extra = (M, O)
            stats.append(("global", M, O))
        elif st[0] == "outliers":
            extra = m.filter_outliers()
        elif st[0] == "move":
            m.set_cameras([st[1]], moved(tb, st[1])[None])
        elif st[0] == "revive":
            pass
        else:
            raise AssertionError(st[0])
        if st[0] in ("filter", "local"):
            margin = min([margin] + [abs(e - MAX_ERROR) for v in m.last_verdicts for e in v.errors])
        at, af, hp, _ = m.download()
        trace.append((st[0], at.tobytes(), af.tobytes(), hp.tobytes(), extra))
    return trace, stats, margin


def thin(at, af, track_of, every_t, every_f):
    """Flags that only clear: every every_t-th of the alive tracks, every every_f-th of the live features (alive, of
    an alive track)."""
    at, af = np.array(at, dtype=np.uint8), np.array(af, dtype=np.uint8)
    live = np.flatnonzero(af.astype(bool) & at.astype(bool)[track_of])
    af[live[::every_f]] = 0
    at[np.flatnonzero(at)[::every_t]] = 0
    return at, af
