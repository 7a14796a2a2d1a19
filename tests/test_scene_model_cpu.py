"""The cases of tests/scene_cases.py bite, shown without a device: every table holds every class and hits its size,
no judged feature is borderline, and each of the planted errors of tests/scene_model.py (MUTATIONS) changes what the
model downloads or selects on every table -- so a device that made the same error would be caught by
tests/test_scene_steps_gpu.py, which holds the device to the unmutated model after every step.

The per-call Python mirror filters.filter_tracks_with_reprojection_error takes its errors from the device through
osfm_filter_reprojection.  It is fed the oracle's here through a stand-in for that one entry (the mirror's own
logic -- which tracks are full, what is kept, what is dropped -- runs as it is) and compared with the model."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
import scene_cases as sc
from scene_model import MUTATIONS, Flat


@functools.lru_cache(maxsize=None)
def _traces(name, model, mutation):
    tb = sc.table(name, model)
    seqs = dict(sc.sequences(tb))
    seqs["F"] = sc.sequence_f(tb)
    return {k: sc.run_model(tb, steps, mutation) for k, steps in seqs.items()}


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_sizes_classes_and_margins(case):
    name, model = case
    tb = sc.table(name, model)
    _, _, target_f, target_t = sc.TABLES[name]
    if target_f:
        assert tb.F == target_f
    else:
        assert tb.T == target_t and tb.F % 256 != 0
    if name == "big":
        assert tb.T > 5 * 256 and tb.T % 256 and tb.F % 256
    # class 9: empty tracks at the head, in the middle and at the tail; tracks of length 1
    ln = np.diff(tb.offsets)
    assert ln[0] == 0 and ln[-1] == 0 and (ln[1:-1] == 0).sum() == 1 and 0 < int(np.flatnonzero(ln[1:-1] == 0)[0]) + 1 < tb.T - 1
    assert (ln == 1).sum() >= sc.MIN_PER_CLASS
    # every planted track shows its class under the oracle's errors; the counts
    for setname, classes in (("local", sc.CLASSES_LOCAL), ("all", sc.CLASSES_ALL)):
        got, margin = sc.classify(tb, setname)
        assert margin > sc.BORDERLINE, (setname, margin)
        counts = {c: 0 for c in classes + (9,)}
        for t, (label, c) in enumerate(zip(tb.labels, got)):
            if label[0] in (setname, "any"):
                assert c == label[1], (setname, t, label, c)
                counts[c] += 1
        print(f"{sc.case_id(case)} {setname}: F {tb.F} T {tb.T} classes {counts} margin {margin:.3e}")
        for c in classes:
            if setname == "local" or not target_f:
                assert counts[c] >= sc.MIN_PER_CLASS, (setname, c, counts)
            elif c in (1, 2, 3):
                assert counts[c] >= 1, (setname, c, counts)         # (a table of 256 features: see scene_cases.py)
    # no judged feature of any step of any sequence is borderline; the permanent filters kill and clear
    for k, (_, stats, margin) in _traces(name, model, None).items():
        assert margin > sc.BORDERLINE, (k, margin)
        for s in stats:
            if s[0] == "filter":
                assert s[1] > 0 and s[2] > 0, (k, s)
        print(f"{sc.case_id(case)} sequence {k}: {stats}")
    d = _traces(name, model, None)["D"][1]
    assert d[-1] == ("local", 0, 0)


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_planted_error_is_seen(case, mutation):
    name, model = case
    true, bad = _traces(name, model, None), _traces(name, model, mutation)
    seen = [k for k in true if true[k][0] != bad[k][0]]
    print(f"{sc.case_id(case)} ({mutation}) {MUTATIONS[mutation]}: seen in {seen}")
    assert seen, (mutation, MUTATIONS[mutation])
    # where each of them has to show: the permanent filter with views outside the set (C) for (a) to (e) -- and over
    # all cameras (A) for (c), (d) on the tables that hold classes 6 and 7 against that set --, the local step (B) for
    # (f), the incremental pass (E) for (g)
    where = {"a": "C", "b": "C", "c": "C", "d": "C", "e": "C", "f": "B", "g": "E"}[mutation]
    assert where in seen, (mutation, seen)
    if mutation in "cd" and not sc.TABLES[name][2]:
        assert "A" in seen, (mutation, seen)


class _StandIn:
    """orthosfm_amd.capi with osfm_filter_reprojection answered by the oracle."""

    class _Lib:
        @staticmethod
        def osfm_filter_reprojection(st_ref, device, max_error, keep, valid, err):
            st = st_ref._obj

            def arr(addr, dt, n):
                return np.ctypeslib.as_array(C.cast(addr, C.POINTER(dt)), shape=(max(n, 1),))[:n].copy()
            Cn, M, O = st.num_cameras, st.num_points, st.num_observations
            p = Flat(st.model, arr(st.cam_params, C.c_double, 7 * Cn), arr(st.cam_const, C.c_uint8, 7 * Cn),
                     arr(st.img_width, C.c_int32, Cn), arr(st.img_height, C.c_int32, Cn), arr(st.points, C.c_double, 4 * M),
                     arr(st.obs_xy, C.c_double, 2 * O), arr(st.obs_camera, C.c_int32, O), arr(st.obs_point, C.c_int32, O),
                     range(M))
            oracle_lib.oracle_ba_triangulate(p)
            _, e = oracle_lib.oracle_ba_residuals(p)
            for k in range(O):
                keep[k] = 1 if e[k] < max_error.value else 0
            return 0

    lib = _Lib()

    @staticmethod
    def check(status):
        assert status == 0

    @staticmethod
    def _ptr(a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype)) if a is not None and a.size else None


@pytest.mark.parametrize("model", sc.MODELS)
def test_per_call_mirror_equals_the_model(model, monkeypatch):
    from orthosfm_amd import ba, filters
    monkeypatch.setattr(filters, "capi", _StandIn)
    tb = sc.table("t256", model)
    m = tb.model_scene()
    m.set_flags(tb.alive_t, tb.alive_f)
    # the reference's list: the live features of the alive tracks (localFeatureID = the feature's index)
    tracks, ids = [], []
    for t in range(tb.T):
        feats = [ba.Feature(int(tb.view[f]), f, float(tb.xy[f, 0]), float(tb.xy[f, 1])) for f in m.live(t)]
        if tb.alive_t[t]:
            tracks.append(ba.Track(feats))
            ids.append(t)
    views = list(sc.LOCAL)
    if model == sc.Q:
        cams = [ba.QuatCamera(v, int(tb.img_w[v]), int(tb.img_h[v]), tb.cams[v, :4], *tb.cams[v, 4:7]) for v in views]
    else:
        cams = [ba.EulerCamera(v, int(tb.img_w[v]), int(tb.img_h[v]), *tb.cams[v, :6]) for v in views]
    assert np.array_equal(np.array([c.params() for c in cams]), tb.cams[views])
    out = filters.filter_tracks_with_reprojection_error(tracks, cams, verbose=False, max_error=sc.MAX_ERROR)
    got = {tuple(f.localFeatureID for f in t.features) for t in out}
    # the model, cameras of the local set aligned, permanent form
    m.align_views(views, tb.cams[views], tb.const[views])
    killed, cleared = m.filter_reprojection(sc.MAX_ERROR)
    assert killed > 0 and cleared > 0
    want = {tuple(m.live(t)) for t in ids if m.alive_t[t]}
    assert got == want
    assert len(out) == sum(1 for t in ids if m.alive_t[t])
