"""The per-track consensus triangulation on the device (osfm_ba_consensus, osfm_scene_filter_consensus, the pipeline's
track_filter="consensus") against its definition, tests/consensus_restatement.py, on the cases of
tests/consensus_cases.py (tests/test_consensus_cases_cpu.py shows that no decision of a case sits at rounding level).

Per case: keep flags, statuses and the counters of the statistics equal the restatement's exactly; the points of CLEAN
and REPAIRED tracks lie within tri_cases' bound, |x - x_ref|_inf <= TAU 2^-53 A_j with x_ref and A_j from its 200-bit
reference over the rays the point was fitted from (the kept rays on every settled track); obs_err equals
osfm_ba_reprojection_errors at the returned points, bit for bit.

Observed on MI355X: every case equal to the restatement; largest |x - x_ref|_inf / (2^-53 A_j) over all cases 1.754
(min_support_2, Euler), against TAU = 8.  The pipeline test (12 views x 300 features, 49 planted features in 49 tracks,
quaternion cameras): under "consensus" 0 planted features alive, 41 features dropped, none of them in a clean track,
rotation error max 2.4e-6 / mean 6.2e-7 degrees; under "reference" 21 planted features alive in live tracks, rotation
error max 8.0e-3 / mean 3.2e-3 degrees.
"""
import ctypes as C

import numpy as np
import pytest

import consensus_cases as cc
import consensus_restatement as cr
import tri_cases as tri
from orthosfm_amd import synth

pytestmark = pytest.mark.gpu

IDS = [cc.key(n, m) for n, m in cc.ALL]


@pytest.fixture(scope="module")
def mods():
    from orthosfm_amd import ba, capi, filters
    assert capi.device_count() >= 1
    return ba, capi, filters


_got = {}


def _run(mods, name, model):
    ba, _, filters = mods
    k = (name, model)
    if k not in _got:
        case = cc.build(name, model)
        _got[k] = filters.consensus(ba.FlatProblem.from_scene(case.sc), **case.opts)
    return _got[k]


def _raw(res):
    return (res.keep.tobytes(), res.status.tobytes(), res.points.tobytes(), res.valid.tobytes(), res.err.tobytes(),
            tuple(sorted(res.stats.counters().items())))


def test_limits(mods):
    l = mods[1].consensus_limits()
    assert (l.short_length, l.short_tracks, l.long_tracks, l.max_sample) == (cc.SHORT_LEN, cc.SHORT_TRACKS, cc.LONG_TRACKS, cc.MAX_SAMPLE)
    o = mods[1].default_consensus_options()
    assert (o.max_error, o.min_support, o.max_sample, o.refit_rounds) == tuple(cr.DEFAULTS[k] for k in
                                                                              ("max_error", "min_support", "max_sample", "refit_rounds"))


@pytest.mark.parametrize("name,model", cc.ALL, ids=IDS)
def test_case_equals_the_restatement(mods, name, model):
    ba = mods[0]
    case, want, got = cc.build(name, model), cc.restated(name, model), _run(mods, name, model)
    sc = case.sc
    print(f"\n[consensus] {cc.key(name, model)}: {got.stats.counters()} {got.stats.device_ms:.3f} ms")
    assert np.array_equal(got.status, want["status"]), np.nonzero(got.status != want["status"])[0][:10]
    assert np.array_equal(got.keep, want["keep"]), np.nonzero(got.keep != want["keep"])[0][:10]
    assert got.stats.counters() == want["stats"]
    assert np.array_equal(got.valid, want["valid"])
    # every track that is not CLEAN or REPAIRED returns its input point
    assert np.array_equal(got.points[~got.valid], sc.points[~got.valid])
    assert (got.points[got.valid, 3] == 1.0).all()
    # the returned points against the 200-bit ray intersection over the rays they were fitted from
    fit = want["fit"]
    sub = synth.BaScene(sc.model, sc.cam_params, sc.cam_const, sc.img_w, sc.img_h, sc.points, sc.obs_xy[fit],
                        sc.obs_camera[fit], sc.obs_point[fit], sc.cam_params, sc.points)
    g = tri.reference(sub)
    assert np.array_equal(g["valid"].astype(bool), want["valid"])
    r, j = tri.worst(got.points, g)
    print(f"[consensus] {cc.key(name, model)}: worst |x - x_ref| / (2^-53 A_j) = {r:.3f} at track {j}")
    assert r <= tri.TAU, (r, j)
    # the errors at the returned points
    at = ba.FlatProblem(sc.model, sc.cam_params, sc.cam_const, sc.img_w, sc.img_h, got.points, sc.obs_xy, sc.obs_camera,
                        sc.obs_point)
    err, _ = ba.reprojection_errors(at)
    assert err.tobytes() == got.err.tobytes()


@pytest.mark.parametrize("name", ("planted", "lengths"))
@pytest.mark.parametrize("model", (cc.Q, cc.E), ids=("quat", "euler"))
def test_repeats_to_the_bit_and_follows_the_track_order(mods, name, model):
    ba, _, filters = mods
    case, first = cc.build(name, model), _run(mods, name, model)
    sc = case.sc
    again = filters.consensus(ba.FlatProblem.from_scene(sc), **case.opts)
    assert _raw(again) == _raw(first)
    # the tracks in another order: the results move with them
    M = sc.points.shape[0]
    perm = np.argsort(synth.uniform(cc.SEED, cc._ST | 0xF0, M), kind="stable")
    start = np.concatenate([[0], np.cumsum(tri.track_lengths(sc))]).astype(np.int64)
    obs = np.concatenate([np.arange(start[j], start[j + 1]) for j in perm]).astype(np.int64)
    ln = tri.track_lengths(sc)[perm]
    fp = ba.FlatProblem(sc.model, sc.cam_params, sc.cam_const, sc.img_w, sc.img_h, sc.points[perm], sc.obs_xy[obs],
                        sc.obs_camera[obs], np.repeat(np.arange(M), ln))
    moved = filters.consensus(fp, **case.opts)
    assert moved.status.tobytes() == first.status[perm].tobytes()
    assert moved.points.tobytes() == first.points[perm].tobytes()
    assert moved.valid.tobytes() == first.valid[perm].tobytes()
    assert moved.keep.tobytes() == first.keep[obs].tobytes()
    assert moved.err.tobytes() == first.err[obs].tobytes()
    assert moved.stats.counters() == first.stats.counters()


def test_null_outputs_and_argument_errors(mods):
    ba, capi, filters = mods
    sc = cc.build("edges_short_33", cc.Q).sc
    fp = ba.FlatProblem.from_scene(sc)
    st = fp.struct()
    points_before = fp.points.copy()
    # every output may be NULL, opts NULL are the defaults
    assert capi.lib.osfm_ba_consensus(C.byref(st), None, None, None, None, None, None, None) == capi.OK
    stats = capi.ConsensusStats()
    assert capi.lib.osfm_ba_consensus(C.byref(st), None, None, None, None, None, None, C.byref(stats)) == capi.OK
    assert stats.counters() == _run(mods, "edges_short_33", cc.Q).stats.counters()
    assert np.array_equal(fp.points, points_before)          # the problem is not written
    bad = [dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=float("nan")), dict(max_error=float("inf")),
           dict(min_support=1), dict(min_support=0), dict(max_sample=1), dict(max_sample=17), dict(refit_rounds=-1),
           dict(refit_rounds=capi.CONSENSUS_MAX_REFIT_ROUNDS + 1), dict(device=-1), dict(device=capi.device_count())]
    for kw in bad:
        o = capi.default_consensus_options(**kw)
        assert capi.lib.osfm_ba_consensus(C.byref(st), C.byref(o), None, None, None, None, None, None) == capi.E_ARG, kw
    assert capi.lib.osfm_ba_consensus(None, None, None, None, None, None, None, None) == capi.E_ARG
    broken = fp.struct()
    broken.obs_xy = None
    assert capi.lib.osfm_ba_consensus(C.byref(broken), None, None, None, None, None, None, None) == capi.E_ARG
    assert capi.lib.osfm_scene_filter_consensus(None, None, None) == capi.E_ARG
    scene = tri.scene_from_ba_scene(sc)
    for kw in bad[:10]:
        o = capi.default_consensus_options(**kw)
        assert capi.lib.osfm_scene_filter_consensus(scene._h_scene, C.byref(o), None) == capi.E_ARG, kw
    # no aligned camera: nothing to test, nothing changes
    st0 = scene.filter_consensus()
    assert st0.tracks_tested == 0 and scene.download()[0].all()
    scene.close()
    # the limits of the options themselves are accepted
    for kw in (dict(min_support=2, max_sample=2, refit_rounds=0), dict(max_sample=16, refit_rounds=capi.CONSENSUS_MAX_REFIT_ROUNDS)):
        filters.consensus(fp, **kw)


@pytest.mark.parametrize("model", (cc.Q, cc.E), ids=("quat", "euler"))
def test_scene_form_equals_the_per_call_form(mods, model):
    """osfm_scene_filter_consensus on a table with dead tracks, dead features and views without a camera against
    osfm_ba_consensus on the same features flattened in table order, applied by the rules of the header."""
    ba, capi, filters = mods
    case = cc.build("planted", model)
    sc = case.sc
    V, T, F = sc.cam_params.shape[0], sc.points.shape[0], sc.obs_xy.shape[0]
    u = synth.uniform(cc.SEED, cc._ST | 0xE0, V + T + F)
    views = np.argsort(u[:V], kind="stable")[:18].astype(np.int32)           # 18 of the 24 views, in a drawn order
    alive_t = u[V:V + T] >= 0.1
    alive_f = u[V + T:] >= 0.1
    scene = tri.scene_from_ba_scene(sc)
    scene.set_flags(alive_t.astype(np.uint8), alive_f.astype(np.uint8))
    scene.align_views(views, sc.cam_params[views], sc.cam_const[views])
    assert scene.triangulate() == 0
    at0, af0, hp0, pt0 = scene.download()
    assert np.array_equal(at0, alive_t) and np.array_equal(af0, alive_f)
    stats = scene.filter_consensus()
    at1, af1, hp1, pt1 = scene.download()
    scene.close()
    # the host's account of it
    cam_of = np.full(V, -1, dtype=np.int32)
    cam_of[views] = np.arange(views.shape[0], dtype=np.int32)
    track_of = sc.obs_point.astype(np.int64)
    live = alive_f & alive_t[track_of]
    in_set = live & (cam_of[sc.obs_camera] >= 0)
    cnt_set, cnt_live = np.bincount(track_of[in_set], minlength=T), np.bincount(track_of[live], minlength=T)
    tested = cnt_set >= 2
    fi = np.nonzero(in_set & tested[track_of])[0]
    fu = np.nonzero(tested)[0]
    slot = np.cumsum(tested) - 1
    fp = ba.FlatProblem(sc.model, sc.cam_params[views], sc.cam_const[views], sc.img_w[views], sc.img_h[views], pt0[fu],
                        sc.obs_xy[fi], cam_of[sc.obs_camera[fi]], slot[track_of[fi]])
    res = filters.consensus(fp)
    assert stats.counters() == res.stats.counters()
    assert res.stats.tracks_repaired >= 8 and res.stats.tracks_unsupported >= 1 and res.stats.tracks_clean >= 8
    want_af, want_at, want_pt = alive_f.copy(), alive_t.copy(), pt0.copy()
    want_af[fi[~res.keep]] = False
    kept = np.bincount(track_of[fi[res.keep]], minlength=T)
    dies = tested & (kept + cnt_live - cnt_set < 2)
    want_at[dies] = False
    take = (res.status == capi.CONSENSUS_REPAIRED) & hp0[fu] & ~dies[fu]
    want_pt[fu[take]] = res.points[take]
    assert dies.any() and take.any() and (~res.keep).any()
    assert np.array_equal(af1, want_af) and np.array_equal(at1, want_at) and np.array_equal(hp1, hp0)
    assert pt1[want_at].tobytes() == want_pt[want_at].tobytes()


def _same(a, b):
    assert a.aligned_views == b.aligned_views
    assert a.cam_params.tobytes() == b.cam_params.tobytes()
    ta, tb = a.tracks, b.tracks
    assert np.array_equal(ta.alive_t, tb.alive_t) and np.array_equal(ta.alive_f, tb.alive_f)
    assert np.array_equal(ta.live_f, tb.live_f) and np.array_equal(ta.alive_lengths(), tb.alive_lengths())
    sel = ta.has_point & ta.alive_t
    assert np.array_equal(sel, tb.has_point & tb.alive_t)
    assert sel.sum() > 50 and ta.point[sel].tobytes() == tb.point[sel].tobytes()
    ca = [(c.kind, c.cameras, c.points, c.observations, c.iterations) for c in a.ba_calls]
    cb = [(c.kind, c.cameras, c.points, c.observations, c.iterations) for c in b.ba_calls]
    assert ca == cb


def test_default_is_unchanged():
    """reconstruct(track_filter="reference") is reconstruct(): the same bytes."""
    from orthosfm_amd import pipeline as P
    iset = synth.make_image_set(6, 800, config_id=73)
    a = P.reconstruct(iset, solver=0, seed=11)
    b = P.reconstruct(iset, solver=0, seed=11, track_filter="reference")
    _same(a, b)
    assert a.consensus_stats == {} and b.consensus_stats == {} and b.timings.consensus_filter_s == 0.0
    with pytest.raises(ValueError):
        P.reconstruct(iset, solver=0, seed=11, track_filter="both")


def _landmark_table(iset, share=0.15, min_len=5):
    """A track table straight from the landmarks of the image set (no matcher, no noise): one track per landmark
    that two or more views see, features in view order.  In `share` of the tracks of min_len or more features, in the
    order of a drawn key, one feature (drawn) is replaced by a distractor of the same view (drawn among those no
    other track has taken).  Returns (TrackTable, planted (F,) bool, contaminated (T,) bool)."""
    from orthosfm_amd import pipeline as P
    V = iset.num_views
    seen = {}
    for v in range(V):
        for i, l in enumerate(iset.landmark[v]):
            if l >= 0:
                seen.setdefault(int(l), []).append((v, i))
    tracks = [seen[l] for l in sorted(seen) if len(seen[l]) >= 2]
    T = len(tracks)
    ln = np.array([len(t) for t in tracks])
    u = synth.uniform(cc.SEED, cc._ST | 0xD0, 3 * T).reshape(T, 3)
    long_ = np.nonzero(ln >= min_len)[0]
    chosen = long_[np.argsort(u[long_, 0], kind="stable")][:int(round(share * long_.size))]
    free = [list(np.nonzero(iset.landmark[v] < 0)[0]) for v in range(V)]
    contaminated = np.zeros(T, dtype=bool)
    chosen = set(chosen.tolist())
    view, feat, planted = [], [], []
    for t, tr in enumerate(tracks):
        hit = int(u[t, 1] * len(tr)) if t in chosen else -1
        for k, (v, i) in enumerate(tr):
            if k == hit and free[v]:
                i = int(free[v].pop(int(u[t, 2] * len(free[v]))))
                contaminated[t] = True
                planted.append(True)
            else:
                planted.append(False)
            view.append(v); feat.append(i)
    view, feat = np.array(view, dtype=np.int32), np.array(feat, dtype=np.int32)
    xy = np.stack([iset.pos[v][i] for v, i in zip(view, feat)]).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    return P.TrackTable(offsets, view, feat, xy, V), np.array(planted), contaminated


def _rotation_errors_deg(P, model, cams, aligned, iset):
    gt, _ = P.canonical_ground_truth(iset, model)
    out = []
    for v in aligned:
        R = P._cam_rotation(model, cams[v]).T @ P._cam_rotation(model, gt[v])
        out.append(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))
    return np.array(out)


def test_pipeline_drops_the_planted_features():
    """run_pose_estimation on a landmark table with planted distractors: under track_filter="consensus" the scene and
    the per-call form agree to the bit, no planted feature survives in a living track with three or more good
    features, and every dropped feature belongs to a contaminated track."""
    from orthosfm_amd import ba as B
    from orthosfm_amd import pipeline as P
    iset = synth.make_image_set(12, 300, config_id=74)
    model = B.MODEL_QUATERNION
    runs = {}
    for key, kw in (("reference", dict(track_filter="reference")), ("consensus", dict(track_filter="consensus")),
                    ("consensus_per_call", dict(track_filter="consensus", use_scene=False))):
        tt, planted, contaminated = _landmark_table(iset)
        tm, cs = P.Timings(), {}
        cams, aligned, groups, calls, _ = P.run_pose_estimation(tt, iset, model, seed=11, timings=tm, consensus_stats=cs, **kw)
        runs[key] = P.Result(cams, aligned, tt, groups, tm, calls, consensus_stats=cs)
        rot = _rotation_errors_deg(P, model, cams, aligned, iset)
        good = np.bincount(tt.track_of[~planted], minlength=tt.alive_t.shape[0])
        survive = planted & tt.alive_f & tt.alive_t[tt.track_of]
        print(f"\n[consensus pipeline] {key}: {len(aligned)} cameras, rotation error max {rot.max():.2e} mean {rot.mean():.2e} deg; "
              f"{int(contaminated.sum())} contaminated tracks, {int(planted.sum())} planted, "
              f"{int(survive.sum())} planted alive ({int((survive & (good[tt.track_of] >= 3)).sum())} with >= 3 good), "
              f"{int((~tt.alive_f).sum())} features dropped ({int((~tt.alive_f & ~contaminated[tt.track_of]).sum())} in clean tracks), "
              f"{int((~tt.alive_t).sum())} tracks dead; stats {cs}; consensus {tm.consensus_filter_s * 1e3:.1f} ms")
    assert contaminated.sum() >= 10
    _same(runs["consensus"], runs["consensus_per_call"])
    assert runs["consensus"].consensus_stats == runs["consensus_per_call"].consensus_stats
    assert runs["consensus"].consensus_stats["calls"] >= 2 and runs["consensus"].timings.consensus_filter_s > 0.0
    tt = runs["consensus"].tracks
    good = np.bincount(tt.track_of[~planted], minlength=tt.alive_t.shape[0])
    survive = planted & tt.alive_f & tt.alive_t[tt.track_of] & (good[tt.track_of] >= 3)
    assert not survive.any(), np.nonzero(survive)[0]
    dropped = ~tt.alive_f
    assert dropped.any() and contaminated[tt.track_of[dropped]].all(), np.nonzero(dropped & ~contaminated[tt.track_of])[0]
