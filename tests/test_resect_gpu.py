"""osfm_resect_view / osfm_scene_resect_view on the GPU against the numpy restatement (tests/resect_restatement.py) on
the seeded cases of tests/resect_cases.py, and the pipeline that places the views of weak camera groups by resection.

Tolerances: both sides are float64; tests/test_resect_cases_cpu.py bounds the conditioning of every hypothesis of
every case so that rounding stays below 1e-9 and keeps every decision (error threshold, pivot, axis ratio, support,
selection, the refit's pivot) off its boundary, so the integer results and the inlier bytes are compared for equality
and the real ones to 1e-8 (a factor 10 on the bound): the argument of tests/test_tk_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import resect_cases as RC
import resect_restatement as R

pytestmark = pytest.mark.gpu

INT_FIELDS = ("status", "iterations", "usable_models", "supported_models", "best_iteration", "ransac_inliers", "num_inliers",
              "refit_used")


def _resect(name, **over):
    from orthosfm_amd import resect
    c = RC.BY_NAME[name]
    X, xy, _, _ = RC.build(name)
    opts = c.options()
    opts.update(over)
    stream = opts.pop("stream_id", c.stream_id)
    return resect.resect(X, xy, c.width, c.height, stream_id=stream, **opts)


@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_case_against_restatement(name):
    ref = RC.reference(name)
    got = _resect(name)
    print(name, {f: getattr(got, f) for f in INT_FIELDS}, "mean", got.mean_error_px, "score ms", got.score_kernel_ms)
    for f in INT_FIELDS:
        assert getattr(got, f) == getattr(ref, f), f
    assert got.num_points == RC.BY_NAME[name].n
    assert np.array_equal(got.inlier, ref.inlier)
    diffs = (np.abs(got.rotation - ref.rotation).max(), abs(got.scale - ref.scale), np.abs(got.offsets - ref.offsets).max(),
             abs(got.mean_error_px - ref.mean_error_px))
    print(name, "max |rotation - ref| %.3g, |scale - ref| %.3g, max |offsets - ref| %.3g, |mean - ref| %.3g" % diffs)
    assert max(diffs) <= 1e-8
    if got.status == R.STATUS_OK:
        assert np.abs(got.rotation @ got.rotation.T - np.eye(3)).max() < 1e-12 and np.linalg.det(got.rotation) > 0.0
    else:
        assert np.array_equal(got.rotation, np.eye(3)) and got.scale == 1.0 and not got.offsets.any() and not got.inlier.any()
        assert got.best_iteration == -1


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("name", ["n257", "scale_est"])
def test_placement_to_params_against_the_reprojection_kernel(name, model):
    """The converted camera under osfm_ba_reprojection_errors gives the inliers the errors the resection gave them."""
    from orthosfm_amd import ba, resect
    c = RC.BY_NAME[name]
    X, xy, _, _ = RC.build(name)
    got = _resect(name)
    assert got.status == R.STATUS_OK
    p = resect.placement_to_params(model, got)
    inl = np.flatnonzero(got.inlier)
    const = np.ones((1, 7), dtype=np.uint8)
    prob = ba.FlatProblem(model, p[None], const, [c.width], [c.height], np.column_stack([X[inl], np.ones(inl.size)]), xy[inl],
                          np.zeros(inl.size, np.int32), np.arange(inl.size, dtype=np.int32))
    err, _ = ba.reprojection_errors(prob)
    u, v = R.normalise(xy, c.width, c.height)
    x, y = got.rotation[:, 0], got.rotation[:, 1]
    own = R.errors(x / got.scale, -got.offsets[0], y / got.scale, -got.offsets[1], X, u, v, c.width, c.height)
    print(name, "model", model, "max |kernel - own| %.3g px" % np.abs(err - own[inl]).max())
    assert np.abs(err - own[inl]).max() <= 1e-8
    assert (own[inl] < 3.0).all() and (own[~got.inlier] >= 3.0).all()
    assert abs(err.mean() - got.mean_error_px) <= 1e-8


def test_repeatable_and_streams():
    for name in ("n513", "out60"):
        a, b = _resect(name), _resect(name)
        for f in ("rotation", "offsets", "inlier"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (name, f)
        assert [getattr(a, f) for f in INT_FIELDS + ("scale", "mean_error_px")] == \
            [getattr(b, f) for f in INT_FIELDS + ("scale", "mean_error_px")]
    s0, s17 = _resect("n257", stream_id=0), _resect("n257", stream_id=17)
    assert s0.status == s17.status == R.STATUS_OK
    assert s0.best_iteration != s17.best_iteration or s0.rotation.tobytes() != s17.rotation.tobytes()
    c = RC.BY_NAME["n257"]
    X, xy, _, _ = RC.build("n257")
    ref17 = R.resect(X, xy, c.width, c.height, stream_id=17, **c.options())
    assert s17.best_iteration == ref17.best_iteration and s17.usable_models == ref17.usable_models
    assert np.array_equal(s17.inlier, ref17.inlier)


def _raw(points, xy, n, opts=None, null=(), width=2048, height=2048):
    from orthosfm_amd import capi
    rot, off, scale = np.zeros(9), np.zeros(2), C.c_double()
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    r = capi.ResectResult()
    st = capi.lib.osfm_resect_view(None if "points" in null else points.ctypes.data, None if "xy" in null else xy.ctypes.data,
                                   n, width, height, None if opts is None else C.byref(opts), 0,
                                   None if "rotation" in null else rot.ctypes.data, None if "scale" in null else C.byref(scale),
                                   None if "offsets" in null else off.ctypes.data, None if "inlier" in null else inl.ctypes.data,
                                   None if "result" in null else C.byref(r))
    return st, rot, r


def test_arguments():
    from orthosfm_amd import capi, resect
    X, xy, _, _ = RC.build("n257")
    X, xy = np.ascontiguousarray(X), np.ascontiguousarray(xy)
    st, rot_full, r_full = _raw(X, xy, 257)
    assert st == capi.OK and r_full.status == capi.RESECT_OK and r_full.iterations == 107       # NULL options: the defaults
    st, rot, r = _raw(X, xy, 257, null=("inlier",))
    assert st == capi.OK and r.best_iteration == r_full.best_iteration and rot.tobytes() == rot_full.tobytes()
    for what in ("points", "xy", "rotation", "scale", "offsets", "result"):
        assert _raw(X, xy, 257, null=(what,))[0] == capi.E_ARG, what
    assert _raw(X, xy, -1)[0] == capi.E_ARG
    assert _raw(X, xy, 257, width=0)[0] == capi.E_ARG and _raw(X, xy, 257, height=-5)[0] == capi.E_ARG
    for bad in (dict(probability=0.0), dict(probability=1.0), dict(inlier_ratio=0.0), dict(inlier_ratio=1.0), dict(max_error_px=0.0),
                dict(max_error_px=float("nan")), dict(min_consensus=-1), dict(max_iterations=-1), dict(max_iterations=(1 << 20) + 1),
                dict(min_pivot=0.0), dict(min_pivot=1.0), dict(min_axis_ratio=-0.1), dict(min_axis_ratio=1.5), dict(scale=0.0),
                dict(scale=float("inf"))):
        assert _raw(X, xy, 257, resect.options(**bad))[0] == capi.E_ARG, bad
    st, _, r = _raw(X, xy, 0)
    assert st == capi.OK and r.status == capi.RESECT_TOO_FEW and r.iterations == 0 and r.best_iteration == -1
    d = capi.ResectOptions()
    capi.check(capi.lib.osfm_resect_options_default(C.byref(d)))
    assert (d.max_iterations, d.probability, d.inlier_ratio, d.min_consensus, d.max_error_px, d.min_pivot, d.min_axis_ratio,
            d.estimate_scale, d.scale, d.seed, d.device) == (0, 0.999, 0.5, 8, 3.0, 1e-6, 0.5, 0, 1.0, 0, 0)
    # the scene entry
    from orthosfm_amd.scene import Scene
    sc = Scene(0, [64, 64], [64, 64], np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.zeros((2, 2), np.float32))
    rot, off, scale, res, n = np.zeros(9), np.zeros(2), C.c_double(), capi.ResectResult(), C.c_int32()
    inl = np.zeros(4, np.uint8)

    def scene_call(view=0, opts=None, capacity=4, rotation=True, result=True):
        return capi.lib.osfm_scene_resect_view(sc._h_scene, view, None if opts is None else C.byref(opts), 0,
                                               rot.ctypes.data if rotation else None, C.byref(scale), off.ctypes.data,
                                               inl.ctypes.data, capacity, C.byref(res) if result else None, C.byref(n))
    assert scene_call() == capi.OK and res.status == capi.RESECT_TOO_FEW and n.value == 0
    assert scene_call(view=2) == capi.E_ARG and scene_call(view=-1) == capi.E_ARG
    assert scene_call(capacity=-1) == capi.E_ARG
    assert scene_call(rotation=False) == capi.E_ARG and scene_call(result=False) == capi.E_ARG
    assert scene_call(opts=resect.options(inlier_ratio=2.0)) == capi.E_ARG
    assert capi.lib.osfm_scene_resect_view(None, 0, None, 0, rot.ctypes.data, C.byref(scale), off.ctypes.data, None, 0,
                                           C.byref(res), None) == capi.E_ARG
    sc.close()


SCENE_VIEWS, SCENE_TRACKS, NEW_VIEW = 6, 257, 4


def _same(a, b):
    for f in ("rotation", "offsets", "inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for f in INT_FIELDS + ("scale", "mean_error_px", "num_points"):
        assert getattr(a, f) == getattr(b, f), f


def _host_form(scene, view, feat_view, track_of, feat_xy, **kw):
    """The scene's correspondences selected on the host from its download, handed to the per-call entry."""
    from orthosfm_amd import resect
    at, af, hp, pt = scene.download()
    f = np.flatnonzero((feat_view == view) & af & at[track_of] & hp[track_of])
    P4 = pt[track_of[f]]
    return resect.resect(P4[:, :3] / P4[:, 3:4], feat_xy[f].astype(np.float64), 2048, 2048, **kw), f


@pytest.mark.parametrize("model", [0, 1])
def test_scene_form_equals_per_call_form(model, monkeypatch):
    """6 views, 257 tracks that all views see, 30 % of view 4's features shifted: views 0, 1, 2, 3, 5 are aligned at the
    ground truth and triangulated, view 4 is resected on the device and, from the scene's download, through the
    per-call entry: the same bytes.  Once more after flags were cleared (dead features, dead tracks, and tracks left
    with one ray, which lose their point), and once on a scene that has compacted."""
    from orthosfm_amd import synth
    from orthosfm_amd.pipeline import _cam_rotation
    from orthosfm_amd.scene import Scene
    T, V = SCENE_TRACKS, SCENE_VIEWS
    bs = synth.make_ba_scene(model, V, T, min_len=V, max_len=V, noise_px=0.2, config_id=77)
    order = np.lexsort((bs.obs_camera, bs.obs_point))                       # track-major, views ascending
    feat_view = bs.obs_camera[order].astype(np.int32)
    track_of = bs.obs_point[order].astype(np.int64)
    feat_xy = bs.obs_xy[order].astype(np.float32)
    rng = np.random.default_rng(3)
    mine = np.flatnonzero(feat_view == NEW_VIEW)
    shifted = mine[rng.permutation(T)[:77]]
    feat_xy[shifted] += rng.choice([-1.0, 1.0], (77, 2)).astype(np.float32) * rng.uniform(40.0, 200.0, (77, 2)).astype(np.float32)
    offsets = np.arange(0, V * T + 1, V, dtype=np.int64)
    sc = Scene(model, np.full(V, 2048, np.int32), np.full(V, 2048, np.int32), offsets, feat_view, feat_xy)
    others = [v for v in range(V) if v != NEW_VIEW]
    const = np.ones((len(others), 7), dtype=np.uint8)
    sc.align_views(others, bs.gt_cams[others], const)
    sc.triangulate()
    kw = dict(stream_id=5, seed=9)
    a = sc.resect_view(NEW_VIEW, **kw)
    b, f = _host_form(sc, NEW_VIEW, feat_view, track_of, feat_xy, **kw)
    assert a.num_points == T == f.size and a.status == R.STATUS_OK
    _same(a, b)
    assert np.array_equal(a.inlier, ~np.isin(mine, shifted))
    err = R.rotation_error_deg(a.rotation, _cam_rotation(model, bs.gt_cams[NEW_VIEW]))
    print("model", model, "resected view", NEW_VIEW, "%.4f deg from the ground truth, %d inliers" % (err, a.num_inliers))
    assert err < 0.1
    # flags cleared: every 7th track dead, every 11th feature dead, every 5th track keeps only its features in views 4 and 0
    alive_t = np.arange(T) % 7 != 3
    alive_f = np.arange(V * T) % 11 != 5
    one_ray = (track_of % 5 == 1) & ~np.isin(feat_view, (NEW_VIEW, 0))
    alive_f &= ~one_ray
    sc.set_flags(alive_t, alive_f)
    sc.triangulate()
    at, af, hp, _ = sc.download()
    live_mine = af[mine] & at
    assert (live_mine & ~hp).sum() > 20 and (~af[mine]).sum() > 10 and (~at).sum() > 30      # all three kinds are skipped
    a2 = sc.resect_view(NEW_VIEW, **kw)
    b2, f2 = _host_form(sc, NEW_VIEW, feat_view, track_of, feat_xy, **kw)
    assert a2.num_points == f2.size == int((live_mine & hp).sum()) < a.num_points and a2.status == R.STATUS_OK
    _same(a2, b2)
    # a compacted scene: the dead tracks are dropped from the table, the correspondences stay the same
    monkeypatch.setenv("OSFM_SCENE_COMPACT", "2")
    sc.filter_outliers()
    a3 = sc.resect_view(NEW_VIEW, **kw)
    b3, f3 = _host_form(sc, NEW_VIEW, feat_view, track_of, feat_xy, **kw)
    sc.close()
    assert 0 < a3.num_points == f3.size <= a2.num_points and a3.status == R.STATUS_OK
    _same(a3, b3)


@pytest.fixture(scope="module")
def iset():
    from orthosfm_amd import synth
    return synth.make_image_set(9, 1500, config_id=71, twin_frac=0.2)


UNREACHABLE = {"min_consensus": 1_000_000}          # no group has that many tracks: every alignment ends in the fallback


@pytest.mark.parametrize("solver", [0, 3])
def test_pipeline_resects_weak_groups(iset, solver):
    """The set of test_pipeline_starts_from_tk with a Tomasi-Kanade min_consensus no group can reach.  weak_group =
    "resect": every group but the first is resected, all views are aligned, and the worst camera is within the bound
    of that test; the per-call form gives the same cameras.  The default policy takes the fallback as before."""
    from orthosfm_amd import capi
    from orthosfm_amd import pipeline as P
    res = P.reconstruct(iset, solver=solver, seed=11, initial_alignment="tk", weak_group="resect", tk_options=UNREACHABLE)
    per_call = P.reconstruct(iset, solver=solver, seed=11, initial_alignment="tk", weak_group="resect", tk_options=UNREACHABLE,
                             use_scene=False)
    V = iset.num_views
    G = len(res.groups)
    assert all(a.status == capi.TK_FALLBACK for a in res.initial_alignments) and len(res.initial_alignments) == G
    assert res.resected_groups == list(range(1, G)) and res.timings.resected_groups == G - 1 > 0
    assert sorted(res.aligned_views) == list(range(V))
    assert per_call.resected_groups == res.resected_groups
    assert np.array_equal(res.cam_params, per_call.cam_params) and res.aligned_views == per_call.aligned_views
    model = 0 if solver == 0 else 1
    gt, _ = P.canonical_ground_truth(iset, model)
    first = P._cam_rotation(model, gt[res.aligned_views[0]])
    worst = 0.0
    for v in range(V):
        Rg, Rc = first.T @ P._cam_rotation(model, gt[v]), P._cam_rotation(model, res.cam_params[v])
        worst = max(worst, R.rotation_error_deg(Rg, Rc))
    print("solver", solver, "groups", G, "resected", res.resected_groups, "worst camera %.3g deg" % worst)
    assert worst < 0.02
    plain = P.reconstruct(iset, solver=solver, seed=11, initial_alignment="tk", tk_options=UNREACHABLE)
    assert all(a.status == capi.TK_FALLBACK for a in plain.initial_alignments) and len(plain.initial_alignments) == G
    assert plain.resected_groups == [] and plain.timings.resected_groups == 0
    assert sorted(plain.aligned_views) == list(range(V))
