"""osfm_tk_align / osfm_tk_resolve_ambiguity / osfm_scene_tk_align on the GPU against the numpy restatement
(tests/tk_restatement.py) on the seeded cases of tests/tk_cases.py, and the pipeline that starts every camera
group from the Tomasi-Kanade model instead of a perturbed ground-truth pose.

Tolerances: both sides are float64; tests/test_tk_cases_cpu.py bounds the conditioning of every hypothesis of every
case so that rounding stays below 1e-9 and keeps every decision (threshold, usability, rank, selection) off its
boundary, so the integer results are compared for equality and the real ones to 1e-8 (a factor 10 on the bound)."""
import ctypes as C

import numpy as np
import pytest

import tk_cases
import tk_restatement as R

pytestmark = pytest.mark.gpu


def _align(name, **over):
    from orthosfm_amd import tk
    c = tk_cases.BY_NAME[name]
    xy, _, _ = tk_cases.build(name)
    opts = tk_cases.options(name)
    opts.update(over)
    group = opts.pop("group_id")
    return tk.align(xy, c.width, c.height, group_id=group, **opts)


@pytest.mark.parametrize("name", [c.name for c in tk_cases.CASES])
def test_case_against_restatement(name):
    ref = tk_cases.reference(name)
    _, _, truth = tk_cases.build(name)
    got = _align(name)
    print(name, "status", got.status, "usable", got.usable_models, "supported", got.supported_models, "best", got.best_iteration,
          "inliers", got.num_inliers, "mean", got.mean_error_px, "ref mean", ref.mean_error_px, "score ms", got.score_kernel_ms)
    assert got.status == ref.status
    assert got.iterations == ref.iterations
    assert got.usable_models == ref.usable_models
    assert got.supported_models == ref.supported_models
    assert got.num_inliers == ref.num_inliers
    assert np.array_equal(got.inlier, ref.inlier)
    assert abs(got.mean_error_px - ref.mean_error_px) <= 1e-8
    if name == "exact40":
        # every model has all 30 other tracks and a mean error at rounding level: which one wins is not compared,
        # the rotations are held to the ground truth instead
        err = min(max(R.rotation_error_deg(B[k], truth[k]) for k in range(3)) for B in (got.basis_1, got.basis_2))
        assert err < 1e-4
        return
    assert got.best_iteration == ref.best_iteration
    print(name, "max |basis - ref|", np.abs(got.basis_1 - ref.basis_1).max(), "offsets", np.abs(got.offsets - ref.offsets).max())
    assert np.abs(got.basis_1 - ref.basis_1).max() <= 1e-8
    assert np.abs(got.basis_2 - ref.basis_2).max() <= 1e-8
    assert np.abs(got.offsets - ref.offsets).max() <= 1e-8


def test_repeatable_and_group_streams():
    a, b = _align("n2053"), _align("n2053")
    for f in ("basis_1", "basis_2", "offsets", "inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()
    assert (a.best_iteration, a.num_inliers, a.mean_error_px) == (b.best_iteration, b.num_inliers, b.mean_error_px)
    g0, g17 = _align("n300", group_id=0), _align("n300", group_id=17)
    assert g0.status == g17.status == R.STATUS_RANSAC
    assert g0.best_iteration != g17.best_iteration or g0.basis_1.tobytes() != g17.basis_1.tobytes()
    ref17 = R.align(tk_cases.build("n300")[0], 2048, 2048, seed=tk_cases.BY_NAME["n300"].seed, group_id=17)
    assert g17.best_iteration == ref17.best_iteration and np.array_equal(g17.inlier, ref17.inlier)


def _raw_align(xy, n, c, sample_size=10, want_inlier=True, want_offsets=True, null_xy=False):
    from orthosfm_amd import capi
    o = capi.TkOptions()
    capi.check(capi.lib.osfm_tk_options_default(C.byref(o)))
    o.sample_size = sample_size
    o.seed = 2
    b1, b2, off = np.zeros((9, 9)), np.zeros((9, 9)), np.zeros((9, 2))
    inl = np.zeros(max(n, 1), dtype=np.uint8)
    r = capi.TkResult()
    st = capi.lib.osfm_tk_align(None if null_xy else xy.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(n), C.c_int32(c),
                                C.c_int32(2048), C.c_int32(2048), C.byref(o), C.c_uint64(0), capi._ptr(b1, C.c_double),
                                capi._ptr(b2, C.c_double), capi._ptr(off, C.c_double) if want_offsets else None,
                                capi._ptr(inl, C.c_uint8) if want_inlier else None, C.byref(r))
    return st, b1, r


def test_arguments():
    from orthosfm_amd import capi
    xy = np.ascontiguousarray(tk_cases.build("n300")[0])
    st, b_full, r_full = _raw_align(xy, 300, 3)
    assert st == capi.OK and r_full.status == capi.TK_RANSAC
    for kw in (dict(want_inlier=False), dict(want_offsets=False), dict(want_inlier=False, want_offsets=False)):
        st, b, r = _raw_align(xy, 300, 3, **kw)
        assert st == capi.OK and r.best_iteration == r_full.best_iteration and b.tobytes() == b_full.tobytes()
    wide = np.zeros((40, 9, 2))
    assert _raw_align(wide, 40, 2)[0] == capi.E_ARG
    assert _raw_align(wide, 40, 9)[0] == capi.E_ARG
    assert _raw_align(xy, 300, 3, sample_size=3)[0] == capi.E_ARG
    assert _raw_align(xy, 300, 3, null_xy=True)[0] == capi.E_ARG
    d = capi.TkOptions()
    capi.check(capi.lib.osfm_tk_options_default(C.byref(d)))
    assert (d.sample_size, d.max_iterations, d.probability, d.inlier_ratio, d.min_consensus, d.max_error_px) == \
        (10, 0, 0.999, 0.7, 25, 3.0)


def test_resolve_ambiguity():
    from orthosfm_amd import tk
    got = _align("c5")
    Q = tk_cases.quat_to_mat(np.array([0.3, -0.5, 0.2, 0.7]))
    for model, want in ((got.basis_1, 1), (got.basis_2, 2)):
        G = np.array([Q @ b for b in model])                       # global cameras: the model under an arbitrary rotation
        assert tk.resolve_ambiguity(got.basis_1, got.basis_2, G, [1, 1, 1, 1, 1]) == want
        assert tk.resolve_ambiguity(got.basis_1, got.basis_2, G, [0, 1, 0, 1, 1]) == want     # the first view is the new one
        assert tk.resolve_ambiguity(got.basis_1, got.basis_2, G, [0, 0, 0, 1, 0]) == 1        # fewer than two shared views
        assert tk.resolve_ambiguity(got.basis_1, got.basis_2, G, [0, 0, 0, 0, 0]) == 1
        for flags in ([1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [0, 0, 0, 1, 0]):
            assert tk.resolve_ambiguity(got.basis_1, got.basis_2, G, flags) == R.resolve_ambiguity(got.basis_1, got.basis_2, G, flags)


def test_scene_form_equals_per_call_form():
    """A small scene of 5 views and ~400 tracks, some flags cleared: the scene selects the live tracks all three
    views see on the device; the same selection made on the host and handed to osfm_tk_align gives the same bytes."""
    from orthosfm_amd import tk
    from orthosfm_amd.scene import Scene
    rng = np.random.default_rng(5)
    xy3, _, _ = tk_cases.build("n300")                              # views 3, 0, 4 of the scene carry this group
    group = [3, 0, 4]
    V, T = 5, 400
    views_of, feats = [], []
    for t in range(T):
        if t < 300:
            vs = list(group) + [v for v in (1, 2) if rng.random() < 0.5]
        else:
            vs = [v for v in range(V) if rng.random() < 0.5] or [1]
            if set(group) <= set(vs):
                vs.remove(4)
        vs = sorted(vs)
        views_of.append(vs)
        for v in vs:
            feats.append(xy3[t, group.index(v)] if t < 300 and v in group else rng.uniform(0, 2048, 2))
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in views_of])]).astype(np.int64)
    feat_view = np.concatenate(views_of).astype(np.int32)
    feat_xy = np.array(feats, dtype=np.float32)
    alive_t = rng.random(T) > 0.1
    alive_f = rng.random(feat_view.shape[0]) > 0.05
    sc = Scene(0, np.full(V, 2048, np.int32), np.full(V, 2048, np.int32), offsets, feat_view, feat_xy)
    sc.set_flags(alive_t, alive_f)
    # the host's selection
    rows = []
    for t in range(T):
        if not alive_t[t]:
            continue
        f = {int(feat_view[k]): k for k in range(offsets[t], offsets[t + 1]) if alive_f[k]}
        if all(v in f for v in group):
            rows.append([feat_xy[f[v]].astype(np.float64) for v in group])
    xy = np.array(rows)
    assert 150 < xy.shape[0] < 300
    a = sc.tk_align(group, group_id=3, seed=9)
    b = tk.align(xy, 2048, 2048, group_id=3, seed=9)
    # with all but a few tracks gone the group is refused, not fitted
    sc.set_flags(alive_t & (np.arange(T) < 12), None)
    few = sc.tk_align(group, group_id=3, seed=9)
    sc.close()
    assert few.status == R.STATUS_TOO_FEW and 0 < few.num_tracks < 10 and few.iterations == 0 and not few.inlier.any()
    assert np.array_equal(few.basis_1, np.tile(np.eye(3), (3, 1, 1)))
    assert a.num_tracks == xy.shape[0] and a.status == b.status == R.STATUS_RANSAC
    for f in ("basis_1", "basis_2", "offsets", "inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.iterations, a.usable_models, a.supported_models, a.best_iteration, a.num_inliers, a.mean_error_px) == \
        (b.iterations, b.usable_models, b.supported_models, b.best_iteration, b.num_inliers, b.mean_error_px)


@pytest.fixture(scope="module")
def iset():
    from orthosfm_amd import synth
    return synth.make_image_set(9, 1500, config_id=71, twin_frac=0.2)


@pytest.mark.parametrize("solver", [0, 3])
def test_pipeline_starts_from_tk(iset, solver):
    """reconstruct(..., initial_alignment="tk"): no pose is known beforehand.  The reconstruction lives in the frame
    of its first aligned camera (normalizeScene, reconstruct.cpp:228), so canonical_ground_truth is expressed in
    that frame before the comparison (the identity when that camera is view 0)."""
    from orthosfm_amd import pipeline as P
    res = P.reconstruct(iset, solver=solver, seed=11, initial_alignment="tk")
    per_call = P.reconstruct(iset, solver=solver, seed=11, initial_alignment="tk", use_scene=False)
    V = iset.num_views
    assert sorted(res.aligned_views) == list(range(V))
    assert len(res.initial_alignments) == len(res.groups)
    print("tk status per group", [a.status for a in res.initial_alignments], "tracks", [a.num_tracks for a in res.initial_alignments],
          "inliers", [a.num_inliers for a in res.initial_alignments])
    assert all(a.status == R.STATUS_RANSAC for a in res.initial_alignments)          # no group ends FALLBACK
    assert np.array_equal(res.cam_params, per_call.cam_params)
    assert res.aligned_views == per_call.aligned_views
    model = 0 if solver == 0 else 1
    gt, _ = P.canonical_ground_truth(iset, model)
    first = P._cam_rotation(model, gt[res.aligned_views[0]])
    worst = 0.0
    for v in range(V):
        Rg, Rc = first.T @ P._cam_rotation(model, gt[v]), P._cam_rotation(model, res.cam_params[v])
        worst = max(worst, R.rotation_error_deg(Rg, Rc))
    print("solver", solver, "first aligned view", res.aligned_views[0], "worst camera %.3g deg" % worst)
    assert worst < 0.02
    assert res.timings.initial_alignment_s > 0
