"""The one-workgroup form of the bundle adjustment (osfm_ba_options::small_form, orthosfm_amd/csrc/ba_small.hip):
the whole Levenberg-Marquardt solve of a problem of at most eight cameras in one launch of one workgroup.

Held against the CPU oracle with the bounds of tests/test_ba_gpu.py (_compare_solve there, copied below: double
precision on both sides, another summation order), every case once with small_form=2 and once, as its control, with
small_form=0; against the general form with the project's bounds for two forms that only sum in another order
(test_one_launch_cholesky_equals_launch_per_column: 1e-12 of the final cost, 1e-10 on cameras, 1e-9 on points); at
the boundaries of the chunks it walks the tracks in; for repeatability to the bit; through the switch, the scene and
the pipeline."""
import functools
import threading

import numpy as np
import pytest

import oracle_lib
from orthosfm_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    from orthosfm_amd import ba as m
    from orthosfm_amd import capi
    assert capi.device_count() >= 1
    return m


def _drop_tracks(sc, tracks):
    keep = ~np.isin(sc.obs_point, tracks)
    sc.obs_xy, sc.obs_camera, sc.obs_point = sc.obs_xy[keep], sc.obs_camera[keep], sc.obs_point[keep]
    return sc


def _huber_scene():
    sc = synth.make_ba_scene(0, 8, 3000, config_id=35)
    sc.obs_xy[::41] += 25.0
    return sc


def _all_seen_by_three(M, single_last=False):
    """Three cameras, every track seen by all three; single_last: the last track keeps one observation."""
    sc = synth.make_ba_scene(0, 3, M, config_id=82, min_len=3, max_len=3)
    assert np.array_equal(np.bincount(sc.obs_point, minlength=M), np.full(M, 3))
    if single_last:
        last = np.nonzero(sc.obs_point == M - 1)[0]
        keep = np.ones(sc.obs_point.shape[0], bool)
        keep[last[1:]] = False
        sc.obs_xy, sc.obs_camera, sc.obs_point = sc.obs_xy[keep], sc.obs_camera[keep], sc.obs_point[keep]
        assert np.bincount(sc.obs_point, minlength=M)[-1] == 1
    return sc


def _chunk():
    from orthosfm_amd import ba as m
    return m.small_limits()[1]


# name -> (scene builder, options of the solve, the points are re-triangulated first)
CASES = {
    "handful-0-3-2500": (lambda: synth.make_ba_scene(0, 3, 2500, config_id=81, min_len=3, max_len=3), {}, False),
    "handful-1-3-400": (lambda: synth.make_ba_scene(1, 3, 400, config_id=81, min_len=2, max_len=3), {}, False),
    "handful-0-8-3000": (lambda: synth.make_ba_scene(0, 8, 3000, config_id=81, min_len=2, max_len=8), {}, False),
    "handful-0-6-50": (lambda: synth.make_ba_scene(0, 6, 50, config_id=81, min_len=1, max_len=4), {}, False),
    "fixed-camera-quat": (lambda: synth.make_ba_scene(0, 8, 300, config_id=34), {}, False),
    "fixed-camera-euler": (lambda: synth.make_ba_scene(1, 8, 300, config_id=34), {}, False),
    "huber": (_huber_scene, {}, False),
    "euler-free-1": (lambda: synth.make_ba_scene(1, 7, 250, config_id=39, euler_free=1), {}, False),
    "euler-free-2": (lambda: synth.make_ba_scene(1, 7, 250, config_id=40, euler_free=2), {}, False),
    "euler-free-3": (lambda: synth.make_ba_scene(1, 7, 250, config_id=41, euler_free=3), {}, False),
    "constant-points": (lambda: synth.make_ba_scene(0, 6, 200, config_id=36, point_perturb=0.0, noise_px=0.2),
                        {"optimize_points": 0}, False),
    "retriangulate": (lambda: synth.make_ba_scene(0, 3, 2500, config_id=81, min_len=3, max_len=3), {}, True),
    "empty-tracks": (lambda: _drop_tracks(synth.make_ba_scene(0, 8, 900, config_id=63), np.arange(5, 900, 37)),
                     {"max_num_iterations": 5}, False),
    "chunk-minus-1": (lambda: _all_seen_by_three(_chunk() - 1), {}, False),
    "chunk": (lambda: _all_seen_by_three(_chunk()), {}, False),
    "chunk-plus-1": (lambda: _all_seen_by_three(_chunk() + 1), {}, False),
    "two-chunks-plus-1": (lambda: _all_seen_by_three(2 * _chunk() + 1), {}, False),
    "last-chunk-one-observation": (lambda: _all_seen_by_three(_chunk() + 1, single_last=True), {}, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's scene and the oracle's solve of it, made once and shared by the two forms: copied before use."""
    build, opt, retri = CASES[name]
    sc = build()
    ref = sc.copy()
    if retri:
        oracle_lib.oracle_ba_triangulate(ref)
    so = oracle_lib.oracle_ba_solve(ref, **opt)
    return sc, ref, so


def _compare_solve(ba, name, small_form):
    """tests/test_ba_gpu.py: _compare_solve, its assertions as they stand there."""
    _, opt, retri = CASES[name]
    sc, ref, so = _case(name)
    fp = ba.FlatProblem.from_scene(sc.copy())
    s = ba.solve(fp, small_form=small_form, retriangulate_points=1 if retri else 0, **opt)
    print(f"{name} small_form={small_form}: initial {s.initial_cost!r} / {so.initial_cost!r}, iterations {s.num_iterations} / "
          f"{so.num_iterations}, final {s.final_cost!r} / {so.final_cost!r}, cameras {np.abs(fp.cam_params - ref.cam_params).max():.3e}, "
          f"points {np.abs(fp.points - ref.points).max():.3e}")
    assert np.isclose(s.initial_cost, so.initial_cost, rtol=1e-11)
    assert s.num_iterations == so.num_iterations
    assert s.num_successful_steps == so.num_successful_steps
    assert s.num_unsuccessful_steps == so.num_unsuccessful_steps
    assert s.termination == so.termination
    assert abs(s.final_cost - so.final_cost) <= 1e-9 * max(1.0, abs(so.final_cost))
    assert np.abs(fp.cam_params - ref.cam_params).max() <= 1e-8
    assert np.abs(fp.points - ref.points).max() <= 1e-7
    assert np.isclose(s.mean_point_change, so.mean_point_change, rtol=1e-6, atol=1e-9)
    return s, fp, sc


@pytest.mark.parametrize("small_form", [2, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_one_workgroup_form_meets_the_oracle(ba, name, small_form):
    s, fp, sc = _compare_solve(ba, name, small_form)
    if small_form == 2:
        # what the general form has and this one has not stays 0; the rest is filled
        assert (s.point_pass_ms, s.pair_pass_ms, s.cholesky_ms, s.back_pass_ms) == (0.0, 0.0, 0.0, 0.0)
        assert (s.num_pair_entries, s.flow_fallbacks, s.order_arcs, s.chain_blocks_natural, s.chain_blocks) == (0, 0, 0, 0, 0)
        assert s.linearizations == s.num_successful_steps + s.num_unsuccessful_steps + 1
        assert s.lm_loop_ms >= 0.0 and s.solve_ms > 0.0
    if name.startswith("fixed-camera"):
        assert s.final_cost < s.initial_cost
        assert np.array_equal(fp.cam_params[0], sc.gt_cams[0])         # fixed camera untouched, to the bit
    if name.startswith("euler-free"):
        const = sc.cam_const.astype(bool)
        assert np.array_equal(fp.cam_params[const], sc.cam_params[const])
    if name == "constant-points":
        assert np.array_equal(fp.points, sc.points)
    if name == "empty-tracks":
        assert np.array_equal(fp.points[5::37], sc.points[5::37])
        assert not np.array_equal(fp.points[6], sc.points[6])


@pytest.mark.parametrize("model,cams,pts,lo,hi", [(0, 3, 400, 3, 3), (1, 3, 700, 2, 3), (0, 8, 1000, 2, 8), (1, 5, 300, 1, 5)])
def test_one_workgroup_form_equals_the_general_form(ba, model, cams, pts, lo, hi):
    """Scenes with the generator's default noise (the final cost is far from zero): the two forms sum in another
    order and nothing else -- the same trajectory, the final cost to 1e-12, cameras to 1e-10, points to 1e-9."""
    sc = synth.make_ba_scene(model, cams, pts, config_id=83, min_len=lo, max_len=hi)
    fp1, fp2 = ba.FlatProblem.from_scene(sc.copy()), ba.FlatProblem.from_scene(sc.copy())
    s1 = ba.solve(fp1, small_form=2)
    s2 = ba.solve(fp2, small_form=0)
    print(f"final cost {s1.final_cost!r} / {s2.final_cost!r}, cameras {np.abs(fp1.cam_params - fp2.cam_params).max():.3e}, "
          f"points {np.abs(fp1.points - fp2.points).max():.3e}")
    assert (s1.num_iterations, s1.num_successful_steps, s1.num_unsuccessful_steps, s1.termination) == \
        (s2.num_iterations, s2.num_successful_steps, s2.num_unsuccessful_steps, s2.termination)
    assert s2.final_cost > 1.0
    assert abs(s1.final_cost - s2.final_cost) <= 1e-12 * s2.final_cost
    assert np.abs(fp1.cam_params - fp2.cam_params).max() <= 1e-10
    assert np.abs(fp1.points - fp2.points).max() <= 1e-9


def _solve_bytes(ba, sc, **opt):
    fp = ba.FlatProblem.from_scene(sc.copy())
    s = ba.solve(fp, **opt)
    return (fp.cam_params.tobytes(), fp.points.tobytes(), s.initial_cost, s.final_cost, s.num_iterations, s.termination)


def test_repeats_to_the_bit_alone_and_beside_another_solve(ba):
    sc = synth.make_ba_scene(0, 3, 700, config_id=84, min_len=2, max_len=3)
    first = _solve_bytes(ba, sc, small_form=2)
    assert first[4] >= 2
    for _ in range(2):
        assert _solve_bytes(ba, sc, small_form=2) == first
    out = [None, None]

    def work(k):
        out[k] = _solve_bytes(ba, sc, small_form=2)
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    assert out[0] == first and out[1] == first


def test_the_switch(ba):
    from orthosfm_amd import capi
    sc9 = synth.make_ba_scene(0, 9, 200, config_id=85)
    with pytest.raises(capi.OsfmError) as e:
        ba.solve(ba.FlatProblem.from_scene(sc9.copy()), small_form=2)
    assert e.value.status == capi.E_ARG and "at most 8" in str(e.value)
    assert _solve_bytes(ba, sc9, small_form=1) == _solve_bytes(ba, sc9, small_form=0)
    for bad in (3, -1):
        with pytest.raises(capi.OsfmError) as e:
            ba.solve(ba.FlatProblem.from_scene(sc9.copy()), small_form=bad)
        assert e.value.status == capi.E_ARG
    # the capture of the first iteration is the general form's
    sc3 = synth.make_ba_scene(0, 3, 60, config_id=85, min_len=3, max_len=3)
    with pytest.raises(capi.OsfmError) as e:
        ba.debug_linearization(ba.FlatProblem.from_scene(sc3.copy()), small_form=2)
    assert e.value.status == capi.E_ARG
    # mode 1 below the threshold takes the one-workgroup form, above it the general one
    auto = ba.small_limits()[2]
    for M in (60, max(auto, 0) // 3 + 40):
        scm = synth.make_ba_scene(0, 3, M, config_id=85, min_len=3, max_len=3)
        want = 2 if 3 * M <= auto else 0
        assert _solve_bytes(ba, scm, small_form=1) == _solve_bytes(ba, scm, small_form=want)


def _status_and_counts(ba, fp, small_form):
    from orthosfm_amd import capi
    try:
        s = ba.solve(fp, small_form=small_form)
    except capi.OsfmError as e:
        return (e.status,)
    return (capi.OK, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.termination, s.initial_cost,
            s.final_cost, s.linearizations)


@pytest.mark.parametrize("what", ["no-points", "no-observations"])
def test_empty_problems_behave_as_in_the_general_form(ba, what):
    sc = synth.make_ba_scene(0, 3, 40, config_id=86, min_len=3, max_len=3)
    res = []
    for form in (0, 2):
        c = sc.copy()
        if what == "no-points":
            c.points = np.zeros((0, 4))
        c.obs_xy, c.obs_camera, c.obs_point = np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros(0, np.int32)
        fp = ba.FlatProblem.from_scene(c)
        res.append(_status_and_counts(ba, fp, form))
        assert np.array_equal(fp.cam_params, sc.cam_params)
    print(res)
    assert res[0] == res[1]


@pytest.fixture(scope="module")
def iset():
    return synth.make_image_set(12, 1000, config_id=74)


def _same_reconstruction(a, b):
    """tests/test_e2e_gpu.py: _same_reconstruction (raw feature flags)."""
    assert a.aligned_views == b.aligned_views
    assert np.array_equal(a.cam_params, b.cam_params)
    ta, tb = a.tracks, b.tracks
    assert np.array_equal(ta.alive_t, tb.alive_t)
    assert np.array_equal(ta.alive_f, tb.alive_f)
    assert np.array_equal(ta.live_f, tb.live_f) and np.array_equal(ta.alive_lengths(), tb.alive_lengths())
    assert np.array_equal(ta.has_point & ta.alive_t, tb.has_point & tb.alive_t)
    sel = ta.has_point & ta.alive_t
    assert sel.sum() > 100 and np.array_equal(ta.point[sel], tb.point[sel])
    ca = [(c.kind, c.cameras, c.points, c.observations, c.iterations) for c in a.ba_calls]
    cb = [(c.kind, c.cameras, c.points, c.observations, c.iterations) for c in b.ba_calls]
    assert ca == cb


def test_scene_local_adjustment_equals_the_per_call_form(iset):
    """The scene's local adjustment (osfm_scene_local_adjustment) and osfm_ba_solve on the flattened problem, both in
    the one-workgroup form, over the first camera groups of the reconstruction: the same cameras to the bit."""
    from orthosfm_amd import pipeline as P
    a = P.reconstruct(iset, solver=0, seed=11, use_scene=True, local_solver="small", max_groups=3)
    b = P.reconstruct(iset, solver=0, seed=11, use_scene=False, local_solver="small", max_groups=3)
    assert [c.kind for c in a.ba_calls].count("local") == 3
    _same_reconstruction(a, b)


def test_pipeline_with_the_one_workgroup_local_solver(iset):
    """reconstruct(..., local_solver="small") against the default on a noise-free synthetic set of 12 views: the same
    groups, order, live tracks and features, the cameras within 1e-7, and at the ground truth within the bound
    tests/test_e2e_gpu.py holds the default path to (0.02 degrees)."""
    from orthosfm_amd import pipeline as P
    a = P.reconstruct(iset, solver=0, seed=11, local_solver="small")
    b = P.reconstruct(iset, solver=0, seed=11, local_solver="general")
    assert [(list(g.ids), g.tracks) for g in a.groups] == [(list(g.ids), g.tracks) for g in b.groups]
    assert a.aligned_views == b.aligned_views
    ta, tb = a.tracks, b.tracks
    assert int(ta.alive_t.sum()) == int(tb.alive_t.sum())
    assert int((ta.alive_f & ta.alive_t[ta.track_of]).sum()) == int((tb.alive_f & tb.alive_t[tb.track_of]).sum())
    print("cameras differ by", np.abs(a.cam_params - b.cam_params).max())
    assert np.abs(a.cam_params - b.cam_params).max() <= 1e-7
    gt, _ = P.canonical_ground_truth(iset, 0)
    for res in (a, b):
        for v in range(iset.num_views):
            Rg, Rc = P._cam_rotation(0, gt[v]), P._cam_rotation(0, res.cam_params[v])
            ang = np.degrees(np.arccos(np.clip((np.trace(Rg.T @ Rc) - 1) / 2, -1, 1)))
            assert ang < 0.02, (v, ang)
    kinds = [c.kind for c in a.ba_calls]
    assert kinds.count("local") == iset.num_views - 2
