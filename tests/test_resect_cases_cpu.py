"""The cases of tests/resect_cases.py are fit to judge the resection kernels: on the numpy restatement
(tests/resect_restatement.py) every case reaches the path it is named for, no decision of any hypothesis of any
case sits on its boundary, and the conditioning is bounded so that rounding stays below 1e-9.  That entitles
tests/test_resect_gpu.py to `==` on integers and 1e-8 on reals (the argument of tests/test_tk_cases_cpu.py).

The rounding argument.  A hypothesis solves a 3 x 3 system of condition number k: its matrix carries a relative
error of about 8 eps k, a pixel error |X| W / 2 ~ 1e3 times that.  With k < 1e6 over ALL usable hypotheses the
errors are good to 2e-6 px, so a threshold margin of 2e-5 px decides every inlier test ten times over; the winner
and the refit, whose numbers reach the outputs, have k < 4e5, i.e. rounding below 8 * 2.2e-16 * 4e5 = 7e-10.

Also here: the prototype's scene (6 cameras, 300 / 1000 points, view 4 resected) in both camera models at 30 % and
60 % outliers recovers the rotation far inside the 2 degrees the pipeline's perturbed start is off, and the table of
the pipeline's decision function."""
import numpy as np
import pytest

import resect_cases as RC
import resect_restatement as R

EPS = np.finfo(np.float64).eps
THR_MARGIN_PX = 2e-5
COND_ALL, COND_WINNER = 1e6, 4e5
OK_CASES = [c.name for c in RC.CASES if c.name not in ("coplanar", "mc_edge_no", "toofew11")]


def test_lists_follow_the_kernel_constants():
    """The case lists were made for these values of osfm_resect_limits."""
    from orthosfm_amd import resect
    assert resect.limits() == (RC.TILE, RC.CHUNK) == (256, 16)
    assert [RC.BY_NAME[n].n for n in ("n255", "n256", "n257", "n513")] == [RC.TILE - 1, RC.TILE, RC.TILE + 1, 2 * RC.TILE + 1]
    assert [dict(RC.BY_NAME[n].opts)["max_iterations"] for n in ("h1", "h15", "h16", "h17", "h33")] == \
        [1, RC.CHUNK - 1, RC.CHUNK, RC.CHUNK + 1, 2 * RC.CHUNK + 1]
    assert R.num_iterations() == 107


@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_no_decision_on_its_boundary(name):
    r = RC.reference(name)
    if r.status == R.STATUS_TOO_FEW:
        return
    d = r.detail
    print(name, {k: v for k, v in d.items()})
    assert d["pivot_margin"] > 1e-3                      # |pivot / (min_pivot * largest entry) - 1|
    assert d["cond"] < COND_ALL
    if d["usable"]:
        assert d["thr_margin"] > THR_MARGIN_PX
        assert d["ratio_margin"] > 1e-6
    if r.status != R.STATUS_OK:
        return
    # the selection between the best two: a tie in the inlier count is split by a mean error far above rounding
    assert d["select_margin"] > 1e-6
    assert d["refit_pivot_margin"] > 1e-3
    assert d["final_thr_margin"] > THR_MARGIN_PX
    if r.refit_used:
        assert d["refit_cond"] < COND_WINNER
    c = RC.BY_NAME[name]
    X, xy, _, _ = RC.build(name)
    s = R.sample(c.options()["seed"], c.stream_id, r.best_iteration, c.n)
    assert np.linalg.cond(X[s[1:]] - X[s[0]]) < COND_WINNER
    assert 8 * EPS * COND_WINNER < 1e-9


@pytest.mark.parametrize("name", OK_CASES)
def test_ok_cases_find_their_camera(name):
    r = RC.reference(name)
    _, _, planted, truth = RC.build(name)
    assert r.status == R.STATUS_OK and r.best_iteration >= 0
    assert r.ransac_inliers - R.SAMPLE >= dict(RC.BY_NAME[name].opts).get("min_consensus", 8)
    assert R.rotation_error_deg(r.rotation, truth) < 0.5
    assert not (r.inlier & planted).any()                # no planted outlier is taken in


def test_cases_reach_their_paths():
    ref = RC.reference
    assert ref("clean40").num_inliers == 40 and ref("clean40").detail["supported"] > 50
    # hypothesis counts: one workgroup row of chunks less, exactly, and more than a chunk
    assert [ref(n).iterations for n in ("h1", "h15", "h16", "h17", "h33")] == [1, 15, 16, 17, 33]
    assert ref("h33").best_iteration == 32               # the winner is the last chunk's only hypothesis
    assert ref("h33").detail["supported"] > 1            # ... and had competitors
    for n in ("n255", "n256", "n257", "n513", "out60"):
        assert ref(n).iterations == 107
    # 60 % outliers: the final inliers are exactly the planted inliers
    X, xy, planted, _ = RC.build("out60")
    assert planted.sum() == 360 and np.array_equal(ref("out60").inlier, ~planted)
    # every point in one plane: no sample has a third pivot
    cp = ref("coplanar")
    assert cp.status == R.STATUS_NO_MODEL and cp.usable_models == 0 and cp.detail["unusable_pivot"] == 107
    assert np.array_equal(cp.rotation, np.eye(3)) and cp.scale == 1.0 and not cp.inlier.any()
    # the same point many times: samples holding it twice are unusable and counted, the others find the camera
    du = ref("dup")
    assert du.status == R.STATUS_OK and du.detail["unusable_pivot"] > 10 and du.usable_models > 10
    assert du.usable_models + du.detail["unusable_pivot"] + du.detail["unusable_ratio"] == 107
    # the best hypothesis has exactly c = 26 inliers outside its sample
    ok, no = ref("mc_edge_ok"), ref("mc_edge_no")
    assert ok.status == R.STATUS_OK and ok.ransac_inliers == R.SAMPLE + 26 and ok.supported_models > 0
    assert no.status == R.STATUS_NO_MODEL and no.supported_models == 0 and no.usable_models == ok.usable_models
    assert ref("toofew11").status == R.STATUS_TOO_FEW and ref("toofew11").iterations == 0
    assert ref("toofew12").status == R.STATUS_OK and ref("toofew12").num_inliers == 12
    # the threshold matters: the same data and samples, other inlier sets
    assert ref("err1").best_iteration == ref("err6").best_iteration
    assert ref("err1").ransac_inliers < ref("err6").ransac_inliers and ref("err1").num_inliers < ref("err6").num_inliers
    # W != H: with the two mixed up the 1536-pixel axis is scored a third too coarse and the inlier set changes
    c = RC.BY_NAME["wide"]
    X, xy, _, _ = RC.build("wide")
    swapped = R.resect(X, xy, c.height, c.width, **c.options())
    assert swapped.status != R.STATUS_OK or not np.array_equal(swapped.inlier, ref("wide").inlier)
    # a camera of scale 1.25: estimated to a few 1e-4, or given; the axes do not depend on which
    est, fix = ref("scale_est"), ref("scale_fix")
    assert abs(est.scale - 1.25) < 2e-3 and est.scale != 1.25 and fix.scale == 1.25
    assert np.array_equal(est.rotation, fix.rotation) and not np.array_equal(est.offsets, fix.offsets)
    # inliers so close to one plane that the refit is refused: the winner's own matrix is kept
    ro = ref("refit_off")
    assert ro.status == R.STATUS_OK and ro.refit_used == 0 and ro.detail["refit_cond"] > 1e6
    assert all(ref(n).refit_used == 1 for n in OK_CASES if n != "refit_off")


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("n,frac", [(300, 0.3), (1000, 0.6)])
def test_prototype_scene_is_no_worse_than_the_perturbed_start(model, n, frac):
    """synth.make_ba_scene(model, 6, N, min_len = max_len = 6, noise_px = 0.3), points perturbed by 5e-4, view 4
    resected: the rotation is within 2 degrees (rot_perturb_deg, the start the pipeline otherwise uses) of the truth."""
    from orthosfm_amd import synth
    from orthosfm_amd.pipeline import _cam_rotation
    sc = synth.make_ba_scene(model, 6, n, min_len=6, max_len=6, noise_px=0.3)
    rng = np.random.default_rng(17)
    sel = np.flatnonzero(sc.obs_camera == RC.VIEW)
    xy = sc.obs_xy[sel].copy()
    X = sc.gt_points + 5e-4 * rng.normal(size=(n, 3))
    planted = np.zeros(n, dtype=bool)
    planted[rng.permutation(n)[:int(frac * n)]] = True
    ang = rng.uniform(0, 2 * np.pi, int(planted.sum()))
    xy[planted] += (rng.uniform(30.0, 300.0, ang.size) * np.array([np.cos(ang), np.sin(ang)])).T
    r = R.resect(X, xy.astype(np.float32).astype(np.float64), 2048, 2048, seed=3)
    err = R.rotation_error_deg(r.rotation, _cam_rotation(model, sc.gt_cams[RC.VIEW]))
    print(f"model {model} N {n} outliers {frac}: rotation {err:.4f} deg, inliers {r.num_inliers} of {int((~planted).sum())}")
    assert r.status == R.STATUS_OK and np.array_equal(r.inlier, ~planted)
    assert err < 2.0


def test_weak_group_decision_table():
    from orthosfm_amd import capi
    from orthosfm_amd.pipeline import weak_group_action as act
    RANSAC, FALLBACK, TOO_FEW, DEGENERATE = capi.TK_RANSAC, capi.TK_FALLBACK, capi.TK_TOO_FEW, capi.TK_DEGENERATE
    want = {
        # (status, first group, policy): action
        (RANSAC, True, "raise"): "tk", (RANSAC, False, "raise"): "tk",
        (RANSAC, True, "resect"): "tk", (RANSAC, False, "resect"): "tk",
        (FALLBACK, True, "raise"): "tk", (FALLBACK, False, "raise"): "tk",
        (FALLBACK, True, "resect"): "tk", (FALLBACK, False, "resect"): "resect",
        (DEGENERATE, True, "raise"): "tk", (DEGENERATE, False, "raise"): "tk",
        (DEGENERATE, True, "resect"): "tk", (DEGENERATE, False, "resect"): "resect",
        (TOO_FEW, True, "raise"): "raise", (TOO_FEW, False, "raise"): "raise",
        (TOO_FEW, True, "resect"): "raise", (TOO_FEW, False, "resect"): "resect",
    }
    for (status, first, policy), action in want.items():
        assert act(status, first, policy) == action, (status, first, policy)
    with pytest.raises(ValueError):
        act(RANSAC, False, "fallback")
    from orthosfm_amd import pipeline as P
    with pytest.raises(ValueError):
        P.run_pose_estimation(None, None, 0, weak_group="fallback")


def test_python_mirror_and_defaults():
    """capi.ResectOptions / ResectResult mirror the header's structs; the documented defaults."""
    import ctypes as C
    from orthosfm_amd import capi, resect
    assert C.sizeof(capi.ResectOptions) == 72 and C.sizeof(capi.ResectResult) == 48
    o = resect.options()
    assert (o.max_iterations, o.probability, o.inlier_ratio, o.min_consensus, o.max_error_px, o.min_pivot, o.min_axis_ratio,
            o.estimate_scale, o.scale, o.seed, o.device) == (0, 0.999, 0.5, 8, 3.0, R.DEFAULT_MIN_PIVOT, 0.5, 0, 1.0, 0, 0)
    assert capi.lib.osfm_resect_options_default(None) == capi.E_ARG
    # refused before any device work
    bad = resect.options(probability=1.5)
    r = capi.ResectResult()
    z = np.zeros(64)
    st = capi.lib.osfm_resect_view(z.ctypes.data, z.ctypes.data, 12, 64, 64, C.byref(bad), 0, z.ctypes.data, z.ctypes.data,
                                   z.ctypes.data, None, C.byref(r))
    assert st == capi.E_ARG
