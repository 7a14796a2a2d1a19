"""osfm_ba_covariance / osfm_scene_covariance on the device against cov_cases.py's extended-precision reference and
checker, in every case where the kernels change path: one tile, a camera block across a tile edge, ragged and empty
camera blocks over three tiles, seven tiles, homogeneous points with w != 1, invalid points, cameras only, an open
gauge.  Each case prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import cov_cases as cc

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def ba():
    from orthosfm_amd import ba
    return ba


def _case(name, ba):
    """(scene, reference), once per session."""
    if name not in _REF:
        if name == "degenerate":
            sc, _ = cc.degenerate()
        elif name == "after_solve":
            def solve(s):
                fp = ba.FlatProblem.from_scene(s)
                ba.solve(fp)
                s.cam_params[:], s.points[:] = fp.cam_params, fp.points
            sc = cc.after_solve(solve)
        else:
            sc = cc.CASES[name]()
        _REF[name] = (sc, cc.reference(sc))
    return _REF[name]


def _check_outputs(ref, cov):
    q = cc.check(ref, cov.cam_cov_full, cov.cam_cov, cov.point_cov, cov.point_valid, cov.cam_ldim)
    assert np.array_equal(cov.cam_cov, cc.blocks_of(ref, cov.cam_cov_full)), "cam_cov is not the diagonal blocks of cam_cov_full"
    assert np.array_equal(cov.cam_cov_full, cov.cam_cov_full.T), "cam_cov_full is not exactly symmetric"
    return q


@pytest.mark.parametrize("name", ["one_tile", "two_tiles", "mixed", "ring40", "after_solve", "degenerate"])
def test_case_against_reference(ba, name):
    sc, ref = _case(name, ba)
    fp = ba.FlatProblem.from_scene(sc)
    before = [a.copy() for a in (fp.cam_params, fp.cam_const, fp.points, fp.obs_xy, fp.obs_camera, fp.obs_point)]
    cov = ba.covariance(fp, full=True)
    after = (fp.cam_params, fp.cam_const, fp.points, fp.obs_xy, fp.obs_camera, fp.obs_point)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "the problem's arrays changed"
    q = _check_outputs(ref, cov)
    print(f"{name}: nc {cov.num_camera_unknowns} kappa {ref['kappa']:.4g} smallest pivot {cov.min_pivot_seen:.3g} "
          f"error / bound {({k: float(f'{v:.3g}') for k, v in q.items()})} dense_schur {cov.dense_schur}")
    assert max(q.values()) <= 1.0, q
    assert (cov.gauge_camera, cov.gauge_axis) == (ref["gauge_camera"], ref["gauge_axis"]) == cc.gauge_choice(sc)
    assert cov.num_camera_unknowns == ref["nc"] and cov.rank_deficient == 0
    assert cov.num_residuals == ref["num_residuals"] and cov.num_unknowns == ref["num_unknowns"]
    assert cov.num_valid_points == int(ref["valid"].sum())
    assert abs(cov.cost - ref["cost"]) <= 1e-9 * ref["cost"]
    assert abs(cov.variance_factor - ref["variance_factor"]) <= 1e-9 * ref["variance_factor"]
    # the smallest relative pivot agrees with the reference's to the conditioning
    assert abs(cov.min_pivot_seen - ref["pivots"].min()) <= 1e-6
    # a second call repeats to the bit
    again = ba.covariance(fp, full=True)
    for k in ("cam_cov", "cam_cov_full", "point_cov", "point_valid", "cam_ldim"):
        assert np.array_equal(getattr(cov, k), getattr(again, k)), k
    assert (cov.cost, cov.variance_factor, cov.min_pivot_seen) == (again.cost, again.variance_factor, again.min_pivot_seen)
    if name == "degenerate":
        _, bad = cc.degenerate()
        assert not cov.point_valid[bad].any() and np.all(cov.point_cov[~cov.point_valid] == 0)
        sig = cov.point_sigma()
        assert np.isnan(sig[~cov.point_valid]).all() and (sig[cov.point_valid] > 0).all()


def test_cameras_only(ba):
    sc = cc.two_tiles()
    ref = cc.reference(sc, optimize_points=False)
    cov = ba.covariance(ba.FlatProblem.from_scene(sc), full=True, optimize_points=0)
    assert cov.point_cov is None and cov.point_valid is None
    q = cc.check(ref, cov.cam_cov_full, cov.cam_cov, cam_ldim=cov.cam_ldim)
    print("cameras_only: error / bound", q, f"kappa {ref['kappa']:.4g}")
    assert max(q.values()) <= 1.0, q
    assert cov.num_unknowns == ref["nc"] and cov.num_residuals == ref["num_residuals"]
    # ... and with arrays given, the point outputs are not written
    fp = ba.FlatProblem.from_scene(sc)
    M = fp.points.shape[0]
    pc, pv = np.full((M, 3, 3), 7.0), np.full(M, 7, dtype=np.uint8)
    r = ba.capi.BaCovResult()
    r.point_cov, r.point_valid = pc.ctypes.data, pv.ctypes.data
    st, o = fp.struct(), ba.cov_options(optimize_points=0)
    ba.capi.check(ba.capi.lib.osfm_ba_covariance(C.byref(st), C.byref(o), C.byref(r)))
    assert np.all(pc == 7.0) and np.all(pv == 7)


@pytest.mark.parametrize("name", ["one_tile", "ring40"])
@pytest.mark.parametrize("how", ["depth_gauge_0", "no_constant_camera"])
def test_open_gauge_is_refused(ba, name, how):
    sc = cc.CASES[name]()
    kw = {"depth_gauge": 0}
    if how == "no_constant_camera":
        sc, kw = cc.without_constant_camera(sc), {}
    fp = ba.FlatProblem.from_scene(sc)
    with pytest.raises(ba.capi.OsfmError) as e:
        ba.covariance(fp, full=True, fill=7, **kw)
    err = e.value
    print(f"{name} {how}: smallest relative pivot {err.min_pivot_seen:.3g}")
    assert err.status == ba.capi.E_NUMERIC and err.rank_deficient == 1
    assert err.min_pivot_seen < cc.MIN_PIVOT_RATIO
    assert (err.gauge_camera, err.gauge_axis) == (-1, -1)
    for k, a in err.arrays.items():
        assert np.all(a == 7), f"{k} was written"


def test_null_arguments(ba):
    sc, ref = _case("two_tiles", ba)
    fp = ba.FlatProblem.from_scene(sc)
    whole = ba.covariance(fp, full=True)
    # opts NULL: the defaults
    arrays = {"cam_cov": np.zeros((8, 6, 6)), "cam_cov_full": np.zeros((ref["nc"], ref["nc"]))}
    r = ba.capi.BaCovResult()
    r.cam_cov, r.cam_cov_full, r.nc = arrays["cam_cov"].ctypes.data, arrays["cam_cov_full"].ctypes.data, ref["nc"]
    st = fp.struct()
    ba.capi.check(ba.capi.lib.osfm_ba_covariance(C.byref(st), None, C.byref(r)))
    assert np.array_equal(arrays["cam_cov_full"], whole.cam_cov_full) and np.array_equal(arrays["cam_cov"], whole.cam_cov)
    # each output pointer NULL in turn: the others are what the whole call gave
    for skip in ba.capi.BaCovResult.ARRAYS:
        part = ba.covariance(fp, full=True, skip=(skip,))
        assert getattr(part, skip) is None
        for k in ba.capi.BaCovResult.ARRAYS:
            if k != skip:
                assert np.array_equal(getattr(part, k), getattr(whole, k)), (skip, k)
    # a wrong nc
    r = ba.capi.BaCovResult()
    full = np.zeros((ref["nc"] + 1, ref["nc"] + 1))
    r.cam_cov_full, r.nc = full.ctypes.data, ref["nc"] + 1
    assert ba.capi.lib.osfm_ba_covariance(C.byref(st), None, C.byref(r)) == ba.capi.E_ARG
    assert r.num_camera_unknowns == ref["nc"]
    assert ba.capi.lib.osfm_ba_covariance(C.byref(st), None, None) == ba.capi.E_ARG
    # a repeated (camera, point) is refused as osfm_ba_solve refuses it
    bad = ba.FlatProblem.from_scene(sc)
    bad.obs_camera[1] = bad.obs_camera[0]
    with pytest.raises(ba.capi.OsfmError) as e:
        ba.covariance(bad)
    assert e.value.status == ba.capi.E_ARG


def test_scene_entry_matches_per_call_entry(ba):
    from orthosfm_amd.scene import Scene
    sc = cc.ring40()
    sc.obs_xy = sc.obs_xy.astype(np.float32).astype(np.float64)          # what a scene's float features can hold
    Cn, M = sc.cam_params.shape[0], sc.points.shape[0]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(sc.obs_point, minlength=M))]).astype(np.int64)
    scene = Scene(sc.model, sc.img_w, sc.img_h, offsets, sc.obs_camera, sc.obs_xy.astype(np.float32))
    scene.align_views(np.arange(Cn), sc.cam_params, sc.cam_const)
    scene.triangulate()
    # dead features and a dead track by hand, then one reprojection filter
    af, at = np.ones(sc.obs_point.shape[0], dtype=np.uint8), np.ones(M, dtype=np.uint8)
    af[offsets[3]] = af[offsets[11] + 1] = 0
    af[offsets[20]:offsets[21] - 1] = 0          # one live feature left: a point that is invalid
    at[30] = 0
    scene.set_flags(at, af)
    scene.filter_reprojection(50.0)
    alive_t, alive_f, has_point, points = scene.download()
    assert not alive_f.all() and not alive_t.all()
    tsel = np.flatnonzero(alive_t & has_point)
    slot = np.full(M, -1)
    slot[tsel] = np.arange(tsel.size)
    fsel = alive_f & alive_t[sc.obs_point] & (slot[sc.obs_point] >= 0)
    fp = ba.FlatProblem(sc.model, sc.cam_params, sc.cam_const, sc.img_w, sc.img_h, points[tsel], sc.obs_xy[fsel],
                        sc.obs_camera[fsel], slot[sc.obs_point[fsel]])
    one = ba.covariance(fp, full=True)
    two = scene.covariance(full=True)
    state = scene.download()
    scene.close()
    for a, b in zip((alive_t, alive_f, has_point, points), state):
        assert np.array_equal(a, b), "the scene changed"
    for k in ("cam_cov", "cam_cov_full", "cam_ldim"):
        assert np.array_equal(getattr(one, k), getattr(two, k)), k
    assert np.array_equal(one.point_cov, two.point_cov[tsel]) and np.array_equal(one.point_valid, two.point_valid[tsel])
    rest = np.setdiff1d(np.arange(M), tsel)
    assert not two.point_valid[rest].any() and np.all(two.point_cov[rest] == 0)
    assert not one.point_valid[slot[20]]
    for k in ("cost", "variance_factor", "min_pivot_seen", "num_residuals", "num_unknowns", "gauge_camera", "gauge_axis"):
        assert getattr(one, k) == getattr(two, k), k


def test_reconstruct_with_uncertainty():
    from orthosfm_amd import pipeline, synth
    iset = synth.make_image_set(6, 2500, config_id=31)
    plain = pipeline.reconstruct(iset, solver=0)
    unc = pipeline.reconstruct(iset, solver=0, uncertainty=True)
    assert plain.point_sigma is None and plain.cam_cov is None
    assert np.array_equal(plain.cam_params, unc.cam_params) and plain.aligned_views == unc.aligned_views
    assert np.array_equal(plain.tracks.point, unc.tracks.point) and np.array_equal(plain.tracks.has_point, unc.tracks.has_point)
    key = lambda c: (c.kind, c.cameras, c.points, c.observations, c.iterations)
    assert [key(c) for c in plain.ba_calls] == [key(c) for c in unc.ba_calls]
    v = unc.point_valid
    assert v.shape == unc.point_sigma.shape == (unc.tracks.point.shape[0],) and v.sum() > 100
    assert np.all(np.isfinite(unc.point_sigma[v]) & (unc.point_sigma[v] > 0)) and np.isnan(unc.point_sigma[~v]).all()
    assert unc.cam_cov.shape == (len(unc.aligned_views), 6, 6) and unc.variance_factor > 0
    assert not v[~(unc.tracks.alive_t & unc.tracks.has_point)].any()
    # the host path (no scene) reports the same
    host = pipeline.reconstruct(iset, solver=0, uncertainty=True, use_scene=False)
    assert np.array_equal(host.point_valid, unc.point_valid) and np.array_equal(host.point_cov, unc.point_cov)
    assert np.array_equal(host.cam_cov, unc.cam_cov)
