"""The cases of tests/dense_refine_cases.py under the restatement alone: every case reaches what it lists and stays
clear of the ambiguity band, the refinement beats the sweep against the exact depth and the meshes' normals against the
exact normals, the recorded figures hold, the bounds of the GPU test see every planted error, and a pixel's result
does not depend on the other pixels."""
import numpy as np
import pytest

import dense_cases as dc
import dense_refine_cases as rc
import dense_refine_restatement as drr
import dense_restatement as dr
import refine_restatement as rr


@pytest.mark.parametrize("name", rc.NAMES)
def test_paths_and_ambiguity(name):
    c = rc.scene(name)
    res = rc.restated(name)
    counts = np.zeros(8, np.int64)
    for k, r in res.items():
        counts += np.bincount(r["status"].ravel(), minlength=8)
        tested = rc.tested(r)
        assert np.array_equal(r["status"] == drr.NOT_OK, rc.swept(name)[k]["status"] != dr.OK)
        share = rc.ambiguous(r).sum() / max(int(tested.sum()), 1)
        print(f"{name} sweep {k}: {dict(zip(drr.STATUS_NAMES, np.bincount(r['status'].ravel(), minlength=8).tolist()))}, ambiguous {share:.5f}")
        assert share <= rc.AMBIGUOUS_SHARE, (name, k, share)
        ref = r["status"] == drr.REFINED
        assert np.isnan(r["gradient"][~ref]).all() and np.isnan(r["normal"][~ref]).all()
        assert np.isfinite(r["gradient"][ref]).all() and np.allclose(np.linalg.norm(r["normal"][ref], axis=-1), 1.0, atol=1e-12)
        assert r["depth"][~ref].tobytes() == np.asarray(rc.swept(name)[k]["depth"])[~ref].tobytes()
        # towards the camera, the sign of mesh_restatement.vertex_normals
        assert (r["normal"][ref] @ np.array(dr.Geometry(c.P[c.sweeps[k].ref]).d) < 0.0).all()
    for status in rc.CASES[name]["reach"]:
        assert counts[status] > 0, (name, drr.STATUS_NAMES[status])
    if name == "step":
        assert tuple(counts.tolist()) == rc.STEP_COUNTS
        assert counts[[drr.NOT_CONVERGED, drr.REJECT_SHIFT, drr.REJECT_SLOPE, drr.REJECT_SCORE]].sum() > 0
    if name == "steep":
        assert all((m["status"] == dr.OK).sum() > 1000 for m in rc.swept(name))      # the sweep still leaves OK pixels there


def test_a_window_that_touches_the_last_row_and_column_counts():
    c = rc.scene("border")
    tx, ty = c.paths["touch"]
    sw, m, r = c.sweeps[0], rc.swept("border")[0], rc.restated("border")[0]
    assert m["status"][ty, tx] == dr.OK and r["status"][ty, tx] == drr.REFINED
    R = rc.refine_options("border", 0)["radius"]
    side = 2 * R + 1
    k = np.arange(side * side)
    ux, uy = (k % side - R).astype(np.float64)[:, None], (k // side - R).astype(np.float64)[:, None]
    pair = dr.Geometry(c.P[sw.ref]).pair(dr.Geometry(c.P[3]))
    one = lambda v: np.array([float(v)])
    T = np.zeros((side * side, 1))
    # at the start and at the refined depth and tilt: view 3 has e = 0 and G = I, so its samples are exact integers
    for z, zx, zy in ((m["depth"][ty, tx], 0.0, 0.0), (r["depth"][ty, tx], *r["gradient"][ty, tx])):
        _, inside, slack = drr.source_sums(dr.grey(c.images[3]), pair, one(tx), one(ty), one(z), one(zx), one(zy), T, ux, uy)
        assert inside[0] and slack[0] == 1.0        # the touching samples are exact and no close call: the nearest other is a pixel in
    _, inside, _ = drr.source_sums(dr.grey(c.images[3]), pair, one(tx + 1), one(ty), one(m["depth"][ty, tx]), one(0.0), one(0.0), T, ux, uy)
    assert not inside[0]


@pytest.mark.parametrize("name", rc.ACCURACY)
def test_refinement_beats_the_sweep_and_the_mesh_normals(name):
    got = rc.accuracy(name)
    print(name, got)
    assert got == rc.MEASURED_CPU[name]
    assert got["median_steps_refined"] < got["median_steps_sweep"]
    assert got["normal_deg_refined"] < got["normal_deg_mesh"]


def test_pipeline_figures():
    plans, fusion = rc.restated_pipeline()
    sc = dc.pipeline_scene()
    median, within, points = dc.cloud_accuracy(sc, fusion["points"], fusion["view"], fusion["pixel"], {v: p.dz for v, p in enumerate(plans)})
    print(f"refined pipeline: median {median:.4f}, within one step {within:.4f}, points {points}")
    want = rc.MEASURED_CPU_PIPELINE
    assert (round(median, 4), round(within, 4), points) == (want["median_steps"], want["within_one_step"], want["points"])
    assert median < dc.MEASURED_CPU_PIPELINE["median_steps"]


def test_pivot_threshold():
    got, want = rc.pivot_figures(), rc.PIVOT
    print(got)
    for key in ("textured_min", "edge_only_min", "edge_only_median"):
        assert abs(got[key] - want[key]) < 1e-6, key
    assert got["edge_only_pixels"] == want["edge_only_pixels"]
    for label in ("below", "above"):
        assert got[label]["pixels"] == want[label]["pixels"]
        for key in ("p90_sweep", "p90_refined"):
            assert abs(got[label][key] - want[label][key]) < 1e-4, (label, key)
    assert got["below"]["p90_refined"] > got["below"]["p90_sweep"] and got["above"]["p90_refined"] < got["above"]["p90_sweep"]
    assert want["threshold"] < got["textured_min"] and want["threshold"] == drr.DEFAULTS["min_pivot"]


def _seen(got, want, dz, R):
    """Whether the GPU test's comparison of `got` with `want` would fail: a status outside the ambiguous pixels, or a
    figure beyond its bound."""
    clear = ~rc.ambiguous(want)
    if not np.array_equal(got["status"][clear], want["status"][clear]):
        return True
    both = (got["status"] == drr.REFINED) & (want["status"] == drr.REFINED) & clear
    worst = {"depth_steps": np.abs(got["depth"] - want["depth"])[both].max() / dz,
             "gradient_steps": np.abs(got["gradient"] - want["gradient"])[both].max() * R / dz,
             "normal": np.abs(got["normal"] - want["normal"])[both].max(),
             "score": np.abs(got["score"].astype(np.float64) - want["score"])[both].max()}
    return any(worst[key] > rc.BOUNDS[key] for key in worst)


@pytest.mark.parametrize("plant", [p for p in drr.PLANTS if p])
def test_bounds_see_the_planted_errors(plant):
    c = rc.scene("slanted")
    sw, m, want = c.sweeps[0], rc.swept("slanted")[0], rc.restated("slanted")[0]
    o = rc.refine_options("slanted", 0)
    got = drr.refine(c.images, c.P, sw.ref, sw.sources, m["depth"], m["status"], sw.dz, score=m["score"], plant=plant, **o)
    assert _seen(got, want, sw.dz, o["radius"]), plant
    if plant == "flat_normal":                     # nothing but the normal is wrong
        assert np.array_equal(got["status"], want["status"]) and got["depth"].tobytes() == want["depth"].tobytes()
    assert not _seen(want, want, sw.dz, o["radius"])


def test_a_pixel_does_not_depend_on_the_others():
    c = rc.scene("step")
    sw, m, want = c.sweeps[0], rc.swept("step")[0], rc.restated("step")[0]
    rect = (23, 17, 58, 49)
    got = drr.refine(c.images, c.P, sw.ref, sw.sources, m["depth"], m["status"], sw.dz, score=m["score"], rect=rect, **rc.refine_options("step", 0))
    window = (slice(rect[1], rect[3]), slice(rect[0], rect[2]))
    assert (got["status"][window] == drr.REFINED).sum() > 500
    for key in ("depth", "gradient", "normal", "score", "status", "iterations", "margin"):
        assert got[key][window].tobytes() == want[key][window].tobytes(), key
    outside = np.ones(m["status"].shape, bool)
    outside[window] = False
    assert (got["status"][outside] == drr.NOT_OK).all()


def test_the_helpers_are_the_refiners():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(200, 3, 3))
    H = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(3)
    H[:20, 2] = H[:20, 1] * (1.0 + 1e-3 * rng.normal(size=(20, 1)))        # some that are ill conditioned
    H[:20, :, 2] = H[:20, 2]
    H[20:24, 1, 1] = -1.0                                                     # and some that are no normal matrix at all
    rhs = rng.normal(size=(200, 3))
    delta, ok, pivot = drr.solve3([[H[:, i, j] for j in range(3)] for i in range(3)], [rhs[:, i] for i in range(3)], 0.035)
    assert 0 < ok.sum() < 200
    for n in range(200):
        want, want_pivot = rr.solve_step(H[n], rhs[n], 0.035)
        assert (want is not None) == bool(ok[n]), n
        if want is not None:
            assert np.array([delta[i][n] for i in range(3)]).tobytes() == want.tobytes() and pivot[n] == want_pivot, n
    # the 16-lane sum: the fold of refine_restatement.wave_sum on 16 lanes
    v = rng.normal(size=(225, 7))
    lanes = [sum((v[k] for k in range(l + 16, 225, 16)), v[l].copy()) for l in range(16)]
    for m in (8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i + m] for i in range(m)]
    assert drr.lane_sum(v).tobytes() == lanes[0].tobytes()
