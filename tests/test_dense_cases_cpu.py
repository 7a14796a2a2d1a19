"""The cases of tests/dense_cases.py under the restatement alone (no device): the cameras, the statuses every case
names, the accuracy against the exact depth, what the fusion drops on the occluded step, and the share of pixels a
rounding may decide."""
import numpy as np
import pytest

import dense_cases as dc
import dense_restatement as dr
from orthosfm_amd import dense, synth


@pytest.mark.parametrize("model", [synth.MODEL_QUATERNION, synth.MODEL_EULER])
def test_affine_cameras_reproduce_the_projection(model):
    sc = synth.make_ba_scene(model, 6, 40, config_id=61, width=640, height=480)
    cams = sc.gt_cams.copy()
    off = 3 if model == synth.MODEL_EULER else 4
    cams[:, off:off + 3] += np.array([0.03, -0.02, 0.1]) * np.arange(1, 7)[:, None]      # offsets and a scale that are not 0 and 1
    w, h = np.array([640, 600, 512, 640, 333, 640]), np.array([480, 400, 512, 480, 257, 480])
    P = dense.affine_cameras(model, cams, w, h)
    X = sc.gt_points
    for v in range(6):
        want = synth._project(model, cams[v], X, w[v], h[v])
        got = X @ P[v, :, :3].T + P[v, :, 3]
        assert np.abs(got - want).max() <= 1e-9
    # the restatement's geometry on them: B is a right inverse of A and d is the unit normal of its rows
    g = dr.Geometry(P[1])
    A, B, d = np.array(g.A), np.array(g.B), np.array(g.d)
    assert np.abs(A @ B - np.eye(2)).max() < 1e-12 and np.abs(A @ d).max() < 1e-9 and abs(d @ d - 1.0) < 1e-12
    assert not dr.Geometry(np.array([[1.0, 2.0, 3.0, 0.0], [2.0, 4.0, 6.0, 1.0]])).ok


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_reaches_what_it_names(name):
    c = dc.case(name)
    for sw, m in zip(c.sweeps, dc.restated(name)):
        for st in sw.expect:
            assert (m["status"] == st).any(), (sw.ref, dr.STATUS_NAMES[st])
        ok = m["status"] == dr.OK
        assert np.isfinite(m["depth"][ok]).all() and np.isnan(m["depth"][~ok]).all() and (m["score"][~ok] == 0).all()
        assert (m["score"][ok] >= sweep_min_score(c, sw)).all()
    if name == "empty":
        assert dc.restated(name)[0]["status"].shape == (1, 1)
    if name == "many_depths":
        assert c.sweeps[0].num_depths == dc.MAX_DEPTHS


def sweep_min_score(c, sw):
    return np.float32(dc.sweep_options(c, sw).get("min_score", dr.DEFAULTS["min_score"])) - np.float32(1e-6)


def test_border_window_touches_the_last_row_and_column():
    """View 3 shows the reference 20 and 15 pixels over, in exact integers: the window of `touch` ends on its last
    column and row and counts, the windows one pixel further do not -- an integer decision, not a close one."""
    c = dc.case("border")
    m = dc.restated("border")[1]                     # sources: view 3 and a view that sees everything, both required
    x, y = c.paths["touch"]
    assert m["status"][y, x] != dr.NO_SOURCES
    assert m["status"][y, x + 1] == dr.NO_SOURCES and m["status"][y + 1, x] == dr.NO_SOURCES
    assert not dc.ambiguous(m)[y, x + 1] and not dc.ambiguous(m)[y + 1, x]
    # in the first sweep the number of valid sources changes from depth to depth
    first = dc.restated("border")[0]
    assert (first["status"] == dr.RANGE_EDGE).any() and (first["status"] == dr.NO_SOURCES).any()


def _accuracy(name):
    c = dc.case(name)
    errs = []
    for sw, m in zip(c.sweeps, dc.restated(name)):
        ok = m["status"] == dr.OK
        errs.append(np.abs(m["depth"][ok] - c.exact(sw.ref)[0][ok]) / sw.dz)
    e = np.concatenate(errs)
    return float(np.median(e)), float((e <= 1.0).mean())


@pytest.mark.parametrize("name", ["slanted", "step"])
def test_depth_against_the_exact_depth(name):
    median, within = _accuracy(name)
    print(f"{name}: median |z - z_exact| {median:.4f} step, {within:.4f} within one step")
    rec = dc.MEASURED_CPU[name]
    assert abs(median - rec["median_steps"]) <= 5e-4 and abs(within - rec["within_one_step"]) <= 5e-4
    assert median < 0.25 and within > 0.9


def test_step_fusion_drops_the_occluded_and_the_wrong():
    c = dc.case("step")
    f = dc.restated_fusion("step")
    geo = [dr.Geometry(p) for p in c.P]
    exact = [c.exact(v) for v in range(len(c.images))]
    assert f["points"].shape[0] > 3000
    # (1) a pixel whose surface point every other view sees something else in front of is not emitted
    hidden_total = 0
    for r in range(len(c.images)):
        h, w = c.images[r].shape[:2]
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        X = geo[r].point(xs, ys, exact[r][0])
        hidden = np.ones((h, w), bool)
        for s in range(len(c.images)):
            if s == r:
                continue
            q = geo[s].project(X)
            ix, iy = np.floor(q[0] + 0.5).astype(np.int64), np.floor(q[1] + 0.5).astype(np.int64)
            hs, ws = c.images[s].shape[:2]
            ins = (ix >= 0) & (ix < ws) & (iy >= 0) & (iy < hs)
            front = np.zeros((h, w), bool)
            front[ins] = exact[s][0][iy[ins], ix[ins]] < geo[s].depth(X)[ins] - 1.0      # a world unit in front
            hidden &= ~ins | front
        hidden_total += int(hidden.sum())
        assert not (hidden & (f["final"][r] == dr.OK)).any()
    assert hidden_total > 100
    # (2) no emitted point is farther than one step from the plane its pixel shows
    for v in range(len(c.images)):
        sel = f["view"] == v
        px = f["pixel"][sel]
        z = geo[v].depth(tuple(f["points"][sel].T))
        dz = [sw.dz for sw in c.sweeps if sw.ref == v][0]
        assert (np.abs(z - exact[v][0][px[:, 1], px[:, 0]]) <= dz).all()
    assert set(np.unique(exact[0][1][f["pixel"][f["view"] == 0][:, 1], f["pixel"][f["view"] == 0][:, 0]])) == {0, 1}
    # the order of the cloud: view, row, column
    key = (f["view"].astype(np.int64) << 40) + (f["pixel"][:, 1].astype(np.int64) << 20) + f["pixel"][:, 0]
    assert (np.diff(key) > 0).all()


@pytest.mark.parametrize("name", dc.NAMES)
def test_ambiguous_share_stays_under_the_cap(name):
    tested = sum(int(dc.tested(m).sum()) for m in dc.restated(name))
    amb = sum(int(dc.ambiguous(m).sum()) for m in dc.restated(name))
    print(f"{name}: {amb} of {tested} tested pixels within {dc.AMBIGUITY_BAND} of a decision")
    assert amb <= dc.AMBIGUOUS_SHARE * tested


def test_bounds_see_uncentred_float32_sums():
    """The ceilings are conditions: float32 sums of the raw grey values (not minus 128, not centred) are the error
    they exist to catch, and it breaks them."""
    c = dc.case("one_source")
    sw, want = c.sweeps[0], dc.restated("one_source")[0]
    got = dr.sweep(c.images, c.P, sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, uncentred_float32=True, **dc.sweep_options(c, sw))
    both = (got["status"] == dr.OK) & (want["status"] == dr.OK)
    assert np.abs(got["score"][both].astype(np.float64) - want["score"][both]).max() > dc.CEILINGS["score"]
    assert (np.abs(got["depth"][both] - want["depth"][both]) / sw.dz).max() > dc.CEILINGS["depth_steps"]
    assert dc.BOUNDS["score"] <= dc.CEILINGS["score"] and dc.BOUNDS["depth_steps"] <= dc.CEILINGS["depth_steps"]


def test_pipeline_scene_under_the_restatement():
    """What tests/test_dense_pipeline_gpu.py holds pipeline.densify to."""
    sc = dc.pipeline_scene()
    for v in range(4):
        want = synth.project_quat(sc["points"], sc["cam_params"][v, :4], *sc["cam_params"][v, 4:], 160, 128)
        assert np.abs(sc["points"] @ sc["P"][v, :, :3].T + sc["P"][v, :, 3] - want).max() < 1e-9
    plans, f = dc.restated_pipeline()
    assert all(p is not None and len(p.sources) == 3 for p in plans)
    median, within, per_plane = dc.cloud_accuracy(sc, f["points"], f["view"], f["pixel"], {v: p.dz for v, p in enumerate(plans)})
    print(f"pipeline scene: {f['points'].shape[0]} points, {per_plane} per plane, median {median:.4f} step, {within:.4f} within one step")
    rec = dc.MEASURED_CPU_PIPELINE
    assert abs(median - rec["median_steps"]) <= 5e-4 and abs(within - rec["within_one_step"]) <= 5e-4 and per_plane == rec["points"]
    assert min(per_plane) > 1000 and median < 0.25 and within > 0.99


def test_plan_view_is_the_stated_rule():
    c = dc.case("eight_sources")
    pts = np.stack(dc.trace(dr.Geometry(c.P[0]), 64, 56, c.planes)[2], axis=-1).reshape(-1, 3)[::97]
    plan = dense.plan_view(c.P, 0, pts, range(9), max_depths=dc.MAX_DEPTHS)
    d = dense.viewing_axes(c.P)
    ang = np.degrees(np.arccos(np.clip(d @ d[0], -1, 1)))
    order = sorted((abs(ang[s] - 15.0), s) for s in range(1, 9) if 5.0 <= ang[s] <= 40.0)
    assert plan.sources == [s for _, s in order[:4]] and len(plan.sources) == 4
    z = pts @ d[0]
    e = max(np.linalg.norm(c.P[s, :, :3] @ d[0]) for s in plan.sources)
    assert plan.dz == pytest.approx(0.5 / e)
    pad = max(0.1 * (z.max() - z.min()), 2.0 * plan.dz)
    assert plan.z_min == pytest.approx(z.min() - pad)
    assert plan.z_min + (plan.num_depths - 1) * plan.dz >= z.max() + pad - 1e-9
    wide = dense.plan_view(c.P, 0, pts * np.array([1.0, 1.0, 40.0]), range(9), max_depths=dc.MAX_DEPTHS)       # 10 % is the larger
    zw = (pts * np.array([1.0, 1.0, 40.0])) @ d[0]
    assert wide.z_min == pytest.approx(zw.min() - 0.1 * (zw.max() - zw.min()))
    flat = dense.plan_view(c.P, 0, pts[:1], range(9), max_depths=dc.MAX_DEPTHS)                                 # one point: two steps each side
    assert flat.num_depths in (5, 6) and flat.z_min == pytest.approx(z[0] - 2.0 * flat.dz)
    tight = dense.plan_view(c.P, 0, pts, range(9), max_depths=8)
    assert tight.num_depths == 8 and tight.dz > plan.dz
    assert dense.plan_view(c.P, 0, pts, [0], max_depths=8) is None
