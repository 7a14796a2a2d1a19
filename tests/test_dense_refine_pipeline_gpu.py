"""pipeline.densify(refine=True, meshes=True) on the four rendered views of dense_cases.pipeline_scene(): the cloud is
nearer to the exact depth than the recorded figure of the unrefined path, the point set's normals are nearer to the
planes' normals than those of the unrefined path, and the device, fed the restatement's sweeps, gives the restated
refined cloud.  With refine=False nothing changes."""
from types import SimpleNamespace

import numpy as np
import pytest

import dense_cases as dc
import dense_refine_cases as rc
import dense_refine_restatement as drr
import dense_restatement as dr
from orthosfm_amd import pipeline
from orthosfm_amd.dense import DenseStereo

pytestmark = pytest.mark.gpu

_results = {}


def densified(refine):
    if refine not in _results:
        sc = dc.pipeline_scene()
        _results[refine] = pipeline.densify(sc["images"], sc["model"], sc["cam_params"], sc["points"], sc["visibility"], keep_maps=True,
                                            meshes=True, refine=refine, **dc.PIPELINE_OPTIONS)
    return _results[refine]


def _normal_angles(sc, pset):
    """The angle of every normal of a point set to the normal of the plane its pixel shows."""
    out = np.zeros(pset.points.shape[0])
    for v in range(4):
        h, w = sc["images"][v].shape[:2]
        view = SimpleNamespace(P=sc["P"], planes=sc["planes"], exact=lambda u: dc.trace(dr.Geometry(sc["P"][u]), w, h, sc["planes"])[:2])
        truth = rc.plane_normals(view, v)
        sel = pset.view == v
        px = pset.pixel[sel]
        out[sel] = rc.angle_deg(pset.normals[sel], truth[px[:, 1], px[:, 0]])
    return out


def test_densify_refined_is_nearer_in_depth_and_in_normals():
    sc, res, plain = dc.pipeline_scene(), densified(True), densified(False)
    assert len(res.refined) == 4 and all((r.status == drr.REFINED).sum() > 5000 for r in res.refined)
    assert res.refine_ms > 0.0 and plain.refined is None and plain.refine_ms == 0.0
    dzs = {v: p.dz for v, p in enumerate(res.plans)}
    median, within, points = dc.cloud_accuracy(sc, res.points, res.view, res.pixel, dzs)
    before = dc.cloud_accuracy(sc, plain.points, plain.view, plain.pixel, dzs)
    print(f"densify refined: median {median:.4f} steps (unrefined {before[0]:.4f}; restated {rc.MEASURED_CPU_PIPELINE['median_steps']:.4f}), "
          f"within one step {within:.4f}, points {points}")
    assert median < dc.MEASURED_CPU_PIPELINE["median_steps"]
    # every emitted point lies at its view's refined depth
    for v in range(4):
        sel = res.view == v
        px = res.pixel[sel]
        X = dr.Geometry(sc["P"][v]).point(px[:, 0].astype(np.float64), px[:, 1].astype(np.float64), res.refined[v].depth[px[:, 1], px[:, 0]])
        assert res.points[sel].tobytes() == np.stack(X, axis=1).tobytes()
    # the meshes are those of the refined maps with the refined normals where there are any; the point set follows
    a, b = _normal_angles(sc, res.pset), _normal_angles(sc, plain.pset)
    print(f"point set normals: median angle {np.median(a):.3f} degrees refined, {np.median(b):.3f} unrefined")
    assert np.median(a) < np.median(b)
    for v, m in enumerate(res.meshes):
        ref = res.refined[v].status[m.pixel[:, 1], m.pixel[:, 0]] == drr.REFINED
        assert ref.sum() > 1000
        assert m.normals[ref].tobytes() == res.refined[v].normal[m.pixel[ref, 1], m.pixel[ref, 0]].tobytes()


def test_the_device_gives_the_restated_refined_cloud():
    sc = dc.pipeline_scene()
    plans, maps, refined = rc.pipeline_maps()
    _, want = rc.restated_pipeline()
    o = {key: dc.PIPELINE_OPTIONS[key] for key in ("radius", "min_sources", "min_score") if key in dc.PIPELINE_OPTIONS}
    worst = 0.0
    with DenseStereo(0, 4) as d:
        for v in range(4):
            d.set_image(v, sc["images"][v])
        d.set_cameras(sc["P"])
        for v, p in enumerate(plans):
            d.set_map(v, maps[v]["depth"], maps[v]["status"], p.dz, score=maps[v]["score"])
        for v, p in enumerate(plans):
            got = d.refine(v, p.sources, **o)
            clear = ~rc.ambiguous(refined[v])
            assert np.array_equal(got.status[clear], refined[v]["status"][clear])
            both = (got.status == drr.REFINED) & (refined[v]["status"] == drr.REFINED) & clear
            worst = max(worst, float(np.abs(got.depth - refined[v]["depth"])[both].max()) / p.dz)
        cloud = d.fuse(**dc.PIPELINE_OPTIONS)
    dzs = {v: p.dz for v, p in enumerate(plans)}
    got_acc = dc.cloud_accuracy(sc, cloud.points, cloud.view, cloud.pixel, dzs)
    want_acc = dc.cloud_accuracy(sc, want["points"], want["view"], want["pixel"], dzs)
    print(f"device on the restated sweeps: median {got_acc[0]:.6f} steps, restated {want_acc[0]:.6f}; max d depth {worst:.3e} steps")
    assert worst <= rc.BOUNDS["depth_steps"]
    assert abs(got_acc[0] - want_acc[0]) <= rc.BOUNDS["depth_steps"] and round(want_acc[0], 4) == rc.MEASURED_CPU_PIPELINE["median_steps"]
    ambiguous = any(rc.ambiguous(r).any() for r in refined.values())
    assert ambiguous or (np.array_equal(cloud.pixel, want["pixel"]) and np.array_equal(cloud.view, want["view"]))


def test_without_refine_nothing_changes():
    sc, plain = dc.pipeline_scene(), densified(False)
    other = pipeline.densify(sc["images"], sc["model"], sc["cam_params"], sc["points"], sc["visibility"], keep_maps=True, meshes=True,
                             **dc.PIPELINE_OPTIONS)
    for field in ("points", "rgb", "view", "pixel"):
        assert getattr(plain, field).tobytes() == getattr(other, field).tobytes(), field
    assert plain.counters == other.counters
    for a, b in zip(plain.maps, other.maps):
        assert a.depth.tobytes() == b.depth.tobytes() and a.status.tobytes() == b.status.tobytes() and a.score.tobytes() == b.score.tobytes()
    for a, b in zip(plain.meshes, other.meshes):
        for field in ("points", "normals", "confidence", "scale", "pixel", "vclass", "triangles"):
            assert getattr(a, field).tobytes() == getattr(b, field).tobytes(), field
    for field in ("points", "normals", "confidence", "scale", "pixel", "rgb", "view"):
        assert getattr(plain.pset, field).tobytes() == getattr(other.pset, field).tobytes(), field
