"""pipeline.densify(meshes=True) on the four rendered views of dense_cases.pipeline_scene(): every view's mesh is the
restatement's mesh of the device's own map and fused statuses, the point set is their vertices with a confidence above
0, and save_project writes files that parse.  With meshes=False nothing changes: the same cloud, the same files."""
import os

import numpy as np
import pytest

import dense_cases as dc
import dense_restatement as dr
import mesh_cases as mc
import mesh_restatement as mr
from orthosfm_amd import dense, pipeline, synth

pytestmark = pytest.mark.gpu

_results = {}


def densified(meshes):
    if meshes not in _results:
        sc = dc.pipeline_scene()
        _results[meshes] = pipeline.densify(sc["images"], sc["model"], sc["cam_params"], sc["points"], sc["visibility"], keep_maps=True,
                                            meshes=meshes, **dc.PIPELINE_OPTIONS)
    return _results[meshes]


def _project(tmp_path, name, cloud):
    tt = pipeline.TrackTable([0, 2, 4], [0, 1, 0, 2], [0, 0, 1, 0], np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]), 3)
    tt.point[:, :3], tt.point[:, 3] = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], 1.0
    tt.has_point[:] = True
    res = pipeline.Result(np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], (3, 1)), [], tt, [], pipeline.Timings(), [])
    folder = tmp_path / name
    pipeline.save_project(res, synth.MODEL_QUATERNION, str(folder), dense_cloud=cloud)
    return folder


def test_densify_with_meshes(tmp_path):
    sc, res = dc.pipeline_scene(), densified(True)
    assert len(res.meshes) == 4 and all(m is not None for m in res.meshes)
    # the fused statuses of the device's maps: the fusion's decisions are exact given the maps
    maps = {v: dict(depth=res.maps[v].depth, status=res.maps[v].status) for v in range(4)}
    dzs = {v: res.plans[v].dz for v in range(4)}
    final = dr.fuse(sc["P"], maps, dzs, **dc.PIPELINE_OPTIONS)["final"]
    worst = [0.0, 0.0]
    for v, got in enumerate(res.meshes):
        want = mr.mesh(sc["P"][v], maps[v]["depth"], maps[v]["status"], dzs[v], final=final[v], use_fused=1)
        assert got.view == v and want["triangles"].shape[0] > 1000
        assert np.array_equal(got.triangles, want["triangles"]) and np.array_equal(got.pixel, want["pixel"])
        assert np.array_equal(got.vclass, want["vclass"]) and np.array_equal(got.confidence, want["confidence"])
        assert got.points.tobytes() == want["points"].tobytes()
        worst[0] = max(worst[0], float(np.abs(got.normals - want["normals"]).max()))
        worst[1] = max(worst[1], float((np.abs(got.scale - want["scale"]) / want["scale"]).max()))
        assert (got.rgb == sc["images"][v][got.pixel[:, 1], got.pixel[:, 0]][:, None]).all()
    print(f"densify meshes: {[m.points.shape[0] for m in res.meshes]} vertices, {res.pset.points.shape[0]} in the point set, "
          f"max |d normal| {worst[0]:.3e}, max rel d scale {worst[1]:.3e}, {res.mesh_ms:.2f} ms")
    assert worst[0] <= mc.BOUNDS["normals"] and worst[1] <= mc.BOUNDS["scale"]
    ps = res.pset
    keep = [m.confidence > 0.0 for m in res.meshes]
    for field in ("points", "normals", "confidence", "scale", "pixel", "rgb"):
        assert np.array_equal(getattr(ps, field), np.concatenate([getattr(m, field)[k] for m, k in zip(res.meshes, keep)])), field
    assert np.array_equal(ps.view, np.concatenate([np.full(int(k.sum()), v, np.int32) for v, k in enumerate(keep)]))
    assert 1000 < ps.points.shape[0] < sum(m.points.shape[0] for m in res.meshes) and (ps.confidence > 0.0).all()
    # the files
    folder = _project(tmp_path, "with", res)
    assert sorted(os.listdir(folder)) == sorted(["tracks.txt", "cameras.txt", "sparse_cloud.ply", "time_measurements.txt", "dense_cloud.ply",
                                                 "dense_pset.ply"] + ["dense_mesh_%04d.ply" % v for v in range(4)])
    back = dense.read_mesh(str(folder / "dense_pset.ply"))
    assert np.array_equal(back["points"], ps.points.astype(np.float32)) and np.array_equal(back["normals"], ps.normals.astype(np.float32))
    assert np.array_equal(back["confidence"], ps.confidence) and np.array_equal(back["scale"], ps.scale.astype(np.float32))
    assert np.array_equal(back["rgb"], ps.rgb) and back["triangles"].shape == (0, 3)
    for v, m in enumerate(res.meshes):
        back = dense.read_mesh(str(folder / ("dense_mesh_%04d.ply" % v)))
        assert np.array_equal(back["triangles"], m.triangles) and np.array_equal(back["points"], m.points.astype(np.float32))
        assert np.array_equal(back["rgb"], m.rgb) and np.array_equal(back["confidence"], m.confidence)


def test_without_meshes_nothing_changes(tmp_path):
    plain, meshed = densified(False), densified(True)
    assert plain.meshes is None and plain.pset is None and plain.mesh_ms == 0.0
    for field in ("points", "rgb", "view", "pixel"):
        assert getattr(plain, field).tobytes() == getattr(meshed, field).tobytes(), field
    assert plain.counters == meshed.counters
    for a, b in zip(plain.maps, meshed.maps):
        assert a.depth.tobytes() == b.depth.tobytes() and a.status.tobytes() == b.status.tobytes()
    folder = _project(tmp_path, "plain", plain)
    assert sorted(os.listdir(folder)) == sorted(["tracks.txt", "cameras.txt", "sparse_cloud.ply", "time_measurements.txt", "dense_cloud.ply"])
    direct = tmp_path / "direct.ply"
    dense.write_cloud(str(direct), plain.points, plain.rgb)
    assert open(folder / "dense_cloud.ply", "rb").read() == open(direct, "rb").read()
    other = _project(tmp_path, "meshed", meshed)
    for name in ("tracks.txt", "cameras.txt", "sparse_cloud.ply", "dense_cloud.ply"):
        assert open(folder / name, "rb").read() == open(other / name, "rb").read(), name
