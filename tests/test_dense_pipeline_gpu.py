"""pipeline.densify on four rendered 160 x 128 views of the two-plane step, with ground-truth cameras and 40 sparse
points: the cloud has points on both planes, is as accurate as the restatement's on the same plan, and
save_project writes a dense_cloud.ply that reads back."""
import numpy as np
import pytest

import dense_cases as dc
from orthosfm_amd import capi, dense, pipeline

pytestmark = pytest.mark.gpu


def test_densify_the_step(tmp_path):
    sc = dc.pipeline_scene()
    res = pipeline.densify(sc["images"], sc["model"], sc["cam_params"], sc["points"], sc["visibility"], keep_maps=True,
                           **dc.PIPELINE_OPTIONS)
    plans, want = dc.restated_pipeline()
    for got, p in zip(res.plans, plans):
        assert got.sources == p.sources and got.num_depths == p.num_depths and got.z_min == p.z_min and got.dz == p.dz
    dzs = {v: p.dz for v, p in enumerate(res.plans)}
    median, within, per_plane = dc.cloud_accuracy(sc, res.points, res.view, res.pixel, dzs)
    print(f"densify: {res.points.shape[0]} points, {per_plane} per plane, median {median:.4f} step, {within:.4f} within one step, "
          f"sweeps {res.sweep_ms:.2f} ms, fusion {res.fuse_ms:.2f} ms")
    rec = dc.MEASURED_CPU_PIPELINE
    assert min(per_plane) > 1000
    assert median <= rec["median_steps"] + dc.BOUNDS["depth_steps"]
    assert within >= rec["within_one_step"] - 0.005          # the share moves with the ambiguous pixels: half a percent of the cloud
    assert abs(res.points.shape[0] - want["points"].shape[0]) <= 0.05 * want["points"].shape[0]
    assert res.counters["ok"] == res.points.shape[0] and res.sweep_ms > 0.0
    for v in range(4):
        assert res.maps[v].status.shape == sc["images"][v].shape and (res.maps[v].status == capi.DENSE_OK).sum() > 5000
    # the colours are the pixels of the emitting views
    k = np.arange(0, res.points.shape[0], 97)
    for i in k:
        assert (res.rgb[i] == sc["images"][res.view[i]][res.pixel[i, 1], res.pixel[i, 0]]).all()
    # the project file
    path = tmp_path / "dense_cloud.ply"
    dense.write_cloud(str(path), res.points, res.rgb)
    xyz, rgb = dense.read_cloud(str(path))
    assert np.array_equal(xyz, res.points.astype(np.float32)) and np.array_equal(rgb, res.rgb)
    head = open(path, "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % res.points.shape[0])


def test_save_project_writes_the_dense_cloud(tmp_path):
    from orthosfm_amd import synth
    tt = pipeline.TrackTable([0, 2, 4], [0, 1, 0, 2], [0, 0, 1, 0], np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]), 3)
    tt.point[:, :3], tt.point[:, 3] = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], 1.0
    tt.has_point[:] = True
    res = pipeline.Result(np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], (3, 1)), [], tt, [], pipeline.Timings(), [])
    pipeline.save_project(res, synth.MODEL_QUATERNION, str(tmp_path / "without"))
    assert not (tmp_path / "without" / "dense_cloud.ply").exists()
    cloud = pipeline.DenseResult(np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]), np.array([[1, 2, 3], [4, 5, 6]], np.uint8),
                                 np.zeros(2, np.int32), np.zeros((2, 2), np.int32), [], [], {}, 0.0, 0.0)
    pipeline.save_project(res, synth.MODEL_QUATERNION, str(tmp_path), dense_cloud=cloud)
    xyz, rgb = dense.read_cloud(str(tmp_path / "dense_cloud.ply"))
    assert np.array_equal(xyz, cloud.points.astype(np.float32)) and np.array_equal(rgb, cloud.rgb)
