"""The depth-map meshes on the device against tests/mesh_restatement.py, through the C ABI, on every case of
tests/mesh_cases.py: triangles, pixels, classes, confidences and counters exactly, points to the bit, normals and
scales within mesh_cases.BOUNDS; the device's own sweeps meshed as the restatement meshes the downloaded maps; the
upload of a map, repeatability, the error codes, the memory ledger and the PLY file."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
import mesh_cases as mc
import mesh_restatement as mr
from orthosfm_amd import capi, dense
from orthosfm_amd.dense import DenseStereo

pytestmark = pytest.mark.gpu

COUNTERS = ("pixels_solid", "pixels_island", "components", "triangles_dropped", "vertices_simple", "vertices_border", "vertices_complex")


def _handle(m):
    d = DenseStereo(0, 1)
    d.set_image(0, m.image)
    d.set_cameras(m.P[None])
    d.set_map(0, m.depth, m.status, m.dz)
    return d


_results = {}


def device(name, i):
    """The device's meshes of every run of map i of a case: computed once, shared."""
    if (name, i) not in _results:
        m = mc.case(name)[i]
        with _handle(m) as d:
            _results[(name, i)] = [d.mesh(0, **run) for run in m.runs]
    return _results[(name, i)]


def _bytes(m):
    return b"".join(a.tobytes() for a in (m.points, m.normals, m.confidence, m.scale, m.pixel, m.vclass, m.triangles))


def _compare(got, want, label):
    """Holds a device mesh to a restated one; returns the largest differences of the normals and of the scales."""
    assert got.triangles.shape == want["triangles"].shape and np.array_equal(got.triangles, want["triangles"]), label
    assert np.array_equal(got.pixel, want["pixel"]), label
    assert np.array_equal(got.vclass, want["vclass"]), label
    assert got.confidence.dtype == np.float32 and np.array_equal(got.confidence, want["confidence"]), label
    assert got.points.tobytes() == want["points"].tobytes(), label
    counters = got.stats.counters()
    for key in COUNTERS:
        assert counters[key] == want["stats"][key], (label, key)
    assert got.stats.threshold_steps == want["stats"]["threshold_steps"], label
    d_n = float(np.abs(got.normals - want["normals"]).max(initial=0.0))
    d_s = float((np.abs(got.scale - want["scale"]) / want["scale"]).max(initial=0.0)) if want["scale"].size else 0.0
    return d_n, d_s


def test_limits_are_what_the_cases_assume():
    assert capi.dense_mesh_limits() == (*mc.LABEL_TILE, mc.MAX_CONFIDENCE_ITERATIONS)
    assert mr.MAX_CONFIDENCE_ITERATIONS == mc.MAX_CONFIDENCE_ITERATIONS
    o = capi.default_dense_mesh_options()
    assert {k: getattr(o, k) for k in mr.DEFAULTS} == mr.DEFAULTS


@pytest.mark.parametrize("name,i,j", mc.runs())
def test_mesh_equals_the_restatement(name, i, j):
    m = mc.case(name)[i]
    got, want = device(name, i)[j], mc.restated(name, i, j)
    d_n, d_s = _compare(got, want, (name, m.label, m.runs[j]))
    print(f"{name} {m.label} {m.runs[j]}: {got.points.shape[0]} vertices, {got.triangles.shape[0]} triangles, "
          f"max |d normal| {d_n:.3e}, max rel d scale {d_s:.3e}")
    assert d_n <= mc.BOUNDS["normals"] and d_s <= mc.BOUNDS["scale"]
    assert got.stats.device_ms > 0.0 and len(list(got.stats.stage_ms)) == len(capi.MESH_STAGES)


def _swept(c):
    d = DenseStereo(0, len(c.images))
    for v, im in enumerate(c.images):
        d.set_image(v, im)
    d.set_cameras(c.P)
    maps = [d.sweep(sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, **dc.sweep_options(c, sw)) for sw in c.sweeps]
    d.fuse(**c.options)
    return d, maps


_sweeps = {}


def swept(name):
    """(maps, final statuses, meshes[use_fused][view]) of the device's own sweeps and fusion of a dense case."""
    if name not in _sweeps:
        c = dc.case(name)
        d, maps = _swept(c)
        with d:
            final = [d.fused_status(sw.ref) for sw in c.sweeps]
            meshes = [[d.mesh(sw.ref, use_fused=f, min_island=mc.MIN_ISLAND) for sw in c.sweeps] for f in (0, 1)]
        _sweeps[name] = (maps, final, meshes)
    return _sweeps[name]


@pytest.mark.parametrize("use_fused", [0, 1])
@pytest.mark.parametrize("name", ["slanted", "step"])
def test_own_sweeps_mesh_as_the_restatement_meshes_the_downloaded_maps(name, use_fused):
    c = dc.case(name)
    maps, final, meshes = swept(name)
    worst = [0.0, 0.0]
    for k, sw in enumerate(c.sweeps):
        want = mr.mesh(c.P[sw.ref], maps[k].depth, maps[k].status, sw.dz, final=final[k], use_fused=use_fused, min_island=mc.MIN_ISLAND)
        d = _compare(meshes[use_fused][k], want, (name, sw.ref, use_fused))
        worst = [max(a, b) for a, b in zip(worst, d)]
        assert want["triangles"].shape[0] > 1000
    print(f"{name} use_fused {use_fused}: max |d normal| {worst[0]:.3e}, max rel d scale {worst[1]:.3e}")
    assert worst[0] <= mc.BOUNDS["normals"] and worst[1] <= mc.BOUNDS["scale"]
    if use_fused:
        assert sum(m.points.shape[0] for m in meshes[1]) < sum(m.points.shape[0] for m in meshes[0])


def test_an_uploaded_sweep_meshes_to_the_same_bytes():
    c = dc.case("step")
    maps, final, meshes = swept("step")
    with DenseStereo(0, len(c.images)) as d:
        for v, im in enumerate(c.images):
            d.set_image(v, im)
        d.set_cameras(c.P)
        for sw, m in zip(c.sweeps, maps):
            d.set_map(sw.ref, m.depth, m.status, sw.dz, score=m.score)
        first = d.mesh(c.sweeps[2].ref, min_island=mc.MIN_ISLAND)
        assert _bytes(first) == _bytes(meshes[0][2])
        with pytest.raises(capi.OsfmError) as e:                    # uploaded maps are not fused yet
            d.mesh(c.sweeps[0].ref, use_fused=1)
        assert e.value.status == capi.E_STATE
        d.fuse(**c.options)
        for k, sw in enumerate(c.sweeps):
            assert np.array_equal(d.fused_status(sw.ref), final[k])
            assert _bytes(d.mesh(sw.ref, use_fused=1, min_island=mc.MIN_ISLAND)) == _bytes(meshes[1][k])
        # an upload is a sweep to an earlier fusion: it is gone
        d.set_map(c.sweeps[0].ref, maps[0].depth, maps[0].status, c.sweeps[0].dz)
        assert capi.lib.osfm_dense_download_cloud(d._h, 0, None, None, None) == capi.E_STATE


def test_repeats_and_does_not_depend_on_what_was_meshed_before():
    m = mc.case("islands")[0]
    first = device("islands", 0)
    other = mc.case("classes")[0]
    with DenseStereo(0, 2) as d:
        d.set_image(0, m.image)
        d.set_image(1, other.image)
        d.set_cameras(np.stack([m.P, other.P]))
        d.set_map(1, other.depth, other.status, other.dz)
        d.mesh(1)                                                # larger options, another size: what the buffers held before
        d.set_map(0, m.depth, m.status, m.dz)
        for j in (2, 0, 1, 0):
            assert _bytes(d.mesh(0, **m.runs[j])) == _bytes(first[j]), j
            d.mesh(1, confidence_iterations=mc.MAX_CONFIDENCE_ITERATIONS)
        assert _bytes(d.mesh(1, **other.runs[0])) == _bytes(device("classes", 0)[0])


def _raw_mesh(d, view, **options):
    """osfm_dense_mesh_view with outputs full of a sentinel; returns (status code, outputs untouched)."""
    nv, nt, stats = C.c_int64(-7), C.c_int64(-7), capi.DenseMeshStats()
    stats.components = 77
    o = capi.DenseMeshOptions()
    capi.check(capi.lib.osfm_dense_mesh_options_default(C.byref(o)))
    for k, v in options.items():
        setattr(o, k, v)
    rcode = capi.lib.osfm_dense_mesh_view(d._h, view, C.byref(o), C.byref(nv), C.byref(nt), C.byref(stats))
    return rcode, nv.value == -7 and nt.value == -7 and stats.components == 77


def _raw_download(d, V, T):
    outs = [np.full((max(V, 1), 3), 7.5), np.full((max(V, 1), 3), 7.5), np.full(max(V, 1), 7.5, np.float32), np.full(max(V, 1), 7.5),
            np.full((max(V, 1), 2), 77, np.int32), np.full(max(V, 1), 77, np.uint8), np.full((max(T, 1), 3), 77, np.int32)]
    before = [a.copy() for a in outs]
    rcode = capi.lib.osfm_dense_download_mesh(d._h, V, T, *[a.ctypes.data for a in outs])
    return rcode, all(np.array_equal(a, b) for a, b in zip(outs, before))


def test_error_codes_write_nothing():
    m = mc.case("classes")[0]
    want = device("classes", 0)[0]
    h, w = m.status.shape
    with DenseStereo(0, 2) as d:
        set_map = lambda view=0, depth=m.depth, status=m.status, dz=m.dz: capi.lib.osfm_dense_set_map(
            d._h, view, np.ascontiguousarray(depth).ctypes.data, None, np.ascontiguousarray(status).ctypes.data, dz)
        assert set_map() == capi.E_STATE                             # no cameras, no image
        d.set_cameras(np.stack([m.P, m.P]))
        assert set_map() == capi.E_STATE                             # no image: no size
        d.set_image(0, m.image)
        assert _raw_mesh(d, 0) == (capi.E_STATE, True)               # no map
        assert _raw_download(d, 10, 10) == (capi.E_STATE, True)      # no mesh
        assert set_map() == capi.OK
        V, T = want.points.shape[0], want.triangles.shape[0]
        good = d.mesh(0)
        assert _bytes(good) == _bytes(want)
        # every refused upload leaves the map, and the mesh on the device, as they are
        bad_status = m.status.copy(); bad_status[0, 0] = capi.DENSE_INCONSISTENT
        bad_depth = m.depth.copy(); bad_depth[m.status == capi.DENSE_OK] = np.inf
        nan_depth = m.depth.copy(); nan_depth[3, 3] = np.nan
        assert m.status[3, 3] == capi.DENSE_OK
        for kw, code in ((dict(status=bad_status), capi.E_ARG), (dict(depth=bad_depth), capi.E_ARG), (dict(depth=nan_depth), capi.E_ARG),
                         (dict(dz=0.0), capi.E_ARG), (dict(dz=-1.0), capi.E_ARG), (dict(dz=np.nan), capi.E_ARG), (dict(dz=np.inf), capi.E_ARG),
                         (dict(view=2), capi.E_RANGE), (dict(view=-1), capi.E_RANGE), (dict(view=1), capi.E_STATE)):
            assert set_map(**kw) == code, kw
            assert _raw_download(d, V, T)[0] == capi.OK
        assert capi.lib.osfm_dense_set_map(d._h, 0, None, None, m.status.ctypes.data, m.dz) == capi.E_ARG
        assert capi.lib.osfm_dense_set_map(d._h, 0, m.depth.ctypes.data, None, None, m.dz) == capi.E_ARG
        assert _bytes(d.mesh(0)) == _bytes(want)
        for options in (dict(dd_factor=-1.0), dict(dd_factor=np.nan), dict(dd_factor=np.inf), dict(confidence_iterations=-1),
                        dict(confidence_iterations=mc.MAX_CONFIDENCE_ITERATIONS + 1), dict(min_island=-1)):
            assert _raw_mesh(d, 0, **options) == (capi.E_ARG, True), options
        for view in (2, -1):
            assert _raw_mesh(d, view) == (capi.E_RANGE, True), view
        assert _raw_mesh(d, 1) == (capi.E_STATE, True)               # view 1 has no map
        assert _raw_mesh(d, 0, use_fused=1) == (capi.E_STATE, True)  # no fusion
        assert capi.lib.osfm_dense_mesh_view(None, 0, None, None, None, None) == capi.E_ARG
        assert capi.lib.osfm_dense_mesh_options_default(None) == capi.E_ARG
        # the refused calls left the last mesh where it was
        assert _raw_download(d, V - 1, T) == (capi.E_CAPACITY, True) and _raw_download(d, V, T - 1) == (capi.E_CAPACITY, True)
        assert _raw_download(d, V, T)[0] == capi.OK
        assert capi.lib.osfm_dense_download_mesh(d._h, V, T, *[None] * 7) == capi.OK
        assert capi.lib.osfm_dense_mesh_view(d._h, 0, None, None, None, None) == capi.OK        # defaults, no outputs
        assert _raw_download(d, V, T)[0] == capi.OK
        # new cameras or a new image drop the mesh with the map
        d.set_cameras(np.stack([m.P, m.P]))
        assert _raw_download(d, V, T) == (capi.E_STATE, True) and _raw_mesh(d, 0) == (capi.E_STATE, True)
        assert set_map() == capi.OK and capi.lib.osfm_dense_mesh_view(d._h, 0, None, None, None, None) == capi.OK
        d.set_image(0, m.image)
        assert _raw_download(d, V, T) == (capi.E_STATE, True)
        d.set_image(1, np.zeros((1, 1), np.uint8))
        assert set_map(view=1, depth=np.zeros((1, 1)), status=np.zeros((1, 1), np.uint8)) == capi.OK
        assert _raw_mesh(d, 1)[0] == capi.OK and _raw_download(d, 0, 0)[0] == capi.OK


def test_memory_returns_after_destroy():
    m = mc.case("islands")[0]
    before = capi.library_memory().device_buffer_bytes
    d = _handle(m)
    held = capi.library_memory().device_buffer_bytes - before
    n = m.status.size
    assert held >= n * (4 + 8 + 4 + 1)
    d.mesh(0, min_island=mc.MIN_ISLAND)
    assert capi.library_memory().device_buffer_bytes - before >= held + 16 * n       # the labelling's arrays and the scans, at the least
    d.close()
    assert capi.library_memory().device_buffer_bytes == before


def test_ply_round_trip(tmp_path):
    got = device("classes", 0)[0]
    rgb = (np.arange(got.points.shape[0] * 3) % 251).astype(np.uint8).reshape(-1, 3)
    path = tmp_path / "mesh.ply"
    dense.write_mesh(str(path), got.points, got.normals, rgb, got.confidence, got.scale, got.triangles)
    back = dense.read_mesh(str(path))
    assert np.array_equal(back["points"], got.points.astype(np.float32)) and np.array_equal(back["normals"], got.normals.astype(np.float32))
    assert np.array_equal(back["rgb"], rgb) and np.array_equal(back["confidence"], got.confidence)
    assert np.array_equal(back["scale"], got.scale.astype(np.float32)) and np.array_equal(back["triangles"], got.triangles)
    head = open(path, "rb").read(600).split(b"end_header\n")[0].decode().splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {got.points.shape[0]}"]
    assert [l.split()[-1] for l in head[3:14]] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "confidence", "value"]
    assert head[14:] == [f"element face {got.triangles.shape[0]}", "property list uchar int vertex_indices"]
    # the point-set form: no face element, defaults for what is not given
    pset = tmp_path / "pset.ply"
    dense.write_mesh(str(pset), got.points, got.normals, confidence=got.confidence, scale=got.scale)
    back = dense.read_mesh(str(pset))
    assert b"element face" not in open(pset, "rb").read(600) and back["triangles"].shape == (0, 3)
    assert np.array_equal(back["confidence"], got.confidence) and (back["rgb"] == 0).all()
    with pytest.raises(capi.OsfmError) as e:
        dense.write_mesh(str(tmp_path / "bad.ply"), got.points[:3], triangles=[[0, 1, 3]])
    assert e.value.status == capi.E_RANGE
