"""The slanted-plane refinement on the device against tests/dense_refine_restatement.py, through the C ABI, on every
case of tests/dense_refine_cases.py: statuses equal outside the ambiguous pixels, depth, gradient, normal and score
within dense_refine_cases.BOUNDS; repeatability and independence; what the fusion and the meshes make of a refined
map; the error codes and the memory ledger."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
import dense_refine_cases as rc
import dense_refine_restatement as drr
import dense_restatement as dr
from orthosfm_amd import capi
from orthosfm_amd.dense import DenseStereo

pytestmark = pytest.mark.gpu


def _handle(c):
    d = DenseStereo(0, len(c.images))
    for v, im in enumerate(c.images):
        d.set_image(v, im)
    d.set_cameras(c.P)
    return d


def _upload(d, name, k):
    sw, m = rc.scene(name).sweeps[k], rc.swept(name)[k]
    d.set_map(sw.ref, m["depth"], m["status"], sw.dz, score=m["score"])
    return sw, m


def _bytes(r):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (r.depth, r.gradient, r.normal, r.score, r.status))


_results = {}


def device(name):
    """{sweep index: RefinedMap} of a case on the device, each map uploaded and refined once: shared."""
    if name not in _results:
        c = rc.scene(name)
        out = {}
        with _handle(c) as d:
            for k in rc.CASES[name]["sweeps"]:
                sw, _ = _upload(d, name, k)
                out[k] = d.refine(sw.ref, sw.sources, **rc.refine_options(name, k))
        _results[name] = out
    return _results[name]


def test_defaults_are_the_restatements():
    o = capi.default_dense_refine_options()
    assert {k: getattr(o, k) for k in drr.DEFAULTS} == drr.DEFAULTS
    assert len(capi.DENSE_REFINE_STATUS) == len(drr.STATUS_NAMES) == 8
    assert [s.upper() for s in capi.DENSE_REFINE_STATUS] == list(drr.STATUS_NAMES)


@pytest.mark.parametrize("name", rc.NAMES)
def test_refinement_equals_the_restatement(name):
    c = rc.scene(name)
    worst = dict.fromkeys(rc.BOUNDS, 0.0)
    for k, got in device(name).items():
        sw, m, want = c.sweeps[k], rc.swept(name)[k], rc.restated(name)[k]
        R = rc.refine_options(name, k).get("radius", drr.DEFAULTS["radius"])
        clear = ~rc.ambiguous(want)
        assert np.array_equal(got.status[clear], want["status"][clear]), (name, k)
        # NaN and untouched exactly where the status says so
        ref = got.status == drr.REFINED
        assert np.isnan(got.gradient[~ref]).all() and np.isnan(got.normal[~ref]).all()
        assert np.isfinite(got.gradient[ref]).all() and np.isfinite(got.normal[ref]).all()
        assert got.depth[~ref].tobytes() == np.asarray(m["depth"])[~ref].tobytes()
        assert got.score[~ref].tobytes() == np.asarray(m["score"])[~ref].tobytes()
        assert np.array_equal(got.status == drr.NOT_OK, m["status"] != dr.OK)
        counts = np.bincount(got.status.ravel(), minlength=8)
        assert list(got.stats.status_count) == counts.tolist() and counts.sum() == got.status.size
        both = ref & (want["status"] == drr.REFINED) & clear
        if both.any():
            worst["depth_steps"] = max(worst["depth_steps"], float(np.abs(got.depth - want["depth"])[both].max()) / sw.dz)
            worst["gradient_steps"] = max(worst["gradient_steps"], float(np.abs(got.gradient - want["gradient"])[both].max()) * R / sw.dz)
            worst["normal"] = max(worst["normal"], float(np.abs(got.normal - want["normal"])[both].max()))
            worst["score"] = max(worst["score"], float(np.abs(got.score.astype(np.float64) - want["score"])[both].max()))
            assert got.stats.iterations == int(want["iterations"][clear].sum()) or rc.ambiguous(want).any()
            assert got.stats.samples > 0 and got.stats.device_ms > 0.0
        if name == "border" and k == 0:
            # the touch pixel's window ends exactly on the last column and row of view 3, its third source: it counts,
            # so the pixel is refined as the restatement refines it, which counts it too
            tx, ty = c.paths["touch"]
            assert want["status"][ty, tx] == drr.REFINED and got.status[ty, tx] == drr.REFINED
    print(f"{name}: " + ", ".join(f"max d {key} {val:.3e}" for key, val in worst.items()))
    for key, val in worst.items():
        assert val <= rc.BOUNDS[key], (name, key, val)


def test_repeats_and_does_not_depend_on_order():
    c = rc.scene("slanted")
    first = device("slanted")
    with _handle(c) as d:
        for k in (3, 1):
            _upload(d, "slanted", k)
        sw3, sw1 = c.sweeps[3], c.sweeps[1]
        a = d.refine(sw3.ref, sw3.sources, **rc.refine_options("slanted", 3))
        b = d.refine(sw1.ref, sw1.sources, **rc.refine_options("slanted", 1))
        assert _bytes(a) == _bytes(first[3]) and _bytes(b) == _bytes(first[1])
        # the same call on the same map, with another view refined in between
        _upload(d, "slanted", 3)
        _upload(d, "slanted", 0)
        sw0 = c.sweeps[0]
        d.refine(sw0.ref, sw0.sources, radius=1)
        again = d.refine(sw3.ref, sw3.sources, download=False, **rc.refine_options("slanted", 3))
        assert again.depth is None and list(again.stats.status_count) == list(first[3].stats.status_count)
        gradient, normal, status = d.refined_planes(sw3.ref)
        assert gradient.tobytes() == first[3].gradient.tobytes() and normal.tobytes() == first[3].normal.tobytes()
        assert np.array_equal(status, first[3].status)
        # refining twice refines the refined depths: allowed, and another result
        twice = d.refine(sw3.ref, sw3.sources, **rc.refine_options("slanted", 3))
        assert (twice.status == drr.REFINED).sum() > 1000 and _bytes(twice) != _bytes(first[3])


@pytest.mark.parametrize("name", ["slanted", "step"])
def test_fusion_and_meshes_take_the_refined_map(name):
    c = dc.case(name)
    with _handle(c) as d:
        for sw in c.sweeps:
            d.sweep(sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, download=False, **dc.sweep_options(c, sw))
        o = {key: c.options[key] for key in ("radius", "min_sources", "min_score") if key in c.options}
        refined = {sw.ref: d.refine(sw.ref, sw.sources, **o) for sw in c.sweeps}
        assert capi.lib.osfm_dense_download_cloud(d._h, 0, None, None, None) == capi.E_STATE       # no fusion yet
        cloud = d.fuse(**c.options)
        assert cloud.points.shape[0] > 1000
        hit = 0
        for v, r in refined.items():
            sel = cloud.view == v
            px = cloud.pixel[sel]
            z = r.depth[px[:, 1], px[:, 0]]
            X = dr.Geometry(c.P[v]).point(px[:, 0].astype(np.float64), px[:, 1].astype(np.float64), z)
            want = np.stack(X, axis=1)
            assert cloud.points[sel].tobytes() == want.tobytes(), (name, v)
            hit += int((r.status[px[:, 1], px[:, 0]] == drr.REFINED).sum())
        assert hit > 1000
        v = c.sweeps[0].ref
        plain, with_normals = d.mesh(v, refined_normals=0), d.mesh(v, refined_normals=1)
        for key in ("triangles", "pixel", "vclass", "confidence", "scale", "points"):
            assert getattr(plain, key).tobytes() == getattr(with_normals, key).tobytes(), key
        px = plain.pixel
        ref = refined[v].status[px[:, 1], px[:, 0]] == drr.REFINED
        assert ref.sum() > 1000 and (~ref).sum() > 0
        assert with_normals.normals[ref].tobytes() == refined[v].normal[px[ref, 1], px[ref, 0]].tobytes()
        assert with_normals.normals[~ref].tobytes() == plain.normals[~ref].tobytes()
        assert with_normals.normals[ref].tobytes() != plain.normals[ref].tobytes()


def _raw_refine(d, view, sources, shape, **options):
    """osfm_dense_refine_view with outputs full of a sentinel; returns (status code, outputs untouched)."""
    outs = [np.full(shape, 7.5), np.full(shape + (2,), 7.5), np.full(shape + (3,), 7.5), np.full(shape, 7.5, np.float32), np.full(shape, 77, np.uint8)]
    before = [a.copy() for a in outs]
    stats = capi.DenseRefineStats()
    stats.iterations = 77
    o = capi.DenseRefineOptions()
    capi.check(capi.lib.osfm_dense_refine_options_default(C.byref(o)))
    for key, val in options.items():
        setattr(o, key, val)
    src = np.ascontiguousarray(sources, dtype=np.int32)
    rcode = capi.lib.osfm_dense_refine_view(d._h, view, src.shape[0], src.ctypes.data, C.byref(o), *[a.ctypes.data for a in outs], C.byref(stats))
    return rcode, all(np.array_equal(a, b) for a, b in zip(outs, before)) and stats.iterations == 77


def _raw_planes(d, view, shape):
    outs = [np.full(shape + (2,), 7.5), np.full(shape + (3,), 7.5), np.full(shape, 77, np.uint8)]
    before = [a.copy() for a in outs]
    rcode = capi.lib.osfm_dense_download_refined(d._h, view, *[a.ctypes.data for a in outs])
    return rcode, all(np.array_equal(a, b) for a, b in zip(outs, before))


def test_error_codes_write_nothing():
    c = rc.scene("one_source")
    sw, m = c.sweeps[0], rc.swept("one_source")[0]
    shape = m["status"].shape
    want = device("one_source")[0]
    o = rc.refine_options("one_source", 0)
    with DenseStereo(0, 3) as d:
        P3 = np.concatenate([c.P, c.P[:1]])
        assert _raw_refine(d, 0, [1], shape, **o) == (capi.E_STATE, True)                  # no cameras
        d.set_cameras(P3)
        d.set_image(0, c.images[0])
        assert _raw_refine(d, 0, [1], shape, **o) == (capi.E_STATE, True)                  # no map
        d.set_map(0, m["depth"], m["status"], sw.dz, score=m["score"])
        assert _raw_refine(d, 0, [1], shape, **o) == (capi.E_STATE, True)                  # the source has no image
        assert _raw_planes(d, 0, shape) == (capi.E_STATE, True)                            # not refined
        d.set_image(1, c.images[1])
        for bad in (dict(radius=0), dict(radius=8), dict(min_sources=0), dict(min_sources=9), dict(max_iterations=0), dict(max_iterations=101),
                    dict(eps=0.0), dict(eps=np.nan), dict(max_shift=-1.0), dict(max_deform=0.5), dict(min_score=1.5), dict(min_pivot=0.0),
                    dict(min_pivot=1.0), dict(min_sources=2)):
            assert _raw_refine(d, 0, [1], shape, **dict(o, **bad)) == (capi.E_ARG, True), bad
        assert _raw_refine(d, 0, [0], shape, **o) == (capi.E_ARG, True)                    # the view itself
        assert _raw_refine(d, 0, [1, 1], shape, **o) == (capi.E_ARG, True)                 # named twice
        assert _raw_refine(d, 0, np.zeros(0, np.int32), shape, **o) == (capi.E_ARG, True)
        assert _raw_refine(d, 0, list(range(1, 10)), shape, **o) == (capi.E_ARG, True)
        assert _raw_refine(d, 3, [1], shape, **o) == (capi.E_RANGE, True) and _raw_refine(d, -1, [1], shape, **o) == (capi.E_RANGE, True)
        assert _raw_refine(d, 0, [3], shape, **o) == (capi.E_RANGE, True)
        assert _raw_refine(d, 0, [2], shape, **o) == (capi.E_STATE, True)                  # view 2 has no image
        assert _raw_refine(d, 1, [0], shape, **o) == (capi.E_STATE, True)                  # view 1 has no map
        assert capi.lib.osfm_dense_refine_view(None, 0, 1, np.zeros(1, np.int32).ctypes.data, *[None] * 7) == capi.E_ARG
        assert capi.lib.osfm_dense_refine_view(d._h, 0, 1, None, *[None] * 7) == capi.E_ARG
        assert capi.lib.osfm_dense_refine_options_default(None) == capi.E_ARG
        assert _raw_planes(d, 3, shape) == (capi.E_RANGE, True) and capi.lib.osfm_dense_download_refined(None, 0, None, None, None) == capi.E_ARG
        with pytest.raises(capi.OsfmError) as e:                                           # the mesh flag needs a refined map
            d.mesh(0, refined_normals=1)
        assert e.value.status == capi.E_STATE
        # none of the refused calls touched the map
        got = d.refine(0, [1], **o)
        assert _bytes(got) == _bytes(want)
        assert _raw_planes(d, 0, shape)[0] == capi.OK
        assert capi.lib.osfm_dense_download_refined(d._h, 0, None, None, None) == capi.OK
        d.mesh(0, refined_normals=1)
        # a new map, a new image and new cameras drop the refined planes
        d.set_map(0, m["depth"], m["status"], sw.dz, score=m["score"])
        assert _raw_planes(d, 0, shape) == (capi.E_STATE, True)
        d.refine(0, [1], download=False, **o)
        d.set_image(0, c.images[0])
        assert _raw_planes(d, 0, shape) == (capi.E_STATE, True)
        d.set_map(0, m["depth"], m["status"], sw.dz, score=m["score"])
        d.refine(0, [1], download=False, **o)
        d.set_cameras(P3)
        assert _raw_planes(d, 0, shape) == (capi.E_STATE, True)


def test_memory_grows_by_the_planes_and_returns():
    c = rc.scene("one_source")
    sw, m = c.sweeps[0], rc.swept("one_source")[0]
    before = capi.library_memory().device_buffer_bytes
    d = _handle(c)
    d.set_map(0, m["depth"], m["status"], sw.dz, score=m["score"])
    held = capi.library_memory().device_buffer_bytes - before
    d.refine(0, [1], download=False, **rc.refine_options("one_source", 0))
    n = m["status"].size
    grown = capi.library_memory().device_buffer_bytes - before - held
    assert n * (1 + 16 + 24) <= grown <= n * (1 + 16 + 24) * 9 // 8 + 4 * 256 + 8192
    d.close()
    assert capi.library_memory().device_buffer_bytes == before
