"""The dense plane sweep and the fusion on the device against tests/dense_restatement.py, through the C ABI, on every
case of tests/dense_cases.py: statuses outside the ambiguous pixels, depth and score within dense_cases.BOUNDS, the
fused cloud outside what an ambiguous pixel touches; repeatability, independence of the order of the sweeps, the
hand-over from a view front end, the error codes and the memory ledger."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
import dense_restatement as dr
from orthosfm_amd import capi
from orthosfm_amd.dense import DenseStereo
from orthosfm_amd.features import ViewFrontEnd

pytestmark = pytest.mark.gpu


def _handle(c):
    d = DenseStereo(0, len(c.images))
    for v, im in enumerate(c.images):
        d.set_image(v, im)
    d.set_cameras(c.P)
    return d


def _sweep(d, c, sw):
    return d.sweep(sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, **dc.sweep_options(c, sw))


_results = {}


def device(name):
    """The device's result on a case -- its sweeps in order, then the fusion where the case has one: computed once,
    shared."""
    if name not in _results:
        c = dc.case(name)
        with _handle(c) as d:
            maps = [_sweep(d, c, sw) for sw in c.sweeps]
            cloud = final = None
            if c.fuse:
                cloud = d.fuse(**c.options)
                final = {sw.ref: d.fused_status(sw.ref) for sw in c.sweeps}
        _results[name] = (maps, cloud, final)
    return _results[name]


def _bytes(m):
    return b"".join(a.tobytes() for a in (m.depth, m.score, m.status))


def test_limits_are_what_the_cases_assume():
    assert capi.dense_limits() == (32, 16, 7, dr.MAX_SOURCES, dc.MAX_DEPTHS)


@pytest.mark.parametrize("name", dc.NAMES)
def test_status(name):
    c = dc.case(name)
    for sw, want, got in zip(c.sweeps, dc.restated(name), device(name)[0]):
        amb = dc.ambiguous(want)
        differs = got.status != want["status"]
        assert not (differs & ~amb).any(), \
            [(int(x), int(y), dr.STATUS_NAMES[got.status[y, x]], dr.STATUS_NAMES[want["status"][y, x]], float(want["margin"][y, x]))
             for y, x in zip(*np.nonzero(differs & ~amb))][:10]
        # among the ambiguous an index one off is allowed, and nothing else
        both = amb & (got.status == dr.OK) & (want["status"] == dr.OK)
        assert (np.abs(got.depth[both] - want["depth"][both]) <= (1.0 + dc.BOUNDS["depth_steps"]) * sw.dz).all()
        counts = got.stats.counters()
        for i, key in enumerate(capi.DENSE_STATUS):
            assert counts[key] == int((got.status == i).sum()), key
        assert sum(counts.values()) == got.status.size
        if name == "border" and len(sw.sources) == 2:
            x, y = c.paths["touch"]
            assert got.status[y, x] == want["status"][y, x] != dr.NO_SOURCES
            assert got.status[y, x + 1] == dr.NO_SOURCES and got.status[y + 1, x] == dr.NO_SOURCES


@pytest.mark.parametrize("name", dc.NAMES)
def test_values(name):
    c = dc.case(name)
    for sw, want, got in zip(c.sweeps, dc.restated(name), device(name)[0]):
        ok = got.status == dr.OK
        both = ok & (want["status"] == dr.OK) & ~dc.ambiguous(want)
        d_score = float(np.abs(got.score[both].astype(np.float64) - want["score"][both]).max()) if both.any() else 0.0
        d_depth = float(np.abs(got.depth[both] - want["depth"][both]).max() / sw.dz) if both.any() else 0.0
        print(f"{name} view {sw.ref}: {int(both.sum())} OK in both, max |d score| {d_score:.3e}, |d depth| {d_depth:.3e} step")
        assert d_score <= dc.BOUNDS["score"] and d_depth <= dc.BOUNDS["depth_steps"]
        assert np.isnan(got.depth[~ok]).all() and np.isfinite(got.depth[ok]).all() and (got.score[~ok] == 0.0).all()


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.case(n).fuse])
def test_fused_cloud(name):
    c, want = dc.case(name), dc.restated_fusion(name)
    _, cloud, final = device(name)
    dzs = {sw.ref: sw.dz for sw in c.sweeps}
    for v in final:
        clear = ~want["touched"][v]
        assert np.array_equal(final[v][clear], want["final"][v][clear]), v
    counts = cloud.stats.counters()
    for i, key in enumerate(capi.DENSE_STATUS):
        assert counts[key] == sum(int((final[v] == i).sum()) for v in final), key
    assert cloud.points.shape[0] == counts["ok"]
    # the cloud outside the touched pixels: the same pixels in the same order, the points a depth bound apart
    g_clear = ~np.array([want["touched"][v][y, x] for v, (x, y) in zip(cloud.view, cloud.pixel)], bool)
    w_clear = ~np.array([want["touched"][v][y, x] for v, (x, y) in zip(want["view"], want["pixel"])], bool)
    assert w_clear.sum() > 0.5 * w_clear.size
    assert np.array_equal(cloud.view[g_clear], want["view"][w_clear]) and np.array_equal(cloud.pixel[g_clear], want["pixel"][w_clear])
    step = np.array([dzs[int(v)] for v in want["view"][w_clear]])
    assert (np.linalg.norm(cloud.points[g_clear] - want["points"][w_clear], axis=1) <= dc.BOUNDS["depth_steps"] * step * (1 + 1e-9)).all()
    key = (cloud.view.astype(np.int64) << 40) + (cloud.pixel[:, 1].astype(np.int64) << 20) + cloud.pixel[:, 0]
    assert (np.diff(key) > 0).all()
    # every emitted point is its pixel at its depth
    maps = {sw.ref: m for sw, m in zip(c.sweeps, device(name)[0])}
    for v in final:
        sel = cloud.view == v
        px = cloud.pixel[sel]
        X = dr.Geometry(c.P[v]).point(px[:, 0].astype(np.float64), px[:, 1].astype(np.float64), maps[v].depth[px[:, 1], px[:, 0]])
        assert np.array_equal(np.stack(X, axis=1), cloud.points[sel])


def test_repeats_and_does_not_depend_on_what_was_swept_before():
    c = dc.case("slanted")
    first = device("slanted")
    with _handle(c) as d:
        alone = _sweep(d, c, c.sweeps[2])                  # view 2 first, in a fresh handle
        again = [_sweep(d, c, sw) for sw in reversed(c.sweeps)][::-1]
        cloud = d.fuse(**c.options)
    assert _bytes(alone) == _bytes(first[0][2])
    for a, b in zip(again, first[0]):
        assert _bytes(a) == _bytes(b)
    assert cloud.points.tobytes() == first[1].points.tobytes() and cloud.view.tobytes() == first[1].view.tobytes()
    assert cloud.pixel.tobytes() == first[1].pixel.tobytes()


def test_image_from_front_equals_upload():
    """set_image_from_front gives what set_image gives on debug_image()'s bytes; the front end halves once, so the
    feature image is not the input and the cameras are those of the halved images."""
    c = dc.case("slanted")
    P = c.P.copy()
    P[:, :, :3] *= 0.5
    P[:, :, 3] = (P[:, :, 3] - 0.5) / 2.0
    sw = c.sweeps[0]
    with ViewFrontEnd(0, 96, 80, max_image_size=6000) as front, DenseStereo(0, 4) as a, DenseStereo(0, 4) as b:
        for v, im in enumerate(c.images):
            s = front.load(im)
            assert s.num_halvings == 1
            a.set_image_from_front(v, front, (s.feature_height, s.feature_width))
            shown = front.debug_image()
            assert shown.shape[:2] == (s.feature_height, s.feature_width)
            b.set_image(v, shown)
        a.set_cameras(P)
        b.set_cameras(P)
        ra = a.sweep(sw.ref, sw.sources, sw.z_min, 2.0 * sw.dz, sw.num_depths // 2 + 3, radius=2)
        rb = b.sweep(sw.ref, sw.sources, sw.z_min, 2.0 * sw.dz, sw.num_depths // 2 + 3, radius=2)
    assert _bytes(ra) == _bytes(rb)
    assert (ra.status == dr.OK).sum() > 500


def _raw(d, c, sw, ref=None, sources=None, z_min=None, dz=None, num_depths=None, options=None):
    """osfm_dense_sweep with outputs full of a sentinel; returns (status code, outputs untouched)."""
    h, w = c.images[sw.ref].shape[:2]
    outs = [np.full((h, w), 7.5), np.full((h, w), 7.5, np.float32), np.full((h, w), 77, np.uint8)]
    before = [o.copy() for o in outs]
    stats = capi.DenseStats()
    stats.samples = 77
    o = capi.default_dense_options(**dict(dc.sweep_options(c, sw), **(options or {})))
    src = np.ascontiguousarray(sw.sources if sources is None else sources, dtype=np.int32)
    rcode = capi.lib.osfm_dense_sweep(d._h, sw.ref if ref is None else ref, src.shape[0], src.ctypes.data,
                                      sw.z_min if z_min is None else z_min, sw.dz if dz is None else dz,
                                      sw.num_depths if num_depths is None else num_depths, C.byref(o),
                                      *[a.ctypes.data for a in outs], C.byref(stats))
    return rcode, all(np.array_equal(a, b) for a, b in zip(outs, before)) and stats.samples == 77


def test_error_codes_write_nothing():
    c = dc.case("many_depths")
    sw = c.sweeps[0]
    with DenseStereo(0, 3) as d:
        d.set_image(0, c.images[0])
        d.set_image(1, c.images[1])
        assert _raw(d, c, sw) == (capi.E_STATE, True)                 # no cameras yet
        d.set_cameras(c.P)
        assert _raw(d, c, sw) == (capi.E_STATE, True)                 # view 2 has no image yet
        d.set_image(2, c.images[2])
        assert _raw(d, c, sw)[0] == capi.OK                           # num_depths == max_depths runs
        assert _raw(d, c, sw, num_depths=dc.MAX_DEPTHS + 1) == (capi.E_ARG, True)
        assert _raw(d, c, sw, num_depths=2) == (capi.E_ARG, True)
        for ref, sources in ((3, None), (-1, None), (None, [1, 3]), (None, [-1, 2])):
            assert _raw(d, c, sw, ref=ref, sources=sources) == (capi.E_RANGE, True), (ref, sources)
        for sources in ([0, 1], [1, 1], [], [1, 2, 1]):
            assert _raw(d, c, sw, sources=sources) == (capi.E_ARG, True), sources
        for options in (dict(radius=0), dict(radius=8), dict(min_sources=0), dict(min_sources=9), dict(min_sources=3),
                        dict(min_contrast=0.0), dict(min_score=1.5), dict(consistency_tol=-1.0), dict(min_consistent=-1)):
            assert _raw(d, c, sw, options=options) == (capi.E_ARG, True), options
        for kw in (dict(dz=0.0), dict(dz=-1.0), dict(dz=np.nan), dict(z_min=np.inf)):
            assert _raw(d, c, sw, **kw) == (capi.E_ARG, True), kw
        with pytest.raises(capi.OsfmError) as e:
            d.set_image(3, c.images[0])
        assert e.value.status == capi.E_RANGE
        bad = c.P.copy()
        bad[1, 1, :3] = 2.0 * bad[1, 0, :3]
        for P in (bad, np.where(np.arange(24).reshape(3, 2, 4) == 5, np.nan, c.P)):
            with pytest.raises(capi.OsfmError) as e:
                d.set_cameras(P)
            assert e.value.status == capi.E_ARG
        assert _raw(d, c, sw)[0] == capi.OK                           # the cameras that were refused changed nothing
        # a cloud before any fusion, and one that does not fit
        assert capi.lib.osfm_dense_download_cloud(d._h, 0, None, None, None) == capi.E_STATE
        n = C.c_int64(-1)
        assert capi.lib.osfm_dense_fuse(d._h, None, C.byref(n), None) == capi.OK and n.value == 0      # one view: no supporter
        d.set_cameras(c.P)
        n.value = -1
        assert capi.lib.osfm_dense_fuse(d._h, None, C.byref(n), None) == capi.OK and n.value == 0      # nothing swept
        assert capi.lib.osfm_dense_download_cloud(d._h, -1, None, None, None) == capi.E_CAPACITY


def test_memory_returns_after_destroy():
    c = dc.case("odd_sizes")
    before = capi.library_memory().device_buffer_bytes
    d = _handle(c)
    held = capi.library_memory().device_buffer_bytes - before
    assert held >= sum(im.shape[0] * im.shape[1] * 4 for im in c.images)
    _sweep(d, c, c.sweeps[0])
    d.fuse()
    assert capi.library_memory().device_buffer_bytes - before >= held + 13 * c.images[0].shape[0] * c.images[0].shape[1]
    d.close()
    assert capi.library_memory().device_buffer_bytes == before
