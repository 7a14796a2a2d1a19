"""The observation refinement on the device against tests/refine_restatement.py, through the C ABI, on every case of
tests/refine_cases.py: statuses and iteration counts outside the ambiguous observations, the refined values within
refine_cases.BOUNDS, everything else bit for bit; repeatability, independence of the order of the tracks, the
hand-over from a view front end, the error codes and the memory ledger."""
import ctypes as C

import numpy as np
import pytest

import refine_cases as rc
import refine_restatement as rr
from orthosfm_amd import capi
from orthosfm_amd.features import ViewFrontEnd
from orthosfm_amd.refine import Refiner

pytestmark = pytest.mark.gpu


def _refiner(c):
    r = Refiner(0, len(c.images))
    for v, im in enumerate(c.images):
        r.set_image(v, im)
    return r


def _run(r, c, **over):
    kw = dict(offsets=c.offsets, view=c.view, xy=c.xy, alive=c.alive, init_affine=c.init_affine, **c.options)
    kw.update(over)
    return r.refine(**kw)


_results = {}


def device(name):
    """The device's result on a case: computed once, shared."""
    if name not in _results:
        c = rc.case(name)
        with _refiner(c) as r:
            _results[name] = _run(r, c)
    return _results[name]


def _bytes(res):
    return b"".join(a.tobytes() for a in (res.xy, res.affine, res.score, res.status, res.iterations))


@pytest.mark.parametrize("name", rc.NAMES)
def test_status_and_iterations(name):
    c, want, got = rc.case(name), rc.restated(name), device(name)
    clear = ~rc.ambiguous(want)
    assert np.array_equal(got.status[clear], want["status"][clear]), \
        [(int(f), rr.STATUS_NAMES[got.status[f]], rr.STATUS_NAMES[want["status"][f]])
         for f in np.flatnonzero(clear & (got.status != want["status"]))]
    assert np.array_equal(got.iterations[clear], want["iterations"][clear])
    if name == "border":
        # the windows that touch the bounds exactly: integer arithmetic, not a close decision
        for k in ("touch", "touch_origin"):
            assert got.status[c.paths[k]] == rr.REFINED, k
    counts = got.stats.counters()
    for i, key in enumerate(capi.REFINE_STATUS):
        assert counts[key] == int((got.status == i).sum()), key
    assert counts["iterations"] == int(got.iterations.sum())
    assert sum(counts[k] for k in capi.REFINE_STATUS) == c.num_obs


@pytest.mark.parametrize("name", rc.NAMES)
def test_values(name):
    c, want, got = rc.case(name), rc.restated(name), device(name)
    both = (got.status == rr.REFINED) & (want["status"] == rr.REFINED)
    d_xy = float(np.abs(got.xy[both] - want["xy"][both]).max()) if both.any() else 0.0
    d_aff = float(np.abs(got.affine[both] - want["affine"][both]).max()) if both.any() else 0.0
    d_score = float(np.abs(got.score[both] - want["score"][both]).max()) if both.any() else 0.0
    print(f"{name}: {int(both.sum())} refined, max |d xy| {d_xy:.3e} px, |d affine| {d_aff:.3e}, |d score| {d_score:.3e}")
    assert d_xy <= rc.BOUNDS["xy"] and d_aff <= rc.BOUNDS["affine"] and d_score <= rc.BOUNDS["score"]
    # every other observation returns its input position and warp, bit for bit
    other = got.status != rr.REFINED
    assert got.xy[other].tobytes() == np.ascontiguousarray(c.xy[other], dtype=np.float64).tobytes()
    a0 = np.tile([1.0, 0.0, 0.0, 1.0], (c.num_obs, 1)) if c.init_affine is None else c.init_affine
    assert got.affine[other].tobytes() == np.ascontiguousarray(a0[other], dtype=np.float64).tobytes()


@pytest.mark.parametrize("name", ["base", "lengths", "mismatch", "radius15"])
def test_repeats_and_follows_a_permutation(name):
    c, first = rc.case(name), device(name)
    T = c.offsets.shape[0] - 1
    perm = np.argsort(rc._u(99, 9, T), kind="stable")
    obs = np.concatenate([np.arange(c.offsets[t], c.offsets[t + 1]) for t in perm])
    offsets = np.concatenate([[0], np.cumsum(np.diff(c.offsets)[perm])]).astype(np.int64)
    with _refiner(c) as r:
        again = _run(r, c)
        moved = _run(r, c, offsets=offsets, view=c.view[obs], xy=c.xy[obs], alive=None if c.alive is None else c.alive[obs],
                     init_affine=None if c.init_affine is None else c.init_affine[obs])
    assert _bytes(again) == _bytes(first)
    for a, b in ((moved.xy, first.xy), (moved.affine, first.affine), (moved.score, first.score), (moved.status, first.status),
                 (moved.iterations, first.iterations)):
        assert a.tobytes() == b[obs].tobytes()


def test_image_from_front_equals_upload():
    """set_image_from_front gives what set_image gives on debug_image()'s bytes; the front end halves once, so the
    feature image is not the input."""
    c = rc.case("rgb_sizes")
    with ViewFrontEnd(0, 160, 128, max_image_size=6000) as front, Refiner(0, 3) as a, Refiner(0, 3) as b:
        sizes = []
        for v, im in enumerate(c.images):
            s = front.load(im)
            assert s.num_halvings == 1
            a.set_image_from_front(v, front)
            shown = front.debug_image()
            assert shown.shape[:2] == (s.feature_height, s.feature_width)
            b.set_image(v, shown)
            sizes.append((s.feature_width, s.feature_height))
        xy = (c.xy - 0.5) / 2.0                      # roughly where the halved image shows the same structures
        ra = a.refine(c.offsets, c.view, xy, radius=4)
        rb = b.refine(c.offsets, c.view, xy, radius=4)
    assert _bytes(ra) == _bytes(rb)
    assert (ra.status == rr.REFINED).any()


def _raw(r, c, view=None, xy=None, options=None):
    """osfm_refine_tracks with outputs full of a sentinel; returns (status code, outputs untouched)."""
    F = c.num_obs
    view = np.ascontiguousarray(c.view if view is None else view, dtype=np.int32)
    xy = np.ascontiguousarray(c.xy if xy is None else xy, dtype=np.float64)
    outs = [np.full((F, 2), 7.5), np.full((F, 4), 7.5), np.full(F, 7.5), np.full(F, 77, np.int32), np.full(F, 77, np.int32)]
    before = [o.copy() for o in outs]
    stats = capi.RefineStats()
    stats.iterations = 77
    o = capi.default_refine_options(**(options or {}))
    rcode = capi.lib.osfm_refine_tracks(r._h, c.offsets.shape[0] - 1, c.offsets.ctypes.data, view.ctypes.data, xy.ctypes.data, None,
                                        None, C.byref(o), *[a.ctypes.data for a in outs], C.byref(stats))
    return rcode, all(np.array_equal(a, b) for a, b in zip(outs, before)) and stats.iterations == 77


def test_error_codes_write_nothing():
    c = rc.case("radius7")
    with Refiner(0, 3) as r:
        r.set_image(0, c.images[0])
        assert _raw(r, c) == (capi.E_STATE, True)                 # view 1 has no image yet
        r.set_image(1, c.images[1])
        assert _raw(r, c)[0] == capi.OK
        bad_view = c.view.copy()
        bad_view[3] = 3
        assert _raw(r, c, view=bad_view) == (capi.E_RANGE, True)
        bad_view[3] = -1
        assert _raw(r, c, view=bad_view) == (capi.E_RANGE, True)
        for options in (dict(radius=1), dict(radius=16), dict(step=0.0), dict(max_iterations=0), dict(max_deform=0.5)):
            assert _raw(r, c, options=options) == (capi.E_ARG, True), options
        for bad in (np.nan, np.inf):
            xy = c.xy.copy()
            xy[5, 1] = bad
            assert _raw(r, c, xy=xy) == (capi.E_ARG, True)
        with pytest.raises(capi.OsfmError) as e:
            r.set_image(3, c.images[0])
        assert e.value.status == capi.E_RANGE


def test_memory_returns_after_destroy():
    c = rc.case("rgb_sizes")
    before = capi.library_memory().device_buffer_bytes
    r = _refiner(c)
    held = capi.library_memory().device_buffer_bytes - before
    assert held >= sum(im.shape[0] * im.shape[1] * 4 for im in c.images)
    _run(r, c)
    r.close()
    assert capi.library_memory().device_buffer_bytes == before
