"""SURF extraction on the device (osfm_surf_*, orthosfm_amd.features) against the numpy restatement and the
reference fixture, on the seeded cases of tests/surf_cases.py.

Response maps, candidates, localised keypoints, x, y, scale, colours and normalised positions must be equal to the
reference's bytes.  Orientations and descriptors must be equal to the bytes of the restatement run with this
machine's C library (the library takes atan2, sinf and cosf from the same one), and within one quantisation step of
the fixture's.  A keypoint with an orientation sample within a few float ulps of a window bound (`ambiguous`,
surf_restatement.orientation) is counted and left out of the byte comparisons of orientation and descriptor.
The edge cases of surf_cases go through the same parametrised tests; a sweep of every width and height up to 80 on
one context is held to the restatement stage by stage.

On the guard: descriptor_computation's margin is 15 s + 1, its samples lie at x + 0.5, y + 0.5 for x, y in -10 .. 9,
so a corner sample at 45 degrees is 9.5 * sqrt(2) * s = 13.44 s from the centre, a rounded coordinate at most 0.5
further and a tap at most s + 1 beyond that: 14.44 s + 1.5 < 15 s + 1 for every s >= 1.  No tap of a descriptor that
passes the margin test leaves its row, let alone the table, so status 2 cannot occur and the placements on the
margins below are equal to the reference's own results on all four sides."""
import ctypes as C

import numpy as np
import pytest

import sift_cases as sc
import surf_cases as uc
import surf_restatement as sr

pytestmark = pytest.mark.gpu

LIVE = [c.name for c in uc.CASES if not c.upright]
DESCRIBED = ["base", "rgb", "many", "big", "upright", "tie"]
MAX_W, MAX_H = 770, 420


@pytest.fixture(scope="module")
def extractors():
    from orthosfm_amd.features import SurfExtractor
    ex = {False: SurfExtractor(0, MAX_W, MAX_H), True: SurfExtractor(0, MAX_W, MAX_H, use_upright_descriptor=1)}
    long_w, long_h = (max(getattr(uc.BY_NAME[n], k) for n in uc.LONG) for k in ("width", "height"))
    ex["long"] = SurfExtractor(0, long_w, long_h)          # a context of their own for the cases of 1031 rows
    yield ex
    for e in ex.values():
        e.close()


@pytest.fixture(scope="module")
def extracted(extractors):
    """Per case what the device made of it.  Computed once; treat as read-only."""
    out = {}
    for c in uc.CASES:
        ex = extractors["long" if c.name in uc.LONG else c.upright]
        s = ex.run(uc.image(c.name))
        out[c.name] = dict(
            summary=(s.num_candidates, s.num_keypoints, s.num_descriptors, s.num_guarded, list(s.keypoints_per_octave),
                     list(s.descriptors_per_octave)),
            maps=[[ex.debug_image(o, k) for k in range(4)] for o in range(4)],
            cand=ex.debug_keypoints(False), kps=ex.debug_keypoints(True), features=ex.download())
    return out


@pytest.mark.parametrize("name", LIVE)
def test_response_maps_equal_the_restatement(name, extracted):
    maps = uc.restated(name)[1]
    for o in range(4):
        for k in range(4):
            assert extracted[name]["maps"][o][k].shape == maps[o][k].shape
            assert extracted[name]["maps"][o][k].tobytes() == maps[o][k].tobytes(), f"octave {o} sample {k}"
    assert [[sc.sha(m) for m in o] for o in extracted[name]["maps"]] == uc.fixture(name)["map_sha"].astype(str).tolist()


@pytest.mark.parametrize("name", [c.name for c in uc.CASES])
def test_candidates_and_keypoints_equal_the_reference(name, extracted):
    fx, got = uc.fixture(name), extracted[name]
    assert got["cand"].tobytes() == fx["candidates"].tobytes()
    assert got["kps"].tobytes() == fx["keypoints"].tobytes()
    n_cand, n_kp, n_desc, n_guarded, kp_oct, desc_oct = got["summary"]
    assert (n_cand, n_kp, n_desc) == (len(fx["candidates"]), len(fx["keypoints"]), len(fx["gen_meta"]))
    assert n_desc == len(got["features"]) and n_guarded == 0
    assert kp_oct == [int((fx["keypoints"][:, 0] == o).sum()) for o in range(4)]
    assert sum(desc_oct) == n_desc
    want = uc.BY_NAME[name].counts
    if want:
        assert all(w is None or w == g for w, g in zip(want, (n_cand, n_kp, n_desc)))


@pytest.fixture(scope="module")
def sweep_context():
    """One context of 80 x 80 for the whole sweep, and what it made of the 80 x 80 window of `base` before any of it."""
    from orthosfm_amd.features import SurfExtractor
    with SurfExtractor(0, uc.SWEEP_SIDE, uc.SWEEP_SIDE) as ex:
        yield ex, _all_bytes(ex, sc.sweep_cut(uc.SWEEP_SIDE, uc.SWEEP_SIDE, uc.image("base")))


def _device_stage_hashes(ex):
    return uc.stage_hashes([[ex.debug_image(o, k) for k in range(4)] for o in range(4)], ex.debug_keypoints(False),
                           ex.debug_keypoints(True))


@pytest.mark.parametrize("chunk", range(len(uc.SWEEP_CHUNKS)))
def test_sweep_equals_the_restatement(chunk, sweep_context):
    """Every width from 1 to 80 at height 80 and every height from 1 to 80 at width 80 (no size is refused), cut from
    one image, on one context: the 16 response maps, the candidates and the keypoints against the restatement, hashed
    once a side.  This moves w and h across every `x + border >= w`.  The restatement takes 0.5 s for all 159 shapes (one
    CPU core), so the range is not cut."""
    ex = sweep_context[0]
    for w, h in uc.SWEEP_CHUNKS[chunk]:
        ex.run(sc.sweep_cut(w, h))
        got, want = _device_stage_hashes(ex), uc.sweep_restated(w, h)
        assert len(got) == len(want)
        differ = [f"{w} x {h}: {a[0]} / {b[0]}" for a, b in zip(got, want) if a != b]
        assert not differ, differ[:6]


def test_sweep_leaves_nothing_behind(sweep_context):
    """After shapes of every size on the context, the 80 x 80 window of `base` (`base` itself does not fit a context of
    80 x 80) gives its earlier bytes, which are the restatement's: nothing depends on the image that was there before."""
    ex, before = sweep_context
    window = sc.sweep_cut(uc.SWEEP_SIDE, uc.SWEEP_SIDE, uc.image("base"))
    for w, h in ((1, 80), (80, 1), (80, 80), (33, 80)):
        ex.run(sc.sweep_cut(w, h))
        assert _all_bytes(ex, window) == before
    maps = sr.response_maps(sr.integral(window))
    cand = sr.extrema(maps)
    assert _device_stage_hashes(ex) == uc.stage_hashes(maps, cand, sr.localise(maps, cand, uc.SWEEP_SIDE, uc.SWEEP_SIDE))
    assert len(cand) > 0


def test_tied_maxima_are_rejected(extracted):
    """`tie` is its own mirror image about the axis between rows 59 and 60, so the maps of octave 0 are equal in those
    rows and the maximum of a blob on the axis ties with the row beside it.  The reference rejects both rows; a
    neighbour test with > for >= accepts them (the planted restatement: 16 candidates and 4 keypoints more)."""
    fx, got = uc.fixture("tie"), extracted["tie"]
    maps = uc.restated("tie")[1]
    planted = sr.extrema(maps, plant_nonstrict=True)
    tied = sorted(set(map(tuple, planted.tolist())) - set(map(tuple, fx["candidates"].tolist())))
    assert len(tied) == 16 and {r[3] for r in tied} == {59.0, 60.0}
    assert all(got["maps"][0][k][59].tobytes() == got["maps"][0][k][60].tobytes() for k in range(4))
    dev = set(map(tuple, got["cand"].tolist()))
    assert not dev & set(tied)
    assert got["cand"].tobytes() == fx["candidates"].tobytes() != planted.tobytes()
    assert got["kps"].tobytes() == fx["keypoints"].tobytes()


def _sorted_rows(rows):
    """The restatement's descriptors in FeatureSet's order: by scale descending, stably."""
    order = sorted(range(len(rows)), key=lambda i: -float(rows[i]["scale"]))
    return order


@pytest.mark.parametrize("name", DESCRIBED)
def test_orientations_and_descriptors(name, extracted):
    from orthosfm_amd import capi
    fx, f = uc.fixture(name), extracted[name]["features"]
    rows = uc.generation_rows(uc.restated(name)[4])
    assert len(rows) == len(fx["gen_meta"]) == len(f) > 0
    order = _sorted_rows(rows)
    ref_col = np.zeros((len(rows), 3), np.uint8)
    ref_nrm = np.zeros((len(rows), 2), np.float32)
    ref_col[fx["sorted_perm"]] = fx["sorted_colors"]
    ref_nrm[fx["sorted_perm"]] = fx["sorted_normalized"]
    q_dev, q_ref = capi.quantize_surf(f.descriptors), capi.quantize_surf(fx["gen_data"])
    clear = ambiguous = worst_q = 0
    worst_o = 0.0
    for d, g in enumerate(order):
        r = rows[g]
        assert f.positions[d].tobytes() == fx["gen_meta"][g, :2].tobytes()
        assert f.scale[d].tobytes() == fx["gen_meta"][g, 2].tobytes()
        assert f.colors[d].tobytes() == ref_col[g].tobytes()
        assert f.normalized[d].tobytes() == ref_nrm[g].tobytes()
        if r["ambiguous"]:
            ambiguous += 1
            continue
        clear += 1
        assert f.orientation[d].tobytes() == r["orientation"].tobytes(), f"row {g}: orientation"
        assert f.descriptors[d].tobytes() == r["data"].tobytes(), f"row {g}: descriptor"
        worst_o = max(worst_o, abs(float(f.orientation[d]) - float(fx["gen_meta"][g, 3])))
        worst_q = max(worst_q, int(np.abs(q_dev[d].astype(np.int32) - q_ref[g].astype(np.int32)).max()))
    print(f"{name}: {clear} descriptors of clear keypoints equal the restatement's bytes; against the fixture: orientation "
          f"{worst_o:.3e}, quantised {worst_q}; {ambiguous} of ambiguous keypoints left out")
    assert clear > 0 and ambiguous <= uc.MEASURED[name][0]
    assert worst_o <= 1e-6 and worst_q <= 1


@pytest.mark.parametrize("name", DESCRIBED)
def test_order_is_the_feature_sets(name, extracted):
    """By scale descending, and the same rows as the fixture's sorted view inside every group of equal scale."""
    fx, f = uc.fixture(name), extracted[name]["features"]
    assert (np.diff(f.scale) <= 0).all()
    ref = fx["gen_meta"][fx["sorted_perm"]]
    assert ref[:, 2].tobytes() == f.scale.tobytes()
    for s in np.unique(f.scale):
        dev = sorted(p.tobytes() for p in f.positions[f.scale == s])
        assert dev == sorted(p.tobytes() for p in ref[ref[:, 2] == s, :2])


def test_contrast_threshold_reaches_the_kernel():
    from orthosfm_amd.features import SurfExtractor
    _, maps, cand, kps, _ = uc.restated("base")
    strict = sr.localise(maps, cand, 257, 190, 2000.0)
    assert 10 < len(strict) < len(kps)
    with SurfExtractor(0, 257, 190, contrast_threshold=2000.0) as ex:
        s = ex.run(uc.image("base"))
        assert ex.debug_keypoints(False).tobytes() == cand.tobytes()
        assert ex.debug_keypoints(True).tobytes() == strict.tobytes()
        assert s.num_keypoints == len(strict)


def test_upright_differs_from_oriented(extracted):
    a, b = extracted["base"]["features"], extracted["upright"]["features"]
    assert a.positions.tobytes() == b.positions.tobytes() and a.orientation.tobytes() == b.orientation.tobytes()
    assert a.descriptors.tobytes() != b.descriptors.tobytes()
    fx = uc.fixture("upright")                                   # no sine or cosine enters: the reference's bytes
    assert b.descriptors.tobytes() == fx["gen_data"][np.argsort(-fx["gen_meta"][:, 2], kind="stable")].tobytes()


def _all_bytes(ex, image):
    ex.run(image)
    f = ex.download()
    return (f.descriptors.tobytes(), f.positions.tobytes(), f.normalized.tobytes(), f.scale.tobytes(), f.orientation.tobytes(),
            f.colors.tobytes(), ex.debug_keypoints(False).tobytes(), ex.debug_keypoints(True).tobytes())


def test_repeatable(extractors):
    ex = extractors[False]
    assert _all_bytes(ex, uc.image("many")) == _all_bytes(ex, uc.image("many"))
    first = _all_bytes(ex, uc.image("big"))
    _all_bytes(ex, uc.image("tiny"))
    _all_bytes(ex, uc.image("rgb"))
    assert _all_bytes(ex, uc.image("big")) == first


def test_error_paths(extractors):
    from orthosfm_amd import capi
    from orthosfm_amd.features import SurfExtractor
    ex = extractors[False]
    base = uc.image("base")
    want = len(uc.fixture("base")["gen_meta"])

    def refused(ex, image, width, height, channels, status, text):
        s = capi.SurfSummary()
        C.memset(C.byref(s), 0x5A, C.sizeof(s))
        before = bytes(s)
        image = np.ascontiguousarray(image)
        rc = capi.lib.osfm_surf_extract(ex._h, image.ctypes.data, width, height, channels, C.byref(s))
        assert rc == status and text in capi.last_error(), (rc, capi.last_error())
        assert bytes(s) == before                                   # nothing written
        guard = np.full((1024, 64), 7.0, np.float32)                # room for a result that should not be there
        assert capi.lib.osfm_surf_download(ex._h, guard.ctypes.data, None, None, None, None, None) == capi.E_STATE
        assert (guard == 7.0).all()
        out, st = np.zeros(64, np.float32), C.c_int32()
        assert capi.lib.osfm_surf_debug_describe(ex._h, 100.0, 100.0, 2.0, 0.0, 0, out.ctypes.data, C.byref(st)) == capi.E_STATE

    assert ex.run(base).num_descriptors == want
    refused(ex, np.zeros((20, 20, 2), np.uint8), 20, 20, 2, capi.E_ARG, "channels")
    assert ex.run(base).num_descriptors == want
    refused(ex, np.zeros((MAX_H + 1, MAX_W), np.uint8), MAX_W, MAX_H + 1, 1, capi.E_RANGE, "exceeds the context")
    # no size is too small: no features, and a result (of no rows) to download
    for tiny in (uc.image("nothing"), np.full((1, 1), 9, np.uint8), np.full((2, 70), 200, np.uint8)):
        s = ex.run(tiny)
        assert (s.num_candidates, s.num_keypoints, s.num_descriptors) == (0, 0, 0) and len(ex.download()) == 0
    n_cand = len(uc.fixture("base")["candidates"])
    with SurfExtractor(0, 300, 200, max_keypoints=n_cand - 1) as small:
        refused(small, base, base.shape[1], base.shape[0], 1, capi.E_CAPACITY, "candidates exceed max_keypoints")
        assert small.run(uc.image("tiny")).num_candidates == len(uc.fixture("tiny")["candidates"])
    with pytest.raises(capi.OsfmError, match="max_keypoints"):
        SurfExtractor(0, 64, 64, max_keypoints=0)


def test_context_memory_is_booked():
    from orthosfm_amd import capi
    from orthosfm_amd.features import SurfExtractor
    before = capi.library_memory().device_buffer_bytes
    ex = SurfExtractor(0, 256, 256)
    held = capi.library_memory().device_buffer_bytes - before
    assert held >= 256 * 256 * (3 + 4 + 4 * 4)          # pixels, the 32-bit table, four maps of octave 0
    ex.close()
    assert capi.library_memory().device_buffer_bytes == before


def _shift_matches(pos_a, pos_b, m12, m21):
    n = 0
    for i, j in enumerate(m12[:len(pos_a)]):
        if j >= 0 and j < len(pos_b) and m21[j] == i:
            d = pos_a[i] - pos_b[j] - np.array(uc.SHIFT, np.float32)
            n += bool(np.abs(d).max() <= 0.5)
    return n


def test_feature_set_through_the_matcher():
    """Two crops of one canvas that differ by an integer shift, SIFT + SURF from FeatureSetExtractor: the device's
    features must match across the shift as well as the reference's do, less the ambiguous keypoints of the views."""
    from orthosfm_amd.features import FeatureSet, FeatureSetExtractor
    from orthosfm_amd.matching import HipExhaustiveMatching
    names = ("crop_a", "crop_b")
    with FeatureSetExtractor(0, 160, 120) as ex:
        sets = [ex.extract(uc.image(n)) for n in names]
    for n, fs in zip(names, sets):
        assert isinstance(fs, FeatureSet)
        assert fs.surf.descriptors.shape == (len(uc.fixture(n)["gen_meta"]), 64) and len(fs.sift) > 0
        assert fs.positions.shape == (len(fs), 2) and fs.colors.shape == (len(fs), 3)
        assert fs.normalized.tobytes() == fs.sift.normalized.tobytes() + fs.surf.normalized.tobytes()
    counts = {}
    for who in ("device", "reference"):
        m = HipExhaustiveMatching(2, device=0)
        pos = []
        for v, n in enumerate(names):
            if who == "device":
                m.set_view_features(v, sets[v])
                assert m.view_size(v) == (len(sets[v].sift), len(sets[v].surf))
                pos.append(sets[v].positions)
            else:
                a, b = sc.fixture(n), uc.fixture(n)
                m.set_view_float(v, a["gen_data"][a["sorted_perm"]], b["gen_data"][b["sorted_perm"]])
                m.set_positions(v, np.concatenate([a["sorted_normalized"], b["sorted_normalized"]]))
                pos.append(np.concatenate([a["gen_meta"][a["sorted_perm"], :2], b["gen_meta"][b["sorted_perm"], :2]]))
        r = m.pairwise_match(0, 1)
        counts[who] = _shift_matches(pos[0], pos[1], r.matches_1_2, r.matches_2_1)
        m.close()
    ambiguous = sum(sc.MEASURED[n][2] + uc.MEASURED[n][0] for n in names)
    print(f"matches across the shift: device {counts['device']}, reference {counts['reference']}, ambiguous keypoints {ambiguous}")
    assert counts["reference"] >= 5
    assert counts["device"] >= counts["reference"] - ambiguous


def test_hand_placed_descriptors(extractors):
    """descriptor_computation alone on `big` at scales 1, 2, 6 and 13: in the interior, upright, on each of the four
    margins at 45 degrees, and one step outside the margin."""
    ex = extractors[False]
    ex.run(uc.image("big"))
    fx = uc.fixture("big")
    sat = uc.restated("big")[0]
    rows = uc.forced()
    assert len(rows) == len(uc.FORCED_SCALES) * len(uc.FORCED_KINDS)
    for i, (x, y, scale, ori, upright) in enumerate(rows):
        kind = uc.FORCED_KINDS[i % len(uc.FORCED_KINDS)]
        got, status = ex.debug_describe(x, y, scale, ori, bool(upright))
        s, c = (np.float32(0), np.float32(1)) if upright else (sr.sinf(ori), sr.cosf(ori))
        want_status, want, _ = sr.describe(sat, x, y, scale, s, c)
        assert status == want_status == int(fx["forced_ok"][i]) == (0 if kind == "rejected" else 1), (i, kind)
        assert got.tobytes() == want.tobytes(), (i, kind)
        if status and (s.tobytes(), c.tobytes()) == (fx["forced_trig"][i, 0].tobytes(), fx["forced_trig"][i, 1].tobytes()):
            assert got.tobytes() == fx["forced_data"][i].tobytes(), (i, kind)
    # the hook leaves the extraction's own result alone
    assert len(ex.download()) == len(fx["gen_meta"])
    # a scale whose products would leave int is refused, as is one below 1 or none at all
    from orthosfm_amd import capi
    for bad in (0.5, 65.0, 3e9, float("inf"), float("nan")):
        with pytest.raises(capi.OsfmError, match="scale"):
            ex.debug_describe(224.3, 208.6, bad, 0.7)


def test_modular_table_wraps_harmlessly():
    """A 4112 x 4112 image of 255s sums to more than 2^32: inside `base` pasted at its bottom-right corner the maps
    still equal the restatement of a small window (box sums do not depend on where the window lies)."""
    from orthosfm_amd.features import SurfExtractor
    n, base = 4112, uc.image("base")
    bh, bw = base.shape
    img = np.full((n, n), 255, np.uint8)
    img[n - bh:, n - bw:] = base
    assert int(img.sum(dtype=np.int64)) > 2 ** 32
    x0, y0 = (n - bw) // 8 * 8, (n - bh) // 8 * 8           # a window whose origin lies on every octave's grid
    sat = sr.integral(img[y0:, x0:])
    with SurfExtractor(0, n, n) as ex:
        ex.run(img)
        for o, k in ((0, 1), (3, 2)):
            want = sr.response_map(sat, o, k)
            got = ex.debug_image(o, k)[y0 >> o:, x0 >> o:]
            assert got.shape == want.shape
            border = sr.filter_size(o, k) + sr.filter_size(o, k) // 2 + 1
            lo = -(-border >> o)                              # first sample whose filter lies inside the window
            assert want[lo:, lo:].any()
            assert got[lo:, lo:].tobytes() == want[lo:, lo:].tobytes(), (o, k)
