"""SIFT extraction on the device (osfm_sift_*, orthosfm_amd.features) against the numpy restatement and the
reference fixture, on the seeded cases of tests/sift_cases.py.

Scale space, candidates and localised keypoints must be equal to the reference's bytes.  Orientations and
descriptors are held to four times the measured distance between the reference and the float64 restatement
(sift_cases.MEASURED): two independent float32 sums, each as far from the exact value as the reference's own, times
two for the order of the reduction tree.  Keypoints with a peak decision inside the ambiguity band may differ in
their number of orientations and are only counted.

The cases of sift_cases.EDGE_CASES go through the same parametrised tests; a sweep of every accepted width and height
up to 80 on one context is held to the restatement stage by stage."""
import ctypes as C

import numpy as np
import pytest

import sift_cases as sc
import sift_restatement as sr

pytestmark = pytest.mark.gpu

LIVE = [c.name for c in sc.CASES if not c.refused]
DESCRIBED = ["base", "up", "rgb", "many"]
MAX_W, MAX_H = 520, 320


@pytest.fixture(scope="module")
def extractors():
    from orthosfm_amd.features import SiftExtractor
    ex = {0: SiftExtractor(0, MAX_W, MAX_H), -1: SiftExtractor(0, MAX_W, MAX_H, min_octave=-1)}
    r32 = sc.BY_NAME["r32"]           # one sample per octave: a blur radius of kMaxRadius = 32
    ex["r32"] = SiftExtractor(0, r32.width, r32.height, num_samples_per_octave=r32.samples, base_blur_sigma=r32.base_blur_sigma)
    yield ex
    for e in ex.values():
        e.close()


@pytest.fixture(scope="module")
def extracted(extractors):
    """Per live case what the device made of it: summary numbers, every octave and DoG image, candidates,
    keypoints and the downloaded features.  Computed once; treat as read-only."""
    out = {}
    for name in LIVE:
        c = sc.BY_NAME[name]
        ex = extractors["r32" if name == "r32" else c.min_octave]
        s = ex.run(sc.image(name))
        n_oct = s.num_octaves
        out[name] = dict(
            summary=(s.num_candidates, s.num_keypoints, s.num_descriptors, n_oct, list(s.keypoints_per_octave)[:n_oct]),
            img=[[ex.debug_image(c.min_octave + o, 0, i) for i in range(c.samples + 3)] for o in range(n_oct)],
            dog=[[ex.debug_image(c.min_octave + o, 1, i) for i in range(c.samples + 2)] for o in range(n_oct)],
            cand=ex.debug_keypoints(False), kps=ex.debug_keypoints(True), features=ex.download())
    return out


@pytest.mark.parametrize("name", LIVE)
def test_scale_space_equals_the_restatement(name, extracted):
    octs = sc.restated(name)[0]
    got = extracted[name]
    assert len(got["img"]) == len(octs)
    for o, (_, imgs, dogs) in enumerate(octs):
        for i, ref in enumerate(imgs):
            assert got["img"][o][i].shape == ref.shape
            assert got["img"][o][i].tobytes() == ref.tobytes(), f"octave {o} image {i}"
        for i, ref in enumerate(dogs):
            assert got["dog"][o][i].tobytes() == ref.tobytes(), f"octave {o} DoG {i}"
    # the restatement takes expf from this machine's C library; where these hashes differ from the fixture's, that
    # library rounds expf differently from the one the fixture was made with (the comparison above still stands)
    fx = sc.fixture(name)
    assert [[sc.sha(i) for i in o[1]] for o in octs] == fx["img_sha"].astype(str).tolist()
    assert [[sc.sha(i) for i in o[2]] for o in octs] == fx["dog_sha"].astype(str).tolist()


@pytest.mark.parametrize("name", LIVE)
def test_candidates_and_keypoints_equal_the_reference(name, extracted):
    fx, got = sc.fixture(name), extracted[name]
    assert got["cand"].tobytes() == fx["candidates"].tobytes()
    assert got["kps"].tobytes() == fx["keypoints"].tobytes()
    n_cand, n_kp, n_desc, n_oct, per_octave = got["summary"]
    assert (n_cand, n_kp) == (len(fx["candidates"]), len(fx["keypoints"]))
    assert n_desc == len(got["features"])
    mo = sc.BY_NAME[name].min_octave
    assert per_octave == [int((fx["keypoints"][:, 0] == mo + o).sum()) for o in range(n_oct)]


def test_the_largest_blur_radius(extracted):
    """`r32`: one sample per octave at the default base blur needs a radius of 32, which fills both LDS tiles of the
    blur kernels to their last element; the scale space equals the restatement's (the parametrised tests above hold it
    to the fixture).  One hundredth more sigma needs 33 and is refused."""
    from orthosfm_amd import capi
    from orthosfm_amd.features import SiftExtractor
    c = sc.BY_NAME["r32"]
    assert sr.blur_radii(sc.options(c)) == [8, 16, 32]
    octs, cand, kps = sc.restated("r32")[:3]
    got = extracted["r32"]
    assert sc.stage_hashes(got["img"], got["dog"], got["cand"], got["kps"]) == \
        sc.stage_hashes([o[1] for o in octs], [o[2] for o in octs], cand, kps)
    assert len(got["img"]) == 5 and len(got["img"][0]) == 4 and len(got["cand"]) > 0
    with pytest.raises(capi.OsfmError, match="blur radius of 33, the kernels hold 32") as e:
        SiftExtractor(0, c.width, c.height, num_samples_per_octave=1, base_blur_sigma=sc.RADIUS_REFUSED_SIGMA)
    assert e.value.status == capi.E_ARG


@pytest.fixture(scope="module")
def sweep_context():
    """One context of 80 x 80 for the whole sweep, and what it made of the 80 x 80 window of `base` before any of it."""
    from orthosfm_amd.features import SiftExtractor
    with SiftExtractor(0, sc.SWEEP_SIDE, sc.SWEEP_SIDE) as ex:
        yield ex, _all_bytes(ex, sc.sweep_cut(sc.SWEEP_SIDE, sc.SWEEP_SIDE, sc.image("base")))


def _device_stage_hashes(ex):
    n_oct = 5
    return sc.stage_hashes([[ex.debug_image(o, 0, i) for i in range(6)] for o in range(n_oct)],
                           [[ex.debug_image(o, 1, i) for i in range(5)] for o in range(n_oct)],
                           ex.debug_keypoints(False), ex.debug_keypoints(True))


@pytest.mark.parametrize("chunk", range(len(sc.SWEEP_CHUNKS)))
def test_sweep_equals_the_restatement(chunk, sweep_context):
    """Every width from 17 to 80 at height 80 and every height from 17 to 80 at width 80, cut from one image, on one
    context: every scale-space and DoG image, the candidates and the keypoints against the restatement, hashed once a
    side.  The restatement takes 1.3 s for all 127 shapes (one CPU core), so the range is not cut."""
    ex = sweep_context[0]
    for w, h in sc.SWEEP_CHUNKS[chunk]:
        assert ex.run(sc.sweep_cut(w, h)).num_octaves == 5
        got, want = _device_stage_hashes(ex), sc.sweep_restated(w, h)
        assert len(got) == len(want)
        differ = [f"{w} x {h}: {stage}" for (stage, a), (_, b) in zip(got, want) if a != b]
        assert not differ, differ[:6]


def test_sweep_leaves_nothing_behind(sweep_context):
    """After shapes of every size on the context, the 80 x 80 window of `base` (`base` itself does not fit a context of
    80 x 80) gives its earlier bytes, which are the restatement's: nothing depends on the image that was there before."""
    ex, before = sweep_context
    window = sc.sweep_cut(sc.SWEEP_SIDE, sc.SWEEP_SIDE, sc.image("base"))
    for w, h in ((17, 80), (80, 17), (80, 80), (33, 80)):
        ex.run(sc.sweep_cut(w, h))
        assert _all_bytes(ex, window) == before
    octs = sr.scale_space(window, sr.Options())
    cand = sr.extrema(octs)
    assert _device_stage_hashes(ex) == sc.stage_hashes([o[1] for o in octs], [o[2] for o in octs], cand,
                                                       sr.localise(octs, cand, sr.Options())[0])
    assert len(cand) > 0


def test_options_reach_the_kernels():
    """Other Sift::Options than the defaults: scale space and keypoints still equal the restatement's."""
    from orthosfm_amd.features import SiftExtractor
    f32 = np.float32
    opts = sr.Options(num_samples_per_octave=2, max_octave=3, base_blur_sigma=f32(1.4), inherent_blur_sigma=f32(0.6),
                      edge_ratio_threshold=f32(8.0), contrast_threshold=f32(0.005))
    octs = sr.scale_space(sc.image("rgb"), opts)
    cand = sr.extrema(octs)
    kps = sr.localise(octs, cand, opts)[0]
    assert len(kps) > 10 and len(kps) < len(cand)
    with SiftExtractor(0, 200, 150, num_samples_per_octave=2, max_octave=3, base_blur_sigma=1.4, inherent_blur_sigma=0.6,
                       edge_ratio_threshold=8.0, contrast_threshold=0.005) as ex:
        s = ex.run(sc.image("rgb"))
        assert s.num_octaves == len(octs) == 4
        for o, (_, imgs, dogs) in enumerate(octs):
            assert [ex.debug_image(o, 0, i).tobytes() for i in range(5)] == [i.tobytes() for i in imgs]
            assert [ex.debug_image(o, 1, i).tobytes() for i in range(4)] == [d.tobytes() for d in dogs]
        assert ex.debug_keypoints(False).tobytes() == cand.tobytes()
        assert ex.debug_keypoints(True).tobytes() == kps.tobytes()


def _rows_by_keypoint(name, f):
    """Per keypoint of the fixture the rows of the downloaded features that belong to it, in generation order: x, y
    and scale are exact functions of the keypoint, and the sort by scale is stable."""
    c = sc.BY_NAME[name]
    opts = sr.Options(min_octave=c.min_octave)
    rows = {}
    for i in range(len(f)):
        rows.setdefault((f.positions[i].tobytes(), f.scale[i].tobytes()), []).append(i)
    out = []
    for kp in sc.fixture(name)["keypoints"]:
        x, y, s, _ = sr.generation_meta(kp, 0.0, opts)
        out.append(rows.pop((np.array([x, y], np.float32).tobytes(), np.float32(s).tobytes()), []))
    assert not rows, "features at positions that belong to no keypoint of the reference"
    return out


@pytest.mark.parametrize("name", DESCRIBED)
def test_orientations_and_descriptors(name, extracted):
    from orthosfm_amd import capi
    c, fx, f = sc.BY_NAME[name], sc.fixture(name), extracted[name]["features"]
    d_ori, d_desc, _, _ = sc.MEASURED[name]
    assert 4.0 * d_desc < 1.0 / 510.0
    clear = sc.measure(name)["clear"]
    ref_rows = sc.groups_of(fx["keypoints"], fx["gen_meta"], c.min_octave)
    dev_rows = _rows_by_keypoint(name, f)
    # the reference's colours and normalised positions by generation row
    ref_col = np.zeros((len(fx["gen_meta"]), 3), np.uint8)
    ref_nrm = np.zeros((len(fx["gen_meta"]), 2), np.float32)
    ref_col[fx["sorted_perm"]] = fx["sorted_colors"]
    ref_nrm[fx["sorted_perm"]] = fx["sorted_normalized"]
    q_dev, q_ref = capi.quantize_sift(f.descriptors), capi.quantize_sift(fx["gen_data"])
    worst_o = worst_d = 0.0
    worst_q = ambiguous = ambiguous_differ = compared = 0
    for k, (rr, dr) in enumerate(zip(ref_rows, dev_rows)):
        if not clear[k]:
            ambiguous += 1
            ambiguous_differ += len(rr) != len(dr)
            continue
        assert len(rr) == len(dr), f"keypoint {k}: {len(dr)} orientations, the reference has {len(rr)}"
        for r, d in zip(rr, dr):
            compared += 1
            assert f.positions[d].tobytes() == fx["gen_meta"][r, :2].tobytes()
            assert f.scale[d].tobytes() == fx["gen_meta"][r, 2].tobytes()
            assert f.colors[d].tobytes() == ref_col[r].tobytes()
            assert f.normalized[d].tobytes() == ref_nrm[r].tobytes()
            worst_o = max(worst_o, abs(float(f.orientation[d]) - float(fx["gen_meta"][r, 3])))
            worst_d = max(worst_d, float(np.abs(f.descriptors[d].astype(np.float64) - fx["gen_data"][r]).max()))
            worst_q = max(worst_q, int(np.abs(q_dev[d].astype(np.int32) - q_ref[r].astype(np.int32)).max()))
    print(f"{name}: {compared} descriptors of clear keypoints, largest orientation difference {worst_o:.3e} "
          f"(bound {4 * d_ori:.3e}), largest element difference {worst_d:.3e} (bound {4 * d_desc:.3e}), quantised {worst_q}; "
          f"{ambiguous} ambiguous keypoints, {ambiguous_differ} of them with another number of orientations")
    assert compared > 0
    assert worst_o <= 4.0 * d_ori
    assert worst_d <= 4.0 * d_desc
    assert worst_q <= 1


@pytest.mark.parametrize("name", DESCRIBED)
def test_order_is_the_feature_sets(name, extracted):
    """By scale descending; the same rows as the fixture's sorted view up to permutations inside groups of equal
    scale (rows of ambiguous keypoints, whose number may differ, left out on both sides)."""
    c, fx, f = sc.BY_NAME[name], sc.fixture(name), extracted[name]["features"]
    assert (np.diff(f.scale) <= 0).all()
    clear = sc.measure(name)["clear"]
    keep_ref = {r for k, rr in enumerate(sc.groups_of(fx["keypoints"], fx["gen_meta"], c.min_octave)) if clear[k] for r in rr}
    keep_dev = {d for k, dr in enumerate(_rows_by_keypoint(name, f)) if clear[k] for d in dr}
    ref = [fx["gen_meta"][r, :3].tobytes() for r in fx["sorted_perm"] if r in keep_ref]
    dev = [np.concatenate([f.positions[d], f.scale[d:d + 1]]).tobytes() for d in range(len(f)) if d in keep_dev]
    assert sorted(ref) == sorted(dev)
    ref_scale = [float(fx["gen_meta"][r, 2]) for r in fx["sorted_perm"] if r in keep_ref]
    dev_scale = [float(f.scale[d]) for d in range(len(f)) if d in keep_dev]
    assert ref_scale == dev_scale


def _all_bytes(ex, image):
    ex.run(image)
    f = ex.download()
    return (f.descriptors.tobytes(), f.positions.tobytes(), f.normalized.tobytes(), f.scale.tobytes(), f.orientation.tobytes(),
            f.colors.tobytes(), ex.debug_keypoints(False).tobytes(), ex.debug_keypoints(True).tobytes())


def test_repeatable(extractors):
    ex = extractors[0]
    assert _all_bytes(ex, sc.image("many")) == _all_bytes(ex, sc.image("many"))
    first = _all_bytes(ex, sc.image("base"))
    _all_bytes(ex, sc.image("tiny"))
    assert _all_bytes(ex, sc.image("base")) == first


def test_error_paths(extractors):
    from orthosfm_amd import capi
    from orthosfm_amd.features import SiftExtractor
    ex = extractors[0]
    base = sc.image("base")
    want = len(sc.fixture("base")["gen_meta"])

    def refused(ex, image, width, height, channels, status, text):
        s = capi.SiftSummary()
        C.memset(C.byref(s), 0x5A, C.sizeof(s))
        before = bytes(s)
        image = np.ascontiguousarray(image)
        rc = capi.lib.osfm_sift_extract(ex._h, image.ctypes.data, width, height, channels, C.byref(s))
        assert rc == status and text in capi.last_error(), (rc, capi.last_error())
        assert bytes(s) == before                                   # nothing written
        guard = np.full((1024, 128), 7.0, np.float32)               # room for a result that should not be there
        assert capi.lib.osfm_sift_download(ex._h, guard.ctypes.data, None, None, None, None, None) == capi.E_STATE
        assert (guard == 7.0).all()

    refused(ex, sc.image("refused"), 9, 9, 1, capi.E_ARG, "too small")
    for name in (c.name for c in sc.CASES if c.refused and c.name in sc.EDGE):        # 16 pixels a side, per dimension
        c = sc.BY_NAME[name]
        refused(ex, sc.image(name), c.width, c.height, 1, capi.E_ARG, "too small")
        assert ex.run(base).num_descriptors >= want - 2
    assert ex.run(base).num_descriptors >= want - 2
    refused(ex, np.zeros((20, 20, 2), np.uint8), 20, 20, 2, capi.E_ARG, "channels")
    assert ex.run(base).num_descriptors >= want - 2
    refused(ex, np.zeros((MAX_H + 1, MAX_W), np.uint8), MAX_W, MAX_H + 1, 1, capi.E_RANGE, "exceeds the context")
    assert ex.run(base).num_descriptors >= want - 2
    with pytest.raises(capi.OsfmError, match="min_octave"):
        SiftExtractor(0, 64, 64, min_octave=1)
    n_cand = len(sc.fixture("base")["candidates"])
    with SiftExtractor(0, 300, 200, max_keypoints=n_cand - 1) as small:
        refused(small, base, base.shape[1], base.shape[0], 1, capi.E_CAPACITY, "candidates exceed max_keypoints")
        assert small.run(sc.image("tiny")).num_candidates == len(sc.fixture("tiny")["candidates"])


def test_context_memory_is_booked():
    from orthosfm_amd import capi
    from orthosfm_amd.features import SiftExtractor
    before = capi.library_memory().device_buffer_bytes
    ex = SiftExtractor(0, 256, 256)
    held = capi.library_memory().device_buffer_bytes - before
    assert held >= 256 * 256 * 4 * 11
    ex.close()
    assert capi.library_memory().device_buffer_bytes == before


def _shift_matches(pos_a, pos_b, m12, m21):
    n = 0
    for i, j in enumerate(m12[:len(pos_a)]):
        if j >= 0 and j < len(pos_b) and m21[j] == i:
            d = pos_a[i] - pos_b[j] - np.array(sc.SHIFT, np.float32)
            n += bool(np.abs(d).max() <= 0.5)
    return n


def test_through_the_matcher(extracted):
    """Two crops of one canvas that differ by an integer shift: the device's features must match across the shift
    as well as the reference's do, less the ambiguous keypoints of the two views."""
    from orthosfm_amd.matching import HipExhaustiveMatching
    counts = {}
    for who in ("device", "reference"):
        m = HipExhaustiveMatching(2, device=0)
        pos = []
        for v, name in enumerate(("crop_a", "crop_b")):
            if who == "device":
                f = extracted[name]["features"]
                m.set_view_features(v, f)
                pos.append(f.positions)
            else:
                fx = sc.fixture(name)
                m.set_view_float(v, fx["gen_data"][fx["sorted_perm"]], np.zeros((0, 64), np.float32))
                m.set_positions(v, fx["sorted_normalized"])
                pos.append(fx["gen_meta"][fx["sorted_perm"], :2])
        r = m.pairwise_match(0, 1)
        counts[who] = _shift_matches(pos[0], pos[1], r.matches_1_2, r.matches_2_1)
        m.close()
    ambiguous = sc.MEASURED["crop_a"][2] + sc.MEASURED["crop_b"][2]
    print(f"matches across the shift: device {counts['device']}, reference {counts['reference']}, ambiguous keypoints {ambiguous}")
    assert counts["reference"] >= 5
    assert counts["device"] >= counts["reference"] - ambiguous


def test_python_front():
    from orthosfm_amd.features import Features, SiftExtractor
    with SiftExtractor(0, 200, 150) as ex:
        f = ex.extract(sc.image("rgb"))
    assert isinstance(f, Features)
    n = len(f)
    assert n >= len(sc.fixture("rgb")["gen_meta"]) - 2 and n > 0
    assert (f.descriptors.shape, f.descriptors.dtype) == ((n, 128), np.float32)
    assert (f.positions.shape, f.positions.dtype) == ((n, 2), np.float32)
    assert (f.normalized.shape, f.normalized.dtype) == ((n, 2), np.float32)
    assert (f.scale.shape, f.scale.dtype) == ((n,), np.float32)
    assert (f.orientation.shape, f.orientation.dtype) == ((n,), np.float32)
    assert (f.colors.shape, f.colors.dtype) == ((n, 3), np.uint8)
    assert np.allclose(np.linalg.norm(f.descriptors, axis=1), 1.0, atol=1e-5)
