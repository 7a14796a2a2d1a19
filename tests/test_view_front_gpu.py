"""The view front end (include/osfm_hip.h, "View front end") on the device: the halving chain against the reference's
bytes, the hand-off kernels against the host path byte for byte on values on every rounding boundary, the front end
against FeatureSetExtractor + set_view_features on the seeded detector cases, matching through it, the ordering of
a load behind a hand-off, and the error paths.  Cases and the chain's restatement: tests/view_cases.py."""
import numpy as np
import pytest

import sift_cases as sc
import surf_cases as uc
import view_cases as vc

pytestmark = pytest.mark.gpu

FEATURE_CASES = ("base", "rgb", "many")         # of sift_cases and of surf_cases: one image for both detectors


def _same_bank(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
            assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k] != b[k]).sum()), "elements differ")
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _same_features(a, b, what):
    for part in ("sift", "surf"):
        fa, fb = getattr(a, part), getattr(b, part)
        for k in ("descriptors", "positions", "normalized", "scale", "orientation", "colors"):
            x, y = getattr(fa, k), getattr(fb, k)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, part, k)
    for k in ("positions", "normalized", "colors"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)


@pytest.fixture(scope="module")
def matcher():
    from orthosfm_amd.matching import HipExhaustiveMatching
    m = HipExhaustiveMatching(2, device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def old_path():
    """name, halved -> (FeatureSet of FeatureSetExtractor on the restated image, that image): computed once, read-only."""
    from orthosfm_amd.features import FeatureSetExtractor
    out = {}
    assert all(uc.image(n) is sc.image(n) for n in FEATURE_CASES)
    with FeatureSetExtractor(0, 401, 299) as ex:
        for name in FEATURE_CASES + ("crop_a", "crop_b"):
            for halved in (False, True):
                img = sc.image(name)
                if halved:
                    img = vc.halve(img)
                out[name, halved] = (ex.extract(img), img)
    return out


# ---- 1. halving -------------------------------------------------------------------------------------------------
def test_halving_equals_the_reference():
    """One halving of every image of the fixture (max_image_size one below the image's size); SURF alone, which
    takes every size."""
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    for name, img in vc.halve_images().items():
        h, w = img.shape[:2]
        with ViewFrontEnd(0, w, h, max_image_size=w * h - 1, feature_types=capi.FEATURE_SURF) as front:
            s = front.load(img)
            got, want = front.debug_image(), vc.golden()[name]
            assert (s.num_halvings, s.feature_width, s.feature_height) == (1, want.shape[1], want.shape[0]), name
            assert (s.import_width, s.import_height) == (w, h)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), name


def test_chains_equal_the_restatement():
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    img = vc.halve_images()["random_65x63x3"]
    for kw in ({"max_image_size": 1000}, {"downscale_factor": 3, "max_image_size": 0}, {"downscale_factor": 2, "max_image_size": 1000},
               {"max_image_size": -1}):
        imported, feat, n = vc.chain(img, **kw)
        with ViewFrontEnd(0, 65, 63, feature_types=capi.FEATURE_SURF, **kw) as front:
            s = front.load(img)
            assert s.num_halvings == n and (s.import_width, s.import_height) == (imported.shape[1], imported.shape[0]), kw
            assert front.debug_image().tobytes() == feat.tobytes() and front.debug_image().shape == feat.shape, kw
    # a grey chain of two halvings, 64 wide, then 32: the 8-byte path both times (32 is a multiple of 8 as well)
    grey = vc.halve_images()["patches_64x64x1"]
    assert vc.takes_grey8(64, 1) and vc.takes_grey8(32, 1)
    with ViewFrontEnd(0, 64, 64, downscale_factor=3, max_image_size=0, feature_types=capi.FEATURE_SURF) as front:
        front.load(grey)
        assert front.debug_image().tobytes() == vc.chain(grey, 3, 0)[1].tobytes()


@pytest.mark.parametrize("chain", vc.HALVE_CHAINS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_grey_chains_equal_the_reference_at_every_step(chain):
    """Chains in which the 8-byte kernel is followed by the general one, follows it, and is not taken at all: every
    step (a front end that stops there) against the reference halving its own last result."""
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    w, h, n = chain
    img = vc.chain_images()[chain]
    for step in range(1, n + 1):
        want = vc.golden()[vc.chain_name(w, h, step)]
        with ViewFrontEnd(0, w, h, downscale_factor=step + 1, max_image_size=0, feature_types=capi.FEATURE_SURF) as front:
            s = front.load(img)
            got = front.debug_image()
            assert (s.num_halvings, s.feature_width, s.feature_height) == (step, want.shape[1], want.shape[0]), step
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), step


# ---- 2. hand-off kernels on hostile values ----------------------------------------------------------------------
@pytest.mark.parametrize("pattern", vc.SPECIAL_PATTERNS)
@pytest.mark.parametrize("index", range(len(vc.ROW_COUNTS)))
def test_handoff_equals_the_host_path(index, pattern, matcher):
    n_sift, n_surf = vc.ROW_COUNTS[index], vc.ROW_COUNTS[::-1][(index + vc.SPECIAL_PATTERNS.index(pattern)) % len(vc.ROW_COUNTS)]
    sift, surf, pos = vc.bank_case(n_sift, n_surf, pattern, 7 + index)
    for kind in ("null", "identity", "shuffle"):
        so, uo = vc.permutation(kind, n_sift, 5), vc.permutation(kind, n_surf, 6)
        matcher.set_view_float(0, sift if so is None else sift[so], surf if uo is None else surf[uo])
        matcher.set_positions(0, pos)
        matcher.debug_set_view_device(1, sift, so, surf, uo, pos)
        want, got = matcher.debug_view_bank(0), matcher.debug_view_bank(1)
        assert (want["n_sift"], want["n_surf"]) == (n_sift, n_surf)
        assert want["n_special"] == len(vc._special_rows(pattern, n_sift)) and want["n_positions"] == n_sift + n_surf
        _same_bank(want, got, (n_sift, n_surf, pattern, kind))


def test_handoff_on_logical_shards():
    """Prepared on the first shard, copied to the second: both hold the host path's bytes."""
    from orthosfm_amd.matching import HipExhaustiveMatching
    sift, surf, pos = vc.bank_case(257, 513, "block_edge", 3)
    so, uo = vc.permutation("shuffle", 257, 1), vc.permutation("shuffle", 513, 2)
    m = HipExhaustiveMatching(2, device=[0, 0])
    try:
        m.set_view_float(0, sift[so], surf[uo])
        m.set_positions(0, pos)
        m.debug_set_view_device(1, sift, so, surf, uo, pos)
        for shard in (0, 1):
            _same_bank(m.debug_view_bank(0, shard), m.debug_view_bank(1, shard), shard)
    finally:
        m.close()


# ---- 3. the front end equals the old path -----------------------------------------------------------------------
@pytest.mark.parametrize("halved", (False, True))
@pytest.mark.parametrize("name", FEATURE_CASES)
def test_front_end_equals_the_old_path(name, halved, old_path, matcher):
    from orthosfm_amd.features import ViewFrontEnd
    img = sc.image(name)
    h, w = img.shape[:2]
    want, seen = old_path[name, halved]
    assert len(want.sift) > 0 and (halved or len(want.surf) > 0)
    with ViewFrontEnd(0, w, h, max_image_size=w * h - 1 if halved else 0) as front:
        s = front.load(img)
        assert s.num_halvings == int(halved) and front.debug_image().tobytes() == seen.tobytes()
        got = front.download()
        _same_features(got, want, name)
        assert (got.import_width, got.feature_width) == (w, seen.shape[1])
        assert (s.num_sift, s.num_surf) == (len(want.sift), len(want.surf))
        matcher.set_view_features(0, want)
        matcher.set_view_from_front(1, front)
        _same_bank(matcher.debug_view_bank(0), matcher.debug_view_bank(1), name)


@pytest.mark.parametrize("types", (1, 2))
def test_one_detector_alone(types, old_path, matcher):
    from orthosfm_amd.features import ViewFrontEnd
    want, _ = old_path["base", False]
    img = sc.image("base")
    with ViewFrontEnd(0, img.shape[1], img.shape[0], max_image_size=0, feature_types=types) as front:
        s = front.load(img)
        got = front.download()
        kept, dropped = (want.sift, got.surf) if types == 1 else (want.surf, got.sift)
        assert (s.num_sift, s.num_surf) == ((len(want.sift), 0) if types == 1 else (0, len(want.surf))) and len(dropped) == 0
        mine = got.sift if types == 1 else got.surf
        for k in ("descriptors", "positions", "normalized", "scale", "orientation", "colors"):
            assert getattr(mine, k).tobytes() == getattr(kept, k).tobytes(), k
        assert got.normalized.tobytes() == kept.normalized.tobytes()
        empty = np.zeros((0, 128 if types == 2 else 64), np.float32)
        matcher.set_view_float(0, *((kept.descriptors, empty) if types == 1 else (empty, kept.descriptors)))
        matcher.set_positions(0, kept.normalized)
        matcher.set_view_from_front(1, front)
        _same_bank(matcher.debug_view_bank(0), matcher.debug_view_bank(1), types)


# ---- 4. matching through it -------------------------------------------------------------------------------------
def _match_results(m):
    r = m.pairwise_match(1, 0)
    out = [r.matches_1_2.tobytes(), r.matches_2_1.tobytes()]
    recs = m.compute([(1, 0)])
    out += [recs[0].status, recs[0].num_matches, recs[0].num_inliers, np.array(recs[0].matches).tobytes()]
    return out


@pytest.mark.parametrize("kind", ("exhaustive", "cascade", "shards"))
def test_matching_through_the_front_end(kind, old_path):
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    from orthosfm_amd.matching import HipCascadeHashing, HipExhaustiveMatching
    names = ("crop_a", "crop_b")
    results, hashes = {}, {}
    for path in ("host", "front"):
        o = capi.default_match_options()
        o.geometric_verification, o.use_lowres_matching, o.min_feature_matches, o.min_matching_inliers = 1, 0, 4, 4
        m = (HipCascadeHashing(2, device=0, options=o) if kind == "cascade"
             else HipExhaustiveMatching(2, device=[0, 0] if kind == "shards" else 0, options=o))
        try:
            with ViewFrontEnd(0, 160, 120, max_image_size=0) as front:
                for v, n in enumerate(names):
                    if path == "host":
                        m.set_view_features(v, old_path[n, False][0])
                    else:
                        front.load(sc.image(n))
                        m.set_view_from_front(v, front)
            results[path] = _match_results(m)
            if kind == "cascade":
                hashes[path] = [a.tobytes() for v in (0, 1) for t in (0, 1) for a in m.cascade_hashes(v, t)]
        finally:
            m.close()
    assert results["host"] == results["front"]
    assert int((np.frombuffer(results["host"][0], np.int32) >= 0).sum()) >= 5      # not a comparison of empty lists
    assert hashes.get("host") == hashes.get("front")


# ---- 5. ordering ------------------------------------------------------------------------------------------------
def test_a_load_waits_for_the_hand_off_before_it(old_path, matcher):
    """View A is handed off and view B loaded at once, through the same arrays: both banks are the host path's,
    twice over."""
    from orthosfm_amd.features import ViewFrontEnd
    from orthosfm_amd.matching import HipExhaustiveMatching
    want = []
    for name in ("many", "base"):
        matcher.set_view_features(0, old_path[name, False][0])
        want.append(matcher.debug_view_bank(0))
    runs = []
    m = HipExhaustiveMatching(2, device=0)
    try:
        with ViewFrontEnd(0, 401, 299, max_image_size=0) as front:
            for run in range(2):
                front.load(sc.image("many"))
                m.set_view_from_front(0, front)
                front.load(sc.image("base"))
                m.set_view_from_front(1, front)
                runs.append([m.debug_view_bank(0), m.debug_view_bank(1)])
    finally:
        m.close()
    for run in runs:
        _same_bank(want[0], run[0], "A")
        _same_bank(want[1], run[1], "B")
    _same_bank(runs[0][0], runs[1][0], "A again")
    _same_bank(runs[0][1], runs[1][1], "B again")


# ---- 6. errors and memory ---------------------------------------------------------------------------------------
def test_errors_leave_no_result_and_no_trace(old_path, matcher):
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    matcher.set_view_features(1, old_path["base", False][0])
    before = matcher.debug_view_bank(1)
    good = sc.image("crop_a")
    with ViewFrontEnd(0, 160, 120, max_image_size=0) as front:
        def refused(status, image):
            with pytest.raises(capi.OsfmError) as e:
                front.load(image)
            assert e.value.status == status, e.value
            assert front.summary is None
            for call in (front.download, front.debug_image, lambda: matcher.set_view_from_front(1, front)):
                with pytest.raises(capi.OsfmError) as e2:
                    call()
                assert e2.value.status == capi.E_STATE
            _same_bank(before, matcher.debug_view_bank(1), "untouched")

        with pytest.raises(capi.OsfmError) as e:                 # hand-off before any load
            matcher.set_view_from_front(1, front)
        assert e.value.status == capi.E_STATE
        for status, image in ((capi.E_ARG, np.zeros((20, 20, 2), np.uint8)), (capi.E_RANGE, np.zeros((120, 161), np.uint8)),
                              (capi.E_ARG, np.zeros((9, 9), np.uint8))):        # 9 x 9: the size SIFT refuses
            front.load(good)                                      # a result that the failing call must take away
            refused(status, image)
        front.load(good)
        with pytest.raises(capi.OsfmError) as e:                 # a view id out of range
            matcher.set_view_from_front(2, front)
        assert e.value.status == capi.E_ARG
        _same_bank(before, matcher.debug_view_bank(1), "untouched")
    # a chain that reaches a side below 2: 3 x 40 -> 2 x 20 -> 1 x 10, still above the limit
    with ViewFrontEnd(0, 40, 40, max_image_size=1, feature_types=capi.FEATURE_SURF) as front:
        with pytest.raises(capi.OsfmError) as e:
            front.load(np.zeros((40, 3), np.uint8))
        assert e.value.status == capi.E_ARG and "below 2" in str(e.value)
        with pytest.raises(capi.OsfmError) as e:
            matcher.set_view_from_front(1, front)
        assert e.value.status == capi.E_STATE
    with pytest.raises(capi.OsfmError) as e:
        ViewFrontEnd(0, 64, 64, feature_types=0)
    assert e.value.status == capi.E_ARG


def test_a_foreign_device_is_refused(old_path, matcher):
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    if capi.device_count() < 2:
        pytest.skip("needs a second device")
    matcher.set_view_features(1, old_path["base", False][0])
    before = matcher.debug_view_bank(1)
    with ViewFrontEnd(1, 160, 120, max_image_size=0) as front:
        front.load(sc.image("crop_a"))
        with pytest.raises(capi.OsfmError) as e:
            matcher.set_view_from_front(1, front)
        assert e.value.status == capi.E_ARG
    _same_bank(before, matcher.debug_view_bank(1), "untouched")


def test_front_end_memory_is_booked():
    from orthosfm_amd import capi
    from orthosfm_amd.features import FeatureSetExtractor, ViewFrontEnd
    before = capi.library_memory()
    with FeatureSetExtractor(0, 256, 192) as ex:
        detectors = capi.library_memory().device_buffer_bytes - before.device_buffer_bytes
    assert capi.library_memory().device_buffer_bytes == before.device_buffer_bytes
    front = ViewFrontEnd(0, 256, 192)
    held = capi.library_memory().device_buffer_bytes - before.device_buffer_bytes
    # both detectors' contexts, two image buffers (the second of half the size), and per feature positions,
    # normalised positions, colours and two row maps
    assert held >= detectors + 256 * 192 * 3 + 128 * 96 * 3 + 2 * 65536 * (8 + 8 + 3 + 4 + 4)
    front.load(sc.image("crop_a"))
    front.close()
    after = capi.library_memory()
    assert after.device_buffer_bytes == before.device_buffer_bytes
    assert (after.live_streams, after.live_events) == (before.live_streams, before.live_events)
