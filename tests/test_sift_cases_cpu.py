"""The numpy restatement of the SIFT detector (tests/sift_restatement.py) against the reference fixture
(tests/golden/sift_reference.npz) on the seeded cases of tests/sift_cases.py: the same image hashes, bit-identical
candidate lists and bit-identical localised keypoints -- and the comparison sees planted errors.  The figures that
tests/sift_cases.py records (the distance between the reference's orientations and descriptors and the float64
restatement's, the ambiguous keypoints) are measured again and must still hold.  The edge cases are held to stand on
the kernel constants they are named for, and the sweep of tests/test_sift_gpu.py to be live."""
import numpy as np
import pytest

import sift_cases as sc
import sift_restatement as sr

LIVE = [c.name for c in sc.CASES if not c.refused]


def _opts(name):
    return sc.options(sc.BY_NAME[name])


def _hashes(octaves):
    return [[sc.sha(i) for i in o[1]] for o in octaves], [[sc.sha(i) for i in o[2]] for o in octaves]


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_input_is_the_fixtures(name):
    assert sc.sha(sc.image(name)) == str(sc.fixture(name)["image_sha"])
    c = sc.BY_NAME[name]
    assert sc.image(name).shape[:2] == (c.height, c.width)
    assert bool(sc.fixture(name)["threw"]) == c.refused == sr.refuses(c.width, c.height, _opts(name))


@pytest.mark.parametrize("name", LIVE)
def test_scale_space_candidates_and_keypoints_equal_the_reference(name):
    fx = sc.fixture(name)
    octs, cand, kps, _, _ = sc.restated(name)
    img, dog = _hashes(octs)
    assert img == fx["img_sha"].astype(str).tolist()
    assert dog == fx["dog_sha"].astype(str).tolist()
    assert [o[1][0].shape for o in octs] == [tuple(s) for s in fx["octave_shape"]]
    assert cand.tobytes() == fx["candidates"].tobytes()
    assert kps.tobytes() == fx["keypoints"].tobytes()


def test_cases_show_what_they_must():
    fx = sc.fixture("base")
    per_octave = [int((fx["keypoints"][:, 0] == o).sum()) for o in (0, 1, 2)]
    assert min(per_octave) >= 1, per_octave
    assert len(sc.fixture("many")["candidates"]) > 512
    assert (sc.fixture("up")["keypoints"][:, 0] == -1).any()
    tiny = sc.fixture("tiny")
    assert tuple(tiny["octave_shape"][-1]) == (3, 3) and len(tiny["gen_meta"]) == 0
    # the blur radius (up to 9 at the defaults) exceeds the small octaves of tiny
    assert max(sr.gaussian_weights(s)[0] for s in (1.2262735, 1.5450078, 1.9465878, 2.452547, 3.0900156)) > 5


def _sizes(name):
    """[(w, h)] of the case's octaves, by the fixture."""
    return [(int(s[1]), int(s[0])) for s in sc.fixture(name)["octave_shape"]]


def _chain(w, h, n):
    out = []
    for _ in range(n):
        out.append((w, h))
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return out


def test_edge_cases_reach_their_edges():
    """Each case of sift_cases.EDGE_CASES stands on the kernel constant it is named for: kBlock = 256 (row segments,
    blocks of interior pixels), kColTile = 32, kMaxRadius = 32 and the 2-pixel bound of octave_sizes()."""
    radii = sr.blur_radii(sr.Options())
    assert 3 < min(radii) and max(radii) < 16, radii             # the defaults stay far below kMaxRadius
    for name in sc.EDGE:
        c = sc.BY_NAME[name]
        assert not c.descriptors and c.refused == sr.refuses(c.width, c.height, _opts(name)) == bool(sc.fixture(name)["threw"])
        if c.refused:
            continue
        first = [(2 * c.width, 2 * c.height)] if c.min_octave < 0 else []
        assert _sizes(name) == first + _chain(c.width, c.height, 5), name
        # every octave that is not all border holds a candidate
        cand = sc.fixture(name)["candidates"]
        for o, (w, h) in enumerate(_sizes(name)):
            if min(w, h) >= sc.MIN_SIDE:
                assert (cand[:, 0] == o + c.min_octave).any(), (name, o, w, h)
    # row segments of 256: exact multiples in octaves 0 and 1, and second segments of 33 and of 3 pixels
    assert [s[0] for s in _sizes("w512")[:2]] == [512, 256] and _sizes("w256")[0][0] == 256
    assert _sizes("w289")[0][0] - 256 == 33 and _sizes("w259")[0][0] - 256 == 3 < min(radii)
    # column tiles of 32: heights and widths of 32, 33, 64 and 65
    assert _sizes("c64x65")[:2] == [(64, 65), (32, 33)] and _sizes("c33x32")[0] == (33, 32)
    # the bound of octave_sizes(), per dimension: 17 is taken with a last octave of 2, 16 is refused
    assert _sizes("min40x17")[-1] == (3, 2) and _sizes("min17x40")[-1] == (2, 3)
    for name, (w, h) in (("ref40x16", (40, 16)), ("ref16x40", (16, 40))):
        assert sc.BY_NAME[name].refused and (sc.BY_NAME[name].width, sc.BY_NAME[name].height) == (w, h)
        assert _chain(w, h, 5)[-1][w > h] == 1                     # the side that falls below 2 at the last halving
    # 32 is the largest side with a last octave of 2 pixels (33 gives 3): no interior pixel, no extrema launch
    assert _sizes("two40x32")[-1] == (3, 2) and _sizes("two32x40")[-1] == (2, 3) and _chain(33, 33, 5)[-1] == (3, 3)
    assert sc.BY_NAME["up17x19"].min_octave == -1 and _sizes("up17x19")[0] == (34, 38) and _sizes("up17x19")[-1] == (2, 2)
    for name in ("min40x17", "min17x40", "two40x32", "two32x40", "up17x19"):
        w, h = _sizes(name)[-1]
        assert max(w - 2, 0) * max(h - 2, 0) == 0
    # blocks of 256 interior pixels: exactly one, and one and a part
    interior = lambda name: [(w - 2) * (h - 2) for w, h in _sizes(name)]
    assert interior("int18x18")[0] == 256 and interior("int19x18")[0] == 272 > 256
    # the largest radius the kernels hold, and one more
    r32 = sc.BY_NAME["r32"]
    assert (r32.samples, r32.base_blur_sigma, r32.width, r32.height) == (1, 1.6, 80, 70)
    assert sr.blur_radii(_opts("r32")) == [8, 16, 32]
    assert abs(float(_opts("r32").base_blur_sigma) * 48 ** 0.5 - 11.085) < 1e-3
    over = sr.Options(num_samples_per_octave=1, base_blur_sigma=np.float32(sc.RADIUS_REFUSED_SIGMA))
    assert max(sr.blur_radii(over)) == 33
    assert sc.fixture("r32")["img_sha"].shape == (5, 4) and sc.fixture("r32")["dog_sha"].shape == (5, 3)


def test_a_mirrored_halo_is_seen_on_the_edge_cases():
    """A blur whose halo mirrors the image where it should repeat the border pixel changes a hash of every edge
    case, and of an octave of every size: the halo is clamped in all of them."""
    for name in sc.EDGE:
        if sc.BY_NAME[name].refused:
            continue
        fx = sc.fixture(name)
        img, dog = _hashes(sr.scale_space(sc.image(name), _opts(name), plant_mirrored=True))
        want_img, want_dog = fx["img_sha"].astype(str).tolist(), fx["dog_sha"].astype(str).tolist()
        assert img != want_img and dog != want_dog, name
        # octave 0 at the defaults starts from a blurred image: every image of every octave differs
        assert all(a != b for o, w in zip(img, want_img) for a, b in zip(o[1:], w[1:])), name


def test_the_sweep_holds_what_it_must():
    """The restatement on all 127 shapes of the sweep takes 1.3 s here (measured on one CPU core), so the range is
    not cut: 17 .. 80 either way.  Every bound of the default radii against 32-row tiles and every halving parity is
    crossed; the sweep is a restatement-only check (tests/test_sift_gpu.py), here its cases are held to be live."""
    shapes = sc.SWEEP_SHAPES
    assert len(shapes) == len(set(shapes)) == 127 and sum(len(c) for c in sc.SWEEP_CHUNKS) == 127
    assert {w for w, h in shapes if h == sc.SWEEP_SIDE} == set(range(17, 81))
    assert {h for w, h in shapes if w == sc.SWEEP_SIDE} == set(range(17, 81))
    assert sr.refuses(16, 80, sr.Options()) and sr.refuses(80, 16, sr.Options()) and not sr.refuses(17, 17, sr.Options())
    full = dict(sc.sweep_restated(80, 80))
    seen = set()
    for w, h in shapes:
        got = dict(sc.sweep_restated(w, h))
        assert len(got) == 5 * 11 + 2
        seen.add(got["candidates"])
        if (w, h) != (80, 80):
            assert got["octave 0 image 0"] != full["octave 0 image 0"]
    assert len(seen) > len(shapes) // 2                         # most shapes have a candidate list of their own
    assert sc.sha(np.zeros((0, 4), np.float32)) not in seen     # and no shape is without any


def test_planted_errors_break_an_equality():
    """A reversed tap order, an unclamped border index, >= replaced by > and one Taylor step fewer."""
    name = "base"
    fx = sc.fixture(name)
    opts = _opts(name)
    octs, cand, kps, _, _ = sc.restated(name)
    for plant in ({"plant_reversed_taps": True}, {"plant_unclamped": True}):
        img, dog = _hashes(sr.scale_space(sc.image(name), opts, **plant))
        assert img != fx["img_sha"].astype(str).tolist() and dog != fx["dog_sha"].astype(str).tolist(), plant
    # a plateau makes > and >= differ: on the case's own image no two neighbours tie, so put a tie in
    tied = [(i, [a.copy() for a in imgs], [d.copy() for d in dogs]) for i, imgs, dogs in octs]
    row = fx["candidates"][0]
    dogs = tied[int(row[0]) - opts.min_octave][2]
    x, y, s = int(row[2]), int(row[3]), int(row[1])
    dogs[s + 1][y, x + 1] = dogs[s + 1][y, x]
    assert len(sr.extrema(tied)) == len(sr.extrema(octs)) - 1
    assert len(sr.extrema(tied, plant_nonstrict=True)) > len(sr.extrema(tied))
    assert sr.localise(octs, cand, opts, plant_steps=4)[0].tobytes() != fx["keypoints"].tobytes()


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.descriptors])
def test_measured_figures_hold(name):
    d_ori, d_desc, ambiguous, keypoints = sc.MEASURED[name]
    fig = sc.measure(name)
    print(f"{name}: d_ori {fig['d_ori']:.3e} d_desc {fig['d_desc']:.3e} ambiguous {fig['ambiguous']} of {fig['keypoints']}")
    assert fig["keypoints"] == keypoints and fig["ambiguous"] == ambiguous
    assert fig["ambiguous"] <= 0.02 * keypoints
    assert fig["f32_count_differs"] == 0 and fig["f64_count_differs"] == 0
    # recorded to four digits
    assert abs(fig["d_ori"] - d_ori) <= 1e-3 * d_ori and abs(fig["d_desc"] - d_desc) <= 1e-3 * d_desc
    assert 4.0 * d_desc < 1.0 / 510.0


def test_sorted_view_and_colours_follow_from_the_generation_order():
    """FeatureSet's view of the fixture: a sort by scale (stable up to groups of equal scale), linear_at colours and
    normalised positions as the restatement computes them."""
    for name in ("base", "rgb"):
        fx, c = sc.fixture(name), sc.BY_NAME[name]
        meta = fx["gen_meta"][fx["sorted_perm"]]
        assert (np.diff(meta[:, 2]) <= 0).all()
        assert sorted(fx["sorted_perm"].tolist()) == list(range(len(meta)))
        for row, col, nrm in zip(meta, fx["sorted_colors"], fx["sorted_normalized"]):
            px = sr.linear_at_u8(sc.image(name), row[0], row[1])
            assert (np.resize(px, 3) == col).all() if c.channels == 1 else (px == col).all()
            assert np.array(sr.normalized_position(row[0], row[1], c.width, c.height), np.float32).tobytes() == nrm.tobytes()
