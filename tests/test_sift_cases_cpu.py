"""The numpy restatement of the SIFT detector (tests/sift_restatement.py) against the reference fixture
(tests/golden/sift_reference.npz) on the seeded cases of tests/sift_cases.py: the same image hashes, bit-identical
candidate lists and bit-identical localised keypoints -- and the comparison sees planted errors.  The figures that
tests/sift_cases.py records (the distance between the reference's orientations and descriptors and the float64
restatement's, the ambiguous keypoints) are measured again and must still hold."""
import numpy as np
import pytest

import sift_cases as sc
import sift_restatement as sr

LIVE = [c.name for c in sc.CASES if not c.refused]


def _opts(name):
    return sr.Options(min_octave=sc.BY_NAME[name].min_octave)


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
