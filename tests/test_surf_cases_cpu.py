"""The numpy restatement of the SURF detector (tests/surf_restatement.py) against the reference fixture
(tests/golden/surf_reference.npz) on the seeded cases of tests/surf_cases.py: the same hashes of the desaturated
image and of the 16 response maps, bit-identical candidates, keypoints, x, y, scale and sample coordinates; bit-identical
orientations and descriptors where this machine's C library gives the sines and cosines the fixture recorded -- and
the comparison sees planted errors."""
import numpy as np
import pytest

import sift_cases as sc
import surf_cases as uc
import surf_restatement as sr

NAMES = [c.name for c in uc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_stages_equal_the_reference(name):
    fx, c = uc.fixture(name), uc.BY_NAME[name]
    sat, maps, cand, kps, _ = uc.restated(name)
    assert sc.sha(uc.image(name)) == str(fx["image_sha"]) and uc.image(name).shape[:2] == (c.height, c.width)
    assert sc.sha(sr.grey_of(uc.image(name))) == str(fx["grey_sha"])
    assert [[sc.sha(m) for m in o] for o in maps] == fx["map_sha"].astype(str).tolist()
    assert [m[0].shape for m in maps] == [tuple(s) for s in fx["map_shape"]]
    assert cand.tobytes() == fx["candidates"].tobytes()
    assert kps.tobytes() == fx["keypoints"].tobytes()
    if c.counts:
        assert all(w is None or w == g for w, g in zip(c.counts, (len(cand), len(kps), len(fx["gen_meta"]))))


@pytest.mark.parametrize("name", NAMES)
def test_orientations_and_descriptors(name):
    from orthosfm_amd import capi
    fx = uc.fixture(name)
    local = uc.local_trig_is_the_fixtures(name)
    rows = uc.generation_rows(uc.restated(name)[4])
    print(f"{name}: this C library {'reproduces' if local else 'does NOT reproduce'} the fixture's sinf / cosf: "
          f"{'bytes' if local else 'tolerances only'}")
    assert len(rows) == len(fx["gen_meta"])
    if not rows:
        return
    meta = np.array([[r["x"], r["y"], r["scale"], r["orientation"]] for r in rows], np.float32)
    data = np.array([r["data"] for r in rows], np.float32)
    clear = np.array([not r["ambiguous"] for r in rows])
    assert meta[:, :3].tobytes() == fx["gen_meta"][:, :3].tobytes()
    assert np.abs(meta[clear, 3].astype(np.float64) - fx["gen_meta"][clear, 3]).max() <= 1e-6
    q, q_ref = capi.quantize_surf(data), capi.quantize_surf(fx["gen_data"])
    assert np.abs(q[clear].astype(np.int32) - q_ref[clear]).max() <= 1
    assert all(r["status"] == 1 for r in rows)
    if local:
        assert meta[clear].tobytes() == fx["gen_meta"][clear].tobytes()
        assert data[clear].tobytes() == fx["gen_data"][clear].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_measured_shares_hold(name):
    ambiguous, with_orientation = uc.measure(name)
    print(f"{name}: {ambiguous} ambiguous of {with_orientation} keypoints with an orientation")
    assert (ambiguous, with_orientation) == uc.MEASURED[name]
    assert ambiguous <= 0.02 * max(1, with_orientation)


def test_cases_show_what_they_must():
    big = uc.fixture("big")
    assert [int((big["keypoints"][:, 0] == o).sum()) for o in range(4)][3] == 16
    assert len({float(s) for s in big["gen_meta"][:, 2]}) == 6 and float(big["gen_meta"][:, 2].max()) == 10.0
    assert all((uc.fixture("base")["keypoints"][:, 0] == o).any() for o in range(4))
    assert len(uc.fixture("many")["candidates"]) > 2 * 256            # more than one scan block
    assert len(uc.fixture("tiny")["keypoints"]) == 1 and len(uc.fixture("tiny")["gen_meta"]) == 0
    assert len(uc.fixture("nothing")["candidates"]) == 0
    tie = uc.image("tie")
    assert tie.tobytes() == tie[::-1].tobytes() and tie.shape[0] % 2 == 0     # equal response maps in the middle rows
    assert uc.fixture("upright")["gen_data"].tobytes() != uc.fixture("base")["gen_data"].tobytes()
    # the scale truncates to the integer the exact value has, for all 12 reachable filters
    for o in range(4):
        for k in range(1, 4):
            fs = sr.filter_size(o, k)
            assert int(sr.keypoint_scale(np.array([o, k, 0, 0], np.float32))) == (3 * fs * 12) // 90
    # the 109 weights and the 16 windows
    assert len(sr.gaussian_table()[0]) == 109 and len(sr.window_starts()) == 16


def test_hand_placed_descriptors_equal_the_reference():
    fx, sat = uc.fixture("big"), uc.restated("big")[0]
    kinds = len(uc.FORCED_KINDS)
    for i, (x, y, scale, ori, upright) in enumerate(uc.forced()):
        s, c = fx["forced_trig"][i]
        status, data, coords = sr.describe(sat, x, y, scale, s, c)
        assert status == int(fx["forced_ok"][i]) == (0 if uc.FORCED_KINDS[i % kinds] == "rejected" else 1)
        if status:
            assert coords.astype(np.int16).tobytes() == fx["forced_coords"][i].tobytes()
            assert data.tobytes() == fx["forced_data"][i].tobytes()
            # the margins hold every tap inside its row (see tests/test_surf_gpu.py)
            ds = int(scale)
            assert coords[:, 0].min() - ds - 1 >= 0 and coords[:, 0].max() + ds < sat.shape[1]
            assert coords[:, 1].min() - ds - 1 >= 0 and coords[:, 1].max() + ds < sat.shape[0]


def test_planted_errors_break_an_equality():
    """An asymmetric border made symmetric, >= replaced by > in the neighbour test, one window fewer and float window
    sums, each held against the reference fixture.  A 17th window cannot be seen by any case: it is the first
    window's image by 2 pi, selects the same samples, and the strict comparison of lengths keeps the first."""
    name = "big"
    fx = uc.fixture(name)
    sat, maps, cand, kps, gen = uc.restated(name)
    planted = sr.response_maps(sat, plant_symmetric_border=True)
    assert [[sc.sha(m) for m in o] for o in planted] != fx["map_sha"].astype(str).tolist()
    # only `tie` holds equal neighbours: its image is its own mirror image about the axis between rows 59 and 60, the
    # box sums are integers, so a blob on the axis has its maximum twice; the reference rejects both rows
    tie_maps, tie_cand = uc.restated("tie")[1:3]
    tie_fx = uc.fixture("tie")
    assert all(m[59].tobytes() == m[60].tobytes() for m in tie_maps[0])
    assert tie_cand.tobytes() == tie_fx["candidates"].tobytes()
    nonstrict = sr.extrema(tie_maps, plant_nonstrict=True)
    assert nonstrict.tobytes() != tie_fx["candidates"].tobytes()
    extra = sorted(set(map(tuple, nonstrict.tolist())) - set(map(tuple, tie_cand.tolist())))
    assert len(extra) == len(nonstrict) - len(tie_cand) == 16 and {r[3] for r in extra} == {59.0, 60.0}
    assert len(sr.localise(tie_maps, nonstrict, 161, 120)) == len(tie_fx["keypoints"]) + 4
    for other in NAMES:
        if other != "tie":
            assert len(sr.extrema(uc.restated(other)[1], plant_nonstrict=True)) == len(uc.fixture(other)["candidates"])

    def oris(g):
        return np.array([r["orientation"] for r in uc.generation_rows(g)], np.float32)

    clear = np.array([not r["ambiguous"] for r in uc.generation_rows(gen)])
    want = fx["gen_meta"][:, 3]
    local = uc.local_trig_is_the_fixtures(name)
    print(f"{name}: planted orientations against {'the bytes' if local else '1e-6'} of the fixture's clear rows")

    def equal_the_fixture(o):
        if len(o) != len(want):
            return False
        if local:
            return o[clear].tobytes() == want[clear].tobytes()
        return bool(np.abs(o[clear].astype(np.float64) - want[clear]).max() <= 1e-6)

    assert clear.sum() >= len(clear) - uc.MEASURED[name][0] and equal_the_fixture(oris(gen))
    assert equal_the_fixture(oris(sr.generate(sat, kps, plant_windows=17)))
    assert not equal_the_fixture(oris(sr.generate(sat, kps, plant_windows=15)))
    assert not equal_the_fixture(oris(sr.generate(sat, kps, plant_float_sums=True)))
