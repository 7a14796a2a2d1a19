"""The numpy restatement of the SURF detector (tests/surf_restatement.py) against the reference fixture
(tests/golden/surf_reference.npz) on the seeded cases of tests/surf_cases.py: the same hashes of the desaturated
image and of the 16 response maps, bit-identical candidates, keypoints, x, y, scale and sample coordinates; bit-identical
orientations and descriptors where this machine's C library gives the sines and cosines the fixture recorded -- and
the comparison sees planted errors.  The edge cases are held to stand on the loop bounds and smallest sizes they are
named for."""
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


def test_edge_cases_reach_their_edges():
    """Each case of surf_cases.EDGE stands on the loop bound it is named for: sat_rows_kernel's rounds of 256 pixels,
    sat_cols_kernel's rounds of 8 rows, and the smallest sizes that give a response, a candidate, a descriptor."""
    size = {n: (uc.BY_NAME[n].width, uc.BY_NAME[n].height) for n in uc.EDGE}
    assert [size[n][0] % 256 for n in ("w256", "w512", "w513", "w769")] == [0, 0, 1, 1]
    assert [-(-size[n][0] // 256) for n in ("w256", "w512", "w513", "w769")] == [1, 2, 3, 4]
    assert size["tall"] == (37, 1031) and divmod(1031, 8) == (128, 7) and uc.LONG == ("tall",)
    residues = lambda names: {uc.BY_NAME[n].height % 8 for n in names}
    assert residues(n for n in NAMES if n not in uc.EDGE) == {0, 1, 3, 6, 7}
    assert residues(("h42", "h44", "h45")) == {2, 4, 5} and size["h48"][1] % 8 == 0
    assert residues(NAMES) == set(range(8))
    # every octave that can hold a candidate at the case's size does
    for n in uc.EDGE:
        cand = uc.fixture(n)["candidates"]
        for o in uc.capable_octaves(*size[n]):
            assert (cand[:, 0] == o).any(), (n, o)
    assert uc.capable_octaves(37, 37) == [0, 1] and uc.capable_octaves(449, 417) == [0, 1, 2, 3]
    assert uc.capable_octaves(16, 40) == uc.capable_octaves(40, 16) == [] and uc.capable_octaves(17, 17) == [0]

    # the three smallest sizes, per dimension: the case gives a first one, its image less a column or a row gives none
    def counts(img):
        sat = sr.integral(np.ascontiguousarray(img))
        maps = sr.response_maps(sat)
        cand = sr.extrema(maps)
        kps = sr.localise(maps, cand, img.shape[1], img.shape[0])
        return (sum(int(np.count_nonzero(m)) for o in maps for m in o), len(cand),
                len(uc.generation_rows(sr.generate(sat, kps))))

    for i, kind in enumerate(("response", "candidate", "descriptor")):
        n = uc.SMALLEST[kind]
        for name, cut in ((kind[:4] + "_w", np.s_[:, :-1]), (kind[:4] + "_h", np.s_[:-1, :])):
            assert min(size[name]) == n == size[name][name.endswith("_h")], name
            assert counts(uc.image(name))[i] >= 1 and counts(uc.image(name)[cut])[i] == 0, name
    assert counts(uc.image("resp_w"))[1] == 0 and counts(uc.image("cand_w"))[2] == 0     # and nothing of the next kind
    for kind, border in (("response", 5), ("candidate", 8)):
        assert uc.SMALLEST[kind] == 2 * border + 1
    assert uc.SMALLEST["descriptor"] == 2 * (15 * 2 + 1) + 1
    assert sr.filter_size(0, 0) + sr.filter_size(0, 0) // 2 + 1 == 5 and sr.filter_size(0, 1) + sr.filter_size(0, 1) // 2 + 1 == 8


def test_a_border_test_with_the_wrong_comparison_is_seen_on_the_edge_cases():
    """x + border > w for x + border >= w keeps one sample more per row and column wherever a sample lies on the
    bound: the maps of the planted restatement differ from the fixture's on the cases below, and on most shapes of
    the sweep (which takes 0.5 s for its 159 shapes here, on one CPU core, so its range is not cut)."""
    seen = []
    for name in uc.EDGE:
        planted = sr.response_maps(uc.restated(name)[0], plant_symmetric_border=True)
        if [[sc.sha(m) for m in o] for o in planted] != uc.fixture(name)["map_sha"].astype(str).tolist():
            seen.append(name)
    assert {"w256", "w512", "w513", "w769", "tall", "resp_w", "resp_h", "cand_w", "cand_h", "desc_w", "desc_h"} <= set(seen), seen
    shapes = uc.SWEEP_SHAPES
    assert len(shapes) == len(set(shapes)) == 159 and sum(len(c) for c in uc.SWEEP_CHUNKS) == 159
    assert {w for w, h in shapes if h == 80} == {h for w, h in shapes if w == 80} == set(range(1, 81))
    differ = [s for s in shapes if uc.sweep_restated(*s) != uc.sweep_restated(*s, plant_symmetric_border=True)]
    # every shape with any response has a sample of octave 0, sample 0 (border 5, step 1) on the bound
    assert set(differ) == {(w, h) for w, h in shapes if min(w, h) >= uc.SMALLEST["response"] - 1}
    empty = sc.sha(np.zeros((0, 4), np.float32))
    assert all((dict(uc.sweep_restated(w, h))["candidates"] != empty) == (min(w, h) >= uc.SMALLEST["candidate"])
               for w, h in shapes if min(w, h) <= uc.SMALLEST["candidate"])
    assert len({dict(uc.sweep_restated(*s))["candidates"] for s in shapes}) > len(shapes) // 2


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
        if other != "tie" and other not in uc.EDGE:
            assert len(sr.extrema(uc.restated(other)[1], plant_nonstrict=True)) == len(uc.fixture(other)["candidates"])
    # the edge cases have few blobs on a flat ground, and flat ground gives equal responses: most of them see the plant too
    tied = [n for n in uc.EDGE if len(sr.extrema(uc.restated(n)[1], plant_nonstrict=True)) > len(uc.fixture(n)["candidates"])]
    print("edge cases with tied neighbours:", tied)
    assert "w256" in tied and len(tied) >= 4

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
