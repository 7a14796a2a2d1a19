"""The shared row function of the view marks (osfm_view_debug_mark_rows, host code) and osfm_tracks_filter_marked
against the numpy restatement of tests/mark_cases.py, byte for byte -- after showing that the seeded cases reach
what they are meant to reach."""
import numpy as np
import pytest

import mark_cases as mc

CLAMPS = ("reference", "image")


# ---- 1. the cases reach their targets ---------------------------------------------------------------------------
def test_row_cases_reach_their_targets():
    cases = mc.row_cases()
    c = cases["landscape"]
    xy = mc.pixel_positions(c["normalized"], c["width"])
    rows, cols = c["mask"].shape
    assert cols > rows
    ref, img = mc.marks(c["mask"], xy, "reference"), mc.marks(c["mask"], xy, "image")
    # a row with x >= rows inside the image, on which the two clamps disagree
    wide = (xy[:, 0] >= rows) & (xy[:, 0] < cols) & (xy[:, 1] >= 0) & (xy[:, 1] < rows)
    assert (wide & ((ref & 1) != (img & 1))).any()
    cx, _ = mc.mask_indices(c["mask"].shape, xy, "reference")
    assert (cx[wide] == rows - 1).all()
    # negative positions clamped to 0, on both axes
    assert (xy[:, 0] < 0).any() and (xy[:, 1] < 0).any()
    assert (mc.mask_indices(c["mask"].shape, xy, "reference")[0][xy[:, 0] < 0] == 0).all()
    # an index outside the mask, only with the reference's clamp
    assert (ref & mc.MARK_OUTSIDE).any() and not (img & mc.MARK_OUTSIDE).any()
    assert not (ref[(ref & mc.MARK_OUTSIDE) != 0] & mc.MARK_IN).any()
    # mask values 16 (out) and 17 (in) are both read
    for clamp in CLAMPS:
        cx, cy = mc.mask_indices(c["mask"].shape, xy, clamp)
        ok = (cx < cols) & (cy < rows)
        read = c["mask"][cy[ok], cx[ok]]
        m = mc.marks(c["mask"], xy, clamp)[ok]
        assert (read == 16).any() and (read == 17).any()
        assert not (m[read == 16] & 1).any() and (m[read == 17] & 1).all()
    # colours: positions beyond the image on both sides are clamped, not dropped
    assert (xy[:, 0] > cols - 1).any() and (xy[:, 1] > rows - 1).any()
    # the portrait mask leaves the mask through x
    p = cases["portrait"]
    pxy = mc.pixel_positions(p["normalized"], p["width"])
    cx, cy = mc.mask_indices(p["mask"].shape, pxy, "reference")
    assert (cx >= p["mask"].shape[1]).any()
    # square and in range: the clamps agree, nothing is outside
    s = cases["square_grey"]
    sxy = mc.pixel_positions(s["normalized"], s["width"])
    assert np.array_equal(mc.marks(s["mask"], sxy, "reference"), mc.marks(s["mask"], sxy, "image"))
    assert not (mc.marks(s["mask"], sxy, "reference") & mc.MARK_OUTSIDE).any()
    assert 0 < int((mc.marks(s["mask"], sxy, "reference") & 1).sum()) < len(sxy)
    # a mask of another size than the image, and a view without one
    o = cases["other_size"]
    assert o["mask"].shape != o["image"].shape[:2]
    assert cases["no_mask"]["mask"] is None
    nxy = mc.pixel_positions(cases["no_mask"]["normalized"], 40)
    assert (mc.marks(None, nxy) == mc.MARK_IN).all()


def test_track_cases_reach_their_targets():
    c = mc.track_cases()["mixed"]
    out = []
    for t in range(len(c["offsets"]) - 1):
        fs = c["features"][c["offsets"][t]:c["offsets"][t + 1]]
        out.append(sum(1 for v, f in fs if c["has_mask"][v] and not c["marks"][v][f] & 1))
    assert out[0] == 0 and out[1] == 1 and 0 in out[2:] and max(out) >= 1
    keep = mc.filter_tracks_with_masks(c["offsets"], c["features"], c["marks"], c["has_mask"])
    assert keep.tolist() == [True, False, True, False, False, True, True]
    n = mc.track_cases()["no_mask_anywhere"]
    assert mc.filter_tracks_with_masks(n["offsets"], n["features"], n["marks"], n["has_mask"]).all()
    s = mc.track_cases()["seeded"]
    k = mc.filter_tracks_with_masks(s["offsets"], s["features"], s["marks"], s["has_mask"])
    assert 5 <= int(k.sum()) <= len(k) - 5


# ---- 2. the library against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("clamp", CLAMPS)
@pytest.mark.parametrize("name", sorted(mc.row_cases()))
def test_row_function_equals_the_restatement(name, clamp):
    from orthosfm_amd.features import mark_rows_host
    c = mc.row_cases()[name]
    want_xy, want_rgb, want_mark = mc.expected_rows(c, clamp)
    xy, rgb, mark = mark_rows_host(c["normalized"], c["image"], c["mask"], clamp)          # pixel_width 0: the image's width
    assert xy.dtype == np.float32 and xy.tobytes() == want_xy.tobytes()
    assert rgb.tobytes() == want_rgb.tobytes()
    assert mark.tobytes() == want_mark.tobytes(), (int((mark != want_mark).sum()), "marks differ")
    xy2, rgb2, mark2 = mark_rows_host(c["normalized"], c["image"], c["mask"], clamp, pixel_width=c["width"])
    assert (xy2.tobytes(), rgb2.tobytes(), mark2.tobytes()) == (xy.tobytes(), rgb.tobytes(), mark.tobytes())


def test_row_function_threshold_and_width():
    """Another threshold and another pixel width than the image's go through to the lookup."""
    from orthosfm_amd.features import mark_rows_host
    c = mc.row_cases()["landscape"]
    xy = mc.pixel_positions(c["normalized"], 33)
    got = mark_rows_host(c["normalized"], c["image"], c["mask"], "reference", threshold=17, pixel_width=33)
    assert got[0].tobytes() == xy.tobytes()
    assert got[1].tobytes() == mc.propagate_colors(c["image"], xy).tobytes()
    assert got[2].tobytes() == mc.marks(c["mask"], xy, "reference", 17).tobytes()
    assert got[2].tobytes() != mc.marks(c["mask"], xy, "reference", 16).tobytes()


def test_row_function_refuses_bad_arguments():
    from orthosfm_amd import capi
    from orthosfm_amd.features import mark_rows_host
    c = mc.row_cases()["landscape"]
    with pytest.raises(capi.OsfmError) as e:
        mark_rows_host(c["normalized"], c["image"], np.zeros((0, 4), np.uint8))
    assert e.value.status == capi.E_ARG
    with pytest.raises(ValueError):
        mark_rows_host(c["normalized"], c["image"], c["mask"], clamp="nearest")


@pytest.mark.parametrize("name", sorted(mc.track_cases()))
def test_track_filter_equals_the_restatement(name):
    from orthosfm_amd import tracks as T
    c = mc.track_cases()[name]
    want = mc.filter_tracks_with_masks(c["offsets"], c["features"], c["marks"], c["has_mask"])
    got = T.filter_marked(c["offsets"], c["features"], c["marks"], c["has_mask"])
    assert got.dtype == np.uint8 and got.tobytes() == want.astype(np.uint8).tobytes()


def test_track_filter_refuses_a_feature_without_a_row():
    from orthosfm_amd import capi, tracks as T
    c = mc.track_cases()["mixed"]
    bad = c["features"].copy()
    bad[3] = (2, 6)                      # view 2 has rows 0..5
    with pytest.raises(capi.OsfmError) as e:
        T.filter_marked(c["offsets"], bad, c["marks"], c["has_mask"])
    assert e.value.status == capi.E_RANGE
