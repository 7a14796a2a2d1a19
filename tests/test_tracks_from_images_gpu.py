"""pipeline.tracks_from_images against the tracks built the old way -- extraction of the restated halved images,
set_view_features, one batch of osfm_match_all, the track builder and the reference's pixel conversion -- on three
windows of one seeded canvas.  The windows lie at even offsets and are halved once, so that the halved windows are
exact shifts of each other and show the same structures."""
import numpy as np
import pytest

import sift_cases as sc
import view_cases as vc

pytestmark = pytest.mark.gpu

CANVAS = (560, 420, 1200, 21)            # width, height, blobs, seed; sizes twice sift_cases' crops, sigmas too
WINDOW = (320, 240)
OFFSETS = ((20, 24), (74, 58), (48, 100))
LIMIT = WINDOW[0] * WINDOW[1] - 1        # max_image_size: one halving


@pytest.fixture(scope="module")
def windows():
    canvas = sc.render(CANVAS[0], CANVAS[1], 1, CANVAS[2], CANVAS[3], 2.0, 32.0)
    assert all(x % 2 == 0 and y % 2 == 0 for x, y in OFFSETS)
    out = [np.ascontiguousarray(canvas[y:y + WINDOW[1], x:x + WINDOW[0]]) for x, y in OFFSETS]
    # the halved windows are windows of the halved canvas
    half = vc.halve(canvas)
    for (x, y), w in zip(OFFSETS, out):
        assert vc.halve(w).tobytes() == np.ascontiguousarray(half[y // 2:y // 2 + 120, x // 2:x // 2 + 160]).tobytes()
    return out


def _options():
    from orthosfm_amd import capi
    o = capi.default_match_options()
    o.min_feature_matches, o.min_matching_inliers = 8, 8
    return o


@pytest.fixture(scope="module")
def old_way(windows):
    """(track offsets, track features, track colours, pixel positions per feature in track order, import width)"""
    from orthosfm_amd import capi, tracks as T
    from orthosfm_amd.features import FeatureSetExtractor
    from orthosfm_amd.matching import HipExhaustiveMatching
    from orthosfm_amd.pipeline import TrackTable
    with FeatureSetExtractor(0, 160, 120) as ex:
        sets = [ex.extract(vc.chain(w, 1, LIMIT)[1]) for w in windows]
    o = _options()
    o.geometric_verification = 1
    m = HipExhaustiveMatching(3, device=0, options=o)
    try:
        for v, fs in enumerate(sets):
            m.set_view_features(v, fs)
        pairs = np.array([capi.pair_from_index(i) for i in range(3)], np.int32)
        ra, corr = m.compute_arrays(pairs)
        builder = T.TracksBuilder([len(fs) for fs in sets])
        builder.feed(pairs, ra, corr)
        _, toff, tfeat, tcol, _ = builder.finish(np.concatenate([fs.colors for fs in sets]), want_track_ids=False)
        builder.close()
    finally:
        m.close()
    tt = TrackTable.from_mve(toff, tfeat, [fs.normalized for fs in sets], WINDOW[0], 3)
    return {"offsets": toff, "features": tfeat, "colors": tcol, "table": tt, "sets": sets, "status": ra["status"].copy()}


def test_the_old_path_gives_tracks_worth_comparing(old_way):
    lengths = np.diff(old_way["offsets"])
    print(f"old path: {len(lengths)} tracks, {int((lengths == 3).sum())} seen by all three views, pair status {old_way['status'].tolist()}")
    assert len(lengths) >= 10
    assert int((lengths >= 3).sum()) >= 1


def test_tracks_from_images_equal_the_old_way(windows, old_way):
    from orthosfm_amd.pipeline import join_background, tracks_from_images
    tt, colors, info = tracks_from_images(windows, device=0, verify=True, max_image_size=LIMIT, options=_options())
    join_background()
    want = old_way["table"]
    assert info["pair_status"].tolist() == old_way["status"].tolist()
    assert np.array_equal(tt.offsets, old_way["offsets"]) and tt.offsets.dtype == old_way["offsets"].dtype
    for k in ("view", "feat", "xy", "track_of", "by_view", "view_start"):
        a, b = getattr(tt, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert colors.dtype == np.uint8 and colors.tobytes() == old_way["colors"].tobytes()
    # the reference's quirk: import_width * (pos + 0.5) on both axes, pos normalised by the feature image's size
    norm = np.stack([old_way["sets"][v].normalized[f] for v, f in zip(tt.view, tt.feat)])
    pixels = (float(WINDOW[0]) * (norm.astype(np.float64) + 0.5)).astype(np.float32)
    assert tt.xy.astype(np.float32).tobytes() == pixels.tobytes()
    assert np.array_equal(tt.xy, pixels.astype(np.float64))
