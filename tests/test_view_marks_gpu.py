"""View masks and pixel colours on the device (include/osfm_hip.h, "View masks and pixel colours") against the numpy
restatement of tests/mark_cases.py: the marks beside an unchanged load (OSFM_MARK_TRACKS), the load with the masked-out
rows removed against the host path on the deleted rows (OSFM_MARK_FEATURES), pipeline.tracks_from_images with masks in
both modes, and save_project with the propagated colours.  Windows and the one-halving limit are those of
tests/test_tracks_from_images_gpu.py: the import image is the 320 x 240 window, the detectors see its half, and
import_width * (pos + 0.5) on both axes puts a row of the half image at y = 2 row + 40.  The windows' rows lie at
x from 48 to 283 and y from 85 to 238, so the masks that show the reference's quirks have 200 rows: x beyond 199
reads column 199 with the reference's clamp, and y beyond 199 leaves the mask."""
import os

import numpy as np
import pytest

import mark_cases as mc
import sift_cases as sc
import view_cases as vc

pytestmark = pytest.mark.gpu

CANVAS = (560, 420, 1200, 21)
WINDOW = (320, 240)
OFFSETS = ((20, 24), (74, 58), (48, 100))
LIMIT = WINDOW[0] * WINDOW[1] - 1        # max_image_size: one halving
COMPACT_PASS_ROWS = 1024                 # view_kernels.h kCompactPassRows: the rows one pass of the compaction's scan takes
BIG = (800, 600, 3, 9000, 33)            # width, height, channels, blobs, seed of the canvas that needs several passes
CHAIN = (640, 480, 3, 1500, 37, 6.0, 24.0)       # blobs wide enough to leave features after three halvings


def _canvas():
    return sc.render(CANVAS[0], CANVAS[1], 1, CANVAS[2], CANVAS[3], 2.0, 32.0)


@pytest.fixture(scope="module")
def windows():
    canvas = _canvas()
    return [np.ascontiguousarray(canvas[y:y + WINDOW[1], x:x + WINDOW[0]]) for x, y in OFFSETS]


def _rect_mask(rows, cols, x0=0.25, x1=0.75, y0=0.25, y1=0.75):
    """0 with a rectangle of 255, a strip of 17 (in) and one of 16 (out) at its left edge."""
    m = np.zeros((rows, cols), np.uint8)
    m[int(rows * y0):int(rows * y1), int(cols * x0):int(cols * x1)] = 255
    m[:, int(cols * x0):int(cols * x0) + 3] = 17
    m[:, int(cols * x0) + 3:int(cols * x0) + 6] = 16
    return m


MASKS = {
    "square": lambda: _rect_mask(200, 200),                 # the landscape mask cropped to a square
    "landscape": lambda: _rect_mask(200, 320),              # 200 rows: the windows' rows reach y = 238
    "other_size": lambda: _rect_mask(300, 400, 0.2, 0.9, 0.1, 0.8),       # not the image's size, and not scaled to it
    "all_out": lambda: np.zeros((240, 320), np.uint8),
    "all_in": lambda: np.full((240, 320), 255, np.uint8),
    "none": lambda: None,
}


@pytest.fixture(scope="module")
def front():
    from orthosfm_amd.features import ViewFrontEnd
    with ViewFrontEnd(0, WINDOW[0], WINDOW[1], max_image_size=LIMIT) as f:
        yield f


@pytest.fixture(scope="module")
def plain(front, windows):
    """Per window the download of a plain load: computed once, read-only."""
    out = []
    for w in windows:
        s = front.load(w)
        assert (s.import_width, s.import_height, s.feature_width, s.num_halvings) == (320, 240, 160, 1)
        out.append(front.download())
    return out


@pytest.fixture(scope="module")
def matcher():
    from orthosfm_amd.matching import HipExhaustiveMatching
    m = HipExhaustiveMatching(2, device=0)
    yield m
    m.close()


def _view_bytes(fs):
    out = []
    for part in (fs.sift, fs.surf):
        out += [getattr(part, k).tobytes() for k in ("descriptors", "positions", "normalized", "scale", "orientation", "colors")]
    return out + [fs.positions.tobytes(), fs.normalized.tobytes(), fs.colors.tobytes()]


def _same_bank(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
            assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k] != b[k]).sum()), "elements differ")
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _summary_counts(ms):
    return {k: getattr(ms, k) for k in ("masked_out_sift", "masked_out_surf", "outside", "kept_sift", "kept_surf", "has_mask",
                                        "pixel_width")}


# ---- 1. OSFM_MARK_TRACKS ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_name,clamp", [("square", "reference"), ("landscape", "reference"), ("landscape", "image"),
                                             ("other_size", "reference"), ("none", "reference")])
def test_marks_ride_beside_an_unchanged_load(mask_name, clamp, front, windows, plain):
    mask = MASKS[mask_name]()
    want = plain[0]
    ns, n = len(want.sift), len(want)
    s = front.load_marked(windows[0], mask, "tracks", clamp)
    assert (s.num_sift, s.num_surf) == (ns, n - ns)
    assert _view_bytes(front.download()) == _view_bytes(want)
    xy, rgb, mark = front.download_marks()
    case = dict(image=windows[0], mask=mask, normalized=want.normalized, width=WINDOW[0])
    want_xy, want_rgb, want_mark = mc.expected_rows(case, clamp)
    out = (want_mark & 1) == 0
    print(f"{mask_name}/{clamp}: {n} rows, {int(out.sum())} masked out, {int(((want_mark & 2) != 0).sum())} outside the mask")
    assert xy.tobytes() == want_xy.tobytes() and rgb.tobytes() == want_rgb.tobytes()
    assert mark.tobytes() == want_mark.tobytes(), int((mark != want_mark).sum())
    assert _summary_counts(front.mark_summary) == dict(
        masked_out_sift=int(out[:ns].sum()), masked_out_surf=int(out[ns:].sum()), outside=int(((want_mark & 2) != 0).sum()),
        kept_sift=ns, kept_surf=n - ns, has_mask=int(mask is not None), pixel_width=WINDOW[0])
    if mask_name == "landscape":
        # the quirks are there: rows beyond the last mask row, and rows on which the clamps part
        other = mc.marks(mask, want_xy, "image" if clamp == "reference" else "reference")
        assert (want_xy[:, 1] > mask.shape[0] - 1).any() and (other != want_mark).any()
        assert ((want_mark & 2) != 0).any() == (clamp == "reference")
    if mask is not None:
        assert 0 < int(out.sum()) < n


def test_the_hand_off_of_a_marked_load_is_the_plain_one(front, windows, matcher):
    front.load(windows[1])
    matcher.set_view_from_front(0, front)
    front.load_marked(windows[1], MASKS["landscape"](), "tracks")
    matcher.set_view_from_front(1, front)
    _same_bank(matcher.debug_view_bank(0), matcher.debug_view_bank(1), "tracks mode")


# ---- 2. OSFM_MARK_FEATURES --------------------------------------------------------------------------------------
def _features_mode_case(front, image, mask, clamp, want_plain, matcher, what):
    """Loads twice in features mode; checks both against the plain download with the rows deleted, and the bank
    against the host path on those rows.  Returns the keep flags."""
    want_mark = mc.marks(mask, mc.pixel_positions(want_plain.normalized, image.shape[1]), clamp)
    keep = (want_mark & 1) != 0
    want = mc.delete_rows(want_plain, keep)
    ns = len(want_plain.sift)
    runs = []
    for _ in range(2):
        s = front.load_marked(image, mask, "features", clamp)
        assert (s.num_sift, s.num_surf) == (int(keep[:ns].sum()), int(keep[ns:].sum())), what
        ms = front.mark_summary
        assert (ms.kept_sift, ms.kept_surf) == (s.num_sift, s.num_surf)
        assert (ms.masked_out_sift, ms.masked_out_surf) == (int((~keep[:ns]).sum()), int((~keep[ns:]).sum()))
        got = front.download()
        xy, rgb, mark = front.download_marks()
        matcher.set_view_from_front(1, front)
        runs.append((_view_bytes(got), xy.tobytes(), rgb.tobytes(), mark.tobytes(), matcher.debug_view_bank(1)))
    assert runs[0][:4] == runs[1][:4], what
    _same_bank(runs[0][4], runs[1][4], (what, "again"))
    assert runs[0][0] == _view_bytes(want), what
    case = dict(image=image, mask=mask, normalized=want.normalized, width=image.shape[1])
    want_xy, want_rgb, _ = mc.expected_rows(case, clamp)
    assert runs[0][1] == want_xy.tobytes() and runs[0][2] == want_rgb.tobytes()
    assert runs[0][3] == np.full(int(keep.sum()), mc.MARK_IN, np.uint8).tobytes()
    matcher.set_view_features(0, want)
    _same_bank(matcher.debug_view_bank(0), runs[0][4], what)
    return keep


@pytest.mark.parametrize("mask_name,clamp", [("landscape", "reference"), ("landscape", "image"), ("other_size", "image"),
                                             ("all_out", "image"), ("all_in", "image"), ("none", "reference")])
def test_features_mode_equals_the_host_path_on_the_kept_rows(mask_name, clamp, front, windows, plain, matcher):
    keep = _features_mode_case(front, windows[0], MASKS[mask_name](), clamp, plain[0], matcher, (mask_name, clamp))
    print(f"{mask_name}/{clamp}: {int(keep.sum())} of {len(keep)} rows kept")
    if mask_name == "all_out":
        assert not keep.any()
    elif mask_name in ("all_in", "none"):
        assert keep.all()
    else:
        assert 0 < int(keep.sum()) < len(keep)


def test_features_mode_over_several_passes(matcher):
    """More kept rows of each detector than one pass of the scan numbers."""
    from orthosfm_amd.features import ViewFrontEnd
    w, h, ch, blobs, seed = BIG
    img = sc.render(w, h, ch, blobs, seed, 1.0, 4.0)
    mask = _rect_mask(h, w, 0.05, 0.95, 0.05, 0.95)
    with ViewFrontEnd(0, w, h, max_image_size=0) as big:
        big.load(img)
        want = big.download()
        keep = _features_mode_case(big, img, mask, "image", want, matcher, "big")
    ns = len(want.sift)
    print(f"big canvas: {ns} + {len(want) - ns} rows, kept {int(keep[:ns].sum())} + {int(keep[ns:].sum())}")
    assert int(keep[:ns].sum()) > COMPACT_PASS_ROWS and int(keep[ns:].sum()) > COMPACT_PASS_ROWS
    assert (~keep[:ns]).any() and (~keep[ns:]).any()
    # kept and dropped rows alternate inside the passes, not only at their ends
    assert int((np.diff(keep.astype(np.int8)) != 0).sum()) > 8


# ---- 3. the import image behind a longer chain ------------------------------------------------------------------
@pytest.mark.parametrize("doubled,downscale,behind", [(False, 1, 2), (True, 2, 2), (False, 2, 1)])
def test_marks_read_the_import_image_behind_the_chain(doubled, downscale, behind):
    """Two halvings behind the import image would overwrite it in the two buffers of a plain load; one does not.
    The doubled image repeats every pixel, so that its first halving gives the image back: the import image lies in
    the second buffer then, and the detectors see what they see in the first case."""
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    img = sc.render(*CHAIN)
    if doubled:
        img = np.ascontiguousarray(np.repeat(np.repeat(img, 2, axis=0), 2, axis=1))
    limit = 160 * 120
    imported, feat, halvings = vc.chain(img, downscale, limit)
    assert halvings - (downscale - 1) == behind and (not doubled or imported.tobytes() == sc.render(*CHAIN).tobytes())
    mask = _rect_mask(imported.shape[0], imported.shape[1])
    before = capi.library_memory().device_buffer_bytes
    with ViewFrontEnd(0, img.shape[1], img.shape[0], downscale_factor=downscale, max_image_size=limit) as f:
        f.load(img)
        want = f.download()
        held = capi.library_memory().device_buffer_bytes
        s = f.load_marked(img, mask, "tracks", "image")
        assert capi.library_memory().device_buffer_bytes > held               # the marks' arrays are booked
        assert (s.import_width, s.import_height, s.num_halvings) == (imported.shape[1], imported.shape[0], halvings)
        assert f.debug_image().tobytes() == feat.tobytes()
        assert _view_bytes(f.download()) == _view_bytes(want) and len(want) > 20
        xy, rgb, mark = f.download_marks()
        case = dict(image=imported, mask=mask, normalized=want.normalized, width=imported.shape[1])
        want_xy, want_rgb, want_mark = mc.expected_rows(case, "image")
        assert xy.tobytes() == want_xy.tobytes() and mark.tobytes() == want_mark.tobytes()
        assert rgb.tobytes() == want_rgb.tobytes(), int((rgb != want_rgb).any(axis=1).sum())
        assert len(np.unique(rgb[:, 0])) > 8
    assert capi.library_memory().device_buffer_bytes == before


def test_the_third_image_buffer_is_taken_only_where_the_chain_needs_it():
    """One halving behind the import image against two, everything else alike: the difference in booked memory is
    the buffer for the import image halved twice (160 x 120 x 3 bytes and a grow-only buffer's slack of an eighth)."""
    from orthosfm_amd import capi
    from orthosfm_amd.features import ViewFrontEnd
    img = sc.render(*CHAIN)
    grown = {}
    for behind, limit in ((1, 320 * 240), (2, 160 * 120)):
        with ViewFrontEnd(0, img.shape[1], img.shape[0], max_image_size=limit) as f:
            s = f.load(img)
            assert s.num_halvings == behind
            held = capi.library_memory().device_buffer_bytes
            f.load_marked(img, None)
            grown[behind] = capi.library_memory().device_buffer_bytes - held
    quarter = 160 * 120 * 3
    assert quarter <= grown[2] - grown[1] < 2 * quarter


# ---- 4. errors --------------------------------------------------------------------------------------------------
def test_errors(front, windows):
    from orthosfm_amd import capi
    front.load(windows[0])
    with pytest.raises(capi.OsfmError) as e:
        front.download_marks()
    assert e.value.status == capi.E_STATE
    for status, image, mask in ((capi.E_ARG, windows[0], np.zeros((0, 7), np.uint8)), (capi.E_RANGE, np.zeros((240, 321), np.uint8), None),
                                (capi.E_ARG, np.zeros((20, 20, 2), np.uint8), None)):
        front.load_marked(windows[0], None)
        with pytest.raises(capi.OsfmError) as e:
            front.load_marked(image, mask)
        assert e.value.status == status and front.summary is None
        for call in (front.download, front.download_marks):
            with pytest.raises(capi.OsfmError) as e2:
                call()
            assert e2.value.status == capi.E_STATE
    with pytest.raises(ValueError):
        front.load_marked(windows[0], None, mode="rows")
    with pytest.raises(TypeError):
        front.load_marked(windows[0], np.zeros((240, 320), np.float32))


# ---- 5. pipeline.tracks_from_images -----------------------------------------------------------------------------
def _options():
    from orthosfm_amd import capi
    o = capi.default_match_options()
    o.min_feature_matches, o.min_matching_inliers = 8, 8
    return o


def _scene_masks():
    """One object in canvas coordinates, seen through every window, in masks of 200 rows; the second view has no mask.
    Of the 41 tracks of the unmasked call 36 survive with the reference's clamp and 38 with the image's."""
    canvas = np.zeros((CANVAS[1], CANVAS[0]), np.uint8)
    canvas[:, 130:420] = 255
    out = [np.ascontiguousarray(canvas[y:y + 200, x:x + WINDOW[0]]) for x, y in OFFSETS]
    out[1] = None
    return out


@pytest.fixture(scope="module")
def unmasked(windows):
    from orthosfm_amd.pipeline import join_background, tracks_from_images
    tt, colors, info = tracks_from_images(windows, device=0, verify=True, max_image_size=LIMIT, options=_options())
    join_background()
    assert "mask" not in info and "feature_rgb" not in info
    return tt, colors, info


def _same_table(a, b):
    assert np.array_equal(a.offsets, b.offsets) and a.offsets.dtype == b.offsets.dtype
    for k in ("view", "feat", "xy", "track_of", "by_view", "view_start"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _restated_marks(plain, windows, masks, clamp):
    xy = [mc.pixel_positions(p.normalized, WINDOW[0]) for p in plain]
    return ([mc.marks(m, p, clamp) for m, p in zip(masks, xy)], [mc.propagate_colors(w, p) for w, p in zip(windows, xy)])


@pytest.mark.parametrize("clamp", ("reference", "image"))
def test_tracks_mode_equals_the_numpy_filter(clamp, windows, plain, unmasked):
    from orthosfm_amd.pipeline import TrackTable, join_background, tracks_from_images
    masks = _scene_masks()
    tt0, col0, info0 = unmasked
    marks, rgb = _restated_marks(plain, windows, masks, clamp)
    has_mask = [m is not None for m in masks]
    tf0 = np.stack([tt0.view, tt0.feat], axis=1)
    keep = mc.filter_tracks_with_masks(tt0.offsets, tf0, marks, has_mask)
    print(f"{clamp}: {len(keep)} tracks, {int((~keep).sum())} dropped, {int(keep.sum())} survive")
    assert int((~keep).sum()) >= 1 and int(keep.sum()) >= 10
    kept_f = keep[tt0.track_of]
    offsets = np.concatenate([[0], np.cumsum(np.diff(tt0.offsets)[keep])]).astype(np.int64)
    want = TrackTable.from_mve(offsets, tf0[kept_f], [p.normalized for p in plain], WINDOW[0], 3)
    tt, colors, info = tracks_from_images(windows, device=0, verify=True, max_image_size=LIMIT, options=_options(), masks=masks,
                                          mask_clamp=clamp, feature_colors=True)
    join_background()
    _same_table(tt, want)
    assert colors.tobytes() == col0[keep].tobytes()
    assert info["pair_status"].tolist() == info0["pair_status"].tolist()
    assert info["mask"]["tracks_built"] == len(keep) and info["mask"]["tracks_dropped"] == int((~keep).sum())
    assert info["mask"]["masked_out_sift"] == [int(((m[:len(p.sift)] & 1) == 0).sum()) for m, p in zip(marks, plain)]
    assert info["mask"]["outside"] == [int(((m & 2) != 0).sum()) for m in marks]
    want_rgb = np.stack([rgb[v][f] for v, f in zip(tt.view, tt.feat)])
    assert info["feature_rgb"].dtype == np.uint8 and info["feature_rgb"].tobytes() == want_rgb.tobytes()
    assert tt.xy.astype(np.float32).tobytes() == np.stack(
        [mc.pixel_positions(plain[v].normalized, WINDOW[0])[f] for v, f in zip(tt.view, tt.feat)]).tobytes()


def test_feature_colors_alone_change_nothing_else(windows, plain, unmasked):
    from orthosfm_amd.pipeline import join_background, tracks_from_images
    tt0, col0, _ = unmasked
    tt, colors, info = tracks_from_images(windows, device=0, verify=True, max_image_size=LIMIT, options=_options(), feature_colors=True)
    join_background()
    _same_table(tt, tt0)
    assert colors.tobytes() == col0.tobytes() and info["mask"]["tracks_dropped"] == 0
    _, rgb = _restated_marks(plain, windows, [None] * 3, "reference")
    assert info["feature_rgb"].tobytes() == np.stack([rgb[v][f] for v, f in zip(tt.view, tt.feat)]).tobytes()


def test_features_mode_equals_the_old_way_on_the_kept_rows(windows, plain):
    """The old way: extract, delete the masked-out rows on the host, set_view_features, one osfm_match_all batch,
    the track builder."""
    from orthosfm_amd import capi, tracks as T
    from orthosfm_amd.features import FeatureSetExtractor
    from orthosfm_amd.matching import HipExhaustiveMatching
    from orthosfm_amd.pipeline import TrackTable, join_background, tracks_from_images
    masks = _scene_masks()
    with FeatureSetExtractor(0, 160, 120) as ex:
        sets = [ex.extract(vc.chain(w, 1, LIMIT)[1]) for w in windows]
    marks = [mc.marks(m, mc.pixel_positions(fs.normalized, WINDOW[0]), "reference") for m, fs in zip(masks, sets)]
    sets = [mc.delete_rows(fs, (mk & 1) != 0) for fs, mk in zip(sets, marks)]
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
        status = ra["status"].copy()
    finally:
        m.close()
    want = TrackTable.from_mve(toff, tfeat, [fs.normalized for fs in sets], WINDOW[0], 3)
    tt, colors, info = tracks_from_images(windows, device=0, verify=True, max_image_size=LIMIT, options=_options(), masks=masks,
                                          mask_mode="features", mask_clamp="reference", feature_colors=True)
    join_background()
    print(f"features mode: {len(toff) - 1} tracks from {[len(fs) for fs in sets]} kept rows of {[len(p) for p in plain]}")
    assert len(toff) - 1 >= 5 and sum(len(fs) for fs in sets) < sum(len(p) for p in plain)
    assert info["pair_status"].tolist() == status.tolist()
    _same_table(tt, want)
    assert colors.tobytes() == tcol.tobytes()
    assert info["mask"]["tracks_dropped"] == 0
    assert [a + b for a, b in zip(info["mask"]["kept_sift"], info["mask"]["kept_surf"])] == [len(fs) for fs in sets]
    rgb = [mc.propagate_colors(w, mc.pixel_positions(fs.normalized, WINDOW[0])) for w, fs in zip(windows, sets)]
    assert info["feature_rgb"].tobytes() == np.stack([rgb[v][f] for v, f in zip(tt.view, tt.feat)]).tobytes()


def test_mixed_import_widths_are_refused(windows):
    from orthosfm_amd.pipeline import tracks_from_images
    mixed = [windows[0], np.ascontiguousarray(windows[1][:, :300]), windows[2]]
    with pytest.raises(ValueError, match="import width"):
        tracks_from_images(mixed, device=0, max_image_size=LIMIT, options=_options(), masks=[None, None, None])
    with pytest.raises(ValueError, match="import width"):
        tracks_from_images(mixed, device=0, max_image_size=LIMIT, options=_options(), feature_colors=True)
    with pytest.raises(ValueError, match="per image"):
        tracks_from_images(windows, device=0, max_image_size=LIMIT, options=_options(), masks=[None])


# ---- 6. save_project --------------------------------------------------------------------------------------------
def test_save_project_writes_the_propagated_colours(windows, plain, unmasked, tmp_path):
    from orthosfm_amd import formats as F, pipeline as P, synth
    import copy
    tt = copy.deepcopy(unmasked[0])              # the test gives tracks points: on a copy
    _, rgb = _restated_marks(plain, windows, [None] * 3, "reference")
    feature_rgb = np.stack([rgb[v][f] for v, f in zip(tt.view, tt.feat)])
    assert len(np.unique(feature_rgb)) > 8
    nt = tt.offsets.shape[0] - 1
    u = synth.uniform(3, 0x5A17 << 16, 3 * nt).reshape(nt, 3)
    tt.point[:, :3], tt.point[:, 3] = u - 0.5, 1.0
    tt.has_point[::2] = True
    res = P.Result(np.zeros((3, 8)), [], tt, [], P.Timings(), [])
    P.save_project(res, synth.MODEL_QUATERNION, str(tmp_path / "with"), feature_rgb=feature_rgb)
    P.save_project(res, synth.MODEL_QUATERNION, str(tmp_path / "without"))
    with pytest.raises(ValueError):
        P.save_project(res, synth.MODEL_QUATERNION, str(tmp_path / "bad"), feature_rgb=feature_rgb[:-1])
    tracks = F.mve_tracks_to_orthosfm(tt.offsets, np.stack([tt.view, tt.feat], axis=1), [p.normalized for p in plain],
                                      WINDOW[0], colors=rgb)
    for t, track in enumerate(tracks):
        track.point = tt.point[t] if tt.has_point[t] else None
    os.makedirs(tmp_path / "want")
    F.save_tracks_to_file(tracks, str(tmp_path / "want" / "tracks.txt"))
    F.save_points_to_ply(str(tmp_path / "want" / "sparse_cloud.ply"), tracks)
    for name in ("tracks.txt", "sparse_cloud.ply"):
        got, want = (tmp_path / "with" / name).read_bytes(), (tmp_path / "want" / name).read_bytes()
        assert got == want, name
        assert got != (tmp_path / "without" / name).read_bytes(), name
