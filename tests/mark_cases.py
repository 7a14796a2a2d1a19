"""Seeded cases for the view marks (include/osfm_hip.h, "View masks and pixel colours") and a numpy restatement of
the three reference functions they stand for, written from the cited lines:

  * pixel_positions            matching_mve.cpp:461-463, imageWidth * (pos + 0.5) on BOTH axes, double, stored as float
  * is_pixel_masked_in         View::isPixelMaskedIn, src/data_structures/view.cpp:100-112: x clamped by rows - 1 and
                               y by cols - 1, then at<uchar>(Point(x, y)), which is row y, column x
  * propagate_colors           propagateColorsToTracks, src/util/common.cpp:289-315
  * filter_tracks_with_masks   filterTracksWithMasks, src/matching/matching.cpp:325-368

The reference reads past the mask where the swapped clamp leaves an index outside it; here that row is masked out
and flagged (mark bit 1), which is the one thing below that is this project's rule and not the reference's.
"""
from functools import lru_cache

import numpy as np

from orthosfm_amd import synth

STREAM = 0x3A5C << 16
MARK_IN, MARK_OUTSIDE = 1, 2
THRESHOLD = 16


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def pixel_positions(normalized, width):
    return (float(width) * (np.asarray(normalized, np.float32).astype(np.float64) + 0.5)).astype(np.float32)


def _index(v, hi):
    """(int)fmax(fmin(v, hi), 0): the float against the int bound, both as double."""
    return np.fmax(np.fmin(np.asarray(v, np.float32).astype(np.float64), float(hi)), 0.0).astype(np.int64)


def mask_indices(mask_shape, xy, clamp="reference"):
    """(column, row) the lookup computes."""
    rows, cols = mask_shape
    if clamp == "reference":
        return _index(xy[:, 0], rows - 1), _index(xy[:, 1], cols - 1)
    assert clamp == "image"
    return _index(xy[:, 0], cols - 1), _index(xy[:, 1], rows - 1)


def is_pixel_masked_in(mask, xy, clamp="reference", threshold=THRESHOLD):
    """(masked in, index outside the mask) per row; an index outside is not masked in."""
    rows, cols = mask.shape
    cx, cy = mask_indices(mask.shape, xy, clamp)
    outside = (cx >= cols) | (cy >= rows)
    value = mask[np.minimum(cy, rows - 1), np.minimum(cx, cols - 1)]
    return (value > threshold) & ~outside, outside


def marks(mask, xy, clamp="reference", threshold=THRESHOLD):
    """The mark byte per row; mask None: hasMask() is false and nothing is masked out."""
    if mask is None:
        return np.full(xy.shape[0], MARK_IN, np.uint8)
    inn, outside = is_pixel_masked_in(mask, xy, clamp, threshold)
    return (inn * MARK_IN + outside * MARK_OUTSIDE).astype(np.uint8)


def propagate_colors(image, xy):
    """uint8 [n, 3]: the pixel under the truncated position, x clamped by cols - 1 and y by rows - 1; a grey image
    gives its value three times."""
    rows, cols = image.shape[:2]
    px = image[_index(xy[:, 1], rows - 1), _index(xy[:, 0], cols - 1)]
    return np.ascontiguousarray(np.repeat(px[:, None], 3, axis=1) if image.ndim == 2 else px).astype(np.uint8)


def filter_tracks_with_masks(offsets, track_features, view_marks, has_mask):
    """keep bool [num_tracks]; view_marks[v]: the mark bytes of view v."""
    n = len(offsets) - 1
    if not any(has_mask):
        return np.ones(n, bool)
    keep = np.ones(n, bool)
    for t in range(n):
        for v, f in track_features[offsets[t]:offsets[t + 1]]:
            if has_mask[v] and not (view_marks[v][f] & MARK_IN):
                keep[t] = False
                break
    return keep


def delete_rows(fs, keep):
    """A features.FeatureSet / ViewFeatures with the rows where keep is False deleted: what OSFM_MARK_FEATURES is
    defined against."""
    from orthosfm_amd.features import Features, FeatureSet
    ns = len(fs.sift)
    ks, ku = keep[:ns], keep[ns:]
    part = lambda f, k: Features(*(np.ascontiguousarray(getattr(f, a)[k]) for a in
                                   ("descriptors", "positions", "normalized", "scale", "orientation", "colors")))
    return FeatureSet(part(fs.sift, ks), part(fs.surf, ku), np.ascontiguousarray(fs.positions[keep]),
                      np.ascontiguousarray(fs.normalized[keep]), np.ascontiguousarray(fs.colors[keep]))


# ---------------------------------------------------------------------------------------------------------------
# row cases
# ---------------------------------------------------------------------------------------------------------------
def _bytes(seed, k, shape, values=None):
    u = synth.uniform(seed, STREAM | k, int(np.prod(shape)))
    if values is None:
        return np.minimum(np.floor(u * 256.0), 255).astype(np.uint8).reshape(shape)
    return np.asarray(values, np.uint8)[np.minimum((u * len(values)).astype(int), len(values) - 1)].reshape(shape)


def _positions(seed, width, n, lo, hi, planted):
    """normalized [n + len(planted), 2] whose pixel positions spread over [lo, hi) on both axes, then the planted
    pixel positions."""
    u = synth.uniform(seed, STREAM | 9, 2 * n).reshape(n, 2)
    target = np.concatenate([lo + u * (hi - lo), np.asarray(planted, np.float64).reshape(-1, 2)])
    return np.ascontiguousarray((target / width - 0.5).astype(np.float32))


@lru_cache(maxsize=None)
def row_cases():
    """name -> dict(image, mask, normalized, width): the import image, the mask (None: no mask), the rows' normalised
    positions and the pixel width (the image's).  Mask values are drawn from {0, 16, 17, 255}."""
    vals = (0, 16, 17, 255)
    out = {}
    # landscape, mask of the image's size: x >= rows reads column rows - 1 with the reference's clamp; y beyond
    # rows - 1 (the width scales both axes) stays below cols - 1 and leaves the mask
    img = _bytes(1, 1, (30, 40, 3))
    mask = _bytes(1, 2, (30, 40), vals).copy()
    mask[12, 29], mask[12, 36] = 255, 0            # the planted row (36.5, 12.25): in by the reference, out by the image
    out["landscape"] = dict(image=img, mask=mask, width=40,
                            normalized=_positions(1, 40, 300, -4.0, 44.0, [(36.5, 12.25), (-2.5, 3.0), (5.0, -1.5), (10.0, 34.0)]))
    # square and in range: both clamps agree
    out["square_grey"] = dict(image=_bytes(2, 1, (32, 32)), mask=_bytes(2, 2, (32, 32), vals), width=32,
                              normalized=_positions(2, 32, 200, 0.0, 31.99, []))
    # a mask the caller resized to another size than the image
    out["other_size"] = dict(image=_bytes(3, 1, (30, 40, 3)), mask=_bytes(3, 2, (15, 20), vals), width=40,
                             normalized=_positions(3, 40, 200, -2.0, 42.0, []))
    # portrait: x clamped by rows - 1 runs past the last column
    out["portrait"] = dict(image=_bytes(4, 1, (40, 30)), mask=_bytes(4, 2, (40, 30), vals), width=30,
                           normalized=_positions(4, 30, 200, -2.0, 42.0, [(35.0, 5.0)]))
    out["no_mask"] = dict(image=_bytes(5, 1, (30, 40, 3)), mask=None, width=40, normalized=_positions(5, 40, 100, -4.0, 44.0, []))
    for c in out.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def expected_rows(case, clamp):
    """(pixel_xy, pixel_rgb, mark) of the restatement."""
    xy = pixel_positions(case["normalized"], case["width"])
    return xy, propagate_colors(case["image"], xy), marks(case["mask"], xy, clamp)


# ---------------------------------------------------------------------------------------------------------------
# track cases
# ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def track_cases():
    """name -> dict(offsets, features [n, 2] (view, feature), marks per view, has_mask per view).  Three views of
    7, 5 and 6 rows; view 1 has no mask and its marks are zero on purpose: they must not be read."""
    view_marks = [np.array([1, 0, 1, 1, 2, 1, 1], np.uint8), np.zeros(5, np.uint8), np.array([1, 1, 0, 1, 1, 3], np.uint8)]
    tracks = [[(0, 0), (1, 0), (2, 0)],          # every feature in
              [(0, 1), (1, 1), (2, 1)],          # exactly one masked-out feature (view 0, row 1)
              [(0, 2), (1, 2)],                  # in; view 1's zero marks are not read
              [(1, 3), (2, 2)],                  # out by view 2
              [(0, 4), (2, 3)],                  # out: an index outside the mask
              [(0, 5), (2, 5)],                  # in: bit 0 decides, whatever else is set
              [(1, 4), (1, 3)]]                  # only views without a mask
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    feats = np.array([f for t in tracks for f in t], np.int32)
    out = {"mixed": dict(offsets=offsets, features=feats, marks=view_marks, has_mask=[True, False, True]),
           "no_mask_anywhere": dict(offsets=offsets, features=feats, marks=view_marks, has_mask=[False, False, False]),
           "empty": dict(offsets=np.zeros(1, np.int64), features=np.zeros((0, 2), np.int32), marks=view_marks,
                         has_mask=[True, False, True])}
    # a seeded larger one
    sizes = (50, 40, 60)
    rnd = [(_bytes(7, 10 + v, (n,), (0, 1, 1, 1, 2, 3))) for v, n in enumerate(sizes)]
    u = synth.uniform(7, STREAM | 20, 400)
    big, at = [], 0
    for t in range(80):
        views = [v for v in range(3) if u[at + v] < 0.7] or [0, 2]
        big.append([(v, int(u[at + 3 + v] * sizes[v])) for v in views])
        at += 6 if at + 12 <= 400 else -at
    out["seeded"] = dict(offsets=np.concatenate([[0], np.cumsum([len(t) for t in big])]).astype(np.int64),
                         features=np.array([f for t in big for f in t], np.int32), marks=rnd, has_mask=[True, True, False])
    return out
