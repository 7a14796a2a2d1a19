"""Seeded images for the SURF extraction tests: the images of tests/sift_cases.py, one larger image whose keypoints
reach the fourth octave, hand-placed descriptors on it, a mirrored image whose response maps hold exact ties, small
images on the loop bounds of the summed-area kernels and at the smallest sizes that give anything (source "edge"), and
a sweep that cuts every width and height up to 80 out of one image.

tests/golden/make_surf_golden.py runs the reference detector on every case and writes
tests/golden/surf_reference.npz; tests/surf_restatement.py restates the detector in numpy;
tests/test_surf_cases_cpu.py pins the restatement to the fixture and tests/test_surf_gpu.py holds the library to both.
"""
import os
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import sift_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surf_reference.npz")


@dataclass(frozen=True)
class Case:
    name: str
    source: str                   # the case of sift_cases whose image this is, or "big", "tie", "edge"
    width: int
    height: int
    channels: int
    counts: tuple = None          # (candidates, keypoints, descriptors) the reference gives, where the case pins them
    upright: bool = False
    contrast_threshold: float = 500.0
    blobs: tuple = None           # source "edge": sift_cases.render(width, height, 1, blobs, seed, 1.0, sigma_hi) of (blobs, seed, sigma_hi)


CASES = [
    Case("base", "base", 257, 190, 1, (278, 152, 49)),
    Case("rgb", "rgb", 193, 143, 3, (151, 67, 12)),
    Case("many", "many", 401, 299, 1, (1261, 85, 54)),
    Case("tiny", "tiny", 40, 33, 1, (11, 1, 0)),
    Case("nothing", "refused", 9, 9, 1, (0, 0, 0)),
    Case("crop_a", "crop_a", 160, 120, 1, (None, None, 12)),
    Case("crop_b", "crop_b", 160, 120, 1, (None, None, 9)),
    Case("big", "big", 449, 417, 1, (843, 349, 179)),
    Case("upright", "base", 257, 190, 1, upright=True),
    Case("tie", "tie", 161, 120, 1, (127, 79, 16)),
    # ---- image-shape edges of surf_kernels.hip; tests/test_surf_cases_cpu.py asserts what each one is there for
    # sat_rows_kernel walks a row 256 pixels at a time: one, two and three rounds that end on the segment, one pixel past it
    Case("w256", "edge", 256, 37, 1, (37, 3, 0), blobs=(11, 1, 6.0)),
    Case("w512", "edge", 512, 37, 1, (78, 12, 0), blobs=(23, 1, 6.0)),
    Case("w513", "edge", 513, 37, 1, (81, 10, 0), blobs=(23, 1, 6.0)),
    Case("w769", "edge", 769, 37, 1, (123, 17, 0), blobs=(35, 1, 6.0)),
    # sat_cols_kernel adds eight rows a round: 128 rounds and a tail of 7
    Case("tall", "edge", 37, 1031, 1, (138, 21, 0), blobs=(47, 1, 6.0)),
    # the residues of h % 8 no other case has (2, 4, 5), and a small height with no tail
    Case("h42", "edge", 45, 42, 1, (7, 0, 0), blobs=(3, 1, 6.0)),
    Case("h44", "edge", 45, 44, 1, (6, 1, 0), blobs=(3, 1, 6.0)),
    Case("h45", "edge", 44, 45, 1, (8, 1, 0), blobs=(3, 1, 6.0)),
    Case("h48", "edge", 45, 48, 1, (7, 1, 0), blobs=(3, 1, 6.0)),
    # the smallest sizes of SMALLEST, per dimension
    Case("resp_w", "edge", 11, 24, 1, (0, 0, 0), blobs=(3, 1, 6.0)),
    Case("resp_h", "edge", 24, 11, 1, (0, 0, 0), blobs=(3, 1, 6.0)),
    Case("cand_w", "edge", 17, 40, 1, (1, 0, 0), blobs=(3, 1, 6.0)),
    Case("cand_h", "edge", 40, 17, 1, (1, 0, 0), blobs=(3, 1, 6.0)),
    Case("desc_w", "edge", 63, 70, 1, (27, 7, 1), blobs=(14, 34, 10.0)),
    Case("desc_h", "edge", 70, 63, 1, (20, 10, 1), blobs=(14, 36, 10.0)),
]
EDGE = [c.name for c in CASES if c.source == "edge"]
LONG = ("tall",)                  # cases that get a context of their own on the device

# The smallest width and height (the other side large enough) at which the detector gives a first non-zero response, a
# first candidate and a first descriptor, found with the restatement and held by tests/test_surf_cases_cpu.py:
#   * response: octave 0, sample 0 has a 3-pixel filter and a border of 5, and keeps x with 5 <= x and x + 5 < w: w = 11;
#   * candidate: samples 1 and 2 alone are searched; sample 1 has a 5-pixel filter and a border of 8: w = 17;
#   * descriptor: the smallest scale a keypoint gets is 2 (the 5-pixel filter), descriptor_computation keeps
#     31 <= x and x + 31 < w, so w = 63.  It keeps 31 <= y and y + 31 <= h: at h = 62 only y == 31.0f passes, which no
#     seed tried gave, so the first height with a descriptor is 63 as well.
# The image of every such case, less its last column or row, gives none.
SMALLEST = {"response": 11, "candidate": 17, "descriptor": 63}


def capable_octaves(width, height):
    """The octaves that can hold a candidate at this size: those whose sample 1 (the smaller of the two searched) has a
    computed response at an interior position of its map."""
    import surf_restatement as sr
    out = []
    for o in range(4):
        fs = sr.filter_size(o, 1)
        border = fs + fs // 2 + 1
        ok = True
        for n in (width, height):
            at = np.arange(0, n, 2 ** o)
            valid = np.nonzero((at >= border) & (at + border < n))[0]
            ok &= bool(((valid >= 1) & (valid <= len(at) - 2)).any())
        if ok:
            out.append(o)
    return out


BY_NAME = {c.name: c for c in CASES}
SHIFT = sc.SHIFT

# Measured by tests/golden/make_surf_golden.py (it prints them; tests/test_surf_cases_cpu.py checks that they still
# hold): per case the keypoints with an orientation sample within AMBIGUITY_ULPS float ulps of a window bound, of the
# keypoints that pass descriptor_orientation's margin test.
MEASURED = {
    # name: (ambiguous keypoints, keypoints with an orientation)
    "base": (0, 91),
    "rgb": (0, 25),
    "many": (0, 70),
    "tiny": (0, 0),
    "nothing": (0, 0),
    "crop_a": (0, 27),
    "crop_b": (0, 19),
    "big": (1, 240),
    "upright": (0, 91),
    "tie": (0, 44),
    "w256": (0, 0),
    "w512": (0, 1),
    "w513": (0, 1),
    "w769": (0, 2),
    "tall": (0, 0),
    "h42": (0, 0),
    "h44": (0, 0),
    "h45": (0, 0),
    "h48": (0, 0),
    "resp_w": (0, 0),
    "resp_h": (0, 0),
    "cand_w": (0, 0),
    "cand_h": (0, 0),
    "desc_w": (0, 1),
    "desc_h": (0, 2),
}

FORCED_SCALES = (1, 2, 6, 13)
FORCED_KINDS = ("interior", "upright", "left", "right", "top", "bottom", "rejected")


@lru_cache(maxsize=None)
def forced():
    """float32 rows (x, y, scale, orientation, upright) on the image of `big`, FORCED_KINDS per scale of FORCED_SCALES:
    in the interior, and on each margin of descriptor_computation's test at 45 degrees."""
    w, h = BY_NAME["big"].width, BY_NAME["big"].height
    q = np.float32(np.pi / 4)
    rows = []
    for s in FORCED_SCALES:
        m = 15 * s + 1
        rows += [(224.3, 208.6, s + 0.25, 0.7, 0), (224.3, 208.6, s + 0.25, 0.7, 1),
                 (m, 208.5, s + 0.25, q, 0), (w - m - 0.5, 208.5, s + 0.25, q, 0),
                 (224.5, m, s + 0.25, q, 0), (224.5, h - m, s + 0.25, -q, 0),
                 (m - 0.5, 208.5, s + 0.25, q, 0)]
    a = np.array(rows, np.float32)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def image(name):
    """The case's image.  Cached: treat it as read-only."""
    c = BY_NAME[name]
    if c.source == "big":
        img = sc.render(449, 417, 1, 600, 4, 1.0, 24.0)
        img.setflags(write=False)
        return img
    if c.source == "tie":
        # mirrored about the axis between its two middle rows: box sums are integers, so the maps of octave 0 are
        # equal in rows 59 and 60 and the two-row maximum of a blob on the axis ties; the detector rejects both rows
        top = sc.render(c.width, c.height // 2, 1, 120, 10, 1.0, 8.0)
        img = np.ascontiguousarray(np.vstack([top, top[::-1]]))
        img.setflags(write=False)
        return img
    if c.source == "edge":
        img = sc.render(c.width, c.height, 1, c.blobs[0], c.blobs[1], 1.0, c.blobs[2])
        img.setflags(write=False)
        return img
    return sc.image(c.source)


@lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def fixture(name):
    """The case's arrays of the fixture, by their short names."""
    return {k.split("/", 1)[1]: v for k, v in golden().items() if k.startswith(name + "/")}


def fixture_trig(name):
    """{orientation bytes: (sin, cos)} as the C library of the fixture's generator gave them."""
    fx = fixture(name)
    return {m[3].tobytes(): (t[0], t[1]) for m, t in zip(fx["gen_meta"], fx["gen_trig"])}


def local_trig_is_the_fixtures(name):
    import surf_restatement as sr
    return all(sr.sinf(np.frombuffer(k, np.float32)[0]).tobytes() == s.tobytes()
               and sr.cosf(np.frombuffer(k, np.float32)[0]).tobytes() == c.tobytes() for k, (s, c) in fixture_trig(name).items())


@lru_cache(maxsize=None)
def restated(name, fixture_trig_values=False):
    """(summed-area table, maps, candidates, keypoints, generate()) of the restatement.  Cached: read-only."""
    import surf_restatement as sr
    c = BY_NAME[name]
    sat = sr.integral(sr.grey_of(image(name)))
    maps = sr.response_maps(sat)
    cand = sr.extrema(maps)
    kps = sr.localise(maps, cand, c.width, c.height, c.contrast_threshold)
    gen = sr.generate(sat, kps, c.upright, fixture_trig(name) if fixture_trig_values else None)
    return sat, maps, cand, kps, gen


# ---- the sweep: every width at the full height and every height at the full width (no size is refused), all cut from
# the top-left corner of the image of sift_cases' sweep: every `x + border >= w` of every octave and sample is crossed
SWEEP_SIDE = sc.SWEEP_SIDE
SWEEP_SHAPES = ([(w, SWEEP_SIDE) for w in range(1, SWEEP_SIDE + 1)] + [(SWEEP_SIDE, h) for h in range(1, SWEEP_SIDE)])   # (w, h)
SWEEP_CHUNK = 20
SWEEP_CHUNKS = [SWEEP_SHAPES[i:i + SWEEP_CHUNK] for i in range(0, len(SWEEP_SHAPES), SWEEP_CHUNK)]


def stage_hashes(maps, cand, kps):
    """[(stage, SHA-256)] of one extraction: the 16 response maps with their shapes, candidates, keypoints."""
    out = [(f"octave {o} sample {k} {maps[o][k].shape}", sc.sha(maps[o][k])) for o in range(4) for k in range(4)]
    return out + [("candidates", sc.sha(cand)), ("keypoints", sc.sha(kps))]


@lru_cache(maxsize=None)
def sweep_restated(w, h, **plant):
    """stage_hashes of the restatement on the sweep's w x h cut.  Cached."""
    import surf_restatement as sr
    maps = sr.response_maps(sr.integral(sc.sweep_cut(w, h)), **plant)
    cand = sr.extrema(maps)
    return stage_hashes(maps, cand, sr.localise(maps, cand, w, h))


def generation_rows(gen):
    """The entries of generate() that became descriptors, in generation order."""
    return [g for g in gen if g is not None and g["status"]]


def measure(name):
    gen = restated(name)[4]
    with_ori = [g for g in gen if g is not None]
    return sum(bool(g["ambiguous"]) for g in with_ori), len(with_ori)
