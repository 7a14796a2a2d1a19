"""Seeded images for the SURF extraction tests: the images of tests/sift_cases.py, one larger image whose keypoints
reach the fourth octave, hand-placed descriptors on it, and a mirrored image whose response maps hold exact ties.

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
    source: str                   # the case of sift_cases whose image this is, or "big"
    width: int
    height: int
    channels: int
    counts: tuple = None          # (candidates, keypoints, descriptors) the reference gives, where the case pins them
    upright: bool = False
    contrast_threshold: float = 500.0


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
]
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


def generation_rows(gen):
    """The entries of generate() that became descriptors, in generation order."""
    return [g for g in gen if g is not None and g["status"]]


def measure(name):
    gen = restated(name)[4]
    with_ori = [g for g in gen if g is not None]
    return sum(bool(g["ambiguous"]) for g in with_ori), len(with_ori)
