"""Seeded images for the SIFT extraction tests.

An image is a sum of anisotropic Gaussian blobs of either sign on a mid-grey ground, with log-uniform sizes
and uniform angles, drawn from the repository's splitmix streams (orthosfm_amd.synth.uniform) and rendered to
8 bits.  A 3-channel case gives every blob its own colour.  A crop case cuts a window out of a larger canvas,
so that two crops that differ by an integer shift show the same structures.  EDGE_CASES are small images whose
octaves stand on the constants of the kernels (segments of 256 pixels, tiles of 32, a radius of 32, the 2-pixel bound of
the last octave), and the sweep cuts every accepted width and height up to 80 out of one image.

tests/golden/make_sift_golden.py runs the reference detector on every case and writes
tests/golden/sift_reference.npz; tests/sift_restatement.py restates the detector in numpy;
tests/test_sift_cases_cpu.py pins the restatement to the fixture and tests/test_sift_gpu.py holds the library
to both.
"""
import hashlib
import os
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from orthosfm_amd import synth

STREAM = 0x51F7 << 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_reference.npz")


@dataclass(frozen=True)
class Case:
    name: str
    width: int
    height: int
    channels: int
    blobs: int
    seed: int
    min_octave: int = 0
    sigma_lo: float = 1.0
    sigma_hi: float = 16.0
    crop: tuple = None            # (canvas width, canvas height, x0, y0): the image is a window of that canvas
    refused: bool = False         # the reference throws on this size
    descriptors: bool = True      # held to the orientation / descriptor checks
    faint: float = 0.0            # share of the blobs drawn at a twelfth of the amplitude: candidates that fail the contrast test
    samples: int = 3              # Sift::Options::num_samples_per_octave
    base_blur_sigma: float = 1.6  # Sift::Options::base_blur_sigma


CASES = [
    Case("base", 257, 190, 1, 300, 4),
    Case("up", 257, 190, 1, 300, 4, min_octave=-1),
    Case("rgb", 193, 143, 3, 180, 2),
    Case("many", 401, 299, 1, 3000, 15, sigma_hi=5.0, faint=0.93),
    Case("tiny", 40, 33, 1, 12, 4, sigma_hi=6.0, descriptors=False),
    Case("refused", 9, 9, 1, 3, 5, sigma_hi=3.0, refused=True, descriptors=False),
    # two windows of one canvas, shifted by SHIFT pixels (the matcher test)
    Case("crop_a", 160, 120, 1, 300, 5, crop=(260, 190, 10, 12)),
    Case("crop_b", 160, 120, 1, 300, 5, crop=(260, 190, 37, 29)),
]

# ---- image-shape edges of sift_kernels.hip and sift_api.hip; tests/test_sift_cases_cpu.py asserts what each one is
# there for.  Seeds are picked so that every octave of at least MIN_SIDE pixels a side holds a candidate.
_E = dict(descriptors=False)
EDGE_CASES = [
    # blur_rows_kernel stages 256 pixels and a halo: two exact segments and one (octaves 0 and 1), one exact segment
    Case("w512", 512, 35, 1, 6, 70, sigma_hi=6.0, **_E),
    Case("w256", 256, 35, 1, 6, 27, sigma_hi=6.0, **_E),
    # a second segment of 33 pixels, and one of 3, narrower than every blur radius of the defaults (4 to 9)
    Case("w289", 289, 33, 1, 12, 25, sigma_hi=6.0, **_E),
    Case("w259", 259, 33, 1, 6, 25, sigma_hi=6.0, **_E),
    # blur_cols_kernel works on 32 x 32 tiles: octaves of 64 x 65, 32 x 33 and 33 x 32
    Case("c64x65", 64, 65, 1, 48, 109, **_E),
    Case("c33x32", 33, 32, 1, 24, 31, **_E),
    # octave_sizes(): the smallest accepted side is 17 (the fifth octave is 2 pixels), 16 is refused
    Case("min40x17", 40, 17, 1, 6, 23, sigma_hi=6.0, **_E),
    Case("min17x40", 17, 40, 1, 6, 23, sigma_hi=6.0, **_E),
    Case("ref40x16", 40, 16, 1, 3, 5, sigma_hi=3.0, refused=True, **_E),
    Case("ref16x40", 16, 40, 1, 3, 5, sigma_hi=3.0, refused=True, **_E),
    # the largest side whose last octave is 2 pixels: extrema_blocks() == 0 there and nothing is launched
    Case("two40x32", 40, 32, 1, 24, 31, **_E),
    Case("two32x40", 32, 40, 1, 48, 46, **_E),
    Case("up17x19", 17, 19, 1, 6, 105, min_octave=-1, sigma_hi=6.0, **_E),
    # extrema_kernel numbers interior pixels in blocks of 256: 16 x 16 = 256 and 17 x 16 = 272 of them in octave 0
    Case("int18x18", 18, 18, 1, 6, 105, sigma_hi=6.0, **_E),
    Case("int19x18", 19, 18, 1, 24, 31, sigma_hi=6.0, **_E),
    # one sample per octave at the default base blur: the last blur step has sigma 1.6 sqrt(48) = 11.085 and a radius of
    # ceil(11.085 * 2.884) = 32 = kMaxRadius, which fills both LDS tiles; in the 80 x 70 of octave 0 columns 32 to 47 and rows
    # 32 to 37 read 32 pixels either way unclamped, every other pixel and every later octave reads clamped ones
    Case("r32", 80, 70, 1, 6, 161, sigma_hi=6.0, samples=1, **_E),
]
EDGE = [c.name for c in EDGE_CASES]
CASES += EDGE_CASES
MIN_SIDE = 8                      # below it no seed gave a candidate: every blur radius exceeds the octave, which is all border
RADIUS_REFUSED_SIGMA = 1.61       # with one sample per octave: a radius of 33
BY_NAME = {c.name: c for c in CASES}
SHIFT = (27, 17)                  # crop_b's origin minus crop_a's: a point at x in crop_a lies at x - SHIFT in crop_b

# Measured by tests/golden/make_sift_golden.py (it prints them; tests/test_sift_cases_cpu.py checks that they still
# hold): per case the largest |orientation(reference) - orientation(float64 restatement)| and the largest absolute
# element difference between the reference's descriptor and the float64 restatement's, over the clear keypoints --
# the size of "same algorithm, other rounding" -- and the number of ambiguous keypoints.
MEASURED = {
    # name: (d_ori, d_desc, ambiguous keypoints, keypoints)
    "base": (6.472e-07, 5.766e-07, 2, 106),
    "up": (8.438e-07, 5.766e-07, 2, 191),
    "rgb": (4.559e-07, 4.934e-07, 0, 68),
    "many": (6.666e-07, 6.407e-07, 4, 243),
    "crop_a": (6.363e-07, 4.385e-07, 0, 46),
    "crop_b": (3.570e-07, 5.136e-07, 0, 51),
}

# a keypoint is ambiguous when a peak decision of its orientation histogram has a relative margin below this:
# ten times the float32 summation bound of the largest window at the defaults, 37 x 37 samples
AMBIGUITY_BAND = 10.0 * 37 * 37 * 2.0 ** -24


def render(width, height, channels, blobs, seed, sigma_lo, sigma_hi, faint=0.0):
    """uint8 [height, width] or [height, width, 3]."""
    u = synth.uniform(seed, STREAM | 1, 9 * blobs).reshape(blobs, 9)
    acc = np.zeros((height, width, channels))
    for b in range(blobs):
        cx, cy = u[b, 0] * width, u[b, 1] * height
        s1 = sigma_lo * (sigma_hi / sigma_lo) ** u[b, 2]
        s2 = s1 * (0.5 + 0.5 * u[b, 3])
        th = np.pi * u[b, 4]
        amp = (0.15 + 0.35 * u[b, 5]) * (1.0 if b % 2 else -1.0) * (1.0 / 12.0 if (b % 100) < 100.0 * faint else 1.0)
        r = int(4.0 * s1) + 1
        x0, x1 = max(0, int(cx) - r), min(width, int(cx) + r + 1)
        y0, y1 = max(0, int(cy) - r), min(height, int(cy) + r + 1)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        dx, dy = xx - cx, yy - cy
        a = (np.cos(th) * dx + np.sin(th) * dy) / s1
        c = (-np.sin(th) * dx + np.cos(th) * dy) / s2
        g = amp * np.exp(-0.5 * (a * a + c * c))
        col = np.ones(channels) if channels == 1 else 0.4 + 0.6 * u[b, 6:9]
        acc[y0:y1, x0:x1, :] += g[:, :, None] * col[None, None, :]
    img = np.clip(np.floor((0.5 + acc) * 255.0 + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[:, :, 0] if channels == 1 else img)


@lru_cache(maxsize=None)
def image(name):
    """The case's image.  Cached: treat it as read-only."""
    c = BY_NAME[name]
    if c.crop:
        cw, ch, x0, y0 = c.crop
        img = render(cw, ch, c.channels, c.blobs, c.seed, c.sigma_lo, c.sigma_hi, c.faint)
        img = np.ascontiguousarray(img[y0:y0 + c.height, x0:x0 + c.width])
    else:
        img = render(c.width, c.height, c.channels, c.blobs, c.seed, c.sigma_lo, c.sigma_hi, c.faint)
    img.setflags(write=False)
    return img


def options(case):
    """The Sift::Options of a case, as the restatement takes them; a negative contrast threshold means 0.02 / samples."""
    import sift_restatement as sr
    f32 = np.float32
    return sr.Options(min_octave=case.min_octave, num_samples_per_octave=case.samples,
                      contrast_threshold=f32(0.02) / f32(case.samples), base_blur_sigma=f32(case.base_blur_sigma))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def timing_canvas(size=2048, blobs=90000, seed=77):
    """The dense canvas of tools/sift_timing.py."""
    return render(size, size, 1, blobs, seed, 1.0, 12.0)


def fixture(name):
    """The case's arrays of the fixture, by their short names."""
    return {k.split("/", 1)[1]: v for k, v in golden().items() if k.startswith(name + "/")}


def groups_of(keypoints, meta, min_octave):
    """Per keypoint the rows of `meta` (x, y, scale, orientation in generation order) that belong to it: the
    detector emits a keypoint's descriptors one after the other, and x, y and scale are exact functions of it."""
    import sift_restatement as sr
    opts = sr.Options(min_octave=min_octave)
    out, p = [], 0
    for kp in keypoints:
        x, y, s, _ = sr.generation_meta(kp, 0.0, opts)
        q = p
        while q < len(meta) and meta[q, 0] == x and meta[q, 1] == y and meta[q, 2] == s:
            q += 1
        out.append(range(p, q))
        p = q
    assert p == len(meta), "descriptor rows that belong to no keypoint"
    return out


@lru_cache(maxsize=None)
def restated(name):
    """(octaves, candidates, keypoints, float64 describe(), float32 describe()) of the restatement.  Cached."""
    import sift_restatement as sr
    c = BY_NAME[name]
    opts = options(c)
    octs = sr.scale_space(image(name), opts)
    cand = sr.extrema(octs)
    kps = sr.localise(octs, cand, opts)[0]
    d64 = sr.describe(octs, kps, opts, np.float64) if c.descriptors else None
    d32 = sr.describe(octs, kps, opts, np.float32) if c.descriptors else None
    return octs, cand, kps, d64, d32


# ---- the sweep: every accepted width at the full height and every accepted height at the full width, all cut from the
# top-left corner of one image, so that every clamp and every segment and tile bound is crossed one pixel at a time
SWEEP_SIDE = 80
SWEEP_SMALLEST = 17               # octave_sizes() refuses 16
SWEEP_SHAPES = ([(w, SWEEP_SIDE) for w in range(SWEEP_SMALLEST, SWEEP_SIDE + 1)]
                + [(SWEEP_SIDE, h) for h in range(SWEEP_SMALLEST, SWEEP_SIDE)])          # (w, h)
SWEEP_CHUNK = 16
SWEEP_CHUNKS = [SWEEP_SHAPES[i:i + SWEEP_CHUNK] for i in range(0, len(SWEEP_SHAPES), SWEEP_CHUNK)]


@lru_cache(maxsize=None)
def sweep_image():
    img = render(SWEEP_SIDE, SWEEP_SIDE, 1, 40, 9, 1.0, 8.0)
    img.setflags(write=False)
    return img


def sweep_cut(w, h, source=None):
    return np.ascontiguousarray((sweep_image() if source is None else source)[:h, :w])


def stage_hashes(images, dogs, cand, kps):
    """[(stage, SHA-256)] of one extraction: images[o][i] and dogs[o][i] per octave, candidates, keypoints."""
    out = []
    for o, (im, dg) in enumerate(zip(images, dogs)):
        out += [(f"octave {o} image {i}", sha(a)) for i, a in enumerate(im)]
        out += [(f"octave {o} DoG {i}", sha(a)) for i, a in enumerate(dg)]
    return out + [("candidates", sha(cand)), ("keypoints", sha(kps))]


@lru_cache(maxsize=None)
def sweep_restated(w, h):
    """stage_hashes of the restatement on the sweep's w x h cut.  Cached."""
    import sift_restatement as sr
    opts = sr.Options()
    octs = sr.scale_space(sweep_cut(w, h), opts)
    cand = sr.extrema(octs)
    return stage_hashes([o[1] for o in octs], [o[2] for o in octs], cand, sr.localise(octs, cand, opts)[0])


def measure(name):
    """The figures MEASURED records, from the fixture and the restatement."""
    _, _, kps, d64, d32 = restated(name)
    fx = fixture(name)
    assert kps.tobytes() == fx["keypoints"].tobytes()
    groups = groups_of(kps, fx["gen_meta"], BY_NAME[name].min_octave)
    fig = dict(d_ori=0.0, d_desc=0.0, ambiguous=0, several=0, f32_count_differs=0, f64_count_differs=0,
               keypoints=len(kps), clear=[])
    for k, rows in enumerate(groups):
        fig["several"] += len(rows) >= 2
        oris, margin, descs = d64[k]
        if margin < AMBIGUITY_BAND:
            fig["ambiguous"] += 1
            fig["clear"].append(False)
            continue
        fig["clear"].append(True)
        got = [(o, d) for o, d in zip(oris, descs) if d is not None]
        fig["f32_count_differs"] += sum(d is not None for d in d32[k][2]) != len(rows)
        if len(got) != len(rows):
            fig["f64_count_differs"] += 1
            continue
        for r, (o, d) in zip(rows, got):
            fig["d_ori"] = max(fig["d_ori"], abs(float(fx["gen_meta"][r, 3]) - float(o)))
            fig["d_desc"] = max(fig["d_desc"], float(np.abs(fx["gen_data"][r].astype(np.float64) - d).max()))
    assert fig["f64_count_differs"] == 0, f"{name}: the float64 restatement disagrees with the reference on a clear keypoint"
    return fig
