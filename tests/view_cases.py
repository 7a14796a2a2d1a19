"""Seeded cases for the view front end (include/osfm_hip.h, "View front end") and a numpy restatement of its halving
chain.

  * halve / chain restate mve::image::rescale_half_size<uint8_t> and the two loops of bundler::Features::compute
    and downscale_image in float32, operation for operation -- not in the integer form the kernel uses.
    tests/golden/make_halve_golden.py runs the reference on every image of halve_images() and writes
    tests/golden/halve_reference.npz; tests/test_view_cases_cpu.py pins the restatement to it.
  * sift_pool / surf_pool are descriptor values on every rounding boundary of osfm_quantize_sift / osfm_quantize_surf
    and outside their range; bank_case builds views of them for the hand-off kernels.
"""
import os
from functools import lru_cache

import numpy as np

from orthosfm_amd import synth

STREAM = 0x71E3 << 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halve_reference.npz")

HALVE_SHAPES = [(2, 2, 1), (3, 2, 1), (2, 3, 3), (5, 7, 3), (64, 64, 1), (65, 63, 3), (257, 190, 1),          # (w, h, c)
                # halve_grey8_kernel (grey, w % 8 == 0) on its edges: one quad per row at even and odd height, odd
                # heights at 2 and 3 quads, 9 x 29 = 261 work items (two workgroups, the second all but empty), 33 quads
                (8, 2, 1), (8, 3, 1), (16, 5, 1), (24, 7, 1), (72, 57, 1), (264, 3, 1)]
GREY8_SHAPES = [s for s in HALVE_SHAPES if s[2] == 1 and s[0] % 8 == 0]
# grey chains (w, h, halvings), every step of which is in the fixture: 72 -> 36 -> 18 -> 9 (the 8-byte kernel, then the
# general one twice), 132 -> 66 -> 33 -> 17 (the general one throughout) and 143 -> 72 -> 36 -> 18 (general, 8-byte at
# an odd height, general)
HALVE_CHAINS = [(72, 57, 3), (132, 80, 3), (143, 10, 3)]
REFUSED_SHAPE = (1, 5, 1)


def _random_image(w, h, c, seed):
    u = synth.uniform(seed, STREAM | 1, w * h * c)
    img = np.minimum(np.floor(u * 256.0), 255).astype(np.uint8).reshape(h, w, c)
    return np.ascontiguousarray(img[:, :, 0] if c == 1 else img)


@lru_cache(maxsize=None)
def halve_images():
    """name -> uint8 image.  Per shape a seeded random image; 2 x 2 patches whose sums are 1, 2 and 3 mod 4 (small and
    near the top of the range, where round-to-nearest and round-down part); all-255 images on both kernel paths."""
    out = {}
    for i, (w, h, c) in enumerate(HALVE_SHAPES):
        out[f"random_{w}x{h}x{c}"] = _random_image(w, h, c, 11 + i)
    for r, patch in {1: (1, 0, 0, 0), 2: (1, 1, 0, 0), 3: (1, 1, 1, 0)}.items():
        out[f"sum{r}_low"] = np.array(patch, np.uint8).reshape(2, 2)
        out[f"sum{r}_high"] = (np.array(patch, np.uint8) + 254 - (r == 3)).astype(np.uint8).reshape(2, 2)
    # the same patches inside a wider image (64 wide: the 8-byte path of the kernel)
    wide = _random_image(64, 64, 1, 31).copy()
    wide[0:2, 0:6] = [[1, 0, 1, 1, 1, 1], [0, 0, 0, 0, 1, 0]]
    wide[62:64, 58:64] = [[255, 254, 255, 255, 255, 255], [254, 254, 254, 254, 255, 254]]
    out["patches_64x64x1"] = wide
    out["all255_5x7x3"] = np.full((7, 5, 3), 255, np.uint8)
    out["all255_64x64x1"] = np.full((64, 64), 255, np.uint8)
    for a in out.values():
        a.setflags(write=False)
    return out


def chain_name(w, h, step):
    return f"chain_{w}x{h}_step{step}"


@lru_cache(maxsize=None)
def chain_images():
    """(w, h, halvings) -> the seeded random grey image a chain of HALVE_CHAINS starts from."""
    out = {}
    for i, (w, h, n) in enumerate(HALVE_CHAINS):
        out[w, h, n] = _random_image(w, h, 1, 51 + i)
        out[w, h, n].setflags(write=False)
    return out


def takes_grey8(w, c):
    """launch_halve's choice of kernel."""
    return c == 1 and w % 8 == 0


@lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def halve(img, round_down=False, plant_drop_last_row=False):
    """rescale_half_size<uint8_t>: (w + 1) >> 1 by (h + 1) >> 1, the last column / row replicated for odd sizes, a
    pixel (uchar)(0.25f a + 0.25f b + 0.25f c + 0.25f d + 0.5f) in float32.  round_down: a planted error (no + 0.5f);
    plant_drop_last_row: another (at an odd height the last row is not repeated: the row above takes its place)."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    if w < 2 or h < 2:
        raise ValueError("Input image too small for half-sizing")
    ow, oh = (w + 1) >> 1, (h + 1) >> 1
    x0, y0 = 2 * np.arange(ow), 2 * np.arange(oh)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    if plant_drop_last_row and h % 2:
        y1[-1] = h - 2
    f = img.astype(np.float32)
    q = np.float32(0.25)
    v = q * f[y0][:, x0]
    v = (v + q * f[y0][:, x1]).astype(np.float32)
    v = (v + q * f[y1][:, x0]).astype(np.float32)
    v = (v + q * f[y1][:, x1]).astype(np.float32)
    if not round_down:
        v = (v + np.float32(0.5)).astype(np.float32)
    return np.ascontiguousarray(v.astype(np.uint8))


def chain(img, downscale_factor=1, max_image_size=6_000_000):
    """(import image, feature image, halvings): downscale_image's downscale_factor - 1 halvings, then
    bundler::Features::compute's while (width * height > max_image_size); max_image_size <= 0: no limit."""
    img = np.asarray(img)
    n = 0
    for _ in range(1, downscale_factor):
        img, n = halve(img), n + 1
    imported = img
    while max_image_size > 0 and img.shape[1] * img.shape[0] > max_image_size:
        img, n = halve(img), n + 1
    return imported, img, n


# ---------------------------------------------------------------------------------------------------------------
# hostile descriptor values for the hand-off kernels
# ---------------------------------------------------------------------------------------------------------------
def _around(x, ulps=2):
    """float32(x) and its neighbours within `ulps` ulps."""
    out = [np.float32(x)]
    lo = hi = np.float32(x)
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


@lru_cache(maxsize=None)
def sift_pool():
    """Every k / 255, the floats within 2 ulps of every rounding boundary (k + 0.5) / 255, and values outside [0, 1]."""
    v = []
    for k in range(256):
        v.append(np.float32(k) / np.float32(255))
        v += _around((k + 0.5) / 255.0)
    v += [np.float32(x) for x in (-0.0, -0.25, -1e-30, -3.0, 1.0000001, 1.5, 7.0, np.inf, 1e-40, 0.0, 1.0)]
    a = np.array(v, np.float32)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def surf_pool():
    """Every +-k / 127, the floats within 2 ulps of +-(k + 0.5) / 127, exactly +-1 and values beyond."""
    v = []
    for k in range(128):
        for sgn in (1.0, -1.0):
            v.append(np.float32(sgn * k) / np.float32(127))
            v += _around(sgn * (k + 0.5) / 127.0)
    v += [np.float32(x) for x in (1.0, -1.0, 1.0000001, -1.0000001, 2.5, -2.5, np.inf, -np.inf, -0.0, 1e-40, -1e-40)]
    a = np.array(v, np.float32)
    a.setflags(write=False)
    return a


SPECIAL_PATTERNS = ("none", "first", "block_edge", "last", "all")
ROW_COUNTS = (0, 1, 255, 256, 257, 513)     # around kRowsPerBlock = 256


def _special_rows(pattern, n):
    rows = {"none": [], "first": [0], "block_edge": [255, 256], "last": [n - 1], "all": list(range(n))}[pattern]
    return sorted({r for r in rows if 0 <= r < n})


def bank_case(n_sift, n_surf, pattern, seed):
    """(sift [n_sift, 128], surf [n_surf, 64], positions [n_sift + n_surf, 2]) float32.  SIFT rows walk through the
    pool in order, so that 13 rows hold every value of it; rows that are not special take the values that quantise
    below 128 only, and special rows carry one value above 127 in any case."""
    pool = sift_pool()
    low = pool[pool < np.float32(127.25 / 255.0)]
    special = set(_special_rows(pattern, n_sift))
    sift = np.zeros((n_sift, 128), np.float32)
    at = [seed * 17, seed * 29]
    for r in range(n_sift):
        src, k = (pool, 0) if r in special else (low, 1)
        sift[r] = src[(at[k] + np.arange(128)) % src.size]
        at[k] += 128
        if r in special:
            sift[r, r % 128] = np.float32(200.0 / 255.0)
    sp = surf_pool()
    surf = sp[(seed * 13 + np.arange(n_surf * 64)) % sp.size].reshape(n_surf, 64).astype(np.float32)
    n = n_sift + n_surf
    pos = (synth.uniform(seed, STREAM | 2, 2 * max(n, 1))[:2 * n].reshape(n, 2) - 0.5).astype(np.float32)
    return sift, surf, pos


def permutation(kind, n, seed):
    """None, the identity, or a seeded shuffle of range(n)."""
    if kind == "null":
        return None
    if kind == "identity":
        return np.arange(n, dtype=np.int32)
    return np.argsort(synth.uniform(seed, STREAM | 3, max(n, 1))[:n], kind="stable").astype(np.int32)
