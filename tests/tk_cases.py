"""Seeded camera groups for the Tomasi-Kanade alignment tests.

The cameras are synth.make_ba_scene(0, C, ..., config_id=41).gt_cams -- a ring with +-30 degrees of tilt
and roll --, the points lie in the ball of radius 0.5, the observations are synth.project_quat plus
Gaussian noise; in a share of the tracks ONE observation is replaced by a uniformly random pixel; the
track order is shuffled and the positions pass through float32, as Feature::x / y do.

tests/test_tk_cases_cpu.py shows on the numpy restatement (tests/tk_restatement.py) that no decision of
any hypothesis of any case sits on a threshold, so that a float64 kernel must reproduce every one of
them; tests/test_tk_gpu.py then holds the library to the restatement on the same bytes.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from orthosfm_amd import synth

CONFIG_ID = 41


@dataclass(frozen=True)
class Case:
    name: str
    cameras: int
    tracks: int
    noise_px: float
    outliers: float
    seed: int
    width: int = 2048
    height: int = 2048
    offsets: float = 0.0
    max_iterations: int = 0
    expect: str = "ransac"          # "ransac" / "fallback" / "too_few"


CASES = [
    Case("exact40", 3, 40, 0.0, 0.0, 1),
    Case("n300", 3, 300, 0.5, 0.3, 2),
    Case("n2053", 3, 2053, 0.5, 0.3, 3),                    # several scoring tiles with a ragged tail
    Case("c5", 5, 300, 0.5, 0.2, 4),
    Case("c8", 8, 70, 0.5, 0.1, 9),
    Case("heavy", 3, 1000, 1.0, 0.45, 5),
    Case("rect", 3, 300, 0.5, 0.3, 10, width=1920, height=1080),
    Case("offs", 3, 300, 0.5, 0.3, 11, offsets=0.05),
    Case("it600", 3, 300, 0.5, 0.3, 12, max_iterations=600),
    Case("it1", 3, 300, 0.5, 0.3, 22, max_iterations=1),
    Case("n35", 3, 35, 0.5, 0.0, 13),                       # exactly enough consensus: 25 outside a sample of 10
    Case("n34", 3, 34, 0.5, 0.0, 14, expect="fallback"),
    Case("n10", 3, 10, 0.5, 0.0, 16, expect="fallback"),
    Case("n9", 3, 9, 0.5, 0.0, 17, expect="too_few"),
]
BY_NAME = {c.name: c for c in CASES}


def quat_to_mat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@lru_cache(maxsize=None)
def build(name):
    """(xy [N, C, 2] float64 holding float32 values, planted-outlier flag per track, ground-truth rotations
    [C, 3, 3] in the frame of camera 0).  Cached: treat the arrays as read-only."""
    c = BY_NAME[name]
    C, N, W, H, seed = c.cameras, c.tracks, c.width, c.height, c.seed
    st = CONFIG_ID << 32
    gt = synth.make_ba_scene(0, C, 10, seed=seed, config_id=CONFIG_ID, min_len=C, max_len=C, noise_px=0.0,
                             width=W, height=H).gt_cams.copy()
    if c.offsets:
        gt[:, 4:6] = c.offsets * (2.0 * synth.uniform(seed, st | 0x66, 2 * C).reshape(C, 2) - 1.0)
    d = synth.normal(seed, st | 0x61, 3 * N).reshape(N, 3)
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * (0.5 * np.cbrt(synth.uniform(seed, st | 0x62, N)))[:, None]
    xy = np.stack([synth.project_quat(pts, gt[k, :4], gt[k, 4], gt[k, 5], gt[k, 6], W, H) for k in range(C)], axis=1)
    xy += c.noise_px * synth.normal(seed, st | 0x63, 2 * N * C).reshape(N, C, 2)
    planted = np.zeros(N, dtype=bool)
    n_out = int(c.outliers * N)
    planted[:n_out] = True
    u = synth.uniform(seed, st | 0x64, 3 * N).reshape(N, 3)
    for t in range(n_out):
        xy[t, int(u[t, 0] * C)] = (u[t, 1] * W, u[t, 2] * H)
    perm = np.argsort(synth.uniform(seed, st | 0x65, N), kind="stable")
    xy = np.ascontiguousarray(xy[perm].astype(np.float32).astype(np.float64))
    planted = planted[perm]
    R = [quat_to_mat(gt[k, :4]) for k in range(C)]
    truth = np.array([R[0].T @ Rk for Rk in R])
    for a in (xy, planted, truth):
        a.setflags(write=False)
    return xy, planted, truth


def options(name):
    """Keyword arguments of tk_restatement.align / orthosfm_amd.tk.align for the case."""
    c = BY_NAME[name]
    return dict(seed=c.seed, group_id=0, max_iterations=c.max_iterations)


@lru_cache(maxsize=None)
def reference(name):
    """The restatement's answer for the case, with the margins the CPU test bounds.  Computed once per
    process and shared by the tests; treat it as read-only."""
    import tk_restatement
    c = BY_NAME[name]
    xy, _, _ = build(name)
    return tk_restatement.align(xy, c.width, c.height, detail=True, **options(name))
