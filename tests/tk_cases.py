"""Seeded camera groups for the Tomasi-Kanade alignment tests.

The cameras are synth.make_ba_scene(0, C, ..., config_id=41).gt_cams -- a ring with +-30 degrees of tilt
and roll --, the points lie in the ball of radius 0.5, the observations are synth.project_quat plus
Gaussian noise; in a share of the tracks ONE observation is replaced by a uniformly random pixel; the
track order is shuffled and the positions pass through float32, as Feature::x / y do.

tests/test_tk_cases_cpu.py shows on the numpy restatement (tests/tk_restatement.py) that no decision of
any hypothesis of any case sits on a threshold, so that a float64 kernel must reproduce every one of
them; tests/test_tk_gpu.py then holds the library to the restatement on the same bytes.

CASES pin the common path.  PATH_CASES (tests/test_tk_paths_gpu.py) sit where the kernels change path:
every camera count, the edges of the 256-track tiles and of the 16-hypothesis chunks, the sample sizes,
the fallback over several tiles, the consensus boundary, groups without a usable hypothesis, inputs
without a rank-3 factorisation, and the options away from their defaults.
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
    expect: str = "ransac"          # "ransac" / "fallback" / "too_few" / "degenerate"
    sample_size: int = 10
    min_consensus: int = 25
    max_error_px: float = 3.0
    probability: float = 0.999
    inlier_ratio: float = 0.7
    twin: float = 0.0               # camera 1 is camera 0 turned by this angle (rad) about its y axis, same offsets
    xy: str = ""                    # a hand-made measurement matrix: a key of HAND_MADE


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

# Where the kernels change path.  The seeds were searched on the restatement until tests/test_tk_cases_cpu.py held
# (if a case misses a condition its seed changes, never the condition); most held at the first one tried.  h17's is
# one whose winner is iteration 16, alone in the last chunk; last1's one whose winner holds a missing track last.
PATH_CASES = [
    # every instance of the scoring and mask kernels that CASES leaves out; c8w: three tiles with a ragged tail
    Case("c4", 4, 300, 0.5, 0.15, 31),
    Case("c6", 6, 300, 0.5, 0.15, 32),
    Case("c7", 7, 200, 0.5, 0.1, 33),
    Case("c8w", 8, 600, 0.5, 0.2, 34),
    # the edges of the 256-track tile
    Case("t255", 3, 255, 0.5, 0.3, 35),
    Case("t256", 3, 256, 0.5, 0.3, 36),
    Case("t257", 3, 257, 0.5, 0.3, 37),
    Case("t512", 3, 512, 0.5, 0.3, 38),
    # the edges of the 16-hypothesis chunk and of the selection's 256-thread stride
    Case("h15", 3, 300, 0.5, 0.3, 39, max_iterations=15),
    Case("h16", 3, 300, 0.5, 0.3, 39, max_iterations=16),
    Case("h17", 3, 300, 0.5, 0.3, 2639, max_iterations=17),
    Case("h256", 3, 300, 0.5, 0.3, 39, max_iterations=256),
    Case("h257", 3, 300, 0.5, 0.3, 39, max_iterations=257),
    # sample sizes
    Case("s5", 3, 300, 0.5, 0.3, 40, sample_size=5),                                   # 37 hypotheses
    Case("s16", 3, 300, 0.5, 0.1, 41, sample_size=16, max_iterations=64),
    Case("s32", 3, 300, 0.5, 0.02, 42, sample_size=32, max_iterations=64),
    Case("s4", 3, 300, 0.5, 0.3, 43, sample_size=4, max_iterations=16),
    Case("s32n32", 3, 32, 0.5, 0.0, 44, sample_size=32, min_consensus=0, max_iterations=16),
    Case("s32n31", 3, 31, 0.5, 0.0, 45, sample_size=32, expect="too_few"),
    # min_consensus = N is out of reach (a consensus set has at most N - sample_size tracks): the fallback, with any data
    Case("fb600", 3, 600, 0.5, 0.0, 46, max_iterations=20, min_consensus=600, expect="fallback"),
    Case("fb8", 8, 300, 0.5, 0.0, 47, max_iterations=20, min_consensus=300, expect="fallback"),
    Case("fb5", 5, 256, 0.5, 0.0, 48, max_iterations=20, min_consensus=256, expect="fallback"),
    # the noise-free data of exact40: every hypothesis has exactly the 30 tracks outside its sample
    Case("mc30", 3, 40, 0.0, 0.0, 1, min_consensus=30),
    Case("mc31", 3, 40, 0.0, 0.0, 1, min_consensus=31, expect="fallback"),
    # cameras 0 and 1 only 0.03 rad apart: isTomasiKanadeResultUsable refuses every hypothesis
    Case("twin3", 3, 300, 0.3, 0.0, 49, twin=0.03, expect="fallback"),
    Case("twin4", 4, 600, 0.3, 0.0, 50, twin=0.03, expect="fallback"),
    # no rank-3 measurement matrix
    Case("copies", 3, 40, 0.0, 0.0, 51, xy="copies", expect="degenerate"),
    Case("rank2", 3, 300, 0.0, 0.0, 52, xy="rank2", expect="degenerate"),
    # options away from their defaults; err1 / err6 on the data of n300
    Case("err1", 3, 300, 0.5, 0.3, 2, max_error_px=1.0),
    Case("err6", 3, 300, 0.5, 0.3, 2, max_error_px=6.0),
    # the winner's last-drawn sample track misses the 1 px bound under its own model: it is an inlier all the same, and
    # its error enters the mean through the hypothesis kernel's correction, not through the scoring kernel
    Case("last1", 3, 300, 0.5, 0.3, 65, max_error_px=1.0),
    Case("opt6", 3, 300, 0.5, 0.3, 53, sample_size=6, inlier_ratio=0.5, probability=0.99),      # 292 hypotheses
    # the formula gives 0.21 hypotheses: one is run (point 11)
    Case("clamp", 3, 300, 0.5, 0.0, 154, sample_size=4, probability=0.5, inlier_ratio=0.99),
]
BY_NAME = {c.name: c for c in CASES + PATH_CASES}


def quat_to_mat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _copies(c):
    """One track at integer pixel positions, c.tracks times: every normalised coordinate, every row sum and every
    row mean is exact, so the centred Gram matrix is exactly zero in numpy and on the device alike."""
    one = np.array([[700.0 + 130.0 * k, 900.0 - 70.0 * k] for k in range(c.cameras)])
    return np.tile(one, (c.tracks, 1, 1))


def _rank2(c):
    """xy = 1024 + a_t u + b_t v with integer a_t, b_t in +-200 and small integer u, v (C, 2): the measurement matrix
    has rank 2 exactly (every entry is an integer below 1024 in magnitude, exact in float32 and after normalisation)."""
    u = np.array([[2, 1], [-1, 2], [1, -1], [0, 1], [1, 0], [-2, 1], [1, 2], [-1, -1]], dtype=np.float64)[:c.cameras]
    v = np.array([[1, -2], [2, 1], [-1, -1], [1, 1], [0, -1], [1, 0], [-1, 1], [2, -1]], dtype=np.float64)[:c.cameras]
    st = CONFIG_ID << 32
    a = np.floor(401.0 * synth.uniform(c.seed, st | 0x67, c.tracks)) - 200.0
    b = np.floor(401.0 * synth.uniform(c.seed, st | 0x68, c.tracks)) - 200.0
    return 1024.0 + a[:, None, None] * u[None] + b[:, None, None] * v[None]


HAND_MADE = {"copies": _copies, "rank2": _rank2}


def build(name):
    """(xy [N, C, 2] float64 holding float32 values, planted-outlier flag per track, ground-truth rotations
    [C, 3, 3] in the frame of camera 0; for a hand-made xy no track is planted and there is no truth: None).
    Cached: treat the arrays as read-only."""
    return build_case(BY_NAME[name])


@lru_cache(maxsize=None)
def build_case(c):
    C, N, W, H, seed = c.cameras, c.tracks, c.width, c.height, c.seed
    if c.xy:
        xy = np.ascontiguousarray(HAND_MADE[c.xy](c))
        assert xy.shape == (N, C, 2) and np.array_equal(xy, xy.astype(np.float32).astype(np.float64))
        planted = np.zeros(N, dtype=bool)
        for a in (xy, planted):
            a.setflags(write=False)
        return xy, planted, None
    st = CONFIG_ID << 32
    gt = synth.make_ba_scene(0, C, 10, seed=seed, config_id=CONFIG_ID, min_len=C, max_len=C, noise_px=0.0,
                             width=W, height=H).gt_cams.copy()
    if c.offsets:
        gt[:, 4:6] = c.offsets * (2.0 * synth.uniform(seed, st | 0x66, 2 * C).reshape(C, 2) - 1.0)
    if c.twin:
        gt[1, :4] = synth.quat_mul(gt[0, :4], np.array([0.0, np.sin(0.5 * c.twin), 0.0, np.cos(0.5 * c.twin)]))
        gt[1, 4:] = gt[0, 4:]
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
    return case_options(BY_NAME[name])


def case_options(c):
    return dict(seed=c.seed, group_id=0, max_iterations=c.max_iterations, sample_size=c.sample_size,
                min_consensus=c.min_consensus, max_error_px=c.max_error_px, probability=c.probability,
                inlier_ratio=c.inlier_ratio)


def reference(name):
    """The restatement's answer for the case, with the margins the CPU test bounds.  Computed once per
    process and shared by the tests; treat it as read-only."""
    return reference_case(BY_NAME[name])


@lru_cache(maxsize=None)
def reference_case(c):
    import tk_restatement
    xy, _, _ = build_case(c)
    return tk_restatement.align(xy, c.width, c.height, detail=True, **case_options(c))
