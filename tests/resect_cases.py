"""Seeded cases of the affine-camera resection for tests/test_resect_cases_cpu.py, which
shows that they are fit to judge a kernel, and tests/test_resect_gpu.py, which holds the library to
tests/resect_restatement.py on them.

A case is one view's observations of synth.make_ba_scene(model, 6, N, min_len=6, max_len=6): every point is seen by
all six cameras, view 4 is the one resected.  The points handed over are the ground truth perturbed by 5e-4 (what a
triangulation leaves); planted outliers are positions shifted by 30 .. 300 pixels; positions go through float32.
The lists follow the scoring kernel's tile T and chunk K (osfm_resect_limits); the values they were made for:"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from orthosfm_amd import synth

import resect_restatement as R

TILE, CHUNK = 256, 16
VIEW = 4


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    outliers: float = 0.3           # planted fraction
    seed: int = 1                   # of the data and of the sampler
    stream_id: int = 0
    width: int = 2048
    height: int = 2048
    kind: str = "ball"              # "ball", "coplanar", "dup", "thin"
    cam_scale: float = 1.0
    noise_px: float = 0.3
    point_perturb: float = 5e-4
    model: int = 0
    opts: tuple = ()                # (name, value) pairs over the defaults

    def options(self):
        o = dict(self.opts)
        o.setdefault("seed", self.seed)
        return o


def _c(name, n, **kw):
    opts = tuple(sorted((k, kw.pop(k)) for k in list(kw) if k not in Case.__dataclass_fields__))
    return Case(name, n, opts=opts, **kw)


CASES = [
    _c("clean40", 40, outliers=0.0),
    _c("n255", TILE - 1), _c("n256", TILE), _c("n257", TILE + 1), _c("n513", 2 * TILE + 1),
    _c("h1", 120, max_iterations=1, seed=4), _c("h15", 120, max_iterations=CHUNK - 1),
    _c("h16", 120, max_iterations=CHUNK), _c("h17", 120, max_iterations=CHUNK + 1),
    _c("h33", 120, max_iterations=2 * CHUNK + 1, seed=36),      # seed: the winner is hypothesis 32, the last chunk's only one
    _c("out60", 600, outliers=0.6, seed=2),
    _c("coplanar", 80, kind="coplanar", outliers=0.0),
    _c("dup", 200, kind="dup", outliers=0.0),
    _c("mc_edge_ok", 50, outliers=0.4, noise_px=0.0, point_perturb=0.0, min_consensus=26),
    _c("mc_edge_no", 50, outliers=0.4, noise_px=0.0, point_perturb=0.0, min_consensus=27),
    _c("toofew11", 11, outliers=0.0), _c("toofew12", 12, outliers=0.0),
    _c("err1", 300, max_error_px=1.0), _c("err6", 300, max_error_px=6.0),
    _c("wide", 300, width=2048, height=1536),
    _c("scale_est", 300, cam_scale=1.25, estimate_scale=1), _c("scale_fix", 300, cam_scale=1.25, scale=1.25),
    _c("refit_off", 300, kind="thin", noise_px=0.0, point_perturb=0.0),
]
BY_NAME = {c.name: c for c in CASES}
THIN = 2e-4                         # thickness of the "thin" cloud relative to its extent
DUPLICATES = 60


@lru_cache(maxsize=None)
def build(name):
    """(points (N, 3), xy (N, 2), planted-outlier mask (N,), ground-truth rotation (3, 3) local -> world)."""
    from orthosfm_amd.pipeline import _cam_rotation
    c = BY_NAME[name]
    sc = synth.make_ba_scene(c.model, 6, c.n, min_len=6, max_len=6, noise_px=c.noise_px, config_id=200 + c.seed,
                             width=c.width, height=c.height)
    rng = np.random.default_rng(1000 + c.seed)
    sel = np.flatnonzero(sc.obs_camera == VIEW)
    assert np.array_equal(sc.obs_point[sel], np.arange(c.n))
    pts = sc.gt_points.copy()
    cam = sc.gt_cams[VIEW].copy()
    if c.kind == "ball" and c.cam_scale == 1.0:
        xy = sc.obs_xy[sel].copy()
    else:
        if c.kind == "coplanar":
            pts[:, 2] = 0.0
        elif c.kind == "thin":
            pts[:, 2] *= THIN
        elif c.kind == "dup":
            pts[1:DUPLICATES] = pts[0]
        cam[6 if c.model == 0 else 5] = c.cam_scale
        xy = synth._project(c.model, cam, pts, c.width, c.height) + c.noise_px * rng.normal(size=(c.n, 2))
        if c.kind == "dup":
            xy[1:DUPLICATES] = xy[0]
    X = pts + c.point_perturb * rng.normal(size=(c.n, 3))
    if c.kind == "coplanar":
        X[:, 2] = 0.0
    if c.kind == "dup":
        X[1:DUPLICATES] = X[0]
    planted = np.zeros(c.n, dtype=bool)
    k = int(c.outliers * c.n)
    if k:
        planted[rng.permutation(c.n)[:k]] = True
        ang = rng.uniform(0.0, 2.0 * np.pi, k)
        xy[planted] += (rng.uniform(30.0, 300.0, k) * np.array([np.cos(ang), np.sin(ang)])).T
    xy = xy.astype(np.float32).astype(np.float64)
    for a in (X, xy, planted):
        a.setflags(write=False)
    return X, xy, planted, _cam_rotation(c.model, cam)


@lru_cache(maxsize=None)
def reference(name):
    """The restatement's result, with its detail; computed once and shared."""
    c = BY_NAME[name]
    X, xy, _, _ = build(name)
    return R.resect(X, xy, c.width, c.height, stream_id=c.stream_id, detail=True, **c.options())
