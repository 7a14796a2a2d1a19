"""Seeded scenes with exact depth for the dense plane sweep (tests/dense_restatement.py is the definition;
tests/test_dense_cases_cpu.py checks the cases, tests/test_dense_gpu.py holds the library to them).

The blob texture of refine_cases.texture lies on planes Z = a X + b Y + c of the world (one texture per plane; a
plane may be bounded in X: a strip in front of another plane).  A view is an affine camera P = [A | t]; its pixel x
looks along the ray B (x - t) + z d, which meets a plane at a depth known in closed form, so every view is rendered
analytically -- the texture at the nearest hit, the smallest z -- and the exact depth of every pixel is known.
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import dense_restatement as dr
import refine_cases as rcs

# A pixel is ambiguous where the restatement's margin is below this band: the float32 sums of the device may decide
# it the other way.  1e-4 is the gap below which the prototype saw an adjacent index win by rounding (and ten times
# the 9e-6 by which a float32 emulation of the sums moved a score); test_dense_cases_cpu.py holds every case to at
# most AMBIGUOUS_SHARE of its tested pixels inside it.
AMBIGUITY_BAND = 1e-4
AMBIGUOUS_SHARE = 0.05

# The restatement against the exact depth, measured on the CPU (test_dense_cases_cpu.py measures again and holds
# them): the median |z - z_exact| in steps and the share within one step, over the OK pixels of every sweep.
MEASURED_CPU = {
    "slanted": {"median_steps": 0.1322, "within_one_step": 0.9921},
    "step": {"median_steps": 0.1205, "within_one_step": 0.9600},
}

# Agreement of the device with the restatement over the pixels OK in both and not ambiguous, all cases, measured
# once on an MI355X (tests/test_dense_gpu.py prints the figures): the largest |score| difference and the largest
# |z| difference in steps.
MEASURED = {"score": 3.171e-05, "depth_steps": 2.110e-03}       # both on radius1, whose 3 x 3 windows have the least to average
# Ten times the measured figures (another order of the float32 box sums), and never above the two ceilings beyond
# which the arithmetic is wrong rather than rounded: 1e-3 in score, 0.01 step in depth.
CEILINGS = {"score": 1e-3, "depth_steps": 0.01}
BOUNDS = {k: min(10.0 * MEASURED[k], CEILINGS[k]) if MEASURED[k] > 0.0 else CEILINGS[k] for k in CEILINGS}


@dataclass
class Plane:
    a: float
    b: float
    c: float
    seed: int
    x_range: tuple = None        # (X0, X1): the plane exists only there
    flat_left: float = None


@dataclass
class Sweep:
    ref: int
    sources: tuple
    z_min: float
    dz: float
    num_depths: int
    options: dict = field(default_factory=dict)
    expect: tuple = ()


@dataclass
class Case:
    name: str
    images: list
    P: np.ndarray                # [V, 2, 4]
    planes: list
    sweeps: list
    options: dict = field(default_factory=dict)
    fuse: bool = False
    paths: dict = field(default_factory=dict)

    def exact(self, v):
        """(depth [h, w], plane index [h, w]) of view v's pixels: the nearest hit, NaN / -1 without one."""
        h, w = self.images[v].shape[:2]
        return trace(dr.Geometry(self.P[v]), w, h, self.planes)[:2]


def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    return Rx @ Ry


def camera(width, height, yaw_deg=0.0, pitch_deg=0.0, scale=1.0, centre=(48.0, 40.0, 0.0), shift=(0.0, 0.0)):
    """P [2, 4] of a view that shows the world point `centre` at its middle (plus `shift` pixels).  yaw = pitch = 0
    and scale = 1 give A = (I | 0) exactly."""
    A = scale * _rot(np.deg2rad(yaw_deg), np.deg2rad(pitch_deg))[:2] if (yaw_deg or pitch_deg or scale != 1.0) else np.eye(3)[:2]
    t = np.array([(width - 1) / 2.0, (height - 1) / 2.0]) + np.asarray(shift, dtype=np.float64) - A @ np.asarray(centre, dtype=np.float64)
    return np.concatenate([A, t[:, None]], axis=1)


def trace(geo, w, h, planes):
    """Per pixel of a view: depth of the nearest hit, its plane, its world point."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    X0 = geo.point(xs, ys, 0.0)
    best = np.full((h, w), np.inf)
    which = np.full((h, w), -1, np.int64)
    for i, p in enumerate(planes):
        n = (-p.a, -p.b, 1.0)
        z = (p.c - (n[0] * X0[0] + n[1] * X0[1] + n[2] * X0[2])) / (n[0] * geo.d[0] + n[1] * geo.d[1] + n[2] * geo.d[2])
        hit = np.ones((h, w), bool)
        if p.x_range is not None:
            X = X0[0] + z * geo.d[0]
            hit = (X >= p.x_range[0]) & (X <= p.x_range[1])
        nearer = hit & (z < best)
        best[nearer], which[nearer] = z[nearer], i
    depth = np.where(which >= 0, best, np.nan)
    zz = np.where(which >= 0, best, 0.0)
    return depth, which, tuple(X0[j] + zz * geo.d[j] for j in range(3))


@lru_cache(maxsize=None)
def _texture(seed, flat_left):
    return rcs.texture(seed, 800, lo=(-50.0, -50.0), hi=(150.0, 130.0), flat_left=flat_left)


def render(P, w, h, planes, channels=1):
    _, which, X = trace(dr.Geometry(P), w, h, planes)
    v = np.zeros((h * w, 3))
    for i, p in enumerate(planes):
        sel = (which == i).ravel()
        if sel.any():
            v[sel] = _texture(p.seed, p.flat_left)(np.stack([X[0].ravel()[sel], X[1].ravel()[sel]], axis=1))
    acc = v.reshape(h, w, 3)
    if channels == 3:
        return np.ascontiguousarray(np.clip(np.floor((0.5 + acc) * 255.0 + 0.5), 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.clip(np.floor((0.5 + acc.mean(axis=2)) * 255.0 + 0.5), 0, 255).astype(np.uint8))


def plan(P, sizes, planes, ref, sources, pad=2.3, num_depths=None, dz_scale=1.0, z_shift=0.0):
    """z_min, dz, D of a sweep that covers the exact depths of the view: dz = 0.5 / max |e|."""
    gr = dr.Geometry(P[ref])
    emax = max(np.hypot(*gr.pair(dr.Geometry(P[s]))[2]) for s in sources)
    dz = dz_scale * 0.5 / max(emax, 1e-3)
    depth = trace(gr, sizes[ref][0], sizes[ref][1], planes)[0]
    lo, hi = float(np.nanmin(depth)), float(np.nanmax(depth))
    z_min = lo - pad * dz + z_shift
    D = int(np.ceil((hi + z_shift - z_min) / dz + pad)) + 1 if num_depths is None else num_depths
    return float(z_min), float(dz), D


def _build(name, cams, planes, sweeps, channels=None, options=None, fuse=False, paths=None, **plan_kw):
    """cams: [(w, h, P)]; sweeps: [(ref, sources, options, expect)] planned over the exact depths."""
    P = np.stack([c[2] for c in cams])
    sizes = [(c[0], c[1]) for c in cams]
    channels = channels or [1] * len(cams)
    images = [render(P[v], sizes[v][0], sizes[v][1], planes, channels[v]) for v in range(len(cams))]
    sw = []
    for ref, sources, o, expect in sweeps:
        z_min, dz, D = plan(P, sizes, planes, ref, sources, **plan_kw)
        sw.append(Sweep(ref, tuple(sources), z_min, dz, D, dict(o), tuple(expect)))
    return Case(name, images, P, planes, sw, dict(options or {}), fuse, dict(paths or {}))


SLANT = Plane(0.15, 0.10, -11.2, 101)


def _ring(n, w=96, h=80, centre=(48.0, 40.0, 0.0)):
    yaws = [0.0, 14.0, -12.0, 21.0, -19.0, 9.0, -7.0, 17.0, -16.0]
    pitches = [0.0, 3.0, -4.0, -2.0, 5.0, 8.0, -9.0, -6.0, 7.0]
    return [(w, h, camera(w, h, yaws[i], pitches[i], centre=centre)) for i in range(n)]


def _slanted():
    cams = _ring(4)
    sweeps = [(r, [s for s in range(4) if s != r], {}, (dr.OK, dr.BORDER)) for r in range(4)]
    return _build("slanted", cams, [SLANT], sweeps, options=dict(radius=2), fuse=True)


def _radius(name, R):
    return _build(name, _ring(3), [SLANT], [(0, [1, 2], {}, (dr.OK, dr.BORDER))], options=dict(radius=R))


def _odd_sizes():
    cams = [(97, 81, camera(97, 81)), (131, 70, camera(131, 70, 13.0, 3.0)), (90, 77, camera(90, 77, -15.0, -2.0))]
    return _build("odd_sizes", cams, [SLANT], [(0, [1, 2], {}, (dr.OK, dr.BORDER))], channels=[1, 3, 3])


def _border():
    W, H, R = 96, 80, 3
    # view 1 sees everything; view 2 is shifted so that what it sees of the reference depends on the depth; view 3
    # has the reference's own orientation and shows it 20 and 15 pixels over: exact integers, G = I, e = 0
    cams = [(W, H, camera(W, H)), (140, 120, camera(140, 120, 14.0, 3.0)), (W, H, camera(W, H, -13.0, -2.0, shift=(34.0, 0.0))),
            (W, H, camera(W, H, shift=(20.0, 15.0)))]
    touch = (W - 1 - 20 - R, H - 1 - 15 - R)     # its window ends on the last column and the last row of view 3
    sweeps = [(0, [1, 2, 3], dict(min_sources=2), (dr.OK, dr.BORDER, dr.NO_SOURCES, dr.RANGE_EDGE)),
              (0, [3, 1], dict(min_sources=2), (dr.OK, dr.NO_SOURCES))]
    c = _build("border", cams, [SLANT], sweeps, options=dict(radius=R), paths={"touch": touch})
    return c


def _flat():
    plane = Plane(0.15, 0.10, -11.2, 103, flat_left=30.0)
    return _build("flat", _ring(3), [plane], [(0, [1, 2], {}, (dr.OK, dr.FLAT))])


def _out_of_range():
    # the range ends eight steps in front of the surface
    c = _build("out_of_range", _ring(3), [SLANT], [(0, [1, 2], {}, ())], num_depths=12, z_shift=-60.0)
    c.sweeps[0].expect = (dr.RANGE_EDGE, dr.LOW_SCORE)
    return c


def _many_depths(max_depths):
    cams = _ring(3, 40, 36, centre=(48.0, 40.0, 0.0))
    c = _build("many_depths", cams, [SLANT], [(0, [1, 2], {}, (dr.OK,))], num_depths=max_depths, pad=120.0)
    return c


def _one_source():
    return _build("one_source", _ring(2, 64, 56), [SLANT], [(0, [1], dict(min_sources=1), (dr.OK,))])


def _eight_sources():
    return _build("eight_sources", _ring(9, 64, 56), [SLANT], [(0, list(range(1, 9)), dict(min_sources=8), (dr.OK,))])


STEP_PLANES = [Plane(0.05, 0.04, 4.0, 105), Plane(-0.04, 0.03, -14.0, 107, x_range=(30.0, 62.0))]


def _step():
    cams = _ring(4)
    sweeps = [(r, [s for s in range(4) if s != r], {}, (dr.OK,)) for r in range(4)]
    # Windows that straddle the strip's edge, or lie half in what another view cannot see, settle between the planes
    # and two views can agree on that; with all three other views required, within half a step, and scores of 0.9
    # the restatement emits no point farther than a step from the plane its pixel shows (test_dense_cases_cpu.py)
    return _build("step", cams, STEP_PLANES, sweeps, options=dict(min_score=0.9, consistency_tol=0.5, min_consistent=3), fuse=True)


def _empty():
    cams = [(1, 1, camera(1, 1))] + _ring(3)[1:]
    return _build("empty", cams, [SLANT], [(0, [1, 2], {}, (dr.BORDER,))])


MAX_DEPTHS = 256          # osfm_dense_limits' max_depths; test_dense_gpu.py checks that the library says the same

# The options tests/test_dense_pipeline_gpu.py hands to pipeline.densify on pipeline_scene(): those of `step`.
PIPELINE_OPTIONS = dict(min_score=0.9, consistency_tol=0.5, min_consistent=3)
# What densify's plan gives on that scene under the restatement (test_dense_cases_cpu.py measures again): the median
# |z - z_exact| in steps and the share within one step over the emitted points, and the points per plane.
MEASURED_CPU_PIPELINE = {"median_steps": 0.0416, "within_one_step": 1.0000, "points": (9711, 2342)}


@lru_cache(maxsize=None)
def pipeline_scene(width=160, height=128, num_points=40):
    """The two planes of `step` seen by four cameras of the quaternion model (ground truth, as an adjustment would
    leave them): dict of images, model, cam_params [4, 7], P [4, 2, 4], planes, points [40, 3] on the surfaces and
    visibility (every view sees every point)."""
    from orthosfm_amd import dense, synth
    yaws, pitches = [0.0, 14.0, -12.0, 21.0], [0.0, 3.0, -4.0, -2.0]
    centre = np.array([48.0, 40.0, 0.0])
    scale = width / 2.0                              # one pixel per world unit along x, height / width along y
    cams = np.zeros((4, 7))
    for v in range(4):
        R = _rot(np.deg2rad(yaws[v]), np.deg2rad(pitches[v]))          # world -> local
        A = np.stack([-width / (2.0 * scale) * R[0], -height / (2.0 * scale) * R[1]])
        t = np.array([(width - 1) / 2.0, (height - 1) / 2.0]) - A @ centre
        cams[v, :4] = synth.mat_to_quat(R.T)
        cams[v, 4:] = (2.0 * (t[0] / width - 0.5), 2.0 * (t[1] / height - 0.5), scale)
    P = dense.affine_cameras(synth.MODEL_QUATERNION, cams, width, height)
    images = [render(P[v], width, height, STEP_PLANES) for v in range(4)]
    X = trace(dr.Geometry(P[0]), width, height, STEP_PLANES)[2]
    u = rcs._u(301, 11, 2 * num_points).reshape(num_points, 2)
    ix, iy = (u[:, 0] * width).astype(np.int64), (u[:, 1] * height).astype(np.int64)
    points = np.stack([X[j][iy, ix] for j in range(3)], axis=1)
    return dict(images=images, model=synth.MODEL_QUATERNION, cam_params=cams, P=P, planes=STEP_PLANES, points=points,
                visibility=[np.arange(num_points)] * 4)

def cloud_accuracy(scene, points, view, pixel, dzs):
    """(median |z - z_exact| in steps, share within one step, points per plane) of a cloud over pipeline_scene()."""
    err, per_plane = [], np.zeros(len(scene["planes"]), np.int64)
    for v in np.unique(view):
        g = dr.Geometry(scene["P"][v])
        h, w = scene["images"][v].shape[:2]
        depth, which, _ = trace(g, w, h, scene["planes"])
        sel = view == v
        px = pixel[sel]
        err.append(np.abs(g.depth(tuple(points[sel].T)) - depth[px[:, 1], px[:, 0]]) / dzs[int(v)])
        per_plane += np.bincount(which[px[:, 1], px[:, 0]], minlength=per_plane.shape[0])
    e = np.concatenate(err) if err else np.zeros(0)
    return float(np.median(e)), float((e <= 1.0).mean()), tuple(int(n) for n in per_plane)


@lru_cache(maxsize=None)
def restated_pipeline():
    """What pipeline.densify computes on pipeline_scene(), by the restatement: (plans, fusion)."""
    from orthosfm_amd import dense
    sc = pipeline_scene()
    plans = [dense.plan_view(sc["P"], v, sc["points"][sc["visibility"][v]], range(4), max_depths=MAX_DEPTHS) for v in range(4)]
    maps = {v: dr.sweep(sc["images"], sc["P"], v, p.sources, p.z_min, p.dz, p.num_depths, **PIPELINE_OPTIONS) for v, p in enumerate(plans)}
    return plans, dr.fuse(sc["P"], maps, {v: p.dz for v, p in enumerate(plans)}, **PIPELINE_OPTIONS)


BUILDERS = {
    "slanted": _slanted,
    "radius1": lambda: _radius("radius1", 1),
    "radius7": lambda: _radius("radius7", 7),
    "odd_sizes": _odd_sizes,
    "border": _border,
    "flat": _flat,
    "out_of_range": _out_of_range,
    "many_depths": lambda: _many_depths(MAX_DEPTHS),
    "one_source": _one_source,
    "eight_sources": _eight_sources,
    "step": _step,
    "empty": _empty,
}
NAMES = tuple(BUILDERS)


@lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def sweep_options(c, sw):
    o = dict(c.options)
    o.update(sw.options)
    return o


@lru_cache(maxsize=None)
def restated(name):
    """The restatement's sweeps of a case, in order: computed once, shared, not to be modified."""
    c = case(name)
    out = []
    for sw in c.sweeps:
        m = dr.sweep(c.images, c.P, sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, **sweep_options(c, sw))
        for a in m.values():
            a.setflags(write=False)
        out.append(m)
    return tuple(out)


def tested(m):
    return m["status"] != dr.BORDER


def ambiguous(m):
    return tested(m) & (m["margin"] < AMBIGUITY_BAND)


@lru_cache(maxsize=None)
def restated_fusion(name):
    """The restatement's fusion of a case whose sweeps cover every view once."""
    c = case(name)
    maps = {sw.ref: m for sw, m in zip(c.sweeps, restated(name))}
    dzs = {sw.ref: sw.dz for sw in c.sweeps}
    amb = {v: ambiguous(m) for v, m in maps.items()}
    return dr.fuse(c.P, maps, dzs, ambiguous=amb, depth_band=BOUNDS["depth_steps"], **c.options)
