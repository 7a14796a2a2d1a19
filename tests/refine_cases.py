"""Seeded cases with exact ground truth for the observation refinement (tests/refine_restatement.py is the
definition; tests/test_refine_cases_cpu.py checks the cases, tests/test_refine_gpu.py holds the library to them).

A texture lives on a plane: Gaussian blobs of either sign on a mid-grey ground (a blob's centre maps into a view by
the view's affine map x = M X + t and its covariance by M C M^T, which is the same as evaluating the plane's texture
at M^-1 (x - t)), for some cases a flat region and one smoothed straight edge.  Every view renders it analytically
under its own map, with its own gain and bias, and quantises to 8 bits as tests/sift_cases.py does.  The exact
correspondence of any pixel of any view in any other view is therefore known (Case.exact).

A case is one call: images, tracks, options, and what it must reach (`expect`: statuses that must occur; further
paths are named in the case's `paths` and checked by test_refine_cases_cpu.py).
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from orthosfm_amd import synth

import refine_restatement as rr

STREAM = 0x7E1F << 16

# The pivot threshold of ILL_CONDITIONED (osfm_refine_options.min_pivot), measured with the restatement on the CPU, run
# with min_pivot 1e-12 so that nothing stops it (tests/test_refine_cases_cpu.py::test_pivot_threshold measures again):
# edge_max, the largest over flat_and_edge's edge observations of the smallest scaled pivot of their iterations;
# textured_min, the smallest over base and strong_init; the threshold is their geometric mean, 0.03447, to two digits.
# What keeps the edge's pivots from being smaller still is the 8-bit quantisation of a slanted edge: its staircase
# is a little texture along the edge.
PIVOT = {"edge_max": 0.0160724, "textured_min": 0.0739201, "threshold": 0.034}

# An observation is ambiguous where the margin of the restatement (the smallest relative distance of a tested
# quantity from its threshold, in pixels for the window test) is below this band: the device may decide it the other
# way.  1e-6 as the issue starts from; nothing has asked for more.
AMBIGUITY_BAND = 1e-6

# Agreement of the device with the restatement over the REFINED observations of all cases, measured once on an
# MI355X (tests/test_refine_gpu.py prints the figures): the largest |out_xy| difference in pixels, |out_affine|
# difference and |score| difference.  All three are 0: the restatement adds in the kernel's order and the build
# contracts nothing, so the two run the same IEEE operations.
MEASURED = {"xy": 0.0, "affine": 0.0, "score": 0.0}
# Ten times the measured worst case would be 0 and hold the test to this compiler's choices, which is what the factor
# was meant to allow for.  The bound is instead what another order of the sums can do: a sum of N <= 961 terms in
# another order differs by at most N eps = 2e-13 of its absolute terms; the step solves a system whose scaled pivots
# are at least 0.034, which amplifies that by at most 1 / 0.034^2 < 1e3; the iteration contracts the errors of
# earlier steps, so what is left is that of the last one: 2e-10 of a step, of positions below 2e2 px.  1e-9 covers
# it, and is a thousandth of the 1e-6 px at which the arithmetic would not be double throughout.
BOUNDS = {"xy": 1e-9, "affine": 1e-9, "score": 1e-9}


@dataclass
class View:
    width: int
    height: int
    M: np.ndarray
    t: np.ndarray
    channels: int = 1
    gain: float = 1.0
    bias: float = 0.0
    copy_of: int = -1        # the bytes of another view (an identity map must not differ by a rounding)
    other: float = 0.0       # share of a second, unrelated texture blended in
    holes: tuple = ()        # (X, Y, radius) on the plane: discs where the texture gives way to the ground, over 1.5 px


@dataclass
class Case:
    name: str
    images: list
    views: list
    offsets: np.ndarray
    view: np.ndarray
    xy: np.ndarray
    alive: np.ndarray = None
    init_affine: np.ndarray = None
    options: dict = field(default_factory=dict)
    expect: tuple = ()
    paths: dict = field(default_factory=dict)      # named observations / sets the CPU test looks at

    @property
    def num_obs(self):
        return int(self.offsets[-1])

    def exact(self, f_from, f_to):
        """Where the position of observation f_from lies in the view of observation f_to."""
        a, b = self.views[int(self.view[f_from])], self.views[int(self.view[f_to])]
        X = np.linalg.solve(a.M, self.xy[f_from] - a.t)
        return b.M @ X + b.t

    def call(self):
        return dict(images=self.images, offsets=self.offsets, view=self.view, xy=self.xy, alive=self.alive,
                    init_affine=self.init_affine, **self.options)


def rot(a):
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def _u(seed, stream, n):
    return synth.uniform(seed, STREAM | stream, n)


def make_view(width, height, M, centre=(80.0, 64.0), **kw):
    """A view whose centre shows the plane point `centre`."""
    M = np.asarray(M, dtype=np.float64)
    t = np.array([(width - 1) / 2.0, (height - 1) / 2.0]) - M @ np.asarray(centre, dtype=np.float64)
    return View(width, height, M, t, **kw)


def texture(seed, n_blobs, lo=(-60.0, -60.0), hi=(220.0, 190.0), sigma=(1.6, 3.5), flat_left=None, edge=None):
    """The plane's texture as a function X [n, 2] -> [n, 3] (three colour planes; a grey view takes their mean).
    flat_left: no blob centre nearer than 4 sigma to x < flat_left, which then is constant.  edge: (x0, x1, angle):
    inside the band x0 < x < x1 there are no blobs either, only one smooth step across the line through its middle."""
    u = _u(seed, 1, 8 * n_blobs).reshape(n_blobs, 8)
    c = np.stack([lo[0] + u[:, 0] * (hi[0] - lo[0]), lo[1] + u[:, 1] * (hi[1] - lo[1])], axis=1)
    s1 = sigma[0] * (sigma[1] / sigma[0]) ** u[:, 2]
    s2 = s1 * (0.6 + 0.4 * u[:, 3])
    ang = np.pi * u[:, 4]
    amp = (0.05 + 0.15 * u[:, 5]) * np.where(u[:, 6] < 0.5, -1.0, 1.0)
    col = 0.4 + 0.6 * _u(seed, 2, 3 * n_blobs).reshape(n_blobs, 3)
    col[:, 0] = 1.0
    keep = np.ones(n_blobs, bool)
    reach = 4.0 * np.maximum(s1, s2)
    if flat_left is not None:
        keep &= c[:, 0] - reach > flat_left
    if edge is not None:
        keep &= (c[:, 0] + reach < edge[0]) | (c[:, 0] - reach > edge[1])
    c, s1, s2, ang, amp, col = c[keep], s1[keep], s2[keep], ang[keep], amp[keep], col[keep]
    # inverse covariances
    ca, sa = np.cos(ang), np.sin(ang)
    p00 = ca * ca / (s1 * s1) + sa * sa / (s2 * s2)
    p11 = sa * sa / (s1 * s1) + ca * ca / (s2 * s2)
    p01 = ca * sa * (1.0 / (s1 * s1) - 1.0 / (s2 * s2))

    far = 6.0 * np.maximum(s1, s2)         # beyond it a blob adds less than 1e-8: left out, for the time it saves

    def f(X):
        out = np.zeros((X.shape[0], 3))
        for p0 in range(0, X.shape[0], 1024):
            P = X[p0:p0 + 1024]
            lo_x, hi_x, lo_y, hi_y = P[:, 0].min(), P[:, 0].max(), P[:, 1].min(), P[:, 1].max()
            sl = np.flatnonzero((c[:, 0] > lo_x - far) & (c[:, 0] < hi_x + far) & (c[:, 1] > lo_y - far) & (c[:, 1] < hi_y + far))
            dx, dy = P[:, None, 0] - c[None, sl, 0], P[:, None, 1] - c[None, sl, 1]
            e = np.exp(-0.5 * (p00[sl] * dx * dx + 2.0 * p01[sl] * dx * dy + p11[sl] * dy * dy)) * amp[sl]
            out[p0:p0 + 1024] = e @ col[sl]
        if edge is not None:
            mid, n = 0.5 * (edge[0] + edge[1]), np.array([np.cos(edge[2]), np.sin(edge[2])])
            d = (X[:, 0] - mid) * n[0] + (X[:, 1] - 64.0) * n[1]
            band = (X[:, 0] > edge[0]) & (X[:, 0] < edge[1])
            out += np.where(band, 0.45 * np.tanh(d / 1.0), 0.0)[:, None]
        return out
    return f


def render(view, f, f_other=None):
    """uint8 [h, w] or [h, w, 3]: floor((0.5 + gain * texture + bias) * 255 + 0.5), clipped."""
    ys, xs = np.mgrid[0:view.height, 0:view.width]
    x = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)
    X = np.linalg.solve(view.M, (x - view.t).T).T
    v = f(X)
    if f_other is not None and view.other > 0.0:
        v = (1.0 - view.other) * v + view.other * f_other(X)
    for hx, hy, hr in view.holes:
        v = v * (0.5 + 0.5 * np.tanh((np.hypot(X[:, 0] - hx, X[:, 1] - hy) - hr) / 1.5))[:, None]
    acc = (view.gain * v + view.bias).reshape(view.height, view.width, 3)
    img = np.clip(np.floor((0.5 + acc) * 255.0 + 0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img if view.channels == 3 else
                                np.clip(np.floor((0.5 + acc.mean(axis=2)) * 255.0 + 0.5), 0, 255).astype(np.uint8))


def render_all(views, f, f_other=None):
    images = []
    for v in views:
        images.append(images[v.copy_of].copy() if v.copy_of >= 0 else render(v, f, f_other))
    return images


def plane_points(seed, n, views, radius, step=1.0, margin=2.0, lo=(0.0, 0.0), hi=(160.0, 128.0)):
    """n plane points whose windows (with `margin` pixels to spare) lie inside every view."""
    u = _u(seed, 3, 2 * 40 * n).reshape(-1, 2)
    X = np.stack([lo[0] + u[:, 0] * (hi[0] - lo[0]), lo[1] + u[:, 1] * (hi[1] - lo[1])], axis=1)
    ok = np.ones(X.shape[0], bool)
    for v in views:
        x = X @ v.M.T + v.t
        reach = radius * step * np.sqrt(2.0) * max(1.0, np.linalg.norm(v.M, 2)) + margin
        ok &= (x[:, 0] > reach) & (x[:, 0] < v.width - 1 - reach) & (x[:, 1] > reach) & (x[:, 1] < v.height - 1 - reach)
    X = X[ok]
    assert X.shape[0] >= n, (X.shape[0], n)
    return X[:n]


def tracks_of(X, views, view_lists, seed, noise):
    """Observations of plane points X[i] in the views view_lists[i], with a planted error uniform in +-noise per axis
    (noise may be an array per observation)."""
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in view_lists])]).astype(np.int64)
    F = int(offsets[-1])
    view = np.concatenate([np.asarray(v, np.int32) for v in view_lists]) if F else np.zeros(0, np.int32)
    xy = np.zeros((F, 2))
    e = (2.0 * _u(seed, 4, 2 * F).reshape(F, 2) - 1.0) * np.broadcast_to(np.asarray(noise, dtype=np.float64).reshape(-1, 1), (F, 1)) \
        if F else np.zeros((0, 2))
    for i, vl in enumerate(view_lists):
        for j, v in enumerate(vl):
            xy[offsets[i] + j] = views[v].M @ X[i] + views[v].t
    return offsets, view, xy + e


def relative_affine(case, jitter_seed=None, jitter=0.0):
    """init_affine per observation: M_t M_ref^-1 against the FIRST observation of its track (the cases that use it
    have no dead observations), times (1 + jitter) noise per entry."""
    A = np.zeros((case.num_obs, 4))
    for t in range(case.offsets.shape[0] - 1):
        r = int(case.offsets[t])
        for f in range(r, int(case.offsets[t + 1])):
            A[f] = (case.views[int(case.view[f])].M @ np.linalg.inv(case.views[int(case.view[r])].M)).reshape(4)
    if jitter_seed is not None:
        A = A * (1.0 + jitter * (2.0 * _u(jitter_seed, 5, A.size).reshape(A.shape) - 1.0))
    return A


# ---------------------------------------------------------------------------------------------------------------
def _base():
    views = [make_view(160, 128, np.eye(2)), make_view(160, 128, 0.9 * rot(0.05), gain=0.8, bias=0.04),
             make_view(160, 128, rot(-0.05) / 0.9 @ np.diag([1.0, 0.95]), gain=1.2, bias=-0.03)]
    f = texture(11, 1400)
    X = plane_points(12, 60, views, 7, margin=4.0)
    offsets, view, xy = tracks_of(X, views, [[0, 1, 2]] * 60, 13, 0.4)
    return Case("base", render_all(views, f), views, offsets, view, xy, expect=(rr.REFERENCE, rr.REFINED))


def _strong(with_init):
    views = [make_view(160, 128, np.eye(2)), make_view(160, 128, 0.7 * rot(np.pi / 4.0), gain=0.9)]
    f = texture(21, 1400)
    X = plane_points(22, 40, views, 7, margin=4.0)
    offsets, view, xy = tracks_of(X, views, [[0, 1]] * 40, 23, 0.4)
    c = Case("strong_init" if with_init else "strong_noinit", render_all(views, f), views, offsets, view, xy,
             expect=(rr.REFINED,) if with_init else ())
    if with_init:
        c.init_affine = relative_affine(c, 24, 0.03)
    return c


def _border():
    W, H, R = 97, 81, 7
    views = [make_view(W, H, np.eye(2), centre=(48.0, 40.0)), make_view(W, H, 0.95 * rot(0.04), centre=(48.0, 40.0)),
             make_view(W, H, np.eye(2), centre=(48.0, 40.0), copy_of=0), make_view(W, H, np.eye(2), centre=(43.0, 37.0))]
    f = texture(31, 800, lo=(-40.0, -40.0), hi=(140.0, 120.0))
    X = plane_points(32, 12, views, R, margin=4.0, hi=(W, H))
    lists = [[0, 1, 2]] * 12
    offsets, view, xy = tracks_of(X, views, lists, 33, 0.3)
    extra_xy, extra_view, paths = [], [], {}
    base = int(offsets[-1])

    def add(name, a, b, va=0, vb=2):
        paths[name] = base + len(extra_xy) + 1
        extra_xy.extend([a, b])
        extra_view.extend([va, vb])
    add("ref_outside", (R - 0.5, 40.0), (30.0, 40.0))
    add("target_outside_first", (30.0, 40.0), (30.0, H - 1 - R + 0.25))
    # view 3 shows the plane 5 px to the right and 3 px down.  The target starts inside with 0.2 px to spare, the
    # texture it belongs to lies 0.6 px further out: a step leaves the image
    add("target_outside_later", (W - 1 - R - 5 + 0.4, 40.3), (W - 1 - R - 0.2, 43.3), vb=3)
    add("target_outside_later_y", (45.2, H - 1 - R - 3 + 0.45), (50.2, H - 1 - R - 0.15), vb=3)
    # touches the last row and column exactly, in the reference and in the target (a copy: the residual is zero)
    add("touch", (float(W - 1 - R), float(H - 1 - R)), (float(W - 1 - R), float(H - 1 - R)))
    add("touch_origin", (float(R), float(R)), (float(R), float(R)))
    n_extra = len(extra_xy) // 2
    offsets = np.concatenate([offsets, base + 2 * np.arange(1, n_extra + 1)]).astype(np.int64)
    view = np.concatenate([view, np.asarray(extra_view, np.int32)])
    xy = np.concatenate([xy, np.asarray(extra_xy, dtype=np.float64)])
    return Case("border", render_all(views, f), views, offsets, view, xy, expect=(rr.REFINED, rr.OUTSIDE), paths=paths)


def _flat_and_edge():
    views = [make_view(160, 128, np.eye(2)), make_view(160, 128, 0.95 * rot(0.03), gain=0.9)]
    f = texture(41, 1400, flat_left=50.0, edge=(60.0, 100.0, 0.3))
    n = 8
    u = _u(42, 6, 6 * n).reshape(n, 6)
    flat = np.stack([16.0 + 18.0 * u[:, 0], 30.0 + 60.0 * u[:, 1]], axis=1)
    # on the edge: the line through (80, 64) with normal (cos 0.3, sin 0.3)
    s = -25.0 + 50.0 * u[:, 2]
    edge = np.stack([80.0 - np.sin(0.3) * s, 64.0 + np.cos(0.3) * s], axis=1) + (u[:, 3:5] - 0.5)
    tex = np.stack([122.0 + 16.0 * u[:, 4], 30.0 + 60.0 * u[:, 5]], axis=1)
    X = np.concatenate([flat, edge, tex])
    offsets, view, xy = tracks_of(X, views, [[0, 1]] * (3 * n), 43, 0.3)
    paths = {"flat": 2 * np.arange(n) + 1, "edge": 2 * (n + np.arange(n)) + 1, "textured": 2 * (2 * n + np.arange(n)) + 1}
    return Case("flat_and_edge", render_all(views, f), views, offsets, view, xy, expect=(rr.FLAT, rr.ILL_CONDITIONED, rr.REFINED),
                paths=paths)


def _mismatch():
    # view 1: the plane at scale 0.8, given the identity as its warp (REJECT_DEFORM with max_deform 1.15); view 2:
    # nearly view 0, observations planted beside their texture (REJECT_SHIFT, NOT_CONVERGED, ...); view 3: a
    # disc beside every point shows the bare ground (REJECT_SCORE at the right position)
    views = [make_view(160, 128, np.eye(2)), make_view(160, 128, 0.8 * np.eye(2)), make_view(160, 128, 0.98 * rot(0.02)),
             make_view(160, 128, np.eye(2))]
    f = texture(51, 1400)
    n = 10
    X = plane_points(53, 4 * n, views, 7, margin=8.0)
    views[3].holes = tuple((x + 4.0, y + 2.0, 5.5) for x, y in X[3 * n:])
    lists = [[0, 1]] * n + [[0, 2]] * (2 * n) + [[0, 3]] * n
    noise = np.concatenate([np.full(2 * n, 0.2), np.full(2 * n, 0.2), np.full(2 * n, 0.2), np.full(2 * n, 0.2)])
    offsets, view, xy = tracks_of(X, views, lists, 54, noise)
    u = _u(55, 7, 4 * n).reshape(2 * n, 2)
    ang = 2.0 * np.pi * u[:, 0]
    far = np.where(np.arange(2 * n) < n, 3.3 + 1.2 * u[:, 1], 6.0 + 6.0 * u[:, 1])      # just over max_shift; well beside
    tgt = 2 * (n + np.arange(2 * n)) + 1
    xy[tgt] += np.stack([far * np.cos(ang), far * np.sin(ang)], axis=1)
    return Case("mismatch", render_all(views, f), views, offsets, view, xy, options=dict(max_deform=1.15, eps=0.02),
                expect=(rr.REJECT_SHIFT, rr.REJECT_DEFORM, rr.REJECT_SCORE, rr.NOT_CONVERGED))


def _radius(name, **options):
    views = [make_view(160, 128, np.eye(2)), make_view(160, 128, 0.95 * rot(0.04), gain=0.9, bias=0.02)]
    f = texture(61, 1400)
    X = plane_points(62, 16, views, 15, margin=4.0)
    offsets, view, xy = tracks_of(X, views, [[0, 1]] * 16, 63, 0.3)
    return Case(name, render_all(views, f), views, offsets, view, xy, options=options)


def _lengths():
    V, W, H = 33, 56, 48
    u = _u(71, 8, 3 * V).reshape(V, 3)
    views = [make_view(W, H, (0.94 + 0.12 * u[v, 0]) * rot(0.16 * (u[v, 1] - 0.5)) if v else np.eye(2), centre=(28.0, 24.0),
                       gain=0.85 + 0.3 * u[v, 2]) for v in range(V)]
    f = texture(72, 260, lo=(-30.0, -30.0), hi=(90.0, 80.0), sigma=(1.6, 3.5))
    X = plane_points(73, 13, views, 7, margin=3.0, hi=(W, H))
    lists = [[0, 5]] * 2 + [[3, 9]] * 2 + [[0, 1, 2]] * 3 + [[4, 7, 30]] * 2 + [list(range(V))] * 2 + [[2, 6, 8]] * 2
    offsets, view, xy = tracks_of(X, views, lists, 74, 0.3)
    alive = np.ones(int(offsets[-1]), np.uint8)
    paths = {}
    alive[offsets[4]] = 0                   # a dead first observation: the reference moves to the second
    paths["moved_reference"] = int(offsets[4]) + 1
    alive[offsets[9] + 0] = 0               # in a long track: dead first and a dead one in the middle
    alive[offsets[9] + 17] = 0
    paths["moved_reference_long"] = int(offsets[9]) + 1
    alive[offsets[11]] = 0                  # one alive observation left
    alive[offsets[11] + 2] = 0
    paths["single"] = np.arange(offsets[11], offsets[12])
    alive[offsets[12] + 1] = 0              # a dead observation that is not the first
    assert int(offsets[-1]) % 4 != 0
    return Case("lengths", render_all(views, f), views, offsets, view, xy, alive=alive,
                expect=(rr.UNTESTED, rr.REFERENCE, rr.REFINED), paths=paths)


def _rgb_sizes():
    views = [make_view(160, 128, np.eye(2)), make_view(131, 101, 0.97 * rot(-0.04), channels=3, gain=1.1),
             make_view(97, 120, rot(0.05) / 0.97, channels=3, gain=0.9, bias=0.03)]
    f = texture(81, 1400)
    X = plane_points(82, 20, views, 7, margin=4.0)
    offsets, view, xy = tracks_of(X, views, [[0, 1, 2]] * 10 + [[1, 2]] * 5 + [[2, 0]] * 5, 83, 0.3)
    return Case("rgb_sizes", render_all(views, f), views, offsets, view, xy, expect=(rr.REFINED,))


def _empty():
    views = [make_view(40, 32, np.eye(2), centre=(20.0, 16.0))]
    return Case("empty", render_all(views, texture(91, 20, lo=(0.0, 0.0), hi=(40.0, 32.0))), views, np.zeros(1, np.int64),
                np.zeros(0, np.int32), np.zeros((0, 2)))


BUILDERS = {
    "base": _base,
    "strong_init": lambda: _strong(True),
    "strong_noinit": lambda: _strong(False),
    "border": _border,
    "flat_and_edge": _flat_and_edge,
    "mismatch": _mismatch,
    "radius2": lambda: _radius("radius2", radius=2),
    "radius3": lambda: _radius("radius3", radius=3),
    "radius7": lambda: _radius("radius7", radius=7),
    "radius15": lambda: _radius("radius15", radius=15),
    "step2": lambda: _radius("step2", radius=7, step=2.0),
    "lengths": _lengths,
    "rgb_sizes": _rgb_sizes,
    "empty": _empty,
}
NAMES = tuple(BUILDERS)


@lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@lru_cache(maxsize=None)
def restated(name):
    """The restatement's result on a case: computed once, shared, not to be modified."""
    out = rr.refine_tracks(**case(name).call())
    for a in out.values():
        a.setflags(write=False)
    return out


def tested(out):
    """Observations that went through the refinement: every status but UNTESTED and REFERENCE."""
    return (out["status"] != rr.UNTESTED) & (out["status"] != rr.REFERENCE)


def ambiguous(out):
    return tested(out) & (out["margin"] < AMBIGUITY_BAND)
