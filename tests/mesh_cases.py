"""Hand-built depth maps for the depth-map meshes (tests/mesh_restatement.py is the definition;
tests/test_mesh_cases_cpu.py checks the cases, tests/test_dense_mesh_gpu.py holds the library to them).

Images are blank and the right size; cameras come from dense_cases.camera.  With A = (I | 0) the footprint of a view
is exactly 1, so a threshold is dd_factor itself and a depth can sit exactly on it.
"""
import math
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import dense_cases as dc
import dense_restatement as dr
import mesh_restatement as mr

# the labelling tile and the largest confidence_iterations of the kernels as built (osfm_dense_mesh_limits;
# test_dense_mesh_gpu.py checks that the library says the same): the islands are placed across these seams
LABEL_TILE = (32, 16)
MAX_CONFIDENCE_ITERATIONS = 16

# The restatement's meshes of the restatement's own sweeps against the exact surfaces, measured on the CPU
# (test_mesh_cases_cpu.py measures again and holds them): the median angle in degrees between a vertex normal and the
# normal of the plane its pixel shows, and the share of confidence-0 vertices among the vertices farther than one
# depth step from that plane (0 of them: the share is 1.0 by convention).
MEASURED_CPU = {
    "slanted": {"median_angle_deg": 6.9454, "far_with_confidence_0": 0.2515, "far": 171},
    "step": {"median_angle_deg": 5.5803, "far_with_confidence_0": 0.6441, "far": 739},
}

# The device against the restatement over all cases, measured once on an MI355X (test_dense_mesh_gpu.py prints the
# figures): the largest absolute difference of a normal's component and the largest relative difference of a scale.
MEASURED = {"normals": 0.0, "scale": 0.0}                 # equal to the bit on every case
# What the comparison allows: the rounding of a few dozen double operations on values of order one is 1e-14; a wrong
# neighbour moves a normal or a scale by 1e-3 or more.
BOUNDS = {"normals": 1e-12, "scale": 1e-12}


@dataclass
class Map:
    label: str
    P: np.ndarray                # [2, 4]
    depth: np.ndarray            # float64 [h, w]: NaN where the status is not OK
    status: np.ndarray           # uint8 [h, w]
    dz: float
    runs: list                   # the option sets the map is meshed with
    paths: dict = field(default_factory=dict)

    @property
    def image(self):
        return np.zeros(self.status.shape, np.uint8)


def _map(label, solid, z, runs, dz=0.25, P=None, paths=None):
    solid = np.asarray(solid, bool)
    h, w = solid.shape
    depth = np.where(solid, np.asarray(z, dtype=np.float64), np.nan)
    # what is not solid carries the sweep's other statuses in turn
    other = (np.arange(h * w).reshape(h, w) % dr.RANGE_EDGE + 1).astype(np.uint8)
    status = np.where(solid, dr.OK, other).astype(np.uint8)
    return Map(label, dc.camera(w, h) if P is None else P, depth, status, dz, runs, dict(paths or {}))


DD = 2.0                                       # the threshold of `quads` on a straight edge
DD_DIAG = DD * math.sqrt(2.0)                  # and on a diagonal one, as the restatement forms it


def quad_list():
    """(name, mask, (z0, z1, z2, z3)) of the 2 x 2 blocks of `quads`, pixels 0 = (x, y), 1 = (x+1, y), 2 = (x, y+1),
    3 = (x+1, y+1)."""
    up = lambda v: float(np.nextafter(v, np.inf))
    return [
        ("mask7", 7, (0.0, 0.0, 0.0, 0.0)), ("mask11", 11, (0.0, 0.5, 0.0, 0.25)), ("mask13", 13, (0.0, 0.0, 0.5, 0.25)),
        ("mask14", 14, (0.0, 0.25, 0.5, 0.0)), ("two_pixels", 3, (0.0, 0.0, 0.0, 0.0)), ("two_diagonal", 9, (0.0, 0.0, 0.0, 0.0)),
        ("diagonal_03", 15, (0.0, 1.0, -1.0, 0.0)),             # |z0 - z3| < |z1 - z2|: T2, T3
        ("diagonal_12", 15, (1.0, 0.0, 0.0, -1.0)),             # else: T1, T4
        ("tie_flat", 15, (0.0, 0.0, 0.0, 0.0)), ("tie_sloped", 15, (0.0, 0.0, 1.0, 1.0)),
        ("straight_at", 15, (0.0, DD, 0.0, 0.0)),               # T2's edges 0-1 and 3-1 exactly at the threshold: kept
        ("straight_above", 15, (0.0, up(DD), 0.0, 0.0)),        # one ulp more: T2 goes, T3 stays
        ("diagonal_at", 7, (DD_DIAG / 2.0, DD_DIAG, 0.0, 0.0)),  # T1's edge 2-1 exactly at the diagonal threshold
        ("diagonal_above", 7, (DD_DIAG / 2.0, up(DD_DIAG), 0.0, 0.0)),
        ("between", 7, (0.0, 0.5 * (DD + DD_DIAG), 0.0, 0.0)),  # above the straight threshold on the straight edge 0-1
        ("between_diagonal", 14, (0.0, 0.5 * (DD + DD_DIAG), 0.0, 1.0)),   # the same difference on the diagonal 1-2: kept
        ("cliff", 15, (0.0, 100.0, 0.0, 100.0)),                # both triangles go, unless dd_factor is 0
    ]


def _quads():
    quads = quad_list()
    h, w = 4, 3 * len(quads) + 1
    solid, z = np.zeros((h, w), bool), np.zeros((h, w))
    for k, (_, mask, zs) in enumerate(quads):
        for c in range(4):
            y, x = 1 + (c >> 1), 1 + 3 * k + (c & 1)
            solid[y, x], z[y, x] = bool(mask >> c & 1), zs[c]
    runs = [dict(dd_factor=DD), dict(dd_factor=0.0), dict(dd_factor=DD, confidence_iterations=1)]
    return [_map("strip", solid, z, runs, paths={"first_x": 1, "pitch": 3, "row": 1})]


def _classes():
    h, w = 16, 24
    ys, xs = np.mgrid[0:h, 0:w]
    solid = (xs >= 1) & (xs <= 13) & (ys >= 1) & (ys <= 11)
    solid[5, 5] = False                                          # a hole one pixel wide
    for x, y in ((16, 2), (16, 3), (17, 3), (18, 3), (18, 4)):   # two triangles that share only the pixel (17, 3)
        solid[y, x] = True
    solid[13:15, 16:18] = True                                   # one 2 x 2 block on its own
    z = 0.1 * xs + 0.05 * ys
    runs = [dict(), dict(confidence_iterations=0), dict(confidence_iterations=1), dict(confidence_iterations=MAX_CONFIDENCE_ITERATIONS)]
    return [_map("classes", solid, z, runs, paths={"bow_tie": (17, 3), "hole": (5, 5), "centre": (9, 6)})]


MIN_ISLAND = 12


def serpentine(h, w):
    s = np.zeros((h, w), bool)
    s[0::2] = True
    for y in range(1, h, 2):
        s[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    return s


def _islands():
    h, w = 81, 97
    tw, th = LABEL_TILE
    s = np.zeros((h, w), bool)
    paths = {}

    def put(name, ys, xs, kept):
        s[ys, xs] = True
        first = lambda a: a.start if isinstance(a, slice) else a
        paths[name] = (first(ys), first(xs), kept)                # (y, x) of its first pixel; does it stay

    put("below", 2, slice(2, 2 + MIN_ISLAND - 1), False)
    put("equal", 4, slice(2, 2 + MIN_ISLAND), True)
    put("above", 6, slice(2, 2 + MIN_ISLAND + 1), True)
    put("vertical_seam", 9, slice(tw - 5, tw - 5 + MIN_ISLAND), True)
    put("vertical_seam_below", 11, slice(tw - 5, tw - 5 + MIN_ISLAND - 1), False)
    put("horizontal_seam", slice(th - 6, th - 6 + MIN_ISLAND), 40, True)
    put("horizontal_seam_below", slice(th - 6, th - 6 + MIN_ISLAND - 1), 44, False)
    put("corner", slice(2 * th - 2, 2 * th + 2), slice(2 * tw - 2, 2 * tw + 2), True)          # 16 pixels, four tiles
    put("corner_below", slice(3 * th - 1, 3 * th + 2), slice(tw - 1, tw + 2), False)          # 9 pixels ...
    s[3 * th - 1:3 * th + 1, tw + 2] = True                                                     # ... and 2: 11, four tiles
    put("diagonal_a", slice(2, 4), slice(70, 73), False)                                        # 6 pixels each: together
    put("diagonal_b", slice(4, 6), slice(73, 76), False)                                        # they would stay
    ys, xs = np.mgrid[0:h, 0:w]
    board = (xs >= 70) & (xs <= 85) & (ys >= 20) & (ys <= 30) & ((xs + ys) % 2 == 0)
    s |= board
    paths["checkerboard"] = (20, 70, False)
    shapes = _map("shapes", s, 0.01 * xs + 0.02 * ys, [dict(min_island=MIN_ISLAND), dict(min_island=0), dict(min_island=1)], paths=paths)
    sp = serpentine(h, w)
    n = int(sp.sum())
    snake = _map("serpentine", sp, 0.01 * xs, [dict(min_island=n), dict(min_island=n + 1)], paths={"size": n})
    return [shapes, snake]


def _tiny():
    maps = []
    for h, w in ((1, 1), (5, 1), (1, 5), (2, 2)):
        for name, fill in (("solid", True), ("empty", False)):
            maps.append(_map(f"{w}x{h}_{name}", np.full((h, w), fill), np.zeros((h, w)), [dict(), dict(min_island=2), dict(min_island=5)]))
    return maps


def slanted_views():
    """(w, h, P) of views 0 (A = (I | 0)) and 1 (rotated) of dense_cases' `slanted`, without rendering them."""
    return dc._ring(4)[:2]


def _slanted_exact():
    maps = []
    for v, (w, h, P) in enumerate(slanted_views()):
        depth = dc.trace(dr.Geometry(P), w, h, [dc.SLANT])[0]
        assert np.isfinite(depth).all()
        maps.append(_map(f"view{v}", np.ones((h, w), bool), depth, [dict(), dict(min_island=MIN_ISLAND)], P=P))
    return maps


BUILDERS = {"quads": _quads, "classes": _classes, "islands": _islands, "tiny": _tiny, "slanted_exact": _slanted_exact}
NAMES = tuple(BUILDERS)


@lru_cache(maxsize=None)
def case(name):
    """The maps of a case: built once, shared, not to be modified."""
    maps = BUILDERS[name]()
    for m in maps:
        m.depth.setflags(write=False)
        m.status.setflags(write=False)
    return tuple(maps)


def runs():
    """(case, map index, run index) of every mesh the cases ask for."""
    return [(n, i, j) for n in NAMES for i, m in enumerate(case(n)) for j in range(len(m.runs))]


@lru_cache(maxsize=None)
def restated(name, i, j):
    """The restatement's mesh of run j of map i of a case: computed once, shared, not to be modified."""
    m = case(name)[i]
    out = mr.mesh(m.P, m.depth, m.status, m.dz, **m.runs[j])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def plane_normal(P, plane):
    """The unit normal of Z = a X + b Y + c that faces the camera of P (n . d < 0)."""
    n = np.array([-plane.a, -plane.b, 1.0])
    n /= np.linalg.norm(n)
    return -n if n @ np.array(dr.Geometry(P).d) > 0.0 else n


@lru_cache(maxsize=None)
def sweep_meshes(name):
    """The restatement's meshes (default options) of the restatement's sweeps of a dense case, per sweep."""
    c = dc.case(name)
    return tuple(mr.mesh(c.P[sw.ref], m["depth"], m["status"], sw.dz) for sw, m in zip(c.sweeps, dc.restated(name)))


def surface_accuracy(name):
    """(median angle in degrees to the true plane normal, share of confidence-0 vertices among those farther than a
    step from their plane, how many those are) over sweep_meshes(name)."""
    c = dc.case(name)
    angles, far, far0 = [], 0, 0
    for sw, mesh in zip(c.sweeps, sweep_meshes(name)):
        exact, which = c.exact(sw.ref)
        px = mesh["pixel"]
        normals = np.stack([plane_normal(c.P[sw.ref], p) for p in c.planes])[which[px[:, 1], px[:, 0]]]
        cos = np.clip((mesh["normals"] * normals).sum(axis=1), -1.0, 1.0)
        angles.append(np.degrees(np.arccos(cos)))
        z = np.asarray(dr.Geometry(c.P[sw.ref]).depth(tuple(mesh["points"].T)))
        off = np.abs(z - exact[px[:, 1], px[:, 0]]) > sw.dz
        far += int(off.sum())
        far0 += int((off & (mesh["confidence"] == 0.0)).sum())
    return float(np.median(np.concatenate(angles))), (far0 / far if far else 1.0), far
