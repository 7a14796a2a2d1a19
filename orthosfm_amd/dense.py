"""Dense depth maps by orthographic plane sweep and their fusion into one point cloud (include/osfm_hip.h, "Dense
depth maps"; DESIGN.md "Dense plane sweep").  No counterpart in the reference."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import capi, synth
from .features import _Handle, _image_arg


def affine_cameras(model, cam_params, widths, heights):
    """P [V, 2, 4] of both camera models, pixel = P[:, :3] X + P[:, 3]: row 0 is -W / (2 scale) times the first row
    of the world -> local rotation with t_0 = W (offX / 2 + 0.5), row 1 the same with H and offY -- the projection
    of synth.project_quat / project_euler written as a matrix."""
    cam_params = np.asarray(cam_params, dtype=np.float64)
    V = cam_params.shape[0]
    widths = np.broadcast_to(np.asarray(widths, dtype=np.float64), (V,))
    heights = np.broadcast_to(np.asarray(heights, dtype=np.float64), (V,))
    P = np.zeros((V, 2, 4))
    for v, p in enumerate(cam_params):
        if model == synth.MODEL_QUATERNION:
            q = p[:4]
            qi = np.array([-q[0], -q[1], -q[2], q[3]]) / np.dot(q, q)
            R = synth.quat_rotate(qi, np.eye(3)).T          # world -> local: column j is the image of e_j
            off_x, off_y, scale = p[4], p[5], p[6]
        else:
            R = synth.euler_matrix(p[0], p[1], p[2]).T @ synth._T
            off_x, off_y, scale = p[3], p[4], p[5]
        P[v, 0, :3] = -widths[v] / (2.0 * scale) * R[0]
        P[v, 1, :3] = -heights[v] / (2.0 * scale) * R[1]
        P[v, 0, 3] = widths[v] * (off_x / 2.0 + 0.5)
        P[v, 1, 3] = heights[v] * (off_y / 2.0 + 0.5)
    return P


def viewing_axes(P):
    """d_v = (a0 x a1) / |a0 x a1| per view, [V, 3]."""
    P = np.asarray(P, dtype=np.float64)
    c = np.cross(P[:, 0, :3], P[:, 1, :3])
    return c / np.linalg.norm(c, axis=1, keepdims=True)


@dataclass
class ViewPlan:
    sources: list
    z_min: float
    dz: float
    num_depths: int


def plan_view(P, r, points_of_view, candidates, max_sources=4, max_depths=None):
    """The sweep of view r, by a fixed rule; None when no candidate or no point serves.
    Sources: up to max_sources of `candidates` whose viewing axis makes 5..40 degrees with d_r, nearest to 15 degrees
    first, ties by index.  Depth range: that of d_r . X over points_of_view [n, 3] (the view's sparse points),
    widened by 10 % on each side and by no less than two steps (a surface at the end of the sparse range, or a
    scene that is flat as the view sees it, still has both neighbours of its best depth).  Step: 0.5 / max_s |e_rs|
    -- half a pixel along the longest epipolar line --, widened so that the range takes at most max_depths steps."""
    P = np.asarray(P, dtype=np.float64)
    pts = np.asarray(points_of_view, dtype=np.float64).reshape(-1, 3)
    if max_depths is None:
        max_depths = capi.dense_limits()[4]
    d = viewing_axes(P)
    ranked = []
    for s in sorted(int(c) for c in candidates):
        if s == r:
            continue
        angle = np.degrees(np.arccos(np.clip(abs(float(d[s] @ d[r])), 0.0, 1.0)))
        if 5.0 <= angle <= 40.0:
            ranked.append((abs(angle - 15.0), s))
    ranked.sort()
    sources = [s for _, s in ranked[:max_sources]]
    if not sources or pts.shape[0] == 0:
        return None
    z = pts @ d[r]
    lo, hi = float(z.min()), float(z.max())
    e = max(float(np.linalg.norm(P[s, :, :3] @ d[r])) for s in sources)
    dz = 0.5 / e
    pad = max(0.1 * (hi - lo), 2.0 * dz)
    lo, hi = lo - pad, hi + pad
    D = int(np.ceil((hi - lo) / dz)) + 1
    if D > max_depths:
        D = max_depths
        dz = (hi - lo) / (D - 1)
    D = max(D, 3)
    return ViewPlan(sources, lo, dz, D)


@dataclass
class DepthMap:
    depth: np.ndarray         # float64 [h, w]: NaN where the status is not DENSE_OK
    score: np.ndarray         # float32 [h, w]
    status: np.ndarray        # uint8 [h, w]: capi.DENSE_*
    stats: capi.DenseStats

    @property
    def ok(self):
        return self.status == capi.DENSE_OK


@dataclass
class RefinedMap:
    """What osfm_dense_refine_view leaves of a view's map; the arrays are None with download=False."""
    depth: np.ndarray         # float64 [h, w]: the map after the call (refined where the status is DENSE_REFINE_REFINED)
    gradient: np.ndarray      # float64 [h, w, 2]: depth per pixel along x and y; NaN where not refined
    normal: np.ndarray        # float64 [h, w, 3]: unit, towards the camera; NaN where not refined
    score: np.ndarray         # float32 [h, w]: the map's after the call
    status: np.ndarray        # uint8 [h, w]: capi.DENSE_REFINE_*
    stats: capi.DenseRefineStats

    @property
    def refined(self):
        return self.status == capi.DENSE_REFINE_REFINED


@dataclass
class Cloud:
    points: np.ndarray        # float64 [N, 3]
    view: np.ndarray          # int32 [N]
    pixel: np.ndarray         # int32 [N, 2]: x, y in the view's image
    stats: capi.DenseStats


@dataclass
class ViewMesh:
    """The mesh of one view's depth map (osfm_dense_mesh_view)."""
    view: int
    points: np.ndarray        # float64 [V, 3]
    normals: np.ndarray       # float64 [V, 3]: unit, towards the camera; 0 where the incident faces cancel
    confidence: np.ndarray    # float32 [V]: 0 on the border of the mesh, 1 from confidence_iterations edges inside
    scale: np.ndarray         # float64 [V]: mean length of the mesh edges at the vertex
    pixel: np.ndarray         # int32 [V, 2]: x, y in the view's image
    vclass: np.ndarray        # uint8 [V]: capi.MESH_VERTEX_*
    triangles: np.ndarray     # int32 [T, 3]: vertex indices, in MVE's winding
    stats: capi.DenseMeshStats
    rgb: np.ndarray = None    # uint8 [V, 3]: the vertices' pixels, where a caller has the image (pipeline.densify)


class DenseStereo(_Handle):
    """One osfm_dense: a grey image per view on the device, the cameras, and the depth maps swept so far."""
    _prefix = "dense"

    def __init__(self, device: int = 0, num_views: int = 1):
        self.num_views = int(num_views)
        self._shape = [None] * self.num_views
        self._h = C.c_void_p()
        capi.check(capi.lib.osfm_dense_create(int(device), self.num_views, C.byref(self._h)))

    def set_image(self, view: int, image):
        """uint8 [h, w] or [h, w, 3] from host memory."""
        image, channels = _image_arg("DenseStereo", image)
        capi.check(capi.lib.osfm_dense_set_image(self._h, int(view), image.ctypes.data, image.shape[1], image.shape[0], channels))
        self._shape[int(view)] = (image.shape[0], image.shape[1])

    def set_image_from_front(self, view: int, front, shape):
        """The feature image of a features.ViewFrontEnd's last load, device to device; shape: its (height, width)."""
        capi.check(capi.lib.osfm_dense_set_image_from_front(self._h, int(view), front._h))
        self._shape[int(view)] = (int(shape[0]), int(shape[1]))

    def set_cameras(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64)
        if P.shape != (self.num_views, 2, 4):
            raise ValueError(f"DenseStereo.set_cameras: P {P.shape}, [{self.num_views}, 2, 4] is expected")
        capi.check(capi.lib.osfm_dense_set_cameras(self._h, P.ctypes.data))

    def sweep(self, ref: int, sources, z_min: float, dz: float, num_depths: int, download=True, **options) -> DepthMap:
        """osfm_dense_sweep; options: the fields of osfm_dense_options.  download=False leaves the map on the device
        (the arrays of the result are None)."""
        o = capi.default_dense_options(**options)
        sources = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        shape = self._shape[int(ref)] if 0 <= int(ref) < self.num_views else None
        res = DepthMap(None, None, None, capi.DenseStats())
        if download and shape is not None:
            res.depth, res.score, res.status = np.zeros(shape), np.zeros(shape, np.float32), np.zeros(shape, np.uint8)
        p = lambda a: a.ctypes.data if a is not None else None
        capi.check(capi.lib.osfm_dense_sweep(self._h, int(ref), sources.shape[0], sources.ctypes.data, float(z_min), float(dz),
                                             int(num_depths), C.byref(o), p(res.depth), p(res.score), p(res.status),
                                             C.byref(res.stats)))
        return res

    def refine(self, view: int, sources, download=True, **options) -> RefinedMap:
        """osfm_dense_refine_view: slanted-plane refinement of the view's map, in place; options: the fields of
        osfm_dense_refine_options.  download=False leaves everything on the device (refined_planes() fetches it)."""
        o = capi.default_dense_refine_options(**options)
        sources = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        shape = self._shape[int(view)] if 0 <= int(view) < self.num_views else None
        res = RefinedMap(None, None, None, None, None, capi.DenseRefineStats())
        if download and shape is not None:
            res.depth, res.gradient, res.normal = np.zeros(shape), np.zeros(shape + (2,)), np.zeros(shape + (3,))
            res.score, res.status = np.zeros(shape, np.float32), np.zeros(shape, np.uint8)
        p = lambda a: a.ctypes.data if a is not None else None
        capi.check(capi.lib.osfm_dense_refine_view(self._h, int(view), sources.shape[0], sources.ctypes.data, C.byref(o), p(res.depth),
                                                   p(res.gradient), p(res.normal), p(res.score), p(res.status), C.byref(res.stats)))
        return res

    def refined_planes(self, view: int):
        """osfm_dense_download_refined: (gradient [h, w, 2], normal [h, w, 3], status [h, w]) of the view's last refine()."""
        shape = self._shape[int(view)] if 0 <= int(view) < self.num_views else None
        shape = shape if shape is not None else (1, 1)
        gradient, normal, status = np.zeros(shape + (2,)), np.zeros(shape + (3,)), np.zeros(shape, np.uint8)
        capi.check(capi.lib.osfm_dense_download_refined(self._h, int(view), gradient.ctypes.data, normal.ctypes.data, status.ctypes.data))
        return gradient, normal, status

    def fuse(self, **options) -> Cloud:
        """osfm_dense_fuse and osfm_dense_download_cloud."""
        o = capi.default_dense_options(**options)
        n, stats = C.c_int64(), capi.DenseStats()
        capi.check(capi.lib.osfm_dense_fuse(self._h, C.byref(o), C.byref(n), C.byref(stats)))
        N = int(n.value)
        cloud = Cloud(np.zeros((N, 3)), np.zeros(N, np.int32), np.zeros((N, 2), np.int32), stats)
        capi.check(capi.lib.osfm_dense_download_cloud(self._h, N, cloud.points.ctypes.data, cloud.view.ctypes.data,
                                                      cloud.pixel.ctypes.data))
        return cloud

    def fused_status(self, view: int) -> np.ndarray:
        """The status of a swept view after the last fuse(), uint8 [h, w]."""
        shape = self._shape[int(view)] if 0 <= int(view) < self.num_views else None
        out = np.zeros(shape if shape is not None else (1, 1), np.uint8)
        capi.check(capi.lib.osfm_dense_download_status(self._h, int(view), out.ctypes.data))
        return out


    def set_map(self, view: int, depth, status, dz: float, score=None):
        """osfm_dense_set_map: a depth map from elsewhere, in the layout sweep() returns; the view counts as swept."""
        shape = self._shape[int(view)] if 0 <= int(view) < self.num_views else None
        depth = np.ascontiguousarray(depth, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.uint8)
        if score is not None:
            score = np.ascontiguousarray(score, dtype=np.float32)
        for name, a in (("depth", depth), ("status", status), ("score", score)):
            if shape is not None and a is not None and a.shape != shape:
                raise ValueError(f"DenseStereo.set_map: {name} {a.shape}, the view's image is {shape}")
        capi.check(capi.lib.osfm_dense_set_map(self._h, int(view), depth.ctypes.data, score.ctypes.data if score is not None else None,
                                               status.ctypes.data, float(dz)))

    def mesh(self, view: int, **options) -> ViewMesh:
        """osfm_dense_mesh_view and osfm_dense_download_mesh; options: the fields of osfm_dense_mesh_options."""
        o = capi.default_dense_mesh_options(**options)
        nv, nt, stats = C.c_int64(), C.c_int64(), capi.DenseMeshStats()
        capi.check(capi.lib.osfm_dense_mesh_view(self._h, int(view), C.byref(o), C.byref(nv), C.byref(nt), C.byref(stats)))
        V, T = int(nv.value), int(nt.value)
        m = ViewMesh(int(view), np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V, np.float32), np.zeros(V), np.zeros((V, 2), np.int32),
                     np.zeros(V, np.uint8), np.zeros((T, 3), np.int32), stats)
        capi.check(capi.lib.osfm_dense_download_mesh(self._h, V, T, m.points.ctypes.data, m.normals.ctypes.data, m.confidence.ctypes.data,
                                                     m.scale.ctypes.data, m.pixel.ctypes.data, m.vclass.ctypes.data, m.triangles.ctypes.data))
        return m


def write_mesh(path, points, normals=None, rgb=None, confidence=None, scale=None, triangles=None):
    """osfm_dense_mesh_write: a binary little-endian PLY with MVE's property names (x y z nx ny nz, red green blue,
    confidence, value); without triangles a point set, as fssrecon reads it."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    V = points.shape[0]

    def arg(name, a, dtype, shape):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype).reshape(shape)
        if a.shape[0] != V:
            raise ValueError(f"write_mesh: {V} points, {a.shape[0]} rows of {name}")
        return a
    normals, rgb = arg("normals", normals, np.float64, (-1, 3)), arg("rgb", rgb, np.uint8, (-1, 3))
    confidence, scale = arg("confidence", confidence, np.float32, (-1,)), arg("scale", scale, np.float64, (-1,))
    tris = np.ascontiguousarray(triangles if triangles is not None else np.zeros((0, 3)), dtype=np.int32).reshape(-1, 3)
    p = lambda a: a.ctypes.data if a is not None else None
    capi.check(capi.lib.osfm_dense_mesh_write(os.fsencode(path), V, points.ctypes.data, p(normals), p(rgb), p(confidence), p(scale),
                                              tris.shape[0], tris.ctypes.data))


def read_mesh(path):
    """dict of points, normals (float32 [V, 3]), rgb (uint8 [V, 3]), confidence, scale (float32 [V]) and triangles
    (int32 [T, 3]) of a file write_mesh wrote."""
    with open(path, "rb") as f:
        counts = {}
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"read_mesh: {path}: no end_header")
            if line.startswith(b"element "):
                counts[line.split()[1].decode()] = int(line.split()[2])
            if line.strip() == b"end_header":
                break
        vrec = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3), ("confidence", "<f4"), ("value", "<f4")])
        frec = np.dtype([("n", "u1"), ("v", "<i4", 3)])
        V, T = counts.get("vertex", 0), counts.get("face", 0)
        v = np.frombuffer(f.read(V * vrec.itemsize), dtype=vrec, count=V)
        t = np.frombuffer(f.read(T * frec.itemsize), dtype=frec, count=T)
    if T and not (t["n"] == 3).all():
        raise ValueError(f"read_mesh: {path}: a face that is no triangle")
    return dict(points=v["xyz"].copy(), normals=v["n"].copy(), rgb=v["rgb"].copy(), confidence=v["confidence"].copy(),
                scale=v["value"].copy(), triangles=t["v"].copy().reshape(-1, 3))


def write_cloud(path, points, rgb=None):
    """osfm_dense_cloud_write: a binary little-endian PLY of float x, y, z and uchar red, green, blue."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if rgb is not None:
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
        if rgb.shape[0] != points.shape[0]:
            raise ValueError(f"write_cloud: {points.shape[0]} points, {rgb.shape[0]} colours")
    capi.check(capi.lib.osfm_dense_cloud_write(os.fsencode(path), points.shape[0], points.ctypes.data,
                                               rgb.ctypes.data if rgb is not None else None))


def read_cloud(path):
    """(points float32 [N, 3], rgb uint8 [N, 3]) of a file write_cloud wrote."""
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"read_cloud: {path}: no end_header")
            if line.startswith(b"element vertex"):
                n = int(line.split()[2])
            if line.strip() == b"end_header":
                break
        rec = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
        data = np.frombuffer(f.read(), dtype=rec, count=n)
    return data["xyz"].copy(), data["rgb"].copy()
