"""The definition of the depth-map meshes (include/osfm_hip.h, "A mesh per depth map"; DESIGN.md "Depth-map meshes")
in float64 numpy: what MVE does between dmrecon and fssrecon -- depthmap_cleanup, depthmap_triangulate, the vertex
normals, depthmap_mesh_confidences, the scale of scene2pset -- for orthographic views.  The kernels of
orthosfm_amd/csrc/mesh_kernels.hip are held to it.

Only the islands and the triangles know the image grid.  Everything after them -- vertices, normals, scales, classes,
confidences -- works on plain vertex and face lists, as MVE's MeshInfo does, so that the device's grid-local logic is
checked and not mirrored.  Every sum that reaches an output is written out in one fixed order, which the kernels
repeat.
"""
import math
from collections import deque

import numpy as np

import dense_restatement as dr

SIMPLE, BORDER, COMPLEX = range(3)
CLASS_NAMES = ("SIMPLE", "BORDER", "COMPLEX")
DEFAULTS = dict(dd_factor=5.0, confidence_iterations=3, min_island=0, use_fused=0)
MAX_CONFIDENCE_ITERATIONS = 16
# block-local corners 0 = (x, y), 1 = (x+1, y), 2 = (x, y+1), 3 = (x+1, y+1); T1..T4 in MVE's vertex order
TRIANGLES = ((0, 2, 1), (0, 3, 1), (0, 2, 3), (1, 2, 3))


def footprint(geo):
    """sqrt(|b0 x b1|) of the columns of B: the side of a world square with a pixel's area."""
    b0, b1 = [geo.B[j][0] for j in range(3)], [geo.B[j][1] for j in range(3)]
    c = (b0[1] * b1[2] - b0[2] * b1[1], b0[2] * b1[0] - b0[0] * b1[2], b0[0] * b1[1] - b0[1] * b1[0])
    return math.sqrt(math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]))


def solid_pixels(status, final=None, use_fused=0):
    s = np.asarray(status) == dr.OK
    if use_fused:
        f = np.asarray(final)
        s = s & ((f == dr.OK) | (f == dr.DUPLICATE))
    return s


def clear_islands(solid, min_island, keep_equal=True):
    """(solid without the 4-connected components of fewer than min_island pixels, pixels cleared, components).
    keep_equal=False is the planted error of test_mesh_cases_cpu.py: <= for <."""
    h, w = solid.shape
    out = solid.copy()
    seen = np.zeros((h, w), bool)
    cleared = components = 0
    for y0, x0 in zip(*np.nonzero(solid)):
        if seen[y0, x0]:
            continue
        components += 1
        seen[y0, x0] = True
        todo, members = deque([(y0, x0)]), []
        while todo:
            y, x = todo.popleft()
            members.append((y, x))
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < h and 0 <= xx < w and solid[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    todo.append((yy, xx))
        small = len(members) < min_island if keep_equal else len(members) <= min_island
        if small:
            cleared += len(members)
            for y, x in members:
                out[y, x] = False
    return out, cleared, components


def triangulate(solid, depth, thr, swap_diagonal=False, cut_equal=False):
    """(triangles [T, 3] of pixel indices y w + x, dropped): blocks row-major, first triangle before the second.
    thr: dd_factor f_r, 0 for none.  swap_diagonal, cut_equal: the planted errors of test_mesh_cases_cpu.py."""
    h, w = solid.shape
    thr_diag = thr * math.sqrt(2.0)
    tris, dropped = [], 0
    for y in range(h - 1):
        for x in range(w - 1):
            px = ((y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1))
            mask = sum(1 << c for c in range(4) if solid[px[c]])
            if bin(mask).count("1") < 3:
                continue
            z = [float(depth[p]) if solid[p] else 0.0 for p in px]
            if mask == 15:
                first = abs(z[0] - z[3]) < abs(z[1] - z[2])
                if swap_diagonal:
                    first = not first
                cand = (1, 2) if first else (0, 3)
            else:
                cand = ({7: 0, 11: 1, 13: 2, 14: 3}[mask],)
            for t in cand:
                c = TRIANGLES[t]
                cut = False
                if thr > 0.0:
                    for i, j in ((c[0], c[1]), (c[1], c[2]), (c[0], c[2])):
                        lim = thr_diag if i + j == 3 else thr
                        diff = abs(z[i] - z[j])
                        cut = cut or (diff >= lim if cut_equal else diff > lim)
                if cut:
                    dropped += 1
                else:
                    tris.append([px[k][0] * w + px[k][1] for k in c])
    return np.array(tris, np.int64).reshape(-1, 3), dropped


# ---- plain vertex and face lists ---------------------------------------------------------------------------------

def incident_faces(num_vertices, tris):
    """Per vertex the indices of its triangles, ascending."""
    inc = [[] for _ in range(num_vertices)]
    for t, tri in enumerate(tris):
        for v in tri:
            inc[int(v)].append(t)
    return inc


def neighbours(num_vertices, tris):
    """Per vertex the vertices it shares a triangle with, ascending."""
    nb = [set() for _ in range(num_vertices)]
    for a, b, c in tris:
        a, b, c = int(a), int(b), int(c)
        nb[a].update((b, c)); nb[b].update((a, c)); nb[c].update((a, b))
    return [sorted(s) for s in nb]


def face_normals(points, tris):
    """cross(b - a, c - a) per triangle, components written out."""
    out = np.zeros((len(tris), 3))
    for t, (a, b, c) in enumerate(tris):
        u = [float(points[b][j]) - float(points[a][j]) for j in range(3)]
        v = [float(points[c][j]) - float(points[a][j]) for j in range(3)]
        out[t] = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    return out


def vertex_normals(points, tris):
    """(unit normals [V, 3], zero [V]): the area-weighted sum of the incident face normals in ascending triangle
    index, over its length; a zero sum gives normal 0."""
    fn = face_normals(points, tris)
    V = len(points)
    out, zero = np.zeros((V, 3)), np.zeros(V, bool)
    for v, faces in enumerate(incident_faces(V, tris)):
        s = [0.0, 0.0, 0.0]
        for t in faces:
            for j in range(3):
                s[j] += float(fn[t][j])
        nn = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        if nn > 0.0:
            out[v] = (s[0] / nn, s[1] / nn, s[2] / nn)
        else:
            zero[v] = True
    return out, zero


def vertex_scales(points, tris):
    """The mean length of the mesh edges at a vertex, neighbours ascending."""
    out = np.zeros(len(points))
    for v, nb in enumerate(neighbours(len(points), tris)):
        total = 0.0
        for n in nb:
            d = [float(points[n][j]) - float(points[v][j]) for j in range(3)]
            total += math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        out[v] = total / float(len(nb)) if nb else 0.0
    return out


def vertex_classes(num_vertices, tris):
    """MVE's MeshInfo by chaining: around vertex v a triangle (v, b, c) -- rotated so that v comes first -- leads
    from b to c, and is followed by the triangle that starts where it ends.  One chain that closes: SIMPLE; one that
    stays open: BORDER; more than one: COMPLEX."""
    out = np.zeros(num_vertices, np.uint8)
    for v, faces in enumerate(incident_faces(num_vertices, tris)):
        steps, arrivals, fan = {}, set(), True
        for t in faces:
            tri = [int(i) for i in tris[t]]
            k = tri.index(v)
            b, c = tri[(k + 1) % 3], tri[(k + 2) % 3]
            fan = fan and b not in steps and c not in arrivals      # an edge that two triangles leave or reach: no fan
            steps[b] = c
            arrivals.add(c)
        if not fan:
            out[v] = COMPLEX
            continue
        chains, closed = 0, False
        for b in [b for b in steps if b not in arrivals]:           # the open chains, each from its first edge
            chains += 1
            while b in steps:
                b = steps.pop(b)
        while steps:                                                 # what is left closes on itself
            b0 = next(iter(steps))
            b = steps.pop(b0)
            while b != b0:
                b = steps.pop(b)
            chains, closed = chains + 1, True
        out[v] = SIMPLE if (chains == 1 and closed) else BORDER if chains == 1 else COMPLEX
    return out


def confidences(num_vertices, tris, vclass, iterations, zero=None):
    """float32(min(dist, K)) / float32(K) with dist the graph distance along mesh edges to the nearest BORDER vertex
    (COMPLEX vertices are no seeds; unreachable: 1); K = 0: all 1.  zero: vertices with a zero normal sum, confidence 0."""
    K = int(iterations)
    conf = np.ones(num_vertices, np.float32)
    if K > 0:
        nb = neighbours(num_vertices, tris)
        dist = np.full(num_vertices, -1, np.int64)
        todo = deque(int(v) for v in np.nonzero(np.asarray(vclass) == BORDER)[0])
        for v in todo:
            dist[v] = 0
        while todo:
            v = todo.popleft()
            for n in nb[v]:
                if dist[n] < 0:
                    dist[n] = dist[v] + 1
                    todo.append(n)
        d = np.where(dist < 0, K, np.minimum(dist, K))
        conf = d.astype(np.float32) / np.float32(K)
    if zero is not None:
        conf = np.where(zero, np.float32(0.0), conf).astype(np.float32)
    return conf


# ---- the mesh of a view ---------------------------------------------------------------------------------------------

def mesh(P, depth, status, dz, final=None, planted=None, **options):
    """The mesh of one view: dict of points [V, 3], normals [V, 3], confidence [V] float32, scale [V], pixel [V, 2]
    int32 (x, y), vclass [V] uint8, triangles [T, 3] int32 (vertex indices), solid (after the islands) and stats (the
    counters of osfm_dense_mesh_stats and threshold_steps).  planted: one of the deliberate errors of
    test_mesh_cases_cpu.py ("swap_diagonal", "island_equal", "cut_equal")."""
    o = dict(DEFAULTS)
    o.update(options)
    geo = dr.Geometry(P)
    depth, status = np.asarray(depth, dtype=np.float64), np.asarray(status)
    h, w = status.shape
    solid = solid_pixels(status, final, o["use_fused"])
    stats = dict(pixels_solid=int(solid.sum()), pixels_island=0, components=0)
    if o["min_island"] > 0:
        solid, stats["pixels_island"], stats["components"] = clear_islands(solid, int(o["min_island"]), planted != "island_equal")
    thr = float(o["dd_factor"]) * footprint(geo)
    px_tris, stats["triangles_dropped"] = triangulate(solid, depth, thr, planted == "swap_diagonal", planted == "cut_equal")
    used = np.unique(px_tris)                                   # row-major pixel order
    index = np.full(h * w, -1, np.int64)
    index[used] = np.arange(used.shape[0])
    tris = index[px_tris].reshape(-1, 3)
    xs, ys = (used % w).astype(np.float64), (used // w).astype(np.float64)
    X = geo.point(xs, ys, depth.reshape(-1)[used]) if used.shape[0] else (np.zeros(0),) * 3
    points = np.stack(X, axis=1).reshape(-1, 3)
    V = points.shape[0]
    normals, zero = vertex_normals(points, tris)
    vclass = vertex_classes(V, tris)
    stats.update(vertices_simple=int((vclass == SIMPLE).sum()), vertices_border=int((vclass == BORDER).sum()),
                 vertices_complex=int((vclass == COMPLEX).sum()), threshold_steps=thr / float(dz))
    return dict(points=points, normals=normals, confidence=confidences(V, tris, vclass, o["confidence_iterations"], zero),
                scale=vertex_scales(points, tris), pixel=np.stack([used % w, used // w], axis=1).astype(np.int32).reshape(-1, 2),
                vclass=vclass, triangles=tris.astype(np.int32), solid=solid, stats=stats)
