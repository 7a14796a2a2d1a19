"""The cases of tests/mesh_cases.py and the restatement tests/mesh_restatement.py, on the CPU: the cases reach every
branch they name, the restatement's vertex classes are those of a brute-force edge count, every face looks at the
camera, a plane comes out as a plane, the planted errors are seen, and the restatement's meshes of the restatement's
sweeps are as good as recorded."""
from collections import Counter

import numpy as np
import pytest

import dense_cases as dc
import dense_restatement as dr
import mesh_cases as mc
import mesh_restatement as mr

ALL_RUNS = mc.runs()


def _blocks(m):
    """(mask, z of the four pixels) of every 2 x 2 block of a map, row-major."""
    solid = m.status == dr.OK
    h, w = solid.shape
    out = []
    for y in range(h - 1):
        for x in range(w - 1):
            px = ((y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1))
            out.append((sum(1 << c for c in range(4) if solid[px[c]]), [m.depth[p] for p in px]))
    return out


def test_quads_reach_every_mask_diagonal_and_threshold():
    m, = mc.case("quads")
    blocks = _blocks(m)
    masks = Counter(mask for mask, _ in blocks)
    assert all(masks[k] >= 1 for k in (7, 11, 13, 14, 15, 3, 9))
    full = [z for mask, z in blocks if mask == 15]
    first = [abs(z[0] - z[3]) < abs(z[1] - z[2]) for z in full]
    ties = [abs(z[0] - z[3]) == abs(z[1] - z[2]) for z in full]
    assert any(first) and any(not a and not t for a, t in zip(first, ties))
    assert any(t and z[0] == z[3] for t, z in zip(ties, full)) and any(t and z[0] != z[3] for t, z in zip(ties, full))
    straight = {abs(z[i] - z[j]) for mask, z in blocks for i, j in ((0, 1), (0, 2), (1, 3), (2, 3)) if mask >> i & 1 and mask >> j & 1}
    diagonal = {abs(z[i] - z[j]) for mask, z in blocks for i, j in ((0, 3), (1, 2)) if mask >> i & 1 and mask >> j & 1}
    above = lambda v: float(np.nextafter(v, np.inf))
    assert {mc.DD, above(mc.DD)} <= straight and {mc.DD_DIAG, above(mc.DD_DIAG)} <= diagonal
    assert mr.footprint(dr.Geometry(m.P)) == 1.0
    assert [r.get("dd_factor") for r in m.runs[:2]] == [mc.DD, 0.0]
    # what each quad gives, by hand
    cut, free = mc.restated("quads", 0, 0), mc.restated("quads", 0, 1)
    want = dict(mask7=1, mask11=1, mask13=1, mask14=1, two_pixels=0, two_diagonal=0, diagonal_03=2, diagonal_12=2, tie_flat=2,
                tie_sloped=2, straight_at=2, straight_above=1, diagonal_at=1, diagonal_above=0, between=0, between_diagonal=1, cliff=0)
    for k, (name, mask, _) in enumerate(mc.quad_list()):
        x0 = m.paths["first_x"] + m.paths["pitch"] * k
        mine = lambda mesh: int(((mesh["pixel"][mesh["triangles"][:, 0], 0] >= x0) & (mesh["pixel"][mesh["triangles"][:, 0], 0] <= x0 + 1)).sum())
        assert mine(cut) == want[name], name
        assert mine(free) == (0 if mask in (3, 9) else 2 if mask == 15 else 1), name
    assert cut["stats"]["triangles_dropped"] == 5 and free["stats"]["triangles_dropped"] == 0
    # the vertex orders are MVE's: T2, T3 on one diagonal, T1, T4 on the other
    tri_px = lambda mesh, t: [tuple(int(v) for v in mesh["pixel"][i]) for i in mesh["triangles"][t]]
    names = [q[0] for q in mc.quad_list()]
    x0 = m.paths["first_x"] + m.paths["pitch"] * names.index("diagonal_03")
    t0 = int(np.nonzero(cut["pixel"][cut["triangles"][:, 0], 0] == x0)[0][0])
    assert tri_px(cut, t0) == [(x0, 1), (x0 + 1, 2), (x0 + 1, 1)] and tri_px(cut, t0 + 1) == [(x0, 1), (x0, 2), (x0 + 1, 2)]
    x0 = m.paths["first_x"] + m.paths["pitch"] * names.index("tie_flat")
    t0 = int(np.nonzero(cut["pixel"][cut["triangles"][:, 0], 0] == x0)[0][0])
    assert tri_px(cut, t0) == [(x0, 1), (x0, 2), (x0 + 1, 1)] and tri_px(cut, t0 + 1) == [(x0 + 1, 1), (x0, 2), (x0 + 1, 2)]


def _vertex_at(mesh, x, y):
    hit = np.nonzero((mesh["pixel"][:, 0] == x) & (mesh["pixel"][:, 1] == y))[0]
    return int(hit[0]) if hit.size else None


def test_classes_reach_every_class_the_hole_and_saturation():
    m, = mc.case("classes")
    mesh = mc.restated("classes", 0, 0)
    assert {mr.SIMPLE, mr.BORDER, mr.COMPLEX} == set(int(c) for c in mesh["vclass"])
    assert mesh["vclass"][_vertex_at(mesh, *m.paths["bow_tie"])] == mr.COMPLEX
    hx, hy = m.paths["hole"]
    assert _vertex_at(mesh, hx, hy) is None
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        v = _vertex_at(mesh, hx + dx, hy + dy)
        assert mesh["vclass"][v] == mr.BORDER and mesh["confidence"][v] == 0.0
    K = mr.DEFAULTS["confidence_iterations"]
    assert mesh["confidence"][_vertex_at(mesh, *m.paths["centre"])] == 1.0
    assert set(np.unique(mesh["confidence"])) == {np.float32(k) / np.float32(K) for k in range(K + 1)}
    runs = {r.get("confidence_iterations", K): mc.restated("classes", 0, j) for j, r in enumerate(m.runs)}
    assert (runs[0]["confidence"] == 1.0).all()
    assert set(np.unique(runs[1]["confidence"])) == {0.0, 1.0}
    deep = runs[mc.MAX_CONFIDENCE_ITERATIONS]["confidence"]
    assert 0.0 < deep.max() < 1.0                                # the mesh is not that wide: nothing saturates
    # the two triangles of the bow tie hold no border vertex but their own: COMPLEX is no seed, yet it gets a distance
    assert mesh["confidence"][_vertex_at(mesh, *m.paths["bow_tie"])] == np.float32(1.0) / np.float32(K)


def test_islands_reach_the_threshold_and_every_seam():
    shapes, snake = mc.case("islands")
    tw, th = mc.LABEL_TILE
    solid = shapes.status == dr.OK
    assert solid.shape == (81, 97)
    kept = mc.restated("islands", 0, 0)["solid"]
    _, _, comps = mr.clear_islands(solid, 0)
    for name, (y, x, stays) in shapes.paths.items():
        assert solid[y, x] and kept[y, x] == stays, name
    # the sizes around the threshold, and the tiles the seam shapes touch
    size = lambda name: int(_component(solid, *shapes.paths[name][:2]).sum())
    assert [size(n) for n in ("below", "equal", "above")] == [mc.MIN_ISLAND - 1, mc.MIN_ISLAND, mc.MIN_ISLAND + 1]
    tiles = lambda name: {(x // tw, y // th) for y, x in zip(*np.nonzero(_component(solid, *shapes.paths[name][:2])))}
    assert len({t[0] for t in tiles("vertical_seam")}) == 2 and len({t[0] for t in tiles("vertical_seam_below")}) == 2
    assert len({t[1] for t in tiles("horizontal_seam")}) == 2 and len({t[1] for t in tiles("horizontal_seam_below")}) == 2
    assert len(tiles("corner")) == 4 and len(tiles("corner_below")) == 4
    assert size("vertical_seam") == size("horizontal_seam") == mc.MIN_ISLAND and size("corner_below") == mc.MIN_ISLAND - 1
    assert size("vertical_seam_below") == size("horizontal_seam_below") == mc.MIN_ISLAND - 1
    # the diagonal pair would stay if a diagonal joined them
    a, b = shapes.paths["diagonal_a"], shapes.paths["diagonal_b"]
    assert size("diagonal_a") + size("diagonal_b") == mc.MIN_ISLAND and solid[a[0] + 1, a[1] + 2] and solid[b[0], b[1]]
    assert (b[0], b[1]) == (a[0] + 2, a[1] + 3)
    assert size("checkerboard") == 1 and comps > 80
    # the serpentine: one component, one pixel wide, in every tile
    s = snake.status == dr.OK
    assert mr.clear_islands(s, 0)[2] == 1 and int(s.sum()) == snake.paths["size"]
    assert {(x // tw, y // th) for y, x in zip(*np.nonzero(s))} == {(i, j) for i in range(4) for j in range(6)}
    assert mc.restated("islands", 1, 0)["solid"].sum() == s.sum() and mc.restated("islands", 1, 1)["solid"].sum() == 0
    assert mc.restated("islands", 1, 0)["stats"]["vertices_complex"] > 0


def _component(solid, y, x):
    """The 4-connected component of (y, x), as a plane."""
    out = np.zeros_like(solid)
    todo = [(y, x)]
    out[y, x] = True
    while todo:
        y, x = todo.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < solid.shape[0] and 0 <= xx < solid.shape[1] and solid[yy, xx] and not out[yy, xx]:
                out[yy, xx] = True
                todo.append((yy, xx))
    return out


def test_tiny_sizes():
    shapes = {m.status.shape for m in mc.case("tiny")}
    assert shapes == {(1, 1), (5, 1), (1, 5), (2, 2)}
    for i, m in enumerate(mc.case("tiny")):
        for j in range(len(m.runs)):
            mesh = mc.restated("tiny", i, j)
            full = m.status.shape == (2, 2) and (m.status == dr.OK).all() and m.runs[j].get("min_island", 0) <= 4
            assert mesh["triangles"].shape == ((2, 3) if full else (0, 3)) and mesh["points"].shape == ((4, 3) if full else (0, 3))


@pytest.mark.parametrize("name,i,j", ALL_RUNS)
def test_classes_equal_an_edge_count(name, i, j):
    """An edge of one triangle is a border edge.  On these meshes (triangles that do not overlap in the image) a
    vertex with no border edge has a closed fan, one with two has one open chain, one with more has several."""
    mesh = mc.restated(name, i, j)
    edges = Counter()
    for a, b, c in mesh["triangles"]:
        for e in ((a, b), (b, c), (a, c)):
            edges[(min(e), max(e))] += 1
    assert all(n <= 2 for n in edges.values())
    border = np.zeros(mesh["points"].shape[0], np.int64)
    for (a, b), n in edges.items():
        if n == 1:
            border[a] += 1
            border[b] += 1
    want = np.where(border == 0, mr.SIMPLE, np.where(border == 2, mr.BORDER, mr.COMPLEX))
    assert np.array_equal(mesh["vclass"], want)


@pytest.mark.parametrize("name,i,j", ALL_RUNS)
def test_every_face_looks_at_the_camera(name, i, j):
    m, mesh = mc.case(name)[i], mc.restated(name, i, j)
    d = np.array(dr.Geometry(m.P).d)
    assert (mr.face_normals(mesh["points"], mesh["triangles"]) @ d < 0.0).all()
    assert (mesh["normals"] @ d < 0.0).all()
    assert np.abs(np.linalg.norm(mesh["normals"], axis=1) - 1.0).max(initial=0.0) < 1e-15 * 4


@pytest.mark.parametrize("i", [0, 1])
def test_a_plane_comes_out_as_a_plane(i):
    m, mesh = mc.case("slanted_exact")[i], mc.restated("slanted_exact", i, 0)
    geo = dr.Geometry(m.P)
    n = mc.plane_normal(m.P, dc.SLANT)
    inner = mesh["vclass"] == mr.SIMPLE
    assert inner.sum() == (m.status.shape[0] - 2) * (m.status.shape[1] - 2)
    assert np.abs(mesh["normals"][inner] - n).max() < 1e-9
    # a step of one pixel along x or y moves the surface point by B's column plus the depth that keeps it on the plane
    B, d = np.array(geo.B), np.array(geo.d)
    ex, ey = (B[:, k] - (n @ B[:, k]) / (n @ d) * d for k in (0, 1))
    zx, zy = -(n @ B[:, 0]) / (n @ d), -(n @ B[:, 1]) / (n @ d)
    across = ex + ey if abs(zx + zy) < abs(zx - zy) else ex - ey          # the diagonal every block takes
    want = (2 * np.linalg.norm(ex) + 2 * np.linalg.norm(ey) + 2 * np.linalg.norm(across)) / 6.0
    assert np.abs(mesh["scale"][inner] - want).max() < 1e-9
    assert (mesh["confidence"][inner] > 0.0).all() and (mesh["confidence"][~inner] == 0.0).all()


def test_planted_errors_are_seen():
    def differs(name, i, j, planted):
        m = mc.case(name)[i]
        a, b = mc.restated(name, i, j), mr.mesh(m.P, m.depth, m.status, m.dz, planted=planted, **m.runs[j])
        return a["triangles"].shape != b["triangles"].shape or not np.array_equal(a["triangles"], b["triangles"]) or \
            not np.array_equal(a["solid"], b["solid"])
    assert differs("quads", 0, 0, "swap_diagonal") and differs("quads", 0, 0, "cut_equal") and differs("islands", 0, 0, "island_equal")
    assert not differs("quads", 0, 0, "island_equal") and not differs("islands", 0, 0, "cut_equal")
    # each is seen where it should be: the threshold quads lose their triangles, the island of min_island pixels goes
    m, = mc.case("quads")
    assert mr.mesh(m.P, m.depth, m.status, m.dz, planted="cut_equal", **m.runs[0])["stats"]["triangles_dropped"] == 5 + 2
    shapes = mc.case("islands")[0]
    y, x, _ = shapes.paths["equal"]
    assert not mr.mesh(shapes.P, shapes.depth, shapes.status, shapes.dz, planted="island_equal", **shapes.runs[0])["solid"][y, x]


@pytest.mark.parametrize("name", ["slanted", "step"])
def test_meshes_of_the_restated_sweeps_against_the_exact_surfaces(name):
    angle, share, far = mc.surface_accuracy(name)
    print(f"{name}: median angle to the plane normal {angle:.4f} deg, {share:.4f} of the {far} vertices farther than a step have confidence 0")
    rec = mc.MEASURED_CPU[name]
    assert abs(angle - rec["median_angle_deg"]) <= 5e-4 and abs(share - rec["far_with_confidence_0"]) <= 5e-4 and far == rec["far"]
    # positions are the fusion's formula on the map's own depth
    c = dc.case(name)
    for sw, m, mesh in zip(c.sweeps, dc.restated(name), mc.sweep_meshes(name)):
        px = mesh["pixel"]
        X = dr.Geometry(c.P[sw.ref]).point(px[:, 0].astype(np.float64), px[:, 1].astype(np.float64), m["depth"][px[:, 1], px[:, 0]])
        assert np.array_equal(np.stack(X, axis=1), mesh["points"])
        assert (m["status"][px[:, 1], px[:, 0]] == dr.OK).all()
