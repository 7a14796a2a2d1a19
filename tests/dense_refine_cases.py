"""Cases of the slanted-plane refinement (tests/dense_refine_restatement.py is the definition;
tests/test_dense_refine_cases_cpu.py checks the cases, tests/test_dense_refine_gpu.py holds the library to them).

The scenes are those of tests/dense_cases.py, which this file imports and does not change, and two of its own:
`steep`, a plane several times as tilted as dense_cases.SLANT, and `edge`, a plane whose texture gives way, in a band,
to one smooth straight edge.  The input of every case is the restatement's sweep (dense_cases.restated), uploaded with
osfm_dense_set_map, so that the float32 ambiguity of the sweep stays out of the comparison.
"""
from functools import lru_cache

import numpy as np

import dense_cases as dc
import dense_restatement as dr
import dense_refine_restatement as drr
import refine_cases as rcs

# A pixel is ambiguous where the restatement's margin (the smallest distance of any deciding comparison from its
# threshold: relative for the convergence test, the pivots, the shift and the singular values, absolute for the
# scores, in pixels for the samples' slack to the image border) is below this band: the device may decide it the
# other way.  1e-6 as in refine_cases; test_dense_refine_cases_cpu.py holds every case to at most AMBIGUOUS_SHARE of
# its tested pixels inside it.
AMBIGUITY_BAND = 1e-6
AMBIGUOUS_SHARE = 0.01

# The pivot threshold of ILL_CONDITIONED (osfm_dense_refine_options.min_pivot), measured with the restatement on the
# CPU over PIVOT_CASES, run with min_pivot 1e-12 so that nothing stops it (pivot_figures();
# test_dense_refine_cases_cpu.py::test_pivot_threshold measures again).
#   textured_min: the smallest, over the REFINED pixels of PIVOT_TEXTURED, of the smallest scaled pivot of their
#   iterations.
#   edge_only_*: the same pivot over the pixels of `edge` whose windows see the straight edge and nothing else.  They
#   are NOT small (median 0.25): a texture with one direction only is no degenerate case here as it is for the 2-D
#   matcher of refine_cases.PIVOT, because only the derivative along the epipolar line enters, and an edge that
#   crosses the window fixes the depth at every point along itself, and with that both tilts.  What makes a pivot small
#   is gradient that is concentrated in a corner of the window (the rim of a flat region, a lone blob): (1, ux, uy)
#   are then nearly dependent under the weights a^2.
#   So the threshold is not put between those two but where refining stops paying: over the REFINED pixels with a
#   pivot in [0.02, threshold) the 90th percentile of |z - z_exact| is worse after the refinement than before
#   (`below`), in [threshold, 0.05) it is better (`above`); 0.035 is that point to two digits, and lies below
#   textured_min.
PIVOT = {"threshold": 0.035, "textured_min": 0.0407127, "edge_only_min": 0.0191050, "edge_only_median": 0.2537200, "edge_only_pixels": 345,
         "below": {"pixels": 39, "p90_sweep": 0.5214, "p90_refined": 0.9778}, "above": {"pixels": 88, "p90_sweep": 0.7237, "p90_refined": 0.5908}}

# The restatement against the exact depth, measured on the CPU (test_dense_refine_cases_cpu.py measures again and
# holds them), per case over the REFINED pixels of all its sweeps: the median |z - z_exact| in steps before and after
# the refinement, the median angle in degrees between the refined normal and the normal of the plane each pixel shows,
# and the same angle for mesh_restatement's vertex normals of the unrefined map on the same pixels.
MEASURED_CPU = {
    "slanted": {"median_steps_sweep": 0.1298, "median_steps_refined": 0.0779, "normal_deg_refined": 4.1315, "normal_deg_mesh": 6.8476},
    "steep": {"median_steps_sweep": 0.2770, "median_steps_refined": 0.0674, "normal_deg_refined": 3.5110, "normal_deg_mesh": 12.0489},
    "step": {"median_steps_sweep": 0.1118, "median_steps_refined": 0.0582, "normal_deg_refined": 2.4163, "normal_deg_mesh": 5.2485},
}
# The statuses `step` reaches over its four sweeps, in the order of dense_refine_restatement.STATUS_NAMES: windows across
# the strip's edge are where the rejections come from.
STEP_COUNTS = (11785, 16658, 97, 13, 2097, 30, 32, 8)

# What densify(refine=True) gives on dense_cases.pipeline_scene() under the restatements (restated_pipeline()), beside
# dense_cases.MEASURED_CPU_PIPELINE of the unrefined path (median 0.0416): dense_cases.cloud_accuracy of the fusion of
# the refined maps -- the median |z - z_exact| in steps, the share within one step, the points per plane.
MEASURED_CPU_PIPELINE = {"median_steps": 0.0383, "within_one_step": 0.9999, "points": (10936, 2691)}

# Agreement of the device with the restatement over the pixels REFINED on both sides and not ambiguous, all cases,
# measured once on an MI355X (tests/test_dense_refine_gpu.py prints the figures): the largest |z| difference in steps,
# the largest gradient difference times the radius in steps, the largest difference of a normal's component and of the
# score (float32 on both sides).
MEASURED = {"depth_steps": 0.0, "gradient_steps": 0.0, "normal": 0.0, "score": 0.0}
# Ten times the measured figures, no less than 1e-9 (what another order of the sums can do: refine_cases.BOUNDS gives
# the reasoning, and the pivots here are no smaller), and never above the ceilings beyond which the arithmetic
# differs, not the rounding: 1e-6 of a step, 1e-6 in a normal's component.
CEILINGS = {"depth_steps": 1e-6, "gradient_steps": 1e-6, "normal": 1e-6, "score": 1e-6}
BOUNDS = {k: min(max(10.0 * MEASURED[k], 1e-9), CEILINGS[k]) for k in CEILINGS}


STEEP = dc.Plane(0.6, -0.4, -11.2, 109)
EDGE = dc.Plane(0.15, 0.10, -11.2, 111)
EDGE_BAND = (30.0, 66.0, 0.35)                       # refine_cases.texture's edge: X from, X to, angle


def _render_with(P, w, h, planes, textures):
    """dense_cases.render with a texture function per plane."""
    _, which, X = dc.trace(dr.Geometry(P), w, h, planes)
    v = np.zeros((h * w, 3))
    for i in range(len(planes)):
        sel = (which == i).ravel()
        if sel.any():
            v[sel] = textures[i](np.stack([X[0].ravel()[sel], X[1].ravel()[sel]], axis=1))
    acc = v.reshape(h, w, 3)
    return np.ascontiguousarray(np.clip(np.floor((0.5 + acc.mean(axis=2)) * 255.0 + 0.5), 0, 255).astype(np.uint8))


def _steep():
    cams = dc._ring(4)
    sweeps = [(r, [s for s in range(4) if s != r], {}, (dr.OK,)) for r in range(2)]
    return dc._build("steep", cams, [STEEP], sweeps, options=dict(radius=2))


def _edge():
    cams = dc._ring(4)
    P = np.stack([c[2] for c in cams])
    sizes = [(c[0], c[1]) for c in cams]
    tex = rcs.texture(EDGE.seed, 800, lo=(-50.0, -50.0), hi=(150.0, 130.0), edge=EDGE_BAND)
    images = [_render_with(P[v], sizes[v][0], sizes[v][1], [EDGE], [tex]) for v in range(4)]
    z_min, dz, D = dc.plan(P, sizes, [EDGE], 0, [1, 2, 3])
    return dc.Case("edge", images, P, [EDGE], [dc.Sweep(0, (1, 2, 3), z_min, dz, D, {}, (dr.OK,))], dict(radius=3))


OWN = {"steep": _steep, "edge": _edge}


@lru_cache(maxsize=None)
def scene(name):
    """The dense_cases.Case behind a case of this file."""
    return OWN[name]() if name in OWN else dc.case(name)


@lru_cache(maxsize=None)
def swept(name):
    """The restatement's sweeps of scene(name), in order: computed once, shared, not to be modified."""
    if name not in OWN:
        return dc.restated(name)
    c = scene(name)
    out = []
    for sw in c.sweeps:
        m = dr.sweep(c.images, c.P, sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, **dc.sweep_options(c, sw))
        for a in m.values():
            a.setflags(write=False)
        out.append(m)
    return tuple(out)


S = drr
CASES = {
    # the window sizes at both ends of the range: 9 samples over 16 lanes (fewer than a lane each) and 225 (15 rounds)
    "slanted": dict(sweeps=(0, 1, 2, 3), reach=(S.NOT_OK, S.REFINED, S.NOT_CONVERGED)),
    "radius1": dict(sweeps=(0,), reach=(S.REFINED, S.NOT_CONVERGED, S.ILL_CONDITIONED)),
    "radius7": dict(sweeps=(0,), reach=(S.REFINED,)),
    # one pixel column and one row into a new 4 x 4 block; RGB sources of other sizes
    "odd_sizes": dict(sweeps=(0,), reach=(S.REFINED,)),
    # sources that stop counting depending on depth and tilt; the touch pixel's window ends on view 3's last row and column
    "border": dict(sweeps=(0, 1), reach=(S.REFINED, S.NOT_CONVERGED)),
    "one_source": dict(sweeps=(0,), reach=(S.REFINED,)),
    "eight_sources": dict(sweeps=(0,), reach=(S.REFINED,)),
    "flat": dict(sweeps=(0,), reach=(S.NOT_OK, S.REFINED, S.ILL_CONDITIONED)),
    "step": dict(sweeps=(0, 1, 2, 3), reach=(S.REFINED, S.OUTSIDE, S.ILL_CONDITIONED, S.NOT_CONVERGED, S.REJECT_SHIFT, S.REJECT_SLOPE, S.REJECT_SCORE)),
    "empty": dict(sweeps=(0,), reach=(S.NOT_OK,)),
    "steep": dict(sweeps=(0, 1), reach=(S.REFINED, S.OUTSIDE, S.REJECT_SHIFT)),
    "edge": dict(sweeps=(0,), reach=(S.REFINED, S.ILL_CONDITIONED)),
}
NAMES = tuple(CASES)
ACCURACY = ("slanted", "steep", "step")


def refine_options(name, k):
    """The options of the refinement of sweep k of a case: the sweep's radius, min_sources and min_score."""
    c = scene(name)
    so = dc.sweep_options(c, c.sweeps[k])
    o = {key: so[key] for key in ("radius", "min_sources", "min_score") if key in so}
    o.update(CASES[name].get("options", {}))
    return o


@lru_cache(maxsize=None)
def restated(name):
    """{sweep index: the restatement's refinement} of a case: computed once, shared, not to be modified."""
    c = scene(name)
    out = {}
    for k in CASES[name]["sweeps"]:
        sw, m = c.sweeps[k], swept(name)[k]
        r = drr.refine(c.images, c.P, sw.ref, sw.sources, m["depth"], m["status"], sw.dz, score=m["score"], **refine_options(name, k))
        for a in r.values():
            a.setflags(write=False)
        out[k] = r
    return out


def tested(r):
    return r["status"] != drr.NOT_OK


def ambiguous(r):
    return tested(r) & (r["margin"] < AMBIGUITY_BAND)


def plane_normals(c, v):
    """Per pixel of view v the unit normal, towards the camera, of the plane it shows (NaN without one)."""
    _, which = c.exact(v)
    d = np.array(dr.Geometry(c.P[v]).d)
    out = np.full(which.shape + (3,), np.nan)
    for i, p in enumerate(c.planes):
        n = np.array([-p.a, -p.b, 1.0])
        n /= np.linalg.norm(n)
        if n @ d > 0.0:
            n = -n
        out[which == i] = n
    return out


def angle_deg(a, b):
    return np.degrees(np.arccos(np.clip((a * b).sum(axis=-1), -1.0, 1.0)))


def edge_only(c, v, radius):
    """The pixels of view v of `edge` whose window, and a pixel more, lies inside the band where the texture is the edge alone."""
    h, w = c.images[v].shape[:2]
    X = dc.trace(dr.Geometry(c.P[v]), w, h, c.planes)[2][0]
    inside = (X > EDGE_BAND[0] + 6.0) & (X < EDGE_BAND[1] - 6.0)
    out = inside.copy()
    for dy in range(-radius - 1, radius + 2):
        for dx in range(-radius - 1, radius + 2):
            out &= np.roll(np.roll(inside, dy, axis=0), dx, axis=1)
    out[:radius + 1] = out[-radius - 1:] = False
    out[:, :radius + 1] = out[:, -radius - 1:] = False
    return out


@lru_cache(maxsize=None)
def accuracy(name):
    """The figures of MEASURED_CPU for a case, over the REFINED pixels of all its refined sweeps."""
    import mesh_restatement as mr
    c = scene(name)
    before, after, angle, mesh_angle = [], [], [], []
    for k, r in restated(name).items():
        sw, m = c.sweeps[k], swept(name)[k]
        good = r["status"] == drr.REFINED
        exact = c.exact(sw.ref)[0]
        truth = plane_normals(c, sw.ref)
        before.append(np.abs(m["depth"] - exact)[good] / sw.dz)
        after.append(np.abs(r["depth"] - exact)[good] / sw.dz)
        angle.append(angle_deg(r["normal"], truth)[good])
        me = mr.mesh(c.P[sw.ref], m["depth"], m["status"], sw.dz)
        px = me["pixel"]
        on = good[px[:, 1], px[:, 0]]
        mesh_angle.append(angle_deg(me["normals"], truth[px[:, 1], px[:, 0]])[on])
    med = lambda parts: round(float(np.median(np.concatenate(parts))), 4)
    return {"median_steps_sweep": med(before), "median_steps_refined": med(after), "normal_deg_refined": med(angle),
            "normal_deg_mesh": med(mesh_angle)}


@lru_cache(maxsize=None)
def pipeline_maps():
    """What pipeline.densify(refine=True) works on over dense_cases.pipeline_scene(), by the restatements:
    (plans, {view: sweep}, {view: refinement})."""
    from orthosfm_amd import dense
    sc = dc.pipeline_scene()
    plans = [dense.plan_view(sc["P"], v, sc["points"][sc["visibility"][v]], range(4), max_depths=dc.MAX_DEPTHS) for v in range(4)]
    maps = {v: dr.sweep(sc["images"], sc["P"], v, p.sources, p.z_min, p.dz, p.num_depths, **dc.PIPELINE_OPTIONS) for v, p in enumerate(plans)}
    o = {key: dc.PIPELINE_OPTIONS[key] for key in ("radius", "min_sources", "min_score") if key in dc.PIPELINE_OPTIONS}
    refined = {v: drr.refine(sc["images"], sc["P"], v, p.sources, maps[v]["depth"], maps[v]["status"], p.dz, score=maps[v]["score"], **o)
               for v, p in enumerate(plans)}
    return plans, maps, refined


@lru_cache(maxsize=None)
def restated_pipeline():
    """(plans, the restated fusion of the refined maps) on dense_cases.pipeline_scene()."""
    sc = dc.pipeline_scene()
    plans, maps, refined = pipeline_maps()
    after = {v: dict(depth=refined[v]["depth"], status=maps[v]["status"]) for v in maps}
    return plans, dr.fuse(sc["P"], after, {v: p.dz for v, p in enumerate(plans)}, **dc.PIPELINE_OPTIONS)


PIVOT_CASES = ("slanted", "steep", "edge", "flat", "radius1", "step", "odd_sizes")
PIVOT_TEXTURED = ("slanted", "steep", "odd_sizes")


@lru_cache(maxsize=None)
def pivot_figures():
    """The figures of PIVOT, measured: the refinement of PIVOT_CASES with min_pivot 1e-12, so that nothing stops it."""
    pivots, before, after, textured, edge = [], [], [], [], None
    for name in PIVOT_CASES:
        c = scene(name)
        for k in CASES[name]["sweeps"]:
            sw, m = c.sweeps[k], swept(name)[k]
            r = drr.refine(c.images, c.P, sw.ref, sw.sources, m["depth"], m["status"], sw.dz, **dict(refine_options(name, k), min_pivot=1e-12))
            good = r["status"] == drr.REFINED
            exact = c.exact(sw.ref)[0]
            pivots.append(r["pivot_min"][good])
            before.append(np.abs(m["depth"] - exact)[good] / sw.dz)
            after.append(np.abs(r["depth"] - exact)[good] / sw.dz)
            if name in PIVOT_TEXTURED:
                textured.append(float(r["pivot_min"][good].min()))
            if name == "edge":
                sel = edge_only(c, sw.ref, refine_options(name, k)["radius"]) & tested(r) & (r["status"] != drr.OUTSIDE)
                edge = r["pivot_min"][sel]
    p, e0, e1 = np.concatenate(pivots), np.concatenate(before), np.concatenate(after)
    out = {"textured_min": min(textured), "edge_only_min": float(edge.min()), "edge_only_median": float(np.median(edge)), "edge_only_pixels": int(edge.size)}
    for label, lo, hi in (("below", 0.02, PIVOT["threshold"]), ("above", PIVOT["threshold"], 0.05)):
        s = (p >= lo) & (p < hi)
        out[label] = {"pixels": int(s.sum()), "p90_sweep": float(np.percentile(e0[s], 90)), "p90_refined": float(np.percentile(e1[s], 90))}
    return out
