#!/usr/bin/env python3
"""Time of the depth-map mesh of one view (dense.DenseStereo.mesh) beside the sweep that made the map, on one MI355X.

The scene is that of tools/dense_timing.py.  The sweep of view 0 and its meshes alternate in one process -- sweep,
mesh with the defaults, mesh with the island labelling on, download -- so that all see the same clocks.  Reported as
medians with the 5th and 95th percentile over calls: the sweep and each mesh by device events, the mesh per stage
(osfm_dense_mesh_stats.stage_ms), the download by the host's clock.

    python tools/dense_mesh_timing.py --out profiles/dense_mesh_timing.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from orthosfm_amd import capi, dense            # noqa: E402
from dense_timing import plane_points, scene    # noqa: E402
from refine_timing import percentiles           # noqa: E402


def mesh_only(ds, view, **options):
    """osfm_dense_mesh_view without the download: (vertices, triangles, stats)."""
    o = capi.default_dense_mesh_options(**options)
    nv, nt, stats = C.c_int64(), C.c_int64(), capi.DenseMeshStats()
    capi.check(capi.lib.osfm_dense_mesh_view(ds._h, view, C.byref(o), C.byref(nv), C.byref(nt), C.byref(stats)))
    return int(nv.value), int(nt.value), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_mesh_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--depths", type=int, default=128)
    ap.add_argument("--min-island", type=int, default=100)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("dense_mesh_timing: no HIP device: nothing is measured without one")
    images, P = scene(a.size)
    V = len(images)
    modes = {"defaults": dict(), f"min_island {a.min_island}": dict(min_island=a.min_island)}
    sweep_ms, down_ms = [], []
    mesh_ms = {k: [] for k in modes}
    stage_ms = {k: [[] for _ in capi.MESH_STAGES] for k in modes}
    with dense.DenseStereo(0, V) as ds:
        for v, im in enumerate(images):
            ds.set_image(v, im)
        ds.set_cameras(P)
        plan = dense.plan_view(P, 0, plane_points(P, 0, a.size), range(V), max_depths=a.depths)
        z_min = -0.5 * (a.depths - 1) * plan.dz
        for k in range(a.warm + a.calls):
            sw = ds.sweep(0, plan.sources, z_min, plan.dz, a.depths, download=False)
            res = {name: mesh_only(ds, 0, **o) for name, o in modes.items()}
            t0 = time.perf_counter()
            m = ds.mesh(0)
            t_all = time.perf_counter() - t0
            if k < a.warm:
                continue
            sweep_ms.append(sw.stats.device_ms)
            for name, (_, _, st) in res.items():
                mesh_ms[name].append(st.device_ms)
                for i in range(len(capi.MESH_STAGES)):
                    stage_ms[name][i].append(st.stage_ms[i])
            down_ms.append(t_all * 1e3 - m.stats.device_ms)
    s = percentiles(sweep_ms)
    lines = [f"dense_mesh_timing: {a.calls} rounds behind {a.warm}, sweep and meshes alternating; ms per call (median, p5 - p95)",
             f"view 0 of {a.size} x {a.size}: {m.points.shape[0]} vertices, {m.triangles.shape[0]} triangles; {m.stats.counters()}",
             f"sweep, {len(plan.sources)} sources, {a.depths} depths, radius 3:",
             f"  device  {s[0]:9.3f} ms  ({s[1]:9.3f} - {s[2]:9.3f})"]
    worst = None
    for name in modes:
        t = percentiles(mesh_ms[name])
        lines.append(f"mesh, {name}: {res[name][0]} vertices, {res[name][1]} triangles")
        lines.append(f"  device  {t[0]:9.3f} ms  ({t[1]:9.3f} - {t[2]:9.3f})   {100.0 * t[0] / s[0]:5.1f} % of the sweep")
        for i, stage in enumerate(capi.MESH_STAGES):
            p = percentiles(stage_ms[name][i])
            lines.append(f"    {stage:12s} {p[0]:9.3f} ms  ({p[1]:9.3f} - {p[2]:9.3f})")
            if worst is None or p[0] > worst[0]:
                worst = (p[0], name, stage)
        lines.append(f"  {a.size * a.size / t[0] / 1e6:.2f} G pixels/s")
    d = percentiles(down_ms)
    n_bytes = m.points.shape[0] * (24 + 24 + 4 + 8 + 8 + 1) + m.triangles.shape[0] * 12
    lines.append(f"download of the default mesh (host clock, call minus its device time), {n_bytes / 1e6:.1f} MB into fresh pageable arrays:")
    lines.append(f"  host    {d[0]:9.3f} ms  ({d[1]:9.3f} - {d[2]:9.3f})")
    lines.append(f"the slowest stage: {worst[2]} ({worst[1]}), {worst[0]:.3f} ms")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
