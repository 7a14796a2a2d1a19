#!/usr/bin/env python3
"""Time of the slanted-plane refinement of one view (dense.DenseStereo.refine) beside the sweep that made the map, on
one MI355X.

The scene is that of tools/dense_timing.py.  The sweep of view 0 and the refinement of its map alternate in one
process -- sweep, refine, sweep, refine -- so that both see the same clocks and every refinement starts from a fresh
sweep.  Reported as medians with the 5th and 95th percentile over calls, both by device events; with them the
refinement's status counts, its Gauss-Newton steps and source evaluations per tested pixel and its sample rate.
Every step on the device runs under a time limit of its own (an alarm with the default action: a step that does not
come back ends the process).

    python tools/dense_refine_timing.py --out profiles/dense_refine_timing.txt
"""
import argparse
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from orthosfm_amd import capi, dense            # noqa: E402
from dense_timing import plane_points, scene    # noqa: E402
from refine_timing import percentiles           # noqa: E402


def limited(seconds, step, *args, **kw):
    """step(*args, **kw) under an alarm of `seconds`."""
    signal.alarm(seconds)
    try:
        return step(*args, **kw)
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_refine_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--depths", type=int, default=128)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--limit", type=int, default=30, help="seconds a single step on the device may take")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("dense_refine_timing: no HIP device: nothing is measured without one")
    images, P = scene(a.size)
    V = len(images)
    sweep_ms, refine_ms = [], []
    with dense.DenseStereo(0, V) as ds:
        for v, im in enumerate(images):
            limited(a.limit, ds.set_image, v, im)
        ds.set_cameras(P)
        plan = dense.plan_view(P, 0, plane_points(P, 0, a.size), range(V), max_depths=a.depths)
        z_min = -0.5 * (a.depths - 1) * plan.dz
        for k in range(a.warm + a.calls):
            sw = limited(a.limit, ds.sweep, 0, plan.sources, z_min, plan.dz, a.depths, download=False, radius=a.radius)
            rf = limited(a.limit, ds.refine, 0, plan.sources, download=False, radius=a.radius)
            if k >= a.warm:
                sweep_ms.append(sw.stats.device_ms)
                refine_ms.append(rf.stats.device_ms)
    s, r = percentiles(sweep_ms), percentiles(refine_ms)
    counts = rf.stats.counters()
    tested = a.size * a.size - counts["not_ok"]
    side = 2 * a.radius + 1
    passes = rf.stats.samples / (side * side)
    lines = [f"dense_refine_timing: {a.calls} rounds behind {a.warm}, sweep and refinement alternating; ms per call (median, p5 - p95)",
             f"view 0 of {a.size} x {a.size}, {len(plan.sources)} sources, radius {a.radius} ({side * side} samples a window)",
             f"sweep, {a.depths} depths:",
             f"  device  {s[0]:9.3f} ms  ({s[1]:9.3f} - {s[2]:9.3f})",
             "refinement of its map:",
             f"  device  {r[0]:9.3f} ms  ({r[1]:9.3f} - {r[2]:9.3f})   {100.0 * r[0] / s[0]:5.1f} % of the sweep",
             f"  statuses {counts}",
             f"  {tested} tested pixels: {rf.stats.iterations / max(tested, 1):.2f} Gauss-Newton steps and {passes / max(tested, 1):.2f} source "
             f"evaluations a pixel",
             f"  {rf.stats.samples / 1e9:.3f} G samples with their gradients, {rf.stats.samples / r[0] / 1e6:.1f} G samples/s; "
             f"{tested / r[0] / 1e3:.1f} M pixels/s"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
