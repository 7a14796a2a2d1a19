#!/usr/bin/env python3
"""Time of the dense plane sweep and of the fusion (dense.DenseStereo) on one MI355X.

The scene: a smoothed-noise texture on the plane Z = 0, seen by eight affine cameras a few degrees apart, each image
rendered by bilinear lookup.  Measured, as medians with the 5th and 95th percentile over calls by device events:

  * one sweep of a size x size reference against 4 sources, 128 depths, radius 3, and the rate of warped samples
    (halo texels x depths x sources, what osfm_dense_stats.samples counts), each of which gathers 4 float32 texels;
  * the same sweep with one part of the kernel left out (osfm_dense_debug_ablation): what the time is made of;
  * the fusion of the eight views' maps, each swept as dense.plan_view plans it at no more than 128 depths;
  * the restatement's time per warped sample on the `slanted` case of tests/dense_cases.py, on this host's CPU.

    python tools/dense_timing.py --out profiles/dense_timing.txt
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
from refine_timing import percentiles, smoothed_noise      # noqa: E402

YAWS = [0.0, 6.0, -6.0, 3.0, -3.0, 8.0, -8.0, 5.0]
PITCHES = [0.0, 2.0, -2.0, -4.0, 4.0, 1.0, -1.0, 6.0]
# MI355X_MICROARCH "Indexed rows: gather into LDS": rows served from the XCD's L2, chip-wide
GUIDE_L2_GATHER_TBS = (16.8, 18.8)


def scene(size, seed=5):
    import dense_cases as dc
    import dense_restatement as dr
    base = smoothed_noise(size, seed).astype(np.float64)
    c = (size - 1) / 2.0
    P = np.stack([dc.camera(size, size, y, p, centre=(c, c, 0.0)) for y, p in zip(YAWS, PITCHES)])
    images = []
    ys, xs = np.mgrid[0:size, 0:size].astype(np.float64)
    for v in range(len(YAWS)):
        g = dr.Geometry(P[v])
        X0 = g.point(xs, ys, 0.0)
        z = -X0[2] / g.d[2]                                   # the plane Z = 0
        X, Y = X0[0] + z * g.d[0], X0[1] + z * g.d[1]
        x0, y0 = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
        fx, fy = X - x0, Y - y0
        a, b = x0 % size, y0 % size
        a1, b1 = (a + 1) % size, (b + 1) % size
        val = (1 - fy) * ((1 - fx) * base[b, a] + fx * base[b, a1]) + fy * ((1 - fx) * base[b1, a] + fx * base[b1, a1])
        images.append(np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8))
    return images, P


def plane_points(P, v, size, n=64):
    """n points of the plane Z = 0 that view v sees: its sparse points."""
    import dense_restatement as dr
    g = dr.Geometry(P[v])
    u = np.linspace(0.05, 0.95, 8) * (size - 1)
    xs, ys = np.meshgrid(u, u)
    X0 = g.point(xs.ravel(), ys.ravel(), 0.0)
    z = -X0[2] / g.d[2]
    return np.stack([X0[j] + z * g.d[j] for j in range(3)], axis=1)[:n]


def timed_sweeps(ds, ref, sources, z_min, dz, D, calls, warm, radius):
    dev, last = [], None
    for k in range(warm + calls):
        last = ds.sweep(ref, sources, z_min, dz, D, download=False, radius=radius)
        if k >= warm:
            dev.append(last.stats.device_ms)
    return percentiles(dev), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_timing.txt"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--depths", type=int, default=128)
    ap.add_argument("--radius", type=int, default=3)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("dense_timing: no HIP device: nothing is measured without one")
    images, P = scene(a.size)
    V = len(images)
    lines = [f"dense_timing: {a.calls} calls per entry behind {a.warm}; device ms per call (median, p5 - p95)"]
    with dense.DenseStereo(0, V) as ds:
        for v, im in enumerate(images):
            ds.set_image(v, im)
        ds.set_cameras(P)
        plan0 = dense.plan_view(P, 0, plane_points(P, 0, a.size), range(V), max_depths=a.depths)
        dz = plan0.dz
        z_min = -0.5 * (a.depths - 1) * dz
        d, m = timed_sweeps(ds, 0, plan0.sources, z_min, dz, a.depths, a.calls, a.warm, a.radius)
        samples = int(m.stats.samples)
        lines.append(f"sweep {a.size} x {a.size}, {len(plan0.sources)} sources {plan0.sources}, {a.depths} depths, radius {a.radius}:")
        lines.append(f"  device  {d[0]:9.3f} ms  ({d[1]:9.3f} - {d[2]:9.3f})")
        lines.append(f"  {m.stats.counters()}")
        rate = samples / d[0] / 1e6
        lines.append(f"  {samples} warped samples: {rate:.1f} G samples/s; 16 bytes of texels each: {rate * 16 / 1e3:.2f} TB/s gathered, "
                     f"beside the {GUIDE_L2_GATHER_TBS[0]}-{GUIDE_L2_GATHER_TBS[1]} TB/s of L2-served row gathers")
        pixel_depths = a.size * a.size * a.depths * len(plan0.sources)
        lines.append(f"  {d[0] * 1e6 / pixel_depths * 1e3:.2f} ps per (pixel, depth, source); {samples / pixel_depths:.2f} samples per (pixel, depth, source): the halo")
        full = d[0]
        names = {1: "no texel gather", 2: "float32 positions", 3: "one tap per box sum"}
        saved = {}
        for mode in (1, 2, 3):
            capi.lib.osfm_dense_debug_ablation(mode)
            try:
                t, _ = timed_sweeps(ds, 0, plan0.sources, z_min, dz, a.depths, max(a.calls // 2, 3), 1, a.radius)
            finally:
                capi.lib.osfm_dense_debug_ablation(0)
            saved[mode] = full - t[0]
            lines.append(f"  left out, {names[mode]:22s} {t[0]:9.3f} ms  ({t[1]:9.3f} - {t[2]:9.3f})   {100.0 * (full - t[0]) / full:5.1f} % less")
        top = max(saved, key=saved.get)
        lines.append(f"  the largest share: {names[top]}")
        # the fusion of all views, each swept as plan_view plans it
        sweep_ms = 0.0
        for v in range(V):
            p = dense.plan_view(P, v, plane_points(P, v, a.size), range(V), max_depths=a.depths)
            sweep_ms += ds.sweep(v, p.sources, p.z_min, p.dz, p.num_depths, download=False, radius=a.radius).stats.device_ms
        dev = []
        for k in range(a.warm + a.calls):
            cloud_stats, n = capi.DenseStats(), C.c_int64()
            capi.check(capi.lib.osfm_dense_fuse(ds._h, None, C.byref(n), C.byref(cloud_stats)))
            if k >= a.warm:
                dev.append(cloud_stats.device_ms)
        f = percentiles(dev)
        lines.append(f"fusion of {V} views of {a.size} x {a.size} (their sweeps: {sweep_ms:.1f} ms of device time in all):")
        lines.append(f"  device  {f[0]:9.3f} ms  ({f[1]:9.3f} - {f[2]:9.3f})   {int(n.value)} points")
        lines.append(f"  {cloud_stats.counters()}")
    import dense_cases as dc
    import dense_restatement as dr
    c = dc.case("slanted")
    sw = c.sweeps[0]
    t0 = time.perf_counter()
    dr.sweep(c.images, c.P, sw.ref, sw.sources, sw.z_min, sw.dz, sw.num_depths, **dc.sweep_options(c, sw))
    cpu = time.perf_counter() - t0
    n_cpu = c.images[0].size * sw.num_depths * len(sw.sources)
    lines.append(f"restatement (numpy, this host's CPU) on `slanted`: {cpu * 1e3:.1f} ms for {n_cpu} (pixel, depth, source): "
                 f"{cpu / n_cpu * 1e9:.1f} ns each, {cpu / n_cpu / (full * 1e-3 / pixel_depths):.0f} times the device's")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as fo:
        fo.write(text)


if __name__ == "__main__":
    main()
