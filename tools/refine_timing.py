#!/usr/bin/env python3
"""Time of the observation refinement (refine.Refiner, osfm_refine_tracks) on one MI355X.

Two entries: a job-sized one -- 50 views of 2048 x 2048 with 1M observations (250k tracks of four), every view an
integer shift of one smoothed-noise texture, detector-like errors of +-0.3 px planted on the positions -- and the
`base` case of tests/refine_cases.py.  Per entry: device time (the two kernels, by events) and wall time per call, as
medians with the 5th and 95th percentile, the statuses, and the rate at which the kernel gathered texels: every
evaluation of a window reads 4 float32 texels per sample, and an observation evaluates its template once, its target
once per Gauss-Newton step and twice at the end.

    python tools/refine_timing.py --out profiles/refine_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from orthosfm_amd import capi, synth            # noqa: E402
from orthosfm_amd.refine import Refiner         # noqa: E402

FRONT_END_MS_PER_VIEW = 7.3                    # what the view front end spends on a 2048 x 2048 view


def smoothed_noise(size, seed):
    """uint8 [size, size]: uniform noise box-filtered twice over 5 pixels (cyclically), stretched to the 8-bit range."""
    a = synth.uniform(seed, 0x7E1F0001, size * size).reshape(size, size)
    for _ in range(2):
        for axis in (0, 1):
            a = sum(np.roll(a, k, axis) for k in range(-2, 3)) / 5.0
    a = (a - a.mean()) / a.std()
    return np.clip(np.floor(128.0 + 40.0 * a + 0.5), 0, 255).astype(np.uint8)


def job(views, size, tracks, length, seed):
    base = smoothed_noise(size, seed)
    u = synth.uniform(seed, 0x7E1F0002, 2 * views).reshape(views, 2)
    shift = np.floor(u * 41.0).astype(np.int64) - 20            # view v shows the texture moved by shift[v]
    shift[0] = 0
    images = [np.ascontiguousarray(np.roll(base, (int(s[1]), int(s[0])), axis=(0, 1))) for s in shift]
    F = tracks * length
    r = synth.uniform(seed, 0x7E1F0003, 5 * F).reshape(F, 5)
    X = np.repeat(40.0 + r[::length, :2] * (size - 80.0), length, axis=0)
    view = np.floor(r[:, 2] * views).astype(np.int32)
    xy = X + shift[view] + (2.0 * r[:, 3:5] - 1.0) * 0.3
    offsets = np.arange(0, F + 1, length, dtype=np.int64)
    return images, offsets, view, xy


def percentiles(x):
    return float(np.median(x)), float(np.percentile(x, 5)), float(np.percentile(x, 95))


def measure(name, images, offsets, view, xy, calls, warm, lines, options=None):
    options = options or {}
    radius = options.get("radius", 7)
    n = (2 * radius + 1) ** 2
    with Refiner(0, len(images)) as r:
        t0 = time.perf_counter()
        for v, im in enumerate(images):
            r.set_image(v, im)
        upload_ms = (time.perf_counter() - t0) * 1e3
        wall, dev = [], []
        for k in range(warm + calls):
            t0 = time.perf_counter()
            res = r.refine(offsets, view, xy, **options)
            if k >= warm:
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(res.stats.device_ms)
    counts = res.stats.counters()
    tested = res.status >= capi.REFINE_REFINED
    evaluations = int((res.iterations[tested] + 3).sum())
    texel_bytes = evaluations * n * 4 * 4
    d, w = percentiles(dev), percentiles(wall)
    lines.append(f"{name}: {len(images)} views, {offsets.shape[0] - 1} tracks, {view.shape[0]} observations, radius {radius}")
    lines.append(f"  device  {d[0]:9.3f} ms  ({d[1]:9.3f} - {d[2]:9.3f})")
    lines.append(f"  wall    {w[0]:9.3f} ms  ({w[1]:9.3f} - {w[2]:9.3f})   images set once in {upload_ms:.1f} ms")
    lines.append(f"  {counts}")
    lines.append(f"  {evaluations} window evaluations of {n} samples: {texel_bytes / 1e9:.2f} GB of texels gathered, "
                 f"{texel_bytes / d[0] / 1e9:.3f} TB/s; {d[0] * 1e6 / max(int(tested.sum()), 1):.1f} ns per refined-or-rejected observation")
    return d[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_timing.txt"))
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tracks", type=int, default=250000)
    a = ap.parse_args()
    lines = [f"refine_timing: {a.calls} calls per entry behind {a.warm}; ms per call (median, p5 - p95)"]
    images, offsets, view, xy = job(a.views, a.size, a.tracks, 4, 7)
    d = measure(f"job {a.views} x {a.size}^2", images, offsets, view, xy, a.calls, a.warm, lines)
    lines.append(f"  per view {d / a.views:.3f} ms of device time, beside {FRONT_END_MS_PER_VIEW} ms the view front end spends on a view")
    import refine_cases as rc
    c = rc.case("base")
    measure("base case", c.images, c.offsets, c.view, c.xy, 4 * a.calls, a.warm, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
