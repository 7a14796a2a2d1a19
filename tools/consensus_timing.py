#!/usr/bin/env python3
"""The per-track consensus filter (osfm_ba_consensus) beside the reference's reprojection filter
(osfm_filter_reprojection) on the same problems, the two alternating call by call (other work shares the host: a
difference is only trusted against the spread of both).  Not bench.py: nothing is promised about this filter's speed;
no time is fixed in advance, this records what is measured.

Shapes: 200 cameras x 100k tracks of 3..12 views (a global adjustment's problem), 60 cameras that all see 3000 tracks
(the wave-per-track path, 120 hypotheses per track), 3 cameras x 3000 tracks (a camera group); ground-truth cameras,
0.3 px noise, every 50th observation replaced by a random pixel.  Per shape and entry: median and 5th - 95th percentile of the call's wall time (upload and download included, as a per-call caller sees it),
and for the consensus filter the device time between its first and last kernel (osfm_consensus_stats.device_ms) with
its counters.

    python tools/consensus_timing.py --out profiles/consensus_timing.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("global 200 x 100k", dict(num_cameras=200, num_points=100000, min_len=3, max_len=12)),
          ("dense 60 x 3000", dict(num_cameras=60, num_points=3000, min_len=60, max_len=60)),
          ("group 3 x 3000", dict(num_cameras=3, num_points=3000, min_len=3, max_len=3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_timing.txt"))
    a = ap.parse_args()
    from orthosfm_amd import ba, capi, filters, synth
    lines = [f"consensus_timing: {a.calls} calls per entry behind {a.warm}, alternating; wall ms per call (median, p5 - p95)"]
    for name, kw in SHAPES:
        sc = synth.make_ba_scene(synth.MODEL_QUATERNION, config_id=4, noise_px=0.3, **kw)
        sc.cam_params = sc.gt_cams.copy()              # adjusted cameras: the filter's place is behind an adjustment
        planted = np.arange(sc.obs_xy.shape[0]) % 50 == 7
        sc.obs_xy[planted] = (synth.uniform(synth.BASE_SEED, 0xC06 << 32, 2 * int(planted.sum())).reshape(-1, 2) * 2048.0
                              ).astype(np.float32)
        fp = ba.FlatProblem.from_scene(sc)
        O, M = fp.obs_camera.shape[0], fp.points.shape[0]
        keep = np.zeros(max(O, 1), dtype=np.uint8)
        wall = {"consensus": [], "reference": []}
        dev, res = [], None
        for i in range(a.warm + a.calls):
            t0 = time.perf_counter()
            res = filters.consensus(fp)
            t1 = time.perf_counter()
            work = ba.FlatProblem.from_scene(sc)          # the reference's entry overwrites the points
            st = work.struct()
            t2 = time.perf_counter()
            capi.check(capi.lib.osfm_filter_reprojection(C.byref(st), 0, C.c_double(1.5), capi._ptr(keep, C.c_uint8), None, None))
            t3 = time.perf_counter()
            if i >= a.warm:
                wall["consensus"].append((t1 - t0) * 1e3)
                wall["reference"].append((t3 - t2) * 1e3)
                dev.append(res.stats.device_ms)
        lines.append(f"{name}: {fp.cam_params.shape[0]} cameras, {M} tracks, {O} observations")
        for k in ("consensus", "reference"):
            p5, med, p95 = np.percentile(wall[k], [5, 50, 95])
            lines.append(f"  {k:10s} wall {med:9.3f} ms  ({p5:9.3f} - {p95:9.3f})")
        p5, med, p95 = np.percentile(dev, [5, 50, 95])
        lines.append(f"  consensus  device {med:7.3f} ms  ({p5:9.3f} - {p95:9.3f})   {res.stats.counters()}")
        lines.append(f"  of {int(planted.sum())} planted observations the reference rule keeps {int(keep[:O][planted].sum())} and drops "
                     f"{int((~keep[:O].astype(bool) & ~planted).sum())} others; consensus keeps {int(res.keep[planted].sum())} and drops "
                     f"{int((~res.keep & ~planted).sum())} others")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
