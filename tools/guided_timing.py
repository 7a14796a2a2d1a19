#!/usr/bin/env python3
"""What guided matching (osfm_match_guided) costs beside the matching it extends, on the benchmark's image set: 50
views of 20000 SIFT features, all 1225 pairs, verify="affine".  One matcher, one process; the parent behaviour
(compute_arrays alone) and compute_arrays + guided_arrays alternate call by call, so that whatever else shares the
machine lands on both.  Median and 5th - 95th percentile of either, the guided share, and what guided matching added
per pair.  Not bench.py: nothing is promised about this step's speed; the figure to hold it against is the
affine-verified matching time of the same pairs, printed beside it.

    python tools/guided_timing.py --out profiles/guided_timing.txt
    python tools/guided_timing.py --twin-frac 0.35 --out profiles/guided_timing.txt --append      # a set with repeated structure
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--features", type=int, default=20000)
    ap.add_argument("--twin-frac", type=float, default=0.0, help="0: the benchmark's set; > 0: that share of the landmarks in twins")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    from orthosfm_amd import capi, synth
    from orthosfm_amd.matching import HipExhaustiveMatching

    V, F = args.views, args.features
    iset = synth.make_image_set(V, F, config_id=2, twin_frac=args.twin_frac)
    o = capi.default_match_options()
    o.geometric_verification, o.ransac_model = 1, capi.RANSAC_AFFINE
    m = HipExhaustiveMatching(V, options=o, copy_results=False)
    W, H = iset.width, iset.height
    for v in range(V):
        m.set_view(v, iset.sift[v])
        m.set_positions(v, ((iset.pos[v] + 0.5 - np.array([W / 2, H / 2])) / max(W, H)).astype(np.float32))
    pairs = np.asarray([capi.pair_from_index(i) for i in range(V * (V - 1) // 2)], dtype=np.int32)
    capacity = F * pairs.shape[0]
    m.use_result_buffer(capi.pinned_rows(capacity))
    plain, both, guided = [], [], []
    gres = None
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        ra, corr = m.compute_arrays(pairs, capacity=capacity)
        t1 = time.perf_counter()
        ra, corr = m.compute_arrays(pairs, capacity=capacity)
        t2 = time.perf_counter()
        m.guided_arrays(pairs, ra, corr)
        t3 = time.perf_counter()
        if i >= args.warmup:
            plain.append(t1 - t0); both.append(t3 - t1); guided.append(t3 - t2)
        gres = m.last_guided[1]
    mem = capi.library_memory().device_buffer_bytes
    m.close()

    def row(name, x):
        p5, med, p95 = np.percentile(np.asarray(x) * 1e3, [5, 50, 95])
        return f"  {name:46s} median {med:9.1f} ms   p5 {p5:9.1f}   p95 {p95:9.1f}"

    added = gres["num_added"]
    lines = [
        f"guided matching beside affine-verified matching: {V} views x {F} SIFT features, {pairs.shape[0]} pairs, twin_frac {args.twin_frac}, "
        f"{args.calls} calls of either behind {args.warmup} warm-up, alternating in one process",
        row("compute_arrays alone (the parent's behaviour)", plain),
        row("compute_arrays + guided_arrays", both),
        row("guided_arrays alone (host marshalling included)", guided),
        f"  guided share of the affine-verified matching: {np.median(guided) / np.median(plain):.3f}",
        f"  verified pairs {gres.shape[0]}, seeds {int(gres['num_seeds'].sum())}, added {int(added.sum())} "
        f"(per pair: median {np.median(added) if added.size else 0:.0f}, max {int(added.max()) if added.size else 0}), "
        f"status ok/too_few/degenerate {[int((gres['status'] == s).sum()) for s in (0, 1, 2)]}, "
        f"largest candidate count of a query {int(gres['max_candidates'].max()) if gres.size else 0}",
        f"  device buffers of the matcher at the end: {mem / 2 ** 30:.2f} GiB",
        "",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
