"""Times osfm_match_all on the bench's headline set (50 views x 20 000 SIFT features, 1225 pairs) three ways:

  off      no geometric verification
  8-point  the reference's RANSAC-F (ransac_kernel)
  affine   the affine RANSAC for orthographic views (ransac_affine_kernel)

One matcher per mode in one process; the three alternate after a warm-up, at least 20 repetitions each; a time is a
host clock around the call (osfm_match_all returns after its last device synchronise).  Reported: median and spread
(5th to 95th percentile) per mode, and the verification cost of a mode, its median minus the median without
verification.  GPU only, no fallback.

    python tools/ransac_affine_timing.py [--reps 20] [--warmup 2] [--out profiles/ransac_affine_timing.txt]

The two kernels' own device times come from a kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ransac_affine_timing.py --trace-loop 5

which does nothing but 5 calls in each of the two verifying modes.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = sorted(v)
    return v[int(round(0.05 * (len(v) - 1)))], v[int(round(0.95 * (len(v) - 1)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--features", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--trace-loop", type=int, default=0, help="only this many calls in each verifying mode (for a kernel trace)")
    a = ap.parse_args()
    import numpy as np
    from orthosfm_amd import capi, synth
    from orthosfm_amd.matching import HipExhaustiveMatching

    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    V, F = a.views, a.features
    iset = synth.make_image_set(V, F, config_id=2)
    pairs = np.asarray([capi.pair_from_index(i) for i in range(V * (V - 1) // 2)], dtype=np.int32).reshape(-1, 2)
    capacity = F * pairs.shape[0]
    modes = {"off": (0, capi.RANSAC_FUNDAMENTAL), "8-point": (1, capi.RANSAC_FUNDAMENTAL), "affine": (1, capi.RANSAC_AFFINE)}
    if a.trace_loop:
        del modes["off"]
    matchers = {}
    for name, (verify, model) in modes.items():
        o = capi.default_match_options()
        o.geometric_verification, o.ransac_model = verify, model
        m = HipExhaustiveMatching(V, device=0, options=o, copy_results=False)
        for v in range(V):
            m.set_view(v, iset.sift[v])
            xy = (iset.pos[v] + 0.5 - np.array([iset.width / 2, iset.height / 2])) / max(iset.width, iset.height)
            m.set_positions(v, xy.astype(np.float32))
        m.use_result_buffer(capi.pinned_rows(capacity))
        matchers[name] = m

    def call(name):
        t0 = time.perf_counter()
        ra, _ = matchers[name].compute_arrays(pairs, capacity=capacity)
        dt = 1e3 * (time.perf_counter() - t0)
        ok = ra["status"] == capi.PAIR_MATCHED
        return dt, int(ok.sum()), int(ra["num_inliers"][ok].sum()) if name != "off" else int(ra["num_matches"][ok].sum())

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.trace_loop:
        for _ in range(a.trace_loop):
            for name in matchers:
                r = call(name)
        print(f"{a.trace_loop} calls per verifying mode on {pairs.shape[0]} pairs; last: {r[1]} pairs kept")
        return
    for _ in range(a.warmup):
        for name in matchers:
            call(name)
    times = {name: [] for name in matchers}
    kept = {}
    for _ in range(max(a.reps, 20)):
        for name in matchers:
            dt, n_pairs, n_corr = call(name)
            times[name].append(dt)
            kept[name] = (n_pairs, n_corr)
    say(f"osfm_match_all, {V} views x {F} SIFT features, {pairs.shape[0]} pairs, {len(times['off'])} alternating repetitions per mode "
        f"after {a.warmup} warm-up calls")
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        lo, hi = spread(t)
        what = "correspondences" if name == "off" else "inliers"
        say(f"  {name:8s} median {med[name]:8.2f} ms  (5-95 %: {lo:.2f} .. {hi:.2f});  {kept[name][0]} pairs kept, {kept[name][1]} {what}")
    noise = max(spread(t)[1] - spread(t)[0] for t in times.values())
    for name in ("8-point", "affine"):
        say(f"  verification cost {name:8s} {med[name] - med['off']:+8.2f} ms per call (median - median without verification)")
    say(f"  affine - 8-point = {med['affine'] - med['8-point']:+.2f} ms per call; largest 5-95 % spread of a mode {noise:.2f} ms")
    for m in matchers.values():
        m.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
