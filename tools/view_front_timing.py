"""Times a view's way from an image in host memory into the matcher, old path against new, per view:

  old   FeatureSetExtractor.extract + HipExhaustiveMatching.set_view_features (for image B after a halving on the
        host, the numpy restatement's -- what a caller of the old entries has to do himself)
  new   ViewFrontEnd.load + HipExhaustiveMatching.set_view_from_front

on image A, tests/sift_cases.timing_canvas() at 2048 x 2048, and image B, a 4096 x 4096 canvas of the same recipe,
which the default max_image_size of 6,000,000 halves once.  The two paths alternate in one process after a warm-up,
over enough views that the window of either exceeds a second; a time is a host clock around a device synchronise.
Reported: median and spread (5th to 95th percentile) per path, the front end's own halving_ms / view_ms, and the
hand-off call alone (its kernels and its one synchronise for two scalars: an upper bound of their device time)
beside the host path's set_view_features.  GPU only, no fallback.

    python tools/view_front_timing.py [--views 0] [--warmup 2] [--out profiles/view_front_timing.txt]

The device time of the hand-off kernels themselves comes from a kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/view_front_timing.py --trace-loop 10

which does nothing but 10 loads and hand-offs of image A; the halving kernels have no work there.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    v = sorted(v)
    return v[int(0.05 * (len(v) - 1))], v[int(round(0.95 * (len(v) - 1)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=0, help="views per path and image; 0: as many as make a window of 1.2 s")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--trace-loop", type=int, default=0, help="only this many loads and hand-offs of image A (for a kernel trace)")
    a = ap.parse_args()
    import numpy as np
    import sift_cases as sc
    import view_cases as vc
    from orthosfm_amd import capi
    from orthosfm_amd.features import FeatureSetExtractor, ViewFrontEnd
    from orthosfm_amd.matching import HipExhaustiveMatching

    def sync():
        assert capi._hip.hipDeviceSynchronize() == 0

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.trace_loop:
        img = sc.timing_canvas()
        m = HipExhaustiveMatching(1, device=0)
        with ViewFrontEnd(0, 2048, 2048, sift={"max_keypoints": 1 << 18}, surf={"max_keypoints": 1 << 18}) as front:
            for _ in range(a.trace_loop):
                s = front.load(img)
                m.set_view_from_front(0, front)
            sync()
        m.close()
        print(f"{a.trace_loop} loads and hand-offs of {s.num_sift} SIFT + {s.num_surf} SURF rows")
        return
    images = {"A 2048 x 2048": sc.timing_canvas(), "B 4096 x 4096": sc.timing_canvas(4096, blobs=360000, seed=78)}
    keypoints = {"max_keypoints": 1 << 18}
    verdicts = []
    for name, img in images.items():
        h, w = img.shape
        m = HipExhaustiveMatching(2, device=0)
        halves = w * h > 6_000_000
        fw, fh = ((w + 1) >> 1, (h + 1) >> 1) if halves else (w, h)
        with FeatureSetExtractor(0, fw, fh, sift=keypoints, surf=keypoints) as ex, \
                ViewFrontEnd(0, w, h, sift=keypoints, surf=keypoints) as front:
            def old():
                t0 = time.perf_counter()
                seen = vc.chain(img)[1] if halves else img
                t1 = time.perf_counter()
                fs = ex.extract(seen)
                t2 = time.perf_counter()
                m.set_view_features(0, fs)
                sync()
                t3 = time.perf_counter()
                return 1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t3 - t2), len(fs.sift), len(fs.surf)

            def new():
                t0 = time.perf_counter()
                s = front.load(img)
                t1 = time.perf_counter()
                m.set_view_from_front(1, front)
                sync()
                t2 = time.perf_counter()
                return 1e3 * (t2 - t0), s.halving_ms, 1e3 * (t2 - t1), s.num_sift, s.num_surf, s.view_ms

            for _ in range(a.warmup):
                o, n = old(), new()
            assert o[3:5] == n[3:5], (o, n)
            views = a.views or max(5, int(1200.0 / min(o[0], n[0])) + 1)
            olds, news = [], []
            for _ in range(views):
                olds.append(old())
                news.append(new())
            a_bank, b_bank = m.debug_view_bank(0), m.debug_view_bank(1)
            same = all(np.array_equal(a_bank[k], b_bank[k]) for k in a_bank)
        m.close()
        to, tn = [r[0] for r in olds], [r[0] for r in news]
        mo, mn = statistics.median(to), statistics.median(tn)
        so, sn = spread(to), spread(tn)
        say(f"image {name}: {n[3]} SIFT + {n[4]} SURF features, {views} views per path, windows {sum(to) / 1e3:.2f} s (old) "
            f"{sum(tn) / 1e3:.2f} s (new); banks equal: {same}")
        say(f"  old path  median {mo:8.2f} ms per view  (5-95 %: {so[0]:.2f} .. {so[1]:.2f}); of it host halving "
            f"{statistics.median(r[1] for r in olds):.2f} ms, set_view_features {statistics.median(r[2] for r in olds):.2f} ms")
        say(f"  new path  median {mn:8.2f} ms per view  (5-95 %: {sn[0]:.2f} .. {sn[1]:.2f}); of it halving_ms "
            f"{statistics.median(r[1] for r in news):.3f}, view_ms {statistics.median(r[5] for r in news):.3f}, "
            f"set_view_from_front {statistics.median(r[2] for r in news):.2f} ms (kernels and one synchronise)")
        gain, noise = mo - mn, max(so[1] - so[0], sn[1] - sn[0])
        verdict = "faster by more than the spread" if gain > noise else "NOT faster by more than the measured spread"
        verdicts.append(gain > noise)
        host_halve = statistics.median(r[1] for r in olds)
        if halves:
            say(f"  without the old path's halving on the host ({host_halve:.2f} ms in numpy): new - old = {mn - (mo - host_halve):+.2f} ms")
        say(f"  new - old = {-gain:+.2f} ms per view ({100.0 * gain / mo:.1f} % of the old path); spread {noise:.2f} ms: {verdict}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
