"""Times the SURF extraction on the seeded 2048 x 2048 canvas of tools/sift_timing.py
(tests/sift_cases.timing_canvas): after a warm-up, the stage times of the summary (events on the context's stream)
and the whole call -- osfm_surf_extract plus osfm_surf_download -- as the median of several calls.  One JSON line.

    python tools/surf_extract_timing.py [--calls 7] [--warmup 2] [--out FILE]

The CPU figure to set beside it is the reference's Surf::set_image + Surf::process on the same canvas, one thread:
python tests/golden/make_surf_golden.py --time (needs the reference's sources).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out")
    a = ap.parse_args()
    import sift_cases as sc
    from orthosfm_amd.features import SurfExtractor
    canvas = sc.timing_canvas(a.size) if a.size == 2048 else sc.timing_canvas(a.size, blobs=int(90000 * (a.size / 2048.0) ** 2))
    stages = ("sat_ms", "response_ms", "extrema_ms", "localisation_ms", "orientation_ms", "descriptor_ms", "total_ms")
    with SurfExtractor(0, a.size, a.size, max_keypoints=1 << 18) as ex:
        for _ in range(a.warmup):
            ex.extract(canvas)
        whole, per_stage = [], {s: [] for s in stages}
        for _ in range(a.calls):
            t0 = time.perf_counter()
            f = ex.extract(canvas)
            whole.append(1e3 * (time.perf_counter() - t0))
            for s in stages:
                per_stage[s].append(getattr(ex.summary, s))
        res = {"image": [a.size, a.size], "calls": a.calls, "candidates": ex.summary.num_candidates,
               "keypoints": ex.summary.num_keypoints, "descriptors": len(f),
               "extract_and_download_ms_median": round(statistics.median(whole), 3),
               "extract_and_download_ms_min": round(min(whole), 3)}
        res.update({s + "_median": round(statistics.median(v), 3) for s, v in per_stage.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
