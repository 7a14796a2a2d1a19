"""Times what the view marks cost and what OSFM_MARK_FEATURES saves:

  per view   ViewFrontEnd.load against ViewFrontEnd.load_marked in tracks mode (a mask of the image's size, the
             reference's clamp) on tests/sift_cases.timing_canvas() at 2048 x 2048.  load() runs the code it ran
             before the marks were added, so it stands for the parent commit's load in the same process.
  per job    a seeded set of windows of that canvas with a centred rectangular mask that keeps about a third of the
             rows: the matching (one osfm_match_all batch over all pairs, no geometric verification) of the bank
             loaded in features mode against the bank loaded in tracks mode, same pairs.

The two sides alternate in one process after a warm-up; a time is a host clock around a device synchronise.
Reported: median and spread (5th to 95th percentile) per side and their difference; for the job also the ratio of the
descriptor products summed over the pairs, which is what the tile kernel's work scales with.  GPU only, no fallback.

    python tools/view_marks_timing.py [--views 0] [--job-views 8] [--job-reps 15] [--out profiles/view_marks_timing.txt]
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
    ap.add_argument("--views", type=int, default=0, help="loads per side; 0: as many as make a window of 1.2 s")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--job-views", type=int, default=8)
    ap.add_argument("--job-window", type=int, default=1024)
    ap.add_argument("--job-reps", type=int, default=15)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import sift_cases as sc
    from orthosfm_amd import capi, synth
    from orthosfm_amd.features import ViewFrontEnd
    from orthosfm_amd.matching import HipExhaustiveMatching

    def sync():
        assert capi._hip.hipDeviceSynchronize() == 0

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def centred(rows, cols, share):
        m = np.zeros((rows, cols), np.uint8)
        f = share ** 0.5
        m[int(rows * (1 - f) / 2):int(rows * (1 + f) / 2), int(cols * (1 - f) / 2):int(cols * (1 + f) / 2)] = 255
        return m

    canvas = sc.timing_canvas()
    keypoints = {"max_keypoints": 1 << 18}

    # ---- per view ---------------------------------------------------------------------------------------------
    h, w = canvas.shape
    mask = centred(h, w, 1.0 / 3.0)
    with ViewFrontEnd(0, w, h, sift=keypoints, surf=keypoints) as front:
        def plain():
            t0 = time.perf_counter()
            s = front.load(canvas)
            sync()
            return 1e3 * (time.perf_counter() - t0), s.view_ms, s.num_sift + s.num_surf

        def marked():
            t0 = time.perf_counter()
            s = front.load_marked(canvas, mask, "tracks", "reference")
            sync()
            return 1e3 * (time.perf_counter() - t0), s.view_ms, s.num_sift + s.num_surf

        def marked_without_a_mask():
            t0 = time.perf_counter()
            s = front.load_marked(canvas, None, "tracks", "reference")
            sync()
            return 1e3 * (time.perf_counter() - t0), s.view_ms, s.num_sift + s.num_surf

        for _ in range(a.warmup):
            p, k, q = plain(), marked(), marked_without_a_mask()
        assert p[2] == k[2] == q[2]
        views = a.views or max(5, int(1200.0 / min(p[0], k[0])) + 1)
        ps, ks, qs = [], [], []
        for _ in range(views):
            ps.append(plain())
            ks.append(marked())
            ms = front.mark_summary
            qs.append(marked_without_a_mask())
    tp, tk = [r[0] for r in ps], [r[0] for r in ks]
    mp, mk = statistics.median(tp), statistics.median(tk)
    sp, sk = spread(tp), spread(tk)
    say(f"per view, 2048 x 2048, {p[2]} rows, {views} loads per side ({ms.masked_out_sift + ms.masked_out_surf} rows masked out, "
        f"{ms.outside} outside the mask)")
    say(f"  load                  median {mp:8.3f} ms  (5-95 %: {sp[0]:.3f} .. {sp[1]:.3f}); view_ms {statistics.median(r[1] for r in ps):.4f}")
    say(f"  load_marked (tracks)  median {mk:8.3f} ms  (5-95 %: {sk[0]:.3f} .. {sk[1]:.3f}); view_ms {statistics.median(r[1] for r in ks):.4f} "
        "(the colour kernel, the marks kernel and the mask's upload queue)")
    tq = [r[0] for r in qs]
    mq, sq = statistics.median(tq), spread(tq)
    say(f"  load_marked, no mask  median {mq:8.3f} ms  (5-95 %: {sq[0]:.3f} .. {sq[1]:.3f}); view_ms {statistics.median(r[1] for r in qs):.4f}: "
        f"the upload of the {mask.nbytes >> 20} MiB mask from pageable memory costs {mk - mq:+.3f} ms")
    inside = sp[0] <= mk <= sp[1]
    say(f"  load_marked - load = {mk - mp:+.3f} ms per view ({100.0 * (mk - mp) / mp:+.2f} %): "
        f"{'inside' if inside else 'OUTSIDE'} the plain load's own 5-95 % band; view_ms differs by "
        f"{statistics.median(r[1] for r in ks) - statistics.median(r[1] for r in ps):+.4f} ms")

    # ---- per job ----------------------------------------------------------------------------------------------
    V, win = a.job_views, a.job_window
    u = synth.uniform(91, 0x7A11 << 16, 2 * V).reshape(V, 2)
    offs = [(2 * int(x * (w - win) / 2), 2 * int(y * (h - win) / 2)) for x, y in u]
    images = [np.ascontiguousarray(canvas[y:y + win, x:x + win]) for x, y in offs]
    jmask = centred(win, win, 1.0 / 3.0)
    o = capi.default_match_options()
    o.geometric_verification = 0
    banks = {mode: HipExhaustiveMatching(V, device=0, options=o) for mode in ("tracks", "features")}
    sizes = {}
    with ViewFrontEnd(0, win, win, sift=keypoints, surf=keypoints) as front:
        for mode, m in banks.items():
            sizes[mode] = []
            for v, img in enumerate(images):
                s = front.load_marked(img, jmask, mode, "image")
                m.set_view_from_front(v, front)
                sizes[mode].append((s.num_sift, s.num_surf))
    pairs = np.array([capi.pair_from_index(i) for i in range(V * (V - 1) // 2)], np.int32)

    def match(m):
        sync()
        t0 = time.perf_counter()
        ra, _ = m.compute_arrays(pairs)
        sync()
        return 1e3 * (time.perf_counter() - t0), int(ra["num_matches"].sum())

    for _ in range(a.warmup):
        match(banks["tracks"]), match(banks["features"])
    tt, tf = [], []
    for _ in range(a.job_reps):
        tt.append(match(banks["tracks"]))
        tf.append(match(banks["features"]))
    for m in banks.values():
        m.close()
    work = {mode: sum(sizes[mode][i][k] * sizes[mode][j][k] for i, j in pairs.tolist() for k in (0, 1)) for mode in sizes}
    rows = {mode: sum(a_ + b_ for a_, b_ in sizes[mode]) for mode in sizes}
    mt, mf = statistics.median(r[0] for r in tt), statistics.median(r[0] for r in tf)
    st, sf = spread([r[0] for r in tt]), spread([r[0] for r in tf])
    say(f"per job, {V} windows of {win} x {win}, {len(pairs)} pairs, {a.job_reps} batches per side; rows {rows['tracks']} (tracks) "
        f"{rows['features']} (features): {100.0 * rows['features'] / rows['tracks']:.1f} % kept")
    say(f"  matching, tracks mode    median {mt:8.2f} ms  (5-95 %: {st[0]:.2f} .. {st[1]:.2f}); {tt[0][1]} matches")
    say(f"  matching, features mode  median {mf:8.2f} ms  (5-95 %: {sf[0]:.2f} .. {sf[1]:.2f}); {tf[0][1]} matches")
    say(f"  features / tracks = {mf / mt:.3f} of the time; descriptor products summed over the pairs: {work['features'] / work['tracks']:.3f}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
