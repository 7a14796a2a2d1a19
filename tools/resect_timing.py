#!/usr/bin/env python3
"""Times the resection of a view against triangulated points (osfm_resect_view, osfm_scene_resect_view).

    python tools/resect_timing.py [--views 200] [--features 20000] > profiles/resect_timing.txt

Part 1: N = 2000 and N = 20000 correspondences (0.3 px noise, points perturbed by 5e-4, 30 % of the positions shifted
by 30 .. 300 px, the defaults: 107 hypotheses), per call and from a scene of 6 views whose other five are aligned at
the ground truth: HIP-event time of the scoring kernel and wall time of the call (it ends in a synchronise), median
and 5th / 95th percentile of `--calls` calls after a warm-up of every shape, the two forms alternating.
Part 2 (--views 0 leaves it out): a `--views`-view reconstruct() with initial_alignment="tk": how many groups end in
the fallback, and the job with weak_group="resect" beside the default."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orthosfm_amd import pipeline as P
from orthosfm_amd import resect, synth
from orthosfm_amd.scene import Scene

VIEW, V = 4, 6


def build(N, seed):
    bs = synth.make_ba_scene(0, V, N, min_len=V, max_len=V, noise_px=0.3, config_id=300 + seed)
    order = np.lexsort((bs.obs_camera, bs.obs_point))
    feat_view = bs.obs_camera[order].astype(np.int32)
    feat_xy = bs.obs_xy[order].astype(np.float32)
    rng = np.random.default_rng(seed)
    mine = np.flatnonzero(feat_view == VIEW)
    k = int(0.3 * N)
    ang = rng.uniform(0.0, 2.0 * np.pi, k)
    feat_xy[mine[rng.permutation(N)[:k]]] += (rng.uniform(30.0, 300.0, k) * np.array([np.cos(ang), np.sin(ang)])).T.astype(np.float32)
    sc = Scene(0, np.full(V, 2048, np.int32), np.full(V, 2048, np.int32), np.arange(0, V * N + 1, V, dtype=np.int64), feat_view, feat_xy)
    others = [v for v in range(V) if v != VIEW]
    sc.align_views(others, bs.gt_cams[others], np.ones((V - 1, 7), np.uint8))
    sc.triangulate()
    _, _, hp, pt = sc.download()
    assert hp.all()
    X = np.ascontiguousarray(pt[:, :3] / pt[:, 3:4])
    xy = np.ascontiguousarray(feat_xy[mine].astype(np.float64))
    return sc, X, xy, P._cam_rotation(0, bs.gt_cams[VIEW])


def pct(x):
    return "%.4f ms (5th .. 95th percentile %.4f .. %.4f)" % (np.median(x), np.percentile(x, 5), np.percentile(x, 95))


def time_calls(calls):
    print("# osfm_tk_align beside these (profiles/tk_timing.txt, C = 3, 241 hypotheses): N = 2000 scoring kernel 0.0177 ms, call "
          "0.22 ms; N = 20000 scoring kernel 0.030 ms, call 0.29 - 0.31 ms")
    for N in (2000, 20000):
        sc, X, xy, truth = build(N, N)
        forms = {"per call": lambda: resect.resect(X, xy, 2048, 2048, seed=1), "from the scene": lambda: sc.resect_view(VIEW, seed=1)}
        for f in forms.values():
            for _ in range(20):
                f()
        wall = {k: [] for k in forms}
        kern = {k: [] for k in forms}
        for _ in range(calls):
            for k, f in forms.items():
                t0 = time.perf_counter()
                a = f()
                wall[k].append(1e3 * (time.perf_counter() - t0))
                kern[k].append(a.score_kernel_ms)
        c = (np.trace(truth.T @ a.rotation) - 1.0) / 2.0
        print(f"N={N}: {a.iterations} hypotheses ({a.usable_models} usable, {a.supported_models} supported), {a.num_inliers} inliers "
              f"of {a.num_points}, mean error {a.mean_error_px:.3f} px, rotation {np.degrees(np.arccos(min(c, 1.0))):.4f} deg from the truth")
        for k in forms:
            print(f"  osfm_{'resect_view' if k == 'per call' else 'scene_resect_view'} N={N} ({k}, {calls} calls): scoring kernel "
                  f"{pct(kern[k])}, call {pct(wall[k])}, {a.iterations * N / (1e6 * np.median(kern[k])):.2f} G point scores/s in the kernel",
                  flush=True)
        sc.close()


def worst_rotation(iset, res):
    """Worst camera against the ground truth in the frame of the first aligned camera, and against the mirror image of
    the scene (orthographic views leave both equally valid)."""
    gt, _ = P.canonical_ground_truth(iset, 0)
    first = P._cam_rotation(0, gt[res.aligned_views[0]])
    T = np.diag([1.0, 1.0, -1.0])
    worst = [0.0, 0.0]
    for v in res.aligned_views:
        G, R = first.T @ P._cam_rotation(0, gt[v]), P._cam_rotation(0, res.cam_params[v])
        for k, truth in enumerate((G, T @ G @ T)):
            worst[k] = max(worst[k], float(np.degrees(np.arccos(np.clip((np.trace(truth.T @ R) - 1) / 2, -1, 1)))))
    return worst


def time_reconstruct(views, features):
    iset = synth.make_image_set(views, features, config_id=3)
    for policy in ("raise", "resect", "raise", "resect"):          # (the first run of each warms the caches up)
        res = P.reconstruct(iset, solver=0, initial_alignment="tk", weak_group=policy)
        t = res.timings
        al = res.initial_alignments
        print(f"reconstruct {views} views x {features} features, initial_alignment=tk, weak_group={policy}: total {t.total_s:.3f} s, "
              f"pose estimation {t.pose_s:.3f} s, of it initial alignment {t.initial_alignment_s:.3f} s; {len(res.aligned_views)} cameras, "
              f"{len(al)} groups, status counts {np.bincount([a.status for a in al], minlength=4).tolist()} (ransac, fallback, too few, "
              f"degenerate), resected groups {res.resected_groups}, "
              "worst rotation error {:.2e} deg (against the mirror image of the scene {:.2e} deg)".format(*worst_rotation(iset, res)),
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--features", type=int, default=20000)
    ap.add_argument("--calls", type=int, default=1000)
    a = ap.parse_args()
    time_calls(a.calls)
    if a.views:
        time_reconstruct(a.views, a.features)
