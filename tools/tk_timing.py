#!/usr/bin/env python3
"""Times the Tomasi-Kanade initial alignment (osfm_tk_align) and what it costs inside a reconstruction.

    python tools/tk_timing.py [--views 200] [--features 20000] > profiles/tk_timing.txt

Part 1: osfm_tk_align at C = 3 for N = 2000 and N = 20000 tracks (0.5 px noise, 30 % outliers, the defaults: 241
hypotheses): HIP-event time of the scoring kernel and wall time of the call, medians of 20 calls after a warm-up.
Part 2: the pose estimation of a `--views`-view reconstruct() with initial_alignment="tk" next to "perturbed"."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orthosfm_amd import pipeline as P
from orthosfm_amd import synth, tk


def group_tracks(C, N, seed, noise=0.5, outliers=0.3, W=2048, H=2048, cid=43):
    st = cid << 32
    gt = synth.make_ba_scene(0, C, 10, seed=seed, config_id=cid, min_len=C, max_len=C, noise_px=0.0, width=W, height=H).gt_cams
    d = synth.normal(seed, st | 0x61, 3 * N).reshape(N, 3)
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * (0.5 * np.cbrt(synth.uniform(seed, st | 0x62, N)))[:, None]
    xy = np.stack([synth.project_quat(pts, gt[k, :4], gt[k, 4], gt[k, 5], gt[k, 6], W, H) for k in range(C)], axis=1)
    xy += noise * synth.normal(seed, st | 0x63, 2 * N * C).reshape(N, C, 2)
    u = synth.uniform(seed, st | 0x64, 3 * N).reshape(N, 3)
    for t in range(0, int(outliers * N)):
        xy[t, int(u[t, 0] * C)] = (u[t, 1] * W, u[t, 2] * H)
    perm = np.argsort(synth.uniform(seed, st | 0x65, N), kind="stable")
    return np.ascontiguousarray(xy[perm].astype(np.float32).astype(np.float64))


def time_calls():
    for N in (2000, 20000):
        xy = group_tracks(3, N, seed=N)
        tk.align(xy, 2048, 2048, seed=1)
        wall, kern = [], []
        for _ in range(20):
            t0 = time.perf_counter()
            a = tk.align(xy, 2048, 2048, seed=1)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(a.score_kernel_ms)
        print(f"osfm_tk_align C=3 N={N}: {a.iterations} hypotheses ({a.usable_models} usable, {a.supported_models} supported), "
              f"{a.num_inliers} inliers, mean error {a.mean_error_px:.3f} px; scoring kernel {np.median(kern):.4f} ms "
              f"(min {min(kern):.4f}), call {np.median(wall):.3f} ms wall (min {min(wall):.3f}), "
              f"{a.iterations * N * 3 / (1e6 * np.median(kern)):.2f} G track-camera scores/s in the kernel", flush=True)


def worst_rotation(iset, res, model):
    """Worst camera against the ground truth in the frame of the first aligned camera; orthographic views leave the
    mirror image of the scene (every rotation R -> T R T, T = diag(1, 1, -1)) equally valid, so both are measured."""
    gt, _ = P.canonical_ground_truth(iset, model)
    first = P._cam_rotation(model, gt[res.aligned_views[0]])
    T = np.diag([1.0, 1.0, -1.0])
    worst = [0.0, 0.0]
    for v in res.aligned_views:
        G, R = first.T @ P._cam_rotation(model, gt[v]), P._cam_rotation(model, res.cam_params[v])
        for k, truth in enumerate((G, T @ G @ T)):
            worst[k] = max(worst[k], float(np.degrees(np.arccos(np.clip((np.trace(truth.T @ R) - 1) / 2, -1, 1)))))
    return worst


def time_reconstruct(views, features):
    iset = synth.make_image_set(views, features, config_id=3)
    for mode in ("perturbed", "tk", "perturbed", "tk"):          # (the first run of each warms the caches up)
        res = P.reconstruct(iset, solver=0, initial_alignment=mode)
        t = res.timings
        line = (f"reconstruct {views} views x {features} features, initial_alignment={mode}: total {t.total_s:.3f} s, pose estimation "
                f"{t.pose_s:.3f} s ({100 * t.pose_s / t.total_s:.1f} % of the job), of it initial alignment {t.initial_alignment_s:.3f} s, "
                f"local BA {t.local_ba_s:.3f} s, global BA {t.global_ba_s:.3f} s; {len(res.aligned_views)} cameras, "
                "worst rotation error {:.2e} deg (against the mirror image of the scene {:.2e} deg)".format(*worst_rotation(iset, res, 0)))
        if res.initial_alignments:
            al = res.initial_alignments
            line += (f"; per group: {1e3 * t.initial_alignment_s / len(al):.3f} ms, tracks min/median/max "
                     f"{min(a.num_tracks for a in al)}/{int(np.median([a.num_tracks for a in al]))}/{max(a.num_tracks for a in al)}, "
                     f"status counts {np.bincount([a.status for a in al], minlength=4).tolist()} (ransac, fallback, too few, degenerate)")
        print(line, flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--features", type=int, default=20000)
    a = ap.parse_args()
    time_calls()
    time_reconstruct(a.views, a.features)
