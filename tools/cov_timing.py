#!/usr/bin/env python3
"""What a covariance call (ba.covariance: osfm_ba_covariance) costs, on three shapes, in one process behind a warm-up:
the whole call (host clock around it; the call ends synchronised) and the device time per kernel family from the
call's own HIP events -- linearisation (pair lists, point and pair pass), factorisation (with the pivot test),
inverse (Z = L^-1, S^-1 = Z^T Z, the cameras' blocks), point kernel --, medians with the 5th - 95th percentile.
Beside it, on the same problem in the same process: one LM iteration of osfm_ba_solve (lm_loop_ms / num_iterations)
and a numpy / scipy Schur-route build of the same outputs in float64 on this host's threads.

  * ring: BASELINE config 4's shape, 200 quaternion cameras, 100k tracks of 3..12 views
  * local: a 3-camera problem of 3000 tracks
  * dense: 60 cameras, every track in every camera (the gather form of the point kernel is quadratic in the track length)

    python tools/cov_timing.py --out profiles/cov_timing.txt

Nothing is promised about these times: this is the first measurement of them."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(v):
    p5, med, p95 = np.percentile(np.asarray(v, dtype=np.float64), [5, 50, 95])
    return f"median {med:9.3f}  p5 {p5:9.3f}  p95 {p95:9.3f}"


def host_schur_build(fp, cov):
    """The Schur route to the same outputs by numpy / scipy in float64, timed: V_j^-1, S from per-camera-pair sums of the
    tracks' blocks (tracks grouped by length, sorted keys and reduceat), its Cholesky inverse, the points' blocks.  The
    library has no entry that hands out its Jacobian, and the route's cost depends on the layout only, so the 2 x 6 and
    2 x 3 blocks are random values in the problem's own layout (S made safely positive definite).  Returns seconds."""
    import scipy.linalg
    rng = np.random.default_rng(1)
    C, M, O = fp.cam_params.shape[0], fp.points.shape[0], fp.obs_camera.shape[0]
    ldim = cov.cam_ldim.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ldim)])
    nc = int(off[-1])
    cam, pt = fp.obs_camera.astype(np.int64), fp.obs_point.astype(np.int64)
    Jc = rng.standard_normal((O, 2, 6)) * (np.arange(6)[None, None, :] < ldim[cam][:, None, None])
    Jp = rng.standard_normal((O, 2, 3))
    start = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=M))])
    length = np.diff(start)
    lengths = np.unique(length[length > 0])
    t_begin = time.perf_counter()
    V = np.zeros((M, 3, 3))
    np.add.at(V, pt, np.einsum("krx,kry->kxy", Jp, Jp))
    V += np.eye(3)
    Vi = np.linalg.inv(V)
    Y = np.einsum("krx,kry->kxy", Jc, np.einsum("krx,kxy->kry", Jp, Vi[pt]))             # (O, 6, 3) = W_ja V_j^-1
    W = np.einsum("krx,kry->kxy", Jc, Jp)                                                # (O, 6, 3)
    blocks = np.zeros((C * C, 6, 6))
    np.add.at(blocks, cam * C + cam, np.einsum("krx,kry->kxy", Jc, Jc))
    for ln in lengths:
        tr = np.nonzero(length == ln)[0]
        step = max(1, (1 << 18) // int(ln * ln))
        for b0 in range(0, tr.size, step):
            K = start[tr[b0:b0 + step]][:, None] + np.arange(ln)[None, :]
            blk = np.einsum("blxc,bmyc->blmxy", Y[K], W[K]).reshape(-1, 6, 6)
            keys = (cam[K][:, :, None] * C + cam[K][:, None, :]).reshape(-1)
            order = np.argsort(keys, kind="stable")
            ks = keys[order]
            first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
            blocks[ks[first]] -= np.add.reduceat(blk[order], first, axis=0)
    S = np.zeros((nc, nc))
    for key in np.flatnonzero(np.abs(blocks).sum(axis=(1, 2)) > 0):
        a, b = divmod(int(key), C)
        S[off[a]:off[a + 1], off[b]:off[b + 1]] = blocks[key, :ldim[a], :ldim[b]]
    S = 0.5 * (S + S.T) + np.eye(nc) * (np.abs(S).sum(1).max() + 1.0)
    Sinv = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S, lower=True), np.eye(nc))
    P = Vi.copy()
    cols = np.minimum(off[:-1][cam][:, None] + np.arange(6)[None, :], max(nc - 1, 0))    # (columns past ldim meet zeros of Y)
    for ln in lengths:
        tr = np.nonzero(length == ln)[0]
        step = max(1, (1 << 16) // int(ln * ln))
        for b0 in range(0, tr.size, step):
            tt = tr[b0:b0 + step]
            K = start[tt][:, None] + np.arange(ln)[None, :]
            ck = cols[K]
            Sb = Sinv[ck[:, :, None, :, None], ck[:, None, :, None, :]]
            P[tt] += np.einsum("blxc,blmxy,bmyd->bcd", Y[K], Sb, Y[K])
    return time.perf_counter() - t_begin


def measure(name, sc, calls, warm, lines, host_calls):
    from orthosfm_amd import ba
    fp = ba.FlatProblem.from_scene(sc)
    rec = []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        cov = ba.covariance(fp)
        wall = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            rec.append((wall, cov.timings_ms["total"], cov.timings_ms["linearize"], cov.timings_ms["factor"], cov.timings_ms["inverse"],
                        cov.timings_ms["point"]))
    rec = np.array(rec)
    lm = []
    for i in range(3 + 5):
        s = ba.solve(ba.FlatProblem.from_scene(sc), max_num_iterations=25)
        if i >= 3:
            lm.append(s.lm_loop_ms / max(s.num_iterations, 1))
    host = [host_schur_build(fp, cov) * 1e3 for _ in range(host_calls)]
    O, M, C = fp.obs_camera.shape[0], fp.points.shape[0], fp.cam_params.shape[0]
    lines += [f"## {name}: {C} cameras, {M} tracks, {O} observations, nc {cov.num_camera_unknowns}, "
              f"{cov.num_valid_points} valid points, dense Schur product {cov.dense_schur}, smallest pivot {cov.min_pivot_seen:.3g}",
              f"  whole call (python clock)   ms  {pct(rec[:, 0])}   ({calls} calls behind {warm})",
              f"  whole call (library clock)  ms  {pct(rec[:, 1])}",
              f"  linearisation (device)      ms  {pct(rec[:, 2])}",
              f"  factorisation (device)      ms  {pct(rec[:, 3])}",
              f"  inverse (device)            ms  {pct(rec[:, 4])}",
              f"  point kernel (device)       ms  {pct(rec[:, 5])}",
              f"  one LM iteration of osfm_ba_solve  ms  {pct(lm)}   (lm_loop_ms / num_iterations, 5 solves behind 3)",
              f"  numpy / scipy Schur route, float64, {os.environ.get('OMP_NUM_THREADS', '?')} threads  ms  {pct(host)}   ({host_calls} builds)",
              f"  ratios of medians: call / LM iteration {np.median(rec[:, 1]) / np.median(lm):.2f}, host build / call "
              f"{np.median(host) / np.median(rec[:, 1]):.1f}, point kernel / everything else on the device "
              f"{np.median(rec[:, 5]) / max(np.median(rec[:, 2] + rec[:, 3] + rec[:, 4]), 1e-9):.2f}", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--dense-tracks", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_timing.txt"))
    a = ap.parse_args()
    from orthosfm_amd import capi, synth
    if capi.device_count() < 1:
        raise SystemExit("cov_timing: no HIP device (a timing without one says nothing)")
    lines = [f"# tools/cov_timing.py --calls {a.calls} --warm {a.warm} --host-calls {a.host_calls} --dense-tracks {a.dense_tracks}",
             "# ba.covariance with the default options (gauge held, points optimised), cam_cov_full not asked for", ""]
    shapes = [("ring", lambda: synth.make_ba_scene(synth.MODEL_QUATERNION, 200, 100000, config_id=4)),
              ("local", lambda: synth.make_ba_scene(synth.MODEL_QUATERNION, 3, 3000, config_id=1, min_len=3, max_len=3)),
              ("dense", lambda: synth.make_ba_scene(synth.MODEL_QUATERNION, 60, a.dense_tracks, config_id=5, min_len=60, max_len=60))]
    for name, build in shapes:
        measure(name, build(), a.calls, a.warm, lines, a.host_calls)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines[-11:]), flush=True)


if __name__ == "__main__":
    main()
