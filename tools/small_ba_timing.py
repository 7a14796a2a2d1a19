#!/usr/bin/env python3
"""The one-workgroup form of the bundle adjustment (osfm_ba_options::small_form = 2) against the general form (0) of
the same build, on the same problems, the two alternating call by call (other work shares the host: a difference is
only trusted against the spread of both).  Not bench.py: nothing is promised about this form's speed; this tool is
where its threshold (auto_max_observations of osfm_ba_small_limits) comes from.

  * the 3-camera shapes of tests/test_ba_small_gpu.py and the local adjustments captured from the end-to-end job
    (capture= of run_pose_estimation): median and 5th - 95th percentile of solve_ms, lm_loop_ms per iteration, the
    time outside the loop, at least 100 calls per form behind a warm-up;
  * a sweep over the observations of a 3-camera adjustment (every track in all three): the threshold is the largest
    O at which the one-workgroup form's 95th percentile lies below the general form's 5th, 0 if there is none;
  * the job's local_ba_s with local_solver either way.

    python tools/small_ba_timing.py --views 200 --features 20000 --out profiles/small_ba_timing.txt

CAMS PTS (as tools/small_ba_profile.sh and tools/local_ba_timeline.sh call it) or --latency: what this tool was before
it compared the two forms -- the latency of few-camera adjustments in the general form (wall time per call, time
inside the LM loop, time per LM iteration), one JSON line per case; --latency alone runs the former default cases."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(ba, make_problem, calls, warm, **opt):
    """calls solves per form behind warm ones, the forms alternating; per form: (solve_ms, lm_loop_ms, iterations)"""
    rec = {0: [], 2: []}
    for i in range(warm + calls):
        for form in (0, 2):
            s = ba.solve(make_problem(), small_form=form, **opt)
            if i >= warm:
                rec[form].append((s.solve_ms, s.lm_loop_ms, s.num_iterations))
    return {f: np.array(v) for f, v in rec.items()}


def row(name, sizes, rec):
    out = []
    for form in (0, 2):
        r = rec[form]
        p5, med, p95 = np.percentile(r[:, 0], [5, 50, 95])
        it = max(float(np.median(r[:, 2])), 1.0)
        out.append(f"{name:26s} {sizes:22s} form {form}: solve_ms median {med:8.3f}  p5 {p5:8.3f}  p95 {p95:8.3f} | "
                   f"lm_loop_ms/iteration {np.median(r[:, 1]) / it:7.4f} ({int(it)} it) | outside the loop {np.median(r[:, 0] - r[:, 1]):7.3f}")
    return out


def latency(cases):
    from orthosfm_amd import ba, synth
    for cams, pts in cases:
        sc = synth.make_ba_scene(synth.MODEL_QUATERNION, cams, pts, config_id=1)
        ba.solve(ba.FlatProblem.from_scene(sc), max_num_iterations=2)
        wall, loop, its = [], [], []
        for _ in range(5):
            fp = ba.FlatProblem.from_scene(sc)
            t0 = time.perf_counter()
            s = ba.solve(fp, max_num_iterations=50)
            wall.append((time.perf_counter() - t0) * 1e3)
            loop.append(s.lm_loop_ms)
            its.append(s.num_iterations)
        k = int(np.argmin(wall))
        print(json.dumps({"cameras": cams, "points": pts, "observations": int(fp.obs_camera.size), "iterations": int(its[k]),
                          "call_ms": round(wall[k], 3), "solve_ms": round(float(s.solve_ms), 3), "lm_loop_ms": round(loop[k], 3),
                          "us_per_iteration": round(1e3 * loop[k] / max(its[k], 1), 1),
                          "iterations_per_s": round(its[k] / (loop[k] * 1e-3))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", nargs="*", type=int, metavar="CAMS PTS", help="the general form's latency on this case only")
    ap.add_argument("--latency", action="store_true", help="the general form's latency only (default cases without CAMS PTS)")
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--features", type=int, default=20000)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--captures", type=int, default=6, help="local adjustments of the job to time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_ba_timing.txt"))
    a = ap.parse_args()
    if a.latency or a.case:
        if len(a.case) not in (0, 2):
            ap.error("CAMS PTS, or neither")
        latency((tuple(a.case),) if a.case else ((3, 300), (3, 3000), (3, 20000), (6, 3000), (12, 5000)))
        return
    if a.calls < 100:
        ap.error("at least 100 calls per form")
    from orthosfm_amd import ba, capi, pipeline as P, synth
    if capi.device_count() < 1:
        raise SystemExit("small_ba_timing: no HIP device (a timing without one says nothing)")
    max_cams, chunk, auto = ba.small_limits()
    lines = [f"# tools/small_ba_timing.py --views {a.views} --features {a.features} --calls {a.calls} --warm {a.warm}",
             f"# osfm_ba_small_limits: max_cameras {max_cams}, track_chunk {chunk}, auto_max_observations {auto} (as built)",
             "# form 0: the general form; form 2: the one-workgroup form; the two alternate call by call on the same problem",
             "# solve_ms: the whole call (upload, set-up, solve, download); lm_loop_ms: form 0 the host's clock around the",
             "# iterations, form 2 the device's clock from the end of the first linearisation to the end of the launch", ""]

    def flush():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    # ---- the 3-camera shapes ----
    lines.append("## 3-camera shapes")
    shapes = [("(0,3,2500,3,3) cfg 81", lambda: synth.make_ba_scene(0, 3, 2500, config_id=81, min_len=3, max_len=3)),
              ("(1,3,400,2,3) cfg 81", lambda: synth.make_ba_scene(1, 3, 400, config_id=81, min_len=2, max_len=3)),
              (f"chunk {chunk}, all in three", lambda: synth.make_ba_scene(0, 3, chunk, config_id=82, min_len=3, max_len=3)),
              ("2 chunks + 1", lambda: synth.make_ba_scene(0, 3, 2 * chunk + 1, config_id=82, min_len=3, max_len=3))]
    for name, build in shapes:
        sc = build()
        rec = alternate(ba, lambda: ba.FlatProblem.from_scene(sc), a.calls, a.warm)
        lines += row(name, f"M {sc.points.shape[0]} O {sc.obs_xy.shape[0]}", rec)
        flush()

    # ---- the sweep over O ----
    lines += ["", "## sweep: three cameras, every track in all three (O = 3 M)"]
    chosen = 0
    for M in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
        sc = synth.make_ba_scene(0, 3, M, config_id=82, min_len=3, max_len=3)
        rec = alternate(ba, lambda: ba.FlatProblem.from_scene(sc), a.calls, a.warm)
        lines += row("sweep", f"M {M} O {3 * M}", rec)
        wins = np.percentile(rec[2][:, 0], 95) < np.percentile(rec[0][:, 0], 5)
        lines.append(f"{'':26s} {'':22s} one-workgroup p95 below general p5: {'yes' if wins else 'no'}")
        if wins:
            chosen = 3 * M
        flush()
    lines += ["", f"auto_max_observations from this sweep: {chosen}  (the build has {auto})"]
    flush()

    # ---- the end-to-end job: its local adjustments captured, and local_ba_s either way ----
    if a.views > 0:
        lines += ["", f"## end-to-end job: {a.views} views, {a.features} features per view, solver 0"]
        iset = synth.make_image_set(a.views, a.features, config_id=3)
        tt, _ = P.match_and_build_tracks(iset, "exhaustive", 0, True, P.Timings())
        P.join_background()
        model = ba.MODEL_QUATERNION
        n_local = a.views - 2
        want = sorted({int(x) for x in np.linspace(0, max(n_local - 1, 0), a.captures)})
        # the call numbers of the local adjustments: a first run lists the calls
        tm = P.Timings()
        _, _, _, calls, _ = P.run_pose_estimation(copy.deepcopy(tt), iset, model, timings=tm)
        local_calls = [i for i, c in enumerate(calls) if c.kind == "local"]
        cap_ids = tuple(local_calls[k] for k in want if k < len(local_calls))
        _, _, _, _, captured = P.run_pose_estimation(copy.deepcopy(tt), iset, model, capture=cap_ids)
        for i in cap_ids:
            kind, fp, retri = captured[i]
            mk = lambda fp=fp: ba.FlatProblem(fp.model, fp.cam_params, fp.cam_const, fp.img_w, fp.img_h, fp.points, fp.obs_xy,
                                              fp.obs_camera, fp.obs_point)
            rec = alternate(ba, mk, a.calls, a.warm, retriangulate_points=retri)
            lines += row(f"job call {i} ({kind})", f"M {fp.points.shape[0]} O {fp.obs_xy.shape[0]}", rec)
            flush()
        obs = [c.observations for c in calls if c.kind == "local"]
        lines.append(f"local adjustments of the job: {len(obs)}, observations min {min(obs)} median {int(np.median(obs))} max {max(obs)}")
        for rnd in range(2):
            for solver in ("general", "small"):
                tm = P.Timings()
                t0 = time.perf_counter()
                P.run_pose_estimation(copy.deepcopy(tt), iset, model, timings=tm, local_solver=solver)
                lines.append(f"run {rnd} local_solver={solver:8s}: local_ba_s {tm.local_ba_s:8.4f}  pose estimation {time.perf_counter() - t0:8.3f} s")
                flush()
    else:
        lines += ["", "## end-to-end job: not measured (--views 0)"]
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
