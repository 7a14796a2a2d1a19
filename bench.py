#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X backend (driver contract).

One "step" = one pass of the hot path over one synthetic image set: exhaustive
pairwise matching (low-res gate, two-way SIFT match, cross-check, thresholds,
ordered correspondence lists -- SURVEY 8d's unit of work, i.e. up to, not including,
RANSAC-F) of ALL V(V-1)/2 pairs of a V-image set with ~20k SIFT features per image,
descriptors resident in HBM.

  N = 1   BASELINE.json configs[1]: 50 images (1225 pairs) on one GPU.
  N > 1   BASELINE.json configs[2]: 200 images (19,900 pairs) held FIXED and sharded
          across the ranks by work (strong scaling); `--weak` grows the set instead so
          that every rank keeps ~1225 pairs.

`value` = image pairs matched per second over all ranks.  Pairs are dealt to the ranks
up front (no data-path collective); the match lists reach rank 0 at the end of every
step, inside the timed region: on one node every rank's lists go straight into its slice
of a shared page-locked host segment and only the per-pair counts are all-gathered over
RCCL -- `--exchange rccl` gathers the lists themselves over xGMI instead, as a
multi-node run would.

A plain run does what the headline needs and nothing more: it sets up, warms up, times the
steps, writes --dump-outputs and prints the line (with the tile kernel's roofline, read from
the timed steps themselves).  With `--full`, reported beside it on rank 0 at N = 1 (each
with the CPU path timed on the host cores, the lists of the timed pass compared with the
CPU oracle's): the same pass through RANSAC-F, a variant whose gates reject pairs and
matches, the cascade-hashing mode, special SIFT rows and FEATURE_ALL, track building, the
per-pair latency of the drop-in interface, the global bundle adjustment of configs[3] with
its roofline, the 200-image matching run on one GPU, and the end-to-end job (match ->
tracks -> groups -> incremental bundle adjustment) on the 200-image set; at N > 1, the
CPU baseline, the pass through RANSAC-F, track building over the exchanged lists and the
bundle adjustment.  The --no-* options leave legs out of a --full run.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus 1 --steps 3 --warmup 1 --full

`--dump-outputs DIR` writes what the last timed step returned (records and match lists of
rank 0's pairs, see dump_outputs) so that two builds can be compared output for output: the
image set is seeded, the same arguments give the same inputs.
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def usable_cores():
    """Host cores this process may really use (affinity mask and cgroup CPU
    quota) -- the GPU boxes expose 256 hardware threads but grant a share."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, int(os.environ.get("OSFM_BENCH_MAX_CORES", "64"))))


# the CPU oracle is OpenMP code: size its team before libgomp is loaded
_OMP_SET_BY_CALLER = "OMP_NUM_THREADS" in os.environ
os.environ.setdefault("OMP_NUM_THREADS", str(usable_cores()))

I8_MFMA_PEAK_TOPS = 5000.0      # dense int8 MFMA, MI355X_MICROARCH.md (2x the 2.5 PF bf16 figure)
HBM_PEAK_GBS = 8000.0
METRIC = "image-pairs matched/sec + BA iterations/sec (N images, M tracks) at 1/2/4/8 GPU"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--views", type=int, default=0, help="0 = 50 at N=1 (configs[1]), 200 at N>1 (configs[2])")
    ap.add_argument("--features", type=int, default=20000)
    ap.add_argument("--weak", action="store_true", help="N>1: grow the image set so that every rank keeps ~1225 pairs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ba", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the extra passes with RANSAC-F")
    ap.add_argument("--no-e2e", action="store_true", help="skip the 200-image matching run and the end-to-end job")
    ap.add_argument("--single-process", action="store_true",
                    help="with --gpus N and WITHOUT torchrun: one process, N devices behind osfm_match_create_multi "
                         "(the form the reference's single C++ caller can use) instead of one rank per GPU")
    ap.add_argument("--config", type=int, default=0, help="1: BASELINE configs[0] (3 views of the Suzanne model, solver 0) as a plumbing run, "
                                                             "one JSON line of its own; 0 (default): the headline workload")
    ap.add_argument("--no-realistic", action="store_true", help="skip the passes with special SIFT rows (bytes > 127)")
    ap.add_argument("--e2e-views", type=int, default=200)
    ap.add_argument("--cpu-sample-pairs", type=int, default=0, help="0 = auto (about 15 s of CPU work)")
    ap.add_argument("--no-lowres-gate", action="store_true",
                    help="kernel experiments only: match every pair in full whatever the results are")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo for rehearsal)")
    ap.add_argument("--exchange", default="shm", choices=["shm", "rccl"],
                    help="how the match lists reach rank 0 for N > 1: shared host segment (one node) or RCCL gather")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0's pairs) as DIR/<name>.npy, at most 64 MB")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline (CPU baselines and the parity checks "
                         "against them, the passes with RANSAC-F, gates at work, cascade hashing, special SIFT rows "
                         "and FEATURE_ALL, track building, the drop-in latency, the bundle adjustments with their "
                         "roofline, the 200-image run and the end-to-end job; at N > 1 track building over the "
                         "exchanged lists) and allow --config 1; the --no-* options leave legs out of it")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.config == 1 and not args.full:
        ap.error("--config 1 is a measurement beside the headline: it needs --full")
    if args.dump_outputs and args.config == 1:
        ap.error("--dump-outputs belongs to the matching pass, not to the --config 1 plumbing run")
    if not args.full:
        # a plain run is the headline alone: set up, warm up, the timed steps, --dump-outputs and the line
        args.no_cpu_baseline = args.no_ba = args.no_verify = args.no_e2e = args.no_realistic = True
    return args


DUMP_BUDGET_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 20240901


def dump_outputs(dir_path, out, budget=DUMP_BUDGET_BYTES):
    """Writes the per-pair results of one pass (TwoViewMatching objects, in pair order) as .npy files:
      pair_records.npy  (n, 6) float64: view_1_id, view_2_id, status, lowres_matches, num_matches, num_inliers
      matches.npy       (rows, 2) float32: the lists of all matched pairs, concatenated in pair order
                        (feature indices, exact in float32 below 2^24)
    When the lists do not fit the budget, matches.npy holds a fixed seeded sample of their rows (in
    order) and matches_rows.npy (float64) the index of each sampled row in the concatenation.
    Returns {name: shape}."""
    os.makedirs(dir_path, exist_ok=True)
    rec = np.array([[tv.view_1_id, tv.view_2_id, tv.status, tv.lowres_matches, tv.num_matches, tv.num_inliers]
                    for tv in out], dtype=np.float64).reshape(-1, 6)
    lists = [np.asarray(tv.matches, dtype=np.int64).reshape(-1, 2) for tv in out]
    allm = np.concatenate(lists) if lists else np.zeros((0, 2), np.int64)
    if allm.size and (allm.min() < 0 or allm.max() >= 1 << 24):
        raise ValueError("dump_outputs: feature index outside the exact float32 range")
    files = {"pair_records": rec}
    room = budget - rec.nbytes - 3 * 128                      # 128 bytes of .npy header per file
    if allm.shape[0] * 8 <= room:
        files["matches"] = allm.astype(np.float32)
    else:
        k = max(room // 16, 0)                                # 8 bytes of float32 row + 8 bytes of float64 index
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(allm.shape[0], size=k, replace=False))
        files["matches"] = allm[rows].astype(np.float32)
        files["matches_rows"] = rows.astype(np.float64)
    for name, a in files.items():
        np.save(os.path.join(dir_path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in files.items()}


def launch_plan(argv, environ, gpus, single_process, config):
    """What `python bench.py <argv>` does about processes, decided from the arguments and the
    environment alone (no HIP, no torch): None = this process is the bench (N = 1, a rank that
    torchrun started, the one-process multi-device front, the plumbing run); otherwise the
    command of the CHILD that runs it -- one rank per GPU under `torch.distributed.run`, which
    is how the pair loop of bundler_matching.cc:74-136 is sharded -- so that a plain
    `python bench.py --gpus N` is the N-rank run and not N = 1 with a flag."""
    if gpus <= 1 or single_process or config == 1:
        return None
    if "WORLD_SIZE" in environ or "RANK" in environ:
        return None                     # already a rank
    port = environ.get("MASTER_PORT") or str(29500 + (os.getpid() % 2000))
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + list(argv)


def run_child(cmd):
    """Starts the rank launcher as a child (never exec: this process may not be replaced once a
    GPU runtime could be live), relays its output as it comes and returns its exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not _OMP_SET_BY_CALLER:
        env.pop("OMP_NUM_THREADS", None)     # each rank sizes its own team
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True, bufsize=1)
    for ln in proc.stdout:
        sys.stdout.write(ln)
        sys.stdout.flush()
    return proc.wait()


def normalised_positions(iset, v):
    """normalize_feature_positions (feature_set.cc:42-55)."""
    return ((iset.pos[v] + 0.5 - np.array([iset.width / 2, iset.height / 2])) / max(iset.width, iset.height)).astype(np.float32)


def exchanged_tracks(gathered, all_pairs, V, F, how):
    """Rank 0 after an N > 1 pass: track building over the lists of ALL ranks, read
    in place from the shared segment (shm) or from the gathered buffer (rccl)."""
    from orthosfm_amd import capi, tracks as T
    pairs = (capi.Pair * len(all_pairs))()
    for i, (a, b) in enumerate(all_pairs):
        pairs[i].view_1, pairs[i].view_2 = a, b
    sizes = np.full(V, F, dtype=np.int32)
    t0 = time.perf_counter()
    if how == "shm":
        counts, starts, corr = gathered
        res = T.compute_flat_ranges(sizes, None, pairs, starts, counts, corr)
    else:
        counts, offs, corr = gathered
        res = T.compute_flat(sizes, None, pairs, offs, np.ascontiguousarray(corr))
    ms = (time.perf_counter() - t0) * 1e3
    return {"how": "shared host segment, lists consumed in place" if how == "shm" else "RCCL gather to rank 0",
            "correspondences_all_ranks": int(np.sum(counts)), "tracks": int(res[4].num_tracks),
            "invalid_tracks": int(res[4].num_invalid_tracks), "track_building_ms": ms}


def cpu_baseline(iset, pairs, n_sample, gpu_lists):
    """Times the CPU oracle (bit-exact restatement of the reference matcher, OpenMP over
    queries) on a bounded sample of the same workload -- and checks what was timed: the
    oracle's cross-checked lists of every sampled full-size pair are compared with the
    lists the GPU pass produced for the same pairs."""
    import oracle_lib
    threads = oracle_lib.oracle().oracle_num_threads()
    empty = np.zeros((0, 64), np.int16)
    # calibrate on one quarter-size pair to pick the sample size
    a, b = pairs[0]
    t0 = time.perf_counter()
    oracle_lib.oracle_pairwise_match(iset.sift[a][:5000], empty, iset.sift[b][:5000], empty)
    t_quarter = time.perf_counter() - t0
    est_pair = t_quarter * 16.0
    if n_sample <= 0:
        n_sample = int(max(1, min(len(pairs), round(15.0 / max(est_pair, 1e-3)))))
    # spread the sample over the pair list (not only its first views)
    sample = sorted({int(i) for i in np.linspace(0, len(pairs) - 1, n_sample)})
    t0 = time.perf_counter()
    results = []
    for i in sample:
        a, b = pairs[i]
        results.append(oracle_lib.oracle_pairwise_match(iset.sift[a], empty, iset.sift[b], empty))
    dt = time.perf_counter() - t0
    checked, bad = 0, []
    for i, (e12, _) in zip(sample, results):
        if gpu_lists is None or gpu_lists[i] is None:
            continue
        idx = np.nonzero(e12 >= 0)[0]
        exp = np.stack([idx, e12[idx]], axis=1).astype(np.int32)
        checked += 1
        if not np.array_equal(np.asarray(gpu_lists[i]), exp):
            bad.append(i)
    n = iset.sift[0].shape[0]
    port = {"value": len(sample) / dt, "unit": "pairs/s", "cores": int(threads), "kind": "port",
            "sample": f"{len(sample)} full-size pairs ({n} x {n} SIFT, two-way + cross-check) spread over the same "
                      f"image set, {dt:.1f} s; OpenMP over the queries of a pair"}
    # The reference's own matcher (sfm::Matching::twoway_match + remove_inconsistent_matches, compiled from
    # /root/reference into oracle/_ref/libref_match.so) when it travelled: the way the reference runs it, one
    # pair per thread (bundler_matching.cc:86-88), on as many pairs as there are threads (at least 8).  The
    # lists it produces are compared with the GPU's as well.
    rm = oracle_lib.ref_matcher()
    if rm is None:
        return port, checked, bad
    from concurrent.futures import ThreadPoolExecutor
    n_thr = int(max(1, min(threads, 16)))
    n_ref = max(8, n_thr)
    ref_sample = sorted({int(i) for i in np.linspace(0, len(pairs) - 1, n_ref)})

    def one(i):
        a, b = pairs[i]
        e12, e21 = rm.twoway(iset.sift[a], iset.sift[b], 0.8)
        return rm.remove_inconsistent(e12, e21)[0]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=n_thr) as ex:
        ref_lists = list(ex.map(one, ref_sample))
    dt_ref = time.perf_counter() - t0
    for i, e12 in zip(ref_sample, ref_lists):
        if gpu_lists is None or gpu_lists[i] is None:
            continue
        idx = np.nonzero(e12 >= 0)[0]
        exp = np.stack([idx, e12[idx]], axis=1).astype(np.int32)
        checked += 1
        if not np.array_equal(np.asarray(gpu_lists[i]), exp):
            bad.append(i)
    base = {"value": len(ref_sample) / dt_ref, "unit": "pairs/s", "cores": n_thr, "kind": "reference",
            "sample": f"{len(ref_sample)} full-size pairs ({n} x {n} SIFT) through the reference's own twoway_match + "
                      f"remove_inconsistent_matches (oracle/_ref/libref_match.so), one pair per thread as "
                      f"bundler_matching.cc:86-88 runs them, {dt_ref:.1f} s",
            "port": port,
            # per core: what the bit-exact restatement (the oracle every parity test uses) costs against the reference
            "port_vs_reference": (port["value"] / port["cores"]) / (len(ref_sample) / dt_ref / n_thr)}
    return base, checked, bad


def newest_profile(pattern):
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def pmc_traffic_per_launch(pairs_per_launch):
    """HBM bytes of one launch of the dominant kernel from the committed PMC passes
    (profiles/r*_match_traffic_pmc.json: FETCH_SIZE and WRITE_SIZE collected in separate
    rocprofv3 --pmc runs of this same command, FETCH_SIZE doubled as the gfx950 guide
    prescribes), scaled to the pairs per launch."""
    path = newest_profile("r*_match_traffic_pmc.json")
    try:
        rec = json.load(open(path))
        return rec["hbm_bytes_per_pair"] * pairs_per_launch, os.path.basename(path)
    except Exception:
        return None, None


def ba_cpu_baseline(iterations=2):
    """The BA oracle (double-precision restatement of the reference's Ceres
    solve, parity unpinned) on the same config-4 scene, bounded to a few LM
    iterations."""
    import oracle_lib
    from orthosfm_amd import synth
    sc = synth.make_ba_scene(synth.MODEL_QUATERNION, 200, 100000, config_id=4)
    t0 = time.perf_counter()
    s = oracle_lib.oracle_ba_solve(sc, max_num_iterations=iterations)
    dt = time.perf_counter() - t0
    return {"value": s.num_iterations / dt, "unit": "LM iterations/s",
            "cores": int(oracle_lib.oracle().oracle_num_threads()), "kind": "port",
            "sample": f"{s.num_iterations} LM iterations of the same 200-camera / 100k-track problem, {dt:.1f} s "
                      "(residual/Jacobian evaluation and the dense Cholesky trailing updates OpenMP-parallel, Schur accumulation serial)"}


def local_ba_cpu_baseline(gpu):
    """The BA oracle on the same 3-camera problem, whole solve (it is small enough)."""
    import oracle_lib
    from orthosfm_amd import synth
    sc = synth.make_ba_scene(synth.MODEL_QUATERNION, 3, 3000, config_id=1)
    t0 = time.perf_counter()
    s = oracle_lib.oracle_ba_solve(sc, max_num_iterations=50)
    dt = time.perf_counter() - t0
    return {"value": 1e6 * dt / max(s.num_iterations, 1), "unit": "us per LM iteration",
            "call_ms": dt * 1e3, "iterations": int(s.num_iterations),
            "cores": int(oracle_lib.oracle().oracle_num_threads()), "kind": "port",
            "sample": "the whole solve of the same problem",
            "iterations_equal_gpu": bool(s.num_iterations == gpu["iterations"]),
            "final_cost_rel_diff": abs(s.final_cost - gpu["final_cost"]) / max(abs(s.final_cost), 1e-300)}


def ba_roofline(ba):
    """Q_B = 2*24*O + 96*M + 2*8*(dC)^2 algorithmic bytes per LM iteration
    (observations read for linearisation and trial cost, points read twice and written,
    dense reduced system written and read) against the HBM peak."""
    O, M, nc = ba["observations"], ba["points"], ba["camera_unknowns"]
    q = 2 * 24 * O + 96 * M + 2 * 8 * nc * nc
    its = ba["lm_loop_iterations_per_s"]
    ach = q * its / 1e9
    traffic, src = None, None
    path = newest_profile("r*_ba_traffic_pmc.json")
    try:
        traffic = json.load(open(path))["hbm_bytes_per_iteration"]
        src = os.path.basename(path)
    except Exception:
        pass
    return {"bound": "hbm (a latency chain in practice: see kernel_ms)", "algorithmic_bytes_per_iteration": q,
            "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": traffic,
            "traffic_source": src, "traffic_over_algorithmic": (traffic / q) if traffic else None,
            "iterations_per_s": its}


import contextlib


@contextlib.contextmanager
def stdout_to_stderr():
    """File descriptor 1 points at stderr inside the block (C++ code of the reference writes to std::cout):
    the bench's stdout carries the one JSON line and nothing else."""
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        os.dup2(saved, 1)
        os.close(saved)


def cascade_bench(iset, V, pairs, capacity, device_index, with_cpu):
    """The same pairs through the cascade-hashing mode (sfm::CascadeHashing, the
    application's default, approximate matcher).  CPU baseline: the reference's
    own cascade_hashing.cc when oracle/_ref travelled (its pairwise_match on a
    sample of pairs, all host threads via its OpenMP init, matching single
    threaded per pair as in one iteration of bundler::Matching::compute's loop)."""
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipCascadeHashing
    m = HipCascadeHashing(V, device=device_index, copy_results=False)
    for v in range(V):
        m.set_view(v, iset.sift[v])
    t0 = time.perf_counter()
    m.cascade_hashes(0, 0)
    init_s = time.perf_counter() - t0
    m.compute(pairs, capacity=capacity)
    t0 = time.perf_counter()
    out = m.compute(pairs, capacity=capacity)
    dt = time.perf_counter() - t0
    st = m.stats()
    res = {"workload": f"{len(pairs)} pairs, cascade hashing (6 bucket groups x 256 buckets, 6..10 candidates)",
           "pairs_per_s": len(pairs) / dt, "ms_per_step": dt * 1e3, "hash_init_ms": init_s * 1e3,
           "kernel_ms": st.cashash_kernel_ms,
           "correspondences": int(sum(tv.num_matches for tv in out if tv.status == capi.PAIR_MATCHED))}
    m.close()
    if with_cpu:
        import oracle_lib
        if oracle_lib.ref_cashash() is not None:
            nv = min(V, 6)
            empty = [np.zeros((0, 64), np.int16)] * nv
            t0 = time.perf_counter()
            with stdout_to_stderr():          # the reference's init prints its timing to std::cout
                ref = oracle_lib.RefCasHash(iset.sift[:nv], empty)
            t_init = time.perf_counter() - t0
            sample = [(a, b) for a in range(nv) for b in range(a)]
            t0 = time.perf_counter()
            for a, b in sample:
                ref.pairwise_match(a, b)
            dtc = time.perf_counter() - t0
            ref.close()
            res["cpu_baseline"] = {"value": len(sample) / dtc, "unit": "pairs/s", "cores": 1, "kind": "reference",
                                   "sample": f"{len(sample)} pairs of the first {nv} views, {dtc:.1f} s "
                                             f"(hash init of those views {t_init:.2f} s not included)"}
    return res


def tracks_bench(out, V, F, with_cpu):
    """Tracks::compute (bundler_tracks.cc:49-145) over the match lists this run
    produced: host code in the reference and here; the CPU baseline is the
    reference's own file when oracle/_ref travelled, the oracle port otherwise."""
    from orthosfm_amd import tracks as T
    matched = [tv for tv in out if tv.matches.shape[0] > 0]
    sizes = np.full(V, F, dtype=np.int32)
    pairs, offsets, corr = T.flatten_matching(matched)
    T.compute_flat(sizes, None, pairs, offsets, corr)
    t0 = time.perf_counter()
    ids, toff, tfeat, tcol, summary = T.compute_flat(sizes, None, pairs, offsets, corr)
    dt = time.perf_counter() - t0
    res = {"workload": f"Tracks::compute over {len(matched)} pairs / {int(offsets[-1])} matches (host code)",
           "ms": dt * 1e3, "tracks": int(summary.num_tracks), "invalid_tracks": int(summary.num_invalid_tracks),
           "track_features": int(summary.num_features), "matches": int(offsets[-1])}
    if with_cpu:
        import oracle_lib
        parr = np.array([(tv.view_1_id, tv.view_2_id) for tv in matched], dtype=np.int32).reshape(-1, 2)
        kind = "reference" if oracle_lib.ref_tracks() is not None else "port"
        fn = oracle_lib.ref_tracks_compute if kind == "reference" else oracle_lib.oracle_tracks
        t0 = time.perf_counter()
        ref = fn(sizes, None, parr, offsets, corr)
        dtc = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": dtc * 1e3, "unit": "ms", "cores": 1, "kind": kind,
                               "sample": "the same match lists, whole job",
                               "identical_output": bool(np.array_equal(ref["track_features"], tfeat)
                                                        and np.array_equal(ref["track_ids"], ids))}
    return res


def outlier_filter_bench(device, with_cpu):
    """filterOutlierTracks on the 100k points of the global-BA config: the
    O(P^2) nearest-neighbour search is the kernel, the rest is O(P) host work."""
    from orthosfm_amd import filters, synth
    sc = synth.make_ba_scene(synth.MODEL_QUATERNION, 200, 100000, config_id=4)
    has = np.ones(sc.points.shape[0], dtype=bool)
    filters.outlier_track_flags(sc.points, has, device)
    t0 = time.perf_counter()
    keep, st = filters.outlier_track_flags(sc.points, has, device)
    dt = time.perf_counter() - t0
    out = {"workload": "filterOutlierTracks, 100000 points (1e10 distance evaluations, f64)",
           "ms": dt * 1e3, "kept": int(keep.sum()), "mean_nn": st.mean, "sigma": st.sigma}
    if with_cpu:
        import oracle_lib
        n = 20000
        t0 = time.perf_counter()
        oracle_lib.oracle_nn_distances(sc.points[:n])
        dtc = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": dtc * 1e3 * (sc.points.shape[0] / n) ** 2, "unit": "ms (extrapolated to 100000 points)",
                               "cores": int(oracle_lib.oracle().oracle_num_threads()), "kind": "port",
                               "sample": f"nearest-neighbour search over the first {n} points, {dtc:.2f} s, scaled by (100000/{n})^2"}
    return out


def gated_bench(V, F, device_index):
    """The gates at work (the headline set matches every pair and every surviving match is
    an inlier): the same 50-view shape with repeated structure -- a third of the landmarks
    are twins with one descriptor at two 3-D positions, whose cross-view matches pass ratio
    test and cross-check and are geometrically wrong -- and four views of another scene,
    whose pairs with the rest fall at the low-res gate."""
    from orthosfm_amd import capi, synth
    from orthosfm_amd.matching import HipExhaustiveMatching
    iset = synth.make_image_set(V, F, config_id=2, twin_frac=0.35, unrelated_views=4)
    o = capi.default_match_options()
    o.geometric_verification = 1
    m = HipExhaustiveMatching(V, device=device_index, options=o, copy_results=False)
    for v in range(V):
        m.set_view(v, iset.sift[v])
        m.set_positions(v, normalised_positions(iset, v))
    pairs = [capi.pair_from_index(i) for i in range(V * (V - 1) // 2)]
    cap = F * len(pairs)
    m.compute(pairs, capacity=cap)
    t0 = time.perf_counter()
    out = m.compute(pairs, capacity=cap)
    dt = time.perf_counter() - t0
    st = np.array([tv.status for tv in out])
    matched = [tv for tv in out if tv.status == capi.PAIR_MATCHED]
    pre = int(sum(tv.num_matches for tv in matched))
    inl = int(sum(tv.num_inliers for tv in matched))
    # how many of the kept correspondences join features of the same landmark
    good = tot = 0
    for tv in matched[:200]:
        la = iset.landmark[tv.view_1_id][tv.matches[:, 0]]
        lb = iset.landmark[tv.view_2_id][tv.matches[:, 1]]
        good += int(((la == lb) & (la >= 0)).sum()); tot += tv.matches.shape[0]
    m.close()
    return {"workload": f"{V} views x {F} features, 35% twin landmarks, 4 views of another scene, RANSAC-F on",
            "pairs_per_s": len(pairs) / dt, "ms_per_step": dt * 1e3,
            "pairs": {"matched": int((st == capi.PAIR_MATCHED).sum()),
                      "rejected_lowres": int((st == capi.PAIR_REJECTED_LOWRES).sum()),
                      "rejected_count": int((st == capi.PAIR_REJECTED_COUNT).sum()),
                      "rejected_inliers": int((st == capi.PAIR_REJECTED_INLIERS).sum())},
            "mutual_matches_of_matched_pairs": pre, "ransac_inliers": inl,
            "outlier_share_removed_by_ransac": 1.0 - inl / max(pre, 1),
            "inliers_on_the_same_landmark": good / max(tot, 1)}


def realistic_operands_bench(iset, V, pairs, capacity, device_index, headline_ms, steps, with_cpu):
    """The headline workload with k descriptors per view holding a byte in 128-255, built as
    MVE builds them (few dominant bins, renormalised after the 0.2 clamp: sift.cc:830-839) --
    the rows a dense Gaussian generator never draws and real images do.  Same 50 x 20k set,
    same pairs, same gates; per k: pairs/s, device time of the tile kernel and of the kernel
    that scores the special descriptors, and a few pairs re-done by the CPU oracle."""
    import copy
    from orthosfm_amd import capi, synth
    from orthosfm_amd.matching import HipExhaustiveMatching
    out = {"what": "k SIFT descriptors per view with a byte > 127 (synth.add_peaky_rows); everything else as the headline",
           "headline_ms_per_step": headline_ms, "cases": []}
    for k in (1, 20, 200, 1000):
        sub = copy.copy(iset)
        sub.sift = [a.copy() for a in iset.sift]
        synth.add_peaky_rows(sub, k)
        m = HipExhaustiveMatching(V, device=device_index, copy_results=False)
        for v in range(V):
            m.set_view(v, sub.sift[v])
        m.use_result_buffer(capi.pinned_rows(capacity))
        for _ in range(2):          # a fresh matcher and a fresh page-locked buffer: two untimed passes
            m.compute_arrays(pairs, capacity=capacity)
        t0 = time.perf_counter()
        tile_ms = sp_ms = 0.0
        launches = 0
        steps = max(steps, 8)       # a ratio of two ~57 ms passes to 1 %: not from three steps
        for _ in range(steps):
            ra, corr = m.compute_arrays(pairs, capacity=capacity)
            st = m.stats()
            tile_ms += st.tile_kernel_ms; sp_ms += st.special_kernel_ms; launches += st.tile_kernel_launches
        dt = (time.perf_counter() - t0) / steps
        case = {"special_rows_per_view": k, "pairs_per_s": len(pairs) / dt, "ms_per_step": dt * 1e3,
                "relative_to_headline": headline_ms / (dt * 1e3),
                "tile_kernel_ms_per_step": tile_ms / steps, "special_kernel_ms_per_step": sp_ms / steps,
                "tile_kernel": "match_tile_kernel<8, false, true, true> only (special_kernel_launches > 0: "
                               + str(bool(st.special_kernel_launches > 0)) + ")"}
        if with_cpu:
            import oracle_lib
            objs = m.as_objects(ra, corr)
            bad, checked = [], 0
            for idx in np.linspace(0, len(pairs) - 1, 3).astype(int):
                tv = objs[idx]
                a, b = pairs[idx]
                e12, _ = oracle_lib.oracle_pairwise_match(sub.sift[a], sub.surf[a], sub.sift[b], sub.surf[b])
                ids = np.nonzero(e12 >= 0)[0]
                exp = np.stack([ids, e12[ids]], axis=1).astype(np.int32)
                if tv.status == capi.PAIR_MATCHED:
                    checked += 1
                    if not np.array_equal(np.asarray(tv.matches), exp):
                        bad.append([int(a), int(b)])
            case["parity_checked_pairs"] = checked
            case["parity_ok"] = not bad
            if bad:
                case["parity_bad_pairs"] = bad
        out["cases"].append(case)
        m.close()
    return out


def feature_all_bench(V, F, n_surf, pairs, device_index, steps, sift_pop_s, with_cpu):
    """The application's FEATURE_ALL (matching_mve.cpp:333, exhaustive_matching.cc:114-180): every view carries SIFT
    AND SURF descriptors -- F + n_surf per view through osfm_match_all (low-res gate on the SIFT block, two-way
    matching of both types, cross-check, combined lists).  pairs/s of the whole pass, and the D = 64 tile kernel's
    rate from its own launches (osfm_match_stats.surf_*), beside the D = 128 kernel's of the same pass."""
    from orthosfm_amd import capi, synth
    from orthosfm_amd.matching import HipExhaustiveMatching
    iset = synth.make_image_set(V, F, n_surf=n_surf, config_id=2)
    m = HipExhaustiveMatching(V, device=device_index, copy_results=False)
    for v in range(V):
        m.set_view(v, iset.sift[v], iset.surf[v])
    cap = (F + n_surf) * len(pairs)
    m.use_result_buffer(capi.pinned_rows(cap))
    parr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    for _ in range(2):
        m.compute_arrays(parr, capacity=cap)
    t0 = time.perf_counter()
    tile_ms = surf_ms = 0.0
    macs = surf_macs = 0
    for _ in range(steps):
        ra, corr = m.compute_arrays(parr, capacity=cap)
        st = m.stats()
        tile_ms += st.tile_kernel_ms; surf_ms += st.surf_tile_kernel_ms
        macs += st.mac_count; surf_macs += st.surf_mac_count
    dt = (time.perf_counter() - t0) / steps
    n_corr = int(np.where(ra["status"] == capi.PAIR_MATCHED, ra["num_matches"], 0).sum())
    out = {"workload": f"{V} views x ({F} SIFT + {n_surf} SURF), {len(pairs)} pairs, exhaustive, both types combined per pair",
           "pairs_per_s": len(pairs) / dt, "ms_per_step": dt * 1e3, "correspondences": n_corr,
           "surf_tile_kernel": {"kernel": "match_tile_kernel<4, false, true, ...> (D = 64)", "ms_per_step": surf_ms / steps,
                                "achieved_TOPs": 2.0 * surf_macs / max(surf_ms, 1e-9) / 1e9,
                                "frac_of_int8_peak": 2.0 * surf_macs / max(surf_ms, 1e-9) / 1e9 / I8_MFMA_PEAK_TOPS},
           "sift_tile_kernel": {"ms_per_step": (tile_ms - surf_ms) / steps,
                                "achieved_TOPs": 2.0 * (macs - surf_macs) / max(tile_ms - surf_ms, 1e-9) / 1e9,
                                "headline_achieved_TOPs": sift_pop_s}}
    if with_cpu:
        import oracle_lib
        objs = m.as_objects(ra, corr)
        bad, checked = [], 0
        for idx in np.linspace(0, len(pairs) - 1, 2).astype(int):
            tv = objs[idx]
            a, b = pairs[idx]
            e12, _ = oracle_lib.oracle_pairwise_match(iset.sift[a], iset.surf[a], iset.sift[b], iset.surf[b])
            ids = np.nonzero(e12 >= 0)[0]
            exp = np.stack([ids, e12[ids]], axis=1).astype(np.int32)
            if tv.status == capi.PAIR_MATCHED:
                checked += 1
                if not np.array_equal(np.asarray(tv.matches), exp):
                    bad.append([int(a), int(b)])
        out["parity_checked_pairs"] = checked
        out["parity_ok"] = not bad
    m.close()
    return out


def multi_device_front_bench(iset, V, pairs, capacity, device_index, ndev_visible, steps, ref_ra, ref_corr):
    """osfm_match_create_multi from ONE process (what the reference's single C++ caller can use):
    all visible devices when there are several, else two logical shards on the one device --
    then the number says what the front costs (one more pass over the lists on the host), not
    what a second GPU gains.  Records and list bytes are compared with the timed single-device pass."""
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    devs = list(range(ndev_visible)) if ndev_visible > 1 else [device_index, device_index]
    m = HipExhaustiveMatching(V, device=devs, copy_results=False)
    for v in range(V):
        m.set_view(v, iset.sift[v])
    m.use_result_buffer(capi.pinned_rows(capacity))
    m.compute_arrays(pairs, capacity=capacity)
    t0 = time.perf_counter()
    for _ in range(steps):
        ra, corr = m.compute_arrays(pairs, capacity=capacity)
    dt = (time.perf_counter() - t0) / steps
    n = int(np.where(ra["status"] == capi.PAIR_MATCHED, ra["num_matches"], 0).sum())
    same = ra.tobytes() == ref_ra.tobytes() and corr[:n].tobytes() == ref_corr[:n].tobytes()
    m.close()
    return {"devices": devs, "logical_shards_on_one_device": ndev_visible <= 1, "pairs_per_s": len(pairs) / dt,
            "ms_per_step": dt * 1e3, "identical_to_single_device": bool(same)}


def per_pair_latency(m, pairs, n=24):
    """The drop-in interface as the reference calls it: one MatchingBase::pairwise_match
    per pair (osfm_match_pair: launch, finish, cross-check, two device-to-host copies,
    one synchronisation each), next to the batched osfm_match_all rate."""
    sel = [pairs[i] for i in np.linspace(0, len(pairs) - 1, n).astype(int)]
    m.pairwise_match(*sel[0])
    t0 = time.perf_counter()
    for a, b in sel:
        m.pairwise_match(a, b)
    dt = (time.perf_counter() - t0) / len(sel)
    t0 = time.perf_counter()
    for a, b in sel:
        m.pairwise_match_lowres(a, b, 500)
    dl = (time.perf_counter() - t0) / len(sel)
    # the reference's loop is an OpenMP parallel for over the pairs (bundler_matching.cc:86-88): the
    # same two calls per pair from `threads` host threads; the library combines whatever calls are
    # waiting into one batch per kind
    import threading
    threads = 16
    many = [pairs[i] for i in np.linspace(0, len(pairs) - 1, min(len(pairs), 30 * threads)).astype(int)]

    def worker(k):
        for a, b in many[k::threads]:
            if m.pairwise_match_lowres(a, b, 500) >= 5:
                m.pairwise_match(a, b)

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dc = time.perf_counter() - t0
    out = {"interface": "MatchingBase::pairwise_match / pairwise_match_lowres, one call per pair (through ctypes)",
           "pairwise_match_ms": dt * 1e3, "pairwise_match_lowres_ms": dl * 1e3, "pairs_per_s": 1.0 / (dt + dl),
           "sample": f"{len(sel)} pairs of 20k x 20k features",
           "concurrent": {"threads": threads, "pairs": len(many), "pairs_per_s": len(many) / dc,
                          "what": "gate + match per pair from 16 Python threads (the interpreter lock serialises "
                                  "the wrapper around the calls)"}}
    # the same loop in the reference's language: tests/host/drop_in_bench.cc, an OpenMP parallel for over
    # the C ABI (a child process with its own matcher: 50 views x 20k features, 1225 pairs)
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "host", "drop_in_bench")
    if os.path.exists(exe):
        import subprocess
        try:
            r = subprocess.run([exe, "50", "20000", "32"], capture_output=True, text=True, timeout=120)
            lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode == 0 and len(lines) == 2:
                out["openmp"] = {"serial_pairs_per_s": lines[0]["pairs_per_s"], "threads": lines[1]["threads"],
                                 "pairs_per_s": lines[1]["pairs_per_s"], "pairs": lines[1]["pairs"],
                                 "identical_to_serial": True}
            else:
                out["openmp"] = {"error": (r.stderr or r.stdout)[-300:]}
        except Exception as e:
            out["openmp"] = {"error": str(e)}
    return out


def schedule_kinds(num_views):
    """The bundle-adjustment calls runPoseEstimation issues for V views (reconstruct.cpp:193-281)."""
    kinds = []
    for g in range(1, num_views - 1):
        kinds.append("local")
        if g > 1 and g % 3 == 0:
            kinds.append("global")
    kinds.append("final")
    return kinds


def end_to_end_bench(args, device_index, cpu_pairs_per_s, cpu_ransac_s_per_pair, tracks_cpu_ms_per_match, cores):
    """BASELINE configs[2]'s image set on ONE GPU: (a) the matching pass alone (the N = 1
    point of the strong-scaling config), (b) the whole job -- match + RANSAC-F, tracks,
    group ordering, incremental bundle adjustment with the reference's schedule -- as one
    wall clock, with the CPU path beside it: the pinned matcher oracle and the RANSAC
    oracle sampled and extrapolated over the pairs, the reference's Tracks::compute
    scaled by matches, the BA oracle on sampled calls of the same schedule scaled by
    iterations x observations (SURVEY 8d allows sampling: the work per pair is
    data-independent)."""
    from orthosfm_amd import capi, pipeline as P, synth
    from orthosfm_amd.matching import HipExhaustiveMatching
    V, F = args.e2e_views, args.features
    t0 = time.perf_counter()
    iset = synth.make_image_set(V, F, config_id=3)
    gen_s = time.perf_counter() - t0
    pairs = [capi.pair_from_index(i) for i in range(V * (V - 1) // 2)]
    out = {"workload": f"{V} orthographic images, {F} SIFT features/img, {len(pairs)} pairs", "generate_s": gen_s}
    # (a) matching only, as the headline pass
    m = HipExhaustiveMatching(V, device=device_index, copy_results=False)
    t0 = time.perf_counter()
    for v in range(V):
        m.set_view(v, iset.sift[v])
    up = time.perf_counter() - t0
    cap = F * len(pairs)
    m.compute(pairs, capacity=cap)
    t0 = time.perf_counter()
    res = m.compute(pairs, capacity=cap)
    dt = time.perf_counter() - t0
    st = m.stats()
    out["matching_single_gpu"] = {"pairs_per_s": len(pairs) / dt, "s_per_pass": dt, "upload_s": up,
                                  "tile_kernel_ms": st.tile_kernel_ms, "tile_kernel_launches": int(st.tile_kernel_launches),
                                  "matched_pairs": int(sum(1 for tv in res if tv.status == capi.PAIR_MATCHED)),
                                  "correspondences": int(sum(tv.num_matches for tv in res if tv.status == capi.PAIR_MATCHED))}
    m.close()
    del res
    # (b) the whole job
    kinds = schedule_kinds(V)
    loc = [i for i, k in enumerate(kinds) if k == "local"]
    glo = [i for i, k in enumerate(kinds) if k == "global"]
    capture = set()
    if not args.no_cpu_baseline:
        capture = {loc[len(loc) // 4], loc[len(loc) // 2], loc[-1]}
        if glo:
            capture |= {glo[len(glo) // 3], glo[-1]}
    # the timed job keeps the track table on the device (osfm_scene_*); the same job in the per-call form (every step
    # flattens its tracks on the host and goes through osfm_ba_solve / _triangulate / _filter_reprojection) runs behind
    # it, untimed here but reported: it is where the sampled BA problems for the CPU baseline come from, and its
    # cameras must be the scene's to the bit
    # (three runs, the MEDIAN one reported and all listed -- the CPU side is a single extrapolation, so this side is not
    #  the best of several either; the job's first call sizes 9 GB of work arrays while the uploads allocate beside it,
    #  and how long the driver takes for that varies by 0.8 s between runs of the same process)
    runs = [P.reconstruct(iset, solver=0, device=device_index) for _ in range(3)]
    r = sorted(runs, key=lambda x: x.timings.total_s)[1]
    r_cap = P.reconstruct(iset, solver=0, device=device_index, capture=capture, use_scene=False) if capture else None
    tm = r.timings
    gpu_total = tm.total_s
    calls = r.ba_calls
    job = {"gpu_wall_s": gpu_total,
           "stages_s": {"descriptor_upload": tm.upload_s, "matching_with_ransac": tm.matching_s,
                        "of_which_matcher_and_page_locked_buffers": tm.setup_s, "tracks": tm.tracks_s,
                        "track_conversion": tm.convert_s, "group_ordering": tm.groups_s,
                        "pose_estimation": tm.pose_s,
                        "pose_parts": {"local_ba": tm.local_ba_s, "reprojection_filter": tm.local_filter_s,
                                       "triangulate_all_tracks": tm.triangulate_s, "global_ba": tm.global_ba_s,
                                       "outlier_filter": tm.outlier_filter_s, "host_flattening": tm.pose_host_s}},
           "matched_pairs": r.matched_pairs, "correspondences_after_ransac": r.correspondences,
           "tracks": r.num_mve_tracks, "invalid_tracks": r.invalid_mve_tracks, "groups": len(r.groups),
           "cameras": len(r.aligned_views), "tracks_after_filters": r.tracks.num_tracks,
           "ba_calls": {k: {"n": sum(1 for c in calls if c.kind == k), "iterations": sum(c.iterations for c in calls if c.kind == k),
                            "ms": sum(c.ms for c in calls if c.kind == k)} for k in ("local", "global", "final")},
           "schedule": "local 3-camera BA per group, global BA every 3rd group, final BA (reconstruct.cpp:193-281); "
                       "new cameras start from the ground truth perturbed by 2 deg / 0.01 (Tomasi-Kanade is out of scope)",
           "track_table": "resident on the device (osfm_scene_*); pose_parts.local_ba includes the group's reprojection filter",
           "gpu_wall_s_of_all_runs": [x.timings.total_s for x in runs], "reported": "median run"}
    if r_cap is not None:
        job["per_call_form"] = {"gpu_wall_s": r_cap.timings.total_s, "pose_estimation_s": r_cap.timings.pose_s,
                                "identical_cameras": bool(np.array_equal(r.cam_params, r_cap.cam_params)),
                                # (live features: alive features of alive tracks -- the per-call form works on compacted
                                #  copies and leaves the feature flags of tracks that were dead at a compaction cleared)
                                "identical_flags_and_points": bool(np.array_equal(r.tracks.alive_t, r_cap.tracks.alive_t) and
                                                                   np.array_equal(r.tracks.live_f, r_cap.tracks.live_f) and
                                                                   np.array_equal(r.tracks.alive_t & r.tracks.has_point, r_cap.tracks.alive_t & r_cap.tracks.has_point) and
                                                                   np.array_equal(r.tracks.point[r.tracks.alive_t & r.tracks.has_point],
                                                                                  r_cap.tracks.point[r_cap.tracks.alive_t & r_cap.tracks.has_point]))}
    gt, _ = P.canonical_ground_truth(iset, 0)
    ang = []
    for v in r.aligned_views:
        Rg, Rc = P._cam_rotation(0, gt[v]), P._cam_rotation(0, r.cam_params[v])
        ang.append(float(np.degrees(np.arccos(np.clip((np.trace(Rg.T @ Rc) - 1) / 2, -1, 1)))))
    job["max_rotation_error_deg"] = max(ang)
    if not args.no_cpu_baseline and cpu_pairs_per_s:
        import oracle_lib
        # BA schedule on the CPU oracle: sampled calls, scaled by iterations x observations
        rate = {"local": [], "global": []}
        ba_ok = True
        for ci, (kind, prob, retri) in sorted(r_cap.captured.items()):
            sc = synth.BaScene(prob.model, prob.cam_params.copy(), prob.cam_const.copy(), prob.img_w.copy(), prob.img_h.copy(),
                               prob.points.copy(), prob.obs_xy.copy(), prob.obs_camera.copy(), prob.obs_point.copy(),
                               prob.cam_params.copy(), prob.points[:, :3].copy())
            t0 = time.perf_counter()
            if retri:
                oracle_lib.oracle_ba_triangulate(sc)
            so = oracle_lib.oracle_ba_solve(sc)
            dtc = time.perf_counter() - t0
            rate[kind].append(dtc / max(1, max(so.num_iterations, 1) * prob.obs_camera.shape[0]))
            ba_ok &= so.num_iterations == calls[ci].iterations
        cpu_ba = 0.0
        for c in calls:
            k = "local" if c.kind == "local" else "global"
            if rate[k]:
                cpu_ba += float(np.mean(rate[k])) * max(c.iterations, 1) * c.observations
        cpu_match = len(pairs) / cpu_pairs_per_s
        cpu_ransac = cpu_ransac_s_per_pair * len(pairs) / max(cores, 1)
        cpu_tracks = tracks_cpu_ms_per_match * r.correspondences * 1e-3
        cpu_total = cpu_match + cpu_ransac + cpu_tracks + cpu_ba
        job["cpu_baseline"] = {"value": cpu_total, "unit": "s (extrapolated)", "cores": int(cores), "kind": "port",
                               "parts_s": {"matching": cpu_match, "ransac": cpu_ransac, "tracks": cpu_tracks, "bundle_adjustment": cpu_ba},
                               "sample": f"matching: the headline's sampled oracle rate x {len(pairs)} pairs; RANSAC-F: oracle on sampled "
                                         f"pairs, one thread each, spread over {cores} cores; tracks: the reference's code scaled by matches; "
                                         f"BA: the oracle on {len(r_cap.captured)} calls of the same schedule scaled by iterations x observations "
                                         "(group ordering and the filters are NOT counted on the CPU side)",
                               "ba_iteration_counts_equal_gpu": bool(ba_ok)}
        job["speedup_vs_cpu"] = cpu_total / gpu_total
    out["end_to_end"] = job
    return out


def config1_plumbing():
    """BASELINE configs[0]: the 3-view Suzanne subset with --solver=0, end to end (match -> verify ->
    tracks -> group -> local BA -> final BA) and as the test bench's own problem (one track per vertex,
    every camera), GPU next to the CPU oracle.  A plumbing run: small, no roofline."""
    import oracle_lib
    from orthosfm_amd import ba as B, pipeline as P, synth
    pts, cams, width, height = synth.suzanne_scene(3)
    iset = synth.make_image_set(3, 3000, config_id=72, landmarks=pts, cameras=cams, width=width, height=height)
    P.reconstruct(iset, solver=0, seed=3)
    t0 = time.perf_counter()
    res = P.reconstruct(iset, solver=0, seed=3)
    t_e2e = time.perf_counter() - t0
    gt, _ = P.canonical_ground_truth(iset, 0)
    err = max(float(np.degrees(np.arccos(np.clip((np.trace(P._cam_rotation(0, gt[v]).T @ P._cam_rotation(0, res.cam_params[v])) - 1) / 2, -1, 1))))
              for v in range(3))
    sc = synth.make_suzanne_ba_scene(0, 3)
    ref = sc.copy()
    t0 = time.perf_counter()
    so = oracle_lib.oracle_ba_solve(ref)
    t_cpu = time.perf_counter() - t0
    fp = B.FlatProblem.from_scene(sc)
    B.solve(B.FlatProblem.from_scene(sc.copy()))
    t0 = time.perf_counter()
    s = B.solve(fp)
    t_gpu = time.perf_counter() - t0
    print(json.dumps({
        "metric": METRIC, "config": {"workload": "BASELINE configs[0]: 3 views of the reference's Suzanne model (7872 vertices, the first three "
                                                   "cameras of its test bench), --solver=0 quaternion; plumbing run", "views": 3},
        "data": "tests/golden/cfg1_suzanne.npz (reference's resources/Suzanne.ply + dataset_generation.cpp:14-38) + synthetic descriptors",
        "end_to_end_s": t_e2e, "tracks": int(res.num_mve_tracks), "groups": len(res.groups),
        "ba_calls": [c.kind for c in res.ba_calls], "max_rotation_error_deg": err,
        "testbench_problem": {"tracks": int(sc.points.shape[0]), "observations": int(sc.obs_xy.shape[0]),
                              "gpu_iterations": int(s.num_iterations), "oracle_iterations": int(so.num_iterations),
                              "gpu_final_cost": float(s.final_cost), "oracle_final_cost": float(so.final_cost),
                              "gpu_solve_ms": t_gpu * 1e3, "cpu_oracle_solve_ms": t_cpu * 1e3,
                              "identical_iteration_count": bool(s.num_iterations == so.num_iterations)}}))


def main():
    args = parse()
    plan = launch_plan(sys.argv[1:], os.environ, args.gpus, args.single_process, args.config)
    if plan is not None:
        raise SystemExit(run_child(plan))
    if args.config == 1:
        config1_plumbing()
        return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch = None
    if world > 1:
        # torch first: it brings its own ROCm runtime, which libosfm_hip.so then shares
        import torch
        import torch.distributed as dist
    from orthosfm_amd import capi, synth
    from orthosfm_amd import distributed as D
    from orthosfm_amd.matching import HipExhaustiveMatching

    ndev = capi.device_count()
    if ndev < 1:
        raise RuntimeError("bench.py: no HIP device (the backend has no CPU fallback)")
    device_index = local_rank % ndev
    tdev = "cpu"
    if world > 1:
        if args.backend == "nccl":
            torch.cuda.set_device(device_index)
            tdev = torch.device("cuda", device_index)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=tdev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    # N = 1: configs[1] (50 views).  N > 1: configs[2], 200 views held fixed (strong
    # scaling); --weak grows the set instead (50 / 71 / 100 / 141 views: ~1225 pairs per rank)
    V = args.views
    scaling = "strong"
    config_id = 2
    if V <= 0:
        if world == 1 and not (args.single_process and args.gpus > 1):
            V = 50
        elif args.weak:
            scaling = "weak"
            V = 50
            while V * (V - 1) // 2 < 1225 * world:
                V += 1
        else:
            V, config_id = 200, 3
    F = args.features
    iset = synth.make_image_set(V, F, config_id=config_id)
    all_pairs = [capi.pair_from_index(i) for i in range(V * (V - 1) // 2)]
    view_sizes = np.array([iset.sift[v].shape[0] for v in range(V)])
    shards = D.deal_pairs(all_pairs, view_sizes, world)
    my_pairs = [all_pairs[i] for i in shards[rank]]
    my_pairs_arr = np.asarray(my_pairs, dtype=np.int32).reshape(-1, 2)     # marshalled once: the timed step passes the array

    o1 = capi.default_match_options()
    if args.no_lowres_gate:
        o1.use_lowres_matching = 0
        o1.min_feature_matches = 0
    front_devices = None
    if world == 1 and args.single_process and args.gpus > 1:
        # one process, several devices behind the C ABI (logical shards on device 0 when the box has fewer)
        front_devices = [d % ndev for d in range(args.gpus)]
    m = HipExhaustiveMatching(V, device=front_devices if front_devices else device_index, options=o1, copy_results=False)
    t0 = time.perf_counter()
    for v in range(V):
        m.set_view(v, iset.sift[v])
    upload_s = time.perf_counter() - t0
    capacity = F * max(len(my_pairs), 1)

    def barrier():
        if world > 1:
            dist.barrier()
            if args.backend == "nccl":
                torch.cuda.synchronize()

    store = None
    if world > 1 and args.exchange == "shm":
        # the matcher writes its lists into this rank's slice of the shared segment
        try:
            store = D.SharedMatchStore(F * max(len(s) for s in shards), rank, world, tdev)   # same on every rank
            m.use_result_buffer(store.slice)
        except D.SharedSegmentUnavailable:
            args.exchange = "rccl"
    if store is None:
        # page-locked result buffer (what a host integration hands the matcher): the lists leave the
        # device at full PCIe rate, at N > 1 on to the gather; pageable memory goes through staging
        m.use_result_buffer(D.pinned_array("local", capacity, tdev) if world > 1 else capi.pinned_rows(capacity))
    gathered = [None]

    last = [None, None]

    def step():
        # the C ABI's own result form (records + one list buffer); the per-pair objects of the
        # Python mirror are built once, after the timed loop
        ra, corr = m.compute_arrays(my_pairs_arr, capacity=capacity)
        last[0], last[1] = ra, corr
        st = m.stats()
        counts = np.where(ra["status"] == capi.PAIR_MATCHED, ra["num_matches"], 0).astype(np.int64)
        n_corr = int(counts.sum())
        # the only collective of the path: the match lists travel to rank 0
        # (pair order restored there) for RANSAC / track building
        if store is not None:
            gathered[0] = store.collect(counts, len(all_pairs), shards)
        elif world > 1:
            gathered[0] = D.gather_match_lists(counts, m.last_flat, len(all_pairs), rank, world, device=tdev, shards=shards)
        return None, st, n_corr

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    kern_ms, kern_launches, macs, n_corr = 0.0, 0, 0, 0
    shader_cycles = refclk_ticks = 0.0
    for _ in range(args.steps):
        out, st, n_corr = step()
        kern_ms += st.tile_kernel_ms
        kern_launches += st.tile_kernel_launches
        macs += st.mac_count
        shader_cycles += st.tile_shader_cycles
        refclk_ticks += st.tile_refclk_ticks
    barrier()
    dt = time.perf_counter() - t0
    dt = D.max_over_ranks(dt, world, device=tdev)
    out = m.as_objects(last[0], last[1])          # the lists of the last timed pass, per pair
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, out)
    total_pairs = len(all_pairs)
    extras = rank == 0 and world == 1

    # the sampled CPU baseline, checked against the lists of the timed pass (rank 0's pairs)
    cpu_base, parity_checked, parity_bad = None, 0, []
    if rank == 0 and not args.no_cpu_baseline:
        gpu_lists = [None] * len(all_pairs)
        for gi, tv in zip(shards[0], out):
            if tv.status == capi.PAIR_MATCHED:
                gpu_lists[int(gi)] = tv.matches
        cpu_base, parity_checked, parity_bad = cpu_baseline(iset, all_pairs, args.cpu_sample_pairs, gpu_lists)

    latency = None
    if extras and not args.no_ba:
        try:
            latency = per_pair_latency(m, my_pairs)
        except Exception as e:
            latency = {"error": str(e)}

    # the same pass continued through geometric verification (RANSAC-F,
    # bundler_matching.cc:194-219), reported beside the headline number
    verified = None
    ransac_cpu_s_per_pair = 0.0
    if not args.no_verify:
        o2 = capi.default_match_options()
        o2.geometric_verification = 1
        m2 = HipExhaustiveMatching(V, device=device_index, options=o2, copy_results=False)
        for v in range(V):
            m2.set_view(v, iset.sift[v])
            m2.set_positions(v, normalised_positions(iset, v))
        m2.compute(my_pairs, capacity=capacity)
        barrier()
        t1 = time.perf_counter()
        outv = m2.compute(my_pairs, capacity=capacity)
        barrier()
        dtv = D.max_over_ranks(time.perf_counter() - t1, world, device=tdev)
        verified = {"pairs_per_s": len(all_pairs) / dtv, "ms_per_step": dtv * 1e3,
                    "ransac": "1000 iterations, threshold 0.0015, >= 30 inliers; the sampler is a counter-based stream "
                              "(the reference's shared std::rand is not reproducible): inlier sets are parity-unpinned "
                              "against the reference, bit-identical to the oracle",
                    "accepted_pairs_rank0": int(sum(1 for tv in outv if tv.status == capi.PAIR_MATCHED)),
                    "inliers_rank0": int(sum(tv.num_inliers for tv in outv if tv.status == capi.PAIR_MATCHED))}
        if extras and not args.no_cpu_baseline:
            # RANSAC-F on the CPU oracle for a few pairs of the timed pass (and the same inliers)
            import oracle_lib
            ts, same = [], True
            for k in np.linspace(0, len(out) - 1, 4).astype(int):
                tv, tw = out[k], outv[k]
                if tv.status != capi.PAIR_MATCHED:
                    continue
                a, b = tv.view_1_id, tv.view_2_id
                pid = a * (a - 1) // 2 + b
                t1 = time.perf_counter()
                n, inl, _ = oracle_lib.oracle_ransac(normalised_positions(iset, a), normalised_positions(iset, b),
                                                     np.asarray(tv.matches), pair_id=pid)
                ts.append(time.perf_counter() - t1)
                same &= tw.status == capi.PAIR_MATCHED and np.array_equal(np.asarray(tv.matches)[inl], np.asarray(tw.matches))
            if ts:
                ransac_cpu_s_per_pair = float(np.mean(ts))
                verified["cpu_baseline"] = {"value": ransac_cpu_s_per_pair * 1e3, "unit": "ms per pair (RANSAC-F alone)", "cores": 1,
                                            "kind": "port", "sample": f"{len(ts)} pairs of the timed pass", "identical_inliers": bool(same)}
        m2.close()

    multi_front = None
    if extras and not args.no_realistic:
        try:
            multi_front = multi_device_front_bench(iset, V, my_pairs, capacity, device_index, ndev, max(args.steps, 3),
                                                   last[0].copy(), np.array(last[1], copy=True))
        except Exception as e:
            multi_front = {"error": repr(e)}

    realistic = None
    if extras and not args.no_realistic:
        try:
            realistic = realistic_operands_bench(iset, V, my_pairs, capacity, device_index, dt / args.steps * 1e3,
                                                 max(args.steps, 3), not args.no_cpu_baseline)
        except Exception as e:
            realistic = {"error": repr(e)}

    feature_all = None
    if extras and not args.no_realistic:
        try:
            ach = 2.0 * macs / max(kern_ms, 1e-9) / 1e9
            feature_all = feature_all_bench(V, F, 5000, my_pairs, device_index, max(args.steps // 2, 3), ach, not args.no_cpu_baseline)
        except Exception as e:
            feature_all = {"error": repr(e)}

    gated = None
    if extras and not args.no_verify and not args.no_ba:
        try:
            gated = gated_bench(V, F, device_index)
        except Exception as e:
            gated = {"error": str(e)}

    cascade = None
    if extras and not args.no_ba and not args.no_verify:
        try:
            cascade = cascade_bench(iset, V, my_pairs, capacity, device_index, not args.no_cpu_baseline)
        except Exception as e:
            cascade = {"error": str(e)}

    # N > 1: rank 0 consumes the lists of all ranks where the exchange left them
    exchanged = None
    if args.full and rank == 0 and world > 1 and gathered[0] is not None:
        exchanged = exchanged_tracks(gathered[0], all_pairs, V, F, args.exchange)

    tracks = None
    if extras and not args.no_ba:
        try:
            tracks = tracks_bench(out, V, F, not args.no_cpu_baseline)
        except Exception as e:
            tracks = {"error": str(e)}

    ba = None
    if not args.no_ba and rank == 0:
        try:
            from orthosfm_amd import ba as ba_mod
            ba = ba_mod.bench_global_ba()
            ba["roofline"] = ba_roofline(ba)
        except Exception as e:       # BA reporting must never hide the matching line
            ba = {"error": str(e)}

    if ba is not None and "error" not in ba and not args.no_cpu_baseline and rank == 0:
        ba["cpu_baseline"] = ba_cpu_baseline()

    if ba is not None and "error" not in ba and rank == 0:
        try:
            ba["local_ba"] = ba_mod.bench_local_ba()
            if not args.no_cpu_baseline:
                ba["local_ba"]["cpu_baseline"] = local_ba_cpu_baseline(ba["local_ba"])
        except Exception as e:
            ba["local_ba"] = {"error": str(e)}

    if ba is not None and "error" not in ba and rank == 0:
        try:
            ba["outlier_filter"] = outlier_filter_bench(device_index, not args.no_cpu_baseline)
        except Exception as e:
            ba["outlier_filter"] = {"error": str(e)}

    m.close()
    e2e = None
    if extras and not args.no_e2e and not args.no_ba:
        try:
            tr_rate = 0.0
            if tracks and "cpu_baseline" in tracks:
                tr_rate = tracks["cpu_baseline"]["value"] / max(tracks["matches"], 1)
            e2e = end_to_end_bench(args, device_index, cpu_base["value"] if cpu_base else 0.0, ransac_cpu_s_per_pair,
                                   tr_rate, usable_cores())
        except Exception as e:
            e2e = {"error": repr(e)}

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = total_pairs * args.steps / dt
        flops_per_launch = 2.0 * macs / max(kern_launches, 1)
        avg_launch_s = kern_ms / max(kern_launches, 1) * 1e-3
        achieved = flops_per_launch / max(avg_launch_s, 1e-12) / 1e12
        statuses = [tv.status for tv in out]
        traffic, traffic_src = pmc_traffic_per_launch(len(my_pairs) * args.steps / max(kern_launches, 1))
        line = {
            "metric": METRIC,
            "value": value, "unit": "pairs/s", "n_gpus": len(front_devices) if front_devices else world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": scaling, "vs_baseline": None, "dtype": "i8",
            "data": "synthetic",
            "config": {"workload": f"{V} orthographic images, {F} SIFT features/img, exhaustive matching "
                                   f"({total_pairs} pairs, low-res gate + two-way + cross-check + lists; "
                                   "SURVEY 8d's unit of work: up to, not including, RANSAC-F -- the pass through "
                                   "RANSAC-F is `with_geometric_verification`)",
                       "views": V, "features_per_view": F, "pairs": total_pairs,
                       "baseline_config": "configs[1]" if world == 1 else ("configs[2]" if scaling == "strong" else "configs[1] grown (weak)"),
                       "sharding": f"pairs dealt by work (N1*N2, longest first) over {world} rank(s); "
                                   f"{'the image set is the same at every N > 1' if scaling == 'strong' else 'the image set grows with N'}"},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": I8_MFMA_PEAK_TOPS,
                         "unit": "TFLOP/s", "frac": achieved / I8_MFMA_PEAK_TOPS,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_over_algorithmic": (traffic / (st.algorithmic_bytes / max(st.tile_kernel_launches, 1)))
                                                     if traffic else None,
                         "kernel": "match_tile_kernel<8, false, true, true>", "launches_per_step": kern_launches / args.steps,
                         "avg_launch_ms": avg_launch_s * 1e3,
                         # the clock the chip held under this kernel (shader cycles over 100 MHz ticks of sampled
                         # workgroups) and the fraction of the int8 peak AT that clock (the nominal peak is at 2.4 GHz)
                         "held_clock_ghz": (shader_cycles / refclk_ticks * 0.1) if refclk_ticks > 0 else None,
                         "frac_at_held_clock": (achieved / (I8_MFMA_PEAK_TOPS * (shader_cycles / refclk_ticks * 0.1) / 2.4))
                                               if refclk_ticks > 0 else None,
                         "algorithmic_bytes_per_launch": st.algorithmic_bytes / max(st.tile_kernel_launches, 1),
                         "hbm_algorithmic_GBs": (st.algorithmic_bytes / max(st.tile_kernel_launches, 1))
                                                / max(avg_launch_s, 1e-12) / 1e9},
            "matched_pairs_rank0": int(sum(1 for s in statuses if s == capi.PAIR_MATCHED)),
            "correspondences_rank0": int(n_corr),
            "upload_s": upload_s,
        }
        if front_devices:
            line["multi_gpu_note"] = ("one process, osfm_match_create_multi over devices %s: the bank on every device, pairs dealt "
                                      "longest-first, no data-path exchange" % front_devices)
        if world > 1:
            line["rccl_ranks"] = int(dist.get_world_size())
            line["backend"] = args.backend
            line["multi_gpu_note"] = "every rank holds the full descriptor bank; no data-path collective; exchange = " + args.exchange
        if cpu_base is not None:
            line["cpu_baseline"] = cpu_base
            line["parity_checked_pairs"] = parity_checked
            line["parity_ok"] = len(parity_bad) == 0
        if latency is not None:
            line["drop_in_per_pair"] = latency
        if tracks is not None:
            line["tracks"] = tracks
        if exchanged is not None:
            line["exchange"] = exchanged
        if cascade is not None:
            line["cascade_hashing"] = cascade
        if verified is not None:
            line["with_geometric_verification"] = verified
        if multi_front is not None:
            line["single_process_multi_device"] = multi_front
        if realistic is not None:
            line["realistic_operands"] = realistic
            if any(not c.get("parity_ok", True) for c in realistic.get("cases", [])):
                parity_bad = parity_bad + ["realistic_operands"]
        if feature_all is not None:
            line["feature_all"] = feature_all
            if not feature_all.get("parity_ok", True):
                parity_bad = parity_bad + ["feature_all"]
        if gated is not None:
            line["gates_at_work"] = gated
        if ba is not None:
            line["ba"] = ba
            if "error" not in ba:
                # the second half of the metric where the driver's record keeps it: BASELINE configs[3] (200 cameras,
                # 100k tracks) -- LM iterations/s per call (SURVEY 8d's unit: upload, pair lists and write-back included)
                # and inside the LM loop, the HBM fraction of the iteration's algorithmic bytes, one factorisation + solve
                # scalars beside the nested form: the driver's record keeps the scalar keys of `roofline` only
                line["roofline"]["ba_iterations_per_s"] = ba["iterations_per_s"]
                line["roofline"]["ba_lm_loop_iterations_per_s"] = ba["lm_loop_iterations_per_s"]
                line["roofline"]["ba_frac"] = ba["roofline"]["frac"]
                line["roofline"]["ba_cholesky_ms"] = ba["kernel_ms"]["cholesky"] / max(ba["iterations"], 1)
                line["roofline"]["ba"] = {"iterations_per_s": ba["iterations_per_s"],
                                          "lm_loop_iterations_per_s": ba["lm_loop_iterations_per_s"],
                                          "frac": ba["roofline"]["frac"],
                                          "cholesky_ms": ba["kernel_ms"]["cholesky"] / max(ba["iterations"], 1),
                                          "workload": ba["workload"]}
        if e2e is not None:
            line["config3_single_gpu"] = e2e
        if dumped is not None:
            line["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        print(json.dumps(line))
        if parity_bad:
            raise SystemExit(f"bench.py: GPU match lists differ from the oracle on pairs {parity_bad}")
    if store is not None:
        store.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
