"""How `python bench.py --gpus N` decides about processes: the plan is a pure
function of arguments + environment, and the child it starts is one torchrun with N ranks --
the unit that is sharded is the reference's pair loop, bundler_matching.cc:74-136."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_launch_with_gpus_becomes_one_rank_per_gpu():
    b = _bench()
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "3"]
    plan = b.launch_plan(argv, {}, 8, False, 0)
    assert plan[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in plan and "--nnodes=1" in plan
    assert plan[plan.index("--master-addr") + 1] == "127.0.0.1"
    assert plan[-len(argv):] == argv and plan[-len(argv) - 1].endswith("bench.py")
    # a caller's port is kept
    plan = b.launch_plan(argv, {"MASTER_PORT": "31234"}, 8, False, 0)
    assert plan[plan.index("--master-port") + 1] == "31234"


def test_no_child_for_one_gpu_a_rank_the_front_or_the_plumbing_run():
    b = _bench()
    assert b.launch_plan([], {}, 1, False, 0) is None
    assert b.launch_plan(["--gpus", "4"], {"WORLD_SIZE": "4", "RANK": "2", "LOCAL_RANK": "2"}, 4, False, 0) is None
    assert b.launch_plan(["--gpus", "4", "--single-process"], {}, 4, True, 0) is None
    assert b.launch_plan(["--gpus", "4", "--config", "1"], {}, 4, False, 1) is None


def test_the_child_form_starts_every_rank(tmp_path):
    """`python bench.py --gpus 2 --backend gloo` here (no GPU): the parent must start ONE launcher
    with two ranks, relay their output and pass the failure on -- each rank stops at the library's
    own "no HIP device" (there is no CPU fallback to run instead)."""
    env = dict(os.environ, OSFM_BENCH_MAX_CORES="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--no-ba", "--no-e2e",
                        "--views", "4", "--features", "512", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=600)
    import ctypes.util  # noqa: F401  (the run below is only meaningful without a device)
    from orthosfm_amd import capi
    if capi.device_count() >= 1:
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and line, r.stderr[-2000:]
        import json
        assert json.loads(line[-1])["n_gpus"] == 2
        return
    assert r.returncode != 0
    assert r.stderr.count("no HIP device") >= 2 or r.stderr.count("OSFM_E_DEVICE") >= 2, r.stderr[-3000:]


import pytest  # noqa: E402


@pytest.mark.gpu
def test_two_ranks_from_a_plain_launch_on_one_gpu():
    """VERDICT r4 #2 "Done": the driver's own command form with --gpus 2 (gloo: two ranks share the
    one device of the box) prints ONE line with n_gpus = 2 and the lists of both ranks exchanged
    (--full: the parity check and the track building over the exchanged lists are not headline)."""
    import json
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--full", "--no-ba",
                        "--no-e2e", "--no-verify", "--views", "12", "--features", "3000", "--steps", "2", "--warmup", "1",
                        "--cpu-sample-pairs", "2"],
                       env=env, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["backend"] == "gloo"
    assert rec["config"]["pairs"] == 66 and rec["parity_ok"]
    assert rec["exchange"]["correspondences_all_ranks"] > 0
