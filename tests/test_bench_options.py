"""What a plain `bench.py` run does and what `--full` adds: a plain run is the headline alone (set up,
warm up, the timed steps, --dump-outputs, the line); every other leg runs only with --full, where the
--no-* options leave legs out as they always did."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("no_cpu_baseline", "no_ba", "no_verify", "no_e2e", "no_realistic")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_plain_run_leaves_every_leg_out():
    a = _bench().parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full
    assert all(getattr(a, k) for k in LEGS)
    assert (a.gpus, a.steps, a.warmup, a.config, a.dump_outputs) == (1, 20, 5, 0, None)


def test_full_runs_every_leg_unless_one_is_left_out():
    b = _bench()
    a = b.parse(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full and not any(getattr(a, k) for k in LEGS)
    a = b.parse(["--full", "--no-ba", "--no-e2e"])
    assert a.no_ba and a.no_e2e and not (a.no_cpu_baseline or a.no_verify or a.no_realistic)


def test_the_timed_arguments_are_the_same_with_and_without_full(tmp_path):
    b = _bench()
    argv = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--views", "12", "--features", "3000",
            "--dump-outputs", str(tmp_path)]
    plain, full = vars(b.parse(argv)), vars(b.parse(argv + ["--full"]))
    for k in ("gpus", "steps", "warmup", "views", "features", "weak", "single_process", "no_lowres_gate",
              "backend", "exchange", "dump_outputs"):
        assert plain[k] == full[k], k


def test_the_plumbing_run_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr
    assert _bench().parse(["--config", "1", "--full"]).config == 1


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone():
    """A small plain run: one line, the headline's keys and the tile kernel's roofline from the timed
    steps, none of what --full adds."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--views", "8", "--features", "3000",
                        "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads(lines[0])
    assert rec["unit"] == "pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "i8"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - rec["config"]["pairs"] / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert rec["roofline"]["launches_per_step"] > 0 and rec["roofline"]["achieved"] > 0
    for k in ("cpu_baseline", "parity_ok", "drop_in_per_pair", "tracks", "cascade_hashing", "with_geometric_verification",
              "single_process_multi_device", "realistic_operands", "feature_all", "gates_at_work", "ba",
              "config3_single_gpu", "exchange"):
        assert k not in rec, k
    assert not any(k.startswith("ba") for k in rec["roofline"])
