"""bench.py --dump-outputs: what the last timed step returned, written as .npy files that two
builds can be compared by (float32 / float64, 64 MB at most, a seeded sample beyond that)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pairs(n_pairs, rows_per_pair, seed=5):
    from orthosfm_amd import capi
    from orthosfm_amd.matching import TwoViewMatching
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_pairs):
        a, b = capi.pair_from_index(i)
        if i % 3 == 2:
            out.append(TwoViewMatching(a, b, np.zeros((0, 2), np.int32), status=1, lowres_matches=2))
            continue
        m = rng.integers(0, 20000, size=(rows_per_pair, 2)).astype(np.int32)
        out.append(TwoViewMatching(a, b, m, status=capi.PAIR_MATCHED, lowres_matches=7, num_matches=rows_per_pair))
    return out


def test_dump_writes_records_and_all_lists_when_they_fit(tmp_path):
    b = _bench()
    out = _pairs(9, 50)
    shapes = b.dump_outputs(str(tmp_path), out)
    assert shapes == {"pair_records": [9, 6], "matches": [300, 2]}
    rec = np.load(tmp_path / "pair_records.npy")
    mat = np.load(tmp_path / "matches.npy")
    assert rec.dtype == np.float64 and mat.dtype == np.float32
    assert np.array_equal(rec[:, 0], [tv.view_1_id for tv in out]) and np.array_equal(rec[:, 4], [tv.num_matches for tv in out])
    assert np.array_equal(mat, np.concatenate([tv.matches for tv in out]).astype(np.float32))
    assert not (tmp_path / "matches_rows.npy").exists()


def test_dump_samples_the_lists_beyond_the_budget_the_same_way_every_time(tmp_path):
    b = _bench()
    out = _pairs(30, 4000)
    budget = 200_000
    b.dump_outputs(str(tmp_path / "a"), out, budget=budget)
    b.dump_outputs(str(tmp_path / "b"), out, budget=budget)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= budget
    allm = np.concatenate([tv.matches for tv in out])
    rows = np.load(tmp_path / "a" / "matches_rows.npy")
    mat = np.load(tmp_path / "a" / "matches.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and mat.shape == (rows.shape[0], 2)
    assert rows.shape[0] > 1000
    assert np.array_equal(mat, allm[rows.astype(np.int64)].astype(np.float32))
    for f in ("pair_records.npy", "matches.npy", "matches_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_dump_of_a_small_run_matches_its_result_line(tmp_path):
    """One small headline pass with --dump-outputs: the line reports the steps it was asked for and
    ms_per_step, and the dumped records agree with the counts in the line."""
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-ba", "--no-e2e", "--no-verify",
                        "--no-realistic", "--no-cpu-baseline", "--views", "8", "--features", "3000",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    recs = np.load(d / "pair_records.npy")
    mat = np.load(d / "matches.npy")
    assert recs.shape == (28, 6) and recs.dtype == np.float64 and mat.dtype == np.float32
    from orthosfm_amd import capi
    matched = recs[:, 2] == capi.PAIR_MATCHED
    assert int(matched.sum()) == rec["matched_pairs_rank0"]
    assert int(recs[matched, 4].sum()) == rec["correspondences_rank0"] == mat.shape[0]
