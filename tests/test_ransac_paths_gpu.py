"""ransac_kernel where its code changes path, through osfm_ransac_fundamental: against the independent reference of
tests/ransac_cases.py (exact null vector, 200-bit rank-2 step, banded Sampson counts; recorded in
tests/golden/ransac_reference.npz, its power shown without a device in tests/test_ransac_cases_cpu.py) and, bit for
bit, against the twin oracle/ransac_oracle.c.  Against the golden: F within TAU 2^-53 A of F_ref up to sign at unit
Frobenius norm -- A = kappa / gap follows the hypothesis, so this identifies the winner --, the inlier list equal to
the reference's clear inliers (no match of a winner lies in its band), the count its length.  The degenerate inputs
and at_threshold have no independent F and are held to the twin and to their stated properties.

TAU = 0.5: the next power of two above four times 0.0914, the twin's largest ratio over every constrained hypothesis
of every case on the CPU (ransac_cases.TWIN_RATIO).  The kernel is the twin bit for bit, so its ratios are the twin's.

Observed on MI355X, largest max|F -+ F_ref| / (2^-53 A) per case (single-hypothesis scenes: over their 64 samples;
path shapes: the winner's F):
  benign 0.0258   near_planar_1e-2 0.0418   near_planar_1e-4 0.0561   scale_1e-4 0.0000 (6e-6)   edge_1 0.0913
  k_8 - (no inlier, F zero)   k_9 0.0008   k_63 0.0032   k_64 0.0440   k_65 0.0096   k_255 0.0105   k_256 0.0272
  k_257 0.0163   k_1023 0.0125   k_1024 0.0124   k_1025 0.0114   k_1027 0.0083   k_2048 0.0407   k_2049 0.0121
  k_2500 0.0028   iters_1, iters_2 0.0008   iters_256 .. iters_1025 0.0089 (one winner, iteration < 256)
  tie_part1 0.0125   tie_both 0.0142   tie_thread 0.0088   mixed_chunks 0.0020   twins 0.0184
mixed_chunks in mode 2: 0 wrong of 1 476 000 pre-classified tests (1000 hypotheses x the 1476 matches outside chunk 1).
The whole file takes 1.5 s.
"""
import numpy as np
import pytest

import oracle_lib
import ransac_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    assert capi.device_count() >= 1
    return HipExhaustiveMatching


def _run(hm, case):
    return [hm.ransac_fundamental(case.pos1, case.pos2, case.corr, max_iterations=case.max_iterations,
                                  threshold=case.threshold, seed=case.seed, pair_id=p) for p in case.pairs]


_gpu, _twin = {}, {}


def _results(hm, name):
    """The kernel's results of a case in the default mode, computed once."""
    if name not in _gpu:
        _gpu[name] = _run(hm, rc.load(name)[0])
    return _gpu[name]


def _twin_results(name):
    if name not in _twin:
        case, _ = rc.load(name)
        _twin[name] = [oracle_lib.oracle_ransac(case.pos1, case.pos2, case.corr, case.max_iterations, case.threshold,
                                                case.seed, p) for p in case.pairs]
    return _twin[name]


def _same(a, b):
    return all(x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", rc.SINGLE + rc.FULL + ("twins",))
def test_against_the_golden(hm, name):
    case, g = rc.load(name)
    res = _results(hm, name)
    bad, worst = rc.check(name, res)
    print(f"\n[ransac] {name:18s} largest ratio {worst:.4f}")
    assert not bad, bad
    if case.kind != "single":
        n, inl, _ = res[0]
        assert n == g["count_ref"][g["winner"]] and np.array_equal(inl, np.nonzero(rc.mask(g["clear"], case.k))[0])


@pytest.mark.parametrize("name", rc.ALL)
def test_against_the_twin(hm, name):
    case, _ = rc.load(name)
    res, ref = _results(hm, name), _twin_results(name)
    for p, a, b in zip(case.pairs, res, ref):
        assert a[0] == b[0], (name, p, a[0], b[0])
        assert np.array_equal(a[1], b[1]), (name, p)
        assert a[2].tobytes() == b[2].tobytes(), (name, p, np.abs(a[2] - b[2]).max())
    n, inl, F = res[0]
    if name == "identical_views":
        assert n == case.k and np.array_equal(inl, np.arange(case.k))
    elif name == "one_point":
        assert n == 0 and inl.size == 0 and F.tobytes() == np.zeros((3, 3)).tobytes()
    elif name == "at_threshold":
        assert n == rc.AT_THRESHOLD_COUNT and rc.AT_THRESHOLD[2] not in inl


@pytest.mark.parametrize("name", rc.FULL)
def test_double_only_mode_gives_the_same_bytes(hm, name):
    from orthosfm_amd import capi
    res = _results(hm, name)
    try:
        capi.ransac_selfcheck(0)
        double = _run(hm, rc.load(name)[0])
    finally:
        capi.ransac_selfcheck(1)
    assert _same(double, res)


def test_mixed_chunks_counters(hm):
    """Chunk 1 holds a coordinate of 1.5 and one of nextafter(1, 2) and is scored in double; chunks 0 and 2 take the
    pre-classification, every decision of which mode 2 compares with the double path."""
    from orthosfm_amd import capi
    case, _ = rc.load("mixed_chunks")
    res = _results(hm, "mixed_chunks")
    try:
        capi.ransac_selfcheck(2)
        checked = _run(hm, case)
        wrong, undecided, tests = capi.ransac_selfcheck(1)
    finally:
        capi.ransac_selfcheck(1)
    assert _same(checked, res)
    assert wrong == 0
    assert 0 < tests < 2 * case.max_iterations * case.k
    assert tests == case.max_iterations * (case.k - 1024)         # every hypothesis is valid; 1476 matches outside chunk 1
    assert undecided < 0.02 * tests


def test_slots_and_counters_are_reused(hm):
    """The per-pair done counter and the best-of-part slots come from a pool: k = 1025 twice in a row, and once more
    after a k = 8 call, give the same bytes."""
    big, small = rc.load("k_1025")[0], rc.load("k_8")[0]
    first = _results(hm, "k_1025")
    assert _same(_run(hm, big), first)
    assert _same(_run(hm, small), _results(hm, "k_8"))
    assert _same(_run(hm, big), first)
