"""The Tomasi-Kanade cases (tests/tk_cases.py) are fit to judge a kernel.  No GPU: every number here
comes from the numpy restatement (tests/tk_restatement.py), never from the library under test.

A float64 kernel agrees with the restatement to ~1e-9 only while no decision sits on a threshold and the
two eigen-problems of a hypothesis are well conditioned; this file bounds both for EVERY hypothesis of
every case, then checks what the selection rule is supposed to deliver.  If a case misses a condition
its seed changes, never the condition."""
import numpy as np
import pytest

import tk_cases
import tk_restatement as R

RANSAC_CASES = [c.name for c in tk_cases.CASES if c.expect == "ransac"]
SCORED_CASES = [c.name for c in tk_cases.CASES if c.expect != "too_few"]


@pytest.mark.parametrize("name", SCORED_CASES)
def test_no_decision_on_a_threshold(name):
    d = tk_cases.reference(name).detail
    print(name, "threshold margin %.3g px, usability margin %.3g, lambda ratios min %.3g, gram cond %.3g, gap %.3g"
          % (d["threshold_margin"], d["usable_margin"], min(np.abs(d["metric_ratio"])), d["gram_cond"], d["gram_gap"]))
    assert d["threshold_margin"] > 1e-7                 # no reprojection error within 1e-7 px of max_error_px
    assert d["usable_margin"] > 1e-6                    # no usability quantity within 1e-6 of 0.1
    for r in d["metric_ratio"]:                         # lambda_min / lambda_max not within a factor 10 of 1e-9
        assert not (1e-10 <= r <= 1e-8), r
    assert d["gram_cond"] < 1e3                         # w1 / w3
    assert d["gram_gap"] > 1e-6                         # (w3 - w4) / w1


@pytest.mark.parametrize("name", RANSAC_CASES)
def test_selection(name):
    c = tk_cases.BY_NAME[name]
    ref = tk_cases.reference(name)
    _, planted, _ = tk_cases.build(name)
    assert ref.status == R.STATUS_RANSAC
    assert ref.iterations == (c.max_iterations or 241)
    assert 0 < ref.supported_models <= ref.usable_models <= ref.iterations
    rank = ref.detail["ranking"]
    if len(rank) > 1 and name != "exact40":             # exact40: every model has all 30 other tracks
        assert rank[0][0] > rank[1][0] or rank[1][1] - rank[0][1] >= 1e-9, rank
    assert not (ref.inlier & planted).any()
    assert ref.num_inliers == int(ref.inlier.sum()) >= 25 + 10


def test_too_few_and_fallback():
    assert tk_cases.reference("n9").status == R.STATUS_TOO_FEW
    for name in ("n34", "n10"):
        ref = tk_cases.reference(name)
        assert ref.status == R.STATUS_FALLBACK and ref.supported_models == 0 and ref.best_iteration == -1
    n35 = tk_cases.reference("n35")
    assert n35.status == R.STATUS_RANSAC and n35.num_inliers == 35          # 25 consensus tracks + the sample


@pytest.mark.parametrize("name", RANSAC_CASES + ["n34"])
def test_rotation_against_ground_truth(name):
    ref = tk_cases.reference(name)
    _, _, truth = tk_cases.build(name)
    err = min(max(R.rotation_error_deg(B[k], truth[k]) for k in range(truth.shape[0]))
              for B in (ref.basis_1, ref.basis_2))
    print(name, "worst camera %.3g deg" % err)
    assert err < (1e-4 if name == "exact40" else 1.0)


def test_sampler():
    s = R.sample(5, 3, 7, 12, 10)
    assert len(set(s)) == 10 and all(0 <= i < 12 for i in s)
    assert s != R.sample(5, 4, 7, 12, 10)
    assert R.num_iterations() == 241
    # first draws, in draw order
    assert s[0] == R.ransac_rand(5, 3, 7, 0) % 12


def test_resolve_ambiguity():
    ref = tk_cases.reference("n300")
    _, _, truth = tk_cases.build("n300")
    Q = tk_cases.quat_to_mat(np.array([0.3, -0.5, 0.2, 0.7]))
    for B, want in ((ref.basis_1, 1), (ref.basis_2, 2)):
        G = np.array([Q @ b for b in B])
        assert R.resolve_ambiguity(ref.basis_1, ref.basis_2, G, [1, 1, 1]) == want
        assert R.resolve_ambiguity(ref.basis_1, ref.basis_2, G, [0, 1, 1]) == want
        assert R.resolve_ambiguity(ref.basis_1, ref.basis_2, G, [0, 0, 1]) == 1
