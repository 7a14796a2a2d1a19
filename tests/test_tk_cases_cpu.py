"""The Tomasi-Kanade cases (tests/tk_cases.py) are fit to judge a kernel.  No GPU: every number here
comes from the numpy restatement (tests/tk_restatement.py), never from the library under test.

A float64 kernel agrees with the restatement to ~1e-9 only while no decision sits on a threshold and the
two eigen-problems of a hypothesis are well conditioned; this file bounds both for EVERY hypothesis of
every case -- and for the factorisation of all tracks where the fallback runs --, then checks what the
selection rule is supposed to deliver and that each case of tk_cases.PATH_CASES takes the path it was made
for.  If a case misses a condition its seed changes, never the condition."""
import numpy as np
import pytest

import tk_cases
import tk_restatement as R

ALL_CASES = tk_cases.CASES + tk_cases.PATH_CASES
RANSAC_CASES = [c.name for c in ALL_CASES if c.expect == "ransac"]
SCORED_CASES = [c.name for c in ALL_CASES if c.expect in ("ransac", "fallback")]
DEGENERATE_CASES = [c.name for c in ALL_CASES if c.expect == "degenerate"]
FORCED_FALLBACK = ["fb600", "fb8", "fb5"]               # min_consensus = N
TWIN_CASES = ["twin3", "twin4"]
CHUNK_EDGE_CASES = ["h15", "h16", "h17", "h256", "h257"]
# every hypothesis has the same consensus and a mean error at rounding level: which one wins is not compared
ANY_WINNER = ("exact40", "s32n32")


def _well_conditioned(d):
    assert d["threshold_margin"] > 1e-7                 # no reprojection error within 1e-7 px of max_error_px
    for r in d["metric_ratio"]:                         # lambda_min / lambda_max not within a factor 10 of 1e-9
        assert not (1e-10 <= r <= 1e-8), r
    assert d["gram_cond"] < 1e3                         # w1 / w3
    assert d["gram_gap"] > 1e-6                         # (w3 - w4) / w1


@pytest.mark.parametrize("name", SCORED_CASES)
def test_no_decision_on_a_threshold(name):
    ref = tk_cases.reference(name)
    d = ref.detail
    print(name, "threshold margin %.3g px, usability margin %.3g, lambda ratios min %.3g, gram cond %.3g, gap %.3g"
          % (d["threshold_margin"], d["usable_margin"], min(np.abs(d["metric_ratio"])), d["gram_cond"], d["gram_gap"]))
    assert len(d["metric_ratio"]) == ref.iterations     # every hypothesis got as far as its metric
    _well_conditioned(d)
    assert d["usable_margin"] > 1e-6                    # no usability quantity within 1e-6 of 0.1
    # the factorisation of all tracks, where the fallback runs, under the same conditions
    fb = d["fallback"]
    assert (fb is not None) == (ref.status == R.STATUS_FALLBACK)
    if fb is not None:
        print(name, "fallback: threshold margin %.3g px, lambda ratio %.3g, gram cond %.3g, gap %.3g"
              % (fb["threshold_margin"], fb["metric_ratio"][0], fb["gram_cond"], fb["gram_gap"]))
        assert len(fb["metric_ratio"]) == 1
        _well_conditioned(fb)


@pytest.mark.parametrize("name", DEGENERATE_CASES)
def test_degenerate_inputs_are_far_from_rank_3(name):
    """A condition on the inputs, not a tolerance on the kernel: w3 / w1 of every hypothesis and of the all-track
    matrix is exactly 0 or below 1e-14, a factor 100 clear of the 1e-12 the factorisation tests."""
    ref = tk_cases.reference(name)
    d = ref.detail
    assert len(d["rank_ratio"]) == ref.iterations == 241 and len(d["fallback"]["rank_ratio"]) == 1
    ratios = d["rank_ratio"] + d["fallback"]["rank_ratio"]
    print(name, "largest |w3| / w1 %.3g" % max(ratios))
    assert all(r == 0.0 or r < 1e-14 for r in ratios), max(ratios)
    assert np.isfinite(ratios).all() and d["metric_ratio"] == [] and d["fallback"]["metric_ratio"] == []
    if name == "copies":
        assert max(ratios) == 0.0                       # the Gram matrices are exactly zero


@pytest.mark.parametrize("name", RANSAC_CASES)
def test_selection(name):
    c = tk_cases.BY_NAME[name]
    ref = tk_cases.reference(name)
    _, planted, _ = tk_cases.build(name)
    assert ref.status == R.STATUS_RANSAC
    assert ref.iterations == (c.max_iterations or R.num_iterations(0, c.probability, c.inlier_ratio, c.sample_size))
    assert 0 < ref.supported_models <= ref.usable_models <= ref.iterations
    rank = ref.detail["ranking"]
    if len(rank) > 1 and name not in ANY_WINNER:
        assert rank[0][0] > rank[1][0] or rank[1][1] - rank[0][1] >= 1e-9, rank
    assert not (ref.inlier & planted).any()
    assert ref.num_inliers == int(ref.inlier.sum()) >= c.min_consensus + c.sample_size


def test_iteration_counts():
    """The number of hypotheses: the reference's formula (tomasi_kanade.cpp:212), at least one of them."""
    assert R.num_iterations() == 241
    assert R.num_iterations(sample_size=5) == 37 == tk_cases.reference("s5").iterations
    assert R.num_iterations(sample_size=6, inlier_ratio=0.5, probability=0.99) == 292 == tk_cases.reference("opt6").iterations
    assert R.num_iterations(64, sample_size=32) == 64
    # one sample of 4 is all inliers with probability 0.96 > 0.5: the quotient is 0.21, and one hypothesis runs
    assert R.num_iterations(sample_size=4, inlier_ratio=0.99, probability=0.5) == 1
    clamp = tk_cases.reference("clamp")
    assert (clamp.iterations, clamp.usable_models, clamp.supported_models, clamp.best_iteration) == (1, 1, 1, 0)
    assert R.num_iterations(sample_size=32, inlier_ratio=0.5, probability=0.999) == 1 << 20      # ... and at most 2^20
    for name in CHUNK_EDGE_CASES:
        assert tk_cases.reference(name).iterations == tk_cases.BY_NAME[name].max_iterations == int(name[1:])


def test_path_cases_take_their_paths():
    """What the cases were chosen for, on the restatement."""
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    assert {c.cameras for c in ALL_CASES} == set(range(3, 9))
    assert {c.sample_size for c in ALL_CASES if c.expect != "too_few"} >= {4, 5, 6, 10, 16, 32}
    assert [tk_cases.BY_NAME[n].tracks for n in ("t255", "t256", "t257", "t512", "c8w")] == [255, 256, 257, 512, 600]
    # the winner lies beyond the first chunk; h17's is iteration 16, alone in the last, ragged chunk
    assert tk_cases.reference("h256").best_iteration >= 16 and tk_cases.reference("h257").best_iteration >= 16
    assert tk_cases.reference("h17").best_iteration == 16
    # the same data under another error bound: another winner
    err1, err6 = tk_cases.reference("err1"), tk_cases.reference("err6")
    assert err1.best_iteration != err6.best_iteration and err1.num_inliers < err6.num_inliers
    for a, b in (("err1", "n300"), ("err6", "n300"), ("mc30", "exact40"), ("mc31", "exact40")):
        assert tk_cases.build(a)[0].tobytes() == tk_cases.build(b)[0].tobytes()
    # sample tracks beyond the bound under their own model: the winner's last-drawn one; two of clamp's four
    assert tk_cases.reference("last1").detail["winner_sample_misses"] == [9]
    assert tk_cases.reference("clamp").detail["winner_sample_misses"] == [0, 1]
    # s32n32: every hypothesis is the same 32 tracks, no track is left for a consensus set
    s = tk_cases.reference("s32n32")
    assert (s.usable_models, s.supported_models, s.num_inliers) == (16, 16, 32) and s.inlier.all()
    assert s.detail["ranking"][0][0] == s.detail["ranking"][1][0] == 0


def test_too_few_and_fallback():
    assert tk_cases.reference("n9").status == R.STATUS_TOO_FEW
    for name in ("n34", "n10"):
        ref = tk_cases.reference(name)
        assert ref.status == R.STATUS_FALLBACK and ref.supported_models == 0 and ref.best_iteration == -1
    n35 = tk_cases.reference("n35")
    assert n35.status == R.STATUS_RANSAC and n35.num_inliers == 35          # 25 consensus tracks + the sample
    # a sample needs sample_size tracks
    s = tk_cases.reference("s32n31")
    assert s.status == R.STATUS_TOO_FEW and s.iterations == 0 and not s.inlier.any()
    # min_consensus = N: every hypothesis is usable and scored, none is supported; no track is an outlier
    for name in FORCED_FALLBACK:
        c, ref = tk_cases.BY_NAME[name], tk_cases.reference(name)
        assert c.min_consensus == c.tracks and c.outliers == 0.0
        assert (ref.status, ref.iterations, ref.usable_models, ref.supported_models, ref.best_iteration) == \
            (R.STATUS_FALLBACK, 20, 20, 0, -1)
        assert ref.num_inliers == c.tracks and ref.inlier.all()
    # the consensus boundary: all 241 hypotheses have exactly the 30 tracks outside their sample
    mc30, mc31 = tk_cases.reference("mc30"), tk_cases.reference("mc31")
    assert (mc30.status, mc30.usable_models, mc30.supported_models, mc30.num_inliers) == (R.STATUS_RANSAC, 241, 241, 40)
    assert (mc31.status, mc31.usable_models, mc31.supported_models, mc31.num_inliers) == (R.STATUS_FALLBACK, 241, 0, 40)
    # twin cameras: no hypothesis passes the usability test, by a wide margin; the fallback is not asked
    for name in TWIN_CASES:
        c, ref = tk_cases.BY_NAME[name], tk_cases.reference(name)
        assert (ref.status, ref.iterations, ref.usable_models, ref.supported_models, ref.best_iteration) == \
            (R.STATUS_FALLBACK, 241, 0, 0, -1)
        assert ref.detail["usable_margin"] > 1e-2
        assert ref.num_inliers == c.tracks and ref.inlier.all() and ref.detail["fallback"]["gram_cond"] < 10
        assert R.usable(ref.basis_1)[0] is False
    # no rank-3 measurement matrix: identities, zeros
    for name in DEGENERATE_CASES:
        c, ref = tk_cases.BY_NAME[name], tk_cases.reference(name)
        assert (ref.status, ref.iterations, ref.usable_models, ref.supported_models, ref.best_iteration) == \
            (R.STATUS_DEGENERATE, 241, 0, 0, -1)
        assert ref.num_inliers == 0 and ref.mean_error_px == 0.0 and not ref.inlier.any()
        ident = np.tile(np.eye(3), (c.cameras, 1, 1))
        assert np.array_equal(ref.basis_1, ident) and np.array_equal(ref.basis_2, ident) and not ref.offsets.any()


# (not "clamp": its one model is fitted to four noisy tracks and is 2 degrees off, which is what such a model is)
@pytest.mark.parametrize("name", [n for n in RANSAC_CASES if n != "clamp"] + ["n34", "mc31"] + FORCED_FALLBACK + TWIN_CASES)
def test_rotation_against_ground_truth(name):
    ref = tk_cases.reference(name)
    _, _, truth = tk_cases.build(name)
    err = min(max(R.rotation_error_deg(B[k], truth[k]) for k in range(truth.shape[0]))
              for B in (ref.basis_1, ref.basis_2))
    print(name, "worst camera %.3g deg" % err)
    assert err < (1e-4 if name in ("exact40", "mc30", "mc31") else 1.0)


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
