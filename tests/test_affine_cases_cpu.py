"""The affine RANSAC check of tests/affine_cases.py without a device: the golden is what the generator gives today, the
inputs keep what the cases promise (nothing is decided inside a band, ties lie where the kernel's split puts them, every
refit regime occurs), the restatement -- tests/affine_restatement.py, the kernel's arithmetic in numpy float64 -- meets
the independent reference on every constrained case, and a restatement with one fault of the kind a kernel could have
fails on the case made for it.  The quality and pipeline comparisons of the GPU tests are made here with the two CPU
implementations (the restatement and the 8-point twin oracle_ransac) on the same inputs."""
import math

import numpy as np
import pytest

import affine_cases as ac
import affine_restatement as ar
import oracle_lib

_runs = {}


def _restated(name, **faults):
    case, _ = ac.load(name)
    key = (name, tuple(sorted(faults.items())))
    if key not in _runs:
        _runs[key] = [ar.run(case.pos1, case.pos2, case.corr, case.max_iterations, case.threshold, case.seed, p, case.refit,
                             **faults) for p in case.pairs]
    return _runs[key]


def _equal(a, b):
    return all(x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2].tobytes() == y[2].tobytes() and x[3] == y[3]
               for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# golden and inputs
# ---------------------------------------------------------------------------

def test_golden_is_current():
    for name in ("k_4", "k_5", "iters_1", "iters_2", "refit_larger"):
        case, g = ac.load(name)
        ref = ac.reference(case)
        assert sorted(ref) == sorted(g), name
        for f in ref:
            assert np.asarray(ref[f]).tobytes() == g[f].tobytes(), (name, f)
    for name in ac.SINGLE:
        case, g = ac.load(name)
        m1, m2 = case.matches()
        for j in (0, 63):
            idx = ac.sample4(case.seed, case.pairs[j], 0, case.k)
            h = ac.hypothesis(m1[idx], m2[idx])
            assert h["uncon"] == g["uncon"][j] and h["v"].tobytes() == g["v"][j].tobytes() and h["kappa"] == g["kappa"][j], (name, j)
            clear, amb = ac.classify(h["v"], ac.TAU * h["kappa"], m1, m2, case.threshold)
            assert np.array_equal(clear, ac.mask(g["clear"][j], case.k)) and np.array_equal(amb, ac.mask(g["ambm"][j], case.k))


def test_sample_stream():
    assert ac.sample4(3, 5, 7, 4) == [0, 1, 2, 3] == ar.sample4(3, 5, 7, 4)
    for it in range(50):
        idx = ac.sample4(11, 9, it, 65)
        assert len(set(idx)) == 4 and idx == sorted(idx) and max(idx) < 65 and idx == ar.sample4(11, 9, it, 65)


def test_shapes_follow_the_kernels_constants():
    assert (ac.HYP, ac.CHUNK, ac.SPLIT) == (2, 1024, 2)              # today's; the lists below move with them
    W, G, C, P = ac.WAVE, ac.GROUP, ac.CHUNK, ac.PASS
    assert ac.K_LIST == (4, 5, W - 1, W, W + 1, G - 1, G, G + 1, C - 1, C, C + 1, C + 3, 2 * C + 1)
    assert ac.ITER_LIST == (1, 2, P - 1, P, P + 1, 1000, 2 * P, 2 * P + 1) and max(ac.ITER_LIST) <= 1025 and max(ac.K_LIST) <= 2500
    assert [ac.load(f"k_{k}")[0].k for k in ac.K_LIST] == list(ac.K_LIST)
    # the second part gets none, none, one, many hypotheses; two passes of part 0 beside one hypothesis of part 1
    assert ac.part_of(P - 1, P)[0] == 0 and ac.part_of(P, P + 1) == (1, 0, 0, 0) and ac.part_of(999, 1000)[0] == 1
    assert ac.part_of(P, 2 * P + 1) == (0, 1, 0, 0) and ac.part_of(2 * P, 2 * P + 1) == (1, 0, 0, 0)
    for n in ac.ITER_LIST:
        case, g = ac.load(f"iters_{n}")
        assert case.k == 700 and case.max_iterations == n
        assert np.array_equal(g["count_ref"], ac.load(f"iters_{max(ac.ITER_LIST)}")[1]["count_ref"][:n])


@pytest.mark.parametrize("name", ac.FULL)
def test_nothing_is_decided_inside_a_band(name):
    case, g = ac.load(name)
    un = g["uncon"].astype(bool)
    assert g["count_ref"].size == case.max_iterations and not un.any()
    best, w = int(g["count_ref"].max()), int(g["winner"])
    assert best >= 4 and g["count_ref"][w] == best and (g["count_ref"][:w] < best).all()
    near = g["count_ref"] + g["amb"] >= best
    assert (g["amb"][near] == 0).all(), (name, np.nonzero(near & (g["amb"] > 0))[0])
    assert not ac.mask(g["ambm"], case.k).any() and ac.mask(g["clear"], case.k).sum() == best
    assert bool(g["refit_ran"]) == (case.refit and best >= ac.REFIT_MIN)
    if g["refit_ran"]:
        assert g["refit_amb"] == 0 and not ac.mask(g["refit_ambm"], case.k).any()
        assert ac.mask(g["refit_clear"], case.k).sum() == g["refit_count"]
        assert bool(g["refit_accepted"]) == (g["refit_count"] >= best)


@pytest.mark.parametrize("name", ac.SINGLE)
def test_single_hypothesis_scenes_are_constrained(name):
    case, g = ac.load(name)
    assert case.k == 400 and case.max_iterations == 1 and len(case.pairs) == 64 and not case.refit
    assert g["uncon"].sum() == 0 and g["amb"].sum() <= 64 * case.k // 1000
    assert len({tuple(ac.sample4(case.seed, p, 0, case.k)) for p in case.pairs}) == 64
    print(f"\n[affine cases] {name:18s} kappa {g['kappa'].min():.1e} .. {g['kappa'].max():.1e}, counts "
          f"{g['count_ref'].min()} .. {g['count_ref'].max()}")


def test_what_the_cases_promise():
    m1, m2 = ac.load("edge_1")[0].matches()
    for m in (m1, m2):
        assert np.abs(m).max() == 1.0 and (np.abs(m) == 1.0).sum() >= 4
    m1, m2 = ac.load("scale_1e-4")[0].matches()
    assert max(np.abs(m1).max(), np.abs(m2).max()) < 1e-4
    # the system's rank falls to 3 on a plane: kappa grows with 1 / relief
    kb = np.median(ac.load("benign")[1]["kappa"])
    k2 = np.median(ac.load("near_planar_1e-2")[1]["kappa"])
    k4 = np.median(ac.load("near_planar_1e-4")[1]["kappa"])
    assert kb < 100 and k2 > 20 * kb and 30 < k4 / k2 < 300, (kb, k2, k4)
    # degenerate inputs
    case, _ = ac.load("identical_views")
    m1, m2 = case.matches()
    assert case.k == 600 and np.array_equal(m1, m2) and np.array_equal(m1 * 1024, np.round(m1 * 1024))
    case, _ = ac.load("one_point")
    m1, m2 = case.matches()
    assert case.k == 20 and len({tuple(r) for r in np.concatenate([m1, m2])}) == 1
    case, _ = ac.load("twins")
    both = np.concatenate(case.matches(), axis=1)
    assert case.k == 1200 and 1200 - len({tuple(r) for r in both}) == 360


def test_ties_lie_where_the_kernel_splits():
    for name in ac.TIES:
        case, g = ac.load(name)
        best = g["count_ref"].max()
        its = np.nonzero(g["count_ref"] == best)[0]
        assert its.size >= 2 and its[0] == g["winner"]
        where = [ac.part_of(int(i), case.max_iterations) for i in its]
        if name == "tie_part1":
            assert all(w[0] == 1 for w in where)
        elif name == "tie_both":
            assert where[0][0] == 0 and any(w[0] == 1 for w in where)
        elif name == "tie_thread":
            a, b = where[0], where[1]
            assert a[:2] == b[:2] and its[0] < its[1] and a[2] > b[2]        # same part and pass, the higher thread first
        else:
            a, b = where[0], where[1]
            assert a[:3] == b[:3] and (a[3], b[3]) == (0, 1)                 # the two hypotheses of one thread
        # the tied iterations have different vectors: taking a later one is seen
        valid, vs = ar.hypotheses(case.pos1, case.pos2, case.corr, case.max_iterations, case.seed, case.pairs[0])
        for it in its[1:]:
            assert valid[it] and ac.ratio(ar.layout(vs[it]), g["v"], float(g["kappa"])) > 1e3 * ac.TAU


def test_every_refit_regime_occurs():
    g = {name: ac.load(name)[1] for name in ac.FULL}
    best = {name: int(x["count_ref"][x["winner"]]) for name, x in g.items()}
    assert g["refit_larger"]["refit_accepted"] and g["refit_larger"]["refit_count"] > best["refit_larger"]
    assert g["refit_equal"]["refit_accepted"] and g["refit_equal"]["refit_count"] == best["refit_equal"]
    assert g["refit_rejected"]["refit_ran"] and not g["refit_rejected"]["refit_accepted"]
    assert g["refit_rejected"]["refit_count"] < best["refit_rejected"] == 230
    assert not g["refit_off"]["refit_ran"] and best["refit_off"] == best["refit_larger"]
    assert not g["k_4"]["refit_ran"] and best["k_4"] == 4 and not g["k_5"]["refit_ran"] and best["k_5"] == 4


# ---------------------------------------------------------------------------
# the restatement against the reference
# ---------------------------------------------------------------------------
_ratios, _ratios_r = {}, {}


@pytest.mark.parametrize("name", ac.SINGLE + ac.FULL)
def test_restatement_meets_the_reference(name):
    case, g = ac.load(name)
    res = _restated(name)
    bad, worst, worst_r = ac.check(name, res)
    _ratios[name], _ratios_r[name] = worst, worst_r
    print(f"\n[affine restatement] {name:18s} largest ratio {worst:.4f}, refit {worst_r:.4f}")
    assert not bad, bad
    if case.kind != "single":
        d = {}
        ar.run(case.pos1, case.pos2, case.corr, case.max_iterations, case.threshold, case.seed, case.pairs[0], case.refit, detail=d)
        assert d["valid"].all() and np.array_equal(d["counts"], g["count_ref"]) and int(np.argmax(d["counts"])) == g["winner"]
        n, inl, _, rec = res[0]
        accepted = bool(g["refit_ran"]) and bool(g["refit_accepted"])
        clear = ac.mask(g["refit_clear"] if accepted else g["clear"], case.k)
        assert n == clear.sum() and np.array_equal(inl, np.nonzero(clear)[0])
        if g["refit_ran"] and not accepted:
            # a rejected refit is not in the result: its vector and its count are held here
            r = ac.ratio(ar.layout(d["refit"]), g["refit_v"], float(g["refit_cond"]))
            _ratios_r[name] = r
            assert r <= ac.TAU_R
            assert int(ar.below(d["refit"], *case.matches(), case.threshold).sum()) == g["refit_count"]


def test_tau_is_set_from_the_measured_ratios():
    for name in ac.SINGLE + ac.FULL:
        if name not in _ratios:                      # run alone or in another order: measured here
            test_restatement_meets_the_reference(name)
    worst, worst_r = max(_ratios.values()), max(_ratios_r.values())
    print(f"\n[affine restatement] largest ratio {worst:.4f} (recorded {ac.MEASURED_RATIO}), TAU {ac.TAU}; refit {worst_r:.4f} "
          f"(recorded {ac.MEASURED_RATIO_R}), TAU_R {ac.TAU_R}")
    # every hypothesis and every refit was measured for the recorded ratios, the winners are a part
    assert worst <= ac.MEASURED_RATIO and worst_r <= ac.MEASURED_RATIO_R
    assert ac.TAU == 2.0 ** math.floor(math.log2(4.0 * ac.MEASURED_RATIO) + 1)
    assert ac.TAU_R == 2.0 ** math.floor(math.log2(4.0 * ac.MEASURED_RATIO_R) + 1)
    # flat in kappa: the scenes at kappa 1e5 and more need no more than the benign ones
    assert max(_ratios[n] for n in ("near_planar_1e-4", "scale_1e-4")) <= _ratios["edge_1"]


def test_degenerate_inputs_are_pinned():
    case, _ = ac.load("identical_views")
    d = {}
    n, inl, F, rec = ar.run(case.pos1, case.pos2, case.corr, case.max_iterations, case.threshold, case.seed, case.pairs[0], True, detail=d)
    # x2 = x1, y2 = y1: two equal columns; the samples that survive the pivots give c = -a, d = -b, e = 0, all matches
    assert 0 < d["valid"].sum() < case.max_iterations and (d["counts"][d["valid"]] == case.k).all()
    assert n == case.k and np.array_equal(inl, np.arange(case.k))
    v = ac.vector(F)
    assert abs(v[0] + v[2]) < 1e-9 and abs(v[1] + v[3]) < 1e-9 and abs(v[4]) < 1e-9
    case, _ = ac.load("one_point")
    d = {}
    n, inl, F, rec = ar.run(case.pos1, case.pos2, case.corr, case.max_iterations, case.threshold, case.seed, case.pairs[0], True, detail=d)
    assert not d["valid"].any() and n == 0 and inl.size == 0 and not F.any() and rec["best_iteration"] == -1
    n, inl, F, rec = _restated("twins")[0]
    assert n > 0.6 * ac.load("twins")[0].k and rec["refit_ran"] == 1
    # at_threshold: the match's n^2 / s IS thr^2 in the kernel's arithmetic, and it is left out
    case, _ = ac.load("at_threshold")
    n, inl, F, rec = _restated("at_threshold")[0]
    a, b, c, dd, e = ac.vector(F)
    m1, m2 = case.matches()
    q = ((m2[:, 0] * a + m2[:, 1] * b) + ((m1[:, 0] * c + m1[:, 1] * dd) + e)) ** 2 / (((a * a + b * b) + c * c) + dd * dd)
    i = ac.AT_THRESHOLD[2]
    assert q[i] == case.threshold * case.threshold and i not in inl and n == ac.AT_THRESHOLD_COUNT == (q < q[i]).sum()
    assert (q <= q[i]).sum() == n + 1


# ---------------------------------------------------------------------------
# power: a restatement with one fault fails
# ---------------------------------------------------------------------------
POWER_CASES = ("benign", "near_planar_1e-4", "iters_513", "tie_part1", "tie_both", "tie_thread", "tie_slot", "refit_larger",
               "refit_equal", "refit_rejected", "at_threshold")


def _passes(name, **faults):
    res = _restated(name, **faults)
    if ac.load(name)[0].kind == "twin":
        return _equal(res, _restated(name))
    return not ac.check(name, res)[0]


def _caught(**faults):
    return {name for name in POWER_CASES if not _passes(name, **faults)}


def test_without_a_fault_every_power_case_passes():
    assert not _caught()


def test_planted_F_transposed():
    assert {"benign", "near_planar_1e-4", "iters_513"} <= _caught(transpose=True)


def test_planted_non_strict_threshold():
    """n^2 / s <= thr^2.  A match with equality lies in every band, so no reference can see this one: it is caught where
    the restatement is pinned, on the case whose threshold squares to a match's distance."""
    assert "at_threshold" in _caught(le=True)


def test_planted_threshold_not_squared():
    assert {"benign", "iters_513"} <= _caught(squared=False)


def test_planted_non_strict_replacement():
    """count >= best: a later tied hypothesis replaces the first."""
    assert {"tie_part1", "tie_both", "tie_thread", "tie_slot"} <= _caught(replace_equal=True)


def test_planted_largest_eigenvector():
    assert {"refit_larger", "refit_equal"} <= _caught(largest=True)


def test_planted_mean_not_subtracted():
    assert {"refit_larger", "refit_equal"} <= _caught(keep_mean=True)


# ---------------------------------------------------------------------------
# quality and pipeline, with the two CPU implementations
# ---------------------------------------------------------------------------

def test_planted_inliers_found():
    """The share of planted inliers in the winner's list at 1000 iterations, affine restatement against the 8-point twin:
    never below, and the seeds of the 0.75 rows satisfy the two caps the GPU test asserts."""
    print("\n| outlier share | noise px | 8-point recall (inliers) | affine recall (inliers) |\n|---|---|---|---|")
    for share in ac.QUALITY_SHARES:
        for noise in ac.QUALITY_NOISE_PX:
            seed = ac.QUALITY_SEEDS[(share, noise)]
            pos1, pos2, corr, planted = ac.quality_scene(share, noise, seed)
            assert corr.shape[0] == ac.QUALITY_MATCHES and planted.sum() == ac.QUALITY_MATCHES - int(share * ac.QUALITY_MATCHES)
            n, inl, _, _ = ar.run(pos1, pos2, corr, 1000, ac.THR, seed, 0, True)
            fn, finl, _ = oracle_lib.oracle_ransac(pos1, pos2, corr, 1000, ac.THR, seed, 0)
            ra, rf = ac.recall(inl, planted), ac.recall(finl, planted)
            print(f"| {share:.2f} | {noise:.2f} | {rf:.3f} ({fn}) | {ra:.3f} ({n}) |")
            assert ra >= rf, (share, noise)
            if share == 0.75:
                assert ra >= 0.9 and rf <= 0.6, (share, noise, ra, rf)


def test_pipeline_set_satisfies_the_comparison():
    """The set of the GPU pipeline test: with the oracle matcher's lists, the 8-point twin and the affine restatement, the
    surviving correspondences between different landmarks are no more and those between equal landmarks no fewer in
    affine mode."""
    iset = ac.pipeline_set()
    empty = np.zeros((0, 64), np.int16)
    lists = {"fundamental": [], "affine": []}
    for a in range(iset.num_views):
        for b in range(a):
            e12, _ = oracle_lib.oracle_pairwise_match(iset.sift[a], empty, iset.sift[b], empty)
            idx = np.nonzero(e12 >= 0)[0]
            corr = np.stack([idx, e12[idx]], axis=1).astype(np.int32)
            if corr.shape[0] < 50:
                continue
            pid, pa, pb = a * (a - 1) // 2 + b, ac.normalised(iset, a), ac.normalised(iset, b)
            fn, finl, _ = oracle_lib.oracle_ransac(pa, pb, corr, 1000, ac.THR, 0, pid)
            an, ainl, _, _ = ar.run(pa, pb, corr, 1000, ac.THR, 0, pid)
            if fn >= 30:
                lists["fundamental"].append((a, b, corr[finl]))
            if an >= 30:
                lists["affine"].append((a, b, corr[ainl]))
    f, a = ac.landmark_counts(iset, lists["fundamental"]), ac.landmark_counts(iset, lists["affine"])
    print(f"\n[affine pipeline] (equal, different) landmarks: 8-point {f}, affine {a}")
    assert a[1] <= f[1] and a[0] >= f[0] and f[1] > 0
