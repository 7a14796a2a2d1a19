"""The RANSAC-F check of tests/ransac_cases.py without a device: the golden is what the generator gives today, the
inputs keep what the cases promise (nothing is decided inside a band, ties lie where the kernel's split puts them), the
twin -- oracle_ransac_fundamental, plain double arithmetic in the kernel's order -- meets the independent reference on
every constrained case, and a twin with one fault of the kind a kernel could have fails on the case made for it."""
import math

import numpy as np
import pytest

import oracle_lib
import ransac_cases as rc


def _twin(name):
    case, _ = rc.load(name)
    return [oracle_lib.oracle_ransac(case.pos1, case.pos2, case.corr, case.max_iterations, case.threshold, case.seed, p)
            for p in case.pairs]


# ---------------------------------------------------------------------------
# golden and inputs
# ---------------------------------------------------------------------------

def test_golden_is_current():
    pytest.importorskip("mpmath")
    for name in ("k_8", "k_9", "iters_1", "iters_2"):
        case, g = rc.load(name)
        ref = rc.reference(case)
        for f in ("count_ref", "amb", "uncon", "winner", "F", "A", "clear", "ambm"):
            assert np.asarray(ref[f]).tobytes() == g[f].tobytes(), (name, f)
    for name in rc.SINGLE:
        case, g = rc.load(name)
        m1, m2 = case.matches()
        for j in (0, 63):
            idx = rc.sample8(case.seed, case.pairs[j], 0, case.k)
            h = rc.hypothesis(m1[idx], m2[idx])
            assert h["uncon"] == g["uncon"][j] and h["F"].tobytes() == g["F"][j].tobytes() and h["A"] == g["A"][j], (name, j)
            if not h["uncon"]:
                clear, amb = rc.classify(h["F"], h["A"], m1, m2, case.threshold)
                assert np.array_equal(clear, rc.mask(g["clear"][j], case.k)) and np.array_equal(amb, rc.mask(g["ambm"][j], case.k))


def test_sample_stream():
    """The Python restatement of ransac_rand.h draws what the twin draws: a k = 8 run can only return the eight
    matches' own hypothesis, and for a larger k the winner's sample reproduces the twin's F."""
    assert rc.sample8(3, 5, 7, 8) == list(range(8))
    case, g = rc.load("k_65")
    m1, m2 = case.matches()
    n, _, F = _twin("k_65")[0]
    idx = rc.sample8(case.seed, case.pairs[0], int(g["winner"]), case.k)
    assert len(set(idx)) == 8 and idx == sorted(idx) and max(idx) < 65
    ok, Fs = oracle_lib.oracle_fundamental_8_point(m1[idx], m2[idx])
    assert ok and np.array_equal(Fs, F)


@pytest.mark.parametrize("name", rc.FULL + ("twins",))
def test_nothing_is_decided_inside_a_band(name):
    case, g = rc.load(name)
    un = g["uncon"].astype(bool)
    assert g["count_ref"].size == case.max_iterations
    best = int(g["count_ref"][~un].max())
    w = int(g["winner"])
    assert (best > 0 or name == "k_8") and g["count_ref"][w] == best and not un[w] and (g["count_ref"][:w][~un[:w]] < best).all()
    near = g["count_ref"] + g["amb"] >= best
    assert (g["amb"][near & ~un] == 0).all(), (name, np.nonzero(near & (g["amb"] > 0))[0])
    if name == "twins":
        # a sample with a copy: no F to compare with; the twin's own counts of these lie below the best
        assert 0 < un.sum() < 60 and g["uncon_below_best"] == 1 and g["twin_uncon_max"] < best
        _, counts, _ = rc.twin_run(case, case.pairs[0])
        assert counts[un].max() == g["twin_uncon_max"]
    else:
        assert not un[near].any(), (name, np.nonzero(near & un)[0])
    assert not rc.mask(g["ambm"], case.k).any()
    assert rc.mask(g["clear"], case.k).sum() == best


@pytest.mark.parametrize("name", rc.SINGLE)
def test_single_hypothesis_scenes_are_constrained(name):
    case, g = rc.load(name)
    assert case.k == 400 and case.max_iterations == 1 and len(case.pairs) == 64
    assert g["uncon"].sum() <= 2
    assert g["amb"].sum() <= 64 * case.k // 1000
    ok = g["uncon"] == 0
    samples = {tuple(rc.sample8(case.seed, p, 0, case.k)) for p in case.pairs}
    assert len(samples) == 64
    print(f"\n[ransac cases] {name:18s} kappa {g['kappa'][ok].min():.1e} .. {g['kappa'][ok].max():.1e}, smallest gap "
          f"{g['gap'][ok].min():.1e}, counts {g['count_ref'][ok].min()} .. {g['count_ref'][ok].max()}")


def test_what_the_cases_promise():
    m1, m2 = rc.load("edge_1")[0].matches()
    for m in (m1, m2):
        assert np.abs(m).max() == 1.0 and (np.abs(m) == 1.0).sum() >= 4
    m1, m2 = rc.load("scale_1e-4")[0].matches()
    assert max(np.abs(m1).max(), np.abs(m2).max()) < 1e-4
    # kappa grows with 1 / relief (by 92 for 100 in the median)
    k2 = np.median(rc.load("near_planar_1e-2")[1]["kappa"])
    k4 = np.median(rc.load("near_planar_1e-4")[1]["kappa"])
    assert k2 > 1e4 and 30 < k4 / k2 < 300, (k2, k4)
    assert [rc.load(f"k_{k}")[0].k for k in rc.K_LIST] == list(rc.K_LIST)
    assert rc.K_LIST == (8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2048, 2049, 2500)
    assert rc.ITER_LIST == (1, 2, 256, 257, 511, 512, 513, 1000, 1024, 1025)
    for n in rc.ITER_LIST:
        case, g = rc.load(f"iters_{n}")
        assert case.k == 700 and case.max_iterations == n
        # prefixes of one run: the counts of a shorter run are those of the longer one
        assert np.array_equal(g["count_ref"], rc.load("iters_1025")[1]["count_ref"][:n])
    assert rc.part_of(512, 513) == (1, 0, 0, 0) and rc.part_of(511, 512)[0] == 0
    assert rc.part_of(512, 1025) == (0, 1, 0, 0) and rc.part_of(1024, 1025) == (1, 0, 0, 0)
    # mixed chunks: chunk 1 alone holds coordinates outside [-1, 1]
    case, _ = rc.load("mixed_chunks")
    m = np.abs(np.concatenate(case.matches(), axis=1)).max(axis=1)
    wide = np.nonzero(m > 1.0)[0]
    assert case.k == 2500 and sorted(wide) == [1500, 2047] and sorted(m[wide]) == [np.nextafter(np.float32(1), np.float32(2)), 1.5]
    # degenerate inputs
    case, _ = rc.load("identical_views")
    m1, m2 = case.matches()
    assert case.k == 600 and np.array_equal(m1, m2) and np.array_equal(m1 * 1024, np.round(m1 * 1024))
    case, _ = rc.load("one_point")
    m1, m2 = case.matches()
    assert case.k == 20 and len({tuple(r) for r in np.concatenate([m1, m2])}) == 1
    case, _ = rc.load("twins")
    both = np.concatenate(case.matches(), axis=1)
    assert case.k == 1200 and 1200 - len({tuple(r) for r in both}) == 360


def test_ties_lie_where_the_kernel_splits():
    for name in rc.TIES:
        case, g = rc.load(name)
        m1, m2 = case.matches()
        best = g["count_ref"].max()
        its = np.nonzero(g["count_ref"] == best)[0]
        assert its.size >= 2 and its[0] == g["winner"]
        where = [rc.part_of(int(i), case.max_iterations) for i in its]
        if name == "tie_part1":
            assert all(w[0] == 1 for w in where)
        elif name == "tie_both":
            assert where[0][0] == 0 and any(w[0] == 1 for w in where)
        else:
            a, b = where[0], where[1]
            assert a[:2] == b[:2] and its[0] < its[1] and a[2] > b[2]        # same part and pass, the higher thread first
        # the tied iterations have different F: taking a later one is seen
        Fs = []
        for it in its:
            idx = rc.sample8(case.seed, case.pairs[0], int(it), case.k)
            ok, F = oracle_lib.oracle_fundamental_8_point(m1[idx], m2[idx])
            assert ok
            Fs.append(F)
        for F in Fs[1:]:
            assert rc.ratio(F, g["F"], float(g["A"])) > 1e3 * rc.TAU


# ---------------------------------------------------------------------------
# the twin against the reference
# ---------------------------------------------------------------------------
_ratios = {}


@pytest.mark.parametrize("name", rc.SINGLE + rc.FULL + ("twins",))
def test_twin_meets_the_reference(name):
    case, g = rc.load(name)
    res = _twin(name)
    bad, worst = rc.check(name, res)
    _ratios[name] = worst
    print(f"\n[ransac twin] {name:18s} largest ratio {worst:.4f}")
    assert not bad, bad
    if case.kind != "single":
        # the same winner: the first iteration whose count reaches the largest, by the twin's own counts
        valid, counts, py = rc.twin_run(case, case.pairs[0])
        un = g["uncon"].astype(bool)
        assert np.array_equal(counts[~un], g["count_ref"][~un]) and valid[~un].all()
        assert int(np.argmax(counts)) == g["winner"]
        # ... and the restated loop is the twin
        assert py[0] == res[0][0] and np.array_equal(py[1], res[0][1]) and np.array_equal(py[2], res[0][2])
        assert res[0][0] == g["count_ref"][g["winner"]] and np.array_equal(res[0][1], np.nonzero(rc.mask(g["clear"], case.k))[0])


def test_tau_is_set_from_the_measured_ratio():
    missing = [n for n in rc.SINGLE + rc.FULL + ("twins",) if n not in _ratios]
    if missing:
        pytest.skip("needs test_twin_meets_the_reference of every case in the same run")
    worst = max(_ratios.values())
    print(f"\n[ransac twin] largest ratio over the cases {worst:.4f} (recorded {rc.TWIN_RATIO}), TAU {rc.TAU}")
    assert worst <= rc.TWIN_RATIO                                # every hypothesis was measured for TWIN_RATIO, these are a part
    assert rc.TAU == 2.0 ** math.floor(math.log2(4.0 * rc.TWIN_RATIO) + 1)
    # flat in kappa: the scenes at kappa 1e7 and more need no more than the benign ones' few tenths
    assert max(_ratios[n] for n in ("near_planar_1e-4", "scale_1e-4")) <= rc.TWIN_RATIO


def test_degenerate_inputs_are_pinned():
    case, _ = rc.load("identical_views")
    valid, counts, _ = rc.twin_run(case, case.pairs[0])
    assert int((~valid).sum()) == rc.IDENTICAL_REFUSED                  # of 1000 hypotheses
    assert (counts[valid] == case.k).all()
    n, inl, F = _twin("identical_views")[0]
    assert n == case.k and np.array_equal(inl, np.arange(case.k)) and np.abs(F + F.T).max() < 1e-12
    case, _ = rc.load("one_point")
    valid, counts, _ = rc.twin_run(case, case.pairs[0])
    assert not valid.any()
    n, inl, F = _twin("one_point")[0]
    assert n == 0 and inl.size == 0 and not F.any()
    # at_threshold: the match's distance IS thr^2 in the twin's arithmetic, and it is left out
    case, _ = rc.load("at_threshold")
    n, inl, F = _twin("at_threshold")[0]
    d = rc.sampson(F, *case.matches())
    i = rc.AT_THRESHOLD[2]
    assert d[i] == case.threshold * case.threshold and i not in inl and n == rc.AT_THRESHOLD_COUNT == (d < d[i]).sum()
    assert (d <= d[i]).sum() == n + 1


# ---------------------------------------------------------------------------
# power: a twin with one fault fails
# ---------------------------------------------------------------------------

def _eig3(A):
    """eig3 of ransac_oracle.c, operation by operation."""
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(30):
        if abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2]) == 0.0:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if A[p][q] == 0.0:
                    continue
                th = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if th >= 0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return V, [A[i][i] for i in range(3)]


def _eight_point(p1, p2, largest=False):
    """oracle_fundamental_8_point restated in Python floats (IEEE double, one rounding per operation);
    largest: the rank-2 step removes the LARGEST singular direction."""
    A = [[float(v) for v in row] for row in rc.system(np.asarray(p1), np.asarray(p2))]
    perm = list(range(9))
    for r in range(8):
        best, pr, pc = -1.0, r, r
        for i in range(r, 8):
            for j in range(r, 9):
                if abs(A[i][j]) > best:
                    best, pr, pc = abs(A[i][j]), i, j
        if not best > 0.0:
            return 0, np.zeros((3, 3))
        A[r], A[pr] = A[pr], A[r]
        if pc != r:
            for row in A:
                row[r], row[pc] = row[pc], row[r]
            perm[r], perm[pc] = perm[pc], perm[r]
        inv = 1.0 / A[r][r]
        for j in range(r, 9):
            A[r][j] *= inv
        for i in range(8):
            if i != r:
                fct = A[i][r]
                for j in range(r, 9):
                    A[i][j] -= fct * A[r][j]
    f, n2 = [0.0] * 9, 1.0
    for r in range(8):
        f[perm[r]] = -A[r][8]
        n2 += A[r][8] * A[r][8]
    f[perm[8]] = 1.0
    invn = 1.0 / math.sqrt(n2)
    f = [v * invn for v in f]
    M = [[f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j] for j in range(3)] for i in range(3)]
    V, w = _eig3(M)
    m = 0
    if largest:
        if w[1] > w[m]:
            m = 1
        if w[2] > w[m]:
            m = 2
    else:
        if w[1] < w[m]:
            m = 1
        if w[2] < w[m]:
            m = 2
    v3 = [V[0][m], V[1][m], V[2][m]]
    F = np.zeros(9)
    for r in range(3):
        fv = f[3 * r] * v3[0] + f[3 * r + 1] * v3[1] + f[3 * r + 2] * v3[2]
        for c in range(3):
            F[3 * r + c] = f[3 * r + c] - fv * v3[c]
    return 1, F.reshape(3, 3)


def _restated(name, **kw):
    """The results of the restated twin (with a fault, if any) on a case, and whether they pass the case's check."""
    case, _ = rc.load(name)
    kw.setdefault("eight_point", _eight_point)
    res = [rc.twin_run(case, p, **kw)[2] for p in case.pairs]
    if case.kind == "twin":
        ref = _twin(name)
        ok = all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(res, ref))
    else:
        ok = not rc.check(name, res)[0]
    return res, ok


POWER_CASES = ("benign", "near_planar_1e-4", "iters_513", "tie_part1", "tie_both", "tie_thread", "at_threshold")


def test_restated_twin_is_the_twin():
    for name in POWER_CASES:
        res, ok = _restated(name)
        assert ok, name
        for a, b in zip(res, _twin(name)):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), name


def _caught(**kw):
    return [name for name in POWER_CASES if not _restated(name, **kw)[1]]


def test_planted_F_transposed():
    assert {"benign", "near_planar_1e-4", "iters_513"} <= set(_caught(transpose=True))


def test_planted_non_strict_replacement():
    """count >= best: a later tied hypothesis replaces the first."""
    assert {"tie_part1", "tie_both", "tie_thread"} <= set(_caught(replace=lambda count, best: count >= best and count > 0))


def test_planted_non_strict_threshold():
    """d <= thr^2.  A match with d == thr^2 lies in every band around thr^2, so no reference can see this one: it is
    caught where the twin is pinned, on the case whose threshold squares to a match's distance."""
    assert "at_threshold" in _caught(below=lambda d, thr: d <= thr * thr)


def test_planted_threshold_not_squared():
    """The threshold compared against d itself: d < thr."""
    assert {"benign", "iters_513"} <= set(_caught(below=lambda d, thr: d < thr))


def test_planted_largest_direction_removed():
    assert {"benign", "near_planar_1e-4", "iters_513"} <= set(_caught(eight_point=lambda a, b: _eight_point(a, b, largest=True)))
