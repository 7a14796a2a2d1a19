"""The restatement of osfm_match_guided (tests/guided_restatement.py) on the cases of tests/guided_cases.py, without a
GPU: every planted fault shows on some case; with the band open, no seeds and no cap the restatement is the plain
two-way match of the oracle (an anchor that shares no code with the band or the seeds); and the twin set's figures."""
import numpy as np
import pytest

import affine_restatement as A
import guided_cases as GC
import guided_restatement as G
from oracle_lib import oracle_matcher, oracle_pairwise_match

FAULTS = ("le", "seeds_in_play", "earlier_wins", "cap_lt", "transpose", "drop_surf_offset")


def run_case(c, **faults):
    return G.run(c.view1, c.view2, c.seeds, c.F, **c.options, **faults)


@pytest.fixture(scope="module")
def results():
    cs = [c for c in GC.cases() if c.view1.n <= 600 and c.view2.n <= 600]
    return cs, [run_case(c) for c in cs]


def same(a, b):
    return (a["status"], a["num_added"], a["max_candidates"]) == (b["status"], b["num_added"], b["max_candidates"]) and \
        np.array_equal(a["list"], b["list"]) and a["F"].tobytes() == b["F"].tobytes()


def test_cases_cover_their_ground(results):
    cs, rs = results
    by = {c.name: r for c, r in zip(cs, rs)}
    assert by["edge"]["list"].tolist() == [[1, 1], [4, 4]]                 # one step inside, on either side
    P = GC.DEFAULT_LIMITS[2]
    assert by["counts"]["max_candidates"] == P + 1 and by["counts"]["num_added"] >= 8
    assert by["counts_all"]["max_candidates"] == 2 * P + 3 and by["counts_all"]["num_added"] == 3
    assert by["ties_ratio1"]["list"].tolist() == [[0, 3]]                   # the later duplicate
    assert by["ties_default"]["num_added"] == 0                             # second == best
    assert by["ties_zero"]["list"].tolist() == [[0, 1]]                     # 0 / 0 accepted
    assert by["too_few"]["status"] == G.TOO_FEW and by["zero_F"]["status"] == G.DEGENERATE
    assert np.array_equal(by["too_few"]["list"], [c for c in cs if c.name == "too_few"][0].seeds)
    assert by["cap_on"]["list"].tolist() == [[0, 0], [1, 1]] and by["cap_off"]["list"].tolist() == [[0, 0], [1, 1], [2, 2]]
    assert by["types_cap_sift_seeds_only"]["num_added"] > 0
    c = [c for c in cs if c.name == "types_cap_sift_seeds_only"][0]
    added = by[c.name]["list"]
    assert (added[:, 0] < c.view1.sift.shape[0]).all()                      # SURF has no seeds: it adds nothing
    assert by["types_both"]["num_added"] > 0 and (by["types_both"]["list"][:, 0] >= [c for c in cs if c.name == "types_both"][0].view1.sift.shape[0]).any()
    assert by["wrap"]["num_added"] > 0 and by["surf_wrap"]["num_added"] > 0 and by["peaky"]["num_added"] > 0


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_shows(results, fault):
    cs, rs = results
    hit = [c.name for c, r in zip(cs, rs) if not same(r, run_case(c, **{fault: True}))]
    print(fault, "changes", hit)
    assert hit, f"no case notices the fault {fault}"


def test_in_order_rule_decides_the_wrap_case():
    """the wrap case's answer is not that of a scan in another order: its products do not fit T"""
    c = GC.wrap_case()
    nn = oracle_matcher()
    q, el = c.view1.sift[0], c.view2.sift
    fwd, rev = nn.nn_find(q, el), nn.nn_find(q, el[::-1].copy())
    assert (int(fwd[0]), int(el.shape[0] - 1 - rev[2])) != (int(rev[0]), int(fwd[2]))


@pytest.mark.parametrize("with_surf", [False, True])
def test_open_band_is_the_plain_two_way_match(with_surf):
    """Threshold so large that every feature is a candidate, no seeds, no cap: the list is the oracle's pairwise_match
    (twoway + remove_inconsistent + combine) of the same views."""
    iset = GC.synth.make_image_set(2, 150, seed=8, twin_frac=0.3, visibility=0.7, n_surf=60 if with_surf else 0)
    rng = np.random.default_rng(8)
    views = []
    for v in range(2):
        pos = GC.norm_pos(iset, v)
        if with_surf:
            pos = np.concatenate([pos, rng.uniform(-0.4, 0.4, (iset.surf[v].shape[0], 2)).astype(np.float32)])
        views.append(G.View(iset.sift[v], iset.surf[v] if with_surf else None, pos))
    r = G.run(views[1], views[0], np.zeros((0, 2), np.int32), GC.layout(a=1.0, c=-1.0), threshold=10.0, cap_from_seeds=False)
    m12, _ = oracle_pairwise_match(iset.sift[1], iset.surf[1], iset.sift[0], iset.surf[0])
    want = np.array([(i, j) for i, j in enumerate(np.asarray(m12).tolist()) if j >= 0], np.int32).reshape(-1, 2)
    assert r["status"] == G.OK and r["max_candidates"] == max(views[0].sift.shape[0], views[1].sift.shape[0])
    assert want.shape[0] > 40
    assert np.array_equal(r["list"], want)


def verified_seeds(iset, v1, v2, pair_id):
    """the oracle's mutual matches, then the affine RANSAC's restatement: (seeds, plain mutual matches)"""
    m12, _ = oracle_pairwise_match(iset.sift[v1], iset.surf[v1], iset.sift[v2], iset.surf[v2])
    corr = np.array([(i, j) for i, j in enumerate(np.asarray(m12).tolist()) if j >= 0], np.int32).reshape(-1, 2)
    n, inl, _, _ = A.run(GC.norm_pos(iset, v1), GC.norm_pos(iset, v2), corr, pair_id=pair_id)
    return corr[inl], corr


def twin_figures(twin_frac):
    iset = GC.image_set(**dict(GC.TWIN, twin_frac=twin_frac))
    rows = []
    for v1, v2 in ((1, 0), (2, 0), (2, 1)):
        seeds, corr = verified_seeds(iset, v1, v2, v1 * (v1 - 1) // 2 + v2)
        r = G.run(G.View(iset.sift[v1], None, GC.norm_pos(iset, v1)), G.View(iset.sift[v2], None, GC.norm_pos(iset, v2)), seeds)
        taken = set(map(tuple, seeds.tolist()))
        added = np.array([p for p in r["list"].tolist() if tuple(p) not in taken], np.int64).reshape(-1, 2)
        true = int((iset.landmark[v1][added[:, 0]] == iset.landmark[v2][added[:, 1]]).sum()) if added.size else 0
        rows.append((v1, v2, corr.shape[0], seeds.shape[0], added.shape[0], true, r["max_candidates"]))
        print(f"twin_frac {twin_frac} pair {v1},{v2}: mutual {corr.shape[0]} seeds {seeds.shape[0]} added {added.shape[0]} "
              f"true {true} max candidates {r['max_candidates']}")
    return rows


def test_twin_set_share_of_true_additions():
    """Seeds that are the affine RANSAC's inliers (not the truth): at least 0.9 of the additions over the three pairs join
    two features of one landmark, and every pair gets at least one.  Set: synth.make_image_set(3, 400, seed=11,
    twin_frac=0.5, visibility=0.6), the issue's own."""
    rows = twin_figures(0.5)
    assert all(r[4] >= 1 for r in rows)
    assert sum(r[5] for r in rows) >= 0.9 * sum(r[4] for r in rows)


def test_set_without_twins_adds_next_to_nothing():
    rows = twin_figures(0.0)
    assert all(r[4] <= 2 for r in rows)
