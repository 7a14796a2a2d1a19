"""The group-builder cases (tests/group_cases.py) are fit to judge a kernel.  No GPU: every number here comes from the
host model or from oracle/groups_oracle.c, never from the library under test.

The model is compared with the literal oracle on every case but group_cases.MODEL_ONLY (big262: 262 views, where the
oracle's V^3 T passes take minutes).  Then each case is shown to reach what it was made for: the tie cases tie (and
the opposite rule changes their result), the word cases depend on their last word, the view cases on their last
candidate chunk, big262 ties across the two strides of the general path's candidate loop.  If a case misses a
condition the case changes, never the condition.  The three inputs on which the product deliberately differs from
the literal restatement are pinned here as what the oracle returns."""
import numpy as np
import pytest

import group_cases as GC
import oracle_lib


def _oracle(name):
    ids, offs, views = GC.build(name)
    return oracle_lib.oracle_build_groups(ids, offs, views, GC.BY_NAME[name].group_size)


def _changed(a, b):
    return (a.groups, a.counts, a.ok) != (b.groups, b.counts, b.ok)


@pytest.mark.parametrize("name", GC.ORACLE_CASES)
def test_model_equals_oracle(name):
    res, want = GC.expected(name), _oracle(name)
    print(name, "groups", len(res.groups), "iterations", res.iterations, "tied seeds", res.tied_seed_iterations,
          "tied picks", res.tied_pick_iterations, "zero at", res.zero_at)
    if want is None:
        assert not res.ok                                   # the literal loop makes no progress
    else:
        assert res.ok
        assert res.groups == [list(map(int, g)) for g in want[0]]
        assert res.counts == list(map(int, want[1]))


def test_only_the_262_view_case_is_left_to_the_model():
    assert GC.MODEL_ONLY == ["big262"]
    assert len(GC.build("big262")[0]) == 262


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_what_the_product_is_expected_to_answer(name):
    c, res = GC.BY_NAME[name], GC.expected(name)
    status, groups, counts = GC.product_expectation(res)
    assert (status == GC.E_STATE) == c.refused
    if not c.refused:
        ids = GC.build(name)[0]
        assert groups[0][:2] == [int(ids[0]), int(ids[1])]
        assert sorted({v for g in groups for v in g}) == sorted(int(v) for v in ids)
        if c.group_size == 3:
            assert len(groups) == len(ids) - 2                  # one view per group after the first
        assert min(counts) > 0
    else:
        assert len(groups) == {"empty": 0, "late": 6, "isolated": 0, "id0": 1, "dry5": 0}[name]


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.TIE_CASES)
def test_tie_cases_tie(name):
    res = GC.expected(name)
    print(name, res.iterations, res.tied_seed_iterations, res.tied_pick_iterations)
    assert 4 * res.tied_seed_iterations >= res.iterations
    assert 4 * res.tied_pick_iterations >= res.iterations


@pytest.mark.parametrize("name", GC.TIE_CASES)
@pytest.mark.parametrize("rule", ["largest id among candidates", "last seed among seeds"])
def test_the_opposite_rule_changes_the_result(name, rule):
    ids, offs, views = GC.build(name)
    kw = {"cand_rule": "max"} if rule.startswith("largest") else {"seed_rule": "last"}
    assert _changed(GC.host_model(ids, offs, views, 3, **kw), GC.expected(name))


@pytest.mark.parametrize("name", ["tie12", "tie34", "tie66", "v33t", "v65t"])
def test_smaller_twin_at_the_larger_index(name):
    """Among the tied picks there is a pair whose smaller id comes later in view_ids, and one the other way round."""
    ids = [int(v) for v in GC.build(name)[0]]
    later, earlier = 0, 0
    for s in GC.expected(name).steps:
        if len(s.tied_ids) >= 2:
            a, b = s.tied_ids[0], s.tied_ids[1]
            assert a < b
            later += ids.index(a) > ids.index(b)
            earlier += ids.index(a) < ids.index(b)
    assert later >= 1 and earlier >= 1


# ---------------------------------------------------------------------------
# words
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.WORD_CASES)
def test_word_cases_depend_on_their_last_words(name):
    ids, offs, views = GC.build(name)
    T = len(offs) - 1
    W = (T + 63) // 64
    assert W == {1: 1, 64: 1, 65: 2, 4096: 64, 4097: 65, 8192: 128, 8193: 129, 12289: 193, 16385: 257}[T]
    full = GC.expected(name)
    for first_word in [W - 1] + [w for w in (64, 128) if w < W]:
        keep = np.arange(T) < 64 * first_word
        assert _changed(GC.host_model(ids, offs, views, 3, keep=keep), full), first_word


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------
def _pick_ranks(name):
    return [GC.rank_of(name, g[-1]) for g in GC.expected(name).groups]


@pytest.mark.parametrize("name,chunks", [("v33", 2), ("v33t", 2), ("v33u", 2), ("v65", 3), ("v65t", 3), ("v65u", 3)])
def test_view_cases_pick_from_every_candidate_chunk(name, chunks):
    ranks = _pick_ranks(name)
    for ch in range(chunks):
        assert any(r // 32 == ch for r in ranks), ch


@pytest.mark.parametrize("name,pair", [("v33t", (31, 32)), ("v33u", (3, 32)), ("v65t", (63, 64)), ("v65u", (5, 64)),
                                       ("v65t", (31, 33)), ("v65u", (20, 40))])
def test_twins_either_side_of_a_chunk_edge_tie(name, pair):
    """The winning pick is tied between the two twins of `pair` (ranks), which fall in different 32-candidate chunks."""
    assert pair[0] // 32 != pair[1] // 32
    hit = [s for s in GC.expected(name).steps if tuple(GC.rank_of(name, v) for v in s.tied_ids) == pair]
    assert len(hit) == 1


@pytest.mark.parametrize("name", [c.name for c in GC.CASES if c.kind == "views"])
def test_first_views_are_not_the_lowest_ids(name):
    ids = GC.build(name)[0]
    assert sorted(GC.rank_of(name, int(v)) for v in ids[:2]) != [0, 1]


def test_pair_count_crosses_a_block_between_23_and_24_views():
    assert 23 * 22 // 2 <= 256 < 24 * 23 // 2


# ---------------------------------------------------------------------------
# the general path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [4, 5, 6, 7, 8])
def test_one_group_cases(gs):
    """V = group size: one group, its count the number of tracks that hold all views (the last step's score)."""
    name = f"g{gs}one"
    ids, offs, views = GC.build(name)
    res = GC.expected(name)
    full = sum(set(int(v) for v in ids) <= set(int(v) for v in views[offs[t]:offs[t + 1]]) for t in range(len(offs) - 1))
    assert len(res.groups) == 1 and sorted(res.groups[0]) == sorted(int(v) for v in ids)
    assert res.counts == [full] and full >= 1
    assert res.groups[0][2:] != sorted(res.groups[0][2:])           # the greedy order is not the id order


@pytest.mark.parametrize("name", [c.name for c in GC.CASES if c.kind == "sizes" and not c.name.endswith("one")])
def test_size_cases_take_several_iterations(name):
    res = GC.expected(name)
    assert len(res.groups) >= 5
    if name.endswith("t"):
        assert res.tied_seed_iterations >= 2 and res.tied_pick_iterations >= 2


def test_big262_ties_across_the_two_strides():
    """While more than 256 candidates remain: one winning pick tied between a thread's first and second stride
    (candidates i and i + 256), one between different threads' strides; the smaller index is the documented pick."""
    steps = [s for s in GC.expected("big262").steps if s.remaining > 256 and len(s.tied) == 2]
    same = [s for s in steps if s.tied[1] - s.tied[0] == 256]
    other = [s for s in steps if s.tied[0] < 256 <= s.tied[1] and (s.tied[1] - s.tied[0]) % 256]
    assert len(same) >= 1 and len(other) >= 1
    assert all(s.pick == s.tied[0] for s in same + other)
    ids, offs, views = GC.build("big262")
    assert _changed(GC.host_model(ids, offs, views, 3, cand_rule="max"), GC.expected("big262"))


# ---------------------------------------------------------------------------
# where the product deliberately differs from the literal restatement
# ---------------------------------------------------------------------------
def test_oracle_two_views_give_one_group_with_id_0():
    want = oracle_lib.oracle_build_groups(np.array([7, 3]), *GC.flatten([[7, 3], [3, 7, 5]]), 3)
    assert want[0].tolist() == [[7, 3, 0]] and want[1].tolist() == [0]


def test_oracle_appends_id_0_when_nothing_scores_and_0_is_unassigned():
    want = _oracle("id0")
    assert want[0].tolist() == [[4, 7, 9], [4, 7, 0]] and want[1].tolist() == [2, 0]
    res = GC.expected("id0")
    assert res.ok and res.zero_at == 1                      # the product refuses where the 0 is appended


def test_oracle_counts_a_view_held_twice_as_two_features():
    """[1, 1, 2] counts as a full track of {1, 2, 4} in the oracle (three features of the group's views); as a set of
    views it holds two.  Such tracks are removed before the group builder runs."""
    ids, (offs, views) = np.array([1, 2, 4]), GC.flatten([[1, 1, 2]])
    want = oracle_lib.oracle_build_groups(ids, offs, views, 3)
    assert want[0].tolist() == [[1, 2, 4]] and want[1].tolist() == [1]
    res = GC.host_model(ids, offs, views, 3)
    assert res.zero_at == 0 and GC.product_expectation(res) == (GC.E_STATE, [], [])


def test_no_case_holds_a_view_twice_in_a_track():
    for c in GC.CASES:
        _, offs, views = GC.build(c.name)
        for t in range(len(offs) - 1):
            tr = views[offs[t]:offs[t + 1]]
            assert len(set(tr.tolist())) == len(tr), (c.name, t)
