"""osfm_build_groups where the kernels of groups_api.hip change path and on ties, on tests/group_cases.py: every case
through groups.build_groups_flat, group size 3 once on the incremental form and once on the general path
(OSFM_GROUPS_GENERAL), sizes 4..8 on the general path.  Integer work: groups and counts are compared for equality
with the host model, which tests/test_group_cases_cpu.py ties to oracle/groups_oracle.c and shows to reach each edge.
Every case also asserts, from the library's result alone, what it was chosen for.

The refusals go through the C entry itself, with the status and *num_groups asserted: OSFM_E_ARG leaves *num_groups
as the caller set it; OSFM_E_CAPACITY and OSFM_E_STATE leave the groups found until then and their number.  Where
the product refuses and the oracle does not (two views; id 0 unassigned while nothing scores; a view twice in a
track) both sides are asserted, so the difference is a recorded decision.

Found by case dry5 (group size 5, the first group dry at its second step): group_score_kernel indexed the bitsets
with the -1 that the step before had left in the seed; such a seed now stays without a pick.

Which tests fail under a mistake of the kind they are for.  Each mistake (a comparison or a value, never an index,
a bound or a launch shape) was built once into a copy of the library, and this file, tests/test_groups_gpu.py and
test_e2e_gpu.py::test_incremental_group_builder_matches_the_oracle ("e2e") were run against it on an MI355X.  [x] is
test_case_against_the_model[x-incremental] or [x-general], whichever path the mistake is on; "late" etc. are
test_refused_case.
  `row[c] > bs` as `>=` in group3_select_kernel      [w1] [v64] [v4t] [v24t] [v33t] [v33u] [v65t] [v65u] [tie12] [tie34]
                                                     [tie66] [ones] [big262], empty / late / isolated / id0 (a group
                                                     with 0 tracks instead of the refusal), a view twice.
                                                     Before: test_unreachable_view_is_reported and e2e
  `~order` as `order` in the key (and its decoding)  [w1] [v4] [v23] [v24] [v32] [v33] [v64] [v65] [outside] [short], every
                                                     twin and tie case, [big262], late, capacity.  Before:
                                                     test_groups_match_oracle[20-6000-3-4], test_shuffled_view_ids..., e2e
  `oi < s_idx[tid]` as `>` in group_score_kernel     [w1] [v64] [g7one] [g8one], every twin and tie case on the general path,
                                                     [g4v12t] [g5v12t] [g6v14t] [g8v12t] [big262], late.  Before: none
  `acc > my_best` as `>=` in the same kernel         [big262-general] alone (candidates 1 and 257, one thread's two
                                                     strides).  Before: none
  one-word tail of group3_score_rows_kernel left out every case of group size 3 but [w8192] (W = 128 has no tail), late,
                                                     id0, capacity.  Before: four of test_groups_gpu.py and e2e
  `acc1` not added                                   [w4097] [w8192] [w8193] [w12289] [w16385].  Before:
                                                     test_groups_match_oracle[20-6000-3-4] (W = 94) and e2e
  `c0` fixed at 0                                    [v33] [v64] [v65] [v33t] [v33u] [v65t] [v65u] [tie34] [tie66] [big262].
                                                     Before: test_scale_500_views (coverage) and e2e
  the `(int)cand == assigned` refresh dropped        every word and tie case, every view case from V = 23, [outside]
                                                     [short] [big262], late, capacity.  Before: six tests.  (The copy
                                                     also refused a pick that was already used, which would have
                                                     paired a view with itself past the score rows.)
  the cache's "pick has been assigned" test dropped  every case on the general path with more than two groups.
                                                     Before: test_groups_match_oracle[9-1500-4-3] alone
So the suite before this file was blind to both tie rules of the general path's kernel, and saw those of the
incremental form only through the refusal test and the e2e case's one random 40-view scene.

The host model's result for big262, the one case left to it, was compared once with oracle/groups_oracle.c as
well (equal; 480 s, which is why no test does it).

Measured on MI355X: the 90 tests of this file run in 2.4 s together; the two of big262 take 0.6 s each (the host
model's 260 iterations included), every other one below 0.3 s.
"""
import ctypes as C

import numpy as np
import pytest

import group_cases as GC
import oracle_lib

pytestmark = pytest.mark.gpu

SENTINEL = -77
RUNS = [(c.name, p) for c in GC.CASES if not c.refused
        for p in (("incremental", "general") if c.group_size == 3 else ("general",))]
REFUSED = [(c.name, p) for c in GC.CASES if c.refused
           for p in (("incremental", "general") if c.group_size == 3 else ("general",))]


def _path(monkeypatch, path):
    if path == "general":
        monkeypatch.setenv("OSFM_GROUPS_GENERAL", "1")
    else:
        monkeypatch.delenv("OSFM_GROUPS_GENERAL", raising=False)


def _build(name):
    from orthosfm_amd import groups as G
    ids, offs, views = GC.build(name)
    got = G.build_groups_flat(ids, offs, views, GC.BY_NAME[name].group_size)
    return [g.ids for g in got], [g.tracks for g in got]


def _raw(ids, offs, views, group_size, max_groups=None):
    """The C entry itself: (status, *num_groups, groups, counts); *num_groups starts as SENTINEL."""
    from orthosfm_amd import capi
    ids = np.ascontiguousarray(ids, np.int32)
    offs = np.ascontiguousarray(offs, np.int64)
    views = np.ascontiguousarray(views, np.int32)
    if views.size == 0:
        views = np.zeros(1, np.int32)
    cap = max(len(ids), 1)
    groups = np.full((cap, max(group_size, 1)), SENTINEL, np.int32)
    counts = np.full(cap, SENTINEL, np.int32)
    n = C.c_int32(SENTINEL)
    st = capi.lib.osfm_build_groups(0, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)), len(offs) - 1,
                                    offs.ctypes.data_as(C.POINTER(C.c_int64)), views.ctypes.data_as(C.POINTER(C.c_int32)),
                                    group_size, cap if max_groups is None else max_groups,
                                    groups.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                    C.byref(n))
    return st, n.value, groups, counts


def _tracks_holding(name, group):
    _, offs, views = GC.build(name)
    want = set(group)
    return sum(want <= set(views[offs[t]:offs[t + 1]].tolist()) for t in range(len(offs) - 1))


def _assert_chosen_for(name, groups, counts):
    """What the case is in the table for, from the library's result alone."""
    c = GC.BY_NAME[name]
    ids = [int(v) for v in GC.build(name)[0]]
    assert groups[0][:2] == ids[:2]
    assert all(len(g) == c.group_size for g in groups)
    assert sorted({v for g in groups for v in g}) == sorted(ids)
    ranks = [GC.rank_of(name, g[-1]) for g in groups]
    if c.kind == "words":                       # every word of the three bitsets counted: the first and last groups'
        assert counts[0] == _tracks_holding(name, groups[0])       # counts recounted from the track list
        assert counts[-1] == _tracks_holding(name, groups[-1])
    if name.startswith("v33"):
        assert max(ranks) >= 32                 # a pick from the second 32-candidate chunk
    if name.startswith("v65"):
        assert max(ranks) >= 64 and any(32 <= r < 64 for r in ranks)
    if name in ("v23", "v24"):
        assert len(groups) == len(ids) - 2      # 253 / 276 seed pairs: one / two blocks of the selection
    if name == "ones":
        assert counts == [1] * 6
        assert groups[0] == [31, 4, 2]          # all six candidates tie: the smallest id
    if name == "v33t":
        assert GC.rank_of(name, groups[[r in (31, 32) for r in ranks].index(True)][-1]) == 31
    if name == "v65t":
        assert GC.rank_of(name, groups[[r in (63, 64) for r in ranks].index(True)][-1]) == 63
    if c.kind == "sizes" and name.endswith("one"):
        assert len(groups) == 1 and counts == [_tracks_holding(name, ids)]
    if c.kind == "sizes" and not name.endswith("one"):
        assert len(groups) >= 5 and counts[-1] == _tracks_holding(name, groups[-1])
    if name == "big262":                        # candidates 3 | 256 and, two groups on, 1 | 257 tie: the lower one
        assert ranks[0] == 3 and ranks[1] == 258 and ranks[2] == 1 and ranks[3] == 261
        assert counts[:4] == [90, 90, 70, 70]
    if name in ("outside", "short"):
        assert len(groups) == len(ids) - 2 and counts[0] == _tracks_holding(name, groups[0])


@pytest.mark.parametrize("name,path", RUNS)
def test_case_against_the_model(name, path, monkeypatch):
    _path(monkeypatch, path)
    status, want_groups, want_counts = GC.product_expectation(GC.expected(name))
    assert status == GC.OK
    groups, counts = _build(name)
    print(name, path, len(groups), "groups; first", groups[0], counts[0], "last", groups[-1], counts[-1])
    _assert_chosen_for(name, groups, counts)
    assert groups == want_groups
    assert counts == want_counts
    if GC.BY_NAME[name].kind == "ties":         # nothing is left to the order in which the device gets there
        assert _build(name) == (groups, counts)


@pytest.mark.parametrize("name,path", REFUSED)
def test_refused_case(name, path, monkeypatch):
    """OSFM_E_STATE where a pick scores 0, with the groups found until then: no track at all, a view that shares only
    pairs (found after six groups), first views that share no track with a third, the first group of a size-5 run
    dry at its second step, and -- unlike the reference, which appends bestViewID's start value -- id 0 unassigned
    while nothing scores."""
    from orthosfm_amd import capi, groups as G
    _path(monkeypatch, path)
    ids, offs, views = GC.build(name)
    gs = GC.BY_NAME[name].group_size
    status, want_groups, want_counts = GC.product_expectation(GC.expected(name))
    assert status == GC.E_STATE == capi.E_STATE
    st, n, groups, counts = _raw(ids, offs, views, gs)
    assert st == capi.E_STATE and n == len(want_groups)
    assert groups[:n].tolist() == want_groups and counts[:n].tolist() == want_counts
    assert (groups[n + 1:] == SENTINEL).all() and (counts[n:] == SENTINEL).all()      # row n may be begun
    with pytest.raises(capi.OsfmError) as e:
        G.build_groups_flat(ids, offs, views, gs)
    assert e.value.status == capi.E_STATE
    if name == "id0":                           # the recorded difference: the oracle goes on with id 0
        want = oracle_lib.oracle_build_groups(ids, offs, views, 3)
        assert want[0].tolist() == [[4, 7, 9], [4, 7, 0]] and want[1].tolist() == [2, 0]
        assert groups[:n].tolist() == want[0][:1].tolist()


@pytest.mark.parametrize("path", ["incremental", "general"])
def test_two_views_are_refused(path, monkeypatch):
    """The oracle, like the reference, returns the one group [v0, v1, 0] with 0 tracks; the product refuses."""
    from orthosfm_amd import capi
    _path(monkeypatch, path)
    ids, (offs, views) = np.array([7, 3], np.int32), GC.flatten([[7, 3], [3, 7, 5]])
    want = oracle_lib.oracle_build_groups(ids, offs, views, 3)
    assert want[0].tolist() == [[7, 3, 0]] and want[1].tolist() == [0]
    st, n, groups, _ = _raw(ids, offs, views, 3)
    assert st == capi.E_STATE and n == 0 and (groups == SENTINEL).all()
    assert "two views" in capi.last_error()


@pytest.mark.parametrize("path", ["incremental", "general"])
def test_a_view_held_twice_counts_once(path, monkeypatch):
    """Outside the precondition: the oracle counts features, so [1, 1, 2] is a full track of {1, 2, 4} to it; the
    bitsets hold a track once per view, nothing scores, and the call is refused."""
    from orthosfm_amd import capi
    _path(monkeypatch, path)
    ids, (offs, views) = np.array([1, 2, 4], np.int32), GC.flatten([[1, 1, 2]])
    want = oracle_lib.oracle_build_groups(ids, offs, views, 3)
    assert want[0].tolist() == [[1, 2, 4]] and want[1].tolist() == [1]
    st, n, _, _ = _raw(ids, offs, views, 3)
    assert st == capi.E_STATE and n == 0


def test_argument_refusals_leave_num_groups_alone():
    from orthosfm_amd import capi
    ids, offs, views = GC.build("v4")
    assert _raw(ids, offs, views, 3)[:2] == (capi.OK, 2)
    for bad_ids, gs in (([5, 9, 5, 2], 3), (ids, 2), (ids, 9), (ids[:1], 3), (ids[:0], 3)):
        st, n, groups, counts = _raw(np.array(bad_ids, np.int32), offs, views, gs)
        assert st == capi.E_ARG and n == SENTINEL, (bad_ids, gs)
        assert (groups == SENTINEL).all() and (counts == SENTINEL).all()


@pytest.mark.parametrize("path", ["incremental", "general"])
def test_capacity_one_short(path, monkeypatch):
    """max_groups = 20 for the 21 groups of v23: the first 20 are written, then OSFM_E_CAPACITY."""
    from orthosfm_amd import capi
    _path(monkeypatch, path)
    ids, offs, views = GC.build("v23")
    res = GC.expected("v23")
    assert len(res.groups) == 21
    st, n, groups, counts = _raw(ids, offs, views, 3, max_groups=20)
    assert st == capi.E_CAPACITY and n == 20
    assert groups[:20].tolist() == res.groups[:20] and counts[:20].tolist() == res.counts[:20]
    assert (groups[20:] == SENTINEL).all() and (counts[20:] == SENTINEL).all()
    st, n, groups, counts = _raw(ids, offs, views, 3, max_groups=21)
    assert st == capi.OK and n == 21 and groups[:21].tolist() == res.groups
