"""The finish kernel's spans: a workgroup of 256 lanes owns 1024 consecutive queries of one problem and one
direction, a lane the queries j * 256 + threadIdx.x of the span in four turns (ballots of the rescans per turn), and
a column gathers its winner's second key only where its test can still pass against the fold's lower bound.  What
can go wrong: a turn or a span that straddles the end of the list, a span that holds a single query, turns past the
end that still run (or live ones that do not), a span wholly past the end of a small problem beside live spans of a
large one, and a column that passes because its second key was not fetched.  The same cases hold for a form with
four neighbouring queries per lane (tools/experiments/r10_finish_wide_fold.patch): last lanes with 3, 1 or 2 live ones.

The plants of test_match_fold_flight_gpu.py (fold_case: one row in the last row block, second bests on both sides of
a 16-block round's edge) at k in {0, 15, 16} and n2 below, at and above a turn's 256 columns and a span's 1024 (also
the planes' row stride), with 1027 and 2049 for a second / third span of three columns and of one.
verify() of test_match_colplanes_gpu.py asserts every plant's premise with the oracle before any list is compared;
every list is compared with the CPU oracle exactly.
"""
import functools

import numpy as np
import pytest

import match_cases
import oracle_lib
from test_match_colplanes_gpu import (ROWS, _NO_SIFT, _NO_SURF, _kinds, check_pair, hm, surf_case)  # noqa: F401
from test_match_fold_flight_gpu import fold_case

pytestmark = pytest.mark.gpu

KS = (0, 15, 16)
N2 = (61, 255, 256, 257, 1023, 1024, 1025, 1027, 2049)
ROW_N1 = (1, 1023, 1024, 1025, 4097)
RAGGED = ((1025, 61), (61, 1025), (257, 2049))


@pytest.mark.parametrize("n2", N2)
@pytest.mark.parametrize("k", KS)
def test_planted_columns(hm, k, n2):
    s1, s2, plants = fold_case(k, n2)
    if k == 0:
        assert plants == []                     # one row block (of one row): nothing to plant
    else:
        assert len(plants) == (11 if k == 15 else 15) and {"same", "cross", "tie", "nan"} <= _kinds(plants)
    e12, e21, handed = check_pair(hm, s1, _NO_SURF, s2, _NO_SURF)
    for p in plants:            # what the oracle says about the plants (the lists above are equal to it)
        if p["kind"] == "same":
            # only the gathered second key can fail this column: a finish that skips the gather where it may
            # not would report r1 here
            assert e21[p["q"]] == -1 and p["r1"] // ROWS == p["r2"] // ROWS, p
        assert e21[p["q"]] == (p["r2"] if p["kind"] == "nan" else -1), p
    if "nan" in _kinds(plants):
        assert handed >= 1      # the accepted tie


@functools.lru_cache(maxsize=None)
def row_case(n1):
    s1, s2 = match_cases.sift_pair(n1, 130, min(n1, 130) // 2, 9500 + n1)
    assert int(max(s1.max(), s2.max())) <= 127
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


@pytest.mark.parametrize("n1", ROW_N1)
def test_row_spans(hm, n1):
    """Row queries: one, one below, at and above a span, and a fifth span of one row."""
    s1, s2 = row_case(n1)
    e12, _, _ = check_pair(hm, s1, _NO_SURF, s2, _NO_SURF)
    if n1 > 1:
        assert (e12 >= 0).sum() > 10            # there are accepted rows to get wrong


@functools.lru_cache(maxsize=None)
def ragged_case():
    views, expect = [], []
    for k, (n1, n2) in enumerate(RAGGED):
        s1, s2 = match_cases.sift_pair(n1, n2, min(n1, n2) * 3 // 4, 9600 + k)
        e12, _ = oracle_lib.oracle_pairwise_match(s1, _NO_SURF, s2, _NO_SURF)
        idx = np.nonzero(e12 >= 0)[0]
        assert idx.size > 10, (n1, n2)
        views += [s1, s2]
        expect.append(np.stack([idx, e12[idx]], axis=1).astype(np.int32))
    return views, expect


def test_ragged_batch(hm):
    """One call, one finish launch sized by the largest list (2049: three spans per direction): spans past the end
    of a 61- or 257-query list lie beside the live spans of the 1025- and 2049-query ones."""
    from orthosfm_amd import capi
    views, expect = ragged_case()
    o = capi.default_match_options()
    o.use_lowres_matching = 0
    o.min_feature_matches = 0
    m = hm(len(views), options=o)
    for v, s in enumerate(views):
        m.set_view(v, s)
    pairs = [(2 * k, 2 * k + 1) for k in range(len(RAGGED))]
    out = m.compute(pairs=pairs)
    m.close()
    for tv, pair, e in zip(out, pairs, expect):
        assert (tv.view_1_id, tv.view_2_id) == pair and tv.status == capi.PAIR_MATCHED
        assert np.array_equal(np.asarray(tv.matches).reshape(-1, 2), e), pair


def test_surf_spans(hm):
    """The signed D = 64 instantiation through the spans: 9 row blocks, a second span of one column."""
    u1, u2, plants = surf_case(2049, 1025)
    _, e21, _ = check_pair(hm, _NO_SIFT, u1, _NO_SIFT, u2)
    for p in plants:
        assert e21[p["q"]] == (p["r2"] if p["kind"] == "nan" else -1), p


@functools.lru_cache(maxsize=None)
def special_pair():
    """2049 x 1025 with 150 rows and 40 columns that hold a byte above 127 (peaky descriptors, far from all others);
    eight of those columns are copies of eight of those rows, so that some special queries of both directions match
    (not all: peaky descriptors that share a peak are near each other too)."""
    s1, s2 = match_cases.sift_pair(2049, 1025, 500, 9700)
    r = np.random.default_rng(9701)
    rows = np.sort(r.choice(2049, 150, replace=False))
    cols = np.sort(r.choice(1025, 40, replace=False))
    for s, ks in ((s1, rows), (s2, cols)):
        for k in ks:
            s[k] = 0
            s[k, r.choice(128, 3, replace=False)] = [int(r.integers(128, 256)), int(r.integers(0, 90)), int(r.integers(0, 60))]
    twins = {int(c): int(w) for c, w in zip(cols[::5], rows[::19])}
    for c, w in twins.items():
        s2[c] = s1[w]
    e12, e21 = oracle_lib.oracle_matcher().twoway(s1, s2, 0.8)
    hit = sum(e21[c] == w and e12[w] == c for c, w in twins.items())
    assert hit >= 2, hit                            # special queries that are accepted, in both directions
    assert (e12 >= 0).sum() > 300
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


@pytest.mark.parametrize("special_kernel_max", [0, -1])
def test_special_rows_spans(hm, special_kernel_max):
    """Descriptors with bytes above 127 in both views.  0 (default): special queries take their state from
    match_special_kernel's partials, not from the lane's merge, and ordinary ones join the other set's special
    descriptors to theirs.  -1: special rows keep their row partials behind the main row blocks, away from the
    lane's 64 contiguous bytes."""
    from orthosfm_amd import capi
    s1, s2 = special_pair()
    o = capi.default_match_options()
    o.special_kernel_max = special_kernel_max
    check_pair(hm, s1, _NO_SURF, s2, _NO_SURF, options=o)
