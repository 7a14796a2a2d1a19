"""match_rescore_kernel with the next bucket in flight: while a bucket is scored, the candidates, corrections and
query rows of the next live bucket of the wave's run and the items of the one after it are already requested, and
the walk to the next problem runs two buckets ahead.  What can go wrong lies at the seams of that pipeline: a
problem's end or the switch from column to row buckets inside a wave's run of 16 buckets, a run with a single
live bucket (everything requested behind it belongs to no bucket), a short last run, a bucket whose further
query blocks are fetched the old way while nothing is in flight, a bucket filled past its capacity.

Every case compares the default path, OSFM_FINISH_RESCAN=wave (the per-query rescan) and the CPU oracle bit for
bit, and runs twice: the slot order inside a bucket comes from atomicAdd and differs between runs, the lists
must not.  The premise of a constructed case is asserted on the oracle's lists first.
"""
import numpy as np
import pytest

import match_cases
import oracle_lib
from test_match_colplanes_gpu import _weaken
from test_match_rescore_gpu import _both, _check_pair, hm  # noqa: F401

pytestmark = pytest.mark.gpu

STRIP = 64          # rows of a column-direction bucket
CAP0, CAP1 = 32, 64  # kRescoreCap0 / kRescoreCap1: queries a row- / column-direction bucket has room for


def _twice(hm, s1, s2):
    first = _check_pair(hm, s1, s2)
    again = _check_pair(hm, s1, s2, oracle=False)
    for x, y, name in zip(first, again, ("e12", "e21", "c12", "c21")):
        assert np.array_equal(x, y), ("second run", name)
    return first


def test_batch_of_four_small_pairs(hm):
    """Buckets per problem 4 nrb + 32 windows = 40, 72, 44, 40 -- 196 in all: problem ends at 40, 112 and 156 and
    the switches from column to row buckets at 8, 48, 124 and 164 fall inside runs of 16, the last run holds 4."""
    from orthosfm_amd import capi
    shapes = [(257, 1088), (300, 1089), (513, 700), (257, 65)]
    assert [4 * ((a + 255) // 256) + 32 * (((b + 63) // 64 + 16) // 17) for a, b in shapes] == [40, 72, 44, 40]
    views = []
    for k, (n1, n2) in enumerate(shapes):
        views += list(match_cases.sift_pair(n1, n2, min(n1, n2) * 3 // 4, 4100 + k))
    pairs = [(2 * k, 2 * k + 1) for k in range(len(shapes))]
    o = capi.default_match_options()
    o.use_lowres_matching = 0
    o.min_feature_matches = 0

    def run():
        m = hm(len(views), options=o)
        for v, s in enumerate(views):
            m.set_view(v, s)
        out = m.compute(pairs=pairs)
        res = [(tv.view_1_id, tv.view_2_id, tv.status, np.asarray(tv.matches).reshape(-1, 2).copy()) for tv in out]
        m.close()
        return res

    new, old = _both(run)
    again, _ = _both(run)
    none = np.zeros((0, 64), np.int16)
    for k, (a, b) in enumerate(pairs):
        for other, name in ((old, "per-query rescan"), (again, "second run")):
            assert new[k][:3] == other[k][:3] and np.array_equal(new[k][3], other[k][3]), (a, b, name)
        assert new[k][:2] == (a, b) and new[k][2] == capi.PAIR_MATCHED
        e12, _ = oracle_lib.oracle_pairwise_match(views[a], none, views[b], none)
        idx = np.nonzero(e12 >= 0)[0]
        assert idx.size > 20, (a, b)                      # there is something to rescore in every problem
        assert np.array_equal(new[k][3], np.stack([idx, e12[idx]], axis=1).astype(np.int32)), (a, b)


def _fails_everywhere(n, seed):
    """n SIFT rows (n even) in which every descriptor occurs twice: whatever is matched against them finds its
    best twice and fails the ratio test."""
    half, _ = match_cases.sift_pair(n // 2, 1, 0, seed)
    return np.concatenate([half, half])


def test_single_live_bucket(hm):
    """One bucket alone among empties: set 2 holds near copies of five rows of ONE 64-row strip of set 1, each
    twice; every other row of set 1 occurs twice.  Column queries are accepted only against those five rows, row
    queries never (every column has a twin).  The copies are weakened ones, at distance 6000: a copy at distance 0
    from both twins would be accepted (0 / 0) and handed to the sequential scan."""
    n1, strip0 = 1024, 256 + STRIP                          # the second strip of the second row block
    s1 = _fails_everywhere(n1, 501)
    rows = strip0 + np.array([3, 17, 31, 32, 60])
    fresh, _ = match_cases.sift_pair(rows.size, 1, 0, 502)
    s1[rows] = fresh                                        # unique rows (so are their former twins: nothing in set 2 is near those)
    near = np.stack([_weaken(s1[k], 3000) for k in rows])
    filler = np.stack([_weaken(s1[k], 3000) for k in range(27)])      # of rows that have a twin
    half = np.concatenate([near, filler])
    s2 = np.concatenate([half, half])                       # 64 columns, every one with a twin
    om = oracle_lib.oracle_matcher()
    e12, e21 = om.twoway(s1, s2, 0.8)
    hit = e21[e21 >= 0]
    assert hit.size == 2 * rows.size and set(hit.tolist()) == set(rows.tolist())    # one strip, nothing else
    assert (e12 >= 0).sum() == 0
    _twice(hm, s1, s2)


def _strip_copies(copies, seed):
    """test_duplicated_descriptors' construction at 3000 x 3000: `copies` columns of set 2 are noisy copies of
    set 1's rows 0 .. 31, whose best rows therefore all lie in the first 64-row strip."""
    r = np.random.default_rng(seed)
    s1, s2 = match_cases.sift_pair(3000, 3000, 1500, 1234)
    src = r.integers(0, 32, copies)
    noisy = s1[src].astype(np.int32) + r.integers(-2, 3, (copies, 128))
    s2[:copies] = np.clip(noisy, 0, 127).astype(np.uint16)
    return s1, s2


def _in_first_strip(s1, s2):
    _, e21 = oracle_lib.oracle_matcher().twoway(s1, s2, 0.8)
    return int(((e21 >= 0) & (e21 < STRIP)).sum())


def test_column_bucket_with_second_block(hm):
    """33 .. 64 accepted column queries in one strip (51 of the generated pair's own, and six copies): the bucket's
    second block of 32 queries runs."""
    s1, s2 = _strip_copies(6, 78)
    assert CAP0 + 1 <= _in_first_strip(s1, s2) <= CAP1
    _twice(hm, s1, s2)


def test_column_bucket_overflow(hm):
    """More than 64: the bucket is full, the rest goes through the per-query rescan."""
    s1, s2 = _strip_copies(200, 79)
    assert _in_first_strip(s1, s2) >= CAP1 + 1
    _twice(hm, s1, s2)


def test_row_bucket_overflow(hm):
    """A row-direction bucket (lane slot, window of starting tiles) filled past kRescoreCap0: 48 rows of set 1 are
    noisy copies of ONE column of set 2, so their winning groups are one group."""
    r = np.random.default_rng(80)
    s1, s2 = match_cases.sift_pair(3000, 3000, 1500, 1235)
    col = 1000 + 13
    rows = 300 + 7 * np.arange(48)
    noisy = s2[col].astype(np.int32)[None, :] + r.integers(-2, 3, (rows.size, 128))
    s1[rows] = np.clip(noisy, 0, 127).astype(np.uint16)
    e12, _ = oracle_lib.oracle_matcher().twoway(s1, s2, 0.8)
    assert int((e12 == col).sum()) >= CAP0 + 1
    _twice(hm, s1, s2)
