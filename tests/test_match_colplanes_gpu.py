"""The column partials as two planes (best keys, second keys): the tile kernels store a partial as one
entry of each plane, the finish kernel streams the best plane in batches of sixteen row blocks and gathers
a single second key per column, the winning row block's.  Every list against the CPU oracle, exactly.

The inputs plant columns whose outcome hangs on that one gathered key or on the fold of the bests:
  same   the two best rows of the column lie in ONE row block, in different waves (64-row strips): the second
         is seen only through the second plane, at the winning block, at the column's own entry;
  cross  the two best rows lie in different row blocks: the loser's best arrives through the fold;
  tie    two row blocks hold equal bests for the column: the equal best of the one that does not win must still
         arrive as the second, or the column passes the ratio test;
  nan    the same with both distances 0, a tie that IS accepted (0 / 0): the finish hands such a column to the
         sequential-scan kernel, which reports the later row like the reference.  (Which block the merge itself
         lets win a tie never reaches the lists: a tied column is rejected or handed over.  What can be seen is
         that the hand-over fires: MatchStats.exact_scan_queries.)
In `same` and `cross` the column fails the ratio test because of its second best row and would pass it
against anything else; verify() asserts that on the CPU with the oracle's own distances before any list
is compared, so a change of the generators cannot empty a case unnoticed.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import match_cases
import oracle_lib
from orthosfm_amd import synth

pytestmark = pytest.mark.gpu

ROWS = 256          # rows per row block of the tile kernels
STRIP = 64          # rows per wave
# row-block counts 1, 8, 9, 16, 17, 18: below, at and one past the finish kernel's batches of 8 / 16 row blocks
N1 = (200, 2048, 2049, 4096, 4097, 4400)
N2 = (130, 1000)    # not multiples of 64; the planes' row stride (n2 rounded up to 1024) exceeds n2


@pytest.fixture(scope="module")
def hm():
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    assert capi.device_count() >= 1, "no HIP device"
    return HipExhaustiveMatching


def _weaken(d, delta):
    """A copy of d whose inner product with d is lower by delta (or up to max |d| more): entries moved
    toward zero one unit at a time, largest first, round after round."""
    r = d.astype(np.int64)
    order = np.argsort(-np.abs(r), kind="stable")
    left, k = int(delta), 0
    while left > 0:
        i = order[k % order.size]
        if r[i] != 0:
            r[i] -= np.sign(r[i])
            left -= abs(int(d[i]))
        k += 1
    return r.astype(d.dtype)


class _Rows:
    """Hands out unused rows of set 1 by (row block, wave)."""

    def __init__(self, n1):
        self.n1, self.used = n1, set()

    def pick(self, block, wave=None):
        lo = block * ROWS + (0 if wave is None else wave * STRIP)
        hi = min(self.n1, block * ROWS + (ROWS if wave is None else (wave + 1) * STRIP))
        for r in range(lo + 5, hi):
            if r not in self.used:
                self.used.add(r)
                return r
        for r in range(lo, min(lo + 5, hi)):
            if r not in self.used:
                self.used.add(r)
                return r
        return None


def _plant(s1, s2, surf):
    """Overwrites columns of s2 and rows of s1 (in place) with fresh descriptors and near copies of them; returns the plants as
    dicts {kind, q, r1, r2}: r1 the row that must win, r2 the second (for ties: r1 the earlier row)."""
    n1, n2 = s1.shape[0], s2.shape[0]
    nrb = (n1 + ROWS - 1) // ROWS
    last = nrb - 1
    # inner product lost by the winner / by the second: distances 2 * (that), ratio 0.71, above lowe^2 (0.64 / 0.49)
    d_win, d_sec = (750, 1050) if surf else (3000, 4200)
    # The planted columns are fresh descriptors (nearly every column of the generated pair has a near copy among
    # the rows), kept only where the best row so far lies far below what is planted.
    r = np.random.default_rng(n1 * 131 + n2)
    if surf:
        fresh = synth.quantize_surf(synth.surf_like(r.standard_normal((32, 64)))).reshape(32, 64)
    else:
        fresh = synth.quantize_sift(synth.sift_like(r.standard_normal((32, 128)))).reshape(32, 128)
    fresh = fresh.astype(s2.dtype)
    far = (s1.astype(np.int64) @ fresh.astype(np.int64).T).max(axis=0) < (fresh.astype(np.int64) ** 2).sum(axis=1) - 2 * d_sec
    fresh = iter(fresh[far])
    places = iter((7 + 11 * k) % n2 for k in range(32))       # distinct: 11 divides neither 130 nor 1000

    def column():
        q = next(places)
        s2[q] = next(fresh)
        return q

    rows = _Rows(n1)
    plants = []

    def rows_in(b):
        return min(ROWS, n1 - b * ROWS)

    # same block, different waves: first block, the blocks on both sides of the batch edges, last block
    wave_pairs = [(0, 1), (3, 0), (1, 2), (2, 3), (1, 0), (0, 3)]
    for k, b in enumerate(sorted({x for x in (0, 7, 8, 15, 16, last) if x < nrb and rows_in(x) > STRIP})):
        nw = (rows_in(b) + STRIP - 1) // STRIP
        w1, w2 = wave_pairs[k][0] % nw, wave_pairs[k][1] % nw
        if w1 == w2:
            w1, w2 = 0, 1
        q = column()
        r1, r2 = rows.pick(b, w1), rows.pick(b, w2)
        s1[r1], s1[r2] = _weaken(s2[q], d_win), _weaken(s2[q], d_sec)
        plants.append(dict(kind="same", q=q, r1=r1, r2=r2))
    # different blocks, winner before and behind the second, across the batch edges
    seen = set()
    for a, b in [(last, 0), (0, last), (7, 8), (8, 7), (15, 16), (16, 15), (0, 7), (7, 0), (8, 15), (15, 8)]:
        if a >= nrb or b >= nrb or a == b or (a, b) in seen:
            continue
        seen.add((a, b))
        r1 = rows.pick(a)
        r2 = rows.pick(b) if r1 is not None else None
        if r1 is None or r2 is None:      # a last block of one row is used up
            continue
        q = column()
        s1[r1], s1[r2] = _weaken(s2[q], d_win), _weaken(s2[q], d_sec)
        plants.append(dict(kind="cross", q=q, r1=r1, r2=r2))
    # equal bests in two blocks
    seen = set()
    for a, b in [(0, last), (7, 8), (15, 16), (0, 7)]:
        if b >= nrb or a == b or (a, b) in seen:
            continue
        seen.add((a, b))
        r1 = rows.pick(a)
        r2 = rows.pick(b) if r1 is not None else None
        if r1 is None or r2 is None:
            continue
        q = column()
        s1[r1] = s1[r2] = _weaken(s2[q], d_win)
        plants.append(dict(kind="tie", q=q, r1=r1, r2=r2))
    # ... and with distance 0 on both (an inner product at the clamp): accepted although tied
    if nrb > 1:
        r1, r2 = rows.pick(0), rows.pick(1)
        if r1 is not None and r2 is not None:
            q = next(places)
            d = np.zeros(s2.shape[1], s2.dtype)
            if surf:
                d[0] = 127                       # 16129, the SURF clamp
            else:
                d[:4], d[4] = 127, 23            # 65045: over the SIFT clamp of 65025, inside 16 bits
            s2[q] = s1[r1] = s1[r2] = d
            plants.append(dict(kind="nan", q=q, r1=r1, r2=r2))
    return plants


def verify(s1, s2, plants, lowe):
    """The planted columns have the property they are there for, by the oracle's nearest-neighbour search."""
    om = oracle_lib.oracle_matcher()
    sq = np.float32(lowe) * np.float32(lowe)

    def ratio(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32(a) / np.float32(b)

    for p in plants:
        q, r1, r2 = p["q"], p["r1"], p["r2"]
        d1, d2, i1, i2 = (int(x) for x in om.nn_find(s2[q], s1))
        hidden = s1.copy()
        if p["kind"] in ("same", "cross", "special"):
            assert (i1, i2) == (r1, r2), p
            assert ratio(d1, d2) > sq, p                          # rejected when the second is seen
            hidden[r2] = 0
            e1, e2, j1, _ = (int(x) for x in om.nn_find(s2[q], hidden))
            assert j1 == r1 and ratio(e1, e2) <= sq, p            # accepted when it is not: the rest lies far below
            if p["kind"] == "same":
                assert r1 // ROWS == r2 // ROWS and (r1 % ROWS) // STRIP != (r2 % ROWS) // STRIP, p
            elif p["kind"] == "cross":
                assert r1 // ROWS != r2 // ROWS, p
        else:
            assert r2 // ROWS > r1 // ROWS, p
            assert (i1, i2) == (r2, r1) and d1 == d2, p           # the later row wins the tie
            if p["kind"] == "nan":
                assert d1 == 0, p                                 # 0 / 0: accepted
            else:
                assert d1 > 0, p
                hidden[r1] = 0
                e1, e2, j1, _ = (int(x) for x in om.nn_find(s2[q], hidden))
                assert j1 == r2 and ratio(e1, e2) <= sq, p


def _kinds(plants):
    return {p["kind"] for p in plants}


@functools.lru_cache(maxsize=None)
def sift_case(n1, n2):
    s1, s2 = match_cases.sift_pair(n1, n2, min(n1, n2) // 2, 7000 + n1 + n2)
    assert int(max(s1.max(), s2.max())) <= 127          # ordinary descriptors only: the correction-free kernel
    plants = _plant(s1, s2, surf=False)
    verify(s1, s2, plants, 0.8)
    assert "same" in _kinds(plants)
    assert n1 <= ROWS or {"cross", "tie", "nan"} <= _kinds(plants)
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2, plants


@functools.lru_cache(maxsize=None)
def surf_case(n1, n2):
    u1, u2 = match_cases.surf_pair(n1, n2, min(n1, n2) // 2, 7100 + n1 + n2)
    plants = _plant(u1, u2, surf=True)
    verify(u1, u2, plants, 0.7)
    assert {"same", "cross", "tie", "nan"} <= _kinds(plants)
    u1.setflags(write=False)
    u2.setflags(write=False)
    return u1, u2, plants


@functools.lru_cache(maxsize=None)
def special_case(n1, n2):
    """sift_case with descriptors that have bytes above 127 in both views, and one more plant: a column whose
    two best rows are special rows 5 and 70 of set 1 (numbered in ascending row order): with the gathered
    special row blocks they are rows of different waves of the first special block."""
    b1, b2, plants = sift_case(n1, n2)
    s1, s2 = b1.copy(), b2.copy()
    r = np.random.default_rng(n1 + n2)
    taken = {p[k] for p in plants for k in ("r1", "r2")}
    rows = np.array(sorted(r.choice([i for i in range(n1) if i not in taken], 150, replace=False)))
    cols = r.choice([j for j in range(n2) if j not in {p["q"] for p in plants}], 41, replace=False)
    for s, ks in ((s1, rows), (s2, cols[1:])):
        for k in ks:          # peaky descriptors: far from every planted column
            s[k] = 0
            s[k, r.choice(128, 3, replace=False)] = [int(r.integers(128, 256)), int(r.integers(0, 90)), int(r.integers(0, 60))]
    q = int(cols[0])
    lift = int(np.argmin(s2[q]))                        # lifted over 127 where the column has (next to) nothing
    for row, delta in ((rows[5], 3000), (rows[70], 4200)):
        s1[row] = _weaken(s2[q], delta)
        s1[row, lift] = 130
    extra = dict(kind="special", q=q, r1=int(rows[5]), r2=int(rows[70]))
    verify(s1, s2, plants + [extra], 0.8)
    return s1, s2


_NO_SURF = np.zeros((0, 64), np.int16)
_NO_SIFT = np.zeros((0, 128), np.uint16)


def check_pair(hm, s1, u1, s2, u2, options=None):
    """pairwise_match (raw tile kernels, cross-checked lists of both directions) and twoway_match of each
    descriptor type present (masked tile kernel, the lists before the cross-check) against the oracle."""
    m = hm(2, options=options) if options is not None else hm(2)
    m.set_view(0, s1, u1)
    m.set_view(1, s2, u2)
    got = m.pairwise_match(0, 1)
    handed = m.stats().exact_scan_queries           # queries of pairwise_match that went to the sequential scan
    two = [m.twoway_match(0, 1, t) for t in (0, 1)]
    m.close()
    e12, e21 = oracle_lib.oracle_pairwise_match(s1, u1, s2, u2)
    assert np.array_equal(got.matches_1_2, e12), "pairwise 1->2"
    assert np.array_equal(got.matches_2_1, e21), "pairwise 2->1"
    om = oracle_lib.oracle_matcher()
    for t, (a, b, lowe) in enumerate(((s1, s2, 0.8), (u1, u2, 0.7))):
        if a.shape[0] and b.shape[0]:
            t12, t21 = om.twoway(a, b, lowe)
            assert np.array_equal(two[t].matches_1_2, t12), ("twoway 1->2", t)
            assert np.array_equal(two[t].matches_2_1, t21), ("twoway 2->1", t)
    return e12, e21, handed


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


@pytest.mark.parametrize("n2", N2)
@pytest.mark.parametrize("n1", N1)
def test_sift_row_block_counts(hm, n1, n2):
    """Row-block counts around the batch edges of the finish kernel, columns short of a tile and of the stride."""
    s1, s2, plants = sift_case(n1, n2)
    e12, e21, handed = check_pair(hm, s1, _NO_SURF, s2, _NO_SURF)
    print(f"n1 {n1} n2 {n2}: {handed} queries handed to the sequential scan")
    for p in plants:            # what the oracle says about the plants (the lists above are equal to it)
        assert e21[p["q"]] == (p["r2"] if p["kind"] == "nan" else -1), p
    if "nan" in _kinds(plants):
        assert handed >= 1      # the accepted tie


def test_surf_signed_finish(hm):
    """D = 64 tile kernels and the signed finish, a small SIFT problem riding along."""
    u1, u2, _ = surf_case(2049, 130)
    s1, s2, _ = sift_case(200, 130)
    check_pair(hm, s1, u1, s2, u2)


def test_per_query_rescan(hm):
    """OSFM_FINISH_RESCAN=wave (read per batch): the finish without the bucketed rescoring reads the planes too."""
    s1, s2, _ = sift_case(4400, 1000)
    with _env("OSFM_FINISH_RESCAN", "wave"):
        check_pair(hm, s1, _NO_SURF, s2, _NO_SURF)


@pytest.mark.parametrize("special_kernel_max", [0, -1])
def test_descriptors_above_127(hm, special_kernel_max):
    """0 (default): the special descriptors go through match_special_kernel, the tile kernel sees them as blanks.
    -1: the per-view operand forms -- raw rows against corrected columns and gathered special row blocks on the
    keyed kernel, whose partials lie behind those of the main row blocks in both planes."""
    from orthosfm_amd import capi
    s1, s2 = special_case(2049, 1000)
    o = capi.default_match_options()
    o.special_kernel_max = special_kernel_max
    check_pair(hm, s1, _NO_SURF, s2, _NO_SURF, options=o)


def test_lowres_gate(hm):
    """The num_features-limited launch (masked kernel, rows and columns behind the limit are real descriptors
    that must not count): 600 of 2049 x 1000, a last row block of 88 rows."""
    nf = 600
    s1, s2, plants = sift_case(2049, 1000)
    inside = [p for p in plants if max(p["r1"], p["r2"]) < nf and p["q"] < nf]
    assert "same" in _kinds(inside)
    verify(s1[:nf], s2[:nf], inside, 0.8)
    m = hm(2)
    m.set_view(0, s1)
    m.set_view(1, s2)
    two = m.twoway_match(0, 1, 0, num_features=nf)
    count = m.pairwise_match_lowres(0, 1, nf)
    m.close()
    t12, t21 = oracle_lib.oracle_matcher().twoway(s1[:nf], s2[:nf], 0.8)
    assert np.array_equal(two.matches_1_2, t12) and np.array_equal(two.matches_2_1, t21)
    assert count == oracle_lib.oracle_pairwise_match_lowres(s1, _NO_SURF, s2, _NO_SURF, nf)
