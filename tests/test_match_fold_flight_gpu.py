"""The column fold of the finish kernel at the seams of its rounds.  The fold walks the best-key plane sixteen row
blocks per round (loads issued together, folded in order, clamped repeats behind the last row block not folded);
a form that keeps the loads of the next round in flight while a round is folded (tools/experiments/
r09_fold_ring.patch, rounds of 16, or of 32 with a second buffer) has its seams at the same places.  What can go
wrong there is a block folded twice or never where two rounds meet, a refill that lands before its predecessor
was folded (the block 16 further on is then seen in its place), and the clamped loads behind the last row block.

The plants of test_match_colplanes_gpu.py at n1 = 256 k + 1 for k in {0, 15, 16, 31, 32, 33}: the last row block
holds one row, and one row block lies before and behind every edge of a 16- and of a 32-block round.  On top of
them, columns whose SECOND best row lies in the block a round ends with (15, 31) or in the one the next round
begins with (16, 32), the winner far away (block 0 or the last block) and right across the edge, and a tie
across the 31 | 32 edge.  n2 in {61, 64, 65, 1023, 1025}: fewer columns than a wave, a full and a started
second wave, one column below and one above a plane stride of 1024.  verify() of that file asserts every plant's
premise with the oracle on the CPU before any list is compared.
"""
import functools

import numpy as np
import pytest

import match_cases
from orthosfm_amd import synth
from test_match_colplanes_gpu import ROWS, _NO_SURF, _Rows, _kinds, _plant, _weaken, check_pair, hm, verify  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (0, 15, 16, 31, 32, 33)
N2 = (61, 64, 65, 1023, 1025)
EDGE_BLOCKS = (15, 16, 31, 32)     # a round's last block and the next round's first, rounds of 16 and of 32


def _plant_edges(s1, s2, plants):
    """More plants of the kinds of _plant (in place): the second best row in each block of EDGE_BLOCKS."""
    n1, n2 = s1.shape[0], s2.shape[0]
    nrb = (n1 + ROWS - 1) // ROWS
    last = nrb - 1
    d_win, d_sec = 3000, 4200
    r = np.random.default_rng(n1 * 977 + n2)
    fresh = synth.quantize_sift(synth.sift_like(r.standard_normal((48, 128)))).reshape(48, 128).astype(s2.dtype)
    far = (s1.astype(np.int64) @ fresh.astype(np.int64).T).max(axis=0) < (fresh.astype(np.int64) ** 2).sum(axis=1) - 2 * d_sec
    fresh = iter(fresh[far])
    taken = {p["q"] for p in plants}
    places = iter(q for q in ((3 + 7 * k) % n2 for k in range(n2)) if q not in taken)     # 7 divides no n2 of N2
    rows = _Rows(n1)
    rows.used |= {p[k] for p in plants for k in ("r1", "r2")}
    more = []

    def add(kind, a, b):
        if a >= nrb or b >= nrb or a == b:
            return
        r1 = rows.pick(a)
        r2 = rows.pick(b) if r1 is not None else None
        if r1 is None or r2 is None:          # the last block's single row is used up
            return
        q = next(places)
        s2[q] = next(fresh)
        if kind == "cross":
            s1[r1], s1[r2] = _weaken(s2[q], d_win), _weaken(s2[q], d_sec)
        else:
            s1[r1] = s1[r2] = _weaken(s2[q], d_win)
        more.append(dict(kind=kind, q=q, r1=r1, r2=r2))

    for b in EDGE_BLOCKS:
        add("cross", 0, b)                    # the winner leads from the first round on
        add("cross", last, b)                 # the winner arrives in the last round
    for a, b in ((31, 32), (32, 31), (16, 15), (15, 16)):
        add("cross", a, b)                    # winner and second on the two sides of an edge
    add("tie", 31, 32)
    return more


@functools.lru_cache(maxsize=None)
def fold_case(k, n2):
    n1 = ROWS * k + 1
    s1, s2 = match_cases.sift_pair(n1, n2, min(n1, n2) // 2, 9000 + n1 + n2)
    assert int(max(s1.max(), s2.max())) <= 127          # ordinary descriptors only
    plants = _plant(s1, s2, surf=False)
    plants = plants + _plant_edges(s1, s2, plants)
    verify(s1, s2, plants, 0.8)
    nrb = k + 1
    if nrb > 1:
        assert {"same", "cross", "tie", "nan"} <= _kinds(plants)
    # the second best in every edge block but a last one (its single row is the winner of a plant of _plant)
    second_blocks = {p["r2"] // ROWS for p in plants if p["kind"] == "cross"}
    assert {b for b in EDGE_BLOCKS if b < nrb - 1} <= second_blocks, (k, sorted(second_blocks))
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2, plants


@pytest.mark.parametrize("n2", N2)
@pytest.mark.parametrize("k", KS)
def test_fold_round_edges(hm, k, n2):
    s1, s2, plants = fold_case(k, n2)
    e12, e21, handed = check_pair(hm, s1, _NO_SURF, s2, _NO_SURF)
    print(f"n1 {s1.shape[0]} n2 {n2}: {len(plants)} plants, {handed} queries handed to the sequential scan")
    for p in plants:            # what the oracle says about the plants (the lists above are equal to it)
        assert e21[p["q"]] == (p["r2"] if p["kind"] == "nan" else -1), p
    if "nan" in _kinds(plants):
        assert handed >= 1      # the accepted tie
