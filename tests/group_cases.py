"""Cases for osfm_build_groups (orthosfm::buildGroups) where its kernels change path and on ties, with a host model.

The model is formulated unlike the product: a boolean (id x track) matrix, no 64-bit words, no stored score rows, no
cached picks -- every seed's pick is recomputed in every iteration (seeds whose views share no track at all score 0
against everybody and are not multiplied out).  It follows the literal restatement oracle/groups_oracle.c in all it
does, the `0` it appends when nothing scores included, and is trusted only because tests/test_group_cases_cpu.py
compares it with that oracle on every case the oracle finishes quickly.  Beside groups and counts it returns, per
iteration, how many seeds shared the maximum and which candidates shared the winning seed's best score.

Precondition of product, oracle and model alike: no track holds a view twice (see include/osfm_hip.h).
"""
import functools
import itertools
from dataclasses import dataclass, field

import numpy as np

OK, E_STATE = 0, -5


# ---------------------------------------------------------------------------
# the host model
# ---------------------------------------------------------------------------
@dataclass
class Step:
    remaining: int              # R: candidates at this iteration
    seeds_at_max: int           # seeds whose best score equals the winning one
    tied: tuple                 # indices into the ascending candidate list that share the winning seed's best score
    pick: int                   # the one taken (index into the candidate list), -1: nothing scored
    tied_ids: tuple = ()        # the ids of `tied`


@dataclass
class Result:
    groups: list
    counts: list
    ok: bool                    # the literal loop terminates (the oracle returns a result)
    zero_at: object             # index of the first group with a pick that scored 0 (the product refuses there), or None
    steps: list = field(default_factory=list)

    @property
    def iterations(self):
        return len(self.steps)

    @property
    def tied_seed_iterations(self):
        return sum(s.seeds_at_max >= 2 for s in self.steps)

    @property
    def tied_pick_iterations(self):
        return sum(len(s.tied) >= 2 for s in self.steps)


def host_model(view_ids, offs, views, group_size=3, cand_rule="min", seed_rule="first", keep=None):
    """buildGroups on sets of tracks.  cand_rule "min" / "max": smallest / largest id among the candidates that share a
    seed's best score; seed_rule "first" / "last": first / last seed in lexicographic order among those that share
    the maximum ("min" and "first" are the documented rule).  keep: boolean [num_tracks], the tracks that count."""
    ids = [int(x) for x in view_ids]
    offs = np.asarray(offs, np.int64)
    T = len(offs) - 1
    feats = np.asarray(views, np.int64)[:int(offs[-1])] if T > 0 else np.zeros(0, np.int64)
    rows = np.array(sorted(set(ids) | {0}), np.int64)            # the oracle counts by id, 0 included
    col = {int(v): i for i, v in enumerate(rows)}
    M = np.zeros((len(rows), max(T, 1)), bool)
    track_of = np.repeat(np.arange(T), np.diff(offs))
    known = np.isin(feats, rows)
    M[np.searchsorted(rows, feats[known]), track_of[known]] = True
    if keep is not None:
        M[:, :T] &= np.asarray(keep, bool)[None, :]
    first_of = (lambda w: w[0]) if cand_rule == "min" else (lambda w: w[-1])
    k = group_size - 1

    def complete(seed, remaining):
        """completeGroup for one seed, view by view."""
        g, added, zero, tied, tied_ids, pick = list(seed), 0, False, (), (), -1
        while len(g) < group_size:
            cands = [c for c in remaining if c not in g]
            best = 0
            if cands and len(set(g)) == len(g):
                mask = np.logical_and.reduce(M[[col[v] for v in g]], axis=0)
                sc = (M[[col[c] for c in cands]] & mask).sum(axis=1)
                best = int(sc.max())
            if best == 0:
                g.append(0)
                zero = True
            else:
                w = np.flatnonzero(sc == best)
                if len(w) > 1 and not tied:
                    tied = tuple(int(remaining.index(cands[i])) for i in w)
                    tied_ids = tuple(cands[i] for i in w)
                pick = int(remaining.index(cands[first_of(w)]))
                g.append(cands[first_of(w)])
            added = best
        return g, added, zero, Step(len(remaining), 1, tied, -1 if zero else pick, tied_ids)

    def iteration(used, remaining):
        """All (group_size - 1)-combinations of the used ids in lexicographic order, each completed by one view."""
        U = M[[col[v] for v in used]].astype(np.float32)
        Cm = M[[col[v] for v in remaining]].astype(np.float32)
        if k == 2:
            seeds = np.argwhere(np.triu(U @ U.T, 1) > 0)         # row-major: lexicographic; pairs without a common track score 0
            masks = U[seeds[:, 0]] * U[seeds[:, 1]]
        else:
            seeds = np.array(list(itertools.combinations(range(len(used)), k)), np.int64).reshape(-1, k)
            masks = np.ones((len(seeds), U.shape[1]), np.float32)
            for j in range(k):
                masks = masks * U[seeds[:, j]]
        scores = masks @ Cm.T if len(seeds) else np.zeros((0, len(remaining)), np.float32)
        best = scores.max(axis=1) if len(seeds) else np.zeros(0, np.float32)
        gmax = int(best.max()) if len(seeds) else 0
        if gmax == 0:                                             # every seed scores 0: the first one wins with id 0
            n_all = 1
            for j in range(k):
                n_all = n_all * (len(used) - j) // (j + 1)
            seed = used[:k] if seed_rule == "first" else used[len(used) - k:]
            return list(seed) + [0], 0, True, Step(len(remaining), n_all, (), -1)
        at_max = np.flatnonzero(best == gmax)
        s = at_max[0] if seed_rule == "first" else at_max[-1]
        w = np.flatnonzero(scores[s] == gmax)
        g = [used[j] for j in seeds[s]] + [remaining[first_of(w)]]
        tied = tuple(int(i) for i in w) if len(w) > 1 else ()
        return g, gmax, False, Step(len(remaining), len(at_max), tied, int(first_of(w)), tuple(remaining[i] for i in tied))

    cap = max(len(ids), 1)
    remaining = sorted(ids[2:])
    used = []
    res = Result([], [], False, None)
    g, added, zero, step = complete(ids[:2], remaining)
    while True:
        res.groups.append([int(v) for v in g])
        res.counts.append(int(added))
        res.steps.append(step)
        if zero and res.zero_at is None:
            res.zero_at = len(res.groups) - 1
        progress = False
        for v in g:
            if v in used:
                continue
            if v in remaining:
                remaining.remove(v)
                progress = True
            used.append(v)
        if len(res.groups) == 1:
            progress = True
        if not remaining:
            res.ok = True
            break
        if not progress or len(res.groups) >= cap:
            break
        used.sort()
        if len(used) < k:
            break
        g, added, zero, step = iteration(used, remaining)
    return res


def product_expectation(res):
    """What osfm_build_groups returns where the literal loop gives `res`: it refuses at the first pick that scores 0."""
    if res.zero_at is None and res.ok:
        return OK, res.groups, res.counts
    assert res.zero_at is not None
    return E_STATE, res.groups[:res.zero_at], res.counts[:res.zero_at]


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def ring_case(V, T, seed, twins=0, twin_ranks=(), first=(0, 1), arc=(2, 4), offset=0, planted=(), extra=0.15,
              last_full=False):
    """Tracks over arcs of a ring of view classes, a class being one view or two twins (views that appear in exactly
    the same tracks).  Everything is said in ranks (positions in ascending id order):
      twin_ranks   explicit twin pairs, `twins` more are drawn at random
      first        the ranks of view_ids[0] and view_ids[1]; their classes are neighbours on the ring
      arc          a track covers lo..hi-1 consecutive classes
      planted      (ranks, copies): tracks of exactly these views, put in front
      last_full    the last track holds every view
    Ids are V distinct values of offset .. offset + 3V - 1, view_ids a random permutation but for `first`."""
    rng = np.random.default_rng(seed)
    ids_sorted = offset + np.sort(rng.choice(3 * V, V, replace=False))
    pairs = [tuple(p) for p in twin_ranks]
    taken = {r for p in pairs for r in p}
    free = [int(r) for r in rng.permutation(V) if r not in taken]
    for _ in range(twins):
        pairs.append((free.pop(0), free.pop(0)))
    classes = [tuple(p) for p in pairs] + [(int(r),) for r in free]
    cls_of = {r: i for i, c in enumerate(classes) for r in c}
    order = [int(i) for i in rng.permutation(len(classes))]
    c0, c1 = cls_of[first[0]], cls_of[first[1]]
    if c0 != c1:                                                  # the two first views side by side
        order.remove(c1)
        order.insert(order.index(c0) + 1, c1)
    n = len(order)
    tracks = [list(r) for r, copies in planted for _ in range(copies)]
    while len(tracks) < T:
        if rng.random() >= extra:
            ln = min(int(rng.integers(arc[0], arc[1])), n)
            st = int(rng.integers(0, n))
            cs = [order[(st + j) % n] for j in range(ln)]
        else:
            cs = [int(c) for c in rng.choice(n, min(int(rng.integers(2, 4)), n), replace=False)]
        tracks.append([r for c in cs for r in classes[c]])
    tracks = tracks[:T]
    if last_full and T > 0:
        tracks[-1] = list(range(V))
    perm = [int(r) for r in rng.permutation(V) if r not in first]
    view_ids = np.array([ids_sorted[r] for r in list(first) + perm], np.int32)
    return view_ids, [[int(ids_sorted[r]) for r in t] for t in tracks]


def flatten(tracks):
    offs = np.zeros(len(tracks) + 1, np.int64)
    offs[1:] = np.cumsum([len(t) for t in tracks])
    views = np.array([v for t in tracks for v in t], np.int32)
    return offs, views


# ---------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                   # words / views / ties / sizes / general3 / edges
    group_size: int
    make: object                # () -> (view_ids, tracks)
    oracle: bool = True         # cheap enough for oracle/groups_oracle.c
    refused: bool = False       # the product answers OSFM_E_STATE


def _words(T, V, seed):
    return lambda: ring_case(V, T, seed, first=(3, 1), arc=(2, 5), last_full=True, offset=seed)


def _views(V, seed, twins=0, twin_ranks=(), first=None):
    first = first or ((V // 2, 2) if V > 4 else (V - 1, 0))
    return lambda: ring_case(V, 6 * V, seed, twins=twins, twin_ranks=twin_ranks, first=first, arc=(2, 5), offset=7 * (seed % 3))


def _all_ones():
    """Every triple of 8 views in exactly one track: every score is 1, every decision a tie."""
    ids = [31, 4, 17, 9, 22, 2, 40, 13]
    return np.array(ids, np.int32), [list(t) for t in itertools.combinations(sorted(ids), 3)]


def _sizes(gs, V, seed, twins=0):
    def make():
        ids, tracks = ring_case(V, 20 * V, seed, twins=twins, first=(V - 2, 1), arc=(gs - 1 if twins == 0 else gs // 2, gs + 2),
                                extra=0.05, offset=seed)
        return ids, tracks
    return make


def _one_group(gs, seed):
    """V = group size: one group, the first seed adds group size - 2 views; arcs of every length from 3 up."""
    def make():
        ids, tracks = ring_case(gs, 12 * gs, seed, first=(gs - 1, 1), arc=(3, gs + 1), extra=0.3, last_full=True, offset=5)
        return ids, tracks
    return make


def _big262():
    """R = 260 candidates at the first group: the general path's candidate loop takes two strides of 256.  Views 0 and
    1 are ranks 100 and 101.  Planted: ranks 3 and 258 (candidates 3 and 256: thread 3's first and thread 0's second
    stride) share 90 tracks with them, ranks 1 and 261 (candidates 1 and 257 once those two are gone: one thread's two
    strides) share 70; the rest is a ring of twins with scores far below."""
    planted = (((100, 101, 3, 258), 90), ((100, 101, 1, 261), 70))
    return ring_case(262, 2400, 262, twins=100, twin_ranks=((3, 258), (1, 261)), first=(100, 101), arc=(2, 5), offset=11,
                     planted=planted, extra=0.0)


def _outside():
    ids, tracks = ring_case(9, 60, 41, first=(4, 2), arc=(2, 5), offset=3)
    rng = np.random.default_rng(41)
    strangers = [1000, -5, int(max(ids)) + 1] + [v for v in range(3, 30) if v not in set(int(i) for i in ids)][:3]
    tracks = [t + [strangers[int(rng.integers(len(strangers)))]] if i % 3 == 0 else t for i, t in enumerate(tracks)]
    tracks += [[1000, -5], [strangers[3], int(ids[0]), strangers[4]]]
    return ids, tracks


def _short_tracks():
    ids, tracks = ring_case(8, 50, 43, first=(5, 2), arc=(2, 5), offset=1)
    out = []
    for i, t in enumerate(tracks):
        out.append(t)
        out.append([] if i % 2 else [int(ids[i % 8])])
    return ids, [[]] + out + [[]]


def _no_tracks():
    return np.array([5, 2, 9, 0], np.int32), []


def _late_unreachable():
    """View 50 appears in pairs only, never in a track of three: every other view is assigned first (6 groups)."""
    ids, tracks = ring_case(8, 60, 47, first=(4, 2), arc=(3, 6), offset=2)
    ids = np.concatenate([ids[:5], [50], ids[5:]]).astype(np.int32)
    tracks += [[50, int(ids[0])], [int(ids[3]), 50], [50]]
    return ids, tracks


def _isolated_first():
    """Views 0 and 1 (ids 8 and 3) share a track only with each other."""
    ids, tracks = ring_case(7, 40, 53, first=(4, 2), arc=(2, 5), offset=20)
    rest = [int(v) for v in ids]
    return np.concatenate([[8, 3], ids]).astype(np.int32), tracks + [[8, 3]] * 3 + [[8, rest[0]], [3, rest[1]]]


def _id_zero():
    """Id 0 is unassigned and every seed scores 0: the reference appends bestViewID's start value 0 and goes on."""
    return np.array([4, 7, 0, 9], np.int32), [[4, 7, 9], [4, 7, 9], [7, 9], [4, 9]]


def _dry_first_group():
    """Group size 5: views 0 and 1 share tracks with view 6 only, so the first group's second step has no candidate."""
    return np.array([2, 9, 6, 4, 11, 7, 5], np.int32), [[2, 9, 6], [2, 9, 6], [6, 4, 11, 7, 5], [9, 4, 11, 7], [2, 4, 5]]


WORD_T = (1, 64, 65, 4096, 4097, 8192, 8193, 12289, 16385)

CASES = (
    [Case(f"w{T}", "words", 3, _words(T, 6 + i % 3, 100 + i)) for i, T in enumerate(WORD_T)]
    + [Case("v3", "views", 3, _views(3, 1)), Case("v4", "views", 3, _views(4, 2)),
       Case("v23", "views", 3, _views(23, 3)), Case("v24", "views", 3, _views(24, 4)),
       Case("v32", "views", 3, _views(32, 5)), Case("v33", "views", 3, _views(33, 6)),
       Case("v64", "views", 3, _views(64, 7)), Case("v65", "views", 3, _views(65, 8)),
       Case("v4t", "views", 3, _views(4, 12, twin_ranks=((1, 3),), first=(2, 0))),
       Case("v24t", "views", 3, _views(24, 13, twins=8)),
       # twins either side of the 32-candidate chunks: ranks 31 | 32, 3 | 32, 63 | 64 and 5 | 64
       Case("v33t", "views", 3, _views(33, 14, twins=8, twin_ranks=((31, 32), (3, 30)))),
       Case("v33u", "views", 3, _views(33, 15, twins=8, twin_ranks=((3, 32),))),
       Case("v65t", "views", 3, _views(65, 16, twins=20, twin_ranks=((63, 64), (31, 33)))),
       Case("v65u", "views", 3, _views(65, 17, twins=20, twin_ranks=((5, 64), (20, 40))))]
    + [Case("tie12", "ties", 3, lambda: ring_case(12, 72, 21, twins=6, first=(7, 3), arc=(2, 4), offset=0)),
       Case("tie34", "ties", 3, lambda: ring_case(34, 200, 22, twins=17, first=(20, 5), arc=(2, 4), offset=9)),
       Case("tie66", "ties", 3, lambda: ring_case(66, 400, 23, twins=33, first=(40, 9), arc=(2, 4), offset=100)),
       Case("ones", "ties", 3, _all_ones)]
    + [Case(f"g{gs}one", "sizes", gs, _one_group(gs, 60 + gs)) for gs in (4, 5, 6, 7, 8)]
    + [Case("g4v11", "sizes", 4, _sizes(4, 11, 71)), Case("g5v12", "sizes", 5, _sizes(5, 12, 72)),
       Case("g6v13", "sizes", 6, _sizes(6, 13, 73)), Case("g7v14", "sizes", 7, _sizes(7, 14, 74)),
       Case("g8v12", "sizes", 8, _sizes(8, 12, 75)),
       Case("g4v12t", "sizes", 4, _sizes(4, 12, 81, twins=6)), Case("g5v12t", "sizes", 5, _sizes(5, 12, 82, twins=5)),
       Case("g6v14t", "sizes", 6, _sizes(6, 14, 83, twins=7)), Case("g8v12t", "sizes", 8, _sizes(8, 12, 84, twins=6))]
    + [Case("big262", "general3", 3, _big262, oracle=False)]
    + [Case("outside", "edges", 3, _outside), Case("short", "edges", 3, _short_tracks),
       Case("empty", "edges", 3, _no_tracks, refused=True),
       Case("late", "edges", 3, _late_unreachable, refused=True),
       Case("isolated", "edges", 3, _isolated_first, refused=True),
       Case("id0", "edges", 3, _id_zero, refused=True),
       Case("dry5", "edges", 5, _dry_first_group, refused=True)]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
TIE_CASES = [c.name for c in CASES if c.kind == "ties"]
WORD_CASES = [c.name for c in CASES if c.kind == "words"]
ORACLE_CASES = [c.name for c in CASES if c.oracle]
MODEL_ONLY = [c.name for c in CASES if not c.oracle]                     # V = 262: the oracle would take minutes


@functools.lru_cache(maxsize=None)
def build(name):
    """(view_ids, track_offsets, track_views) of a case; computed once, never modified."""
    ids, tracks = BY_NAME[name].make()
    offs, views = flatten(tracks)
    for a in (ids, offs, views):
        a.setflags(write=False)
    return ids, offs, views


@functools.lru_cache(maxsize=None)
def expected(name):
    """The host model's result under the documented rule; computed once and shared."""
    ids, offs, views = build(name)
    return host_model(ids, offs, views, BY_NAME[name].group_size)


def rank_of(name, view_id):
    return int(np.searchsorted(np.sort(build(name)[0]), view_id))
