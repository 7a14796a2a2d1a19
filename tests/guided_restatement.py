"""osfm_match_guided (orthosfm_amd/csrc/guided_kernels.hip) restated in numpy: what the entry returns for one pair --
record, list, F -- equals run() in every byte.

  F        given: (a, b, c, d, e) = F[0,2], F[1,2], F[2,0], F[2,1], F[2,2]; else affine_restatement.refit_vector over
           all seeds (every seed an inlier); fewer than 5 seeds without F: TOO_FEW, F zero; s = ((a^2 + b^2) + c^2) + d^2
           not > 0 or a coefficient not finite: DEGENERATE.  Either way the list is the seeds as given.
  band     affine_restatement.below on the match (i, j), for every i of view_1 and j of view_2
  seeds    a feature of a seed is neither a query nor a candidate
  search   per type, oracle_lib's nn_find (the pinned restatement of NearestNeighbor<T>::find) over the candidate rows
           in ascending feature index; no candidate: -1; then matching.h:114-146 with the squared ratio in float,
           0 / 0 accepted, no distance threshold
  cap      per type the largest dist_1st of nn_find(seed's row of view_1, [seed's row of view_2]); dist_1st > cap
           is dropped; a type without seeds has cap -1
  list     (i, j) added when i -> j and j -> i; seeds and additions ascending in feature_1
The keyword arguments behind * plant the faults that tests/test_guided_cases_cpu.py shows the cases to catch.
"""
import numpy as np

import affine_restatement as A
from oracle_lib import oracle_matcher

OK, TOO_FEW, DEGENERATE = 0, 1, 2


class View:
    """sift (ns, 128) uint16, surf (nu, 64) int16, pos (ns + nu, 2) float32 normalised positions."""

    def __init__(self, sift=None, surf=None, pos=None):
        self.sift = np.zeros((0, 128), np.uint16) if sift is None else np.ascontiguousarray(sift, dtype=np.uint16).reshape(-1, 128)
        self.surf = np.zeros((0, 64), np.int16) if surf is None else np.ascontiguousarray(surf, dtype=np.int16).reshape(-1, 64)
        n = self.sift.shape[0] + self.surf.shape[0]
        self.pos = np.zeros((n, 2), np.float32) if pos is None else np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 2)
        assert self.pos.shape[0] == n, (self.pos.shape, n)

    @property
    def n(self):
        return self.pos.shape[0]


def band_matrix(v, pos1, pos2, thr, le=False, transpose=False):
    """(n1, n2) bool: the verifier's test on every match (i, j)."""
    n1, n2 = pos1.shape[0], pos2.shape[0]
    if n1 == 0 or n2 == 0:
        return np.zeros((n1, n2), bool)
    m1 = np.repeat(pos1.astype(np.float64), n2, axis=0)
    m2 = np.tile(pos2.astype(np.float64), (n1, 1))
    return A.below(v, m1, m2, thr, le=le, transpose=transpose).reshape(n1, n2)


def _oneway(nn, Q, Cn, cand_of, coff, sq_lowe, cap, earlier_wins, cap_lt):
    """Results of the queries Q against the rows Cn: cand_of(i) gives the ascending local candidate ids of query i."""
    out = np.full(Q.shape[0], -1, np.int32)
    counts = np.zeros(Q.shape[0], np.int64)
    for i in range(Q.shape[0]):
        js = cand_of(i)
        counts[i] = js.size
        if js.size == 0:
            continue
        order = js[::-1] if earlier_wins else js
        r = nn.nn_find(Q[i], Cn[order])
        d1, d2, i1 = int(r[0]), int(r[1]), int(r[2])
        if (d1 >= cap) if cap_lt else (d1 > cap):
            continue
        with np.errstate(all="ignore"):
            if np.float32(d1) / np.float32(d2) > sq_lowe:
                continue
        out[i] = coff + int(order[i1])
    return out, counts


def run(view1, view2, seeds, F=None, threshold=0.0015, sift_lowe_ratio=0.8, surf_lowe_ratio=0.7, cap_from_seeds=True, *,
        le=False, seeds_in_play=False, earlier_wins=False, cap_lt=False, transpose=False, drop_surf_offset=False):
    """One pair of osfm_match_guided: dict(status, num_seeds, num_added, max_candidates, list (rows, 2) int32, F (3, 3)).
    Faults: le -- <= at the band's edge; seeds_in_play -- the seeds' features stay queries and candidates;
    earlier_wins -- the earlier index wins a tie; cap_lt -- a result AT the cap is dropped; transpose -- the views'
    roles exchanged in the band; drop_surf_offset -- SURF results without the other view's SIFT count."""
    nn = oracle_matcher()
    seeds = np.asarray(seeds, dtype=np.int32).reshape(-1, 2)
    k = seeds.shape[0]
    res = {"status": OK, "num_seeds": k, "num_added": 0, "max_candidates": 0, "list": seeds.copy(), "F": np.zeros((3, 3))}
    if F is None:
        if k < 5:
            res["status"] = TOO_FEW
            return res
        m1, m2 = A.matches(view1.pos, view2.pos, seeds)
        v = A.refit_vector(m1, m2, np.ones(k, bool))
    else:
        F = np.asarray(F, dtype=np.float64).reshape(3, 3)
        v = np.array([F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]])
    res["F"] = A.layout(v)
    a, b, c, d = (float(x) for x in v[:4])
    with np.errstate(all="ignore"):
        s = ((a * a + b * b) + c * c) + d * d
    if not np.all(np.isfinite(v)) or not s > 0.0:
        res["status"] = DEGENERATE
        return res
    band = band_matrix(v, view1.pos, view2.pos, threshold, le=le, transpose=transpose)
    if not seeds_in_play:
        band[seeds[:, 0], :] = False
        band[:, seeds[:, 1]] = False
    n1, n2 = view1.n, view2.n
    m12, m21 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
    maxc = 0
    types = ((view1.sift, view2.sift, 0, 0, np.float32(sift_lowe_ratio)),
             (view1.surf, view2.surf, view1.sift.shape[0], view2.sift.shape[0], np.float32(surf_lowe_ratio)))
    for t, (D1, D2, off1, off2, lowe) in enumerate(types):
        sq = np.float32(lowe * lowe)
        t1, t2 = D1.shape[0], D2.shape[0]
        mine = seeds[(seeds[:, 0] >= off1) & (seeds[:, 0] < off1 + t1)]
        cap = -1
        for f1, f2 in mine.tolist():
            cap = max(cap, int(nn.nn_find(D1[f1 - off1], D2[f2 - off2:f2 - off2 + 1])[0]))
        if not cap_from_seeds:
            cap = 1 << 30
        sub = band[off1:off1 + t1, off2:off2 + t2]
        r12, c12 = _oneway(nn, D1, D2, lambda i: np.nonzero(sub[i])[0], 0 if (t and drop_surf_offset) else off2, sq, cap,
                           earlier_wins, cap_lt)
        r21, c21 = _oneway(nn, D2, D1, lambda j: np.nonzero(sub[:, j])[0], 0 if (t and drop_surf_offset) else off1, sq, cap,
                           earlier_wins, cap_lt)
        m12[off1:off1 + t1], m21[off2:off2 + t2] = r12, r21
        maxc = max([maxc] + c12.tolist() + c21.tolist())
    taken = set(seeds[:, 0].tolist())
    added = [(i, int(m12[i])) for i in range(n1) if m12[i] >= 0 and m21[m12[i]] == i and i not in taken]
    rows = np.concatenate([seeds, np.asarray(added, np.int32).reshape(-1, 2)])
    res["list"] = rows[np.argsort(rows[:, 0], kind="stable")].astype(np.int32)
    res["num_added"] = len(added)
    res["max_candidates"] = int(maxc)
    return res
