"""Seeded cases of osfm_match_guided for tests/test_guided_cases_cpu.py (the restatement against its planted faults and
an independent anchor) and tests/test_guided_gpu.py (the entry against the restatement).  A case is a Case: two
guided_restatement.View, the seeds, F or None, and the options of the call.  cases(limits) builds them all;
limits = (queries_per_workgroup, positions_per_chunk, candidates_per_pass) of osfm_guided_limits -- sizes marked L
follow it.  Everything is drawn from numpy generators seeded by the case's name: the same bytes on every run."""
import zlib
from dataclasses import dataclass, field

import numpy as np

import affine_restatement as A
from guided_restatement import View
from orthosfm_amd import synth

DEFAULT_LIMITS = (16, 2048, 64)
THR = 2.0 ** -9          # a float32 (and float64) number: the band-edge positions are exact
TWIN = dict(num_views=3, feats_per_view=400, seed=11, twin_frac=0.5, visibility=0.6)


@dataclass
class Case:
    name: str
    view1: View
    view2: View
    seeds: np.ndarray
    F: object = None
    options: dict = field(default_factory=dict)


def _rng(name):
    return np.random.default_rng([zlib.crc32(name.encode()), 0x6D])


def rand_sift(rng, n):
    return synth.quantize_sift(synth.sift_like(rng.normal(size=(n, 128))))


def rand_surf(rng, n):
    return synth.quantize_surf(synth.surf_like(rng.normal(size=(n, 64))))


def near_sift(rng, rows, noise=0.02):
    """Rows a little off `rows` (uint16 SIFT): what a second view sees of the same landmark."""
    f = rows.astype(np.float64) / 255.0 + noise * np.abs(rng.normal(size=rows.shape)) * 0.2
    return synth.quantize_sift(synth.sift_like(f))


def near_surf(rng, rows, noise=0.02):
    return synth.quantize_surf(synth.surf_like(rows.astype(np.float64) / 127.0 + noise * rng.normal(size=rows.shape) * 0.2))


def layout(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0):
    return A.layout(np.array([a, b, c, d, e], dtype=np.float64))


def norm_pos(iset, v):
    """feature_set.cc:42-55, as pipeline.match_and_build_tracks uploads them"""
    W, H = iset.width, iset.height
    return ((iset.pos[v] + 0.5 - np.array([W / 2, H / 2])) / max(W, H)).astype(np.float32)


def true_matches(iset, v1, v2, n1=None, n2=None):
    """(f1, f2) of the landmarks both views show (within the first n1 / n2 rows), ascending in f1."""
    l1, l2 = iset.landmark[v1][:n1], iset.landmark[v2][:n2]
    where2 = {int(l): j for j, l in enumerate(l2) if l >= 0}
    return np.array([(i, where2[int(l)]) for i, l in enumerate(l1) if l >= 0 and int(l) in where2], np.int32).reshape(-1, 2)


_sets = {}


def image_set(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _sets:
        _sets[key] = synth.make_image_set(**kw)
    return _sets[key]


def image_case(name, iset, v1, v2, n1=None, n2=None, seed_every=2, give_F=False, options=None):
    """Two views of a synthetic scene cut to their first n1 / n2 rows; every seed_every-th true match is a seed; F is
    fitted to the seeds by the call, or (give_F) given: the least-squares F_A of ALL true matches of the uncut views."""
    t = true_matches(iset, v1, v2, n1, n2)
    F = None
    if give_F:
        full = true_matches(iset, v1, v2)
        m1, m2 = A.matches(norm_pos(iset, v1), norm_pos(iset, v2), full)
        F = A.layout(A.refit_vector(m1, m2, np.ones(full.shape[0], bool)))
    return Case(name, View(iset.sift[v1][:n1], None, norm_pos(iset, v1)[:n1]), View(iset.sift[v2][:n2], None, norm_pos(iset, v2)[:n2]),
                t[::seed_every], F, dict(options or {}))


def cluster_case(name, sizes2, per1=2, surf_sizes2=(), seeds_per_cluster=0, options=None, no_sift1=False):
    """F_A = x2 - x1: cluster g sits at x = 0.01 g in both views, so a feature of view_1 in cluster g has the features
    of view_2 in cluster g as candidates and no others.  View_1 holds per1 features per cluster, each a near copy of
    one member of its cluster in view_2 (where the cluster has any); the first seeds_per_cluster of them are seeds."""
    rng = _rng(name)
    opts = dict(threshold=THR, cap_from_seeds=0)
    opts.update(options or {})

    def side(sizes, rand, near, x0):
        d2, x2, d1, x1, seeds = [], [], [], [], []
        for g, n in enumerate(sizes):
            rows = rand(rng, n)
            base = len(x2)
            d2.append(rows)
            x2 += [x0 + 0.01 * g] * n
            picks = rng.permutation(n)[:per1] if n else []
            for q in range(per1):
                if q < len(picks):
                    d1.append(near(rng, rows[picks[q]:picks[q] + 1]))
                    if q < seeds_per_cluster:
                        seeds.append((len(x1), base + int(picks[q])))
                else:
                    d1.append(rand(rng, 1))
                x1.append(x0 + 0.01 * g)
        return np.concatenate(d1), np.concatenate(d2), x1, x2, seeds

    s1, s2, xs1, xs2, seeds = side(sizes2, rand_sift, near_sift, -0.4)
    if no_sift1:
        s1, xs1, seeds = s1[:0], [], []
    ns1, ns2 = s1.shape[0], s2.shape[0]
    u1 = u2 = None
    if surf_sizes2:
        u1, u2, xu1, xu2, useeds = side(surf_sizes2, rand_surf, near_surf, 0.1)
        xs1, xs2 = xs1 + xu1, xs2 + xu2
        seeds += [(a + ns1, b + ns2) for a, b in useeds]

    def pos(xs):
        return np.stack([np.asarray(xs), rng.uniform(-0.4, 0.4, len(xs))], axis=1).astype(np.float32)

    return Case(name, View(s1, u1, pos(xs1)), View(s2, u2, pos(xs2)), np.array(seeds, np.int32).reshape(-1, 2),
                layout(a=1.0, c=-1.0), opts)


def edge_case():
    """a = 1, e = -t: the residual of (i, j) is x2_j - t, a float32 difference.  Features 0..5 of view_2 sit at t +- THR,
    one float32 step inside and one outside; feature i of view_1 has the descriptor of feature i of view_2."""
    rng = _rng("edge")
    t = np.float32(0.25)
    up, dn = np.float32(t + np.float32(THR)), np.float32(t - np.float32(THR))
    xs = np.array([up, np.nextafter(up, np.float32(0)), np.nextafter(up, np.float32(1)),
                   dn, np.nextafter(dn, np.float32(1)), np.nextafter(dn, np.float32(0))], np.float32)
    assert float(xs[0]) - 0.25 == THR and 0.25 - float(xs[3]) == THR
    d = rand_sift(rng, 6)
    p2 = np.stack([xs, rng.uniform(-0.3, 0.3, 6).astype(np.float32)], axis=1)
    p1 = rng.uniform(-0.3, 0.3, (6, 2)).astype(np.float32)
    return Case("edge", View(d, None, p1), View(d.copy(), None, p2), np.zeros((0, 2), np.int32), layout(a=1.0, e=-0.25),
                dict(threshold=THR, cap_from_seeds=0, sift_lowe_ratio=1.0))


def ties_cases():
    """View_2: rows 1 and 3 are one descriptor, both in the band of query 0 of view_1 (its near copy); rows 0 and 2 are
    far off in x.  With the ratio at 1 the later duplicate is the match; at the default the pair is rejected
    (second == best).  `zero`: the query and its only two candidates are one row with a product of 65025 -- 0 / 0."""
    out = []
    for name, ratio in (("ties_ratio1", 1.0), ("ties_default", 0.8)):
        rng = _rng("ties")
        d = rand_sift(rng, 4)
        d[3] = d[1]
        q = np.concatenate([near_sift(rng, d[1:2]), rand_sift(rng, 1)])
        p2 = np.array([[0.3, 0.0], [0.1, 0.1], [-0.3, 0.2], [0.1, -0.2]], np.float32)
        p1 = np.array([[0.1, 0.3], [-0.2, 0.0]], np.float32)
        out.append(Case(name, View(q, None, p1), View(d, None, p2), np.zeros((0, 2), np.int32), layout(a=1.0, c=-1.0),
                        dict(threshold=THR, cap_from_seeds=0, sift_lowe_ratio=ratio)))
    z = np.zeros((1, 128), np.uint16)
    z[0, 5] = 255
    out.append(Case("ties_zero", View(z, None, np.array([[0.1, 0.0]], np.float32)),
                    View(np.concatenate([z, z]), None, np.array([[0.1, 0.2], [0.1, -0.2]], np.float32)),
                    np.zeros((0, 2), np.int32), layout(a=1.0, c=-1.0), dict(threshold=THR, cap_from_seeds=0)))
    return out


def wrap_case():
    """Products above 65535 (rows with two bytes of 255 in different 16-bit lanes score 130050, held as 64514 in the
    T-typed state): the result depends on the ORDER the candidates are taken in, which is the index order."""
    rng = _rng("wrap")
    big = np.zeros(128, np.uint16)
    big[[0, 1]] = 255
    mid = np.zeros(128, np.uint16)
    mid[0] = 254                     # 64770 against `big`: above the held 64514, below the true 130050
    low = np.zeros(128, np.uint16)
    low[1] = 200
    cands = np.stack([low, big, mid, low, big, mid, mid, big, low])
    cands = np.concatenate([cands, rand_sift(rng, 3)])
    q = np.stack([big, mid, low, big])
    n1, n2 = q.shape[0], cands.shape[0]
    p1 = np.stack([np.full(n1, 0.2), rng.uniform(-0.3, 0.3, n1)], axis=1).astype(np.float32)
    p2 = np.stack([np.full(n2, 0.2), rng.uniform(-0.3, 0.3, n2)], axis=1).astype(np.float32)
    return Case("wrap", View(q, None, p1), View(cands, None, p2), np.zeros((0, 2), np.int32), layout(a=1.0, c=-1.0),
                dict(threshold=THR, cap_from_seeds=0, sift_lowe_ratio=2.0))     # (a wrapped best is FARTHER than the second)


def surf_wrap_case():
    """SURF rows whose 16-bit lanes wrap (eight products of 127 * 127 in one lane) and whose sums leave int16."""
    rng = _rng("surf_wrap")
    hot = np.zeros(64, np.int16)
    hot[0::8] = 127                  # lane 0: 8 * 16129 = 129032 -> wraps
    half = np.zeros(64, np.int16)
    half[0:16:8] = 127
    neg = -hot
    cands = np.concatenate([np.stack([half, hot, neg, half, hot]), rand_surf(rng, 4)])
    q = np.stack([hot, half, neg])
    n1, n2 = q.shape[0], cands.shape[0]
    p1 = np.stack([np.full(n1, -0.1), rng.uniform(-0.3, 0.3, n1)], axis=1).astype(np.float32)
    p2 = np.stack([np.full(n2, -0.1), rng.uniform(-0.3, 0.3, n2)], axis=1).astype(np.float32)
    return Case("surf_wrap", View(None, q, p1), View(None, cands, p2), np.zeros((0, 2), np.int32), layout(a=1.0, c=-1.0),
                dict(threshold=THR, cap_from_seeds=0, surf_lowe_ratio=1.0))


def peaky_case():
    """synth.add_peaky_rows: rows with bytes above 127 among queries and candidates of a wide band."""
    iset = synth.make_image_set(2, 160, seed=5, twin_frac=0.5, visibility=0.6)
    synth.add_peaky_rows(iset, 24, seed=5)
    return image_case("peaky", iset, 1, 0, seed_every=3, options=dict(threshold=0.02, sift_lowe_ratio=0.9))


def cap_cases():
    """Cluster 0 holds a seed (q_s, c_s).  Cluster 1: a copy of q_s whose only candidate is a copy of c_s -- exactly at
    the cap, kept.  Cluster 2: the same with one byte of the candidate lowered -- a step above the cap, dropped; with
    the cap off it is added."""
    out = []
    for name, cap in (("cap_on", 1), ("cap_off", 0)):
        rng = _rng("cap")
        c = rand_sift(rng, 1)
        q = near_sift(rng, c)
        c_less = c.copy()
        k = int(np.argmax(q[0] * (c[0] > 0)))
        c_less[0, k] -= 1
        xs = np.array([0.0, 0.01, 0.02], np.float32)
        p1 = np.stack([xs, rng.uniform(-0.3, 0.3, 3).astype(np.float32)], axis=1)
        p2 = np.stack([xs, rng.uniform(-0.3, 0.3, 3).astype(np.float32)], axis=1)
        out.append(Case(name, View(np.concatenate([q, q, q]), None, p1), View(np.concatenate([c, c, c_less]), None, p2),
                        np.array([[0, 0]], np.int32), layout(a=1.0, c=-1.0), dict(threshold=THR, cap_from_seeds=cap)))
    return out


def cases(limits=DEFAULT_LIMITS):
    Q, CH, P = limits
    out = [edge_case()]
    # candidate counts per query (L): 0, 1, 2, P - 1, P, P + 1; and every row of the other view
    out.append(cluster_case("counts", (0, 1, 2, P - 1, P, P + 1)))
    out.append(cluster_case("counts_all", (2 * P + 3,), per1=3))
    out += ties_cases()
    # types: both with the combined offsets; a view without SURF; view_1 without SIFT; a type without seeds under the cap
    out.append(cluster_case("types_both", (3, 5, 2), surf_sizes2=(4, 1, 6), options=dict(surf_lowe_ratio=0.9)))
    out.append(cluster_case("types_no_surf2", (3, 5), surf_sizes2=(0, 0)))
    out.append(cluster_case("types_no_sift1", (3, 4), surf_sizes2=(4, 3), no_sift1=True))
    out.append(cluster_case("types_cap_sift_seeds_only", (4, 4, 4), surf_sizes2=(3, 3), seeds_per_cluster=1, options=dict(cap_from_seeds=1)))
    out.append(cluster_case("types_cap_both_seeds", (4, 4, 4), surf_sizes2=(3, 3, 3), seeds_per_cluster=1, options=dict(cap_from_seeds=1)))
    out[-2].seeds = out[-2].seeds[out[-2].seeds[:, 0] < out[-2].view1.sift.shape[0]]
    out += [wrap_case(), surf_wrap_case(), peaky_case()]
    out += cap_cases()
    # the twin set: F fitted to the seeds, F given, too few seeds, a zero F
    twin = image_set(**TWIN)
    out.append(image_case("twin_fit", twin, 1, 0))
    out.append(image_case("twin_given", twin, 2, 1, give_F=True))
    out.append(image_case("twin_no_cap", twin, 2, 0, options=dict(cap_from_seeds=0)))
    few = image_case("too_few", twin, 1, 0, n1=150, n2=150)
    few.seeds = few.seeds[:4][::-1].copy()          # not ascending: the list is the seeds AS GIVEN
    out.append(few)
    zero = image_case("zero_F", twin, 1, 0, n1=150, n2=150)
    zero.F = np.zeros((3, 3))
    out.append(zero)
    # view sizes: 1, 63, 64, 65, and (L) the workgroup's queries and the chunk +- 1
    small = image_set(num_views=2, feats_per_view=80, seed=3, twin_frac=0.5, visibility=0.9)
    for n1, n2 in ((1, 65), (65, 1), (63, 64), (64, 63), (Q - 1, Q + 1), (Q + 1, Q - 1)):
        out.append(image_case(f"size_{n1}_{n2}", small, 1, 0, n1=n1, n2=n2, give_F=True, options=dict(threshold=0.004)))
    big = image_set(num_views=2, feats_per_view=CH + 1, seed=4, twin_frac=0.5, visibility=0.7)
    out.append(image_case(f"size_{CH - 1}_{CH + 1}", big, 1, 0, n1=CH - 1, n2=CH + 1, seed_every=3))
    out.append(image_case(f"size_{CH + 1}_{CH - 1}", big, 1, 0, n1=CH + 1, n2=CH - 1, seed_every=3))
    return out


def batch_set():
    """9 views, 36 pairs and 4 of them once more: 40 pairs of one call, F fitted to each pair's seeds."""
    iset = image_set(num_views=9, feats_per_view=120, seed=21, twin_frac=0.5, visibility=0.7)
    pairs = [(a, b) for a in range(9) for b in range(a)]
    pairs += pairs[3:7]
    seeds = [true_matches(iset, a, b)[::2] for a, b in pairs]
    views = [View(iset.sift[v], None, norm_pos(iset, v)) for v in range(9)]
    return views, pairs, seeds
