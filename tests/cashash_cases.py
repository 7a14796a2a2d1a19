"""Seeded adversarial inputs for the cascade-hashing tests: what uniformly random
descriptors never produce -- buckets of several hundred entries, equal Hamming
distances, exact duplicates, SIFT rows whose inner products leave 16 bits, views
of every awkward size, a thousand pairs in one launch, a view at the size limit.

Plain numpy builders that return (sift, surf): one u16 [n, 128] and one s16
[m, 64] array per view.  The CPU tests (tests/test_cashash_cases_cpu.py: the
inputs reach what they claim, the oracle equals the reference on them) and the
GPU tests (tests/test_cashash_paths_gpu.py) import them, so both see the same
bytes.
"""
import numpy as np

from orthosfm_amd import synth

LIMIT = (1 << 17) - 1        # descriptors of one type in a view: the position field of a candidate key


def _rng(seed):
    return np.random.default_rng(seed)


def _sift_norm2(row):
    return int((row.astype(np.int64) ** 2).sum())


def _lift(row, lo=65025, hi=65535):
    """The u16 SIFT row with single bytes raised until lo <= |row|^2 <= hi: a copy of
    such a row is at distance 0 (NearestNeighbor clamps the product at 255^2), which the
    ratio test accepts whatever the second-best is -- exact duplicates MATCH, and which
    of them wins shows the candidate order."""
    row = row.copy()
    k = 0
    while _sift_norm2(row) < lo:
        row[(37 * k) % 128] += 1
        k += 1
    assert _sift_norm2(row) <= hi
    return row


def _shuffle(r, parts):
    rows = np.concatenate(parts, axis=0)
    return np.ascontiguousarray(rows[r.permutation(rows.shape[0])])


def _one_byte_off(r, row, n, exact, lo, hi):
    """n copies of a row: the first `exact` as they are, the others with one byte one off."""
    out = np.repeat(row[None].astype(np.int32), n, axis=0)
    col = r.integers(0, row.shape[0], n)
    step = np.where(r.integers(0, 2, n) > 0, 1, -1) * (np.arange(n) >= exact)
    out[np.arange(n), col] += step
    return np.clip(out, lo, hi).astype(row.dtype)


def _lane_rows(pattern, n=10):
    """n near-copies of one SIFT row whose elements 0, 8, 16, ... are all 64: in a product of two of
    them that 16-bit lane sums to exactly 2^16 and vanishes, and what the other lanes leave lies between
    255^2 and 65535.  The reference therefore ranks these rows by the REST of the product, while a sum
    formed in 32 bits (above 65535 for every one of them) beats any 16-bit best-so-far: a kernel that
    only truncates what it stores answers with the last candidate, not with the best."""
    p = pattern.copy()
    p[0::8] = 0
    k = 0
    while _sift_norm2(p) < 65250:
        k += 1
        if (37 * k) % 8:
            p[(37 * k) % 128] += 1
    p[0::8] = 64
    rows = np.repeat(p[None].astype(np.int32), n, axis=0)
    for j in range(1, n):
        rows[j, 8 * j + 1 + j % 6] += 1 if j % 2 else -1          # told apart by one byte outside the lane
    assert rows.min() >= 0 and rows.max() <= 255
    return rows.astype(np.uint16)


# rows of the clustered views, per view
CLUSTERED_SIFT = (900, 641, 130)
CLUSTERED_SURF = (700, 600, 90)
HEAVY_LEVELS = (24, 23, 22)       # 128 * 23 * 22 = 64768 stays inside 16 bits, every other product of two levels leaves them


def clustered_views():
    """Three views, each a shuffled mix of
      * rows drawn tightly around two centres: buckets of several hundred entries;
      * 300 (SURF: 150) landmarks shared by the views with small noise: real matches;
      * groups of 7 / 5 / 3 exact duplicates, identical in every view;
      * a "tight" group: one row of squared norm just above 255^2 with single bytes
        changed by one -- equal hashes, a few differing bucket ids, products on
        both sides of the clamp: many candidates on one Hamming level that first
        appear in different bucket groups, and matches among them that depend on
        the order;
      * SIFT only: 12 "heavy" constant-like rows on three levels and 6 rows of
        uniformly random bytes, each with an exact copy in the other views: inner
        products above 65535 (whole sums for the level rows, the single 16-bit
        lanes as well for the random ones), and next to them products of the same
        query that stay below;
      * SIFT only: 10 "lane" rows, the same in every view (see _lane_rows)."""
    r = _rng(4101)
    c_sift = r.standard_normal((2, 128))
    c_surf = r.standard_normal((2, 64))
    lm_sift = synth.sift_like(r.standard_normal((300, 128)))
    lm_surf = synth.surf_like(r.standard_normal((150, 64)))
    dup_sift = synth.quantize_sift(synth.sift_like(r.standard_normal((3, 128))))
    dup_sift = np.stack([_lift(d) for d in dup_sift])
    dup_sift = np.repeat(dup_sift, (7, 5, 3), axis=0)
    dup_surf = np.repeat(synth.quantize_surf(synth.surf_like(r.standard_normal((3, 64)))), (7, 5, 3), axis=0)
    tight_sift = _lift(synth.quantize_sift(synth.sift_like(r.standard_normal((1, 128))))[0], lo=65040)
    tight_surf = synth.quantize_surf(synth.surf_like(r.standard_normal((1, 64))))[0]
    heavy = np.empty((12, 128), np.uint16)
    for k in range(12):
        heavy[k] = HEAVY_LEVELS[k % 3]
        heavy[k, 8 * k:8 * k + 4] += 1            # told apart by four bytes
    wild = r.integers(0, 256, (6, 128)).astype(np.uint16)
    lane = _lane_rows(synth.quantize_sift(synth.sift_like(_rng(4102).standard_normal((1, 128))))[0])
    sifts, surfs = [], []
    for v in range(3):
        n = CLUSTERED_SIFT[v]
        which = r.integers(0, 2, n)
        clu = synth.quantize_sift(synth.sift_like(synth.sift_like(c_sift)[which] + 0.01 * r.standard_normal((n, 128))))
        lm = synth.quantize_sift(synth.sift_like(lm_sift + 0.004 * r.standard_normal(lm_sift.shape)))
        sifts.append(_shuffle(r, [clu, lm, dup_sift, _one_byte_off(r, tight_sift, 40, 8, 0, 255), heavy, wild, lane]))
        n = CLUSTERED_SURF[v]
        which = r.integers(0, 2, n)
        clu = synth.quantize_surf(synth.surf_like(synth.surf_like(c_surf)[which] + 0.012 * r.standard_normal((n, 64))))
        lm = synth.quantize_surf(synth.surf_like(lm_surf + 0.02 * r.standard_normal(lm_surf.shape)))
        surfs.append(_shuffle(r, [clu, lm, dup_surf, _one_byte_off(r, tight_surf, 24, 6, -127, 127)]))
    return sifts, surfs


def heavy_rows(sift):
    """Indices of the heavy and random-byte rows of a clustered view (squared norm above 65535)."""
    return np.nonzero((sift.astype(np.int64) ** 2).sum(axis=1) > 65535)[0]


TAIL_SIFT = (0, 1, 63, 64, 65, 255, 256, 257, 512, 513)
TAIL_SURF = (40, 0, 1, 64, 63, 65, 0, 128, 257, 256)
TAIL_SAME_SIFT, TAIL_SAME_SURF = 3, 5       # the views whose 64 SIFT / 65 SURF descriptors are all one row


def tail_views():
    """Ten views of one scene cut to the sizes at which the preparation kernels change
    path: nothing, one row, one short of / exactly / one past a chunk of 64 and a round
    of 256, two rounds, two rounds and a row.  View 3 holds one SIFT row 64 times and
    view 5 one SURF row 65 times (one bucket per group takes them all; a full wave of
    equal bucket ids); views 8 and 9 hold a copy of each, so that those rows have
    partners -- and more than ten candidates at Hamming distance 0."""
    iset = synth.make_image_set(len(TAIL_SIFT), max(TAIL_SIFT), n_surf=max(TAIL_SURF), config_id=41, visibility=0.6)
    sifts = [np.ascontiguousarray(iset.sift[v][:n]) for v, n in enumerate(TAIL_SIFT)]
    surfs = [np.ascontiguousarray(iset.surf[v][:n]) for v, n in enumerate(TAIL_SURF)]
    same_sift = _lift(sifts[9][17])
    same_surf = surfs[9][11].copy()
    sifts[TAIL_SAME_SIFT][:] = same_sift
    surfs[TAIL_SAME_SURF][:] = same_surf
    for v, at_sift, at_surf in ((8, 300, 200), (9, 17, 11)):
        sifts[v][at_sift] = same_sift
        surfs[v][at_surf] = same_surf
    return sifts, surfs


MANY_VIEWS = 46


def many_small_views():
    """46 small views of one scene: 1035 pairs, enough for a launch to take 64 buckets
    per workgroup.  Every view has a length of its own (94..130 SIFT, 22..40 SURF), every
    ninth has no SURF at all.  The last two views show another scene: their pairs with the
    other 44 stay below the match-count threshold."""
    iset = synth.make_image_set(MANY_VIEWS, 130, n_surf=40, config_id=42, visibility=0.8, distractor_frac=0.1,
                                unrelated_views=2)
    sifts = [np.ascontiguousarray(iset.sift[v][:130 - (v * 7) % 37]) for v in range(MANY_VIEWS)]
    surfs = [np.ascontiguousarray(iset.surf[v][:0 if v % 9 == 4 else 40 - (v * 5) % 19]) for v in range(MANY_VIEWS)]
    return sifts, surfs


def all_pairs(num_views):
    """The pairs of Matching::compute in its order (view_1 > view_2)."""
    return [(a, b) for a in range(num_views) for b in range(a)]


def limit_row():
    """The SIFT row the limit view repeats (squared norm inside 255^2 .. 65535: its copies match)."""
    return _lift(synth.quantize_sift(synth.sift_like(_rng(4301).standard_normal((1, 128))))[0])


def limit_views(n=LIMIT):
    """View 0: n (default: the most a view may hold, 2^17 - 1) copies of one SIFT row --
    33 MB, so built when called.  View 1: three rows, the middle one that same row.  No SURF."""
    row = limit_row()
    big = np.ascontiguousarray(np.broadcast_to(row, (n, 128)))
    small = synth.quantize_sift(synth.sift_like(_rng(4302).standard_normal((3, 128))))
    small[1] = row
    none = np.zeros((0, 64), np.int16)
    return [big, small], [none, none.copy()]
