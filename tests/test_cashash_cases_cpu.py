"""The cascade-hashing cases (tests/cashash_cases.py) do what they claim, and the
oracle is pinned to the reference on them.  No GPU: every number here comes from
the oracle (oracle/cashash_oracle.c), the reference build (oracle/_ref) and numpy,
never from the library under test.

The condition tests keep the GPU tests (tests/test_cashash_paths_gpu.py) honest: a
generator that stops producing buckets of three candidate chunks, ties, wrapping
inner products or a launch of a thousand pairs fails here, on any machine."""
import numpy as np
import pytest

import cashash_cases
import oracle_lib

needs_ref = pytest.mark.skipif(oracle_lib.ref_cashash() is None, reason="oracle/_ref/libref_cashash.so not built")
MIN_CAND, MAX_CAND = oracle_lib.CASHASH_MIN, oracle_lib.CASHASH_MAX


@pytest.fixture(scope="module")
def clustered():
    sifts, surfs = cashash_cases.clustered_views()
    return sifts, surfs, oracle_lib.OracleCasHash(sifts, surfs)


@pytest.fixture(scope="module")
def tails():
    sifts, surfs = cashash_cases.tail_views()
    return sifts, surfs, oracle_lib.OracleCasHash(sifts, surfs)


@pytest.fixture(scope="module")
def many():
    sifts, surfs = cashash_cases.many_small_views()
    return sifts, surfs, oracle_lib.OracleCasHash(sifts, surfs)


@pytest.fixture(scope="module")
def limit():
    sifts, surfs = cashash_cases.limit_views()
    return sifts, surfs, oracle_lib.OracleCasHash(sifts, surfs)


# ---------------------------------------------------------------------------
# CascadeHashing::oneway_match once more, in numpy, from the oracle's hashes and
# bucket ids: what the candidate lists look like, and what another ranking or
# another arithmetic would answer
# ---------------------------------------------------------------------------
def bucket_sizes(ids):
    """[groups, 256] entries per bucket."""
    return np.stack([np.bincount(ids[g], minlength=256) for g in range(ids.shape[0])])


def hash_bits(hashes):
    return np.unpackbits(np.ascontiguousarray(hashes).view(np.uint8), axis=1)


def candidates(bits1, ids1, bits2, ids2, q):
    """(ids, Hamming distances) of the candidates of query q in order of first appearance
    over the bucket groups (collect_features_from_buckets)."""
    seen = np.zeros(ids2.shape[1], bool)
    out = []
    for g in range(ids1.shape[0]):
        c = np.nonzero((ids2[g] == ids1[g, q]) & ~seen)[0]
        seen[c] = True
        out.append(c)
    c = np.concatenate(out)
    return c, (bits2[c] != bits1[q]).sum(axis=1)


def top_ranked(c, hd, by_id=False):
    """collect_top_ranked_candidates: whole Hamming levels until six are in, never more than ten.
    by_id: inside a level by feature id and not by first appearance."""
    order = np.lexsort((c, hd)) if by_id else np.argsort(hd, kind="stable")
    c, hd = c[order], hd[order]
    top = []
    for level in np.unique(hd):
        for x in c[hd == level]:
            top.append(int(x))
            if len(top) >= MAX_CAND:
                break
        if len(top) >= MIN_CAND:
            break
    return top


def products(q, rows, signed, wrap):
    """Inner products of a query with candidate rows: wrap -- as NearestNeighbor<T> forms them, eight
    16-bit lanes (element i in lane i % 8) that wrap, signed lanes read back as signed; else exact."""
    p = q.astype(np.int64)[None] * rows.astype(np.int64)
    if not wrap:
        return p.sum(axis=1)
    lanes = p.reshape(rows.shape[0], -1, 8).sum(axis=1) & 0xffff
    if signed:
        lanes = np.where(lanes >= 32768, lanes - 65536, lanes)
    return lanes.sum(axis=1)


def nearest(ips, signed, lowe, wrap=True):
    """NearestNeighbor<T>::find + the ratio test of oneway_match over products in candidate
    order: index into the list or -1.  wrap=False: the state is not truncated to T either."""
    best = second = i1 = 0
    bits = 0xffff
    for j, ip in enumerate(int(x) for x in ips):
        if ip >= second:
            t = ip if not wrap else ((ip & bits) - 65536 if signed and (ip & bits) >= 32768 else ip & bits)
            if ip >= best:
                second, best, i1 = best, t, j
            else:
                second = t
    if signed:
        d1, d2 = (32258 - 2 * min(16129, max(0, x)) for x in (best, second))
        if wrap:
            d1, d2 = ((d + 32768) % 65536 - 32768 for d in (d1, d2))
    else:
        d1, d2 = (min(32767, 65025 - min(65025, x)) * 2 for x in (best, second))
    with np.errstate(divide="ignore", invalid="ignore"):
        if np.float32(d1) / np.float32(d2) > np.float32(lowe) * np.float32(lowe):
            return -1
    return i1 if len(ips) else -1


class Model:
    """One direction of one descriptor type of a pair."""

    def __init__(self, orc, t, v1, v2):
        self.t, self.lowe = t, orc.lowe[t]
        self.d1, self.d2 = ((orc.sifts, orc.surfs)[t][v] for v in (v1, v2))
        (h1, self.ids1), (h2, self.ids2) = orc.local[t][v1], orc.local[t][v2]
        self.bits1, self.bits2 = hash_bits(h1), hash_bits(h2)
        self.oracle = oracle_lib.oracle_cashash_oneway(t, self.d1, h1, self.ids1, self.d2, h2, self.ids2, self.lowe)

    def cand(self, q):
        return candidates(self.bits1, self.ids1, self.bits2, self.ids2, q)

    def answer(self, q, by_id=False, lanes=True):
        """lanes=False: the products as 32-bit sums, only the best / second-best state in 16 bits."""
        top = top_ranked(*self.cand(q), by_id=by_id)
        if not top:
            return -1
        j = nearest(products(self.d1[q], self.d2[top], self.t == 1, lanes), self.t == 1, self.lowe)
        return top[j] if j >= 0 else -1

    def plain(self, q):
        """Exact arithmetic over ALL rows of the other view: what a nearest-neighbour search that
        neither hashes nor wraps answers."""
        return nearest(products(self.d1[q], self.d2, self.t == 1, False), self.t == 1, self.lowe, wrap=False)


# ---------------------------------------------------------------------------
# clustered_views
# ---------------------------------------------------------------------------
def test_clustered_buckets_span_three_candidate_chunks(clustered):
    """The scan kernel takes queries and candidates 128 at a time: more than 256 entries in a
    bucket are three chunks; an odd bucket ends on the single-candidate tail."""
    sifts, surfs, orc = clustered
    for t in (0, 1):
        largest = [int(bucket_sizes(orc.local[t][v][1]).max()) for v in range(3)]
        print("type", t, "largest bucket per view", largest)
        assert sum(x > 256 for x in largest) >= 2, (t, largest)
        sizes = np.concatenate([bucket_sizes(orc.local[t][v][1]).ravel() for v in range(3)])
        assert ((sizes % 2 == 1) & (sizes > 128)).any(), t      # an odd tail behind a full chunk
        # a bucket of more than 128 queries meets the same bucket with more than 128 candidates
        a, b = bucket_sizes(orc.local[t][0][1]), bucket_sizes(orc.local[t][1][1])
        assert ((a > 128) & (b > 128)).any(), t
        assert ((a > 256) & (b > 256)).any(), t


def test_clustered_pairs_match(clustered):
    """Large buckets are no use if nothing is decided in them: the views still share their landmarks."""
    sifts, surfs, orc = clustered
    m12, _ = orc.pairwise_match(0, 1)
    ns = sifts[0].shape[0]
    print("matches 0 -> 1: sift", int((m12[:ns] >= 0).sum()), "surf", int((m12[ns:] >= 0).sum()))
    assert (m12[:ns] >= 0).sum() >= 250 and (m12[ns:] >= 0).sum() >= 100


@pytest.mark.parametrize("t", (0, 1))
def test_model_restates_the_oracle(clustered, t):
    """The numpy model the tests below argue with is the oracle's one-way match, query for query."""
    _, _, orc = clustered
    m = Model(orc, t, 1, 2)
    got = np.array([m.answer(q) for q in range(m.d1.shape[0])])
    assert np.array_equal(got, m.oracle)


def test_first_appearance_is_not_feature_id_order(clustered):
    """Candidates of one Hamming level are taken in the order the bucket groups bring them up, not
    by feature id: where a level is cut at ten, or two candidates tie in the inner product (the later
    one wins), ranking by id answers differently."""
    _, _, orc = clustered
    differ = 0
    for t in (0, 1):
        m = Model(orc, t, 0, 1)
        for q in range(m.d1.shape[0]):
            c, hd = m.cand(q)
            if top_ranked(c, hd) == top_ranked(c, hd, by_id=True):
                continue
            assert m.answer(q) == m.oracle[q]
            differ += int(m.answer(q, by_id=True) != m.oracle[q])
    print("queries whose answer depends on first appearance against id order:", differ)
    assert differ >= 1


def test_heavy_rows_wrap_and_change_the_answer(clustered):
    """SIFT rows of squared norm above 65535 with an exact copy in the other view: the 16-bit state of
    the reference loses the copy's product, and the answer is not the exact search's.  Among the
    candidates of such a query are products on both sides of 65535."""
    sifts, _, orc = clustered
    changed = mixed = lanes = 0
    for a, b in ((0, 1), (1, 0), (0, 2), (2, 1)):
        m = Model(orc, 0, a, b)
        for q in cashash_cases.heavy_rows(sifts[a]):
            copy = np.nonzero((sifts[b] == sifts[a][q]).all(axis=1))[0]
            assert copy.size == 1
            assert products(sifts[a][q], sifts[b][copy], False, False)[0] > 65535
            top = top_ranked(*m.cand(q))
            assert copy[0] in top                                   # it is a candidate: same hashes
            ips = products(sifts[a][q], sifts[b][top], False, False)
            mixed += int((ips > 65535).any() and (ips <= 65535).any())
            changed += int(m.oracle[q] != m.plain(q))
            # the wrap is per LANE: forming the sum in 32 bits and truncating only the stored state
            # agrees with the reference unless a wrapped sum loses a comparison the whole sum wins
            assert m.answer(q) == m.oracle[q]
            lanes += int(m.answer(q, lanes=False) != m.oracle[q])
    print("heavy queries answered differently from exact arithmetic:", changed, "with products on both sides:", mixed,
          "from 32-bit sums with a 16-bit state:", lanes)
    assert changed >= 8 and mixed >= 4 and lanes >= 8


def test_six_to_ten_rule_meets_every_kind_of_query(clustered, tails):
    """No candidate at all, one to five, more than ten on the best Hamming level, a level that
    straddles the sixth slot -- for both descriptor types."""
    for t in (0, 1):
        kinds = dict(none=0, few=0, crowded=0, straddle=0)
        for orc, a, b in ((clustered[2], 0, 1), (tails[2], 8, 1 if t == 0 else 2), (tails[2], 9, 2), (tails[2], 9, 8),
                          (tails[2], 8, cashash_cases.TAIL_SAME_SIFT if t == 0 else cashash_cases.TAIL_SAME_SURF)):
            m = Model(orc, t, a, b)
            for q in range(m.d1.shape[0]):
                c, hd = m.cand(q)
                kinds["none"] += int(c.size == 0)
                kinds["few"] += int(1 <= c.size < MIN_CAND)
                if c.size:
                    levels, counts = np.unique(hd, return_counts=True)
                    kinds["crowded"] += int(counts[0] > MAX_CAND)
                    below = np.cumsum(counts) - counts              # candidates on lower levels
                    kinds["straddle"] += int(((below > 0) & (below < MIN_CAND) & (below + counts > MIN_CAND)).any())
        print("type", t, kinds)
        assert all(v > 0 for v in kinds.values()), (t, kinds)


# ---------------------------------------------------------------------------
# tail_views, many_small_views, limit_views
# ---------------------------------------------------------------------------
def test_tail_views_have_the_sizes(tails):
    sifts, surfs, orc = tails
    assert tuple(s.shape[0] for s in sifts) == (0, 1, 63, 64, 65, 255, 256, 257, 512, 513)
    assert {0, 1, 63, 64, 65, 256, 257} <= set(u.shape[0] for u in surfs) and surfs[0].shape[0] > 0
    # one row throughout: one bucket per group holds the whole view
    for t, v in ((0, cashash_cases.TAIL_SAME_SIFT), (1, cashash_cases.TAIL_SAME_SURF)):
        d = (sifts, surfs)[t][v]
        assert d.shape[0] >= 64 and (d == d[0]).all()
        assert (bucket_sizes(orc.local[t][v][1]).max(axis=1) == d.shape[0]).all()
    # and those rows are matched: the copies in views 8 and 9 find them
    m12, _ = orc.pairwise_match(8, cashash_cases.TAIL_SAME_SIFT)
    assert m12[300] >= 0
    assert sum(int((orc.pairwise_match(a, b)[0] >= 0).sum() >= 8) for a in range(10) for b in range(a)) >= 15


def test_many_small_views_fill_a_large_launch(many):
    sifts, surfs, orc = many
    pairs = cashash_cases.all_pairs(len(sifts))
    assert len(pairs) >= 1024
    assert max(s.shape[0] for s in sifts) <= 130 and max(u.shape[0] for u in surfs) <= 40
    assert len(set(s.shape[0] for s in sifts)) > 20 and any(u.shape[0] == 0 for u in surfs)
    good = sum(int((orc.pairwise_match(a, b)[0] >= 0).sum() >= 8) for a, b in pairs)
    print("pairs with 8 or more matches:", good, "of", len(pairs))
    assert good >= 900


def test_limit_views_sit_at_the_limit(limit):
    sifts, surfs, orc = limit
    assert sifts[0].shape[0] == (1 << 17) - 1 and (sifts[0] == sifts[0][0]).all()
    assert (bucket_sizes(orc.local[0][0][1]).max(axis=1) == sifts[0].shape[0]).all()
    m12, m21 = orc.pairwise_match(1, 0)
    # ten candidates at distance 0 in order of appearance, the last of equals wins: feature 9
    assert m12.tolist() == [-1, 9, -1] and np.nonzero(m21 >= 0)[0].tolist() == [9]


# ---------------------------------------------------------------------------
# the oracle equals the reference on these inputs
# ---------------------------------------------------------------------------
def pin(sifts, surfs, orc, pairs):
    ref = oracle_lib.RefCasHash(sifts, surfs)
    try:
        for t in (0, 1):
            for v in range(len(sifts)):
                rh, rb = ref.local(t, v)
                oh, ob = orc.local[t][v]
                assert np.array_equal(rh, oh) and np.array_equal(rb, ob), (t, v)
        for a, b in pairs:
            r12, r21 = ref.pairwise_match(a, b)
            o12, o21 = orc.pairwise_match(a, b)
            assert np.array_equal(r12, o12) and np.array_equal(r21, o21), (a, b)
    finally:
        ref.close()


@needs_ref
def test_oracle_equals_reference_on_clustered_views(clustered):
    pin(*clustered, [(a, b) for a in range(3) for b in range(3) if a != b])


@needs_ref
def test_oracle_equals_reference_on_tail_views(tails):
    pin(*tails, [(a, b) for a in range(10) for b in range(10) if a != b])


@needs_ref
def test_oracle_equals_reference_on_many_small_views(many):
    pairs = cashash_cases.all_pairs(len(many[0]))
    pick = np.random.default_rng(4201).permutation(len(pairs))[:40]
    pin(*many, [pairs[k] if k % 2 else pairs[k][::-1] for k in pick])


@needs_ref
def test_oracle_equals_reference_at_the_limit(limit):
    pin(*limit, [(0, 1), (1, 0)])
