"""GPU tests of the cascade-hashing kernels where they change path, through the C ABI,
bit for bit against the oracle (oracle/cashash_oracle.c, pinned to the reference on
these very inputs in tests/test_cashash_cases_cpu.py, which also shows that the inputs
reach the paths named here):

  clustered_views    buckets of several candidate chunks with odd tails, ties in the
                     Hamming distance, exact duplicates, SIFT products beyond 16 bits;
  tail_views         the preparation kernels at 0, 1, 63 .. 65, 255 .. 257, 512, 513 rows,
                     64 lanes of one bucket id, pairs with an empty side;
  many_small_views   1035 pairs per launch down to 16: 64 .. 1 buckets per workgroup;
  limit_views        2^17 - 1 descriptors in one bucket, and the refusal of one more."""
import numpy as np
import pytest

import cashash_cases
import oracle_lib

pytestmark = pytest.mark.gpu


def matcher(sifts, surfs, device=0, **options):
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipCascadeHashing
    assert capi.device_count() >= 1
    o = capi.default_match_options()
    for k, v in options.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    m = HipCascadeHashing(len(sifts), device=device, options=o)
    for v in range(len(sifts)):
        m.set_view(v, sifts[v], surfs[v])
    return m


def check_hashes(m, orc, num_views):
    for t in (0, 1):
        for v in range(num_views):
            h, b = m.cascade_hashes(v, t)
            oh, ob = orc.local[t][v]
            assert h.shape == oh.shape and np.array_equal(h, oh), (t, v)
            assert b.shape == ob.shape and np.array_equal(b, ob.astype(np.uint8)), (t, v)


def check_pair(m, orc, a, b, **kw):
    got = m.pairwise_match(a, b)
    o12, o21 = orc.pairwise_match(a, b, **kw)
    for name, g, o in (("1_2", got.matches_1_2, o12), ("2_1", got.matches_2_1, o21)):
        assert g.shape == o.shape, (a, b, name, g.shape, o.shape)
        if not np.array_equal(g, o):
            bad = np.nonzero(g != o)[0]
            raise AssertionError(f"pair ({a}, {b}) matches_{name}: {bad.size} of {o.size} entries differ, first at "
                                 f"{bad[:8].tolist()}: got {g[bad[:8]].tolist()}, oracle {o[bad[:8]].tolist()}")
    return o12


# ---------------------------------------------------------------------------
def test_clustered_views_bit_exact():
    sifts, surfs = cashash_cases.clustered_views()
    orc = oracle_lib.OracleCasHash(sifts, surfs)
    m = matcher(sifts, surfs)
    try:
        check_hashes(m, orc, 3)
        for a in range(3):
            for b in range(3):
                if a != b:
                    o12 = check_pair(m, orc, a, b)
                    assert (o12 >= 0).sum() > 50, (a, b)
    finally:
        m.close()


@pytest.fixture(scope="module")
def tails():
    sifts, surfs = cashash_cases.tail_views()
    return sifts, surfs, oracle_lib.OracleCasHash(sifts, surfs)


@pytest.mark.parametrize("keep_empty_blocks", (0, 1))
def test_tail_views_bit_exact(tails, keep_empty_blocks):
    """Every view size at which a preparation kernel changes path in ONE matcher (the average runs
    over all of them), every ordered pair of them -- an empty side, a single row, a view of one
    repeated row included -- in the reference's layout and in the exhaustive matcher's."""
    sifts, surfs, orc = tails
    m = matcher(sifts, surfs, cascade_keep_empty_blocks=keep_empty_blocks)
    try:
        check_hashes(m, orc, len(sifts))
        matched = 0
        for a in range(len(sifts)):
            for b in range(len(sifts)):
                if a != b:
                    matched += int((check_pair(m, orc, a, b, keep_empty_blocks=bool(keep_empty_blocks)) >= 0).sum())
        assert matched > 1000
    finally:
        m.close()


# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    sifts, surfs = cashash_cases.many_small_views()
    orc = oracle_lib.OracleCasHash(sifts, surfs)
    pairs = cashash_cases.all_pairs(len(sifts))
    want = [orc.pairwise_match(a, b)[0] for a, b in pairs]
    return sifts, surfs, pairs, want


def expected_launches(sifts, surfs, pairs, per_batch):
    """cashash_kernel_launches of one compute(): one per batch and descriptor type with a problem in
    it -- a pair has one of a type when both of its views have descriptors of that type."""
    per_batch = per_batch if per_batch > 0 else len(pairs)
    n = 0
    for start in range(0, len(pairs), per_batch):
        part = pairs[start:start + per_batch]
        n += any(sifts[a].shape[0] and sifts[b].shape[0] for a, b in part)
        n += any(surfs[a].shape[0] and surfs[b].shape[0] for a, b in part)
    return n


def run_many(many, per_batch, device=0):
    sifts, surfs, pairs, _ = many
    m = matcher(sifts, surfs, device=device, use_lowres_matching=0, min_feature_matches=8, pairs_per_batch=per_batch)
    try:
        before = m.stats().cashash_kernel_launches
        ra, _ = m.compute_arrays(pairs)
        launches = m.stats().cashash_kernel_launches - before
        return ra.copy(), m.last_flat.copy(), launches
    finally:
        m.close()


def test_buckets_per_workgroup_1_to_64(many):
    """All 1035 pairs in one launch (64 buckets per workgroup for SIFT), in launches of 600 and 435
    (32 and 16), of 40 (2) and of 16 (1): the same records and the same bytes, and they are the
    oracle's.  The launch counter shows that the batches were what this test takes them for."""
    from orthosfm_amd import capi
    sifts, surfs, pairs, want = many
    assert len(pairs) == 1035
    runs = {}
    for per_batch in (0, 600, 40, 16):
        ra, flat, launches = run_many(many, per_batch)
        assert launches == expected_launches(sifts, surfs, pairs, per_batch), (per_batch, launches)
        runs[per_batch] = (ra, flat)
    assert expected_launches(sifts, surfs, pairs, 0) == 2 and expected_launches(sifts, surfs, pairs, 16) >= 120
    ra, flat = runs[0]
    for per_batch, (rb, fb) in runs.items():
        assert ra.tobytes() == rb.tobytes(), per_batch
        assert flat.shape == fb.shape and flat.tobytes() == fb.tobytes(), per_batch
    matched = 0
    for k, (o12, rec) in enumerate(zip(want, ra)):
        idx = np.nonzero(o12 >= 0)[0]
        assert rec["num_matches"] == idx.size, (pairs[k], int(rec["num_matches"]), idx.size)
        assert rec["status"] == (capi.PAIR_MATCHED if idx.size >= 8 else capi.PAIR_REJECTED_COUNT), pairs[k]
        if rec["status"] == capi.PAIR_MATCHED:
            got = flat[rec["offset"]:rec["offset"] + idx.size]
            assert np.array_equal(got, np.stack([idx, o12[idx]], axis=1).astype(np.int32)), pairs[k]
            matched += 1
    assert 900 <= matched < len(pairs)          # and some pairs do fall below the threshold


def test_two_shards_equal_one_device(many):
    """The same set and pair list through two logical shards of device 0."""
    ra, flat, _ = run_many(many, 0)
    rb, fb, _ = run_many(many, 0, device=[0, 0])
    assert ra.tobytes() == rb.tobytes()
    assert flat.shape == fb.shape and flat.tobytes() == fb.tobytes()


# ---------------------------------------------------------------------------
def test_view_at_the_size_limit_and_one_past_it():
    """2^17 - 1 copies of one row: every bucket list position the candidate keys can hold, in one
    bucket per group; the ten winners are the first ten by appearance.  One descriptor more is
    refused with the library's range error before anything is launched for it, and the matcher
    answers again once the view has been replaced."""
    from orthosfm_amd import capi
    sifts, surfs = cashash_cases.limit_views()
    assert sifts[0].shape[0] == cashash_cases.LIMIT == 131071
    orc = oracle_lib.OracleCasHash(sifts, surfs)
    m = matcher(sifts, surfs)
    try:
        check_hashes(m, orc, 2)
        assert check_pair(m, orc, 1, 0).tolist() == [-1, 9, -1]
        check_pair(m, orc, 0, 1)
        over = cashash_cases.limit_views(cashash_cases.LIMIT + 1)[0][0]
        m.set_view(0, over, surfs[0])
        with pytest.raises(capi.OsfmError) as e:
            m.pairwise_match(0, 1)
        assert e.value.status == capi.E_RANGE and "131072" in str(e.value)
        with pytest.raises(capi.OsfmError) as e:
            m.cascade_hashes(1, 0)
        assert e.value.status == capi.E_RANGE
        legal = [np.ascontiguousarray(sifts[0][:1000]), sifts[1]]
        m.set_view(0, legal[0], surfs[0])
        orc2 = oracle_lib.OracleCasHash(legal, surfs)
        check_hashes(m, orc2, 2)
        assert check_pair(m, orc2, 1, 0).tolist() == [-1, 9, -1]
        check_pair(m, orc2, 0, 1)
    finally:
        m.close()
