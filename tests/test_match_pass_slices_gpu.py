"""osfm_match_all with the post-work of a call's last part cut into slices (OSFM_POST_SLICES, read per call): whatever the
number of slices, the records and the list bytes are the ones of one slice, and both are what the CPU oracle gives.

Six ragged views (300 to 900 SIFT descriptors), pairs_per_batch 4: the 15 pairs run in parts of 4, 4, 4 and 3, and the
last part -- the pairs (5,2), (5,3), (5,4) -- is the one that is sliced (2 slices: 1 + 2 pairs; 3, 5 and 64: one pair
each; 64 is also above the pairs of every part here).  What a case is meant to exercise is confirmed on the oracle's
counts before the device is touched (the premise asserts in _Case)."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib
from orthosfm_amd import synth

pytestmark = pytest.mark.gpu

SLICES = (1, 2, 3, 5, 64)
SIZES = (900, 777, 880, 300, 320, 850)
_RECORD_FIELDS = ("status", "lowres_matches", "num_matches", "num_inliers", "offset")


@pytest.fixture(scope="module")
def hm():
    # (no device call here: a test's premise is checked on the oracle before its first matcher is made)
    from orthosfm_amd.matching import HipExhaustiveMatching
    return HipExhaustiveMatching


@contextlib.contextmanager
def _slices(n):
    old = os.environ.get("OSFM_POST_SLICES")
    os.environ["OSFM_POST_SLICES"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("OSFM_POST_SLICES", None)
        else:
            os.environ["OSFM_POST_SLICES"] = old


def _all_pairs(v):
    from orthosfm_amd import capi
    return [tuple(capi.pair_from_index(i)) for i in range(v * (v - 1) // 2)]


class _Case:
    """Views, pairs and options of a call, and what the oracle says it returns: one record per pair and the lists
    back to back (bundler_matching.cc up to RANSAC: low-res gate, count threshold, ordered correspondences)."""

    def __init__(self, sift, surf=None, pairs=None, **options):
        from orthosfm_amd import capi
        self.sift = sift
        self.surf = surf if surf is not None else [np.zeros((0, 64), np.int16) for _ in sift]
        self.pairs = pairs if pairs is not None else _all_pairs(len(sift))
        self.opts = capi.default_match_options()
        self.opts.pairs_per_batch = 4
        for k, v in options.items():
            setattr(self.opts, k, v)
        o = self.opts
        rec, lists, written = [], [], 0
        for a, b in self.pairs:
            s1, u1, s2, u2 = self.sift[a], self.surf[a], self.sift[b], self.surf[b]
            low = -1
            if o.use_lowres_matching and (len(s1) + len(u1)) * (len(s2) + len(u2)) > 1000000:
                low = oracle_lib.oracle_pairwise_match_lowres(s1, u1, s2, u2, o.num_lowres_features)
                if low < o.min_lowres_matches:
                    rec.append((capi.PAIR_REJECTED_LOWRES, low, 0, -1, 0))
                    continue
            e12, _ = oracle_lib.oracle_pairwise_match(s1, u1, s2, u2)
            idx = np.nonzero(e12 >= 0)[0]
            if len(idx) < max(8, o.min_feature_matches):
                rec.append((capi.PAIR_REJECTED_COUNT, low, len(idx), -1, 0))
                continue
            rec.append((capi.PAIR_MATCHED, low, len(idx), -1, written))
            lists.append(np.stack([idx, e12[idx]], axis=1).astype(np.int32))
            written += len(idx)
        self.records = rec
        self.flat = np.concatenate(lists + [np.zeros((0, 2), np.int32)])
        self.status = [r[0] for r in rec]

    def matcher(self, hm):
        m = hm(len(self.sift), options=self.opts)
        for v in range(len(self.sift)):
            m.set_view(v, self.sift[v], self.surf[v] if len(self.surf[v]) else None)
        return m

    def check(self, ra, flat, what):
        got = [tuple(int(r[f]) for f in _RECORD_FIELDS) for r in ra]
        assert got == self.records, what
        assert np.asarray(flat).tobytes() == self.flat.tobytes(), what


def _run_all_settings(hm, case, settings=SLICES):
    """The call under every slice setting on one matcher: equal to the oracle, and byte for byte to one another."""
    m = case.matcher(hm)
    first = None
    for n in settings:
        with _slices(n):
            ra, _ = m.compute_arrays(case.pairs)
        flat = np.array(m.last_flat)
        case.check(ra, flat, f"OSFM_POST_SLICES={n}")
        if first is None:
            first = (ra.tobytes(), flat.tobytes())
        assert (ra.tobytes(), flat.tobytes()) == first, n
    return m


_sets = {}


def _base():
    if "base" not in _sets:
        iset = synth.make_image_set(6, 900, config_id=41)
        _sets["base"] = (iset, [iset.sift[v][:n].copy() for v, n in enumerate(SIZES)])
    return _sets["base"]


def _kept(case):
    from orthosfm_amd import capi
    return [s == capi.PAIR_MATCHED for s in case.status]


def test_a_all_pairs_kept(hm):
    case = _Case(_base()[1])
    assert all(_kept(case)) and len(case.records) == 15 and min(r[2] for r in case.records) >= 50
    _run_all_settings(hm, case).close()


def test_b_slices_that_keep_no_pair(hm):
    """min_feature_matches between the counts of (5,2) and of (5,3), (5,4), the two short views: of the last part only
    its first pair is kept, so with 3 slices the middle slice and the last slice keep nothing (and with 2 the last)."""
    plain = _Case(_base()[1])
    c52, c53, c54 = (plain.records[k][2] for k in (12, 13, 14))
    assert plain.pairs[12:] == [(5, 2), (5, 3), (5, 4)] and c52 > max(c53, c54) + 1
    case = _Case(_base()[1], min_feature_matches=max(c53, c54) + 1)
    kept = _kept(case)
    assert kept[12:] == [True, False, False] and any(kept[:12]) and not all(kept[:12])
    _run_all_settings(hm, case).close()
    # the other way round: only the last pair's slice keeps nothing ... and a last part that keeps nothing at all
    none = _Case(_base()[1], min_feature_matches=c52 + 1)
    assert _kept(none)[12:] == [False, False, False] and any(_kept(none))
    _run_all_settings(hm, none).close()


def test_c_pairs_that_fall_at_the_lowres_gate(hm):
    """SURF beside the SIFT lifts every pair above the 10^6 products of the low-res gate; view 4 shows another scene,
    so its five pairs end there and the full matching sees 10 pairs in parts of 4, 4 and 2 (both descriptor types)."""
    from orthosfm_amd import capi
    if "gate" not in _sets:
        iset = synth.make_image_set(6, 900, n_surf=750, config_id=42)
        rr = np.random.default_rng(9)
        sift = [iset.sift[v][:n].copy() for v, n in enumerate(SIZES)]
        surf = [iset.surf[v].copy() for v in range(6)]
        sift[4] = synth.quantize_sift(synth.sift_like(rr.standard_normal((SIZES[4], 128))))
        surf[4] = synth.quantize_surf(synth.surf_like(rr.standard_normal((750, 64))))
        _sets["gate"] = (sift, surf)
    case = _Case(*_sets["gate"])
    st = case.status
    assert all(r[1] >= 0 for r in case.records), "every pair goes through the gate"
    gated = [k for k, s in enumerate(st) if s == capi.PAIR_REJECTED_LOWRES]
    assert gated == [k for k, p in enumerate(case.pairs) if 4 in p] and len(gated) == 5
    assert st.count(capi.PAIR_MATCHED) == 10
    _run_all_settings(hm, case).close()


def test_d_capacity_exact_and_one_short(hm):
    from orthosfm_amd import capi
    case = _Case(_base()[1])
    total, guard = len(case.flat), 64
    m = case.matcher(hm)
    for n in SLICES:
        buf = np.full((total + guard, 2), -5, np.int32)
        m.use_result_buffer(buf)
        with _slices(n):
            ra, _ = m.compute_arrays(case.pairs, capacity=total)
        case.check(ra, buf[:total], n)
        assert np.all(buf[total:] == -5), n
        buf[:] = -5
        with _slices(n), pytest.raises(capi.OsfmError) as e:
            m.compute_arrays(case.pairs, capacity=total - 1)
        assert e.value.status == capi.E_CAPACITY and str(total) in str(e.value), (n, str(e.value))
        assert np.all(buf[total - 1:] == -5), n
        # what did arrive lies where the full result has it
        arrived = np.any(buf[:total - 1] != -5, axis=1)
        assert np.array_equal(buf[:total - 1][arrived], case.flat[:total - 1][arrived]), n
    m.close()


def test_e_special_jobs_and_exact_scans_across_slices(hm):
    """Descriptors with bytes above 127 in views 2 and 5 (special jobs in every slice of the last part, whose pairs all
    name view 5), and one descriptor of two bins of 255 in views 2 to 5: its inner product with itself, 130050, leaves
    the 16-bit range, so in every pair of these views -- every slice of the last part among them -- a query of either
    direction goes through the wrap-exact scan, whose item list the slices share and whose counters they do not."""
    if "peaky" not in _sets:
        iset = synth.make_image_set(6, 900, config_id=41)
        plain = [s.copy() for s in iset.sift]
        synth.add_peaky_rows(iset, 40)
        sift = [iset.sift[v] if v in (2, 5) else plain[v] for v in range(6)]
        sift = [sift[v][:n].copy() for v, n in enumerate(SIZES)]
        wide = np.zeros(128, np.uint16)
        wide[[3, 77]] = 255
        for v, row in ((2, 7), (3, 290), (4, 8), (5, 11)):
            sift[v][row] = wide
        assert all(int((sift[v] > 127).any(axis=1).sum()) >= 20 for v in (2, 5))
        assert not any((sift[v] > 127).any() for v in (0, 1))
        for a, b in ((5, 2), (5, 3), (5, 4), (4, 3)):
            assert (sift[a].astype(np.int64) @ sift[b].astype(np.int64).T).max() > 65535
        _sets["peaky"] = sift
    case = _Case(_sets["peaky"])
    assert all(_kept(case))
    m = _run_all_settings(hm, case)
    for n in (1, 3):
        with _slices(n):
            m.compute_arrays(case.pairs[12:])      # the last part alone: (5,2), (5,3), (5,4)
        st = m.stats()
        assert st.special_kernel_launches > 0 and st.exact_scan_queries >= 6, (n, st.exact_scan_queries)
    m.close()


def test_f_page_locked_and_pageable_result_buffers(hm):
    from orthosfm_amd import capi
    case = _Case(_base()[1])
    rows = len(case.flat) + 8
    m = case.matcher(hm)
    pinned = capi.pinned_rows(rows)
    for kind, buf in (("page-locked", pinned), ("pageable", np.empty((rows, 2), np.int32))):
        for n in SLICES:
            buf[:] = -5
            m.use_result_buffer(buf)
            with _slices(n):
                ra, _ = m.compute_arrays(case.pairs, capacity=rows)
            case.check(ra, buf[:len(case.flat)].copy(), (kind, n))
            assert np.all(buf[len(case.flat):] == -5), (kind, n)
    m.close()
    # (given back only when everything held: a failure report still prints the arrays above)
    m.use_result_buffer(np.empty((1, 2), np.int32))
    del buf
    assert capi.pinned_free(pinned)


def test_g_verification_is_untouched_by_the_knob(hm):
    """With geometric verification nothing is sliced: every setting gives the bytes of the first."""
    from orthosfm_amd import capi
    iset, sift = _base()
    o = capi.default_match_options()
    o.pairs_per_batch = 4
    o.geometric_verification = 1
    m = hm(6, options=o)
    for v in range(6):
        m.set_view(v, sift[v])
        xy = (iset.pos[v][:SIZES[v]] + 0.5 - np.array([iset.width / 2, iset.height / 2])) / max(iset.width, iset.height)
        m.set_positions(v, xy.astype(np.float32))
    first = None
    for n in SLICES:
        with _slices(n):
            ra, _ = m.compute_arrays()
        got = (ra.tobytes(), np.array(m.last_flat).tobytes())
        first = first or got
        assert got == first, n
    assert (ra["status"] == capi.PAIR_MATCHED).sum() >= 10 and len(m.last_flat) > 500
    m.close()


def test_h_one_matcher_large_small_large(hm):
    """Staging blocks, plan copies and slice events of one matcher reused by calls of different sizes."""
    big = _Case(_base()[1])
    small = _Case(_base()[1], pairs=[(3, 1), (5, 4)])
    m = big.matcher(hm)
    for n in (3, 1, 64):
        with _slices(n):
            for _ in range(2):
                for case in (big, small, big):
                    ra, _ = m.compute_arrays(case.pairs)
                    case.check(ra, np.array(m.last_flat), (n, len(case.pairs)))
    m.close()


def test_i_single_pair_and_exactly_one_part(hm):
    one = _Case(_base()[1], pairs=[(4, 2)])
    part = _Case(_base()[1], pairs=[(1, 0), (2, 0), (5, 3), (4, 1)])
    assert all(_kept(one)) and all(_kept(part))
    _run_all_settings(hm, one).close()
    _run_all_settings(hm, part).close()


def test_j_default_slices_of_a_large_part(hm):
    """The knob unset: 15 views, 105 pairs in one part (pairs_per_batch 0), which is above the 96 pairs from which the
    default is 3 slices of 35 pairs; equal to the oracle and to the explicit settings 1 and 3."""
    iset = synth.make_image_set(15, 400, config_id=43)
    case = _Case([s.copy() for s in iset.sift], pairs_per_batch=0)
    assert len(case.pairs) == 105 and any(_kept(case)) and len(case.flat) > 1000
    m = case.matcher(hm)
    old = os.environ.pop("OSFM_POST_SLICES", None)
    try:
        ra, _ = m.compute_arrays(case.pairs)
    finally:
        if old is not None:
            os.environ["OSFM_POST_SLICES"] = old
    flat = np.array(m.last_flat)
    case.check(ra, flat, "knob unset")
    for n in (1, 3):
        with _slices(n):
            rb, _ = m.compute_arrays(case.pairs)
        assert (rb.tobytes(), np.array(m.last_flat).tobytes()) == (ra.tobytes(), flat.tobytes()), n
    m.close()
