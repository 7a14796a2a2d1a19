"""The SIFT finish's bucketed rescoring (match_rescore_kernel) against the per-query rescan it
replaces (OSFM_FINISH_RESCAN=wave, read per batch) and against the CPU oracle.

The winning groups of the raw tile kernels are rescored by bucket -- column queries by
(row block, 64-row strip), row queries by (lane slot, window of starting tiles) -- and everything
else keeps the in-kernel rescan.  Both must give the same m12 / m21 bit for bit.
"""
import contextlib
import os

import numpy as np
import pytest

import match_cases
import oracle_lib
from orthosfm_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    assert capi.device_count() >= 1, "no HIP device"
    return HipExhaustiveMatching


@contextlib.contextmanager
def _rescan(mode):
    old = os.environ.get("OSFM_FINISH_RESCAN")
    if mode is None:
        os.environ.pop("OSFM_FINISH_RESCAN", None)
    else:
        os.environ["OSFM_FINISH_RESCAN"] = mode
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("OSFM_FINISH_RESCAN", None)
        else:
            os.environ["OSFM_FINISH_RESCAN"] = old


def _both(fn):
    """fn() with the bucketed rescoring (default) and with the per-query rescan."""
    with _rescan(None):
        new = fn()
    with _rescan("wave"):
        old = fn()
    return new, old


def _pair_lists(m, a, b):
    two = m.twoway_match(a, b, 0)
    got = m.pairwise_match(a, b)
    return two.matches_1_2, two.matches_2_1, got.matches_1_2, got.matches_2_1


def _check_pair(hm, s1, s2, oracle=True, options=None):
    m = hm(2, options=options) if options is not None else hm(2)
    m.set_view(0, s1)
    m.set_view(1, s2)
    new, old = _both(lambda: _pair_lists(m, 0, 1))
    m.close()
    for x, y, name in zip(new, old, ("e12", "e21", "c12", "c21")):
        assert np.array_equal(x, y), name
    if oracle:
        om = oracle_lib.oracle_matcher()
        e12, e21 = om.twoway(s1, s2, 0.8)
        c12, c21 = om.remove_inconsistent(e12, e21)
        for x, y, name in zip(new, (e12, e21, c12, c21), ("e12", "e21", "c12", "c21")):
            assert np.array_equal(x, y), name
    return new


@pytest.mark.parametrize("n1,n2,seed", [(1999, 3001, 1), (4133, 700, 2), (257, 6271, 3), (2111, 2113, 4)])
def test_odd_shapes_against_rescan_and_oracle(hm, n1, n2, seed):
    """n1 / n2 not multiples of 64 or 256: partial row blocks, partial tiles, groups that run past n2."""
    s1, s2 = match_cases.sift_pair(n1, n2, min(n1, n2) // 2, 900 + seed)
    _check_pair(hm, s1, s2)


def test_full_size_pair(hm):
    """20000 x 20000 through the per-pair entry (a single pair is cut into 20 column segments, so
    row groups cross segment ends), new path against the rescan and the oracle."""
    iset = synth.make_image_set(2, 20000, config_id=2)
    new = _check_pair(hm, iset.sift[0], iset.sift[1])
    assert int((new[2] >= 0).sum()) > 5000


def test_duplicated_descriptors(hm):
    """Ties inside a group and one bucket that holds most queries of the pair (more than it has
    room for: the rest goes through the per-query rescan)."""
    r = np.random.default_rng(77)
    s1, s2 = match_cases.sift_pair(3000, 3000, 1500, 1234)
    # set 2: 2000 noisy copies of set 1's rows 0 .. 31 -- their best rows all lie in one 64-row strip
    src = r.integers(0, 32, 2000)
    noisy = s1[src].astype(np.int32) + r.integers(-2, 3, (2000, 128))
    s2[:2000] = np.clip(noisy, 0, 127).astype(np.uint16)
    # exact duplicates 32 and 64 columns apart: equal candidates inside one row group
    for c in range(2000, 2900, 128):
        s2[c + 32] = s2[c]
        s2[c + 64] = s2[c]
    # and repeated rows in set 1
    s1[1000:1100] = s1[1000]
    _check_pair(hm, s1, s2)


def test_special_descriptors_mixed_in(hm):
    """Rows and columns with bytes > 127 (special descriptors) next to the rescored groups."""
    s1, s2 = match_cases.sift_pair(5000, 4500, 2500, 4321)
    r = np.random.default_rng(5)
    for s in (s1, s2):
        for k in r.choice(s.shape[0], 120, replace=False):
            s[k, r.choice(128, 2, replace=False)] = [int(r.integers(128, 256)), int(r.integers(128, 200))]
    _check_pair(hm, s1, s2)
    from orthosfm_amd import capi
    o = capi.default_match_options()
    o.special_kernel_max = -1          # the per-view operand forms: special row blocks, corrected columns
    _check_pair(hm, s1, s2, oracle=False, options=o)


def test_batch_with_surf_and_ragged_views(hm):
    """A multi-pair compute() over ragged views with SURF riding along (the SURF and keyed groups keep
    the per-query rescan): every list equal under both paths and to the oracle."""
    from orthosfm_amd import capi
    sizes = [700, 3001, 5000, 1025, 4200]
    base = synth.make_image_set(len(sizes), 5000, n_surf=300, config_id=15, twin_frac=0.2)
    sift = [base.sift[v][:n].copy() for v, n in enumerate(sizes)]
    o = capi.default_match_options()
    o.use_lowres_matching = 0
    o.min_feature_matches = 0

    def run():
        m = hm(len(sizes), options=o)
        for v in range(len(sizes)):
            m.set_view(v, sift[v], base.surf[v])
        out = m.compute()
        res = {(tv.view_1_id, tv.view_2_id): (tv.status, np.asarray(tv.matches).reshape(-1, 2).copy()) for tv in out}
        m.close()
        return res

    new, old = _both(run)
    assert new.keys() == old.keys() and len(new) == len(sizes) * (len(sizes) - 1) // 2
    for k in new:
        assert new[k][0] == old[k][0] and np.array_equal(new[k][1], old[k][1]), k
    for (a, b), (status, got) in new.items():
        e12, _ = oracle_lib.oracle_pairwise_match(sift[a], base.surf[a], sift[b], base.surf[b])
        idx = np.nonzero(e12 >= 0)[0]
        expect = np.stack([idx, e12[idx]], axis=1).astype(np.int32)
        if status == capi.PAIR_MATCHED:
            assert np.array_equal(got, expect), (a, b)
