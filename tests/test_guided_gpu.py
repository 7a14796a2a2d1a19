"""osfm_match_guided against its restatement (tests/guided_restatement.py): record, list and F_out equal in every byte
on every case of tests/guided_cases.py -- the band's edge, the candidate counts around candidates_per_pass, view sizes
around the workgroup's queries and the staged chunk, ties, both descriptor types, special SIFT rows and products that
do not fit T, the cap, F given or fitted, the statuses -- and batching, repetition, capacity and validation.  The power
of the restatement and of the cases is shown without a device in tests/test_guided_cases_cpu.py."""
import numpy as np
import pytest

import guided_cases as GC
import guided_restatement as G

pytestmark = pytest.mark.gpu


def _limits():
    try:
        from orthosfm_amd import capi
        return capi.guided_limits()
    except Exception:            # collection without the library: the names below are then those of the defaults
        return GC.DEFAULT_LIMITS


_cases = {}


def _case(name):
    if not _cases:
        _cases.update({c.name: c for c in GC.cases(_limits())})
    return _cases[name]


NAMES = [c.name for c in GC.cases(_limits())]


@pytest.fixture(scope="module")
def hm():
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    assert capi.device_count() >= 1
    return HipExhaustiveMatching


def _matcher(hm, views, device=0, cls=None):
    m = (cls or hm)(len(views), device=device)
    for v, vw in enumerate(views):
        m.set_view(v, vw.sift, vw.surf if vw.surf.shape[0] else None)
        m.set_positions(v, vw.pos)
    return m


def _call(hm, c, device=0, cls=None):
    m = _matcher(hm, [c.view1, c.view2], device, cls)
    try:
        return m.guided_match([(0, 1)], [0, c.seeds.shape[0]], c.seeds, None if c.F is None else np.asarray(c.F)[None], **c.options)
    finally:
        m.close()


def _equal(rec, lst, F, want, what):
    got = (int(rec["status"]), int(rec["num_seeds"]), int(rec["num_added"]), int(rec["max_candidates"]))
    exp = (want["status"], want["num_seeds"], want["num_added"], want["max_candidates"])
    assert got == exp, (what, got, exp)
    assert lst.dtype == np.int32 and np.array_equal(lst, want["list"]), what
    assert np.asarray(F).tobytes() == want["F"].tobytes(), (what, F, want["F"])


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_restatement(hm, name):
    c = _case(name)
    want = G.run(c.view1, c.view2, c.seeds, c.F, **c.options)
    rec, corr, F = _call(hm, c)
    assert int(rec[0]["offset"]) == 0 and corr.shape[0] == want["list"].shape[0]
    _equal(rec[0], corr, F[0], want, name)


def test_limits_are_the_kernels():
    from orthosfm_amd import capi
    q, ch, p = capi.guided_limits()
    assert q >= 1 and p >= 2 and ch >= p and ch % 64 == 0
    assert {f"size_{q - 1}_{q + 1}", f"size_{ch + 1}_{ch - 1}", "counts"} <= set(NAMES)


def test_multi_device_handle_and_cascade_matcher(hm):
    """a handle of osfm_match_create_multi runs the call on its first shard; the matcher type does not matter"""
    from orthosfm_amd.matching import HipCascadeHashing
    c = _case("twin_fit")
    want = G.run(c.view1, c.view2, c.seeds, c.F, **c.options)
    for kw in (dict(device=[0, 0]), dict(cls=HipCascadeHashing)):
        rec, corr, F = _call(hm, c, **kw)
        _equal(rec[0], corr, F[0], want, str(kw))


def test_batch_equals_single_calls_and_repeats(hm):
    views, pairs, seeds = GC.batch_set()
    assert len(pairs) == 40
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in seeds])]).astype(np.int64)
    m = _matcher(hm, views)
    try:
        rec, corr, F = m.guided_match(pairs, off, np.concatenate(seeds))
        rec2, corr2, F2 = m.guided_match(pairs, off, np.concatenate(seeds))
        assert rec.tobytes() == rec2.tobytes() and corr.tobytes() == corr2.tobytes() and F.tobytes() == F2.tobytes()
        assert int(rec["num_added"].sum()) > 100
        for k, (p, s) in enumerate(zip(pairs, seeds)):
            r1, c1, F1 = m.guided_match([p], [0, s.shape[0]], s)
            lo = int(rec[k]["offset"])
            n = int(rec[k]["num_seeds"] + rec[k]["num_added"])
            assert [int(r1[0][f]) for f in ("status", "num_seeds", "num_added", "max_candidates")] == \
                   [int(rec[k][f]) for f in ("status", "num_seeds", "num_added", "max_candidates")], k
            assert np.array_equal(c1, corr[lo:lo + n]) and F1[0].tobytes() == F[k].tobytes(), k
        # three of them against the restatement as well: the batch is not merely consistent with itself
        for k in (0, 17, 39):
            a, b = pairs[k]
            want = G.run(views[a], views[b], seeds[k])
            lo = int(rec[k]["offset"])
            _equal(rec[k], corr[lo:lo + want["list"].shape[0]], F[k], want, f"pair {k}")
        # capacity: the total is reported, nothing else
        from orthosfm_amd import capi
        with pytest.raises(capi.OsfmError) as e:
            m.guided_match(pairs, off, np.concatenate(seeds), capacity=corr.shape[0] - 1)
        assert e.value.status == capi.E_CAPACITY and m.last_guided_total == corr.shape[0]
        m.guided_match(pairs, off, np.concatenate(seeds), capacity=corr.shape[0])
    finally:
        m.close()


def test_validation(hm):
    from orthosfm_amd import capi
    c = _case("types_both")
    ns1, ns2 = c.view1.sift.shape[0], c.view2.sift.shape[0]
    m = hm(4, device=0)
    try:
        for v, vw in enumerate((c.view1, c.view2)):
            m.set_view(v, vw.sift, vw.surf)
        m.set_view(2, c.view1.sift, c.view1.surf)
        m.set_positions(0, c.view1.pos)
        m.set_positions(1, c.view2.pos)

        def bad(pairs, off, seeds, **kw):
            with pytest.raises(capi.OsfmError) as e:
                m.guided_match(pairs, off, seeds, np.repeat(c.F[None], len(pairs), axis=0), capacity=1000, **kw)
            assert e.value.status == capi.E_ARG, e.value

        none = np.zeros((0, 2), np.int32)
        bad([(0, 2)], [0, 0], none)                                     # a view without positions
        bad([(0, 1)], [0, 1], [[0, c.view2.n]])                         # a seed out of range
        bad([(0, 1)], [0, 1], [[-1, 0]])
        bad([(0, 1)], [0, 2], [[0, 0], [0, 1]])                         # a feature twice
        bad([(0, 1)], [0, 2], [[0, 1], [1, 1]])
        bad([(0, 1)], [0, 1], [[0, ns2]])                               # SIFT row joined to a SURF row
        bad([(0, 1)], [0, 1], [[ns1, 0]])
        bad([(0, 1), (0, 1)], [0, 1, 0], [[0, 0]])                      # offsets that decrease
        bad([(0, 1)], [0, 0], none, threshold=0.0)                      # threshold not > 0
        bad([(0, 1)], [0, 0], none, threshold=float("nan"))
        bad([(0, 3)], [0, 0], none)                                     # a view without features set
        bad([(0, 4)], [0, 0], none)                                     # no such view
        # the same feature in the seeds of two PAIRS of a call is fine
        rec, _, _ = m.guided_match([(0, 1), (0, 1)], [0, 1, 2], [[0, 0], [0, 0]], np.repeat(c.F[None], 2, axis=0))
        assert rec["status"].tolist() == [0, 0]
    finally:
        m.close()
