"""guided=True through pipeline.match_and_build_tracks on the twin set of the issue (synth.make_image_set(3, 400,
seed=11, twin_frac=0.5, visibility=0.6), verify="affine", both count gates at 8): with guided=False nothing changes; with
it every pair keeps its seeds, every addition lies in the band of the pair's F, the lists are ascending and one-to-one,
and at least 0.9 of the additions join two features of one landmark (tests/test_guided_cases_cpu.py shows the
restatement itself to stay within that on this set, fed with the affine RANSAC's inliers)."""
import numpy as np
import pytest

import affine_restatement as A
import guided_cases as GC

pytestmark = pytest.mark.gpu

PAIRS = [(1, 0), (2, 0), (2, 1)]


@pytest.fixture(scope="module")
def runs():
    from orthosfm_amd import capi, pipeline as P
    iset = GC.image_set(**GC.TWIN)

    def options():
        o = capi.default_match_options()
        o.min_feature_matches, o.min_matching_inliers = 8, 8
        return o

    plain = P.match_and_build_tracks(iset, verify="affine", options=options())
    off = P.match_and_build_tracks(iset, verify="affine", options=options(), guided=False)
    tm = P.Timings()
    on = P.match_and_build_tracks(iset, verify="affine", options=options(), guided=True, timings=tm)
    P.join_background()
    return iset, plain, off, on, tm, options


def _same_tracks(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("offsets", "view", "feat", "xy"))


def test_guided_false_is_todays_call(runs):
    _, (tt0, info0), (tt1, info1), _, _, _ = runs
    assert _same_tracks(tt0, tt1)
    assert "guided" not in info1 and set(info0) == set(info1)
    for k in info0:
        if k == "match_stats":
            continue                    # device times of the call
        assert np.array_equal(info0[k], info1[k]), k


def test_guided_lists(runs):
    """the matcher's own lists of the three pairs, guided, held to the properties; the pipeline's counts agree with them"""
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    iset, (tt0, info0), _, (tt2, info2), tm, options = runs
    o = options()
    o.geometric_verification, o.ransac_model = 1, capi.RANSAC_AFFINE
    m = HipExhaustiveMatching(3, options=o)
    try:
        pos = [GC.norm_pos(iset, v) for v in range(3)]
        for v in range(3):
            m.set_view(v, iset.sift[v])
            m.set_positions(v, pos[v])
        ra, corr = m.compute_arrays(PAIRS)
        assert (ra["status"] == capi.PAIR_MATCHED).all()
        ga, gcorr, F = m.guided_arrays(PAIRS, ra, corr)
        sel, gres = m.last_guided
    finally:
        m.close()
    added_all = true_all = 0
    for k, (v1, v2) in enumerate(PAIRS):
        seeds = corr[ra[k]["offset"]:ra[k]["offset"] + ra[k]["num_inliers"]]
        lst = gcorr[ga[k]["offset"]:ga[k]["offset"] + ga[k]["num_inliers"]]
        have = set(map(tuple, lst.tolist()))
        assert set(map(tuple, seeds.tolist())) <= have                                 # every seed is kept
        assert (np.diff(lst[:, 0]) > 0).all() and np.unique(lst[:, 1]).size == lst.shape[0]      # ascending, one-to-one
        added = np.array(sorted(have - set(map(tuple, seeds.tolist()))), np.int64).reshape(-1, 2)
        assert added.shape[0] == gres[k]["num_added"] >= 1
        v = np.array([F[k][0, 2], F[k][1, 2], F[k][2, 0], F[k][2, 1], F[k][2, 2]])
        m1, m2 = A.matches(pos[v1], pos[v2], added)
        assert A.below(v, m1, m2, 0.0015).all()                                        # in the band of the F used
        true = int((iset.landmark[v1][added[:, 0]] == iset.landmark[v2][added[:, 1]]).sum())
        print(f"pair {v1},{v2}: seeds {seeds.shape[0]} added {added.shape[0]} true {true} max candidates {gres[k]['max_candidates']}")
        added_all += added.shape[0]
        true_all += true
    assert true_all >= 0.9 * added_all
    g = info2["guided"]
    assert g["pairs"] == 3 and g["status"] == {"ok": 3, "too_few": 0, "degenerate": 0}
    assert g["added"] == added_all and g["seeds"] == info0["correspondences"]
    assert info2["correspondences"] == info0["correspondences"] + added_all
    assert tm.guided_s > 0.0
    for name, tt in (("without", tt0), ("with", tt2)):
        ln = np.diff(tt.offsets)
        print(f"tracks {name} guided: length 2: {int((ln == 2).sum())}, length 3: {int((ln == 3).sum())}")


def test_guided_needs_a_verification(runs):
    from orthosfm_amd import pipeline as P
    with pytest.raises(ValueError):
        P.match_and_build_tracks(runs[0], verify=False, guided=True)
