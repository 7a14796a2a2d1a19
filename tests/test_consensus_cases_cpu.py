"""The cases of tests/consensus_cases.py under the definition of tests/consensus_restatement.py, on the CPU: that no
decision of a case sits where rounding could take it either way (so that the kernels can be held to the restatement
exactly), that the definition returns what was planted, and that the reference's rule does not."""
import numpy as np
import pytest

import consensus_cases as cc
import consensus_restatement as cr
import tri_cases as tri

IDS = [cc.key(n, m) for n, m in cc.ALL]
PLANTED = [(n, m) for n, m in cc.ALL if n in ("planted", "lengths")]


@pytest.mark.parametrize("name,model", cc.ALL, ids=IDS)
def test_guards(name, model):
    """Every scored or refit error lies outside max_error (1 +- 1e-6); among the hypotheses with the winning count
    but another mask the sums differ by 1e-6 relative or more.  With refit_rounds == 0 the winner's own midpoint is
    returned, so there the second guard covers every other hypothesis with the winning count."""
    case, r = cc.build(name, model), cc.restated(name, model)
    print(f"{cc.key(name, model)}: guard_error {r['guard_error']:.3e} guard_gap {r['guard_gap']:.3e} "
          f"guard_gap_any {r['guard_gap_any']:.3e} stats {r['stats']}")
    assert r["guard_error"] >= 1e-6
    assert r["guard_gap"] >= 1e-6
    if case.opts.get("refit_rounds", 2) == 0:
        assert r["guard_gap_any"] >= 1e-6


@pytest.mark.parametrize("name,model", cc.ALL, ids=IDS)
def test_bookkeeping(name, model):
    """The restatement's own sums: the statuses partition the tested tracks, the counters match the flags."""
    case, r = cc.build(name, model), cc.restated(name, model)
    st, status = r["stats"], r["status"]
    ln = tri.track_lengths(case.sc)
    assert st["tracks_tested"] == int((ln >= 2).sum()) and st["obs_tested"] == int(ln[ln >= 2].sum())
    for field, code in (("tracks_clean", cr.CLEAN), ("tracks_repaired", cr.REPAIRED), ("tracks_unsupported", cr.UNSUPPORTED),
                        ("tracks_degenerate", cr.DEGENERATE)):
        assert st[field] == int((status == code).sum())
    assert int((status == cr.UNTESTED).sum()) == int((ln < 2).sum())
    assert st["obs_dropped"] == int((~r["keep"]).sum())
    assert (r["valid"] == np.isin(status, (cr.CLEAN, cr.REPAIRED))).all()
    untouched = ~r["valid"]
    assert np.array_equal(r["points"][untouched], case.sc.points[untouched])


@pytest.mark.parametrize("name,model", PLANTED, ids=[cc.key(n, m) for n, m in PLANTED])
def test_planted_mask_is_returned(name, model):
    case, r = cc.build(name, model), cc.restated(name, model)
    want = cc.expected_keep(case)
    wrong = np.nonzero(r["keep"] != want)[0]
    assert wrong.size == 0, (wrong[:10], case.sc.obs_point[wrong[:10]])
    assert r["stats"]["tracks_unsettled"] == 0


@pytest.mark.parametrize("model", (cc.Q, cc.E), ids=("quat", "euler"))
def test_every_verdict_occurs(model):
    """At least 8 tracks of each of CLEAN, REPAIRED and UNSUPPORTED over planted and lengths."""
    status = np.concatenate([cc.restated(n, model)["status"] for n in ("planted", "lengths")])
    for code in (cr.CLEAN, cr.REPAIRED, cr.UNSUPPORTED):
        assert int((status == code).sum()) >= 8, (code, np.bincount(status, minlength=5))


@pytest.mark.parametrize("model", (cc.Q, cc.E), ids=("quat", "euler"))
def test_reference_rule_keeps_no_contaminated_track_whole(model):
    """The gap this closes: the reference's rule (all rays intersected, the wrong one included; every feature judged
    against that point), run on every track of planted, returns the planted mask on not one contaminated track."""
    case = cc.build("planted", model)
    keep = cr.reference_rule(case.sc)
    start = np.concatenate([[0], np.cumsum(tri.track_lengths(case.sc))]).astype(np.int64)
    contaminated = [j for j in range(len(start) - 1) if case.planted[start[j]:start[j + 1]].any()]
    assert len(contaminated) >= 60
    whole = [j for j in contaminated
             if np.array_equal(keep[start[j]:start[j + 1]], ~case.planted[start[j]:start[j + 1]])]
    lost = int((~keep & ~case.planted).sum())
    print(f"reference rule: {len(whole)} of {len(contaminated)} contaminated tracks kept whole, {lost} good observations lost")
    assert not whole
