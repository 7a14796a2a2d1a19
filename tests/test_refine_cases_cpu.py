"""The cases of tests/refine_cases.py under the restatement alone (no device): every case reaches the statuses and
paths it is there for, the restatement does what the refinement is for (on `base`: errors a tenth of what they were,
19 of 20 observations refined), few observations are ambiguous, and the bounds see three planted errors."""
import numpy as np
import pytest

import refine_cases as rc
import refine_restatement as rr


def _reference_of(c):
    """Per observation, the reference observation of its track (itself where the track has no alive observation)."""
    alive = np.ones(c.num_obs, bool) if c.alive is None else c.alive.astype(bool)
    ref = np.arange(c.num_obs)
    for t in range(c.offsets.shape[0] - 1):
        obs = np.arange(c.offsets[t], c.offsets[t + 1])
        live = obs[alive[obs]]
        if live.size:
            ref[obs] = live[0]
    return ref


def _errors(c, out):
    """(before, after) distances of the REFINED observations to the exact correspondence of their reference."""
    ref = _reference_of(c)
    sel = np.flatnonzero(out["status"] == rr.REFINED)
    truth = np.array([c.exact(ref[f], f) for f in sel]).reshape(-1, 2)
    return np.linalg.norm(c.xy[sel] - truth, axis=1), np.linalg.norm(out["xy"][sel] - truth, axis=1)


def _base_figures(out):
    c = rc.case("base")
    before, after = _errors(c, out)
    nonref = out["status"] != rr.REFERENCE
    ratio = np.median(after) / np.median(before) if after.size else np.inf
    return ratio, float((out["status"] == rr.REFINED).sum()) / float(nonref.sum())


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_reaches_its_paths(name):
    c, out = rc.case(name), rc.restated(name)
    st = out["status"]
    for s in c.expect:
        assert (st == s).any(), (name, rr.STATUS_NAMES[s])
    # what no status moves
    unmoved = st != rr.REFINED
    assert np.array_equal(out["xy"][unmoved], c.xy[unmoved])
    if name == "border":
        assert c.images[0].shape == (81, 97)
        for k in ("ref_outside", "target_outside_first"):
            assert st[c.paths[k]] == rr.OUTSIDE and out["iterations"][c.paths[k]] == 0, k
        for k in ("target_outside_later", "target_outside_later_y"):
            assert st[c.paths[k]] == rr.OUTSIDE and out["iterations"][c.paths[k]] >= 1, k
        for k in ("touch", "touch_origin"):
            f = c.paths[k]
            assert st[f] == rr.REFINED and np.array_equal(out["xy"][f], c.xy[f]), k
        f = c.paths["touch"]
        assert tuple(c.xy[f] + 7) == (96.0, 80.0)       # the window ends on the last column and row
    if name == "flat_and_edge":
        assert (st[c.paths["flat"]] == rr.FLAT).all()
        assert (st[c.paths["edge"]] == rr.ILL_CONDITIONED).all()
        assert (st[c.paths["textured"]] == rr.REFINED).all()
    if name == "lengths":
        assert set(np.diff(c.offsets)) == {2, 3, 33}
        assert st[c.paths["moved_reference"]] == rr.REFERENCE and st[c.paths["moved_reference"] - 1] == rr.UNTESTED
        assert st[c.paths["moved_reference_long"]] == rr.REFERENCE
        assert (st[c.paths["single"]] == rr.UNTESTED).all()
        assert c.num_obs % 4 != 0
    if name == "rgb_sizes":
        assert {im.shape for im in c.images} == {(128, 160), (101, 131, 3), (120, 97, 3)}
    if name == "empty":
        assert c.num_obs == 0 and st.shape == (0,)
    if name.startswith("radius") or name == "step2":
        side = 2 * c.options["radius"] + 1
        assert (side * side) % 64 != 0                    # a masked tail in the last stride of 64 lanes


def test_radii_cover_every_stride_count():
    sides = [2 * rc.case(n).options["radius"] + 1 for n in ("radius2", "radius3", "radius7", "radius15")]
    assert [s * s for s in sides] == [25, 49, 225, 961]
    assert rc.case("step2").options["step"] == 2.0


def test_strong_runs_differ():
    a, b = rc.restated("strong_init")["status"], rc.restated("strong_noinit")["status"]
    assert rc.case("strong_init").xy.tobytes() == rc.case("strong_noinit").xy.tobytes()
    assert not np.array_equal(a, b)
    assert (a == rr.REFINED).sum() > (b == rr.REFINED).sum()


def test_base_bounds():
    ratio, share = _base_figures(rc.restated("base"))
    print(f"base: median error ratio {ratio:.4f}, refined {share:.3f}")
    assert ratio <= 0.1
    assert share >= 0.95


@pytest.mark.parametrize("name", rc.NAMES)
def test_few_ambiguous(name):
    out = rc.restated(name)
    n = int(rc.tested(out).sum())
    assert int(rc.ambiguous(out).sum()) <= 0.02 * n


@pytest.mark.parametrize("plant", [p for p in rr.PLANTS if p])
def test_bounds_see_planted_error(plant):
    ratio, share = _base_figures(rr.refine_tracks(plant=plant, **rc.case("base").call()))
    print(f"{plant}: median error ratio {ratio:.4f}, refined {share:.3f}")
    assert ratio > 0.1 or share < 0.95


def test_pivot_threshold():
    """PIVOT's two measured values, and the threshold as their geometric mean."""
    def smallest(name, which=None):
        c = rc.case(name)
        out = rr.refine_tracks(**{**c.call(), "min_pivot": 1e-12})
        p = out["pivot_min"][c.paths[which]] if which else out["pivot_min"][rc.tested(out) & np.isfinite(out["pivot_min"])]
        return p
    edge_max = smallest("flat_and_edge", "edge").max()
    textured_min = min(smallest("base").min(), smallest("strong_init").min())
    print(f"edge_max {edge_max:.6g} textured_min {textured_min:.6g} geometric mean {np.sqrt(edge_max * textured_min):.6g}")
    assert edge_max < textured_min
    assert abs(edge_max - rc.PIVOT["edge_max"]) <= 1e-5 * edge_max
    assert abs(textured_min - rc.PIVOT["textured_min"]) <= 1e-5 * textured_min
    assert rc.PIVOT["threshold"] == round(float(np.sqrt(edge_max * textured_min)), 3) == rr.DEFAULTS["min_pivot"]
