"""The covariance checker (cov_cases.py) on the CPU: it accepts an independent float64 build -- the full J^T J
inverted densely, no Schur route --, rejects that build with each of eight planted faults, and the cases keep it
from being blind (condition, pivot gap).  No device."""
import numpy as np
import pytest

import cov_cases as cc

_REF = {}


def _case(name):
    """(scene, reference), built once per session."""
    if name not in _REF:
        if name == "degenerate":
            sc, _ = cc.degenerate()
        else:
            sc = cc.CASES[name]()
        _REF[name] = (sc, cc.reference(sc))
    return _REF[name]


def _ratios(name, fault=None, scene=None, ref=None):
    sc, r = (scene, ref) if scene is not None else _case(name)
    b = cc.dense_build(sc, fault=fault)
    return cc.check(r, b["cam_cov_full"], b["cam_cov"], b["point_cov"], b["point_valid"], b["cam_ldim"])


@pytest.mark.parametrize("name", ["one_tile", "two_tiles", "mixed", "after_solve", "degenerate"])
def test_checker_accepts_float64_build(name):
    q = _ratios(name)
    print(name, {k: f"{v:.3g}" for k, v in q.items()}, f"kappa {_case(name)[1]['kappa']:.3g}")
    assert max(q.values()) <= 1.0, q


def test_degenerate_points_are_invalid():
    sc, bad = cc.degenerate()
    r = _case("degenerate")[1]
    assert not r["valid"][bad].any()
    assert r["valid"].sum() >= sc.points.shape[0] - 12
    assert np.all(r["point_cov"][~r["valid"]] == 0)


@pytest.mark.parametrize("name,fault", [
    ("two_tiles", "lm_diagonal"), ("two_tiles", "one_sided_scale"), ("two_tiles", "dropped_term"),
    ("two_tiles", "transposed_pair"), ("two_tiles", "no_vinv"), ("after_solve", "identity_G"),
    ("degenerate", "invalid_kept")])
def test_checker_rejects_planted_fault(name, fault):
    q = _ratios(name, fault)
    print(name, fault, {k: f"{v:.3g}" for k, v in q.items()})
    assert max(q.values()) > 1.0, q


def test_checker_rejects_tangent_matrix_for_w2():
    sc = cc.two_tiles()
    sc.points[7] *= 2.0                  # the same Euclidean point, w = 2
    r = cc.reference(sc)
    assert max(_ratios(None, None, sc, r).values()) <= 1.0
    q = _ratios(None, "tangent", sc, r)
    assert q["point_cov"] > 1.0, q


@pytest.mark.parametrize("name", ["one_tile", "two_tiles", "mixed", "ring40", "after_solve", "degenerate"])
def test_condition_keeps_the_check_sharp(name):
    r = _case(name)[1]
    print(name, f"nc {r['nc']} kappa {r['kappa']:.4g} tol*kappa {cc.tolerance(r) * r['kappa']:.3g} newton residual {r['resid']:.2g}")
    assert r["resid"] < 1e-16
    assert cc.tolerance(r) * r["kappa"] <= 1e-7


def test_case_shapes():
    assert _case("one_tile")[1]["nc"] == 9
    assert _case("two_tiles")[1]["nc"] == 34
    m = _case("mixed")[1]
    assert 65 <= m["nc"] <= 96
    assert {0, 1, 2, 4, 5, 6} <= set(m["cam_ldim"].tolist()) and (m["cam_ldim"] == 0).sum() == 2
    assert _case("ring40")[1]["nc"] == 194
    assert not np.allclose(_case("after_solve")[0].points[:, 3], 1.0)


@pytest.mark.parametrize("name", ["one_tile", "two_tiles", "mixed", "ring40", "after_solve", "degenerate"])
def test_pivot_gap_gauge_held(name):
    """With the gauge held every relative pivot of S is at least 1e-4: four orders above the default threshold."""
    p = _case(name)[1]["pivots"]
    print(name, f"smallest relative pivot {p.min():.3g}")
    assert p.min() >= 1e-4


@pytest.mark.parametrize("name,no_const", [("one_tile", False), ("ring40", False), ("one_tile", True), ("ring40", True)])
def test_pivot_gap_gauge_open(name, no_const):
    """With the gauge open (depth_gauge = 0, or no constant camera for the rule to start from) one relative pivot is
    at most 1e-10: two orders below the default threshold."""
    sc = cc.CASES[name]()
    if no_const:
        sc = cc.without_constant_camera(sc)
        assert cc.gauge_choice(sc) == (-1, -1)
    p = cc.system_pivots(sc, depth_gauge=no_const)         # (without a constant camera the rule holds nothing anyway)
    print(name, no_const, f"smallest relative pivot {p.min():.3g}")
    assert p.min() <= 1e-10
