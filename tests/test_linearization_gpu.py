"""The kernels on either side of the bundle adjustment's Cholesky -- the point pass (ba_point_win / _over kernels),
the pair pass with its chunked lists and fused tail, the dense Schur product, the camera update, the back pass and
the cost pass -- against a reference of the same operations in extended precision (tests/lin_cases.py; its power
is shown without a device in tests/test_lin_cases_cpu.py).  ba.debug_linearization runs osfm_ba_solve and copies out
its first iteration: the Jacobi scales, the LM diagonals, V_j^-1 and g_j of the points, the reduced camera system and
its rhs, then the camera step, the candidate cameras and points, the model cost change, the candidate cost, the
relative decrease and the decision.  Every case asserts the regime it took from the capture, then checks each
quantity componentwise (|gpu - ref| <= tau u A, the taus of lin_cases.TAU) and what the padding rows hold.

Observed on MI355X (largest |gpu - ref| / (tau u A) over the quantities of each case, and the quantity; <= 1 is
asserted; S alone in the last column):
  3 cameras x 2500, quaternion: small lists, N = 32 solve, 3 pairs of 10 chunks   7.9e-01 (vinv)   S 2.2e-05
  the same, general list build (S, rhs, step, candidates bit-identical)           7.9e-01 (vinv)   S 2.2e-05
  3 cameras x 2500, Euler (and its general build)                                 3.7e-01 (vinv)   S 5.6e-06
  8 cameras, tracks of 1-2 views                                                  4.0e-01 (scale_p) S 2.1e-06
  tracks of 33-60 views (window and over-window kernels), empty tracks, quat.     3.3e-01 (vinv)   S 2.2e-03
  the same, Euler                                                                 1.9e-01 (vinv)   S 8.9e-04
  Huber: outliers, squared norms within 8 ulps of huber^2 either side and on it   1.3e-02 (vinv)   S 2.2e-05
  constant points (pdim 0), euler_free 3                                          7.1e-03 (S)      S 7.1e-03
  euler_free 4, a constant camera, mixed cam_ldim                                 1.7e-01 (vinv)   S 2.3e-05
  dense Schur product split 16 ways over K, 40 cameras / 30 cameras              5.0e-01 / 5.2e-01 (vinv)
  dense Schur product unsplit (written into S in place), 30 cameras x 60 tracks   3.0e-02 (vinv)   S 1.1e-04
  ring of 200 cameras, elimination order chosen / OSFM_BA_ORDER=0                 5.4e-01 (vinv)   S 4.5e-05
  Jacobi scaling off                                                              8.2e-01 (vinv)   S 2.6e-05
  radius 1e-3 / 1e4 / 1e16                                                        2.3e-01 / 1.7e-01 / 1.7e-01 (vinv)
  OSFM_BA_SEPARATE_BACK / OSFM_BA_SEPARATE_POST                                   5.6e-01 (vinv)   S 1.2e-04
  two-view tracks, nearly parallel rays, radius 1e12 (kappa(V) > 1e6)            6.93e-02 (scale_p) S 2.4e-15
  config 4 at its stated size (200 cameras, 100k tracks)                          8.2e-01 (vinv)   S 2.3e-05
Every capture's padding rows were identity rows.  The file runs in about 25 s, most of it the config-4 reference.
"""
import os

import numpy as np
import pytest

import lin_cases as lc
from orthosfm_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    from orthosfm_amd import ba as m
    from orthosfm_amd import capi
    assert capi.device_count() >= 1
    return m


def _capture(ba, sc, opt=None, env=None):
    fp = ba.FlatProblem.from_scene(sc)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        cap = ba.debug_linearization(fp, **(opt or {}))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return cap


def _check(ba, sc, opt=None, env=None, name=""):
    """Capture, check every quantity against the reference, check the padding rows; returns the capture."""
    cap = _capture(ba, sc, opt, env)
    assert not cap["stopped"] and not cap["flow_aborted"]
    R = lc.reference(sc, opt or {})
    ratios = lc.check(sc, R, cap)
    worst = max(ratios, key=ratios.get)
    print(f"\n[lin] {name:28s} worst {ratios[worst]:.2e} ({worst})  " +
          " ".join(f"{k}={v:.1e}" for k, v in sorted(ratios.items())))
    assert ratios[worst] <= 1.0, ratios
    assert cap["num_pad"] == cap["N"] - R["L"].nc
    if cap["num_pad"]:
        assert cap["pad_diag_min"] == 1.0 and cap["pad_diag_max"] == 1.0 and cap["pad_off_max"] == 0.0
    return cap


def _drop_tracks(sc, tracks):
    """The scene without the observations of the given tracks (their points stay: tracks without observations)."""
    keep = ~np.isin(sc.obs_point, tracks)
    out = sc.copy()
    out.obs_xy = np.ascontiguousarray(sc.obs_xy[keep])
    out.obs_camera = np.ascontiguousarray(sc.obs_camera[keep])
    out.obs_point = np.ascontiguousarray(sc.obs_point[keep])
    return out


@pytest.mark.parametrize("model", [0, 1])
def test_three_camera_local_problems(ba, model):
    """Every track in every camera, 2500 tracks: each pair list holds ten 256-entry chunks; the small list build,
    the one-block solve; the general build of the same lists gives the same system to the bit."""
    sc = synth.make_ba_scene(model, 3, 2500, config_id=81, min_len=3, max_len=3)
    cap = _check(ba, sc, name=f"3 cameras, model {model}")
    assert cap["small_lists"] and cap["small_solve"] and not cap["dense"] and cap["dense_splits"] == 0 and cap["N"] == 32
    assert cap["pair_chunk"] == 256 and cap["multi_chunk_pairs"] == cap["num_pairs"] > 0
    assert cap["post_fused"] and cap["back_fused"] and cap["win_over"] == 0
    gen = _check(ba, sc, env={"OSFM_BA_PAIR_LISTS_GENERAL": "1"}, name=f"3 cameras, model {model}, general")
    assert not gen["small_lists"] and gen["multi_chunk_pairs"] == cap["multi_chunk_pairs"]
    for k in ("S", "rhs", "diag_c", "vinv", "ge", "y_c", "cand_cams", "cand_points"):
        assert np.array_equal(gen[k], cap[k]), k
    if model == 0:
        # repeatability: the same capture to the bit
        again = _capture(ba, sc)
        for k in ("S", "rhs", "y_c", "cand_cams", "cand_points"):
            assert np.array_equal(again[k], cap[k]), k
        assert again["model_cost_change"] == cap["model_cost_change"] and again["cand_cost"] == cap["cand_cost"]


def test_eight_cameras_with_tracks_of_one_or_two_views(ba):
    sc = synth.make_ba_scene(0, 8, 3000, config_id=81, min_len=1, max_len=2)
    cap = _check(ba, sc, name="8 cameras, tracks of 1-2")
    assert cap["small_lists"] and not cap["small_solve"] and cap["N"] == 64


@pytest.mark.parametrize("model", [0, 1])
def test_long_tracks_take_the_over_window_kernels(ba, model):
    """Tracks of 33..60 views (a window with more than 256 observations: the wave-per-track kernels beside the
    window kernels), tracks without observations, an observation count that is not a multiple of 64."""
    sc = synth.make_ba_scene(model, 64, 400, config_id=83, min_len=33, max_len=60)
    sc = _drop_tracks(sc, [0, 5, 77, 399])
    assert sc.obs_camera.size % 64 != 0
    cap = _check(ba, sc, name=f"long tracks, model {model}")
    assert 0 < cap["win_over"] < cap["win_num"]


def test_huber_outliers_and_the_threshold(ba):
    """Outliers far out on the linear branch, and squared residual norms within a few ulps of huber^2 on either side
    and on it.  The images are 8 pixels wide, so that a pixel position has ulps of 1e-15: the observation is put at
    the projection in x and at (projection - t) in y, t = 1 + i 2^-52, i in -3..3; the subtraction the residual makes
    is exact (Sterbenz), and the oracle's squared norms land within 8 ulps of 1."""
    from oracle_lib import oracle_ba_residuals
    sc = synth.make_ba_scene(0, 12, 800, config_id=35, width=8, height=8, noise_px=0.02)
    sc.obs_xy[::41] += 3.0
    raw, _ = oracle_ba_residuals(sc)
    proj = raw + sc.obs_xy
    near = [k for k in range(3, sc.obs_xy.shape[0], 53) if k % 41]
    for i, k in enumerate(near):
        sc.obs_xy[k] = (proj[k, 0], proj[k, 1] - (1.0 + ((i % 7) - 3) * 2.0 ** -52))
    raw2, _ = oracle_ba_residuals(sc)
    ulps = ((raw2[near] ** 2).sum(1) - 1.0) / 2.0 ** -52
    assert np.abs(ulps).max() <= 8 and (ulps > 0).sum() >= 20 and (ulps < 0).sum() >= 20 and (ulps == 0).sum() >= 10
    assert ((raw2 ** 2).sum(1) > 4.0).sum() >= 100         # the outliers
    _check(ba, sc, name="huber")


@pytest.mark.parametrize("variant", ["constant points", "euler dof, constant cameras"])
def test_constant_points_constant_cameras_and_degrees_of_freedom(ba, variant):
    if variant == "constant points":
        sc = synth.make_ba_scene(1, 10, 600, config_id=84, euler_free=3)
        cap = _check(ba, sc, {"optimize_points": 0}, name="pdim 0, euler_free 3")
    else:
        sc = synth.make_ba_scene(1, 10, 600, config_id=84, euler_free=4)
        sc.cam_const[3, :] = 1                       # a constant camera
        sc.cam_const[6, [1, 4]] = 1                  # another with two more columns held
        cap = _check(ba, sc, name="euler_free 4, mixed ldim")
    assert cap["small_lists"] == 0


@pytest.mark.parametrize("model,cams,pts,lo,hi,splits", [(0, 40, 900, 12, 24, 16), (1, 30, 5000, 3, 8, 16),
                                                         (1, 30, 60, 20, 30, 1)])
def test_dense_schur_product(ba, model, cams, pts, lo, hi, splits):
    """The product split over K (partials, then ba_dense_reduce_kernel) and unsplit (fewer than 16 K steps: the
    product written into S in place)."""
    sc = synth.make_ba_scene(model, cams, pts, config_id=71, min_len=lo, max_len=hi)
    cap = _check(ba, sc, env={"OSFM_BA_DENSE_SCHUR": "1"}, name=f"dense, {cams} cameras x {pts}")
    assert cap["dense"] and not cap["small_lists"] and cap["dense_splits"] == splits


@pytest.mark.parametrize("order", ["1", "0"])
def test_ordered_layout_of_a_ring(ba, order):
    sc = synth.make_ba_scene(0, 200, 20000, config_id=81, max_len=12)
    cap = _check(ba, sc, env={"OSFM_BA_ORDER": order}, name=f"ring of 200, order {order}")
    assert (cap["order_arcs"] > 0) == (order == "1")
    if order == "1":
        assert cap["span"] >= cap["S"].shape[0] and cap["num_pad"] == cap["N"] - cap["S"].shape[0]
    assert cap["one_launch"]


@pytest.mark.parametrize("opt", [{"jacobi_scaling": 0}, {"initial_trust_region_radius": 1e-3},
                                 {"initial_trust_region_radius": 1e4}, {"initial_trust_region_radius": 1e16}])
def test_option_variants(ba, opt):
    sc = synth.make_ba_scene(1, 12, 700, config_id=85)
    _check(ba, sc, opt, name=str(opt))


@pytest.mark.parametrize("env", [{"OSFM_BA_SEPARATE_BACK": "1"}, {"OSFM_BA_SEPARATE_POST": "1"}])
def test_separate_post_and_back_launches(ba, env):
    sc = synth.make_ba_scene(0, 20, 1500, config_id=86)
    cap = _check(ba, sc, env=env, name=str(env))
    assert cap["back_fused"] == ("OSFM_BA_SEPARATE_BACK" not in env)
    assert cap["post_fused"] == ("OSFM_BA_SEPARATE_POST" not in env)


def test_ill_conditioned_points(ba):
    """Two-view tracks between cameras whose viewing directions differ by 1e-4 rad: nearly parallel rays.  With the
    default radius the LM diagonal keeps kappa(V_j) near 2e4; at a radius of 1e12 it is above 1e6."""
    sc = synth.make_ba_scene(1, 3, 400, config_id=87, min_len=2, max_len=2)
    sc.cam_params[1, :3] = sc.cam_params[0, :3] + np.array([1e-4, 0.0, 0.0])
    sc.cam_params[2, :3] = sc.cam_params[0, :3] + np.array([0.0, 1e-4, 0.0])
    cap = _check(ba, sc, {"initial_trust_region_radius": 1e12}, name="nearly parallel rays")
    V = np.linalg.inv(cap["vinv"])
    assert np.linalg.cond(V).max() > 1e6


def test_config4_at_its_stated_size(ba):
    """BASELINE config 4: 200 cameras, 100k tracks."""
    sc = synth.make_ba_scene(0, 200, 100000, config_id=4)
    cap = _check(ba, sc, name="config 4")
    assert not cap["small_lists"] and cap["one_launch"]
