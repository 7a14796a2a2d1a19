"""The triangulation check of tests/tri_cases.py without a device: the golden is what the generator gives today, the
reference's rays agree with the projection model (the oracle's jets, tested on their own in test_oracle_ba.py), plain
double arithmetic -- oracle_ba_triangulate, the kernel's twin -- passes every case with tau = 4, and an implementation
with one fault of the kind a kernel could have fails on the case that was made for it."""
import numpy as np
import pytest

import oracle_lib
import tri_cases as tc
from orthosfm_amd import synth


def _twin(sc):
    """oracle_ba_triangulate on a copy: (points, valid)."""
    w = sc.copy()
    valid = oracle_lib.oracle_ba_triangulate(w)
    return w.points, valid


@pytest.mark.parametrize("name", ["single", "parallel_axis"])
def test_golden_is_current(name):
    pytest.importorskip("mpmath")
    for model in tc.CASES[name]:
        sc, g = tc.load(name, model)
        ref = tc.reference(sc)
        for f in ("points", "A", "ratios", "valid"):
            assert ref[f].tobytes() == g[f].tobytes(), (name, model, f)


def test_hashes_and_eigenvalue_bands():
    below = set()
    total = 0
    for name, model in tc.ALL:
        sc, g = tc.load(name, model)                     # asserts the hash
        ln = tc.track_lengths(sc)
        assert np.array_equal(g["valid"].astype(bool), ln >= 2)
        v = g["valid"].astype(bool)
        total += int(v.sum())
        r = g["ratios"][v]
        assert ((r >= tc.BAND_HI) | (r < tc.BAND_LO)).all(), (name, model, r[(r < tc.BAND_HI) & (r >= tc.BAND_LO)])
        assert (r[:, 0] == 1.0).all() and (r[:, 1] >= tc.BAND_HI).all()
        if (r < tc.BAND_LO).any():
            below.add(name)
            assert (r[:, 2] < tc.BAND_LO).all()          # rank 2 on every track
        assert (g["A"][v] > 0).all() and np.isfinite(g["A"]).all() and np.isfinite(g["points"]).all()
    assert below == {"parallel_axis"}
    assert total > 1000
    # what the cases promise
    sc, _ = tc.load("lengths", 0)
    ln = tc.track_lengths(sc)
    assert ln.size == 33 and sorted(ln[ln >= 2]) == sorted(tc.LENGTHS) and set(ln[ln < 2]) == {0, 1}
    assert ln[0] == 260 and ln[1] < 2 and ln[32] == 250
    sc, _ = tc.load("single", 1)
    assert sc.points.shape[0] == 1 and sc.obs_xy.shape[0] == 2
    sc, _ = tc.load("non_unit_quat", 0)
    n = np.linalg.norm(sc.cam_params[:, :4], axis=1)
    assert n.min() < 0.971 and n.max() > 1.029 and (np.abs(n - 1) <= 0.0301).all() and (np.abs(n - 1) > 1e-3).all()
    sc, _ = tc.load("intrinsics", 0)
    assert {(1920, 1080), (3, 5)} == set(zip(sc.img_w.tolist(), sc.img_h.tolist()))
    assert (sc.obs_xy == 0).any() and (sc.obs_xy < 0).any() and (sc.obs_xy[:, 0] > 1920).any()
    assert (sc.obs_xy.astype(np.float32).astype(np.float64) == sc.obs_xy).all()
    sc, _ = tc.load("angles", 1)
    assert np.abs(sc.cam_params[:, [0, 2]]).max() == 100.0


def test_reference_rays_agree_with_the_projection_model():
    """Every point o + t d of a reference ray projects onto its observation: the oracle's residual (its jets) is
    within the project's residual tolerance, 1e-9 px.  non_unit_quat is left out: for a non-unit q Eigen's q * v and
    the functor's q.inverse() are different maps."""
    pytest.importorskip("mpmath")
    seen = 0
    for name, model in tc.ALL:
        if name == "non_unit_quat":
            continue
        sc, _ = tc.load(name, model)
        O = sc.obs_xy.shape[0]
        # the first 40 observations (intrinsics: the out-of-frame positions are among them) and 40 drawn ones
        ks = np.unique(np.concatenate([np.arange(min(O, 40)),
                                       np.floor(synth.uniform(tc.SEED, tc._ST | 0x90, 40) * O).astype(np.int64)]))
        o, d = tc.rays(sc, ks)
        for t in (0.0, 5.0, 10.0, 20.0):
            P = np.ones((ks.size, 4))
            P[:, :3] = o + t * d
            probe = synth.BaScene(sc.model, sc.cam_params, sc.cam_const, sc.img_w, sc.img_h, P, sc.obs_xy[ks].copy(),
                                  sc.obs_camera[ks].copy(), np.arange(ks.size, dtype=np.int32), sc.gt_cams, sc.gt_points)
            _, err = oracle_lib.oracle_ba_residuals(probe)
            assert (err <= 1e-9).all(), (name, model, t, err.max())
        seen += ks.size
    assert seen >= 500
    # parallel_axis: the one look direction is the z axis (Euler: up to cos(fl(pi/2)) = 6e-17, which 1 - d d^T loses)
    for model in (0, 1):
        sc, _ = tc.load("parallel_axis", model)
        _, d = tc.rays(sc, np.arange(sc.obs_xy.shape[0]))
        assert (d[:, 0] == 0).all() and (d[:, 2] == 1).all() and (np.abs(d[:, 1]) < 1e-16).all()


@pytest.mark.parametrize("name,model", tc.ALL)
def test_double_twin_passes(name, model):
    sc, g = tc.load(name, model)
    pts, valid = _twin(sc)
    assert np.array_equal(valid, g["valid"])
    r, j = tc.worst(pts, g)
    print(f"\n[tri twin] {tc.key(name, model):28s} worst {r:.2f} at track {j} (A {g['A'][j]:.2e})")
    assert r <= tc.TAU_TWIN
    assert tc.check(pts, g, tc.TAU_TWIN)
    inv = ~g["valid"].astype(bool)
    assert np.array_equal(pts[inv], sc.points[inv])
    assert (pts[~inv, 3] == 1.0).all()


def _must_fail(pts, g):
    r, _ = tc.worst(pts, g)
    assert r > max(tc.TAU, tc.TAU_TWIN) and not tc.check(pts, g) and not tc.check(pts, g, tc.TAU_TWIN)
    return r


@pytest.mark.parametrize("model", [0, 1])
def test_planted_observation_dropped(model):
    """The last observation of every track longer than 8 is not summed (a lane's last trip lost)."""
    sc, g = tc.load("lengths", model)
    ln = tc.track_lengths(sc)
    last = np.cumsum(ln) - 1
    drop = last[ln > 8]
    keep = np.ones(sc.obs_xy.shape[0], dtype=bool)
    keep[drop] = False
    w = sc.copy()
    w.obs_xy, w.obs_camera, w.obs_point = sc.obs_xy[keep].copy(), sc.obs_camera[keep].copy(), sc.obs_point[keep].copy()
    pts, _ = _twin(w)
    _must_fail(pts, g)
    # ... and each of those tracks fails, none of the others
    r = tc.ratios(pts, g)
    assert (r[ln > 8] > max(tc.TAU, tc.TAU_TWIN)).all() and (r[ln <= 8] <= tc.TAU_TWIN).all()


def test_planted_quaternion_normalised():
    sc, g = tc.load("non_unit_quat", 0)
    w = sc.copy()
    w.cam_params[:, :4] /= np.linalg.norm(w.cam_params[:, :4], axis=1, keepdims=True)
    pts, _ = _twin(w)
    _must_fail(pts, g)


def test_planted_direction_not_normalised():
    """d d^T without the normalisation of d: exact for unit quaternions, wrong for the scaled ones."""
    pytest.importorskip("mpmath")
    sc, g = tc.load("non_unit_quat", 0)
    o, d = tc.rays(sc, np.arange(sc.obs_xy.shape[0]))
    pts = sc.points.copy()
    start = np.concatenate([[0], np.cumsum(tc.track_lengths(sc))])
    for j in range(pts.shape[0]):
        k = slice(start[j], start[j + 1])
        Pm = np.eye(3)[None] - d[k, :, None] * d[k, None, :]
        pts[j, :3] = np.linalg.solve(Pm.sum(0), np.einsum("kab,kb->a", Pm, o[k]))
    _must_fail(pts, g)


@pytest.mark.parametrize("model", [0, 1])
def test_planted_component_along_the_null_direction(model):
    """Rank 2: the answer is the minimum-norm point, so 1e-6 d added to it is an error."""
    sc, g = tc.load("parallel_axis", model)
    pts, _ = _twin(sc)
    assert tc.check(pts, g, tc.TAU_TWIN)
    pts[:, :3] += 1e-6 * np.array([0.0, 0.0, 1.0])
    _must_fail(pts, g)


@pytest.mark.parametrize("model", [0, 1])
def test_planted_width_and_height_swapped(model):
    sc, g = tc.load("intrinsics", model)
    w = sc.copy()
    w.img_w, w.img_h = sc.img_h.copy(), sc.img_w.copy()
    pts, _ = _twin(w)
    _must_fail(pts, g)


@pytest.mark.parametrize("model", [0, 1])
def test_planted_1e11_on_one_point(model):
    """An error that the absolute 1e-9 of test_ba_gpu.py::test_triangulation lets pass."""
    sc, g = tc.load("benign", model)
    pts, _ = _twin(sc)
    assert tc.check(pts, g, tc.TAU_TWIN)
    j = int(np.argsort(g["A"])[g["A"].size // 2])        # a track of median conditioning
    pts[j, 1] += 1e-11
    assert np.abs(pts[:, :3] - g["points"]).max() <= 1e-9
    _must_fail(pts, g)
    assert int(np.argmax(tc.ratios(pts, g))) == j
