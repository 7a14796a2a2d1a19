"""ba_triangulate_kernel against the independent 200-bit reference of tests/tri_cases.py (recorded in
tests/golden/tri_reference.npz; the power of the check is shown without a device in tests/test_tri_cases_cpu.py),
through every entry that launches it: osfm_ba_triangulate, osfm_filter_reprojection and the device-resident scene's
full and incremental passes.  Every valid track is held to |x - x_ref|_inf <= TAU 2^-53 A_j, A_j = n_j (max |o_k| +
|x_ref|) / lambda+min: the bound follows the conditioning of the track.  test_ba_gpu.py::test_triangulation and
test_filters_gpu.py compare the kernel with oracle_ba_triangulate, its line-for-line twin, at an absolute 1e-9.

TAU = 8: the smallest power of two that is at least four times the largest ratio observed, 1.62 (the factor allows
for another compiler's FMA contraction and fold order).  The double twin on the CPU needs 1.71.

Observed on MI355X, largest |x - x_ref|_inf / (2^-53 A_j) over the valid tracks of each case (per-call entry; the
filter on benign and lengths and the scene's full and incremental passes gave the same bytes, so the same ratios):
  case                      quaternion   Euler
  benign                    1.619        0.725
  lengths                   0.882        0.948
  single                    0.357        0.558
  near_parallel_1e-2        0.830        0.963
  near_parallel_1e-4        0.743        0.951
  parallel_axis             0.095        0.096
  non_unit_quat             1.103        -
  intrinsics                1.295        1.587
  angles                    -            0.738
"""
import ctypes as C

import numpy as np
import pytest

import tri_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    from orthosfm_amd import ba as m
    from orthosfm_amd import capi
    assert capi.device_count() >= 1
    return m


_per_call = {}


def _triangulate(ba, name, model):
    """(scene, golden, points, valid) of the per-call entry, computed once per case."""
    k = (name, model)
    if k not in _per_call:
        sc, g = tc.load(name, model)
        fp = ba.FlatProblem.from_scene(sc)
        valid = ba.triangulate(fp)
        fp.points.setflags(write=False)
        _per_call[k] = (sc, g, fp.points, valid)
    return _per_call[k]


def _hold(points, g, what):
    r, j = tc.worst(points, g)
    print(f"\n[tri] {what:44s} worst {r:.3f} at track {j} (A {g['A'][j]:.2e})")
    assert r <= tc.TAU, (what, r, j)
    return r


@pytest.mark.parametrize("name,model", tc.ALL)
def test_per_call(ba, name, model):
    sc, g, pts, valid = _triangulate(ba, name, model)
    assert np.array_equal(valid, g["valid"])
    v = g["valid"].astype(bool)
    assert pts[~v].tobytes() == sc.points[~v].tobytes()            # fewer than two rays: the point keeps its bytes
    assert (pts[v, 3] == 1.0).all()
    _hold(pts, g, tc.key(name, model))
    # a second call gives the same bytes
    fp = ba.FlatProblem.from_scene(sc)
    valid2 = ba.triangulate(fp)
    assert np.array_equal(valid2, valid) and fp.points.tobytes() == pts.tobytes()


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("name", ["benign", "lengths"])
def test_reprojection_filter(ba, name, model):
    from orthosfm_amd import capi
    sc, g, pts, _ = _triangulate(ba, name, model)
    fp = ba.FlatProblem.from_scene(sc)
    st = fp.struct()
    O, M = fp.obs_camera.shape[0], fp.points.shape[0]
    keep, valid, err = np.zeros(O, dtype=np.uint8), np.zeros(M, dtype=np.uint8), np.zeros(O)
    capi.check(capi.lib.osfm_filter_reprojection(C.byref(st), 0, C.c_double(1.5), capi._ptr(keep, C.c_uint8),
                                                 capi._ptr(valid, C.c_uint8), capi._ptr(err, C.c_double)))
    assert np.array_equal(valid, g["valid"])
    _hold(fp.points, g, tc.key(name, model) + " filter")
    v = g["valid"].astype(bool)
    assert (fp.points[v, 3] == 1.0).all() and fp.points[~v].tobytes() == sc.points[~v].tobytes()
    assert fp.points.tobytes() == pts.tobytes()
    # point_valid and err are optional: without them the points are the same
    fp2 = ba.FlatProblem.from_scene(sc)
    st2 = fp2.struct()
    capi.check(capi.lib.osfm_filter_reprojection(C.byref(st2), 0, C.c_double(1.5), capi._ptr(keep, C.c_uint8), None, None))
    assert fp2.points.tobytes() == pts.tobytes()


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("name", ["benign", "lengths"])
def test_scene(ba, name, model):
    sc, g, pts, _ = _triangulate(ba, name, model)
    V = sc.cam_params.shape[0]
    views = np.arange(V, dtype=np.int32)
    v = g["valid"].astype(bool)
    # all views aligned in order, one full pass
    a = tc.scene_from_ba_scene(sc)
    a.align_views(views, sc.cam_params, sc.cam_const)
    assert a.triangulate() == 0
    _, _, hp, pt = a.download()
    a.close()
    assert np.array_equal(hp, v)
    _hold(pt, g, tc.key(name, model) + " scene")
    assert pt[v].tobytes() == pts[v].tobytes()
    # all but the last three views, then those three and an incremental pass checked against a full one
    b = tc.scene_from_ba_scene(sc)
    b.align_views(views[:-3], sc.cam_params[:-3], sc.cam_const[:-3])
    assert b.triangulate() == 0
    hp0 = b.download()[2]
    seen = np.bincount(sc.obs_point[sc.obs_camera < V - 3], minlength=v.size)
    touched = np.unique(sc.obs_point[sc.obs_camera >= V - 3])
    assert np.array_equal(hp0, seen >= 2) and 0 < touched.size < v.size       # the second pass is a partial one
    b.align_views(views[-3:], sc.cam_params[-3:], sc.cam_const[-3:])
    assert b.triangulate(views[-3:], check_full=True) == 0
    _, _, hp, pt = b.download()
    b.close()
    assert np.array_equal(hp, v)
    _hold(pt, g, tc.key(name, model) + " scene, incremental")
    assert pt[v].tobytes() == pts[v].tobytes()
