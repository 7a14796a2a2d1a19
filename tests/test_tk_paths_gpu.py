"""osfm_tk_align / osfm_scene_tk_align where the kernels of tk_kernels.hip change path, against the numpy restatement
(tests/tk_restatement.py) on tk_cases.PATH_CASES: every instance C = 3..8 of the scoring and mask kernels, the edges
of the 256-track tile and of the 16-hypothesis chunk, sample sizes 4..32, the all-track fallback over several tiles and
at C = 8, the consensus boundary, groups in which no hypothesis is usable, inputs without a rank-3 factorisation, the
options away from their defaults, and the scene's gather for a 5-view group.

tests/test_tk_cases_cpu.py shows on the restatement alone that every case keeps each decision of each hypothesis
-- and of the all-track factorisation where the fallback runs -- off its threshold, and that the degenerate inputs are
a factor 100 clear of the rank test.  So, as in tests/test_tk_gpu.py, the integer results are compared for equality
and the real ones to 1e-8.  Every case also asserts, from the result alone, the path it was chosen for (PATH below).

Which cases of test_path_case_against_restatement fail under a mistake of the kind they are for (each mistake was
built into a copy of the library once and the two Tomasi-Kanade files run against it on an MI355X):
  `cons < min_consensus` as `<=` in tk_select_kernel     [mc30] ends FALLBACK with 0 supported models instead of 241,
                                                         [s32n32] (consensus 0 = min_consensus 0) likewise
  tk_fallback_gram_kernel leaves its last tile out       [fb600] loses 88 of 600 tracks, [fb8] 44 of 300, [fb5] all 256;
                                                         [mc31], [twin3], [twin4] fail as well
  `case 6:` of the scoring dispatch launches <5>         [c6], and no test of tests/test_tk_gpu.py
  fix_err summed over S - 1 tracks                       [last1]: the winner's last-drawn sample track misses the bound
                                                         and the mean error comes out low; no test of tests/test_tk_gpu.py

Observed on MI355X, largest |gpu - restatement| per case (1e-8 is asserted):
  case      basis     offsets   mean error
  c4        1.4e-15   0.0e+00   1.7e-14
  c6        1.2e-15   0.0e+00   3.8e-14
  c7        1.4e-15   0.0e+00   4.9e-15
  c8w       1.1e-15   0.0e+00   2.5e-14
  t255      8.5e-16   0.0e+00   1.4e-14
  t256      6.1e-16   0.0e+00   8.3e-15
  t257      6.7e-16   0.0e+00   2.0e-14
  t512      1.6e-15   0.0e+00   5.8e-14
  h15       1.1e-15   0.0e+00   5.6e-14
  h16       1.1e-15   0.0e+00   5.6e-14
  h17       7.8e-16   0.0e+00   4.3e-14
  h256      1.0e-15   0.0e+00   1.3e-14
  h257      1.0e-15   0.0e+00   1.3e-14
  s5        2.4e-15   0.0e+00   4.3e-14
  s16       5.6e-16   0.0e+00   7.6e-14
  s32       1.1e-15   0.0e+00   6.4e-15
  s4        1.3e-15   0.0e+00   3.9e-15
  s32n32    2.9e-15   0.0e+00   1.0e-14
  s32n31    0.0e+00   0.0e+00   0.0e+00
  fb600     1.8e-15   0.0e+00   1.1e-16
  fb8       1.5e-15   0.0e+00   4.4e-16
  fb5       1.1e-15   0.0e+00   4.7e-15
  mc30      2.0e-15   0.0e+00   5.6e-15
  mc31      1.3e-15   0.0e+00   4.3e-14
  twin3     1.8e-13   0.0e+00   3.5e-14
  twin4     2.6e-15   0.0e+00   9.5e-15
  copies    0.0e+00   0.0e+00   0.0e+00
  rank2     0.0e+00   0.0e+00   0.0e+00
  err1      6.1e-16   0.0e+00   8.3e-15
  err6      1.2e-15   0.0e+00   2.8e-14
  last1     4.4e-16   0.0e+00   3.2e-14
  opt6      2.1e-15   0.0e+00   9.4e-14
  clamp     4.4e-14   0.0e+00   1.5e-12
The offsets are the negated row means: the tile partials of the device and numpy's sum gave the same bits everywhere.
The file runs in about 2 s.
"""
import ctypes as C

import numpy as np
import pytest

import tk_cases
import tk_restatement as R

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in tk_cases.PATH_CASES]

# name -> (status, iterations, usable_models, supported_models): None where the number is the seed's, not the path's
PATH = {
    "c4": (R.STATUS_RANSAC, 241, None, None), "c6": (R.STATUS_RANSAC, 241, None, None),
    "c7": (R.STATUS_RANSAC, 241, None, None), "c8w": (R.STATUS_RANSAC, 241, None, None),
    "t255": (R.STATUS_RANSAC, 241, None, None), "t256": (R.STATUS_RANSAC, 241, None, None),
    "t257": (R.STATUS_RANSAC, 241, None, None), "t512": (R.STATUS_RANSAC, 241, None, None),
    "h15": (R.STATUS_RANSAC, 15, None, None), "h16": (R.STATUS_RANSAC, 16, None, None),
    "h17": (R.STATUS_RANSAC, 17, None, None), "h256": (R.STATUS_RANSAC, 256, None, None),
    "h257": (R.STATUS_RANSAC, 257, None, None),
    "s5": (R.STATUS_RANSAC, 37, None, None), "s16": (R.STATUS_RANSAC, 64, None, None),
    "s32": (R.STATUS_RANSAC, 64, None, None), "s4": (R.STATUS_RANSAC, 16, None, None),
    "s32n32": (R.STATUS_RANSAC, 16, 16, 16), "s32n31": (R.STATUS_TOO_FEW, 0, 0, 0),
    "fb600": (R.STATUS_FALLBACK, 20, 20, 0), "fb8": (R.STATUS_FALLBACK, 20, 20, 0), "fb5": (R.STATUS_FALLBACK, 20, 20, 0),
    "mc30": (R.STATUS_RANSAC, 241, 241, 241), "mc31": (R.STATUS_FALLBACK, 241, 241, 0),
    "twin3": (R.STATUS_FALLBACK, 241, 0, 0), "twin4": (R.STATUS_FALLBACK, 241, 0, 0),
    "copies": (R.STATUS_DEGENERATE, 241, 0, 0), "rank2": (R.STATUS_DEGENERATE, 241, 0, 0),
    "err1": (R.STATUS_RANSAC, 241, None, None), "err6": (R.STATUS_RANSAC, 241, None, None),
    "last1": (R.STATUS_RANSAC, 241, None, None), "opt6": (R.STATUS_RANSAC, 292, None, None),
    "clamp": (R.STATUS_RANSAC, 1, 1, 1),
}


def _align(name):
    from orthosfm_amd import tk
    c = tk_cases.BY_NAME[name]
    xy, _, _ = tk_cases.build(name)
    opts = tk_cases.options(name)
    group = opts.pop("group_id")
    return tk.align(xy, c.width, c.height, group_id=group, **opts)


def _assert_path(name, got):
    """The path the case was chosen for, from the library's result alone."""
    c = tk_cases.BY_NAME[name]
    status, iterations, usable, supported = PATH[name]
    assert got.status == status and got.iterations == iterations and got.num_tracks == c.tracks
    if usable is not None:
        assert got.usable_models == usable
    if supported is not None:
        assert got.supported_models == supported
    ident = np.tile(np.eye(3), (c.cameras, 1, 1))
    if status == R.STATUS_RANSAC:
        assert 0 < got.supported_models <= got.usable_models <= iterations
        assert 0 <= got.best_iteration < iterations
        assert got.num_inliers == int(got.inlier.sum()) >= c.min_consensus + c.sample_size
    else:
        assert got.supported_models == 0 and got.best_iteration == -1
    if status == R.STATUS_FALLBACK:                     # all cases that end here are free of outliers
        assert got.num_inliers == c.tracks and got.inlier.all() and got.mean_error_px > 0
        assert not np.array_equal(got.basis_1, ident)
    if status in (R.STATUS_DEGENERATE, R.STATUS_TOO_FEW):
        assert got.num_inliers == 0 and got.mean_error_px == 0.0 and not got.inlier.any()
        assert np.array_equal(got.basis_1, ident) and np.array_equal(got.basis_2, ident) and not got.offsets.any()
    if name in ("h256", "h257"):
        assert got.best_iteration >= 16                 # beyond the first chunk
    if name == "h17":
        assert got.best_iteration == 16                 # alone in the last, ragged chunk
    if name == "s32n32":
        assert got.num_inliers == 32 and got.inlier.all()


@pytest.mark.parametrize("name", NAMES)
def test_path_case_against_restatement(name):
    ref = tk_cases.reference(name)
    got = _align(name)
    print(name, "status", got.status, "iterations", got.iterations, "usable", got.usable_models, "supported", got.supported_models,
          "best", got.best_iteration, "inliers", got.num_inliers, "mean", got.mean_error_px, "ref mean", ref.mean_error_px)
    print("observed %-8s basis %.1e  offsets %.1e  mean error %.1e" % (
        name, max(np.abs(got.basis_1 - ref.basis_1).max(), np.abs(got.basis_2 - ref.basis_2).max()),
        np.abs(got.offsets - ref.offsets).max(), abs(got.mean_error_px - ref.mean_error_px)))
    _assert_path(name, got)
    assert got.status == ref.status
    assert got.iterations == ref.iterations
    assert got.usable_models == ref.usable_models
    assert got.supported_models == ref.supported_models
    assert got.num_inliers == ref.num_inliers
    assert np.array_equal(got.inlier, ref.inlier)
    assert abs(got.mean_error_px - ref.mean_error_px) <= 1e-8
    if name != "s32n32":        # every hypothesis is the same 32 tracks in another order: the means differ at 1e-14
        assert got.best_iteration == ref.best_iteration
    assert np.abs(got.basis_1 - ref.basis_1).max() <= 1e-8
    assert np.abs(got.basis_2 - ref.basis_2).max() <= 1e-8
    assert np.abs(got.offsets - ref.offsets).max() <= 1e-8


@pytest.mark.parametrize("name", ["fb600", "c8w", "s32"])
def test_repeatable_to_the_byte(name):
    """The fallback's tile partials over three tiles, the C = 8 scoring over three tiles, a sample of 32."""
    a, b = _align(name), _align(name)
    _assert_path(name, a)
    for f in ("basis_1", "basis_2", "offsets", "inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.status, a.iterations, a.usable_models, a.supported_models, a.best_iteration, a.num_inliers) == \
        (b.status, b.iterations, b.usable_models, b.supported_models, b.best_iteration, b.num_inliers)
    assert np.float64(a.mean_error_px).tobytes() == np.float64(b.mean_error_px).tobytes()


def test_sample_size_limits():
    """The raw call: 4 and 32 are sample sizes (the cases s4, s32), 3 and 33 are not; 31 tracks are too few for 32."""
    from orthosfm_amd import capi
    xy = np.ascontiguousarray(tk_cases.build("s32")[0])

    def raw(sample_size, n):
        o = capi.TkOptions()
        capi.check(capi.lib.osfm_tk_options_default(C.byref(o)))
        o.sample_size, o.max_iterations, o.seed = sample_size, 16, 42
        b1, b2 = np.full((3, 9), 7.0), np.full((3, 9), 7.0)
        r = capi.TkResult()
        st = capi.lib.osfm_tk_align(xy.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(n), C.c_int32(3), C.c_int32(2048),
                                    C.c_int32(2048), C.byref(o), C.c_uint64(0), capi._ptr(b1, C.c_double),
                                    capi._ptr(b2, C.c_double), None, None, C.byref(r))
        return st, r, b1

    assert raw(33, 300)[0] == capi.E_ARG
    assert raw(3, 300)[0] == capi.E_ARG
    for s in (4, 32):
        st, r, _ = raw(s, 300)
        assert st == capi.OK and r.iterations == 16 and r.status in (capi.TK_RANSAC, capi.TK_FALLBACK)
    st, r, b1 = raw(32, 31)
    assert st == capi.OK and r.status == capi.TK_TOO_FEW and r.iterations == 0 and r.best_iteration == -1
    assert np.array_equal(b1, np.tile(np.eye(3).reshape(9), (3, 1)))


def test_scene_form_at_five_views():
    """A scene of 7 views and 400 tracks, some flags cleared; views 5, 1, 6, 0, 3 -- in this order -- carry the c5
    group.  The scene selects the live tracks all five views see and gathers them on the device; the same selection
    made on the host and handed to osfm_tk_align gives the same bytes."""
    from orthosfm_amd import tk
    from orthosfm_amd.scene import Scene
    rng = np.random.default_rng(7)
    xy5, _, _ = tk_cases.build("c5")
    group = [5, 1, 6, 0, 3]
    others = [2, 4]
    V, T = 7, 400
    views_of, feats = [], []
    for t in range(T):
        if t < 300:
            vs = list(group) + [v for v in others if rng.random() < 0.5]
        else:
            vs = [v for v in range(V) if rng.random() < 0.6] or [2]
            if set(group) <= set(vs):
                vs.remove(group[t % 5])
        vs = sorted(vs)
        views_of.append(vs)
        for v in vs:
            feats.append(xy5[t, group.index(v)] if t < 300 and v in group else rng.uniform(0, 2048, 2))
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in views_of])]).astype(np.int64)
    feat_view = np.concatenate(views_of).astype(np.int32)
    feat_xy = np.array(feats, dtype=np.float32)
    alive_t = rng.random(T) > 0.1
    alive_f = rng.random(feat_view.shape[0]) > 0.03
    sc = Scene(0, np.full(V, 2048, np.int32), np.full(V, 2048, np.int32), offsets, feat_view, feat_xy)
    sc.set_flags(alive_t, alive_f)
    rows = []
    for t in range(T):
        if not alive_t[t]:
            continue
        f = {int(feat_view[k]): k for k in range(offsets[t], offsets[t + 1]) if alive_f[k]}
        if all(v in f for v in group):
            rows.append([feat_xy[f[v]].astype(np.float64) for v in group])
    xy = np.array(rows)
    assert 150 < xy.shape[0] < 300 and xy.shape[1:] == (5, 2)
    a = sc.tk_align(group, group_id=2, seed=9)
    sc.close()
    b = tk.align(xy, 2048, 2048, group_id=2, seed=9)
    assert a.num_tracks == xy.shape[0] and a.status == b.status == R.STATUS_RANSAC
    for f in ("basis_1", "basis_2", "offsets", "inlier"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.iterations, a.usable_models, a.supported_models, a.best_iteration, a.num_inliers, a.mean_error_px) == \
        (b.iterations, b.usable_models, b.supported_models, b.best_iteration, b.num_inliers, b.mean_error_px)
    assert a.iterations == 241 and a.supported_models > 0 and a.num_inliers >= 35
