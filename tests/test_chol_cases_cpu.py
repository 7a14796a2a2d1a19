"""The matrices and the checker of tests/test_cholesky_gpu.py, without a device: the cases have the shape they claim,
the checker passes an exact solve and has the power to reject the wrong solves it exists for (one tile off by 1e-9,
a block update dropped), and osfm_ba_debug_cholesky_solve refuses bad arguments before it looks for a device."""
import numpy as np
import pytest

import chol_cases as cc


def _tile(A, i, j, nb=32):
    return A[i * nb:(i + 1) * nb, j * nb:(j + 1) * nb]


def _largest_off_tile(A, nb=32):
    nblk = A.shape[0] // nb
    best = max(((i, j) for i in range(nblk) for j in range(i)), key=lambda t: np.abs(_tile(A, *t)).max())
    assert np.abs(_tile(A, *best)).max() > 0.05
    return best


@pytest.mark.parametrize("n,kind", [(97, "sparse"), (300, "graded"), (640, "band"), (700, "dense")])
def test_exact_solve_passes_and_a_tile_off_by_1e_9_fails(n, kind):
    B = cc.size_batch(n, 3, kind, n)
    for r in range(3):
        A, b = B.A[r], B.b[r]
        ref = cc.reference(A, b)
        assert cc.check_solution(A, b, np.asarray(ref.x, dtype=np.float64), ref).ok
        assert cc.check_solution(A, b, np.linalg.solve(A, b), ref).ok
        i, j = _largest_off_tile(A)
        bad = np.linalg.solve(cc.perturb_tile(A, i, j, 1e-9, seed=r), b)
        c = cc.check_solution(A, b, bad, ref)
        assert not c.ok, (kind, r, str(c))


@pytest.mark.parametrize("n,kind,drop", [(160, "sparse", (3, 2, 0)), (300, "dense", (6, 4, 3)), (640, "band", (12, 12, 11))])
def test_a_dropped_block_update_fails(n, kind, drop):
    B = cc.size_batch(n, 3, kind, n + 7)
    A, b = B.A[0], B.b[0]
    ref = cc.reference(A, b)
    assert cc.check_solution(A, b, cc.solve_with_factor(cc.blocked_cholesky(A), b), ref).ok
    L = cc.blocked_cholesky(A, drop=drop)
    i, j, k = drop
    assert np.abs(_tile(L, i, k)).max() > 0 and np.abs(_tile(L, j, k)).max() > 0      # the update was not a zero
    c = cc.check_solution(A, b, cc.solve_with_factor(L, b), ref)
    assert not c.ok, str(c)


def test_the_stale_tile_of_the_previous_system_fails():
    """What a consumer that reads a tile before its producer wrote it gets: the same tile of the system before."""
    B = cc.size_batch(300, 3, "sparse", 11)
    for r in (1, 2):
        A, b = B.A[r], B.b[r]
        i, j = _largest_off_tile(A)
        S = np.array(A)
        S[i * 32:(i + 1) * 32, j * 32:(j + 1) * 32] = _tile(B.A[r - 1], i, j)
        S[j * 32:(j + 1) * 32, i * 32:(i + 1) * 32] = _tile(B.A[r - 1], i, j).T
        assert not cc.check_solution(A, b, np.linalg.solve(S, b)).ok


def test_cases_have_the_shape_of_a_reduced_camera_system():
    rng = np.random.default_rng(0)
    for n in (33, 995, 5121):
        ldim = cc.mixed_ldim(n, rng)
        assert ldim.sum() == n and set(ldim[:-1].tolist()) <= set(cc.LDIMS) and 1 <= ldim[-1] <= 7
    B = cc.size_batch(640, 5, "sparse", 3)
    B = cc.make_batch(B.ldim, cc.sparse_tracks(len(B.ldim), np.random.default_rng(4)), 5, 0, mus=cc.MUS)
    kappas = []
    for r in range(5):
        A = B.A[r]
        assert np.array_equal(A, A.T) and np.allclose(np.diag(A), 1.0)
        kappas.append(cc.reference(A, B.b[r]).kappa)
        # every tile the camera pairs allow holds entries of order one, every other tile is zero
        off = np.concatenate([[0], np.cumsum(B.ldim)])
        allowed = np.zeros((20, 20), dtype=bool)
        for a, c in B.pairs:
            for x in range(off[a] // 32, (off[a + 1] - 1) // 32 + 1):
                for y in range(off[c] // 32, (off[c + 1] - 1) // 32 + 1):
                    allowed[max(x, y), min(x, y)] = True
        for i in range(20):
            for j in range(i + 1):
                assert (np.abs(_tile(A, i, j)).max() > 1e-2) == allowed[i, j], (i, j)
    # mu 1e-1 .. 1e-10: condition numbers from about 1e1 to about 1e12
    assert 1e1 <= kappas[0] <= 1e3 and 1e10 <= kappas[-1] <= 1e13 and np.all(np.diff(kappas) > 0)
    assert not np.allclose(B.A[0], B.A[1]) and not np.allclose(B.b[0], B.b[1])
    G = cc.size_batch(300, 3, "graded", 5)
    d = np.diag(G.A[0])
    assert d.min() < 1e-5 and d.max() > 1e5


@pytest.mark.parametrize("cams,w,closed", [(200, 11, True), (500, 11, True), (120, 11, True), (96, 7, False), (64, 5, True)])
def test_ring_and_strip_cases_get_an_elimination_order(cams, w, closed):
    """The ordered-layout cases of the GPU test are laid out as arcs and separators (host code: osfm_ba_debug_order)."""
    B = cc.ring_batch(cams, w, closed, 1, cams)
    info = cc.order_info(B.ldim, B.pairs)
    assert info["ordered"] == 1 and info["arcs"] >= 2 and info["sep"] == w
    assert info["span"] == B.n + info["pad"]


def test_debug_cholesky_solve_refuses_bad_arguments():
    from orthosfm_amd import ba, capi
    B = cc.size_batch(64, 1, "sparse", 1)
    A, b = B.A, B.b

    def refused(*args, **kw):
        with pytest.raises(capi.OsfmError) as e:
            ba.debug_cholesky_solve(*args, **kw)
        assert e.value.status == capi.E_ARG, e.value

    refused(A[:, :32, :32], b[:, :32])                                # one block: chol_small_kernel's
    refused(A, b, form=2)
    refused(A, b, max_d=-1)
    refused(A, b, max_groups=-3)
    refused(A, b, form=ba.FORM_PER_COLUMN, max_d=2)                  # the launch-per-column form has no D's
    refused(A, b, cam_ldim=B.ldim[:-1], pairs=B.pairs[:1])            # cameras short of n unknowns
    refused(A, b, cam_ldim=B.ldim, pairs=np.array([[0, len(B.ldim)]]))
    bad = np.array(B.ldim)
    bad[0] = -bad[0]
    refused(A, b, cam_ldim=bad)
    if capi.device_count() == 0:
        with pytest.raises(capi.OsfmError) as e:
            ba.debug_cholesky_solve(A, b, cam_ldim=B.ldim, pairs=B.pairs)
        assert e.value.status == capi.E_DEVICE
