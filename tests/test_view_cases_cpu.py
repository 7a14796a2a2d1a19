"""The numpy restatement of the view front end's halving chain (tests/view_cases.py) against the reference's bytes
(tests/golden/halve_reference.npz, written by tests/golden/make_halve_golden.py), and the chain's int arithmetic."""
import numpy as np
import pytest

import view_cases as vc


def test_the_fixture_holds_every_shape():
    shapes = {(a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2]) for a in vc.halve_images().values()}
    assert set(vc.HALVE_SHAPES) <= shapes
    chains = {vc.chain_name(w, h, k) for w, h, n in vc.HALVE_CHAINS for k in range(1, n + 1)}
    assert set(vc.halve_images()) | chains | {"refused"} == set(vc.golden())


@pytest.mark.parametrize("name", sorted(vc.halve_images()))
def test_restatement_equals_the_reference(name):
    img, want = vc.halve_images()[name], vc.golden()[name]
    got = vc.halve(img)
    assert got.shape == want.shape == (((img.shape[0] + 1) >> 1, (img.shape[1] + 1) >> 1) + img.shape[2:])
    assert got.tobytes() == want.tobytes()


def test_the_grey8_shapes_stand_on_the_kernels_edges():
    """halve_grey8_kernel (grey, w % 8 == 0; a thread per 8 source bytes of two rows, 256 threads a workgroup): even and
    odd heights, one quad per row, a work count over two workgroups that is no multiple of 256."""
    work = {(w, h): (w // 8) * ((h + 1) >> 1) for w, h, c in vc.GREY8_SHAPES}
    assert all(vc.takes_grey8(w, c) for w, h, c in vc.GREY8_SHAPES) and not vc.takes_grey8(8, 3) and not vc.takes_grey8(132, 1)
    assert work[8, 2] == 1 and work[8, 3] == 2                                     # w == 8: one quad per row
    assert {h % 2 for w, h, c in vc.GREY8_SHAPES} == {0, 1}
    assert sum(h % 2 for w, h, c in vc.GREY8_SHAPES) >= 5                          # y1 = min(2y + 1, h - 1) clamps
    assert work[72, 57] == 261 and 256 < work[72, 57] < 512 and work[72, 57] % 256 == 5
    assert work[64, 64] == 256 and work[264, 3] == 66


def test_chains_equal_the_reference_step_by_step():
    """Every step of the grey chains against the reference halving its own last result, and the kernel each step takes."""
    taken = {}
    for (w, h, n), img in vc.chain_images().items():
        assert img.shape == (h, w)
        for step in range(1, n + 1):
            taken.setdefault((w, h), []).append(vc.takes_grey8(img.shape[1], 1))
            img = vc.halve(img)
            want = vc.golden()[vc.chain_name(w, h, step)]
            assert img.shape == want.shape and img.tobytes() == want.tobytes(), (w, h, step)
        assert vc.chain(vc.chain_images()[w, h, n], n + 1, 0)[1].tobytes() == img.tobytes()
    assert taken[72, 57] == [True, False, False]          # 72 -> 36 -> 18 -> 9
    assert taken[132, 80] == [False, False, False]        # 132 -> 66 -> 33 -> 17
    assert taken[143, 10] == [False, True, False]         # 143 -> 72 (5 high: odd) -> 36 -> 18
    assert vc.golden()[vc.chain_name(132, 80, 3)].shape == (10, 17) and vc.golden()[vc.chain_name(143, 10, 1)].shape == (5, 72)


def test_the_golden_sees_a_dropped_last_row():
    """A halving that does not repeat the last row of an odd height (it takes the row above instead) differs from the
    reference on every new shape of odd height, on both kernels' shapes, and on the 8-byte step of a chain."""
    seen = {name for name, img in vc.halve_images().items()
            if vc.halve(img, plant_drop_last_row=True).tobytes() != vc.golden()[name].tobytes()}
    odd = {f"random_{w}x{h}x{c}" for w, h, c in vc.HALVE_SHAPES if h % 2}
    assert seen == odd                                     # all255_5x7x3 is odd too, and cannot show it
    assert {"random_8x3x1", "random_16x5x1", "random_24x7x1", "random_72x57x1", "random_264x3x1"} <= seen
    step1 = vc.halve(vc.chain_images()[143, 10, 3])
    assert step1.shape == (5, 72)
    assert vc.halve(step1, plant_drop_last_row=True).tobytes() != vc.golden()[vc.chain_name(143, 10, 2)].tobytes()


def test_the_cases_hold_every_remainder_and_the_top_of_the_range():
    for r in (1, 2, 3):
        for kind in ("low", "high"):
            assert int(vc.halve_images()[f"sum{r}_{kind}"].astype(int).sum()) % 4 == r
    w = vc.halve_images()["patches_64x64x1"].astype(int)
    assert [int(w[0:2, x:x + 2].sum()) % 4 for x in (0, 2, 4)] == [1, 2, 3]
    assert [int(w[62:64, x:x + 2].sum()) % 4 for x in (58, 60, 62)] == [1, 2, 3]
    for name in ("all255_5x7x3", "all255_64x64x1"):
        assert (vc.golden()[name] == 255).all()


def test_a_size_below_two_is_refused():
    w, h, _ = vc.REFUSED_SHAPE
    assert bool(vc.golden()["refused"])
    with pytest.raises(ValueError):
        vc.halve(np.zeros((h, w), np.uint8))
    with pytest.raises(ValueError):
        vc.chain(np.zeros((h, w), np.uint8), downscale_factor=2)


def test_chain_arithmetic():
    img = vc.halve_images()["random_65x63x3"]
    imported, feat, n = vc.chain(img, max_image_size=1000)          # 4095 -> 33 x 32 = 1056 -> 17 x 16 = 272
    assert n == 2 and imported.shape == img.shape and feat.shape == (16, 17, 3)
    assert feat.tobytes() == vc.halve(vc.halve(img)).tobytes()
    imported, feat, n = vc.chain(img, downscale_factor=3, max_image_size=0)
    assert n == 2 and imported.shape == feat.shape == (16, 17, 3)
    imported, feat, n = vc.chain(img, downscale_factor=2, max_image_size=1000)      # 1056 > 1000: one more
    assert n == 2 and imported.shape == (32, 33, 3) and feat.shape == (16, 17, 3)
    for limit in (0, -1):
        imported, feat, n = vc.chain(img, max_image_size=limit)
        assert n == 0 and feat is imported and feat.tobytes() == img.tobytes()
    assert vc.chain(img, max_image_size=4095)[2] == 0 and vc.chain(img, max_image_size=4094)[2] == 1


def test_the_golden_sees_a_planted_rounding_error():
    """Rounding down instead of to nearest differs on every patch whose sum is 2 or 3 mod 4."""
    seen = [name for name, img in vc.halve_images().items() if vc.halve(img, round_down=True).tobytes() != vc.golden()[name].tobytes()]
    assert {"sum2_low", "sum3_low", "sum2_high", "sum3_high", "patches_64x64x1", "random_257x190x1"} <= set(seen)
    assert "sum1_low" not in seen and "all255_5x7x3" not in seen


def test_hostile_pools_sit_on_the_boundaries():
    from orthosfm_amd import capi
    p = vc.sift_pool()
    q = capi.quantize_sift(np.resize(p, (p.size + 127) // 128 * 128))[:].reshape(-1)[:p.size]
    assert set(q.tolist()) == set(range(256))
    # the five floats around a boundary fall on both of its sides
    for k in (0, 1, 127, 128, 254):
        five = q[6 * k + 1:6 * k + 6]
        assert set(five.tolist()) == {k, k + 1}
    u = vc.surf_pool()
    r = capi.quantize_surf(np.resize(u, (u.size + 63) // 64 * 64)).reshape(-1)[:u.size]
    assert set(r.tolist()) == set(range(-127, 128))
    sift, surf, pos = vc.bank_case(257, 257, "block_edge", 3)
    qs = capi.quantize_sift(sift)
    assert sorted(np.nonzero(qs.max(axis=1) > 127)[0].tolist()) == [255, 256]
    assert pos.shape == (514, 2) and surf.shape == (257, 64)
