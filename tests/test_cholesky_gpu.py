"""The bundle adjustment's dense Cholesky solve (orthosfm_amd/csrc/ba_cholesky.hip) against a high-precision solve
of the same system, in each of its regimes, through osfm_ba_debug_cholesky_solve: the solve osfm_ba_solve runs on a
reduced camera system of more than one block, on a batch of systems that share one set of work arrays as the
iterations of the LM loop do (hand-off flags zeroed once, a new epoch per system, the factor's matrix filled with
NaN once and never cleared).  A tile read before its producer wrote it is the previous system's: every system of a
batch is a different matrix, so that read is an error the checker sees (tests/chol_cases.py; its power is shown
without a device in tests/test_chol_cases_cpu.py).

Every solution must pass the textbook bounds -- backward error <= n 2^-53, forward error <= 4 n 2^-53 kappa_inf --
in both forms (the one-launch form and launch per block column), and the one-launch form repeats bit for bit.

Observed on MI355X, first run (largest over the solutions of each regime; backward error: the larger of the plain
and the equilibrated one; forward error, and as a share of its bound -- the bounds above are what is asserted):
  one launch, D per row, no P tiles (n <= 96)           12 solutions  backward 1.3e-16  forward 7.8e-07 (3.2e-04)
  one launch, D per row, one P per tile                 32            3.3e-16           6.3e-07 (2.3e-04)
  one launch, D per row, P round robin (n 995, 1760)     6            8.1e-16           7.7e-10 (1.7e-04)
  one launch, D shared, one P per tile (forced grids)    9            3.1e-16           1.2e-10 (8.6e-05)
  one launch, D shared, P round robin                   29            4.9e-16           2.6e-07 (8.6e-05)
  one launch, ordered layout (D per row / shared)       32            2.8e-16           6.2e-07 (1.0e-04)
  launch per column                                     70            7.8e-16           3.0e-06 (3.2e-04)
The device's capacity was 460 workgroups: the P tiles get a workgroup each up to 31 blocks (n <= 992) and are dealt
round robin from 32 blocks (n = 995: 427 P workgroups for 435 tiles) on.  The file runs in about 12 s."""
import numpy as np
import pytest

import chol_cases as cc

pytestmark = pytest.mark.gpu

K_FLOW_ABORTED = 1 << 20
SIZES = {33: "sparse", 64: "sparse", 65: "band", 96: "sparse", 97: "sparse", 128: "band", 129: "sparse", 160: "dense",
         300: "graded", 995: "dense", 1760: "sparse", 1761: "band", 1792: "sparse", 1793: "dense", 2495: "sparse",
         5120: "band", 5121: "sparse"}
RINGS = [(200, 11, True), (500, 11, True), (120, 11, True), (96, 7, False), (64, 5, True)]
OBSERVED = {}


@pytest.fixture(scope="module")
def ba():
    from orthosfm_amd import ba as m
    from orthosfm_amd import capi
    assert capi.device_count() >= 1
    return m


_refs = {}


def _reference(key, batch, r):
    if (key, r) not in _refs:
        _refs[(key, r)] = cc.reference(batch.A[r], batch.b[r])
    return _refs[(key, r)]


def regime(launch):
    if not launch["one_launch"]:
        return "launch per column"
    p = "no P tiles" if launch["num_tiles"] == 0 else \
        "one P per tile" if launch["num_p"] >= launch["num_tiles"] else "P round robin"
    d = "D shared" if launch["num_d"] < launch["nblk"] + 1 else "D per row"
    return f"one launch, {d}, {p}" + (", ordered" if launch["arcs"] else "")


def _check_all(key, batch, x, info, launch, rows=None):
    """Every system of the batch (or those in rows) solved: info 0 and within the bounds; the errors recorded."""
    for r in (range(batch.A.shape[0]) if rows is None else rows):
        assert info[r] == 0, (key, r, int(info[r]), launch)
        c = cc.check_solution(batch.A[r], batch.b[r], x[r], _reference(key, batch, r))
        assert c.ok, (key, r, regime(launch), str(c))
        o = OBSERVED.setdefault(regime(launch), [0.0, 0.0, 0.0, 0])
        o[0] = max(o[0], c.eta, c.eta_s)
        o[1] = max(o[1], c.fwd)
        o[2] = max(o[2], c.fwd / c.fwd_bound)
        o[3] += 1


_batches = {}


def _size_batch(n):
    if n not in _batches:
        _batches[n] = cc.size_batch(n, 3 if n <= 2500 else 2, SIZES[n], n)
    return _batches[n]


@pytest.mark.parametrize("n", sorted(SIZES))
def test_sizes_in_both_forms(ba, n):
    """Natural order at the sizes where the regimes switch: no P tiles (n <= 96) / the first P tiles (4 and 5
    blocks), a D workgroup per block row up to 1760 unknowns and shared D's from 1761 on, the one-launch form up to
    5120 and launch per column beyond; whether the P tiles have a workgroup each depends on the device (recorded)."""
    B = _size_batch(n)
    x, info, L = ba.debug_cholesky_solve(B.A, B.b)
    nblk = (n + 31) // 32
    assert L["nblk"] == nblk and L["span"] == n and L["arcs"] == 0
    if n <= 5120:
        assert L["one_launch"] == 1
        assert L["num_tiles"] == sum(max(nblk - 3 - j, 0) for j in range(nblk))
        if nblk <= 3:
            assert L["num_tiles"] == 0
        if nblk in (4, 5):
            assert L["num_tiles"] == nblk * 2 - 7         # 1, 3: the right-hand side's row first
        if n <= 1760:
            assert L["num_d"] == nblk + 1
        else:
            assert L["num_d"] == 56 and L["num_d"] < nblk + 1
    else:
        assert L["one_launch"] == 0
    _check_all(n, B, x, info, L)
    print(f"n {n}: {regime(L)}: groups {L['groups']}, D {L['num_d']}, P {L['num_p']} for {L['num_tiles']} tiles")
    x2, info2, _ = ba.debug_cholesky_solve(B.A, B.b)
    assert np.array_equal(info2, info) and np.array_equal(x2, x)       # bit for bit
    xc, infoc, Lc = ba.debug_cholesky_solve(B.A, B.b, form=ba.FORM_PER_COLUMN)
    assert Lc["one_launch"] == 0
    _check_all(n, B, xc, infoc, Lc)


@pytest.mark.parametrize("max_d,max_groups", [(1, 1), (2, 1), (3, 1), (7, 1), (2, 0), (3, 0), (7, 0)])
def test_forced_grids(ba, max_d, max_groups):
    """20 blocks (640 unknowns, 153 P tiles) with the grid forced: shared D's (a D for every block row down to one for
    all 21 rows) and the fewest workgroups the D's allow (max_groups 1: one P workgroup for every tile with a single
    D) or as many as the tiles want."""
    B = _size_batch_forced()
    x, info, L = ba.debug_cholesky_solve(B.A, B.b, max_d=max_d, max_groups=max_groups)
    d_span = 8 * (max_d - 1) + 1
    assert L["one_launch"] == 1 and L["nblk"] == 20 and L["num_tiles"] == 153 and L["num_d"] == max_d < 21
    if max_groups == 1:
        assert L["groups"] == d_span + 1 and L["num_p"] == d_span + 1 - min((d_span + 8) >> 3, max_d) < 153
        if max_d == 1:
            assert L["num_p"] == 1
    else:
        assert L["num_p"] >= 153
    _check_all("forced", B, x, info, L)
    x2, _, _ = ba.debug_cholesky_solve(B.A, B.b, max_d=max_d, max_groups=max_groups)
    assert np.array_equal(x2, x)


def _size_batch_forced():
    if "forced" not in _batches:
        _batches["forced"] = cc.size_batch(640, 3, "sparse", 640)
    return _batches["forced"]


def test_overrides_that_cannot_run_are_refused(ba):
    from orthosfm_amd import capi
    A = np.eye(5121)[None]
    with pytest.raises(capi.OsfmError) as e:
        ba.debug_cholesky_solve(A, np.ones((1, 5121)), max_d=2)          # 161 blocks: no one-launch form
    assert e.value.status == capi.E_ARG


@pytest.mark.parametrize("cams,w,closed", RINGS)
def test_ordered_layout(ba, cams, w, closed):
    """Rings and a strip laid out as arcs and separators (ba_order.hip) with interior padding rows and the block
    pattern that skips zero tiles, in both forms and with one D and one P workgroup for the whole grid; and the natural order of the
    same batch."""
    B = cc.ring_batch(cams, w, closed, 3, cams)
    key = ("ring", cams)
    order = cc.order_info(B.ldim, B.pairs)
    assert order["ordered"] == 1 and order["arcs"] > 0
    x, info, L = ba.debug_cholesky_solve(B.A, B.b, B.ldim, B.pairs)
    assert L["one_launch"] == 1 and L["arcs"] == order["arcs"] and L["span"] == B.n + order["pad"] == order["span"]
    _check_all(key, B, x, info, L)
    x2, _, _ = ba.debug_cholesky_solve(B.A, B.b, B.ldim, B.pairs)
    assert np.array_equal(x2, x)
    xc, infoc, Lc = ba.debug_cholesky_solve(B.A, B.b, B.ldim, B.pairs, form=ba.FORM_PER_COLUMN)
    assert Lc["one_launch"] == 0 and Lc["arcs"] == order["arcs"]
    _check_all(key, B, xc, infoc, Lc)
    xf, infof, Lf = ba.debug_cholesky_solve(B.A, B.b, B.ldim, B.pairs, max_d=1, max_groups=1)
    assert Lf["one_launch"] == 1 and Lf["num_d"] == 1 and Lf["num_p"] == 1 and Lf["arcs"] == order["arcs"]
    _check_all(key, B, xf, infof, Lf)
    xn, infon, Ln = ba.debug_cholesky_solve(B.A, B.b)
    assert Ln["arcs"] == 0 and Ln["span"] == B.n
    _check_all(key, B, xn, infon, Ln)


def _expected_info(nblk, k, blocks=None):
    """The info word of a factorisation whose first pivot that is not positive lies in block k: a failing pivot
    leaves NaNs that every later block reached from block k through the factor's pattern (all of them without a
    pattern) inherits, each such block fails in every panel, and info keeps the largest position
    (ba_cholesky.hip: kblock * 32 + the first row of the panel + 1) -- the last panel, rows 28..31, of the last block
    reached."""
    reached = {k}
    for j in range(k + 1, nblk):
        if blocks is None or any((int(blocks[j, c >> 6]) >> (c & 63)) & 1 for c in reached):
            reached.add(j)
    return 32 * max(reached) + 28 + 1


def test_not_positive_definite(ba):
    """A pivot that is not positive in the middle of a 15-block system (a ring of 120 cameras): every form reports
    0 < info < kFlowAborted at the position the rule yields, and the positive definite system solved next on the
    same flags and epochs is right."""
    B = cc.ring_batch(120, 11, True, 3, 120)
    off, blocks, order = cc.order_layout(B.ldim, B.pairs)
    nblk = (B.n + 31) // 32
    assert nblk >= 10
    u = (nblk // 2) * 32 + 13                      # block nblk / 2 of the natural order
    A = np.array(B.A)
    A[1] = cc.indefinite_at(A[1], u)
    # where u sits in the ordered layout
    cam = int(np.searchsorted(np.cumsum(B.ldim), u, side="right"))
    pos = int(off[cam] + u - (np.cumsum(B.ldim)[cam] - B.ldim[cam]))
    cases = [(dict(), _expected_info(nblk, u // 32)),
             (dict(form=ba.FORM_PER_COLUMN), _expected_info(nblk, u // 32)),
             (dict(cam_ldim=B.ldim, pairs=B.pairs), _expected_info(order["nblk"], pos // 32, blocks)),
             (dict(cam_ldim=B.ldim, pairs=B.pairs, form=ba.FORM_PER_COLUMN), _expected_info(order["nblk"], pos // 32))]
    for kw, want in cases:
        x, info, L = ba.debug_cholesky_solve(A, B.b, **kw)
        assert 0 < info[1] < K_FLOW_ABORTED and info[1] == want, (kw.keys(), int(info[1]), want, L)
        assert L["arcs"] == (order["arcs"] if "cam_ldim" in kw else 0)
        _check_all(("npd", 120), B, x, info, L, rows=(0, 2))


def test_a_launch_given_up_reports_it(ba):
    """With every wait that is not satisfied at once giving the launch up (the library's own hook): a system reports
    info >= kFlowAborted or is solved right -- never a wrong x with info 0; the next batch is right again."""
    from orthosfm_amd import capi
    B = _size_batch_forced()
    capi.check(capi.lib.osfm_ba_debug_flow_spin_limit(1))
    try:
        x, info, L = ba.debug_cholesky_solve(B.A, B.b)
    finally:
        capi.check(capi.lib.osfm_ba_debug_flow_spin_limit(0))
    assert L["one_launch"] == 1
    aborted = info >= K_FLOW_ABORTED
    assert aborted.any(), info
    assert np.all(aborted | (info == 0)), info
    done = [r for r in range(3) if info[r] == 0]
    _check_all("forced", B, x, info, L, rows=done)
    x2, info2, L2 = ba.debug_cholesky_solve(B.A, B.b)
    _check_all("forced", B, x2, info2, L2)


def test_zz_observed_errors():
    """(The largest errors per regime of this run, printed for the record: pytest -rP shows them.)"""
    for k, (eta, fwd, rel, cnt) in sorted(OBSERVED.items()):
        print(f"{k}: {cnt} solutions, backward error <= {eta:.3g}, forward error <= {fwd:.3g} ({rel:.3g} of its bound)")
