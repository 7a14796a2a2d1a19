"""The correction-free tile kernel leaves its unrolled 16-tile cycle behind the segment's last real tile.

What is open at such an exit is what these cases look at: the row-direction groups of all 32 slots, whose first
tiles depend on where in the cycle the exit lies, and the column partials of the last two to five tiles (all of
them when the segment ends before tile 5), which the loop has not merged yet.  A wrong first tile makes the
finish rescan the wrong columns for a row whose best lies in such a group; a missed or misplaced merge loses the
2->1 result of a column of those tiles.  Both show in a list only where the oracle accepts a match there, so
every case first asserts, on the CPU and from the oracle's lists alone, that each of the last min(16, ntiles)
tiles holds an accepted 1->2 match column and an accepted 2->1 query column.  Then every list is compared
exactly.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases
import match_tile_exit_child as child
import oracle_lib

pytestmark = pytest.mark.gpu

TILE = 64
ROWS = 256
_NO_SURF = np.zeros((0, 64), np.int16)
_NO_SIFT = np.zeros((0, 128), np.uint16)

# every exit point of a first cycle (k tiles, the last three columns short), one column, one full tile, a full cycle
FIRST_N1 = 300                      # two row blocks, the second of 44 rows
FIRST_N2 = tuple(TILE * k - 3 for k in range(1, 17)) + (1, 64, 1024)


@pytest.fixture(scope="module")
def hm():
    from orthosfm_amd import capi
    from orthosfm_amd.matching import HipExhaustiveMatching
    assert capi.device_count() >= 1, "no HIP device"
    return HipExhaustiveMatching


def ntiles_of(n2):
    return (n2 + TILE - 1) // TILE


def assert_tail_tiles_matched(e12, e21, n1, n2, off12=0, off21=0):
    """Each of the last min(16, ntiles) tiles of set 2 holds a column some row of set 1 is matched to, and a column
    that is itself matched (the oracle's lists; off12 / off21: where this descriptor type starts in them)."""
    nt = ntiles_of(n2)
    to = e12[off12:off12 + n1]
    to = to[to >= 0] - off21
    hit12 = np.bincount(to // TILE, minlength=nt) > 0
    hit21 = np.bincount(np.nonzero(e21[off21:off21 + n2] >= 0)[0] // TILE, minlength=nt) > 0
    for t in range(max(nt - 16, 0), nt):
        assert hit12[t], f"no accepted 1->2 match into tile {t} of {nt}"
        assert hit21[t], f"no accepted 2->1 query in tile {t} of {nt}"


@functools.lru_cache(maxsize=None)
def first_case(n2):
    s1, s2 = match_cases.sift_pair(FIRST_N1, n2, min(FIRST_N1, n2), 9000 + n2)
    assert int(max(s1.max(), s2.max())) <= 127          # ordinary descriptors only: the correction-free kernel
    e12, e21 = oracle_lib.oracle_pairwise_match(s1, _NO_SURF, s2, _NO_SURF)
    assert_tail_tiles_matched(e12, e21, FIRST_N1, n2)
    for a in (s1, s2, e12, e21):
        a.setflags(write=False)
    return s1, s2, e12, e21


def match_pair(hm, s1, u1, s2, u2):
    m = hm(2)
    m.set_view(0, s1, u1)
    m.set_view(1, s2, u2)
    got = m.pairwise_match(0, 1)
    wg = m.stats().tile_workgroups
    m.close()
    return got, wg


@pytest.mark.parametrize("n2", FIRST_N2)
def test_exit_in_first_cycle(hm, n2):
    """A single pair is cut into segments of one cycle: the sweep of n2 = 64 k - 3 leaves behind tile k - 1."""
    s1, s2, e12, e21 = first_case(n2)
    got, wg = match_pair(hm, s1, _NO_SURF, s2, _NO_SURF)
    assert wg == 2 * ((ntiles_of(n2) + 15) // 16)       # two row blocks, segments of one cycle
    assert np.array_equal(got.matches_1_2, e12), "1->2"
    assert np.array_equal(got.matches_2_1, e21), "2->1"


# --- exits in a later cycle: one segment of 17 .. 33, 48, 49 tiles, forced, in a process of its own ----------------

@pytest.fixture(scope="module")
def later_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("tile_exit") / "later.npz"
    env = dict(os.environ)
    env["OSFM_SEG_TILES"] = str(child.SEG_TILES)
    r = subprocess.run([sys.executable, "-s", child.__file__, str(out)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("k", child.LATER_TILES)
def test_exit_in_later_cycle(later_run, k):
    s1, s2 = child.later_case(k)
    n1, n2 = s1.shape[0], s2.shape[0]
    assert ntiles_of(n2) == k and int(max(s1.max(), s2.max())) <= 127
    e12, e21 = oracle_lib.oracle_pairwise_match(s1, _NO_SURF, s2, _NO_SURF)
    assert_tail_tiles_matched(e12, e21, n1, n2)
    # the long segment was used: one workgroup per row block
    assert int(later_run[f"wg_{k}"]) == (n1 + ROWS - 1) // ROWS
    assert np.array_equal(later_run[f"m12_{k}"], e12), "1->2"
    assert np.array_equal(later_run[f"m21_{k}"], e21), "2->1"


def test_surf_exit_in_later_cycle(later_run):
    """CH = 4 with the exit-free whole cycle in front of the exit: 21 tiles in one forced segment."""
    u1, u2 = child.surf_later_case()
    n1, n2 = u1.shape[0], u2.shape[0]
    assert ntiles_of(n2) == child.SURF_TILES
    e12, e21 = oracle_lib.oracle_pairwise_match(_NO_SIFT, u1, _NO_SIFT, u2)
    assert_tail_tiles_matched(e12, e21, n1, n2)
    assert int(later_run["wg_surf"]) == (n1 + ROWS - 1) // ROWS
    assert np.array_equal(later_run["m12_surf"], e12), "1->2"
    assert np.array_equal(later_run["m21_surf"], e21), "2->1"


def test_fold_17_row_blocks_33_tiles(hm):
    """The finish kernel's fold of the column partials: one batch of sixteen row blocks and one more, over 33 tiles
    (three segments, the last left behind its first tile)."""
    n1, n2 = 16 * ROWS + 104, TILE * 33 - 5
    s1, s2 = match_cases.sift_pair(n1, n2, min(n1, n2), 9300)
    assert int(max(s1.max(), s2.max())) <= 127
    e12, e21 = oracle_lib.oracle_pairwise_match(s1, _NO_SURF, s2, _NO_SURF)
    assert_tail_tiles_matched(e12, e21, n1, n2)
    got, wg = match_pair(hm, s1, _NO_SURF, s2, _NO_SURF)
    assert wg == 17 * 3                                  # 17 row blocks, three segments of one cycle
    assert np.array_equal(got.matches_1_2, e12), "1->2"
    assert np.array_equal(got.matches_2_1, e21), "2->1"


# --- SURF: the CH = 4 instantiation ------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 21])
def test_surf_exit(hm, k):
    n1, n2 = 300, TILE * k - 3
    u1, u2 = match_cases.surf_pair(n1, n2, min(n1, n2), 9100 + k)
    e12, e21 = oracle_lib.oracle_pairwise_match(_NO_SIFT, u1, _NO_SIFT, u2)
    assert_tail_tiles_matched(e12, e21, n1, n2)
    got, wg = match_pair(hm, _NO_SIFT, u1, _NO_SIFT, u2)
    assert wg == 2 * ((k + 15) // 16)
    assert np.array_equal(got.matches_1_2, e12), "1->2"
    assert np.array_equal(got.matches_2_1, e21), "2->1"


# --- one launch with three different exits -------------------------------------------------------------------------

BATCH_N2 = (TILE * 3 - 3, TILE * 7 - 10, TILE * 18 - 31)       # exits behind tiles 2 and 6, and 15 then 1 (two segments)


@functools.lru_cache(maxsize=None)
def batch_case():
    s1, s2 = match_cases.sift_pair(FIRST_N1, max(BATCH_N2), FIRST_N1, 9200)
    assert int(max(s1.max(), s2.max())) <= 127
    cols = [s2[:n] for n in BATCH_N2]               # the shared landmarks lie all over s2
    expect = []
    for c in cols:
        e12, e21 = oracle_lib.oracle_pairwise_match(s1, _NO_SURF, c, _NO_SURF)
        assert_tail_tiles_matched(e12, e21, FIRST_N1, c.shape[0])
        idx = np.nonzero(e12 >= 0)[0]
        expect.append(np.stack([idx, e12[idx]], axis=1).astype(np.int32))
    return s1, cols, expect


def test_batch_mixes_exits(hm):
    from orthosfm_amd import capi
    s1, cols, expect = batch_case()
    o = capi.default_match_options()
    o.use_lowres_matching = 0
    o.min_feature_matches = 0
    m = hm(4, options=o)
    for v, c in enumerate(cols):
        m.set_view(v, c)
    m.set_view(3, s1)
    out = m.compute([(3, 0), (3, 1), (3, 2)])
    st = m.stats()
    m.close()
    assert st.tile_kernel_launches == 1
    assert st.tile_workgroups == 2 * sum((ntiles_of(n) + 15) // 16 for n in BATCH_N2)
    for tv, e in zip(out, expect):
        assert tv.status == capi.PAIR_MATCHED and np.array_equal(tv.matches, e), (tv.view_1_id, tv.view_2_id)


def test_repeatable(hm):
    """The same call twice: identical bytes (the stores that overwrite the throw-away merge are ordered)."""
    s1, s2, e12, e21 = first_case(TILE * 3 - 3)
    m = hm(2)
    m.set_view(0, s1)
    m.set_view(1, s2)
    a = m.pairwise_match(0, 1)
    b = m.pairwise_match(0, 1)
    m.close()
    assert a.matches_1_2.tobytes() == b.matches_1_2.tobytes() == e12.tobytes()
    assert a.matches_2_1.tobytes() == b.matches_2_1.tobytes() == e21.tobytes()
