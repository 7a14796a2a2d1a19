"""Helper of test_match_tile_exit_gpu.py: the cases whose column segment is longer than one 16-tile cycle.

The segment length of the correction-free tile kernel is chosen by the planner; OSFM_SEG_TILES forces it and is
read once per process, so these cases run in a process of their own:

    OSFM_SEG_TILES=64 python match_tile_exit_child.py out.npz

matches every case of later_cases() with pairwise_match and writes the lists and the number of tile workgroups
each call launched (one per row block when the whole of n2 is one segment).  The comparison with the oracle is
the test's.  Imported, it only provides the inputs."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import match_cases  # noqa: E402

TILE = 64
SEG_TILES = 64                       # four cycles: every case below is one segment
LATER_N1 = 2100                      # nine row blocks, the last one of 52 rows
LATER_TILES = tuple(range(17, 34)) + (48, 49)


@functools.lru_cache(maxsize=None)
def _later_pair():
    n2 = TILE * max(LATER_TILES) - 5
    s1, s2 = match_cases.sift_pair(LATER_N1, n2, LATER_N1, 8800)
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


def later_case(k):
    """k tiles, the last one five columns short: the first 64 k - 5 columns of one pair of sets."""
    s1, s2 = _later_pair()
    return s1, s2[:TILE * k - 5]


SURF_TILES = 21                      # CH = 4: one whole cycle, then an exit behind the fifth tile of the next
SURF_N1 = 300


@functools.lru_cache(maxsize=None)
def surf_later_case():
    u1, u2 = match_cases.surf_pair(SURF_N1, TILE * SURF_TILES - 5, SURF_N1, 8900)
    u1.setflags(write=False)
    u2.setflags(write=False)
    return u1, u2


def main(out_path):
    assert os.environ.get("OSFM_SEG_TILES") == str(SEG_TILES)
    from orthosfm_amd.matching import HipExhaustiveMatching
    out = {}
    m = HipExhaustiveMatching(2)
    for k in LATER_TILES:
        s1, s2 = later_case(k)
        m.set_view(0, s1)
        m.set_view(1, s2)
        got = m.pairwise_match(0, 1)
        out[f"m12_{k}"] = got.matches_1_2
        out[f"m21_{k}"] = got.matches_2_1
        out[f"wg_{k}"] = np.int64(m.stats().tile_workgroups)
    m.close()
    u1, u2 = surf_later_case()
    none = np.zeros((0, 128), np.uint16)
    m = HipExhaustiveMatching(2)
    m.set_view(0, none, u1)
    m.set_view(1, none, u2)
    got = m.pairwise_match(0, 1)
    out["m12_surf"], out["m21_surf"] = got.matches_1_2, got.matches_2_1
    out["wg_surf"] = np.int64(m.stats().tile_workgroups)
    m.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
