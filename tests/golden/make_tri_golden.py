"""Writes tests/golden/tri_reference.npz: per case and camera model of tests/tri_cases.py the triangulated points of the
mpmath reference (tri_cases.reference, 200 bits) as float64, the bound A_j, the eigenvalue ratios of R, the valid mask
and the SHA-256 of the inputs the case was built from.  Needs mpmath; about 10 s.

    python tests/golden/make_tri_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tri_cases as tc  # noqa: E402


def main():
    out = {}
    for name, model in tc.ALL:
        sc = tc.build(name, model)
        ref = tc.reference(sc)
        k = tc.key(name, model)
        for f in ("points", "A", "ratios", "valid"):
            out[f"{k}/{f}"] = ref[f]
        out[f"{k}/sha256"] = np.array(tc.input_hash(sc))
        v = ref["valid"].astype(bool)
        print(f"{k:28s} tracks {v.size:4d} valid {int(v.sum()):4d}  smallest retained ratio "
              f"{min((r[r > tc.BAND_LO].min() for r in ref['ratios'][v]), default=0.0):.2e}  largest A {ref['A'].max():.2e}")
    np.savez_compressed(tc.GOLDEN, **out)
    print(tc.GOLDEN, os.path.getsize(tc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
