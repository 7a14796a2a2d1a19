"""Writes tests/golden/ransac_reference.npz: per case of tests/ransac_cases.py the SHA-256 of its inputs and the results
of the exact / 200-bit reference (ransac_cases.reference): per iteration (single-hypothesis scenes: per pair id)
count_ref, amb, the unconstrained flag, kappa and the rank-2 gap; the winner iteration with its F_ref, A and the
bitmasks of its clear inliers and of its band (single-hypothesis scenes: all of these per pair id).  For `twins` the
counts of the unconstrained iterations are taken from the twin and `twins/uncon_below_best` records that they lie below
the best constrained count.  Needs mpmath and oracle/liboracle.so; about two minutes on 8 cores.  It also prints the
twin's F ratio over every hypothesis of every case, from which ransac_cases.TAU is set; the stored count_ref and amb
depend on TAU, so run it again after changing TAU (--cache FILE keeps the TAU-independent hypotheses between runs).

    python tests/golden/make_ransac_golden.py [--cache FILE]
"""
import io
import multiprocessing
import os
import pickle
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ransac_cases as rc  # noqa: E402


def main():
    out = {}
    cache = sys.argv[sys.argv.index("--cache") + 1] if "--cache" in sys.argv else None
    if cache and os.path.exists(cache):
        with open(cache, "rb") as f:
            rc._hyp_cache.update(pickle.load(f))
    worst = 0.0
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in rc.ALL:
            case = rc.build(name)
            if case.kind == "twin":
                out[f"{name}/sha256"] = np.array(rc.input_hash(case))
                print(f"{name:18s} held to the twin")
                continue
            ref = rc.reference(case, pool)
            if name == "twins":
                _, counts, _ = rc.twin_run(case, case.pairs[0])
                un = ref["uncon"].astype(bool)
                best = int(ref["count_ref"][~un].max())
                ref["twin_uncon_max"] = np.array(int(counts[un].max()) if un.any() else -1, np.int32)
                ref["uncon_below_best"] = np.array(int(ref["twin_uncon_max"]) < best, np.uint8)
            for f, v in ref.items():
                out[f"{name}/{f}"] = v
            # diagnostics, not stored: conditioning, and the twin's F against the reference on EVERY hypothesis
            ok = ref["uncon"] == 0
            if case.kind == "single":
                hyps = [rc.hypotheses(case, p, 1)[0] for p in case.pairs]
                tw = np.array([rc.twin_ratios(case, p, [h])[0] for p, h in zip(case.pairs, hyps)])
            else:
                hyps = rc.hypotheses(case, case.pairs[0], case.max_iterations)
                tw = rc.twin_ratios(case, case.pairs[0], hyps)
            kappa, gap = np.array([h["kappa"] for h in hyps])[ok], np.array([h["gap"] for h in hyps])[ok]
            worst = max(worst, float(tw.max()))
            print(f"{name:18s} k {case.k:5d} hyps {ok.size:5d} unconstrained {int((~ok).sum()):3d}  kappa "
                  f"{kappa.min():.1e}..{kappa.max():.1e}  smallest gap {gap.min():.1e}  best {int(ref['count_ref'].max()):5d}  "
                  f"amb {int(ref['amb'].sum())}  twin ratio {tw.max():.4f} (at kappa {kappa[np.argmax(tw[ok])]:.1e})", flush=True)
    print(f"largest twin ratio {worst:.4f}")
    if cache:
        with open(cache, "wb") as f:
            pickle.dump(rc._hyp_cache, f)
    # an .npz whose bytes depend on its arrays alone: fixed entry order and time stamps
    with zipfile.ZipFile(rc.GOLDEN, "w") as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(rc.GOLDEN, os.path.getsize(rc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
