"""Writes tests/golden/affine_reference.npz: per case of tests/affine_cases.py the SHA-256 of its inputs and the results
of the exact / 200-bit reference (affine_cases.reference): per iteration (single-hypothesis scenes: per pair id)
count_ref, amb and the unconstrained flag; the winner iteration with its vector, kappa and the bitmasks of its clear
inliers and of its band; where the refit runs, its vector, condition, eigenvalues, masks and whether it is accepted.
Needs mpmath; a few minutes on 8 cores.  It also prints the restatement's ratio over every constrained hypothesis and
every refit of every case, from which affine_cases.TAU and TAU_R are set; the stored masks depend on them, so run it
again after changing either (--cache FILE keeps the hypotheses, which do not depend on them, between runs).

    python tests/golden/make_affine_golden.py [--cache FILE]
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

import affine_cases as ac  # noqa: E402
import affine_restatement as ar  # noqa: E402


def restatement_ratios(case, pair, hyps):
    """Per hypothesis the ratio max |v -+ v_ref| / (2^-53 kappa) of the restatement (0 where unconstrained)."""
    valid, vs = ar.hypotheses(case.pos1, case.pos2, case.corr, len(hyps), case.seed, pair)
    r = np.zeros(len(hyps))
    for it, h in enumerate(hyps):
        if not h["uncon"]:
            r[it] = ac.ratio(ar.layout(vs[it]), h["v"], h["kappa"]) if valid[it] else np.inf
    return r


def main():
    out = {}
    cache = sys.argv[sys.argv.index("--cache") + 1] if "--cache" in sys.argv else None
    if cache and os.path.exists(cache):
        with open(cache, "rb") as f:
            ac._hyp_cache.update(pickle.load(f))
    worst, worst_r = 0.0, 0.0
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in ac.ALL:
            case = ac.build(name)
            if case.kind == "twin":
                out[f"{name}/sha256"] = np.array(ac.input_hash(case))
                print(f"{name:18s} held to the restatement")
                continue
            ref = ac.reference(case, pool)
            for f, v in ref.items():
                out[f"{name}/{f}"] = v
            # diagnostics, not stored: conditioning, and the restatement against the reference on EVERY hypothesis
            ok = ref["uncon"] == 0
            if case.kind == "single":
                hyps = [ac.hypotheses(case, p, 1)[0] for p in case.pairs]
                tw = np.array([restatement_ratios(case, p, [h])[0] for p, h in zip(case.pairs, hyps)])
            else:
                hyps = ac.hypotheses(case, case.pairs[0], case.max_iterations)
                tw = restatement_ratios(case, case.pairs[0], hyps)
            kappa = np.array([h["kappa"] for h in hyps])[ok]
            worst = max(worst, float(tw.max()))
            line = (f"{name:18s} k {case.k:5d} hyps {ok.size:5d} unconstrained {int((~ok).sum()):3d}  kappa {kappa.min():.1e}.."
                    f"{kappa.max():.1e}  best {int(ref['count_ref'].max()):5d}  amb {int(ref['amb'].sum())}  ratio {tw.max():.4f} "
                    f"(at kappa {kappa[np.argmax(tw[ok])]:.1e})")
            if case.kind != "single" and ref["refit_ran"]:
                m1, m2 = case.matches()
                vr = ar.refit_vector(m1, m2, ac.mask(ref["clear"], case.k))
                rr = ac.ratio(ar.layout(vr), ref["refit_v"], float(ref["refit_cond"]))
                worst_r = max(worst_r, rr)
                line += (f"  refit count {int(ref['refit_count'])} amb {int(ref['refit_amb'])} accepted {int(ref['refit_accepted'])} "
                         f"cond {float(ref['refit_cond']):.1e} ratio {rr:.4f}")
            print(line, flush=True)
    print(f"largest ratio {worst:.4f}, largest refit ratio {worst_r:.4f}")
    if cache:
        with open(cache, "wb") as f:
            pickle.dump(ac._hyp_cache, f)
    # an .npz whose bytes depend on its arrays alone: fixed entry order and time stamps
    with zipfile.ZipFile(ac.GOLDEN, "w") as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(ac.GOLDEN, os.path.getsize(ac.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
