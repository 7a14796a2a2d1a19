"""Cases, reference, bounds and check of the affine geometric verification (ransac_affine_kernel in
orthosfm_amd/csrc/ransac_affine.hip, reached through osfm_ransac_affine).

The reference is written from the mathematics of the mode, not from the kernel or from tests/affine_restatement.py,
which is the kernel's operation-for-operation twin.  Only the sample stream is the library's (splitmix64 / ransac_rand of
ransac_cases.py): the first 4 distinct draws mod k, ascending.  Per iteration:
  null vector   of the 4 x 5 system with rows (x2, y2, x1, y1, 1), EXACTLY: float32 inputs are rationals and the
                elimination runs in fractions.Fraction.  An exact rank below 4 makes the iteration *unconstrained*.
                The vector is brought to a^2 + b^2 + c^2 + d^2 = 1 with mpmath at 200 bits.
  kappa         sigma_1 / sigma_4 of the 4 x 5 system (mpmath).
  distances     |n| = |a x2 + b y2 + c x1 + d y1 + e| against thr sqrt(a^2 + b^2 + c^2 + d^2) in float64 numpy under the
                reference vector rounded to float64, with a band (below): count_ref = matches clearly inside, amb =
                matches in the band.
The reference winner is the first constrained iteration that reaches the largest count_ref.
  refit         when the winner has >= 5 inliers: the mean and the 4 x 4 scatter of z = (x2, y2, x1, y1) over the
                reference's inlier set in Fractions, EXACTLY; its eigenvalues l1 <= l2 <= l3 <= l4 and the eigenvector
                of l1 at 200 bits, e = -(a, b, c, d) . mean; cond = l4 / (l2 - l1).  Its matches are classified like a
                hypothesis's; it is accepted when it has at least the winner's count.

Bounds, up to sign, on the vector (a, b, c, d, e) at a^2 + b^2 + c^2 + d^2 = 1:
  hypothesis    max |v -+ v_ref| <= TAU 2^-53 kappa: the null vector of a full-rank 4 x 5 system moves by kappa times a
                relative perturbation of the system.  kappa is 1e1 .. 1e4 on the benign scene and grows like 1 / relief
                near a plane, where the system's rank falls to 3 (two orthographic views of a plane are related by an
                affine map, so x2 and y2 are combinations of x1, y1, 1).
  refit         max |v -+ v_ref| <= TAU_R 2^-53 cond: the eigenvector turns by |dC| / (l2 - l1) and the float64 scatter is
                off by a few 2^-53 l4.

Band.  A match is an inlier when |n| < thr rs, rs = sqrt(a^2 + b^2 + c^2 + d^2).  For v' = v + dv, max |dv| <= eps_v:
|dn| <= eps_v c1 with c1 = |x2| + |y2| + |x1| + |y1| + 1, and |d rs| <= 2 eps_v (four components).  The float64
evaluations of both sides add at most FL 2^-53 c1 max(1, |e|) to n (9 operations on either side and the rounding of the
reference to float64: 19, 32 taken) and FL 2^-53 to rs.  So the decision can differ only where
    | |n| / (thr rs) - 1 | <= beta,  beta = (c1 (B + FL max(1, |e|)) + thr (2 B + FL)) 2^-53 / (thr rs),
B = TAU kappa for a hypothesis and TAU_R cond for a refit.  A match with beta >= 1 is ambiguous.

TAU and TAU_R.  tests/golden/make_affine_golden.py measures the restatement's ratio on every constrained hypothesis and
on every refit of every case (CPU); each constant is the next power of two above four times the largest ratio.  The
kernel is the restatement bit for bit, so no GPU measurement enters.  test_affine_cases_cpu.py repeats the measurement
on the winners and the single-hypothesis scenes.

Inputs are those of ransac_cases.py's generators (two orthographic views of points in the unit cube; float32 positions,
every step a float64 +, * written out: the same bits on any machine) and a few of their own; the SHA-256 of each case is
in the golden (tests/golden/affine_reference.npz) and asserted by load().

Cases (threshold 0.0015; the match counts and iteration counts follow the kernel's constants, read from its headers):
  single hypotheses (max_iterations 1, refit off, pair ids 0..63, 400 matches): the inputs of ransac_cases.SINGLE
    benign, near_planar_1e-2, near_planar_1e-4, scale_1e-4, edge_1
  path shapes (refit on)
    k_4 .. k_2049       K_LIST matches, 1000 iterations, 30 % outliers: 4 and 5 (k_4: one sample, 4 inliers, no refit),
                        around the wave (64), the workgroup (256) and the LDS chunk with its four-at-a-time loop
                        (chunk - 1, chunk, chunk + 1, chunk + 3), two chunks and one
    iters_1 .. iters_1025
                        700 matches, ITER_LIST iterations: 1, 2; one pass of a workgroup (256 x hypotheses per thread)
                        - 1 / exact / + 1, which leave the second part none, none, one hypothesis; 1000 (many); two
                        passes exact and + 1 (a second pass of part 0 beside one hypothesis of part 1)
    tie_part1, tie_both, tie_thread, tie_slot
                        150 matches, noise 6e-4; the largest count is reached in part 1 only / in both parts, first in part 0 /
                        by two threads of one pass, first by the higher thread / by the two hypotheses of one thread.
                        The tied iterations have different vectors
  refit
    refit_larger        noise 1e-3 on 600 matches, 32 iterations: the refit holds more matches than the winner
    refit_equal         no noise: winner and refit hold every true match
    refit_rejected      constructed: 90 matches exactly on a hyperplane, 110 spread to 0.9 thr about it, 30 in a
                        cluster at one end, all 0.9 thr to one side.  A sample among the 90 holds all 230; the least-
                        squares fit is pulled towards the cluster and loses matches at the far side
    refit_off           refit_larger's inputs with refit = 0
    (skipped for fewer than 5 inliers: k_4)
  at_threshold          one hypothesis whose threshold t has t * t == n^2 / s of one match in the kernel's arithmetic:
                        < leaves it out, <= would take it.  Such a match lies in every band; held to the restatement
  degenerate (held to the restatement and to stated properties)
    identical_views     600 matches on a 2^-10 grid, pos2 = pos1
    one_point           20 matches at one position: every sample is refused; count 0, F zero, empty list
    twins               1200 matches, 30 % of them copies of another match
"""
import hashlib
import os
import re
from fractions import Fraction

import numpy as np

import ransac_cases as rc
from ransac_cases import ransac_rand, splitmix64  # noqa: F401  (the library's sample stream)

U = 2.0 ** -53
# The restatement's largest ratios as make_affine_golden.py prints them (CPU), over every constrained hypothesis and
# every refit of every case; TAU / TAU_R: the next power of two above four times each.
MEASURED_RATIO = 0.3668              # on refit_rejected at kappa 4; 0.08 at kappa 6e5 (near_planar_1e-4): flat in kappa
MEASURED_RATIO_R = 0.5149            # the refit of k_257
TAU = 2.0
TAU_R = 4.0
THR = 0.0015
BITS = 200
FL_ROUNDINGS = 32.0
REFIT_MIN = 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affine_reference.npz")
_ST = 0xAF1 << 32                    # streams of synth's counter-based generator used by this file's own scenes


def _constant(header, name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "orthosfm_amd", "csrc", header)
    return int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)", open(path).read()).group(1))


WAVE, GROUP = 64, 256
HYP = _constant("ransac_affine.h", "kAffineHyp")
CHUNK = _constant("ransac_affine.h", "kAffineChunk")
SPLIT = _constant("ransac_kernels.h", "kRansacSplit")
PASS = GROUP * HYP

K_LIST = (4, 5, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 3, 2 * CHUNK + 1)
ITER_LIST = (1, 2, PASS - 1, PASS, PASS + 1, 1000, SPLIT * PASS, SPLIT * PASS + 1)
SINGLE = rc.SINGLE
PAIRS = rc.PAIRS
# (seed, pair id) of the tie cases, found with the restatement on the CPU and confirmed from count_ref
TIES = {"tie_part1": (1, 27), "tie_both": (1, 7), "tie_thread": (3, 77), "tie_slot": (12, 24)}
REFIT = ("refit_larger", "refit_equal", "refit_rejected", "refit_off")
# at_threshold: (seed, pair id, match, threshold as float.hex), found on the CPU with the restatement
AT_THRESHOLD = (11, 0, 122, "0x1.402d321a0b680p-10")
AT_THRESHOLD_COUNT = 299             # inliers of at_threshold; 300 matches have n^2 / s <= thr^2


class Case(rc.Case):
    def __init__(self, *a, refit=True, **kw):
        super().__init__(*a, **kw)
        self.refit = bool(refit)


def sample4(seed, pair, it, k):
    """4 distinct match ids in [0, k), ascending."""
    got, d = [], 0
    while len(got) < 4:
        v = ransac_rand(seed, pair, it, d) % k
        d += 1
        if v not in got:
            got.append(v)
    return sorted(got)


def part_of(it, max_iterations):
    """(part, pass, thread, slot) of an iteration in the kernel's split over SPLIT workgroups in passes of HYP x 256."""
    per_part = ((max_iterations + SPLIT - 1) // SPLIT + PASS - 1) // PASS * PASS
    r = it % per_part
    return it // per_part, r // PASS, r % GROUP, (r % PASS) // GROUP


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _from(case, kind, name=None, **kw):
    return Case(name or case.name, kind, case.pos1, case.pos2, case.corr, **kw)


def _k_case(k):
    stream = 0x1000 + 0x10 * K_LIST.index(k)
    return Case(f"k_{k}", "full", *rc._scatter(*rc._views(k, 0.3, stream), stream), pairs=(k,))


def _iters_case(n):
    return Case(f"iters_{n}", "full", *rc._scatter(*rc._views(700, 0.3, 0x2000), 0x2000), max_iterations=n, pairs=(5,))


def _tie_case(name):
    seed, pair = TIES[name]
    return Case(name, "full", *rc._scatter(*rc._views(150, 0.3, 0x3000, noise=6e-4), 0x3000), seed=seed, pairs=(pair,))


def _refit_rejected():
    """Matches about the hyperplane H: a x2 + b y2 + c x1 + d y1 + e = 0 (unit (a, b, c, d)); a residual r moves y2 by
    r / b, which is a Sampson distance of r^2."""
    from orthosfm_amd import synth
    a, b, c, d, e = 0.5, 0.5, -0.5, 0.5, 0.0625
    n_on, n_spread, n_cluster, n_out = 90, 110, 30, 70
    n = n_on + n_spread + n_cluster + n_out
    u = synth.uniform(rc.SEED, _ST | 0x100, 4 * n).reshape(n, 4)
    x1, y1, x2 = u[:, 0] - 0.5, u[:, 1] - 0.5, u[:, 2] - 0.5
    lo, hi = n_on + n_spread, n_on + n_spread + n_cluster
    # the cluster sits at one end of the x1 axis
    x1[lo:hi] = 0.45 + 0.05 * u[lo:hi, 0]
    r = np.zeros(n)
    r[n_on:lo] = (2.0 * u[n_on:lo, 3] - 1.0) * 0.9 * THR
    r[lo:hi] = 0.9 * THR
    y2 = -((a * x2 + c * x1) + (d * y1 + e)) / b + r / b
    y2[hi:] = u[hi:, 3] - 0.5
    p1, p2 = rc._f32(np.stack([x1, y1], axis=1)), rc._f32(np.stack([x2, y2], axis=1))
    order = rc._order(0x8100, n)
    return Case("refit_rejected", "full", *rc._scatter(p1[order], p2[order], 0x8100), pairs=(6,))


def _refit_case(name):
    if name == "refit_rejected":
        return _refit_rejected()
    if name == "refit_equal":
        return Case(name, "full", *rc._scatter(*rc._views(600, 0.3, 0x8200, noise=0.0), 0x8200), pairs=(7,))
    p1, p2 = rc._views(600, 0.3, 0x8300, noise=1e-3)
    return Case(name, "full", *rc._scatter(p1, p2, 0x8300), max_iterations=32, pairs=(8,), refit=name != "refit_off")


def _at_threshold():
    seed, pair, _, thr = AT_THRESHOLD
    return Case("at_threshold", "twin", *rc._scatter(*rc._views(400, 0.25, 0x5000), 0x5000), max_iterations=1,
                threshold=float.fromhex(thr), seed=seed, pairs=(pair,), refit=False)


FULL = tuple(f"k_{k}" for k in K_LIST) + tuple(f"iters_{n}" for n in ITER_LIST) + tuple(TIES) + REFIT
TWIN_ONLY = ("at_threshold", "identical_views", "one_point", "twins")
ALL = SINGLE + FULL + TWIN_ONLY


def build(name):
    if name in SINGLE:
        return _from(rc.build(name), "single", max_iterations=1, pairs=PAIRS, refit=False)
    if name.startswith("k_"):
        return _k_case(int(name[2:]))
    if name.startswith("iters_"):
        return _iters_case(int(name[6:]))
    if name in TIES:
        return _tie_case(name)
    if name in REFIT:
        return _refit_case(name)
    if name == "at_threshold":
        return _at_threshold()
    src = rc.build(name)
    return _from(src, "twin", pairs=src.pairs)


def input_hash(case):
    h = hashlib.sha256()
    h.update(np.array([case.k, case.max_iterations, case.seed, int(case.refit), *case.pairs], dtype=np.int64).tobytes())
    h.update(np.array([case.threshold], dtype=np.float64).tobytes())
    for a in (case.pos1, case.pos2, case.corr):
        h.update(np.array(a.shape, dtype=np.int64).tobytes())
        h.update(a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------

def system(m1, m2):
    """The 4 x 5 system of a sample: rows (x2, y2, x1, y1, 1)."""
    return np.stack([m2[:, 0], m2[:, 1], m1[:, 0], m1[:, 1], np.ones(m1.shape[0])], axis=1)


def exact_null_vector(A):
    """The null vector (Fractions) of a full-rank r x (r + 1) float64 matrix, or None when its exact rank is below r."""
    M = [[Fraction(float(v)) for v in row] for row in A]
    rows, cols = len(M), len(M[0])
    piv, r = [], 0
    for c in range(cols):
        if r == rows:
            break
        p = next((i for i in range(r, rows) if M[i][c] != 0), None)
        if p is None:
            continue
        M[r], M[p] = M[p], M[r]
        inv = 1 / M[r][c]
        M[r] = [v * inv for v in M[r]]
        for i in range(rows):
            if i != r and M[i][c] != 0:
                f = M[i][c]
                M[i] = [x - f * y for x, y in zip(M[i], M[r])]
        piv.append(c)
        r += 1
    if r < rows:
        return None
    free = next(c for c in range(cols) if c not in piv)
    f = [Fraction(0)] * cols
    f[free] = Fraction(1)
    for i, c in enumerate(piv):
        f[c] = -M[i][free]
    return f


def hypothesis(m1, m2, bits=BITS):
    """The reference's vector of one sample: dict(uncon, v (5,) float64 at a^2 + b^2 + c^2 + d^2 = 1, kappa)."""
    import mpmath as mp
    A = system(m1, m2)
    f = exact_null_vector(A)
    res = {"uncon": 1, "v": np.zeros(5), "kappa": 0.0}
    if f is None or not any(f[:4]):
        return res
    with mp.workprec(bits):
        fm = [mp.mpf(x.numerator) / mp.mpf(x.denominator) for x in f]
        n = mp.sqrt(sum(x * x for x in fm[:4]))
        sv = mp.svd_r(mp.matrix(A.tolist()), compute_uv=False)
        sv = sorted((sv[i] for i in range(4)), reverse=True)
        res.update(uncon=0, v=np.array([float(x / n) for x in fm]), kappa=float(sv[0] / sv[3]))
    return res


def _hyp_job(args):
    return hypothesis(*args)


def refit_reference(m1, m2, inl, bits=BITS):
    """The least-squares vector of the matches of mask inl: dict(v (5,), cond, lam (4,))."""
    import mpmath as mp
    z = [[Fraction(float(m2[i, 0])), Fraction(float(m2[i, 1])), Fraction(float(m1[i, 0])), Fraction(float(m1[i, 1]))]
         for i in np.nonzero(inl)[0]]
    n = len(z)
    mu = [sum(r[q] for r in z) / n for q in range(4)]
    C = [[sum((r[p] - mu[p]) * (r[q] - mu[q]) for r in z) for q in range(4)] for p in range(4)]
    with mp.workprec(bits):
        toM = lambda x: mp.mpf(x.numerator) / mp.mpf(x.denominator)
        lam, vec = mp.eigsy(mp.matrix([[toM(x) for x in row] for row in C]))
        order = sorted(range(4), key=lambda i: lam[i])
        l = [lam[i] for i in order]
        v = [vec[q, order[0]] for q in range(4)]
        nn = mp.sqrt(sum(x * x for x in v))
        v = [x / nn for x in v]
        e = -sum(x * toM(m) for x, m in zip(v, mu))
        gap = l[1] - l[0]
        cond = float(l[3] / gap) if gap > 0 else float("inf")
        return {"v": np.array([float(x) for x in v] + [float(e)]), "cond": cond, "lam": np.array([float(x) for x in l])}


def classify(v, B, m1, m2, thr):
    """(clear inliers, ambiguous) masks of the matches under the reference vector v with bound B 2^-53 on it."""
    a, b, c, d, e = (float(x) for x in v)
    x1, y1, x2, y2 = m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]
    n = np.abs(a * x2 + b * y2 + c * x1 + d * y1 + e)
    rs = np.sqrt(a * a + b * b + c * c + d * d)
    c1 = np.abs(x2) + np.abs(y2) + np.abs(x1) + np.abs(y1) + 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = (c1 * (B + FL_ROUNDINGS * max(1.0, abs(e))) + thr * (2.0 * B + FL_ROUNDINGS)) * U / (thr * rs)
        beta = np.where(np.isfinite(beta), beta, np.inf)
        r = n / (thr * rs)
    sure = beta < 1.0
    clear_in = sure & (r < 1.0 - beta)
    clear_out = sure & (r > 1.0 + beta)
    return clear_in, ~(clear_in | clear_out)


_hyp_cache = {}


def hypotheses(case, pair, n_iter, pool=None):
    """The reference hypotheses of iterations 0..n_iter-1 of a pair (cached per input arrays and sample)."""
    h = hashlib.sha256()
    for a in (case.pos1, case.pos2, case.corr):
        h.update(a.tobytes())
    have = _hyp_cache.setdefault(h.hexdigest(), {})
    samples = [tuple(sample4(case.seed, pair, it, case.k)) for it in range(n_iter)]
    new = sorted(set(samples) - set(have))
    if new:
        m1, m2 = case.matches()
        jobs = [(m1[list(idx)], m2[list(idx)]) for idx in new]
        have.update(zip(new, pool.map(_hyp_job, jobs, chunksize=8) if pool is not None else map(_hyp_job, jobs)))
    return [have[idx] for idx in samples]


def reference(case, pool=None, tau=None, tau_r=None):
    """The golden arrays of a case (a dict of numpy arrays)."""
    tau = TAU if tau is None else tau
    tau_r = TAU_R if tau_r is None else tau_r
    m1, m2 = case.matches()
    k = case.k
    out = {"sha256": np.array(input_hash(case))}
    if case.kind == "single":
        hyps = [hypotheses(case, p, 1, pool)[0] for p in case.pairs]
    else:
        hyps = hypotheses(case, case.pairs[0], case.max_iterations, pool)
    n = len(hyps)
    count, amb = np.zeros(n, np.int16), np.zeros(n, np.int16)
    clear, ambm = np.zeros((n, k), bool), np.zeros((n, k), bool)
    for i, h in enumerate(hyps):
        if not h["uncon"]:
            clear[i], ambm[i] = classify(h["v"], tau * h["kappa"], m1, m2, case.threshold)
            count[i], amb[i] = clear[i].sum(), ambm[i].sum()
    out["count_ref"], out["amb"] = count, amb
    out["uncon"] = np.array([h["uncon"] for h in hyps], np.uint8)
    if case.kind == "single":
        out["kappa"] = np.array([h["kappa"] for h in hyps])
        out["v"] = np.stack([h["v"] for h in hyps])
        out["clear"], out["ambm"] = np.packbits(clear, axis=1), np.packbits(ambm, axis=1)
        return out
    ok = out["uncon"] == 0
    w = int(np.argmax(np.where(ok, count, -1)))
    out["winner"] = np.array(w, np.int32)
    out["v"], out["kappa"] = hyps[w]["v"], np.array(hyps[w]["kappa"])
    out["clear"], out["ambm"] = np.packbits(clear[w]), np.packbits(ambm[w])
    ran = bool(case.refit and count[w] >= REFIT_MIN and not ambm[w].any())
    out["refit_ran"] = np.array(int(ran), np.uint8)
    if ran:
        rr = refit_reference(m1, m2, clear[w])
        rc_, ra_ = classify(rr["v"], tau_r * rr["cond"], m1, m2, case.threshold)
        out["refit_v"], out["refit_cond"], out["refit_lam"] = rr["v"], np.array(rr["cond"]), rr["lam"]
        out["refit_clear"], out["refit_ambm"] = np.packbits(rc_), np.packbits(ra_)
        out["refit_count"], out["refit_amb"] = np.array(int(rc_.sum()), np.int32), np.array(int(ra_.sum()), np.int32)
        out["refit_accepted"] = np.array(int(rc_.sum() >= count[w]), np.uint8)
    return out


# ---------------------------------------------------------------------------
# golden and check
# ---------------------------------------------------------------------------
_golden = None
_cases = {}


def golden(name):
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    g = {k[len(name) + 1:]: v for k, v in _golden.items() if k.startswith(name + "/")}
    for v in g.values():
        v.setflags(write=False)
    return g


def load(name):
    """(case, golden) of a case; the case is rebuilt and must hash to what the golden was made from."""
    if name not in _cases:
        case, g = build(name), golden(name)
        assert input_hash(case) == str(g["sha256"]), f"{name}: inputs differ from those of tests/golden/affine_reference.npz"
        _cases[name] = (case, g)
    return _cases[name]


def mask(bits, k):
    return np.unpackbits(bits, axis=-1)[..., :k].astype(bool)


def vector(F):
    """(a, b, c, d, e) of an F in the layout of sampson()."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    return F[[2, 5, 6, 7, 8]]


def ratio(F, v_ref, B):
    """max |v -+ v_ref| / (2^-53 B) at a^2 + b^2 + c^2 + d^2 = 1, the smaller of both signs; inf when F has no such
    vector (not finite, zero, or an entry outside the affine layout)."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    v = vector(F)
    nrm = np.sqrt((v[:4] * v[:4]).sum())
    if not np.isfinite(nrm) or nrm == 0.0 or not np.isfinite(v[4]) or F[[0, 1, 3, 4]].any():
        return np.inf
    v = v / nrm
    return float(min(np.abs(v - v_ref).max(), np.abs(v + v_ref).max()) / (U * B))


def check_list(inliers, clear, amb):
    """True when the inlier list holds every clear inlier and nothing but clear inliers and ambiguous matches."""
    got = np.zeros(clear.size, bool)
    got[np.asarray(inliers, dtype=np.int64)] = True
    return bool((got[clear].all()) and not (got & ~clear & ~amb).any())


def check(name, results, tau=None, tau_r=None):
    """What an implementation's results miss of a SINGLE or FULL case's golden: (findings -- empty when it passes --, the
    largest hypothesis ratio, the largest refit ratio).  results: one (count, inlier ids, F, record) per pair id."""
    tau = TAU if tau is None else tau
    tau_r = TAU_R if tau_r is None else tau_r
    case, g = load(name)
    bad, worst, worst_r = [], 0.0, 0.0
    assert len(results) == len(case.pairs)
    for j, (n, inl, F, rec) in enumerate(results):
        single = case.kind == "single"
        what = f"{name} pair {case.pairs[j]}"
        if single and g["uncon"][j]:
            continue
        if n != len(inl):
            bad.append(f"{what}: count {n} but {len(inl)} ids")
        if single:
            v_ref, B, clear, amb = g["v"][j], tau * float(g["kappa"][j]), mask(g["clear"][j], case.k), mask(g["ambm"][j], case.k)
        else:
            w, best = int(g["winner"]), int(g["count_ref"][g["winner"]])
            if best == 0:
                if n != 0 or np.any(np.asarray(F) != 0) or rec["best_iteration"] != -1:
                    bad.append(f"{what}: no inlier under the reference, got {n}")
                continue
            if (rec["best_iteration"], rec["ransac_inliers"]) != (w, best):
                bad.append(f"{what}: winner {rec['best_iteration']} with {rec['ransac_inliers']}, reference {w} with {best}")
            if rec["refit_ran"] != int(g["refit_ran"]):
                bad.append(f"{what}: refit ran {rec['refit_ran']}, reference {int(g['refit_ran'])}")
            accepted = bool(g["refit_ran"]) and bool(g["refit_accepted"])
            if rec["refit_accepted"] != int(accepted):
                bad.append(f"{what}: refit accepted {rec['refit_accepted']}, reference {int(accepted)}")
            # (a rejected refit is not in the result: its count lies below the winner's; the CPU test holds its vector)
            if accepted:
                v_ref, B = g["refit_v"], tau_r * float(g["refit_cond"])
                clear, amb = mask(g["refit_clear"], case.k), mask(g["refit_ambm"], case.k)
            else:
                v_ref, B, clear, amb = g["v"], tau * float(g["kappa"]), mask(g["clear"], case.k), mask(g["ambm"], case.k)
        lim = tau_r if not single and accepted else tau
        r = ratio(F, v_ref, B / lim)                   # in units of 2^-53 x the condition; the bound is lim
        if not single and accepted:
            worst_r = max(worst_r, r)
        else:
            worst = max(worst, r)
        if not r <= lim:
            bad.append(f"{what}: the vector is {r:.3g} x 2^-53 x its condition {B / lim:.2e} from the reference (bound {lim})")
        if not (np.all(np.diff(inl) > 0) and check_list(inl, clear, amb)):
            bad.append(f"{what}: inlier list differs from the reference's ({len(inl)} ids, {int(clear.sum())} clear, {int(amb.sum())} in the band)")
    return bad, worst, worst_r


# ---------------------------------------------------------------------------
# quality: planted inliers found, against the 8-point twin
# ---------------------------------------------------------------------------
QUALITY_MATCHES = 600
QUALITY_SHARES = (0.5, 0.65, 0.75)
QUALITY_NOISE_PX = (0.25, 1.0)
# One seed per (outlier share, noise).  At 0.75 the seeds are chosen so that on the CPU the affine restatement finds
# >= 0.9 of the planted inliers and the 8-point twin (oracle_ransac) <= 0.6: conditions on the inputs, checked by
# test_affine_cases_cpu.py; the first seed from 1 on that satisfies them is taken.  The other rows take seed 1.
QUALITY_SEEDS = {(0.5, 0.25): 1, (0.5, 1.0): 1, (0.65, 0.25): 1, (0.65, 1.0): 1, (0.75, 0.25): 1, (0.75, 1.0): 1}


def quality_scene(out_frac, noise_px, seed, n=QUALITY_MATCHES, width=2048):
    """(pos1, pos2, corr, planted) of n matches of two orthographic views of points in the ball |p| <= 0.5 (synth's
    cameras and normalisation), noise_px of Gaussian noise on the second view, a share out_frac of the matches with a
    uniformly drawn second position; planted: the matches that kept their geometry."""
    from orthosfm_amd import synth
    st = (0xAF2 << 32) | (seed << 8)
    d = synth._unit_rows(synth.normal(rc.SEED, st | 1, 3 * n).reshape(n, 3))
    P = d * (0.5 * np.cbrt(synth.uniform(rc.SEED, st | 2, n)))[:, None]
    xy1 = synth.project_euler(P, 0.3, 0.1, -0.05, 0.0, 0.0, 1.0, width, width)
    xy2 = synth.project_euler(P, 0.9, -0.2, 0.1, 0.0, 0.0, 1.0, width, width)
    xy2 = xy2 + noise_px * synth.normal(rc.SEED, st | 3, 2 * n).reshape(n, 2)
    p1 = (xy1 + 0.5 - width / 2) / width
    p2 = (xy2 + 0.5 - width / 2) / width
    n_out = int(out_frac * n)
    out = np.argsort(synth.uniform(rc.SEED, st | 4, n), kind="stable")[:n_out]
    p2[out] = synth.uniform(rc.SEED, st | 5, 2 * n_out).reshape(n_out, 2) - 0.5
    planted = np.ones(n, bool)
    planted[out] = False
    perm1 = np.argsort(synth.uniform(rc.SEED, st | 6, n), kind="stable")
    perm2 = np.argsort(synth.uniform(rc.SEED, st | 7, n), kind="stable")
    pos1, pos2 = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    pos1[perm1], pos2[perm2] = p1, p2
    corr = np.stack([perm1, perm2], axis=1).astype(np.int32)
    order = np.argsort(corr[:, 0], kind="stable")
    return pos1, pos2, corr[order], planted[order]


def recall(inliers, planted):
    """The share of the planted inliers in an inlier list."""
    got = np.zeros(planted.size, bool)
    got[np.asarray(inliers, dtype=np.int64)] = True
    return float((got & planted).sum()) / float(planted.sum())


# ---------------------------------------------------------------------------
# pipeline: a set with repeated structure, and what survives the verification
# ---------------------------------------------------------------------------
PIPELINE_SET = dict(num_views=5, feats_per_view=1500, config_id=24, twin_frac=0.3)


def pipeline_set():
    from orthosfm_amd import synth
    kw = dict(PIPELINE_SET)
    return synth.make_image_set(kw.pop("num_views"), kw.pop("feats_per_view"), **kw)


def normalised(iset, v):
    """normalize_feature_positions of view v (feature_set.cc:42-55)."""
    return ((iset.pos[v] + 0.5 - np.array([iset.width / 2, iset.height / 2])) / max(iset.width, iset.height)).astype(np.float32)


def landmark_counts(iset, lists):
    """(correspondences between equal landmarks, between different ones) of lists of (view 1, view 2, (n, 2) ids)."""
    same = diff = 0
    for a, b, c in lists:
        la, lb = iset.landmark[a][c[:, 0]], iset.landmark[b][c[:, 1]]
        ok = (la == lb) & (la >= 0)
        same += int(ok.sum())
        diff += int((~ok).sum())
    return same, diff
