"""Cases, reference, bound and check of the geometric verification (ransac_kernel in ransac_kernels.hip, reached
through osfm_ransac_fundamental).

The reference is written from the reference project's fundamental_8_point, enforce_fundamental_constraints and
sampson_distance (fundamental.cc:78-127,225-246) and RansacFundamental::estimate (ransac_fundamental.cc:26-105), not
from the kernel or from oracle/ransac_oracle.c, which is the kernel's line-for-line twin.  Only the sample stream is
the library's: draw d of iteration i of pair p is splitmix64 of (seed, p, i, d) as ransac_rand.h defines it, restated
here in Python integers; 8 distinct draws mod k, in ascending order (the std::set of :71-76).  Per iteration:
  null vector   of the 8x9 system (rows x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1), EXACTLY: the inputs are
                float32, their products are exact in float64, and the elimination runs in fractions.Fraction.  An exact
                rank below 8 makes the iteration *unconstrained*: the reference's "last column of V" is then any vector
                of a null space of two or more dimensions.
  rank 2        with mpmath at 200 bits: the null vector at unit norm, its 3x3 SVD, sigma_3 set to 0 (U S V^T), the
                result brought to unit Frobenius norm for the comparison.  gap = (sigma_2 - sigma_3) / sigma_1; below
                GAP_MIN = 2^-40 the direction that is removed is decided at rounding level and the iteration is
                *unconstrained* too.
  kappa         sigma_1 / sigma_8 of the 8x9 system (mpmath), and A = kappa / gap.
  Sampson       distance of every match under the reference F (rounded to float64) in float64 numpy, and a band
                around thr^2 (below): count_ref = matches clearly below, amb = matches inside.
The reference winner is the first constrained iteration that reaches the largest count_ref.

Bound on F.  With both matrices at unit Frobenius norm, max |F_gpu -+ F_ref| <= TAU 2^-53 A over both signs.  The
null vector of a full-rank 8x9 system moves by kappa times a relative perturbation of the system, and the singular
pair that the rank-2 step removes turns by |dF| / (sigma_2 - sigma_3), so A follows each hypothesis's conditioning:
2e2 .. 8e5 on the benign scene, up to 1.5e9 within 1e-4 of a plane, 1e11 .. 1.5e12 at a coordinate scale of 1e-4.

Band.  A match is an inlier when n^2 / s < thr^2, n = x2^T F x1, s = a^2 + b^2 + t3^2 + t4^2 (the first two
components of F x1 and of F^T x2), i.e. when |n| < thr sqrt(s).  Let F' = F + dF with max |dF| <= eps and put
c1 = |x1| + |y1| + 1, c2 = |x2| + |y2| + 1.  Then |dn| <= eps c1 c2 (nine terms |x2_i| |x1_j| eps), each of a, b is
off by at most eps c1 and each of t3, t4 by eps c2, so that |d sqrt(s)| <= eps sqrt(2 c1^2 + 2 c2^2) (triangle
inequality in R^4); for coordinates of modulus <= 1 these are 9 eps and 6 eps.  The decision under F' can differ
from the one under F only if  | |n| - thr sqrt(s) | <= |dn| + thr |d sqrt(s)|,  that is for
    d / thr^2 in [(1 - beta)^2, (1 + beta)^2],   beta = (c1 c2 + thr sqrt(2 c1^2 + 2 c2^2)) eps / (thr sqrt(s)),
sqrt(s) per match from the reference.  eps = (TAU A + 32) 2^-53: the 32 stands for the float64 roundings of both
evaluations (|F_ij| <= 1; n and every term of s are sums of at most 9 products, 8 roundings deep at most on either
side, plus the rounding of F_ref to float64: 17 in all, 32 taken).  A match with beta >= 1 or s = 0 is ambiguous.

TAU.  The twin (oracle_fundamental_8_point, plain double arithmetic: Gauss-Jordan with full pivoting, Jacobi on
F^T F) was measured on every constrained hypothesis of every case, test_ransac_cases_cpu.py prints the ratio per
case; TAU is the next power of two above four times the largest.  The ratio does not grow with kappa: see
TWIN_RATIO below and DESIGN 2.5.

Inputs are the same on any machine: positions are float32 and correspondences int32; the rotations (sin, cos) and the
noise (log, cos) are rounded to float32 before they are used, and every later step is +, * on float64 arrays written
out term by term, so no BLAS and no libm can move a bit.  The SHA-256 of each case's arrays and parameters is stored
in the golden (tests/golden/ransac_reference.npz, written by tests/golden/make_ransac_golden.py) and asserted by
load(); the GPU tests read only that file and need neither mpmath nor the reference.

Cases (threshold 0.0015 unless said otherwise; positions of a scene are two orthographic views of points in the unit
cube, noise 2e-4 on the second view, a share of the matches with a uniformly drawn second position):
  single hypotheses (max_iterations = 1, pair ids 0..63: 64 samples per scene), 400 matches, 25 % outliers unless said
    benign              noise 1e-3
    near_planar_1e-2, near_planar_1e-4
                        points within that relief of a plane, no noise but the float32 rounding of the positions
                        and no outliers (two of them in a sample lift the planar system's rank from 6 to 8 and hide
                        the conditioning).  The median kappa is 4.3e4 and 3.9e6, the largest 2.2e6 and 1.2e9: it
                        grows like 1 / relief (the relief adds z, z x1, z y1 at first order to the six polynomials
                        that span a planar system's columns), not like its square
    scale_1e-4          positions times 1e-4, neither noise nor outliers (kappa 1e10 .. 1e12 from the columns' scales)
    edge_1              positions stretched to +-1, the largest four of each view exactly +-1
  path shapes (1000 iterations, 30 % outliers)
    k_8 .. k_2500       K_LIST matches: around the wave (64), the listing loop (256) and the LDS chunk (1024), the
                        scalar tail of the four-at-a-time scoring loop (1025, 1027), two and three chunks.  k_8: every
                        sample is the same eight matches, two of them outliers; its one F has no inlier, which is the
                        kernel's exit with valid hypotheses and a best count of 0 (count 0, F zero)
    iters_1 .. iters_1025
                        700 matches, ITER_LIST iterations: a part without an iteration (<= 512), with one (513), a
                        second pass of part 0 beside one hypothesis in part 1 (1025)
    tie_part1, tie_both, tie_thread
                        150 matches; the largest count is reached in part 1 only / in both parts, first in part 0 /
                        twice in one pass of one part, first by the higher thread.  The tied iterations have different F
    mixed_chunks        2500 matches; two of chunk 1 (ids 1024..2047) have a coordinate outside [-1, 1], one 1.5 and
                        one nextafter(1, 2): that chunk is scored in double, chunks 0 and 2 are pre-classified
  at_threshold          one hypothesis whose threshold t has t * t == the Sampson distance of one match in the twin's
                        arithmetic: d < thr^2 leaves it out, d <= thr^2 would take it.  Such a match lies in every
                        band, so this case is held to the twin and to that property
  degenerate (held to the twin and to stated properties)
    identical_views     600 matches on a 2^-10 grid, pos2 = pos1: most samples are refused, the others give an
                        antisymmetric F under which every match is an inlier (n == k)
    one_point           20 matches at one position: every sample is refused, count 0, F zero, empty list
    twins               1200 matches, 30 % of them copies of another match: a sample with a copy has exact rank < 8
                        (unconstrained) while the twin's pivots are rounding noise and it reports the sample valid.
                        Their counts, taken from the twin, lie below the best constrained count (recorded in the
                        golden), so the reference winner holds here too
"""
import hashlib
import os
from fractions import Fraction

import numpy as np

from orthosfm_amd import synth

U = 2.0 ** -53
# The twin's largest ratio max|F -+ F_ref| / (2^-53 A) over the 21 000 constrained hypotheses of all cases, as
# make_ransac_golden.py prints it (CPU): 0.0914, on edge_1 at kappa 1e2.  It does not grow with kappa -- 0.026 on
# benign (kappa <= 2e4), 0.042 and 0.056 on near_planar_1e-2 and _1e-4 (kappa up to 2.2e6 and 1.2e9), 6e-6 on scale_1e-4
# (kappa 3e10 .. 1.4e12, all of it the columns' scales, which full pivoting does not feel): the elimination loses
# nothing that kappa / gap does not explain.
TWIN_RATIO = 0.0914
TAU = 0.5                            # the next power of two above 4 x TWIN_RATIO; the kernel is the twin bit for bit
IDENTICAL_REFUSED = 950              # of the 1000 hypotheses of identical_views, refused by the twin (a zero pivot)
AT_THRESHOLD_COUNT = 279             # inliers of at_threshold; 280 matches have d <= thr^2
THR = 0.0015
BITS = 200
GAP_MIN = 2.0 ** -40
FL_ROUNDINGS = 32.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac_reference.npz")
SEED = synth.BASE_SEED
_ST = 0x8F2 << 32                    # streams of synth's counter-based generator used here

K_LIST = (8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2048, 2049, 2500)
ITER_LIST = (1, 2, 256, 257, 511, 512, 513, 1000, 1024, 1025)
SINGLE = ("benign", "near_planar_1e-2", "near_planar_1e-4", "scale_1e-4", "edge_1")
PAIRS = tuple(range(64))
# (seed, pair id) of the tie cases, found with the twin on the CPU and confirmed from count_ref (test_ransac_cases_cpu.py)
TIES = {"tie_part1": (1, 7), "tie_both": (1, 1), "tie_thread": (1, 0)}
# at_threshold: (seed, pair id, match, threshold as float.hex)
AT_THRESHOLD = (11, 0, 382, "0x1.8a03a238e76cdp-10")


# ---------------------------------------------------------------------------
# sample stream (ransac_rand.h in Python integers)
# ---------------------------------------------------------------------------
_M = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def ransac_rand(seed, pair, it, draw):
    return splitmix64((splitmix64((seed ^ (pair * 0xD1342543DE82EF95)) & _M) + it * 0x2545F4914F6CDD1D + draw) & _M)


def sample8(seed, pair, it, k):
    """8 distinct match ids in [0, k), ascending."""
    got, d = [], 0
    while len(got) < 8:
        v = ransac_rand(seed, pair, it, d) % k
        d += 1
        if v not in got:
            got.append(v)
    return sorted(got)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

class Case:
    def __init__(self, name, kind, pos1, pos2, corr, max_iterations=1000, threshold=THR, seed=11, pairs=(0,)):
        self.name, self.kind = name, kind
        self.pos1 = np.ascontiguousarray(pos1, dtype=np.float32)
        self.pos2 = np.ascontiguousarray(pos2, dtype=np.float32)
        self.corr = np.ascontiguousarray(corr, dtype=np.int32)
        self.max_iterations, self.threshold, self.seed, self.pairs = max_iterations, threshold, seed, tuple(pairs)
        for a in (self.pos1, self.pos2, self.corr):
            a.setflags(write=False)

    @property
    def k(self):
        return self.corr.shape[0]

    def matches(self):
        """(k, 2) float64 positions of the matches in view 1 and in view 2."""
        return self.pos1[self.corr[:, 0]].astype(np.float64), self.pos2[self.corr[:, 1]].astype(np.float64)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _order(stream, n):
    return np.argsort(synth.uniform(SEED, _ST | stream, n), kind="stable")


def _views(k, out_frac, stream, noise=2e-4, relief=None):
    """Matched positions p1, p2 (k, 2) float64 on the float32 grid: two orthographic views of k points."""
    P = synth.uniform(SEED, _ST | stream, 3 * k).reshape(k, 3) - 0.5
    if relief is not None:
        P[:, 2] *= 2.0 * relief
    P = _f32(P)
    out = []
    for ang in ((0.3, 0.1, -0.05), (0.9, -0.2, 0.1)):
        R = _f32(synth.euler_matrix(*ang).T @ synth._T)
        x = (P[:, 0] * R[0, 0] + P[:, 1] * R[0, 1]) + P[:, 2] * R[0, 2]
        y = (P[:, 0] * R[1, 0] + P[:, 1] * R[1, 1]) + P[:, 2] * R[1, 2]
        out.append(np.stack([-0.5 * x, -0.5 * y], axis=1))
    p1, p2 = out
    if noise:
        p2 = p2 + noise * _f32(synth.normal(SEED, _ST | (stream + 1), 2 * k)).reshape(k, 2)
    n_out = int(out_frac * k)
    if n_out:
        p2[_order(stream + 2, k)[:n_out]] = synth.uniform(SEED, _ST | (stream + 3), 2 * n_out).reshape(n_out, 2) - 0.5
    return _f32(p1), _f32(p2)


def _scatter(p1, p2, stream):
    """Feature arrays in which the matches lie scattered, and the correspondences in the order of view 1."""
    k = p1.shape[0]
    perm1, perm2 = _order(stream + 4, k), _order(stream + 5, k)
    pos1, pos2 = np.zeros((k, 2), np.float32), np.zeros((k, 2), np.float32)
    pos1[perm1], pos2[perm2] = p1, p2
    corr = np.stack([perm1, perm2], axis=1).astype(np.int32)
    return pos1, pos2, corr[np.argsort(corr[:, 0], kind="stable")]


def _single(name):
    stream = 0x100 + 0x10 * SINGLE.index(name)
    if name == "benign":
        p1, p2 = _views(400, 0.25, stream, noise=1e-3)
    elif name.startswith("near_planar"):
        p1, p2 = _views(400, 0.0, stream, noise=0.0, relief=float(name.split("_")[-1]))
    elif name == "scale_1e-4":
        # neither noise nor outliers: a sample that fits noise at this scale has an F of quadratic terms alone, under
        # which sqrt(s) is 1e-5 and every match lies in the band of any bound that follows kappa >= 1e10
        p1, p2 = _views(400, 0.0, stream, noise=0.0)
        p1, p2 = _f32(p1 * 1e-4), _f32(p2 * 1e-4)
    else:
        p1, p2 = _views(400, 0.25, stream)
        s = 1.0 / max(np.abs(p1).max(), np.abs(p2).max())
        p1, p2 = np.clip(_f32(p1 * s), -1.0, 1.0), np.clip(_f32(p2 * s), -1.0, 1.0)
        for p in (p1, p2):
            flat = p.reshape(-1)
            top = np.argsort(-np.abs(flat), kind="stable")[:4]
            flat[top] = np.sign(flat[top])
    return Case(name, "single", *_scatter(p1, p2, stream), max_iterations=1, pairs=PAIRS)


def _k_case(k):
    stream = 0x1000 + 0x10 * K_LIST.index(k)
    return Case(f"k_{k}", "full", *_scatter(*_views(k, 0.3, stream), stream), pairs=(k,))


def _iters_case(n):
    return Case(f"iters_{n}", "full", *_scatter(*_views(700, 0.3, 0x2000), 0x2000), max_iterations=n, pairs=(5,))


def _tie_case(name):
    seed, pair = TIES[name]
    return Case(name, "full", *_scatter(*_views(150, 0.3, 0x3000), 0x3000), seed=seed, pairs=(pair,))


def _mixed_chunks():
    p1, p2 = _views(2500, 0.3, 0x4000)
    pos1, pos2, corr = _scatter(p1, p2, 0x4000)
    pos2[corr[1500, 1], 0] = 1.5
    pos1[corr[2047, 0], 1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    return Case("mixed_chunks", "full", pos1, pos2, corr, pairs=(9,))


def _at_threshold():
    seed, pair, _, thr = AT_THRESHOLD
    return Case("at_threshold", "twin", *_scatter(*_views(400, 0.25, 0x5000), 0x5000), max_iterations=1,
                threshold=float.fromhex(thr), seed=seed, pairs=(pair,))


def _identical_views():
    g = np.floor(synth.uniform(SEED, _ST | 0x6000, 1200) * 1024.0).reshape(600, 2) * 2.0 ** -10 - 0.5
    pos1, _, corr = _scatter(g, g, 0x6000)
    corr = np.stack([corr[:, 0], corr[:, 0]], axis=1)
    return Case("identical_views", "twin", pos1, pos1.copy(), corr, pairs=(2,))


def _one_point():
    pos = np.tile(np.array([[0.25, -0.125]], np.float32), (20, 1))
    corr = np.stack([np.arange(20), np.arange(20)[::-1]], axis=1)
    return Case("one_point", "twin", pos, pos.copy(), corr, pairs=(3,))


def _twins():
    p1, p2 = _views(1200, 0.2, 0x7000)
    order = _order(0x7006, 1200)
    copies, rest = order[:360], order[360:]
    src = rest[np.floor(synth.uniform(SEED, _ST | 0x7007, 360) * rest.size).astype(np.int64)]
    p1[copies], p2[copies] = p1[src], p2[src]
    return Case("twins", "twins", *_scatter(p1, p2, 0x7000), pairs=(4,))


FULL = tuple(f"k_{k}" for k in K_LIST) + tuple(f"iters_{n}" for n in ITER_LIST) + tuple(TIES) + ("mixed_chunks",)
TWIN_ONLY = ("at_threshold", "identical_views", "one_point")
ALL = SINGLE + FULL + ("twins",) + TWIN_ONLY


def build(name):
    if name in SINGLE:
        return _single(name)
    if name.startswith("k_"):
        return _k_case(int(name[2:]))
    if name.startswith("iters_"):
        return _iters_case(int(name[6:]))
    if name in TIES:
        return _tie_case(name)
    return {"mixed_chunks": _mixed_chunks, "at_threshold": _at_threshold, "identical_views": _identical_views,
            "one_point": _one_point, "twins": _twins}[name]()


def input_hash(case):
    h = hashlib.sha256()
    h.update(np.array([case.k, case.max_iterations, case.seed, *case.pairs], dtype=np.int64).tobytes())
    h.update(np.array([case.threshold], dtype=np.float64).tobytes())
    for a in (case.pos1, case.pos2, case.corr):
        h.update(np.array(a.shape, dtype=np.int64).tobytes())
        h.update(a.tobytes())
    return h.hexdigest()


def part_of(it, max_iterations):
    """(part, pass, thread, slot) of an iteration in the kernel's split over 2 workgroups in passes of 2 x 256."""
    per_part = ((max_iterations + 1) // 2 + 511) // 512 * 512
    r = it % per_part
    return it // per_part, r // 512, r % 256, (r % 512) // 256


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------

def system(p1, p2):
    """The 8x9 system of fundamental.cc:85-98; exact in float64 for float32 positions."""
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=1)


def exact_null_vector(A):
    """(rank, null vector as 9 Fractions or None when the rank is below 8) of an 8x9 float64 matrix."""
    M = [[Fraction(float(v)) for v in row] for row in A]
    rows, cols = len(M), len(M[0])
    piv = []
    r = 0
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
                M[i] = [a - f * b for a, b in zip(M[i], M[r])]
        piv.append(c)
        r += 1
    if r < 8:
        return r, None
    free = next(c for c in range(cols) if c not in piv)
    f = [Fraction(0)] * cols
    f[free] = Fraction(1)
    for i, c in enumerate(piv):
        f[c] = -M[i][free]
    return 8, f


def hypothesis(p1, p2, bits=BITS):
    """The reference's F of one sample: dict(uncon, F (9,) float64 at unit Frobenius norm, A, kappa, gap)."""
    import mpmath as mp
    A = system(p1, p2)
    _, f = exact_null_vector(A)
    res = {"uncon": 1, "F": np.zeros(9), "A": 0.0, "kappa": 0.0, "gap": 0.0}
    if f is None:
        return res
    with mp.workprec(bits):
        fm = [mp.mpf(v.numerator) / mp.mpf(v.denominator) for v in f]
        n = mp.sqrt(sum(v * v for v in fm))
        Fm = mp.matrix(3, 3)
        for i in range(9):
            Fm[i // 3, i % 3] = fm[i] / n
        Um, S, Vm = mp.svd_r(Fm)
        order = sorted(range(3), key=lambda i: -S[i])
        s1, s2, s3 = (S[i] for i in order)
        gap = (s2 - s3) / s1
        F2 = mp.matrix(3, 3)
        for i in order[:2]:
            for a in range(3):
                for b in range(3):
                    F2[a, b] += S[i] * Um[a, i] * Vm[i, b]
        nn = mp.sqrt(sum(F2[a, b] ** 2 for a in range(3) for b in range(3)))
        sv = mp.svd_r(mp.matrix(A.tolist()), compute_uv=False)
        sv = sorted((sv[i] for i in range(8)), reverse=True)
        kappa = sv[0] / sv[7]
        res["gap"], res["kappa"] = float(gap), float(kappa)
        if gap < GAP_MIN:
            return res
        res["uncon"] = 0
        res["F"] = np.array([float(F2[i // 3, i % 3] / nn) for i in range(9)])
        res["A"] = float(kappa / gap)
    return res


def _hyp_job(args):
    return hypothesis(*args)


def classify(F, A, m1, m2, thr, tau=None):
    """(clear inliers, ambiguous) boolean masks of the matches under the reference F (9,) with bound A."""
    tau = TAU if tau is None else tau
    x1, y1, x2, y2 = m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]
    a = x1 * F[0] + y1 * F[1] + F[2]
    b = x1 * F[3] + y1 * F[4] + F[5]
    c = x1 * F[6] + y1 * F[7] + F[8]
    n = np.abs(x2 * a + y2 * b + c)
    t3 = x2 * F[0] + y2 * F[3] + F[6]
    t4 = x2 * F[1] + y2 * F[4] + F[7]
    rs = np.sqrt(a * a + b * b + t3 * t3 + t4 * t4)
    c1, c2 = np.abs(x1) + np.abs(y1) + 1.0, np.abs(x2) + np.abs(y2) + 1.0
    eps = (tau * A + FL_ROUNDINGS) * U
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = (c1 * c2 + thr * np.sqrt(2.0 * c1 * c1 + 2.0 * c2 * c2)) * eps / (thr * rs)
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
    samples = [tuple(sample8(case.seed, pair, it, case.k)) for it in range(n_iter)]
    new = sorted(set(samples) - set(have))
    if new:
        m1, m2 = case.matches()
        jobs = [(m1[list(idx)], m2[list(idx)]) for idx in new]
        have.update(zip(new, pool.map(_hyp_job, jobs, chunksize=8) if pool is not None else map(_hyp_job, jobs)))
    return [have[idx] for idx in samples]


def reference(case, pool=None, tau=None):
    """The golden arrays of a case (a dict of numpy arrays)."""
    m1, m2 = case.matches()
    k = case.k
    out = {"sha256": np.array(input_hash(case))}
    if case.kind == "single":
        hyps = [hypotheses(case, p, 1, pool)[0] for p in case.pairs]
    else:
        hyps = hypotheses(case, case.pairs[0], case.max_iterations, pool)
    n = len(hyps)
    count, amb = np.zeros(n, np.int16), np.zeros(n, np.int16)
    clear = np.zeros((n, k), bool)
    ambm = np.zeros((n, k), bool)
    for i, h in enumerate(hyps):
        if not h["uncon"]:
            clear[i], ambm[i] = classify(h["F"], h["A"], m1, m2, case.threshold, tau)
            count[i], amb[i] = clear[i].sum(), ambm[i].sum()
    out["count_ref"], out["amb"] = count, amb
    out["uncon"] = np.array([h["uncon"] for h in hyps], np.uint8)
    if case.kind == "single":
        out["kappa"] = np.array([h["kappa"] for h in hyps])
        out["gap"] = np.array([h["gap"] for h in hyps])
        out["F"] = np.stack([h["F"] for h in hyps])
        out["A"] = np.array([h["A"] for h in hyps])
        out["clear"], out["ambm"] = np.packbits(clear, axis=1), np.packbits(ambm, axis=1)
    else:
        ok = out["uncon"] == 0
        w = int(np.argmax(np.where(ok, count, -1)))
        out["winner"] = np.array(w, np.int32)
        out["F"], out["A"] = hyps[w]["F"], np.array(hyps[w]["A"])
        out["clear"], out["ambm"] = np.packbits(clear[w]), np.packbits(ambm[w])
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
        assert input_hash(case) == str(g["sha256"]), f"{name}: inputs differ from those of tests/golden/ransac_reference.npz"
        _cases[name] = (case, g)
    return _cases[name]


def mask(bits, k):
    return np.unpackbits(bits, axis=-1)[..., :k].astype(bool)


def ratio(F, F_ref, A):
    """max |F / |F| -+ F_ref| / (2^-53 A), the smaller of both signs; inf when F is not finite or zero."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    nrm = np.sqrt((F * F).sum())
    if not np.isfinite(nrm) or nrm == 0.0:
        return np.inf
    F = F / nrm
    return float(min(np.abs(F - F_ref).max(), np.abs(F + F_ref).max()) / (U * A))


def check_list(inliers, clear, amb):
    """True when the inlier list holds every clear inlier and nothing but clear inliers and ambiguous matches."""
    got = np.zeros(clear.size, bool)
    got[np.asarray(inliers, dtype=np.int64)] = True
    return bool((got[clear].all()) and not (got & ~clear & ~amb).any())


# ---------------------------------------------------------------------------
# the twin, hypothesis by hypothesis (Python sampling, oracle_fundamental_8_point, numpy count)
# ---------------------------------------------------------------------------

def sampson(F, m1, m2):
    """Sampson distances in the operation order of fundamental.cc:234-246 (float64, no contraction)."""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    x1, y1, x2, y2 = m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]
    n = x2 * ((x1 * F[0] + y1 * F[1]) + F[2])
    n = n + y2 * ((x1 * F[3] + y1 * F[4]) + F[5])
    n = n + 1.0 * ((x1 * F[6] + y1 * F[7]) + F[8])
    n = n * n
    t = (x1 * F[0] + y1 * F[1]) + F[2]
    s = t * t
    t = (x1 * F[3] + y1 * F[4]) + F[5]
    s = s + t * t
    t = (x2 * F[0] + y2 * F[3]) + F[6]
    s = s + t * t
    t = (x2 * F[1] + y2 * F[4]) + F[7]
    s = s + t * t
    with np.errstate(divide="ignore", invalid="ignore"):
        return n / s


def twin_run(case, pair, eight_point=None, below=None, replace=None, transpose=False):
    """RansacFundamental::estimate as oracle_ransac_fundamental runs it, restated: per iteration (valid, count), and
    the result (count, inlier ids, F (3, 3)).  eight_point(p1, p2) -> (ok, F), below(d, thr) -> mask and
    replace(count, best) -> bool can be swapped for a perturbed version; transpose scores with F^T."""
    import oracle_lib
    eight_point = eight_point or oracle_lib.oracle_fundamental_8_point
    below = below or (lambda d, thr: d < thr * thr)
    replace = replace or (lambda count, best: count > best)
    m1, m2 = case.matches()
    best, bestF = 0, np.zeros((3, 3))
    valid, counts = np.zeros(case.max_iterations, bool), np.zeros(case.max_iterations, np.int32)
    for it in range(case.max_iterations):
        idx = sample8(case.seed, pair, it, case.k)
        ok, F = eight_point(m1[idx], m2[idx])
        if not ok:
            continue
        F = np.asarray(F, dtype=np.float64).reshape(3, 3)
        if transpose:
            F = F.T.copy()
        valid[it] = True
        counts[it] = int(below(sampson(F, m1, m2), case.threshold).sum())
        if replace(counts[it], best):
            best, bestF = int(counts[it]), F
    inl = np.nonzero(below(sampson(bestF, m1, m2), case.threshold))[0].astype(np.int32) if best > 0 else np.zeros(0, np.int32)
    return valid, counts, (inl.size, inl, bestF)


def twin_ratios(case, pair, hyps):
    """Per hypothesis the ratio of oracle_fundamental_8_point's F against the reference (0 where unconstrained)."""
    import oracle_lib
    m1, m2 = case.matches()
    r = np.zeros(len(hyps))
    for it, h in enumerate(hyps):
        if not h["uncon"]:
            idx = sample8(case.seed, pair, it, case.k)
            ok, F = oracle_lib.oracle_fundamental_8_point(m1[idx], m2[idx])
            r[it] = ratio(F, h["F"], h["A"]) if ok else np.inf
    return r


def check(name, results, tau=None):
    """What an implementation's results miss of a SINGLE, FULL or `twins` case's golden: a list of findings, empty when
    it passes, and the largest F ratio seen.  results: one (count, inlier ids, F) per pair id of the case."""
    tau = TAU if tau is None else tau
    case, g = load(name)
    bad, worst = [], 0.0
    assert len(results) == len(case.pairs)
    for j, (n, inl, F) in enumerate(results):
        single = case.kind == "single"
        if single and g["uncon"][j]:
            continue
        Fr, A = (g["F"][j], float(g["A"][j])) if single else (g["F"], float(g["A"]))
        clear, amb = mask(g["clear"][j] if single else g["clear"], case.k), mask(g["ambm"][j] if single else g["ambm"], case.k)
        what = f"{name} pair {case.pairs[j]}"
        if n != len(inl):
            bad.append(f"{what}: count {n} but {len(inl)} ids")
        if not clear.any() and not amb.any():
            if n != 0 or np.any(np.asarray(F) != 0):
                bad.append(f"{what}: no inlier under the reference, got {n}")
            continue
        r = ratio(F, Fr, A)
        worst = max(worst, r)
        if not r <= tau:
            bad.append(f"{what}: F is {r:.3g} x 2^-53 A from the reference (A {A:.2e})")
        if not (np.all(np.diff(inl) > 0) and check_list(inl, clear, amb)):
            bad.append(f"{what}: inlier list differs from the reference's ({len(inl)} ids, {int(clear.sum())} clear, {int(amb.sum())} in the band)")
    return bad, worst
