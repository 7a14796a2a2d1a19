"""The affine RANSAC of orthosfm_amd/csrc/ransac_affine.hip in numpy float64, operation for operation: what
osfm_ransac_affine returns -- count, inlier list, F, result record -- equals run() in every byte.

Python floats and numpy float64 arrays are IEEE doubles without contraction, as the kernel's build is; math.sqrt and the
division are correctly rounded on both sides.  The order of every sum is written out here and is the kernel's:

  sample      the first 4 distinct values of ransac_rand(seed, pair, it, d) % k, d = 0, 1, ..., ascending
  hypothesis  rows (x2, y2, x1, y1, 1) of the 4 matches; Gauss-Jordan elimination with full pivoting, the pivot the
              first largest modulus in row-major order of the remaining block, not > 0: invalid; row r times 1 / pivot,
              then row i -= A[i][r] * row r; null vector f[perm[r]] = -A[r][4], f[perm[4]] = 1;
              s = ((f0^2 + f1^2) + f2^2) + f3^2, not > 0: invalid; v = f * (1 / sqrt(s))
  test        n = (x2 a + y2 b) + ((x1 c + y1 d) + e), squared; s = ((a^2 + b^2) + c^2) + d^2; inlier when
              n < s thr_lo, not when n >= s thr_hi, else when n / s < thr^2 (thr_lo, thr_hi = thr^2 (1 -+ 2^-49)).
              This is sampson(F_A) < thr^2 of the 8-point kernel, term for term, with F_A's zeros left out.
  selection   strictly more inliers wins, so equal counts keep the lower iteration; a count of 0 never wins
  refit       when the winner has >= 5 inliers: z = (x2, y2, x1, y1); lane t = i % 256 adds its matches i = t, t + 256,
              ... in order (a match that is no inlier adds +0.0), then p[t] += p[t + st] for st = 128, 64, ..., 1;
              mean = sum / count; the ten products (z_p - mean_p)(z_q - mean_q), p <= q, summed the same way; cyclic
              Jacobi (eig3_fixed's steps on 4 x 4, at most 30 sweeps, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3));
              (a, b, c, d) = the column of the smallest diagonal entry (the first of equal ones),
              e = -(((a m0 + b m1) + c m2) + d m3); accepted when its count >= the winner's
The keyword arguments of run() plant the faults that tests/test_affine_cases_cpu.py shows the reference to catch.
"""
import math

import numpy as np

from ransac_cases import ransac_rand

LANES = 256
REFIT_MIN = 5
JACOBI_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def sample4(seed, pair, it, k):
    """4 distinct match ids in [0, k), ascending."""
    got, d = [], 0
    while len(got) < 4:
        v = ransac_rand(seed, pair, it, d) % k
        d += 1
        if v not in got:
            got.append(v)
    return sorted(got)


def four_point(m1, m2):
    """(ok, v (5,) float64) of 4 matches m1, m2 (4, 2): the null vector (a, b, c, d, e), zero when not ok."""
    A = [[float(m2[i][0]), float(m2[i][1]), float(m1[i][0]), float(m1[i][1]), 1.0] for i in range(4)]
    perm = [0, 1, 2, 3, 4]
    for r in range(4):
        best, pr, pc = -1.0, r, r
        for i in range(r, 4):
            for j in range(r, 5):
                m = abs(A[i][j])
                if m > best:
                    best, pr, pc = m, i, j
        if not best > 0.0:
            return False, np.zeros(5)
        A[r], A[pr] = A[pr], A[r]
        if pc != r:
            for i in range(4):
                A[i][r], A[i][pc] = A[i][pc], A[i][r]
            perm[r], perm[pc] = perm[pc], perm[r]
        inv = 1.0 / A[r][r]
        for j in range(r + 1, 5):
            A[r][j] = A[r][j] * inv
        for i in range(4):
            if i != r:
                fct = A[i][r]
                for j in range(r + 1, 5):
                    A[i][j] = A[i][j] - fct * A[r][j]
    f = [0.0] * 5
    f[perm[4]] = 1.0
    for r in range(4):
        f[perm[r]] = -A[r][4]
    s = ((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) + f[3] * f[3]
    if not s > 0.0:
        return False, np.zeros(5)
    inv = 1.0 / math.sqrt(s)
    return True, np.array([c * inv for c in f])


def below(v, m1, m2, thr, le=False, squared=True, transpose=False):
    """Mask of the matches the kernel's test takes for inliers of v.  Faults: le -- <= at the threshold; squared=False
    -- the threshold itself in the place of its square; transpose -- F_A^T scores (the two views' roles exchanged)."""
    a, b, c, d, e = (float(x) for x in v)
    if transpose:
        a, b, c, d = c, d, a, b
    thr2 = thr * thr if squared else thr
    thr_lo = thr2 * (1.0 - 1.7763568394002505e-15)
    thr_hi = thr2 * (1.0 + 1.7763568394002505e-15)
    x1, y1, x2, y2 = m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]
    n = (x2 * a + y2 * b) + ((x1 * c + y1 * d) + e)
    n = n * n
    s = ((a * a + b * b) + c * c) + d * d
    with np.errstate(all="ignore"):
        sure = n < s * thr_lo
        never = n >= s * thr_hi
        q = np.divide(n, s)
        sliver = q < thr2
        if le:
            return q <= thr2
    return sure | (~never & sliver)


def lane_sums(vals, mask):
    """vals (q, k) summed over the matches of mask in the kernel's order: per lane in order, then the fixed tree."""
    q, k = vals.shape
    rounds = (k + LANES - 1) // LANES
    pad = np.zeros((q, rounds * LANES))
    pad[:, :k] = np.where(mask[None, :], vals, 0.0)
    acc = np.zeros((q, LANES))
    for r in range(rounds):
        acc = acc + pad[:, r * LANES:(r + 1) * LANES]
    st = LANES // 2
    while st >= 1:
        acc[:, :st] = acc[:, :st] + acc[:, st:2 * st]
        st //= 2
    return acc[:, 0].copy()


def eig4_fixed(C):
    """(w [4], V [4][4]) of a symmetric 4 x 4 matrix (list of lists of floats) by the kernel's cyclic Jacobi."""
    A = [[float(x) for x in row] for row in C]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(30):
        off = ((((abs(A[0][1]) + abs(A[0][2])) + abs(A[0][3])) + abs(A[1][2])) + abs(A[1][3])) + abs(A[2][3])
        if off == 0.0:
            break
        for p, q in JACOBI_PAIRS:
            if A[p][q] == 0.0:
                continue
            th = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
            t = (1.0 if th >= 0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(4):
                akp, akq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(4):
                apk, aqk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return [A[i][i] for i in range(4)], V


def refit_vector(m1, m2, inl, largest=False, keep_mean=False):
    """The least-squares F_A (5,) of the matches of mask inl.  Faults: largest -- the eigenvector of the largest
    eigenvalue; keep_mean -- the mean is not subtracted before the products."""
    z = np.stack([m2[:, 0], m2[:, 1], m1[:, 0], m1[:, 1]])
    mu = lane_sums(z, inl) / float(int(inl.sum()))
    dz = z if keep_mean else z - mu[:, None]
    prods = np.stack([dz[p] * dz[q] for p in range(4) for q in range(p, 4)])
    c = lane_sums(prods, inl)
    C = [[0.0] * 4 for _ in range(4)]
    n = 0
    for p in range(4):
        for q in range(p, 4):
            C[p][q] = C[q][p] = float(c[n])
            n += 1
    w, V = eig4_fixed(C)
    m = 0
    for i in (1, 2, 3):
        if (w[i] > w[m]) if largest else (w[i] < w[m]):
            m = i
    a, b, cc, d = (V[q][m] for q in range(4))
    mu = [float(x) for x in mu]
    e = -(((a * mu[0] + b * mu[1]) + cc * mu[2]) + d * mu[3])
    return np.array([a, b, cc, d, e])


def layout(v):
    """F_A (3, 3) in the layout of sampson(): F[2] = a, F[5] = b, F[6] = c, F[7] = d, F[8] = e."""
    F = np.zeros(9)
    F[2], F[5], F[6], F[7], F[8] = v
    return F.reshape(3, 3)


def matches(pos1, pos2, corr):
    pos1 = np.asarray(pos1, dtype=np.float32).reshape(-1, 2)
    pos2 = np.asarray(pos2, dtype=np.float32).reshape(-1, 2)
    corr = np.asarray(corr, dtype=np.int32).reshape(-1, 2)
    return pos1[corr[:, 0]].astype(np.float64), pos2[corr[:, 1]].astype(np.float64)


def hypotheses(pos1, pos2, corr, max_iterations, seed, pair_id):
    """(valid (n,) bool, v (n, 5)) of iterations 0 .. max_iterations - 1."""
    m1, m2 = matches(pos1, pos2, corr)
    k = m1.shape[0]
    valid, vs = np.zeros(max_iterations, bool), np.zeros((max_iterations, 5))
    for it in range(max_iterations):
        idx = sample4(seed, pair_id, it, k)
        valid[it], vs[it] = four_point(m1[idx], m2[idx])
    return valid, vs


def run(pos1, pos2, corr, max_iterations=1000, threshold=0.0015, seed=0, pair_id=0, refit=True, *, le=False,
        squared=True, transpose=False, replace_equal=False, largest=False, keep_mean=False, detail=None):
    """osfm_ransac_affine: (count, inlier ids int32, F (3, 3), record dict).  detail (a dict) receives the per-iteration
    `valid` and `counts` and the winner's and the refit's vectors."""
    record = {"best_iteration": -1, "ransac_inliers": 0, "refit_ran": 0, "refit_accepted": 0}
    m1, m2 = matches(pos1, pos2, corr)
    k = m1.shape[0]
    if k < 4:
        return -1, np.zeros(0, np.int32), np.zeros((3, 3)), record
    test = lambda v: below(v, m1, m2, threshold, le=le, squared=squared, transpose=transpose)
    valid, vs = hypotheses(pos1, pos2, corr, max_iterations, seed, pair_id)
    counts = np.zeros(max_iterations, np.int32)
    best, best_it = 0, -1
    for it in range(max_iterations):
        if not valid[it]:
            continue
        counts[it] = int(test(vs[it]).sum())
        if counts[it] > best or (replace_equal and counts[it] == best and best > 0):
            best, best_it = int(counts[it]), it
    if detail is not None:
        detail.update(valid=valid, counts=counts, vectors=vs)
    if best == 0:
        return 0, np.zeros(0, np.int32), np.zeros((3, 3)), record
    v = vs[best_it]
    record.update(best_iteration=best_it, ransac_inliers=best)
    if refit and best >= REFIT_MIN:
        vr = refit_vector(m1, m2, test(v), largest=largest, keep_mean=keep_mean)
        record["refit_ran"] = 1
        if detail is not None:
            detail.update(winner=v.copy(), refit=vr.copy())
        if int(test(vr).sum()) >= best:
            record["refit_accepted"] = 1
            v = vr
    inl = np.nonzero(test(v))[0].astype(np.int32)
    return int(inl.size), inl, layout(v), record
