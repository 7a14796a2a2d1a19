"""Placing one view against triangulated points by a RANSAC over affine cameras, restated in numpy.

A float64 statement of INTEGRATION.md section 3b, written from that text -- not from the kernels -- with
numpy.linalg.solve / svd / cholesky where the library runs an elimination, closed forms and a Cholesky of its
own.  tests/test_resect_cases_cpu.py shows on it that the cases of tests/resect_cases.py are fit to judge a
kernel; tests/test_resect_gpu.py holds osfm_resect_view and osfm_scene_resect_view to it.

`resect(..., detail=True)` also returns what the CPU test bounds: per hypothesis the margins to every threshold
and the conditioning of its solve, the margin of the selection and the refit's pivot and conditioning.
"""
import math
from dataclasses import dataclass

import numpy as np

STATUS_OK, STATUS_TOO_FEW, STATUS_NO_MODEL = 0, 1, 2
SAMPLE = 4
M64 = (1 << 64) - 1
MAX_ITERATIONS = 1 << 20
DEFAULT_MIN_PIVOT = 1e-6


# ---- the counter-based generator of the library's RANSACs ----
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def ransac_rand(seed, stream, it, draw):
    return splitmix64((splitmix64(seed ^ ((stream * 0xD1342543DE82EF95) & M64)) + it * 0x2545F4914F6CDD1D + draw) & M64)


def sample(seed, stream, it, n):
    """The first four distinct values of ransac_rand(...) % n, in draw order."""
    out, k = [], 0
    while len(out) < SAMPLE:
        i = ransac_rand(seed, stream, it, k) % n
        k += 1
        if i not in out:
            out.append(i)
    return out


def num_iterations(max_iterations=0, probability=0.999, inlier_ratio=0.5):
    if max_iterations > 0:
        return int(max_iterations)
    h = math.floor(math.log(1.0 - probability) / math.log(1.0 - inlier_ratio ** SAMPLE))
    return int(min(max(h, 1), MAX_ITERATIONS))


def normalise(xy, width, height):
    xy = np.asarray(xy, dtype=np.float64)
    return -2.0 * (xy[:, 0] / width - 0.5), -2.0 * (xy[:, 1] / height - 0.5)


def elimination_pivots(D):
    """|pivots| of Gaussian elimination with partial pivoting on the 3 x 3 D (zeros from the first zero pivot on)."""
    M = np.array(D, dtype=np.float64)
    piv = np.zeros(3)
    for k in range(3):
        r = k + int(np.argmax(np.abs(M[k:, k])))
        if M[r, k] == 0.0:
            break
        M[[k, r]] = M[[r, k]]
        piv[k] = abs(M[k, k])
        for i in range(k + 1, 3):
            M[i, k:] -= (M[i, k] / M[k, k]) * M[k, k:]
    return piv


def errors(a, c, b, d, X, u, v, width, height):
    return np.hypot(0.5 * width * (X @ a + c - u), 0.5 * height * (X @ b + d - v))


@dataclass
class Placement:
    status: int
    iterations: int = 0
    usable_models: int = 0
    supported_models: int = 0
    best_iteration: int = -1
    ransac_inliers: int = 0
    num_inliers: int = 0
    mean_error_px: float = 0.0
    refit_used: int = 0
    rotation: np.ndarray = None
    scale: float = 1.0
    offsets: np.ndarray = None
    inlier: np.ndarray = None
    detail: dict = None


def project(A):
    """Q = (A A^T)^(-1/2) A, the nearest matrix with orthonormal rows, and the singular values of A."""
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    return U @ Vt, s


def resect(points, xy, width, height, stream_id=0, seed=0, max_iterations=0, probability=0.999, inlier_ratio=0.5,
           min_consensus=8, max_error_px=3.0, min_pivot=None, min_axis_ratio=0.5, estimate_scale=0, scale=1.0, detail=False):
    X = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = X.shape[0]
    min_pivot = DEFAULT_MIN_PIVOT if min_pivot is None else min_pivot

    def empty(status, H=0):
        return Placement(status, iterations=H, rotation=np.eye(3), scale=scale, offsets=np.zeros(2), inlier=np.zeros(n, dtype=bool))

    if n < SAMPLE + min_consensus:
        return empty(STATUS_TOO_FEW)
    u, v = normalise(xy, width, height)
    H = num_iterations(max_iterations, probability, inlier_ratio)
    usable = supported = 0
    keys = []                                   # (-inliers, mean, iteration) of the supported hypotheses
    models = {}
    det = dict(thr_margin=np.inf, pivot_margin=np.inf, ratio_margin=np.inf, cond=0.0, unusable_pivot=0, unusable_ratio=0)
    for it in range(H):
        s = sample(seed, stream_id, it, n)
        D = X[s[1:]] - X[s[0]]
        big = np.abs(D).max()
        piv = elimination_pivots(D)
        if not big > 0.0:
            det["unusable_pivot"] += 1
            continue
        det["pivot_margin"] = min(det["pivot_margin"], abs(piv.min() / (min_pivot * big) - 1.0))
        if piv.min() < min_pivot * big:
            det["unusable_pivot"] += 1
            continue
        a = np.linalg.solve(D, u[s[1:]] - u[s[0]])
        b = np.linalg.solve(D, v[s[1:]] - v[s[0]])
        sv = np.linalg.svd(np.array([a, b]), compute_uv=False)
        det["ratio_margin"] = min(det["ratio_margin"], abs(sv[1] / sv[0] - min_axis_ratio))
        if sv[1] / sv[0] < min_axis_ratio:
            det["unusable_ratio"] += 1
            continue
        usable += 1
        det["cond"] = max(det["cond"], np.linalg.cond(D))
        c, d = u[s[0]] - a @ X[s[0]], v[s[0]] - b @ X[s[0]]
        e = errors(a, c, b, d, X, u, v, width, height)
        others = np.ones(n, dtype=bool)
        others[s] = False
        det["thr_margin"] = min(det["thr_margin"], np.abs(e[others] - max_error_px).min())
        inl = (e < max_error_px) | ~others
        cnt = int(inl.sum())
        if cnt - SAMPLE < min_consensus:
            continue
        supported += 1
        keys.append((-cnt, e[inl].sum() / cnt, it))
        models[it] = (a, c, b, d, inl)
    det.update(usable=usable, supported=supported)
    if not keys:
        out = empty(STATUS_NO_MODEL, H)
        out.usable_models, out.supported_models = usable, supported
        out.detail = det if detail else None
        return out
    keys.sort()
    # the margin of the selection: between the best two, equal inlier counts are split by the mean error
    det["select_margin"] = np.inf if len(keys) < 2 or keys[0][0] != keys[1][0] else keys[1][1] - keys[0][1]
    _, _, best = keys[0]
    a, c, b, d, inl = models[best]
    # the refit over the winner's inliers
    Xi, ui, vi = X[inl], u[inl], v[inl]
    m, um, vm = Xi.mean(0), ui.mean(), vi.mean()
    Xc = Xi - m
    cov = Xc.T @ Xc
    refit = 0
    A = np.array([a, b])
    try:
        L = np.linalg.cholesky(cov)
        pivots = np.diag(L) ** 2
    except np.linalg.LinAlgError:
        pivots = np.zeros(3)
    least = min_pivot * np.diag(cov).max()
    det["refit_pivot_margin"] = abs(pivots.min() / least - 1.0)
    det["refit_cond"] = np.linalg.cond(cov)
    if pivots.min() >= least:
        A = np.array([np.linalg.solve(cov, Xc.T @ (ui - um)), np.linalg.solve(cov, Xc.T @ (vi - vm))])
        refit = 1
    Q, sv = project(A)
    x, y = Q
    z = np.cross(x, y)
    s_out = 2.0 / (sv[0] + sv[1]) if estimate_scale else scale
    off = np.array([x @ m / s_out - um, y @ m / s_out - vm])
    e = errors(x / s_out, -off[0], y / s_out, -off[1], X, u, v, width, height)
    det["final_thr_margin"] = np.abs(e - max_error_px).min()
    fin = e < max_error_px
    cnt = int(fin.sum())
    return Placement(STATUS_OK, H, usable, supported, best, int(inl.sum()), cnt, e[fin].sum() / cnt if cnt else 0.0, refit,
                     np.column_stack([x, y, z]), s_out, off, fin, det if detail else None)


def rotation_error_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
