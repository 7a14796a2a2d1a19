"""The Tomasi-Kanade RANSAC initial alignment of a camera group, restated in numpy.

A float64 statement of INTEGRATION.md section 3 (robustlyEstimateTomasiKanadeFactorization,
src/algorithms/tomasi_kanade.cpp:193-370, with the eleven departures listed there), written from that
text and the reference -- not from the kernels -- with numpy.linalg.eigh / solve where the library
runs Jacobi sweeps and an elimination of its own.  tests/test_tk_cases_cpu.py shows on it that the
cases of tests/tk_cases.py are fit to judge a kernel; tests/test_tk_gpu.py holds osfm_tk_align and
osfm_tk_resolve_ambiguity to it.

`align(..., detail=True)` also returns what the CPU test bounds: per hypothesis the margins to every
threshold and the conditioning of the two eigen-problems, and the same for the factorisation of all
tracks where the fallback runs (detail["fallback"]).
"""
import math
from dataclasses import dataclass, field

import numpy as np

STATUS_RANSAC, STATUS_FALLBACK, STATUS_TOO_FEW, STATUS_DEGENERATE = 0, 1, 2, 3
M64 = (1 << 64) - 1
T_MIRROR = np.diag([1.0, 1.0, -1.0])


# ---- point 1: the counter-based generator of the library's RANSACs ----
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def ransac_rand(seed, group, it, draw):
    return splitmix64((splitmix64(seed ^ ((group * 0xD1342543DE82EF95) & M64)) + it * 0x2545F4914F6CDD1D + draw) & M64)


def sample(seed, group, it, n, size):
    """The first `size` distinct values of ransac_rand(...) % n, in draw order."""
    out, k = [], 0
    while len(out) < size:
        i = ransac_rand(seed, group, it, k) % n
        k += 1
        if i not in out:
            out.append(i)
    return out


MAX_ITERATIONS = 1 << 20


def num_iterations(max_iterations=0, probability=0.999, inlier_ratio=0.7, sample_size=10):
    """Point 11: the reference's formula (:212), held to 1 .. 2^20 hypotheses."""
    if max_iterations > 0:
        return int(max_iterations)
    h = math.floor(math.log(1.0 - probability) / math.log(1.0 - inlier_ratio ** sample_size))
    return int(min(max(h, 1), MAX_ITERATIONS))


def normalise(xy, width, height):
    """Point 3: the coordinates getPointOnCameraPlane uses."""
    xy = np.asarray(xy, dtype=np.float64)
    return np.stack([-2.0 * (xy[:, :, 0] / width - 0.5), -2.0 * (xy[:, :, 1] / height - 0.5)], axis=2)


@dataclass
class Model:
    ok: bool
    basis_1: np.ndarray = None          # (C, 3, 3) rotations, camera 0 the identity
    basis_2: np.ndarray = None          # the mirror solution T B T
    offsets: np.ndarray = None          # (C, 2)
    gram_w: np.ndarray = None           # eigenvalues of the Gram matrix, descending
    metric_w: np.ndarray = None         # eigenvalues of L, ascending


def _sym_row(u, v):
    return [u[0] * v[0], u[0] * v[1] + u[1] * v[0], u[0] * v[2] + u[2] * v[0],
            u[1] * v[1], u[1] * v[2] + u[2] * v[1], u[2] * v[2]]


def factorise(xn):
    """tomasiKanadeFactorization of the normalised coordinates xn (n, C, 2) of n tracks (points 2-5)."""
    n, C, _ = xn.shape
    D = np.concatenate([xn[:, :, 0].T, xn[:, :, 1].T], axis=0)          # 2C x n: x rows, then y rows
    mean = D.mean(axis=1)
    Dc = D - mean[:, None]
    w, U = np.linalg.eigh(Dc @ Dc.T)
    w, U = w[::-1], U[:, ::-1]
    if not w[2] > 1e-12 * w[0]:
        return Model(False, gram_w=w)
    U = U[:, :3]
    A, b = [], []
    for c in range(C):
        i, j = U[c], U[C + c]
        A += [_sym_row(i, i), _sym_row(j, j), _sym_row(i, j)]
        b += [1.0, 1.0, 0.0]
    A, b = np.array(A), np.array(b)
    try:
        l = np.linalg.solve(A.T @ A, A.T @ b)
    except np.linalg.LinAlgError:
        return Model(False, gram_w=w)
    L = np.array([[l[0], l[1], l[2]], [l[1], l[3], l[4]], [l[2], l[4], l[5]]])
    ev, V = np.linalg.eigh(L)
    if not ev[0] > 1e-9 * ev[2]:
        return Model(False, gram_w=w, metric_w=ev)
    R = U @ (V * np.sqrt(ev))
    Bs = []
    for c in range(C):
        x = R[c] / np.linalg.norm(R[c])
        y = R[C + c] - (R[C + c] @ x) * x
        y = y / np.linalg.norm(y)
        Bs.append(np.stack([x, y, np.cross(x, y)], axis=1))
    B1 = np.array([Bs[0].T @ B for B in Bs])
    B2 = np.array([T_MIRROR @ B @ T_MIRROR for B in B1])
    if B1[1][0, 2] < 0:
        B1, B2 = B2, B1
    return Model(True, B1, B2, np.stack([-mean[:C], -mean[C:]], axis=1), w, ev)


def phi_theta(B):
    """OrthographicCamera::basisToPhiThetaRho(B, true), its first two angles (OrthographicCamera.cpp:151-167)."""
    b = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]) @ B
    return (math.atan2(-b[1, 2], -b[0, 2]) - math.pi / 2,
            math.acos(b[2, 2] / np.linalg.norm(b[:, 2])) - math.pi / 2)


def usable(Bs):
    """isTomasiKanadeResultUsable (tomasi_kanade.cpp:446-470), and how close any quantity came to its 0.1."""
    ok, margin = True, np.inf
    for i in range(len(Bs)):
        for j in range(len(Bs)):
            if i == j:
                continue
            p1, t1 = phi_theta(Bs[i])
            p2, t2 = phi_theta(Bs[j])
            a, b = abs(p1 - p2), abs(t1 - t2)
            f = np.linalg.norm(Bs[i] - Bs[j])
            margin = min(margin, abs(a - 0.1), abs(b - 0.1), abs(f - 0.1))
            if (a < 0.1 and b < 0.1) or f < 0.1:
                ok = False
    return ok, margin


def reprojection_errors(Bs, off, xn, width, height):
    """Every track triangulated from all C rays (intersectRays), its reprojection error per camera in pixels."""
    n, C, _ = xn.shape
    Rm = np.zeros((3, 3))
    q = np.zeros((n, 3))
    for c, B in enumerate(Bs):
        P = np.eye(3) - np.outer(B[:, 2], B[:, 2])
        Rm += P
        o = -10.0 * B[:, 2][None] + (xn[:, c, 0] + off[c, 0])[:, None] * B[:, 0][None] \
            + (xn[:, c, 1] + off[c, 1])[:, None] * B[:, 1][None]
        q += o @ P.T
    p = np.linalg.solve(Rm, q.T).T
    err = np.zeros((n, C))
    for c, B in enumerate(Bs):
        loc = p @ B
        ex = (loc[:, 0] - off[c, 0] - xn[:, c, 0]) * width / 2.0
        ey = (loc[:, 1] - off[c, 1] - xn[:, c, 1]) * height / 2.0
        err[:, c] = np.sqrt(ex * ex + ey * ey)
    return err


@dataclass
class Result:
    status: int
    iterations: int = 0
    usable_models: int = 0
    supported_models: int = 0
    best_iteration: int = -1
    num_inliers: int = 0
    mean_error_px: float = 0.0
    basis_1: np.ndarray = None
    basis_2: np.ndarray = None
    offsets: np.ndarray = None
    inlier: np.ndarray = None
    detail: dict = field(default_factory=dict)


def _conditioning(d, m):
    """Folds the eigenvalues of one factorisation into the detail dictionary d.  A Gram matrix without a
    positive third eigenvalue has no finite w1 / w3 and no gap to speak of: its |w3| / w1 (0 for the zero
    matrix) goes to d["rank_ratio"], which the degenerate cases bound instead."""
    w = m.gram_w
    d["rank_ratio"].append(abs(w[2]) / w[0] if w[0] > 0 else 0.0)
    d["gram_cond"] = max(d["gram_cond"], w[0] / w[2] if w[2] > 0 else np.inf)
    if len(w) > 3 and w[0] > 0:
        d["gram_gap"] = min(d["gram_gap"], (w[2] - w[3]) / w[0])
    if m.metric_w is not None:
        d["metric_ratio"].append(m.metric_w[0] / m.metric_w[2])


def _new_detail():
    return {"threshold_margin": np.inf, "metric_ratio": [], "rank_ratio": [], "gram_cond": 0.0, "gram_gap": np.inf}


def align(xy, width, height, seed=0, group_id=0, sample_size=10, max_iterations=0, probability=0.999,
          inlier_ratio=0.7, min_consensus=25, max_error_px=3.0, detail=False):
    xy = np.asarray(xy, dtype=np.float64)
    N, C, _ = xy.shape
    ident = np.tile(np.eye(3), (C, 1, 1))
    res = Result(STATUS_TOO_FEW, basis_1=ident, basis_2=ident.copy(), offsets=np.zeros((C, 2)),
                 inlier=np.zeros(N, dtype=bool))
    if N < max(10, sample_size):                                        # point 9
        return res
    xn = normalise(xy, width, height)
    H = num_iterations(max_iterations, probability, inlier_ratio, sample_size)
    res.iterations = H
    d = dict(_new_detail(), usable_margin=np.inf, ranking=[], fallback=None)
    supported = []
    for it in range(H):
        s = sample(seed, group_id, it, N, sample_size)
        m = factorise(xn[s])
        if detail:
            _conditioning(d, m)
        if not m.ok:
            continue
        ok, margin = usable(m.basis_1)
        d["usable_margin"] = min(d["usable_margin"], margin)
        if not ok:
            continue
        res.usable_models += 1
        err = reprojection_errors(m.basis_1, m.offsets, xn, width, height)
        d["threshold_margin"] = min(d["threshold_margin"], np.abs(err - max_error_px).min())
        in_sample = np.zeros(N, dtype=bool)
        in_sample[s] = True
        consensus = ~in_sample & (err <= max_error_px).all(axis=1)              # point 6
        nc = int(consensus.sum())
        if nc >= min_consensus:
            members = consensus | in_sample
            mean = err[members].sum() / (int(members.sum()) * C)                # point 7
            # (detail) where in draw order the sample holds tracks that miss the bound under their own model
            misses = [k for k, t in enumerate(s) if not (err[t] <= max_error_px).all()]
            supported.append((-nc, mean, it, m, members, misses))
    res.supported_models = len(supported)
    if supported:
        supported.sort(key=lambda r: r[:3])
        nc, mean, it, m, members, d["winner_sample_misses"] = supported[0]
        res.status, res.best_iteration, res.num_inliers, res.mean_error_px = STATUS_RANSAC, it, int(members.sum()), mean
        res.basis_1, res.basis_2, res.offsets, res.inlier = m.basis_1, m.basis_2, m.offsets, members
        d["ranking"] = [(-r[0], r[1], r[2]) for r in supported[:2]]
    else:
        # point 9: the factorisation of all N given tracks; the tracks it reprojects within the bound are its inliers
        m = factorise(xn)
        d["fallback"] = _new_detail()
        _conditioning(d["fallback"], m)
        if not m.ok:
            res.status = STATUS_DEGENERATE
        else:
            err = reprojection_errors(m.basis_1, m.offsets, xn, width, height)
            d["fallback"]["threshold_margin"] = np.abs(err - max_error_px).min()
            members = (err <= max_error_px).all(axis=1)
            res.status, res.num_inliers = STATUS_FALLBACK, int(members.sum())
            res.mean_error_px = err[members].sum() / (res.num_inliers * C) if res.num_inliers else 0.0
            res.basis_1, res.basis_2, res.offsets, res.inlier = m.basis_1, m.basis_2, m.offsets, members
    if detail:
        res.detail = d
    return res


def resolve_ambiguity(basis_1, basis_2, global_rotation, has_global):
    """Point 10.  global_rotation: (C, 3, 3) local -> world of the views that have a global camera.
    Returns 1 or 2."""
    shared = [c for c in range(len(has_global)) if has_global[c]]
    if len(shared) < 2:
        return 1
    a, b = shared[0], shared[1]

    def look_difference(Ra, Rb):
        Rb_in_a = Ra.T @ Rb                           # a canonical: its z is (0, 0, 1)
        return np.array([0.0, 0.0, 1.0]) - Rb_in_a[:, 2]

    g = look_difference(np.asarray(global_rotation[a]), np.asarray(global_rotation[b]))
    s1 = g @ look_difference(basis_1[a], basis_1[b])
    s2 = g @ look_difference(basis_2[a], basis_2[b])
    return 2 if s2 > s1 else 1


def rotation_error_deg(A, B):
    return float(np.degrees(np.arccos(np.clip((np.trace(A.T @ B) - 1.0) / 2.0, -1.0, 1.0))))
