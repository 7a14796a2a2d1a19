"""The definition of the observation refinement (include/osfm_hip.h, "Sub-pixel refinement"; DESIGN.md "Observation
refinement") in float64 numpy.  The kernels of orthosfm_amd/csrc/refine_kernels.hip are held to it.

The first alive observation of a track is its reference.  T(u) = I_ref(p_ref + step u), u integer in [-R, R]^2 in
row-major order (k = (uy + R) (2 R + 1) + ux + R), is the template of every other alive observation, each refined on
its own by Gauss-Newton on T(u) ~ g I_t(p + A step u) + b over b, g, p (2) and A (4).

The statuses are tested in the order of the table in the header at every point where a test can be made, and the
first test that fails, in time, decides: the template window and the first target window (OUTSIDE), the template's
contrast (FLAT), then per iteration the window (OUTSIDE) and the pivots (ILL_CONDITIONED); behind the loop the final
window (OUTSIDE), NOT_CONVERGED, and the three rejections.

Sums follow the kernel's order -- 64 partial sums over k = l, l + 64, ..., folded 32, 16, ..., 1 -- so that the two
differ by what a compiler may still do differently, not by the order of a sum.

`plant`: one of the deliberate errors tests/test_refine_cases_cpu.py uses to show that its bounds see them.
"""
import numpy as np

UNTESTED, REFERENCE, REFINED, OUTSIDE, FLAT, ILL_CONDITIONED, NOT_CONVERGED, REJECT_SHIFT, REJECT_DEFORM, REJECT_SCORE = range(10)
STATUS_NAMES = ("UNTESTED", "REFERENCE", "REFINED", "OUTSIDE", "FLAT", "ILL_CONDITIONED", "NOT_CONVERGED", "REJECT_SHIFT",
                "REJECT_DEFORM", "REJECT_SCORE")
# min_pivot: see refine_cases.PIVOT
DEFAULTS = dict(radius=7, max_iterations=10, step=1.0, eps=1e-3, min_contrast=2.0, max_shift=3.0, max_deform=2.0,
                min_score=0.9, min_pivot=0.034)
PLANTS = (None, "grad_sign", "no_gain", "half_pixel")


def grey(image):
    """float32 [h, w]: the byte, or (float32)(r + g + b) / 3.0f."""
    im = np.asarray(image)
    assert im.dtype == np.uint8
    if im.ndim == 2:
        return im.astype(np.float32)
    return im.astype(np.int32).sum(axis=2).astype(np.float32) / np.float32(3.0)


def wave_sum(v):
    """Sum over axis 0 (the samples in order k) as a wave adds: lane partials, then the fold."""
    v = np.asarray(v, dtype=np.float64)
    pad = (-v.shape[0]) % 64
    if pad:
        v = np.concatenate([v, np.zeros((pad,) + v.shape[1:])])
    rounds = v.reshape((-1, 64) + v.shape[1:])
    acc = rounds[0].copy()
    for r in rounds[1:]:
        acc = acc + r
    m = 32
    while m >= 1:
        acc = acc[:m] + acc[m:2 * m]
        m //= 2
    return acc[0]


def slack(x, y, w, h):
    """Per sample: the distance to the nearest bound of [0, w - 1] x [0, h - 1], negative outside (NaN: -inf)."""
    s = np.minimum(np.minimum(x, (w - 1.0) - x), np.minimum(y, (h - 1.0) - y))
    return np.where(np.isnan(s), -np.inf, s)


def bilinear(img, x, y):
    """Value and derivative of the bilinear interpolant at points inside the image; a point on the last column (row)
    is interpolated in the cell to its left (above) with weight 1."""
    h, w = img.shape
    x0 = np.minimum(np.floor(x).astype(np.int64), max(w - 2, 0))
    y0 = np.minimum(np.floor(y).astype(np.int64), max(h - 2, 0))
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = x - x0, y - y0
    i00, i01 = img[y0, x0].astype(np.float64), img[y0, x1].astype(np.float64)
    i10, i11 = img[y1, x0].astype(np.float64), img[y1, x1].astype(np.float64)
    top, bot = (1.0 - fx) * i00 + fx * i01, (1.0 - fx) * i10 + fx * i11
    v = (1.0 - fy) * top + fy * bot
    gx = (1.0 - fy) * (i01 - i00) + fy * (i11 - i10)
    gy = (1.0 - fx) * (i10 - i00) + fx * (i11 - i01)
    return v, gx, gy


def solve_step(H, rhs, min_pivot):
    """(delta or None, smallest pivot): Cholesky of D H D with D = diag(H)^-1/2."""
    n = H.shape[0]
    diag = np.diag(H)
    if not np.all(diag > 0.0):
        return None, 0.0
    d = 1.0 / np.sqrt(diag)
    L = np.zeros((n, n))
    pivot_min = np.inf
    ok = True
    for j in range(n):
        s = (H[j, j] * d[j]) * d[j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        pivot_min = min(pivot_min, s) if not np.isnan(s) else -np.inf
        if not s >= min_pivot:
            ok = False
            if not s > 0.0:
                return None, pivot_min
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            t = (H[i, j] * d[i]) * d[j]
            for k in range(j):
                t = t - L[i, k] * L[j, k]
            L[i, j] = t / L[j, j]
    if not ok:
        return None, pivot_min
    y = np.zeros(n)
    for i in range(n):
        t = rhs[i] * d[i]
        for k in range(i):
            t = t - L[i, k] * y[k]
        y[i] = t / L[i, i]
    z = np.zeros(n)
    for i in range(n - 1, -1, -1):
        t = y[i]
        for k in range(i + 1, n):
            t = t - L[k, i] * z[k]
        z[i] = t / L[i, i]
    return z * d, pivot_min


def singular_values(M):
    E, F = 0.5 * (M[0, 0] + M[1, 1]), 0.5 * (M[0, 0] - M[1, 1])
    G, H = 0.5 * (M[1, 0] + M[0, 1]), 0.5 * (M[1, 0] - M[0, 1])
    Q, S = np.sqrt(E * E + H * H), np.sqrt(F * F + G * G)
    return Q + S, abs(Q - S)


def _rel(q, thr):
    return abs(q - thr) / abs(thr) if thr != 0 else abs(q)


def refine_one(ir, it, p_ref, p0, A0, o, plant=None):
    """One observation against its reference.  Returns a dict: status, xy, affine, score, iterations, margin (the
    smallest relative distance to its threshold of any test on the way: a result whose margin is below the band could
    have gone the other way in another arithmetic), pivot_min (over the iterations; inf before the first)."""
    R, step = int(o["radius"]), float(o["step"])
    side = 2 * R + 1
    k = np.arange(side * side)
    sx, sy = step * (k % side - R).astype(np.float64), step * (k // side - R).astype(np.float64)
    N = float(side * side)
    p0 = np.asarray(p0, dtype=np.float64)
    A0 = np.asarray(A0, dtype=np.float64).reshape(2, 2)
    res = dict(status=None, xy=p0.copy(), affine=A0.reshape(4).copy(), score=0.0, iterations=0, margin=np.inf, pivot_min=np.inf)
    shift = 0.5 if plant == "half_pixel" else 0.0

    def done(status):
        res["status"] = status
        return res

    def window(img, x, y):
        """True when outside; books the margin (in pixels) either way."""
        s = slack(x, y, img.shape[1], img.shape[0])
        bad = s < 0.0
        # a sample at integer coordinates exactly on a bound is legal by definition and exact in any arithmetic
        # (the sums that led to it have integer terms): it does not make the decision a close one
        close = np.abs(s[~((s == 0.0) & (x == np.floor(x)) & (y == np.floor(y)))])
        if bad.any():
            res["margin"] = min(res["margin"], float(-s.min()))
        elif close.size:
            res["margin"] = min(res["margin"], float(close.min()))
        return bool(bad.any())

    def warp(p, A):
        return p[0] + (A[0, 0] * sx + A[0, 1] * sy), p[1] + (A[1, 0] * sx + A[1, 1] * sy)

    x, y = p_ref[0] + sx, p_ref[1] + sy
    if window(ir, x, y):
        return done(OUTSIDE)
    T = bilinear(ir, x, y)[0]
    mean_t = wave_sum(T) / N
    ct = T - mean_t
    ss_t = wave_sum(ct * ct)
    if window(it, *warp(p0, A0)):
        return done(OUTSIDE)
    std = np.sqrt(ss_t / N)
    res["margin"] = min(res["margin"], _rel(std, o["min_contrast"]))
    if std < o["min_contrast"]:
        return done(FLAT)

    # The parameters in the order of the elimination: bias, gain, px, py, a00, a01, a10, a11.  The gain multiplies
    # I - mean(T) and the bias starts at mean(T): the model g I + b in other coordinates (Gauss-Newton's steps do not
    # depend on a linear change of the parameters), chosen so that the pivots of the six geometric parameters are what
    # is left of them once brightness and contrast are accounted for.
    p, A, gain, bias = p0.copy(), A0.copy(), 1.0, mean_t
    converged = False
    idx_a, idx_b = np.triu_indices(8)
    for iteration in range(int(o["max_iterations"])):
        x, y = warp(p, A)
        if window(it, x, y):
            return done(OUTSIDE)
        v, gx, gy = bilinear(it, x + shift, y + shift)
        if plant == "grad_sign":
            gx, gy = -gx, -gy
        centred = v - mean_t
        r = T - (gain * centred + bias)
        j0, j1 = gain * gx, gain * gy
        J = np.stack([np.ones_like(v), centred, j0, j1, j0 * sx, j0 * sy, j1 * sx, j1 * sy], axis=1)
        sums = wave_sum(np.concatenate([J[:, idx_a] * J[:, idx_b], J * r[:, None], (r * r)[:, None]], axis=1))
        H = np.zeros((8, 8))
        H[idx_a, idx_b] = sums[:36]
        H[idx_b, idx_a] = sums[:36]
        rhs = sums[36:44].copy()
        if plant == "no_gain":
            H[1, :] = 0.0
            H[:, 1] = 0.0
            H[1, 1] = 1.0
            rhs[1] = 0.0
        delta, pivot = solve_step(H, rhs, o["min_pivot"])
        res["pivot_min"] = min(res["pivot_min"], pivot)
        res["margin"] = min(res["margin"], _rel(pivot, o["min_pivot"]))
        if delta is None:
            return done(ILL_CONDITIONED)
        bias, gain = bias + delta[0], gain + delta[1]
        p = p + delta[2:4]
        A = A + delta[4:8].reshape(2, 2)
        res["iterations"] = iteration + 1
        dp = np.sqrt(delta[2] * delta[2] + delta[3] * delta[3])
        res["margin"] = min(res["margin"], _rel(dp, o["eps"]))
        if dp < o["eps"]:
            converged = True
            break
    x, y = warp(p, A)
    if window(it, x, y):
        return done(OUTSIDE)
    Jv = bilinear(it, x + shift, y + shift)[0]
    mean_j = wave_sum(Jv) / N
    cj = Jv - mean_j
    c = wave_sum(np.stack([ct * cj, cj * cj], axis=1))
    den = np.sqrt(ss_t * c[1])
    res["score"] = float(c[0] / den) if den > 0.0 else 0.0
    if not converged:
        return done(NOT_CONVERGED)
    d = p - p0
    moved = np.sqrt(d[0] * d[0] + d[1] * d[1])
    res["margin"] = min(res["margin"], _rel(moved, o["max_shift"]))
    if moved > o["max_shift"]:
        return done(REJECT_SHIFT)
    det0 = A0[0, 0] * A0[1, 1] - A0[0, 1] * A0[1, 0]
    inv0 = np.array([[A0[1, 1] / det0, -A0[0, 1] / det0], [-A0[1, 0] / det0, A0[0, 0] / det0]])
    M = np.array([[A[0, 0] * inv0[0, 0] + A[0, 1] * inv0[1, 0], A[0, 0] * inv0[0, 1] + A[0, 1] * inv0[1, 1]],
                  [A[1, 0] * inv0[0, 0] + A[1, 1] * inv0[1, 0], A[1, 0] * inv0[0, 1] + A[1, 1] * inv0[1, 1]]])
    smax, smin = singular_values(M)
    res["margin"] = min(res["margin"], _rel(smax, o["max_deform"]), _rel(smin, 1.0 / o["max_deform"]))
    if smax > o["max_deform"] or smin < 1.0 / o["max_deform"]:
        return done(REJECT_DEFORM)
    res["margin"] = min(res["margin"], _rel(res["score"], o["min_score"]))
    if res["score"] < o["min_score"]:
        return done(REJECT_SCORE)
    res["xy"], res["affine"] = p, A.reshape(4).copy()
    return done(REFINED)


def refine_tracks(images, offsets, view, xy, alive=None, init_affine=None, plant=None, **options):
    """images: uint8 arrays per view (None: no image).  Returns a dict of arrays over the observations: status, xy,
    affine, score, iterations, margin, pivot_min."""
    o = dict(DEFAULTS)
    for key, val in options.items():
        if key not in o:
            raise TypeError(f"refine_tracks: no option {key!r}")
        o[key] = val
    offsets = np.asarray(offsets, dtype=np.int64)
    F = int(offsets[-1]) if offsets.size else 0
    view = np.asarray(view, dtype=np.int32).reshape(F)
    xy = np.asarray(xy, dtype=np.float64).reshape(F, 2)
    alive = np.ones(F, bool) if alive is None else np.asarray(alive).astype(bool).reshape(F)
    A0 = np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (F, 1)) if init_affine is None else np.asarray(init_affine, np.float64).reshape(F, 4)
    greys = {}
    out = dict(status=np.zeros(F, np.int32), xy=xy.copy(), affine=A0.copy(), score=np.zeros(F), iterations=np.zeros(F, np.int32),
               margin=np.full(F, np.inf), pivot_min=np.full(F, np.inf))

    def image_of(v):
        if v not in greys:
            greys[v] = grey(images[v])
        return greys[v]

    for t in range(offsets.shape[0] - 1):
        obs = np.arange(offsets[t], offsets[t + 1])
        live = obs[alive[obs]]
        if live.size < 2:
            continue                       # UNTESTED
        ref = int(live[0])
        out["status"][ref] = REFERENCE
        for f in live[1:]:
            r = refine_one(image_of(int(view[ref])), image_of(int(view[f])), xy[ref], xy[f], A0[f], o, plant)
            for key in out:
                out[key][f] = r[key]
    return out
