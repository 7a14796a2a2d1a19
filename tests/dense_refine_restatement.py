"""The definition of the depth-map refinement (include/osfm_hip.h, "Slanted-plane refinement"; DESIGN.md "3z-c") in
float64 numpy.  The kernel of orthosfm_amd/csrc/dense_refine_kernels.hip is held to it.

A reference pixel x with sweep depth z0 gets the local depth model z(x + u) = z + p . u, p = (zx, zy) in depth per
reference pixel.  With G, g, e of dense_restatement.Geometry.pair its window lands in source s at

    c + M u,   c = G x + g + z e,   M = G + e p^T

(one affine map per pixel and source, exact for a planar patch).  T(u) = I_r(x + u), u integer in [-R, R]^2 in row-major
order (k = (uy + R) (2 R + 1) + ux + R), are grey values, float32 as stored; everything after them is double.  The
residual of source s is rho_s(u) = g_s W_s(u) + b_s - T(u) with W_s the bilinear sample of I_s at c + M u; Gauss-Newton
runs over the shared (z, zx, zy) and a gain and bias per source.  d rho / d (z, zx, zy) = g_s a (1, ux, uy) with
a = grad I_s . e, the derivative along the epipolar line.

Which sources count is frozen at the start: a source counts when every sample of its window at (z0, p = 0) is inside its
image.  Fewer than min_sources of them: OUTSIDE.  A frozen source that has a sample outside at any later evaluation:
OUTSIDE.

One evaluation of a source is one pass over the window for eighteen sums that do not depend on gain and bias
(`source_sums`); everything else is closed form on them (`normal_equations`), in the order written there: the 5 x 5
normal equations of (g a m, W, 1), m = (1, ux, uy), the elimination of the 2 x 2 block of gain and bias, the 3 x 3
remainder.  The remainders are added over the counting sources in ascending order of the `sources` argument and solved
by the scaled Cholesky of refine_restatement.solve_step (`solve3` is the same operations on arrays, and
test_dense_refine_cases_cpu.py holds the two together to the bit).  Gain and bias start as the least-squares fit of W to
T at the start and follow each step by back-substitution.

Statuses; the first test to fail, in time, decides.  Within one evaluation the order is: a sample outside (OUTSIDE),
the count (OUTSIDE), a source whose gain/bias block is singular (ILL_CONDITIONED), the pivots (ILL_CONDITIONED).
Behind the loop: the final windows (OUTSIDE), NOT_CONVERGED, REJECT_SHIFT, REJECT_SLOPE, REJECT_SCORE.

Sums follow the kernel's order: 16 lane partials over k = l, l + 16, ..., folded 8, 4, 2, 1 (`lane_sum`, the 16-lane
form of refine_restatement.wave_sum).

The normal of a REFINED pixel is cross(b1 + zy d, b0 + zx d) normalised (b0, b1 the columns of B_r): the negative of
cross(b0 + zx d, b1 + zy d).  mesh_restatement.vertex_normals sums cross(b - a, c - a) over MVE's triangles, whose first
is (x, y), (x, y + 1), (x + 1, y): cross(dY, dX).  Since cross(b0, b1) is a positive multiple of d, that normal has
n . d < 0 -- it points against the viewing axis, towards the camera -- and so has this one.

`plant`: one of the deliberate errors test_dense_refine_cases_cpu.py uses to show that its bounds see them.
"""
import numpy as np

import dense_restatement as dr
import refine_restatement as rr

NOT_OK, REFINED, OUTSIDE, ILL_CONDITIONED, NOT_CONVERGED, REJECT_SHIFT, REJECT_SLOPE, REJECT_SCORE = range(8)
STATUS_NAMES = ("NOT_OK", "REFINED", "OUTSIDE", "ILL_CONDITIONED", "NOT_CONVERGED", "REJECT_SHIFT", "REJECT_SLOPE", "REJECT_SCORE")
# radius: the sweep's; min_pivot: see dense_refine_cases.PIVOT
DEFAULTS = dict(radius=3, min_sources=2, max_iterations=10, eps=1e-3, max_shift=1.5, max_deform=2.0, min_score=0.8, min_pivot=0.035)
PLANTS = (None, "grad_sign", "no_gain", "no_tilt", "flat_normal")
BLOCK_EPS = 1e-12        # the gain/bias block is singular when its determinant is not above this share of its diagonal's product


def lane_sum(v):
    """Sum over axis 0 (the samples in order k) as 16 lanes add: lane partials, then the fold 8, 4, 2, 1."""
    v = np.asarray(v, dtype=np.float64)
    pad = (-v.shape[0]) % 16
    if pad:
        v = np.concatenate([v, np.zeros((pad,) + v.shape[1:])])
    rounds = v.reshape((-1, 16) + v.shape[1:])
    acc = rounds[0].copy()
    for r in rounds[1:]:
        acc = acc + r
    m = 8
    while m >= 1:
        acc = acc[:m] + acc[m:2 * m]
        m //= 2
    return acc[0]


def solve3(H, rhs, min_pivot):
    """refine_restatement.solve_step for n = 3 on arrays: H[i][j], rhs[i] are arrays over the pixels.  Returns
    (delta [3], ok, smallest pivot); where ok is False delta means nothing."""
    n = 3
    with np.errstate(all="ignore"):
        pos = (H[0][0] > 0.0) & (H[1][1] > 0.0) & (H[2][2] > 0.0)
        d = [1.0 / np.sqrt(H[i][i]) for i in range(n)]
        L = [[None] * n for _ in range(n)]
        pivot_min = np.full(np.shape(H[0][0]), np.inf)
        ok = pos.copy()
        for j in range(n):
            s = (H[j][j] * d[j]) * d[j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            pivot_min = np.where(np.isnan(s), -np.inf, np.minimum(pivot_min, s))
            ok &= s >= min_pivot
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, n):
                t = (H[i][j] * d[i]) * d[j]
                for k in range(j):
                    t = t - L[i][k] * L[j][k]
                L[i][j] = t / L[j][j]
        y = [None] * n
        for i in range(n):
            t = rhs[i] * d[i]
            for k in range(i):
                t = t - L[i][k] * y[k]
            y[i] = t / L[i][i]
        z = [None] * n
        for i in range(n - 1, -1, -1):
            t = y[i]
            for k in range(i + 1, n):
                t = t - L[k][i] * z[k]
            z[i] = t / L[i][i]
        delta = [z[i] * d[i] for i in range(n)]
    pivot_min = np.where(pos, pivot_min, 0.0)
    return delta, ok, pivot_min


def source_sums(img, pair, xs, ys, z, zx, zy, T, ux, uy, plant=None):
    """One evaluation of a source for the pixels (xs, ys) [P]: (sums dict of [P] arrays, inside [P], slack [P]).
    T [N, P]; ux, uy [N, 1]."""
    G, g, e = pair
    h, w = img.shape
    m00, m01 = G[0][0] + e[0] * zx, G[0][1] + e[0] * zy
    m10, m11 = G[1][0] + e[1] * zx, G[1][1] + e[1] * zy
    cx = (G[0][0] * xs + G[0][1] * ys) + (g[0] + z * e[0])
    cy = (G[1][0] * xs + G[1][1] * ys) + (g[1] + z * e[1])
    sx = cx + (m00 * ux + m01 * uy)
    sy = cy + (m10 * ux + m11 * uy)
    sl = rr.slack(sx, sy, w, h)
    ins = sl >= 0.0
    exact = (sl == 0.0) & (sx == np.floor(sx)) & (sy == np.floor(sy))       # legal by definition, exact in any arithmetic
    slack = np.where(exact, np.inf, np.abs(sl)).min(axis=0)
    inside = ins.all(axis=0)
    W, gx, gy = rr.bilinear(img, np.where(ins, sx, 0.0), np.where(ins, sy, 0.0))
    a = gx * e[0] + gy * e[1]
    if plant == "grad_sign":
        a = -a
    am = (a, a * ux, a * uy)
    S = dict(sW=lane_sum(W), sWW=lane_sum(W * W), sWT=lane_sum(W * T))
    for i in range(3):
        for k in range(i, 3):
            S[f"A{i}{k}"] = lane_sum(am[i] * am[k])
        S[f"P{i}"] = lane_sum(am[i] * W)
        S[f"Q{i}"] = lane_sum(am[i])
        S[f"U{i}"] = lane_sum(am[i] * T)
    return S, inside, slack


def block(S, N):
    """(det, ok) of the gain/bias block [[sWW, sW], [sW, N]]."""
    det = S["sWW"] * N - S["sW"] * S["sW"]
    return det, det > BLOCK_EPS * (S["sWW"] * N)


def fit(S, det, N, sT):
    """Gain and bias of the least-squares fit of W to T."""
    return (S["sWT"] * N - S["sW"] * sT) / det, (S["sWW"] * sT - S["sW"] * S["sWT"]) / det


def zncc(S, N, sT, sTT):
    cov = S["sWT"] - S["sW"] * sT / N
    var_w = S["sWW"] - S["sW"] * S["sW"] / N
    var_t = sTT - sT * sT / N
    den = np.sqrt(var_t * var_w)
    return np.where(den > 0.0, cov / np.where(den > 0.0, den, 1.0), 0.0)


def normal_equations(S, det, N, sT, gain, bias):
    """What is left of a source's 5 x 5 normal equations once gain and bias are eliminated: (H [3][3] upper, r [3]) and
    what the back-substitution needs (D [3][2], rc [2])."""
    D = [(gain * S[f"P{i}"], gain * S[f"Q{i}"]) for i in range(3)]
    rc = ((gain * S["sWW"] + bias * S["sW"]) - S["sWT"], (gain * S["sW"] + bias * N) - sT)
    E = [((D[i][0] * N - D[i][1] * S["sW"]) / det, (D[i][1] * S["sWW"] - D[i][0] * S["sW"]) / det) for i in range(3)]
    gg = gain * gain
    H = [[None] * 3 for _ in range(3)]
    r = [None] * 3
    for i in range(3):
        for k in range(i, 3):
            H[i][k] = gg * S[f"A{i}{k}"] - (E[i][0] * D[k][0] + E[i][1] * D[k][1])
        r[i] = gain * ((gain * S[f"P{i}"] + bias * S[f"Q{i}"]) - S[f"U{i}"]) - (E[i][0] * rc[0] + E[i][1] * rc[1])
    return H, r, D, rc


def back_substitute(S, det, N, D, rc, delta):
    """The step of gain and bias that goes with delta."""
    t0 = rc[0] + ((D[0][0] * delta[0] + D[1][0] * delta[1]) + D[2][0] * delta[2])
    t1 = rc[1] + ((D[0][1] * delta[0] + D[1][1] * delta[1]) + D[2][1] * delta[2])
    return -((N * t0 - S["sW"] * t1) / det), -((S["sWW"] * t1 - S["sW"] * t0) / det)


def normal(geo, zx, zy, plant=None):
    """cross(b1 + zy d, b0 + zx d) normalised, per pixel: [P, 3]."""
    if plant == "flat_normal":
        zx, zy = np.zeros_like(zx), np.zeros_like(zy)
    u = [geo.B[j][0] + zx * geo.d[j] for j in range(3)]
    v = [geo.B[j][1] + zy * geo.d[j] for j in range(3)]
    c = (v[1] * u[2] - v[2] * u[1], v[2] * u[0] - v[0] * u[2], v[0] * u[1] - v[1] * u[0])
    nn = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    return np.stack([c[0] / nn, c[1] / nn, c[2] / nn], axis=-1)


def _rel(q, thr):
    return np.abs(q - thr) / abs(thr) if thr != 0 else np.abs(q)


def refine(images, P, ref, sources, depth, status, dz, score=None, plant=None, rect=None, **options):
    """The refinement of view `ref`'s map (depth, status as dense_restatement.sweep returns them; dz the view's step)
    against `sources`.  rect = (x0, y0, x1, y1): only the pixels x0 <= x < x1, y0 <= y < y1 are processed (the others
    come out NOT_OK) -- a pixel's result does not depend on it.  Returns a dict of planes: depth (refined where the
    status is REFINED, the input elsewhere), gradient [h, w, 2] and normal [h, w, 3] (NaN where not REFINED), score
    (float32: the mean correlation at the end where REFINED, the input elsewhere), status (uint8), iterations (int32),
    margin, pivot_min, score0 and score1 (the mean correlation at the start and at the end, NaN where not reached)."""
    o = dict(DEFAULTS)
    for key, val in options.items():
        if key not in o:
            raise TypeError(f"refine: no option {key!r}")
        o[key] = val
    R = int(o["radius"])
    side = 2 * R + 1
    N = float(side * side)
    k = np.arange(side * side)
    ux, uy = (k % side - R).astype(np.float64)[:, None], (k // side - R).astype(np.float64)[:, None]
    iux, iuy = (k % side - R)[:, None], (k // side - R)[:, None]
    gr = dr.Geometry(P[ref])
    pairs = [gr.pair(dr.Geometry(P[s])) for s in sources]
    imgs = [dr.grey(images[s]) for s in sources]
    img_r = dr.grey(images[ref])
    h, w = img_r.shape
    depth0 = np.asarray(depth, dtype=np.float64)
    status0 = np.asarray(status)
    out = dict(depth=depth0.copy(), gradient=np.full((h, w, 2), np.nan), normal=np.full((h, w, 3), np.nan),
               score=(np.zeros((h, w), np.float32) if score is None else np.asarray(score, np.float32).copy()),
               status=np.full((h, w), NOT_OK, np.uint8), iterations=np.zeros((h, w), np.int32), margin=np.full((h, w), np.inf),
               pivot_min=np.full((h, w), np.inf), score0=np.full((h, w), np.nan), score1=np.full((h, w), np.nan))
    sel = status0 == dr.OK
    if rect is not None:
        inr = np.zeros((h, w), bool)
        inr[rect[1]:rect[3], rect[0]:rect[2]] = True
        sel &= inr
    py, px = np.nonzero(sel)
    n = px.shape[0]
    if n == 0:
        return out
    st = np.full(n, -1, np.int64)                      # -1: still running
    margin = np.full(n, np.inf)
    pivot_min = np.full(n, np.inf)
    iterations = np.zeros(n, np.int64)
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    z0 = depth0[py, px].copy()
    z, zx, zy = z0.copy(), np.zeros(n), np.zeros(n)
    ns = len(sources)
    gain, bias = np.ones((ns, n)), np.zeros((ns, n))
    frozen = np.zeros((ns, n), bool)
    score0, score1 = np.full(n, np.nan), np.full(n, np.nan)
    converged = np.zeros(n, bool)

    def settle(idx, which, code):
        """The running pixels idx[which] end with `code`."""
        hit = idx[which]
        hit = hit[st[hit] < 0]
        st[hit] = code

    with np.errstate(all="ignore"):
        # the template: its window inside the reference image, its sums
        tx, ty = px[None, :] + iux, py[None, :] + iuy
        t_in = ((tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)).all(axis=0)
        T_all = img_r[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)].astype(np.float64)
        sT_all, sTT_all = lane_sum(T_all), lane_sum(T_all * T_all)
        st[~t_in] = OUTSIDE
        thr = float(o["eps"]) * float(dz)
        for it in range(int(o["max_iterations"])):
            idx = np.nonzero((st < 0) & ~converged)[0]
            if idx.size == 0:
                break
            T, sT, sTT = T_all[:, idx], sT_all[idx], sTT_all[idx]
            Ht = [[np.zeros(idx.size) for _ in range(3)] for _ in range(3)]
            rt = [np.zeros(idx.size) for _ in range(3)]
            outside, ill = np.zeros(idx.size, bool), np.zeros(idx.size, bool)
            count, total = np.zeros(idx.size, np.int64), np.zeros(idx.size)
            kept = []
            for s in range(ns):
                S, inside, slack = source_sums(imgs[s], pairs[s], xs[idx], ys[idx], z[idx], zx[idx], zy[idx], T, ux, uy, plant)
                if it == 0:
                    frozen[s, idx] = inside
                    margin[idx] = np.minimum(margin[idx], slack)
                    counts = inside
                else:
                    counts = frozen[s, idx]
                    margin[idx] = np.minimum(margin[idx], np.where(counts, slack, np.inf))
                    outside |= counts & ~inside
                det, ok = block(S, N)
                margin[idx] = np.minimum(margin[idx], np.where(counts & inside, np.abs(det / (S["sWW"] * N) - BLOCK_EPS), np.inf))
                ill |= counts & ~ok
                if it == 0:
                    gn, bs = fit(S, det, N, sT)
                    if plant == "no_gain":
                        gn, bs = np.ones_like(gn), np.zeros_like(bs)
                    gain[s, idx], bias[s, idx] = gn, bs
                    total = total + np.where(counts, zncc(S, N, sT, sTT), 0.0)
                H, r, D, rc = normal_equations(S, det, N, sT, gain[s, idx], bias[s, idx])
                for i in range(3):
                    for kk in range(i, 3):
                        Ht[i][kk] = Ht[i][kk] + np.where(counts, H[i][kk], 0.0)
                    rt[i] = rt[i] + np.where(counts, r[i], 0.0)
                count += counts
                kept.append((S, det, D, rc, counts))
            few = count < int(o["min_sources"])
            settle(idx, outside | few, OUTSIDE)
            settle(idx, ill, ILL_CONDITIONED)
            if it == 0:
                score0[idx] = total / np.maximum(count, 1)
            for i in range(3):
                for kk in range(i):
                    Ht[i][kk] = Ht[kk][i]
            if plant == "no_tilt":
                for i in (1, 2):
                    for kk in range(3):
                        Ht[i][kk] = np.zeros(idx.size)
                        Ht[kk][i] = np.zeros(idx.size)
                    Ht[i][i] = np.ones(idx.size)
                    rt[i] = np.zeros(idx.size)
            delta, ok, pivot = solve3(Ht, [-rt[0], -rt[1], -rt[2]], float(o["min_pivot"]))
            run = st[idx] < 0
            pivot_min[idx] = np.where(run, np.minimum(pivot_min[idx], pivot), pivot_min[idx])
            margin[idx] = np.where(run, np.minimum(margin[idx], _rel(pivot, float(o["min_pivot"]))), margin[idx])
            settle(idx, ~ok, ILL_CONDITIONED)
            run = st[idx] < 0
            go = idx[run]
            z[go], zx[go], zy[go] = z[go] + delta[0][run], zx[go] + delta[1][run], zy[go] + delta[2][run]
            for s, (S, det, D, rc, counts) in enumerate(kept):
                if plant == "no_gain":
                    continue
                dg, db = back_substitute(S, det, N, D, rc, delta)
                upd = run & counts
                gain[s, idx[upd]] += dg[upd]
                bias[s, idx[upd]] += db[upd]
            iterations[go] = it + 1
            c0 = np.abs(delta[0])
            c1 = float(R) * (np.abs(delta[1]) + np.abs(delta[2]))
            margin[go] = np.minimum(margin[go], np.minimum(_rel(c0, thr), _rel(c1, thr))[run])
            converged[go] = ((c0 <= thr) & (c1 <= thr))[run]

        # behind the loop: the final windows and their scores
        idx = np.nonzero(st < 0)[0]
        if idx.size:
            T, sT, sTT = T_all[:, idx], sT_all[idx], sTT_all[idx]
            outside = np.zeros(idx.size, bool)
            count, total = np.zeros(idx.size, np.int64), np.zeros(idx.size)
            for s in range(ns):
                S, inside, slack = source_sums(imgs[s], pairs[s], xs[idx], ys[idx], z[idx], zx[idx], zy[idx], T, ux, uy, plant)
                counts = frozen[s, idx]
                margin[idx] = np.minimum(margin[idx], np.where(counts, slack, np.inf))
                outside |= counts & ~inside
                total = total + np.where(counts, zncc(S, N, sT, sTT), 0.0)
                count += counts
            score1[idx] = total / np.maximum(count, 1)
            settle(idx, outside, OUTSIDE)
            settle(idx, ~converged[idx], NOT_CONVERGED)
            # the three rejections
            run = st[idx] < 0
            shift = np.abs(z[idx] - z0[idx]) / float(dz)
            margin[idx] = np.where(run, np.minimum(margin[idx], _rel(shift, float(o["max_shift"]))), margin[idx])
            settle(idx, shift > float(o["max_shift"]), REJECT_SHIFT)
            run = st[idx] < 0
            bad = np.zeros(idx.size, bool)
            lo, hi = 1.0 / float(o["max_deform"]), float(o["max_deform"])
            for s in range(ns):
                G, g, e = pairs[s]
                M = np.array([[G[0][0] + e[0] * zx[idx], G[0][1] + e[0] * zy[idx]], [G[1][0] + e[1] * zx[idx], G[1][1] + e[1] * zy[idx]]])
                smax, smin = rr.singular_values(M)
                counts = frozen[s, idx]
                margin[idx] = np.where(run & counts, np.minimum(margin[idx], np.minimum(_rel(smax, hi), _rel(smin, lo))), margin[idx])
                bad |= counts & ((smax > hi) | (smin < lo))
            settle(idx, bad, REJECT_SLOPE)
            run = st[idx] < 0
            sc = score1[idx]
            margin[idx] = np.where(run, np.minimum(margin[idx], np.minimum(np.abs(sc - float(o["min_score"])), np.abs(sc - score0[idx]))), margin[idx])
            settle(idx, (sc < float(o["min_score"])) | (sc < score0[idx]), REJECT_SCORE)
            settle(idx, np.ones(idx.size, bool), REFINED)

    good = st == REFINED
    gy_, gx_ = py[good], px[good]
    out["depth"][gy_, gx_] = z[good]
    out["gradient"][gy_, gx_, 0], out["gradient"][gy_, gx_, 1] = zx[good], zy[good]
    out["normal"][gy_, gx_] = normal(gr, zx[good], zy[good], plant)
    out["score"][gy_, gx_] = score1[good].astype(np.float32)
    out["status"][py, px] = st.astype(np.uint8)
    out["iterations"][py, px] = iterations
    out["margin"][py, px] = margin
    out["pivot_min"][py, px] = pivot_min
    out["score0"][py, px], out["score1"][py, px] = score0, score1
    return out
