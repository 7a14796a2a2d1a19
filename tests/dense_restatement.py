"""The definition of the dense plane sweep and of the fusion (include/osfm_hip.h, "Dense depth maps"; DESIGN.md
"Dense plane sweep") in float64 numpy.  The kernels of orthosfm_amd/csrc/dense_kernels.hip are held to it.

Cameras are affine: view v maps X to the pixel A_v X + t_v (P_v = [A_v | t_v], [2][4]), pixel centres at integers.
For a reference view r: d_r = (a0 x a1) / |a0 x a1|, B_r = A_r^T (A_r A_r^T)^-1, X(x, z) = B_r (x - t_r) + z d_r, and
for a source s: G = A_s B_r, g = t_s - G t_r, e = A_s d_r, so that pixel x at depth z is seen at G x + g + z e.

Everything that decides a test exactly -- the geometry, the warped positions, the inside test, the consistency
test -- is written out in scalar operations in one fixed order, which dense_api.hip and the kernels repeat (the
build contracts nothing), so those decisions are the same to the bit.  The correlation sums are float64 here and
float32 on the centred values on the device: tests/dense_cases.py holds the two together within BOUNDS, outside the
pixels whose `margin` says that a rounding may decide them.
"""
import math

import numpy as np

OK, BORDER, FLAT, NO_SOURCES, LOW_SCORE, RANGE_EDGE, INCONSISTENT, DUPLICATE = range(8)
STATUS_NAMES = ("OK", "BORDER", "FLAT", "NO_SOURCES", "LOW_SCORE", "RANGE_EDGE", "INCONSISTENT", "DUPLICATE")
DEFAULTS = dict(radius=3, min_contrast=2.0, min_score=0.8, min_sources=2, consistency_tol=2.0, min_consistent=2)
MAX_SOURCES = 8


def grey(image):
    """float32 [h, w]: the byte, or (float32)(r + g + b) / 3.0f -- the refiner's image."""
    im = np.asarray(image)
    assert im.dtype == np.uint8
    if im.ndim == 2:
        return im.astype(np.float32)
    return im.astype(np.int32).sum(axis=2).astype(np.float32) / np.float32(3.0)


def centred(image):
    """The samples the score is formed on: the grey image minus 128.0f, in float32, then float64."""
    return (grey(image) - np.float32(128.0)).astype(np.float64)


class Geometry:
    """What a view contributes: A [2][3], t [2], the viewing axis d [3] and B [3][2]; ok is False when a value is not finite or A has no rank 2."""

    def __init__(self, P):
        P = [[float(v) for v in row] for row in np.asarray(P, dtype=np.float64).reshape(2, 4)]
        a0, a1 = P[0][:3], P[1][:3]
        self.A, self.t = (a0, a1), (P[0][3], P[1][3])
        c = (a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0])
        nn = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        m00 = (a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2]
        m01 = (a0[0] * a1[0] + a0[1] * a1[1]) + a0[2] * a1[2]
        m11 = (a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2]
        det = m00 * m11 - m01 * m01
        self.ok = all(math.isfinite(v) for row in P for v in row) and det > 1e-12 * (m00 * m11) and nn > 0.0
        if not self.ok:
            return
        self.d = (c[0] / nn, c[1] / nn, c[2] / nn)
        i00, i01, i11 = m11 / det, -m01 / det, m00 / det
        self.B = tuple((a0[j] * i00 + a1[j] * i01, a0[j] * i01 + a1[j] * i11) for j in range(3))

    def pair(self, src):
        """G [2][2], g [2], e [2] of the source `src` seen from this reference."""
        As, ts, B, d, tr = src.A, src.t, self.B, self.d, self.t
        G = tuple(tuple((As[i][0] * B[0][j] + As[i][1] * B[1][j]) + As[i][2] * B[2][j] for j in range(2)) for i in range(2))
        g = tuple(ts[i] - (G[i][0] * tr[0] + G[i][1] * tr[1]) for i in range(2))
        e = tuple((As[i][0] * d[0] + As[i][1] * d[1]) + As[i][2] * d[2] for i in range(2))
        return G, g, e

    def point(self, x, y, z):
        """X(x, z) in the kernel's order; x, y, z arrays or scalars."""
        dx, dy = x - self.t[0], y - self.t[1]
        return tuple((self.B[j][0] * dx + self.B[j][1] * dy) + z * self.d[j] for j in range(3))

    def project(self, X):
        return tuple(((self.A[i][0] * X[0] + self.A[i][1] * X[1]) + self.A[i][2] * X[2]) + self.t[i] for i in range(2))

    def depth(self, X):
        return (self.d[0] * X[0] + self.d[1] * X[1]) + self.d[2] * X[2]


def box(a, R):
    """Sums over the (2R+1)^2 windows that lie inside a [h, w]: [h - 2R, w - 2R]."""
    h, w = a.shape
    side = 2 * R + 1
    row = a[:, 0:w - 2 * R].copy()
    for j in range(1, side):
        row = row + a[:, j:j + w - 2 * R]
    out = row[0:h - 2 * R].copy()
    for j in range(1, side):
        out = out + row[j:j + h - 2 * R]
    return out


def box_running_float32(a, R):
    """The same sums from a float32 summed-area table: running sums, which keep the rounding of everything they
    have passed.  Only for the deliberate error of tests/test_dense_cases_cpu.py."""
    h, w = a.shape
    side = 2 * R + 1
    t = np.zeros((h + 1, w + 1), np.float32)
    t[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.float32), axis=0, dtype=np.float32), axis=1, dtype=np.float32)
    return ((t[side:, side:] - t[:-side, side:]) - (t[side:, :-side] - t[:-side, :-side])).astype(np.float64)


def warp(img, G, g, e, z, xs, ys):
    """(sample, inside) of every reference pixel at depth z in the source image img (centred, float64)."""
    h, w = img.shape
    px = (G[0][0] * xs + G[0][1] * ys) + (g[0] + z * e[0])
    py = (G[1][0] * xs + G[1][1] * ys) + (g[1] + z * e[1])
    inside = (px >= 0.0) & (px <= float(w - 1)) & (py >= 0.0) & (py <= float(h - 1))
    qx, qy = np.where(inside, px, 0.0), np.where(inside, py, 0.0)
    x0 = np.minimum(np.floor(qx).astype(np.int64), max(w - 2, 0))
    y0 = np.minimum(np.floor(qy).astype(np.int64), max(h - 2, 0))
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = qx - x0, qy - y0
    top = (1.0 - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (1.0 - fx) * img[y1, x0] + fx * img[y1, x1]
    return np.where(inside, (1.0 - fy) * top + fy * bot, 0.0), inside


def sweep(images, P, ref, sources, z_min, dz, num_depths, uncentred_float32=False, **options):
    """The depth map of view `ref` against `sources`: dict of depth [h, w] (NaN where the status is not OK), score
    (0 there), status (uint8), margin, best (k*, -1 without one).  uncentred_float32: the deliberate error of
    tests/test_dense_cases_cpu.py -- running float32 sums of the raw grey values."""
    o = dict(DEFAULTS)
    o.update(options)
    R, D = int(o["radius"]), int(num_depths)
    n = float((2 * R + 1) ** 2)
    thr = n * o["min_contrast"] ** 2
    gr = Geometry(P[ref])
    img_r = centred(images[ref])
    if uncentred_float32:
        img_r = grey(images[ref])
    h, w = img_r.shape
    status = np.full((h, w), BORDER, np.uint8)
    depth = np.full((h, w), np.nan)
    score = np.zeros((h, w), np.float32)
    margin = np.full((h, w), np.inf)
    best = np.full((h, w), -1, np.int32)
    out = dict(depth=depth, score=score, status=status, margin=margin, best=best)
    if h <= 2 * R or w <= 2 * R:
        return out
    sums = box_running_float32 if uncentred_float32 else box
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sr, srr = sums(img_r, R), sums(img_r * img_r, R)
    var_r = srr - sr * sr / n
    hh, ww = var_r.shape
    c = np.zeros((D, hh, ww))
    valid = np.zeros((D, hh, ww), bool)
    vw_margin = np.full((hh, ww), np.inf)
    pairs = [gr.pair(Geometry(P[s])) for s in sources]
    imgs = [grey(images[s]) if uncentred_float32 else centred(images[s]) for s in sources]
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(D):
            z = z_min + k * dz
            total, count = np.zeros((hh, ww)), np.zeros((hh, ww), np.int64)
            for (G, g, e), img_s in zip(pairs, imgs):
                v, inside = warp(img_s, G, g, e, z, xs, ys)
                full = sums(inside.astype(np.float64), R) == n
                sw = sums(v, R)
                sww = sums(v * v, R)
                swr = sums(v * img_r, R)
                var_w = sww - sw * sw / n
                cov = swr - sw * sr / n
                ok = full & (var_w >= thr)
                vw_margin = np.minimum(vw_margin, np.where(full, np.abs(var_w / thr - 1.0), np.inf))
                s = cov / np.sqrt(var_r * var_w)
                total += np.where(ok, s, 0.0)
                count += ok
            valid[k] = count >= int(o["min_sources"])
            c[k] = np.where(valid[k], total / np.maximum(count, 1), -np.inf)
    kb = np.argmax(c, axis=0)                       # the lowest k of the largest valid c
    any_valid = valid.any(axis=0)
    c0 = np.take_along_axis(c, kb[None], 0)[0]
    km, kp = np.clip(kb - 1, 0, D - 1), np.clip(kb + 1, 0, D - 1)
    cm, cp = np.take_along_axis(c, km[None], 0)[0], np.take_along_axis(c, kp[None], 0)[0]
    edge = (kb == 0) | (kb == D - 1) | ~np.isfinite(cm) | ~np.isfinite(cp)
    st = np.full((hh, ww), OK, np.uint8)
    st[edge] = RANGE_EDGE
    st[c0 < o["min_score"]] = LOW_SCORE
    st[~any_valid] = NO_SOURCES
    st[var_r < thr] = FLAT
    good = st == OK
    with np.errstate(invalid="ignore", divide="ignore"):
        off = 0.5 * (cm - cp) / (cm - 2.0 * c0 + cp)
    zz = z_min + (kb + np.where(good, off, 0.0)) * dz
    # the margin: how far every tested quantity is from deciding otherwise
    others = c.copy()
    np.put_along_axis(others, kb[None], -np.inf, 0)
    runner = others.max(axis=0)
    m = np.abs(var_r / thr - 1.0)
    tested = st != FLAT
    m = np.where(tested, np.minimum(m, vw_margin), m)
    scored = tested & any_valid
    with np.errstate(invalid="ignore"):
        m = np.where(scored, np.minimum(m, np.minimum(np.abs(c0 - o["min_score"]), c0 - runner)), m)
    inner = (slice(R, h - R), slice(R, w - R))
    status[inner] = st
    depth[inner] = np.where(good, zz, np.nan)
    score[inner] = np.where(good, c0, 0.0).astype(np.float32)
    margin[inner] = m
    best[inner] = np.where(any_valid & (st != FLAT), kb, -1)
    return out


def fuse(P, maps, dzs, **options):
    """Consistency and fusion over the swept views: maps {view: sweep result}, dzs {view: dz}.  Returns dict of
    final {view: status plane}, points [N, 3], view [N], pixel [N, 2] (x, y), and touched {view: bool plane}: the
    pixels whose outcome may change when every depth moves by up to depth_band steps of its view, or through an
    ambiguous pixel -- ambiguous {view: bool plane} says which pixels of the sweeps are."""
    o = dict(DEFAULTS)
    o.update(options)
    ambiguous = o.get("ambiguous") or {v: np.zeros(maps[v]["status"].shape, bool) for v in maps}
    band = float(o.get("depth_band", 0.0))
    geo = {v: Geometry(P[v]) for v in maps}
    final, touched = {}, {}
    pts, vws, pxs = [], [], []
    for r in sorted(maps):
        st, z = maps[r]["status"], maps[r]["depth"]
        h, w = st.shape
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        okr = st == OK
        zr = np.where(okr, z, 0.0)
        X = geo[r].point(xs, ys, zr)
        support, lower = np.zeros((h, w), np.int64), np.zeros((h, w), bool)
        touch = ambiguous[r].copy()
        for s in sorted(maps):
            if s == r:
                continue
            q = geo[s].project(X)
            fx, fy = np.floor(q[0] + 0.5), np.floor(q[1] + 0.5)
            hs, ws = maps[s]["status"].shape
            ins = okr & (fx >= 0) & (fx <= ws - 1) & (fy >= 0) & (fy <= hs - 1)
            ix, iy = np.where(ins, fx, 0).astype(np.int64), np.where(ins, fy, 0).astype(np.int64)
            oks = ins & (maps[s]["status"][iy, ix] == OK)
            zs = np.where(oks, maps[s]["depth"][iy, ix], 0.0)
            diff = np.abs(zs - geo[s].depth(X))
            sup = oks & (diff <= o["consistency_tol"] * dzs[s])
            support += sup
            lower |= sup & (s < r)
            # what may turn out otherwise: the pixel looked at is ambiguous; q moves by |e| per unit of this view's
            # depth, past a rounding to the nearest pixel; the depth test sees both depths move
            e = geo[r].pair(geo[s])[2]
            reach = band * dzs[r] * max(abs(e[0]), abs(e[1]))
            near = np.minimum(np.abs(q[0] + 0.5 - np.round(q[0] + 0.5)), np.abs(q[1] + 0.5 - np.round(q[1] + 0.5))) <= reach
            touch |= okr & near
            touch |= ins & ambiguous[s][iy, ix]
            touch |= oks & (np.abs(diff / dzs[s] - o["consistency_tol"]) <= band * (1.0 + dzs[r] / dzs[s]))
        f = st.copy()
        f[okr & (support < int(o["min_consistent"]))] = INCONSISTENT
        f[okr & (support >= int(o["min_consistent"])) & lower] = DUPLICATE
        final[r], touched[r] = f, touch
        keep = f == OK
        iy, ix = np.nonzero(keep)
        pts.append(np.stack([X[0][keep], X[1][keep], X[2][keep]], axis=1))
        vws.append(np.full(ix.shape[0], r, np.int32))
        pxs.append(np.stack([ix, iy], axis=1).astype(np.int32))
    cat = lambda a, shape, dt: np.concatenate(a) if a else np.zeros(shape, dt)
    return dict(final=final, touched=touched, points=cat(pts, (0, 3), np.float64), view=cat(vws, (0,), np.int32),
                pixel=cat(pxs, (0, 2), np.int32))
