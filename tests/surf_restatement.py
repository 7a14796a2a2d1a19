"""numpy restatement of the SURF detector the library follows (MVE's sfm/surf.cc).

Every float32 operation is one numpy float32 operation (one rounding, as the reference's scalar SSE code), every
double operation a float64 one, in the reference's order; the summed-area table is int64 as the reference's.
expf, sinf, cosf, atan2f and atan2 come from the C library through ctypes.  Sequential sums are numpy cumsums (which
add in order, unlike numpy sums).

The keyword arguments named `plant_*` put a known error in; the CPU test uses them to show that its comparisons
see such errors.
"""
import ctypes
import ctypes.util
import math

import numpy as np

f32, f64 = np.float32, np.float64
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
for _n in ("expf", "sinf", "cosf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2.restype = ctypes.c_double
_libm.atan2.argtypes = [ctypes.c_double, ctypes.c_double]


def expf(x):
    return f32(_libm.expf(float(x)))


def sinf(x):
    return f32(_libm.sinf(float(x)))


def cosf(x):
    return f32(_libm.cosf(float(x)))


def atan2f(y, x):
    return f32(_libm.atan2f(float(y), float(x)))


PI = 3.14159265358979323846264338327950288
AMBIGUITY_ULPS = 8


def filter_size(o, k):
    return 2 ** (o + 1) * (k + 1) + 1


# ----------------------------------------------------------------------------- summed-area table

def desaturate_lightness(rgb):
    hi, lo = rgb.max(axis=2).astype(f32), rgb.min(axis=2).astype(f32)
    return (hi * f32(0.5) + lo * f32(0.5) + f32(0.5)).astype(np.uint8)


def grey_of(image):
    return image if image.ndim == 2 else desaturate_lightness(image)


def integral(grey):
    return grey.astype(np.int64).cumsum(axis=1).cumsum(axis=0)


# ----------------------------------------------------------------------------- response maps

def _dxx(S, w, fs, x, y):
    fs2 = fs // 2
    r1 = (x - fs - fs2 - 1) + w * (y - fs)
    r2 = r1 + w * (fs + fs - 1)
    v = [S[r1], S[r1 + fs], S[r1 + 2 * fs], S[r1 + 3 * fs], S[r2], S[r2 + fs], S[r2 + 2 * fs], S[r2 + 3 * fs]]
    return (v[5] + v[0] - v[4] - v[1]) - 2 * (v[6] + v[1] - v[5] - v[2]) + (v[7] + v[2] - v[6] - v[3])


def _dyy(S, w, fs, x, y):
    fs2 = fs // 2
    r1 = (x - fs) + w * (y - fs - fs2 - 1)
    r2, r3, r4 = r1 + w * fs, r1 + 2 * w * fs, r1 + 3 * w * fs
    e = fs + fs - 1
    v = [S[r1], S[r2], S[r3], S[r4], S[r1 + e], S[r2 + e], S[r3 + e], S[r4 + e]]
    return (v[5] + v[0] - v[1] - v[4]) - 2 * (v[6] + v[1] - v[2] - v[5]) + (v[7] + v[2] - v[3] - v[6])


def _dxy(S, w, fs, x, y):
    r1 = (x - fs - 1) + w * (y - fs - 1)
    r2 = r1 + w * fs
    r3 = r2 + w
    r4 = r3 + w * fs
    ret = S[r2 + fs] + S[r1] - S[r2] - S[r1 + fs]
    ret = ret - (S[r2 + fs + fs + 1] + S[r1 + fs + 1] - S[r2 + fs + 1] - S[r1 + fs + fs + 1])
    ret = ret - (S[r4 + fs] + S[r3] - S[r4] - S[r3 + fs])
    return ret + (S[r4 + fs + fs + 1] + S[r3 + fs + 1] - S[r4 + fs + 1] - S[r3 + fs + fs + 1])


def response_map(sat, o, k, plant_symmetric_border=False):
    h, w = sat.shape
    S = sat.reshape(-1)
    fs, step = filter_size(o, k), 2 ** o
    inv_karea = f32(1.0 / (fs * (2 * fs - 1)))
    weight = f32(0.912)
    border = fs + fs // 2 + 1
    xs, ys = np.arange(0, w, step), np.arange(0, h, step)
    out = np.zeros((len(ys), len(xs)), f32)
    hi = 0 if plant_symmetric_border else 1
    vx = np.nonzero((xs >= border) & (xs + border + hi <= w))[0]
    vy = np.nonzero((ys >= border) & (ys + border + hi <= h))[0]
    if len(vx) and len(vy):
        x, y = np.meshgrid(xs[vx], ys[vy])
        dxx_t = _dxx(S, w, fs, x, y).astype(f32) * inv_karea
        dyy_t = _dyy(S, w, fs, x, y).astype(f32) * inv_karea
        dxy_t = _dxy(S, w, fs, x, y).astype(f32) * inv_karea
        out[np.ix_(vy, vx)] = dxx_t * dyy_t - weight * dxy_t * dxy_t
    return out


def response_maps(sat, **plant):
    return [[response_map(sat, o, k, **plant) for k in range(4)] for o in range(4)]


# ----------------------------------------------------------------------------- extrema

def extrema(maps, plant_nonstrict=False):
    """Candidates as rows (octave, sample, x, y), float32, in the detector's order."""
    rows = []
    for o in range(4):
        oh, ow = maps[o][0].shape
        if ow < 3 or oh < 3:
            continue
        for s in (1, 2):
            c = maps[o][s][1:-1, 1:-1]
            flag = (c > maps[o][s][1:-1, :-2]) & (c > maps[o][s][1:-1, 2:])
            for layer in (s, s - 1, s + 1):
                for dy in (0, 1, 2):
                    for dx in (0, 1, 2):
                        if layer == s and dy == 1 and dx == 1:
                            continue
                        v = maps[o][layer][dy:oh - 2 + dy, dx:ow - 2 + dx]
                        flag &= ~((v > c) if plant_nonstrict else (v >= c))
            for y, x in np.argwhere(flag):
                rows.append((o, s, x + 1, y + 1))
    return np.array(rows, f32).reshape(-1, 4)


# ----------------------------------------------------------------------------- localisation

def localise(maps, cand, width, height, contrast_threshold=500.0):
    thr = f32(contrast_threshold)
    out = []
    for c in cand:
        o, sample, x, y = int(c[0]), int(c[1]), int(c[2]), int(c[3])
        N = [maps[o][sample + d][y - 1:y + 2, x - 1:x + 2].reshape(-1) for d in (-1, 0, 1)]
        b = [f64(-(N[1][5] - N[1][3])) * 0.5, f64(-(N[1][7] - N[1][1])) * 0.5, f64(-(N[2][4] - N[0][4])) * 0.5]
        m = [None] * 9
        m[0] = f64(N[1][3]) - 2.0 * f64(N[1][4]) + f64(N[1][5])
        m[1] = f64(N[1][8] - N[1][6] - N[1][2] + N[1][0]) * 0.25
        m[2] = f64(N[2][5] - N[2][3] - N[0][5] + N[0][3]) * 0.25
        m[3] = m[1]
        m[4] = f64(N[1][1]) - 2.0 * f64(N[1][4]) + f64(N[1][7])
        m[5] = f64(N[2][7] - N[2][1] - N[0][7] + N[0][1]) * 0.25
        m[6], m[7] = m[2], m[5]
        m[8] = f64(N[0][4]) - 2.0 * f64(N[1][4]) + f64(N[2][4])
        det = (m[0] * m[4] * m[8] + m[1] * m[5] * m[6] + m[2] * m[3] * m[7]
               - m[2] * m[4] * m[6] - m[1] * m[3] * m[8] - m[0] * m[5] * m[7])
        if f64(f32(0.0) - f32(1.0e-5)) <= det <= f64(f32(0.0) + f32(1.0e-5)):
            continue
        inv = [m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
               m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
               m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
        with np.errstate(all="ignore"):
            inv = [v / det for v in inv]
        vx = [f64(0.0) + inv[3 * r] * b[0] + inv[3 * r + 1] * b[1] + inv[3 * r + 2] * b[2] for r in range(3)]
        if max(vx) > 0.5 or min(vx) < f64(f32(-0.5)):
            continue
        dog_value = f32(f64(N[1][4]) - 0.5 * (f64(0.0) + b[0] * vx[0] + b[1] * vx[1] + b[2] * vx[2]))
        if dog_value < thr:
            continue
        sampling = f32(2 ** o)
        kx = f32((f64(c[2]) + vx[0]) * f64(sampling))
        ky = f32((f64(c[3]) + vx[1]) * f64(sampling))
        ks = f32(f64(c[1]) + vx[2])
        if kx < f32(0.0) or kx + f32(1.0) > f32(width) or ky < f32(0.0) or ky + f32(1.0) > f32(height):
            continue
        out.append((f32(o), ks, kx, ky))
    return np.array(out, f32).reshape(-1, 4)


def keypoint_scale(kp):
    sample = int(f32(kp[1]) + f32(0.5))
    return f32(3 * filter_size(int(kp[0]), sample)) * f32(1.2) / f32(9.0)


# ----------------------------------------------------------------------------- Haar responses

def haar(S, w, x, y, fs):
    """The integer numerators of filter_dx_dy at arrays x, y, and whether a tap left the table (read as zero)."""
    size = S.shape[0]
    xb = (x - fs - 1) + (y - fs - 1) * w
    yb = (x - fs - 1) + (y - 1) * w
    lower = xb + w * (2 * fs + 1)
    outside = np.zeros(np.shape(xb), bool)

    def tap(i):
        bad = (i < 0) | (i >= size)
        outside[...] |= bad
        return np.where(bad, 0, S[np.clip(i, 0, size - 1)])
    x1, x2, x3, x4 = tap(xb), tap(xb + fs), tap(xb + fs + 1), tap(xb + 2 * fs + 1)
    x5, x6, x7, x8 = tap(lower), tap(lower + fs), tap(lower + fs + 1), tap(lower + 2 * fs + 1)
    y1, y2, y3, y4 = tap(yb), tap(yb + 2 * fs + 1), tap(yb + w), tap(yb + w + 2 * fs + 1)
    return (x8 + x2 - x4 - x6) - (x7 + x1 - x3 - x5), (x8 + y1 - x5 - y2) - (y4 + x1 - y3 - x4), outside


# ----------------------------------------------------------------------------- orientation

def gaussian_table():
    """(weights, rx, ry) of the 109 samples: the weights as the reference spells them, six significant digits."""
    g, rxs, rys = [], [], []
    for ry in range(-5, 6):
        for rx in range(-5, 6):
            if rx * rx + ry * ry >= 36:
                continue
            g.append(f32(float("%.6g" % math.exp(-(rx * rx + ry * ry) / 12.5))))
            rxs.append(rx)
            rys.append(ry)
    return np.array(g, f32), np.array(rxs), np.array(rys)


_TABLE = gaussian_table()


def window_starts(windows=None):
    deg, out = -PI, []
    while deg < PI if windows is None else len(out) < windows:
        out.append(deg)
        deg += PI / 8.0
    return out


def _ulp(v):
    return float(np.spacing(np.abs(f32(v))))


def orientation(sat, x, y, scale, plant_windows=None, plant_float_sums=False):
    """descriptor_orientation for a keypoint at float x, y with float scale: None where the margin test rejects it,
    else (orientation float32, best_dx, best_dy, ambiguous)."""
    h, w = sat.shape
    S = sat.reshape(-1)
    dx_, dy_, ds = int(f32(x) + f32(0.5)), int(f32(y) + f32(0.5)), int(scale)
    spacing = 8 * ds + 1
    if dx_ < spacing or dy_ < spacing or dx_ + spacing >= w or dy_ + spacing >= h:
        return None
    g, rx, ry = _TABLE
    fs = 2 * ds
    ix, iy, outside = haar(S, w, dx_ + rx * ds, dy_ + ry * ds, fs)
    assert not outside.any()
    norm = f32((2 * fs + 1) * fs * (fs + 1))
    dx = ix.astype(f32) / norm * g
    dy = iy.astype(f32) / norm * g
    ang = np.array([atan2f(b, a) for a, b in zip(dx, dy)], f32)
    a64 = ang.astype(f64)
    ap, am = a64 + 2.0 * PI, a64 - 2.0 * PI
    best_dx = best_dy = best_len = 0.0
    half = PI / 6.0
    ambiguous = False
    live = (dx != 0) | (dy != 0)
    acc = f32 if plant_float_sums else f64
    for deg in window_starts(plant_windows):
        ws, we = deg - half, deg + half
        sel = ((a64 > ws) & (a64 < we)) | ((ap > ws) & (ap < we)) | ((am > ws) & (am < we))
        for bound in (ws, we):
            for shift in (0.0, 2.0 * PI, -2.0 * PI):
                # the float angle against the bound, and against its images by 2 pi
                near = np.abs(a64 - (bound - shift)) <= AMBIGUITY_ULPS * np.spacing(np.abs(ang)).astype(f64)
                ambiguous |= bool((near & live).any())
        sx = float(np.cumsum(np.concatenate([[0.0], dx[sel]]).astype(acc))[-1])      # 0.0 + d0 + d1 ...
        sy = float(np.cumsum(np.concatenate([[0.0], dy[sel]]).astype(acc))[-1])
        length = sx * sx + sy * sy
        if length > best_len:
            best_dx, best_dy, best_len = sx, sy, length
    return f32(_libm.atan2(best_dy, best_dx)), best_dx, best_dy, ambiguous


# ----------------------------------------------------------------------------- descriptor

def descriptor_weights():
    sq = (f32(2.0) * f32(3.3)) * (f32(2.0) * f32(3.3))
    return np.array([[expf(-f32(x * x + y * y) / sq) for x in range(-10, 10)] for y in range(-10, 10)], f32)


_WEIGHTS = None


def describe(sat, x, y, scale, sin_ori, cos_ori):
    """descriptor_computation: (status, descriptor float32 [64], sample coordinates int [400, 2]); status 0 rejected,
    1 ok, 2 ok with taps outside the table read as zero."""
    global _WEIGHTS
    if _WEIGHTS is None:
        _WEIGHTS = descriptor_weights()
    h, w = sat.shape
    S = sat.reshape(-1)
    x, y, s, c = f32(x), f32(y), f32(sin_ori), f32(cos_ori)
    ds = int(scale)
    spacing = f32(15 * ds + 1)
    if x < spacing or y < spacing or x + spacing >= f32(w) or y + spacing > f32(h):
        return 0, np.zeros(64, f32), None
    gy, gx = np.mgrid[-10:10, -10:10]
    fx, fy = gx.astype(f32) + f32(0.5), gy.astype(f32) + f32(0.5)
    px = x + (c * fx - s * fy) * f32(ds)
    py = y + (s * fx + c * fy) * f32(ds)
    rnd = lambda p: np.where(p > 0, np.floor(p + f32(0.5)), np.ceil(p - f32(0.5))).astype(np.int64)
    rx, ry = rnd(px), rnd(py)
    ix, iy, outside = haar(S, w, rx, ry, ds)
    norm = f32((2 * ds + 1) * ds * (ds + 1))
    dx, dy = ix.astype(f32) / norm, iy.astype(f32) / norm
    ori_dx = c * dx + s * dy
    ori_dy = (-s) * dx + c * dy
    wt = _WEIGHTS
    v = np.stack([wt * ori_dx, wt * ori_dy, wt * np.abs(ori_dx), wt * np.abs(ori_dy)], axis=-1)     # [20, 20, 4]
    terms = v.reshape(4, 5, 4, 5, 4).transpose(0, 2, 4, 1, 3).reshape(64, 25)                          # (cy, cx, bin), (yy, xx)
    d = np.cumsum(np.concatenate([np.zeros((64, 1), f32), terms], axis=1), axis=1, dtype=f32)[:, -1]     # 0.0f + t0 + t1 ...
    nrm = np.cumsum(d * d, dtype=f32)[-1]
    coords = np.stack([rx.reshape(-1), ry.reshape(-1)], axis=1)
    if f64(f32(0.0)) - 1e-8 <= f64(nrm) <= f64(f32(0.0)) + 1e-8:
        return 0, np.zeros(64, f32), coords
    return (2 if outside.any() else 1), d / np.sqrt(nrm), coords


# ----------------------------------------------------------------------------- the detector

def generate(sat, kps, upright=False, trig=None, **plant):
    """descriptor_assignment: per keypoint None, or a dict with x, y, scale, orientation, sin, cos, ambiguous, status
    and data.  trig: {orientation bytes: (sin, cos)} to take instead of this machine's sinf / cosf."""
    out = []
    for kp in kps:
        scale = keypoint_scale(kp)
        o = orientation(sat, kp[2], kp[3], scale, **plant)
        if o is None:
            out.append(None)
            continue
        ori, _, _, ambiguous = o
        s, c = (f32(0.0), f32(1.0)) if upright else (trig or {}).get(ori.tobytes(), (sinf(ori), cosf(ori)))
        status, data, _ = describe(sat, kp[2], kp[3], scale, s, c)
        out.append(dict(x=f32(kp[2]), y=f32(kp[3]), scale=scale, orientation=ori, sin=f32(s), cos=f32(c),
                        ambiguous=ambiguous, status=status, data=data))
    return out
