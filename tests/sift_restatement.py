"""numpy restatement of the SIFT detector the library follows (MVE's sfm/sift.cc with Sift::Options defaults).

Scale space, extrema and localisation are float32 in the reference's operation order -- every numpy float32
operation rounds once, as the reference's scalar SSE code does -- with expf / powf taken from the C library, so
these stages are held to the reference bit for bit (tests/test_sift_cases_cpu.py).  Orientation assignment and
the descriptor exist twice, selected by `dtype`: float32 in the reference's order, and float64.

The keyword arguments of scale_space / extrema / localise named `plant_*` put a known error in; the CPU test uses
them to show that its comparisons see such errors.
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
for _n in ("expf", "powf"):
    getattr(_libm, _n).restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def expf(x):
    return f32(_libm.expf(float(x)))


def powf(x, y):
    return f32(_libm.powf(float(x), float(y)))


class Options:
    num_samples_per_octave = 3
    min_octave = 0
    max_octave = 4
    contrast_threshold = f32(0.02) / f32(3.0)
    edge_ratio_threshold = f32(10.0)
    base_blur_sigma = f32(1.6)
    inherent_blur_sigma = f32(0.5)

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(Options, k), k
            setattr(self, k, v)


# ----------------------------------------------------------------------------- scale space

def byte_to_float(img):
    v = img.astype(f32) / f32(255.0)
    return np.minimum(f32(1.0), np.maximum(f32(0.0), v))


def desaturate_average(rgb):
    t = f32(1.0) / f32(3.0)
    return (rgb[:, :, 0] * t + rgb[:, :, 1] * t) + rgb[:, :, 2] * t


def gaussian_weights(sigma):
    """(ks, weights[0..ks]) of blur_gaussian, or (0, None) where it returns a copy."""
    sigma = f32(sigma)
    if f32(-0.1) <= sigma <= f32(0.1):
        return 0, None
    ks = int(np.ceil(sigma * f32(2.884)))
    w = [expf(-((f32(i) * f32(i)) / (f32(2.0) * sigma * sigma))) for i in range(ks + 1)]
    return ks, np.array(w, dtype=f32)


def _border(idx, n, unclamped, mirrored=False):
    if mirrored:                    # ... 1 0 | 0 1 ... n-1 | n-1 n-2 ...
        m = idx % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    return idx % n if unclamped else np.clip(idx, 0, n - 1)


def blur_radii(opts):
    """The blur radius of every image of an octave after the first: (ks of image 1, ..., ks of image S + 2)."""
    S = opts.num_samples_per_octave
    k = powf(2.0, f32(1.0) / f32(S))
    sigma, out = opts.base_blur_sigma, []
    for _ in range(1, S + 3):
        sigmak = sigma * k
        out.append(gaussian_weights(np.sqrt(sigmak * sigmak - sigma * sigma, dtype=f32))[0])
        sigma = sigmak
    return out


def blur_gaussian(img, sigma, plant_reversed_taps=False, plant_unclamped=False, plant_mirrored=False):
    ks, wt = gaussian_weights(sigma)
    if wt is None:
        return img.copy()
    h, w = img.shape
    taps = range(ks, -ks - 1, -1) if plant_reversed_taps else range(-ks, ks + 1)
    out = img
    for axis, n in ((1, w), (0, h)):
        acc = np.zeros((h, w), dtype=f32)
        wsum = f32(0.0)
        base = np.arange(n)
        for i in taps:
            idx = _border(base + i, n, plant_unclamped, plant_mirrored)
            acc = acc + np.take(out, idx, axis=axis) * wt[abs(i)]
            wsum = wsum + wt[abs(i)]
        out = acc / wsum
    return out


def rescale_half_size_gaussian(img, sigma=f32(0.866025403784439)):
    h, w = img.shape
    assert w >= 2 and h >= 2
    ow, oh = (w + 1) >> 1, (h + 1) >> 1
    s2 = f32(2.0) * (sigma * sigma)
    w1, w2, w3 = expf(f32(-0.5) / s2), expf(f32(-2.5) / s2), expf(f32(-4.5) / s2)
    y2, x2 = np.arange(oh) * 2, np.arange(ow) * 2
    rows = [np.maximum(0, y2 - 1), y2, np.minimum(h - 1, y2 + 1), np.minimum(h - 1, y2 + 2)]
    cols = [np.maximum(0, x2 - 1), x2, np.minimum(w - 1, x2 + 1), np.minimum(w - 1, x2 + 2)]
    wts = [[w3, w2, w2, w3], [w2, w1, w1, w2], [w2, w1, w1, w2], [w3, w2, w2, w3]]
    acc = np.zeros((oh, ow), dtype=f32)
    wsum = f32(0.0)
    for r in range(4):
        for c in range(4):
            acc = acc + img[np.ix_(rows[r], cols[c])] * wts[r][c]
            wsum = wsum + wts[r][c]
    return acc / wsum


def rescale_double_size_supersample(img):
    h, w = img.shape
    oh, ow = 2 * h, 2 * w
    y, x = np.arange(oh), np.arange(ow)
    y0, y1 = y >> 1, (y + (y + 1 < oh)) >> 1
    x0, x1 = x >> 1, (x + (x + 1 < ow)) >> 1
    q = f32(0.25)
    return ((img[np.ix_(y0, x0)] * q + img[np.ix_(y0, x1)] * q) + img[np.ix_(y1, x0)] * q) + img[np.ix_(y1, x1)] * q


def refuses(width, height, opts):
    """create_octaves throws when rescale_half_size_gaussian meets an image below 2 pixels a side: it halves
    max(0, min_octave) times before the first octave and once after every octave, the last included."""
    w, h = width, height
    for _ in range(max(0, opts.min_octave) + opts.max_octave - max(0, opts.min_octave) + 1):
        if w < 2 or h < 2:
            return True
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return False


def scale_space(image, opts, **plant):
    """[(octave index, [S+3 images], [S+2 DoG images])], float32."""
    orig = byte_to_float(image)
    if orig.ndim == 3:
        orig = desaturate_average(orig)
    S = opts.num_samples_per_octave
    k = powf(2.0, f32(1.0) / f32(S))
    octaves = []

    def add_octave(index, img, has_sigma, target_sigma):
        sigma = np.sqrt(target_sigma * target_sigma - has_sigma * has_sigma, dtype=f32) if target_sigma > has_sigma else None
        base = blur_gaussian(img, sigma, **plant) if sigma is not None else img.copy()
        imgs, dogs = [base], []
        sigma = target_sigma
        for _ in range(1, S + 3):
            sigmak = sigma * k
            blur_sigma = np.sqrt(sigmak * sigmak - sigma * sigma, dtype=f32)
            nxt = blur_gaussian(base, blur_sigma, **plant)
            imgs.append(nxt)
            dogs.append(nxt - base)
            base, sigma = nxt, sigmak
        octaves.append((index, imgs, dogs))

    if opts.min_octave < 0:
        add_octave(-1, rescale_double_size_supersample(orig), opts.inherent_blur_sigma * f32(2.0), opts.base_blur_sigma)
    img = orig
    for _ in range(opts.min_octave):
        img = rescale_half_size_gaussian(img)
    img_sigma = opts.inherent_blur_sigma
    for i in range(max(0, opts.min_octave), opts.max_octave + 1):
        add_octave(i, img, img_sigma, opts.base_blur_sigma)
        img = rescale_half_size_gaussian(img)
        img_sigma = opts.base_blur_sigma
    return octaves


# ----------------------------------------------------------------------------- extrema

def extrema(octaves, plant_nonstrict=False):
    """float32 [n, 4] rows (octave, sample, x, y) in the reference's order (octave, sample, y, x)."""
    rows = []
    for index, _, dogs in octaves:
        for s in range(len(dogs) - 2):
            h, w = dogs[s].shape
            if h < 3 or w < 3:
                continue
            c = dogs[s + 1][1:h - 1, 1:w - 1]
            largest = np.ones(c.shape, dtype=bool)
            smallest = np.ones(c.shape, dtype=bool)
            for layer in range(3):
                for oy in range(3):
                    for ox in range(3):
                        if layer == 1 and oy == 1 and ox == 1:
                            continue
                        n = dogs[s + layer][oy:oy + h - 2, ox:ox + w - 2]
                        if plant_nonstrict:
                            largest &= ~(n > c)
                            smallest &= ~(n < c)
                        else:
                            largest &= ~(n >= c)
                            smallest &= ~(n <= c)
            ys, xs = np.nonzero(largest | smallest)
            for y, x in zip(ys, xs):
                rows.append((index, s, x + 1, y + 1))
    return np.array(rows, dtype=f32).reshape(-1, 4)


# ----------------------------------------------------------------------------- localisation

REJECTION_TESTS = ("contrast", "score<0", "score>thres", "|fx|>1.5", "|fy|>1.5", "|fs|>1", "sample<-1", "sample>S",
                   "x outside", "y outside")


def localise(octaves, cand, opts, plant_steps=5):
    """(keypoints float32 [m, 4] rows (octave, sample, x, y), rejected-by [n, 10] bool, moved [n] bool,
    singular [n] bool) -- Sift::keypoint_localization on one candidate at a time, float32 scalars."""
    by_index = {o[0]: o for o in octaves}
    S = opts.num_samples_per_octave
    half, quarter, two = f32(0.5), f32(0.25), f32(2.0)
    thres = ((opts.edge_ratio_threshold + f32(1.0)) * (opts.edge_ratio_threshold + f32(1.0))) / opts.edge_ratio_threshold
    out, rejected, moved, singular = [], [], [], []
    with np.errstate(all="ignore"):
        for row in cand:
            oi, sample = int(row[0]), int(row[1])
            dogs = by_index[oi][2][sample:sample + 3]
            h, w = dogs[0].shape
            ix, iy, is_ = int(row[2]), int(row[3]), sample
            sing = False
            for _ in range(plant_steps):
                def AT(s, dx, dy):
                    return dogs[s][iy + dy, ix + dx]
                Dx = (AT(1, 1, 0) - AT(1, -1, 0)) * half
                Dy = (AT(1, 0, 1) - AT(1, 0, -1)) * half
                Ds = (AT(2, 0, 0) - AT(0, 0, 0)) * half
                Dxx = AT(1, 1, 0) + AT(1, -1, 0) - two * AT(1, 0, 0)
                Dyy = AT(1, 0, 1) + AT(1, 0, -1) - two * AT(1, 0, 0)
                Dss = AT(2, 0, 0) + AT(0, 0, 0) - two * AT(1, 0, 0)
                Dxy = (AT(1, 1, 1) + AT(1, -1, -1) - AT(1, -1, 1) - AT(1, 1, -1)) * quarter
                Dxs = (AT(2, 1, 0) + AT(0, -1, 0) - AT(2, -1, 0) - AT(0, 1, 0)) * quarter
                Dys = (AT(2, 0, 1) + AT(0, 0, -1) - AT(2, 0, -1) - AT(0, 0, 1)) * quarter
                m = [Dxx, Dxy, Dxs, Dxy, Dyy, Dys, Dxs, Dys, Dss]
                det = (m[0] * m[4] * m[8] + m[1] * m[5] * m[6] + m[2] * m[3] * m[7]
                       - m[2] * m[4] * m[6] - m[1] * m[3] * m[8] - m[0] * m[5] * m[7])
                if f32(0.0) - f32(1e-15) <= det <= f32(0.0) + f32(1e-15):
                    fx = fy = fs = f32(0.0)
                    sing = True
                    break
                inv = [m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                       m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                       m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
                inv = [v / det for v in inv]
                b = [-Dx, -Dy, -Ds]
                fx, fy, fs = [((f32(0.0) + inv[3 * r] * b[0]) + inv[3 * r + 1] * b[1]) + inv[3 * r + 2] * b[2] for r in range(3)]
                dx = int(fx > f32(0.6) and ix < w - 2) - int(fx < f32(-0.6) and ix > 1)
                dy = int(fy > f32(0.6) and iy < h - 2) - int(fy < f32(-0.6) and iy > 1)
                if dx != 0 or dy != 0:
                    ix += dx
                    iy += dy
                    continue
                break
            val = dogs[1][iy, ix] + half * (Dx * fx + Dy * fy + Ds * fs)
            trace = Dxx + Dyy
            hdet = Dxx * Dyy - Dxy * Dxy
            score = (trace * trace) / hdet
            kx, ky, ks = f32(ix) + fx, f32(iy) + fy, f32(is_) + fs
            rej = (abs(val) < opts.contrast_threshold, score < f32(0.0), score > thres,
                   abs(fx) > f32(1.5), abs(fy) > f32(1.5), abs(fs) > f32(1.0),
                   ks < f32(-1.0), ks > f32(S), kx < f32(0.0) or kx > f32(w - 1), ky < f32(0.0) or ky > f32(h - 1))
            rejected.append(rej)
            moved.append(ix != int(row[2]) or iy != int(row[3]))
            singular.append(sing)
            if not any(rej):
                out.append((f32(oi), ks, kx, ky))
    return (np.array(out, dtype=f32).reshape(-1, 4), np.array(rejected, dtype=bool).reshape(-1, 10),
            np.array(moved, dtype=bool), np.array(singular, dtype=bool))


# ----------------------------------------------------------------------------- orientation and descriptor

def relative_scale(sample, opts):
    return opts.base_blur_sigma * powf(2.0, (f32(sample) + f32(1.0)) / f32(opts.num_samples_per_octave))


def absolute_scale(octave, sample, opts):
    return opts.base_blur_sigma * powf(2.0, f32(octave) + (f32(sample) + f32(1.0)) / f32(opts.num_samples_per_octave))


def mve_round(x):
    return np.floor(x + f32(0.5)) if x > 0 else np.ceil(x - f32(0.5))


PI = 3.14159265358979323846
SQRT2 = 1.41421356237309504880


def grad_ori(img, dtype):
    """Gradient magnitude and orientation (interior pixels, border zero) of one octave image."""
    F = dtype
    img = img.astype(F)
    h, w = img.shape
    grad = np.zeros((h, w), dtype=F)
    ori = np.zeros((h, w), dtype=F)
    if h < 3 or w < 3:
        return grad, ori
    dx = F(0.5) * (img[1:-1, 2:] - img[1:-1, :-2])
    dy = F(0.5) * (img[2:, 1:-1] - img[:-2, 1:-1])
    a = np.arctan2(dy, dx)
    grad[1:-1, 1:-1] = np.sqrt(dx * dx + dy * dy)
    ori[1:-1, 1:-1] = np.where(a < 0, (a.astype(np.float64) + PI * 2.0).astype(F), a)
    return grad, ori


def orientations(kp, grad, ori, opts, dtype):
    """([orientation], smallest relative margin of the peak decisions, float(h1)s)."""
    F = dtype
    nbins = 36
    x, y, sample = f32(kp[2]), f32(kp[3]), f32(kp[1])
    ix, iy = int(x + f32(0.5)), int(y + f32(0.5))
    sigma = relative_scale(sample, opts)
    h, w = grad.shape
    win = int(sigma * f32(1.5) * f32(3.0))
    if ix < win or ix + win >= w or iy < win or iy + win >= h:
        return [], np.inf
    dxf, dyf = F(x - f32(ix)), F(y - f32(iy))
    maxdist = F(win * win) + F(0.5)
    d = np.arange(-win, win + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    dist = (dx.astype(F) - dxf) ** 2 + (dy.astype(F) - dyf) ** 2
    keep = (dist <= maxdist).ravel()
    gm = grad[iy - win:iy + win + 1, ix - win:ix + win + 1].ravel()[keep]
    go = ori[iy - win:iy + win + 1, ix - win:ix + win + 1].ravel()[keep]
    s = F(sigma * f32(1.5))
    weight = np.exp(-(dist.ravel()[keep] / (F(2.0) * s * s)))
    bins = np.clip(((F(nbins) * go).astype(np.float64) / (2.0 * PI)).astype(np.int64), 0, nbins - 1)
    hist = np.zeros(nbins, dtype=F)
    np.add.at(hist, bins, gm * weight)
    for _ in range(6):
        first, prev = hist[0], hist[nbins - 1]
        for j in range(nbins - 1):
            cur = hist[j]
            hist[j] = (prev + cur + hist[j + 1]) / F(3.0)
            prev = cur
        hist[nbins - 1] = (prev + hist[nbins - 1] + first) / F(3.0)
    maxh = hist.max()
    out, margin = [], np.inf
    cut = F(0.8) * maxh if F is f32 else F(f32(0.8)) * maxh
    for i in range(nbins):
        h0, h1, h2 = hist[(i + nbins - 1) % nbins], hist[i], hist[(i + 1) % nbins]
        if maxh > 0:
            # how far the three decisions of this bin are from flipping, relative to the histogram's scale; a bin
            # that is no local maximum by a wide margin cannot become a peak whatever the cut says
            local = min(float(h1 - h0), float(h1 - h2)) / float(maxh)
            above = float(h1 - cut) / float(maxh)
            if local > 0 and above > 0:
                margin = min(margin, local, above)
            else:
                margin = min(margin, max(-local, -above))
        if h1 <= cut or h1 <= h0 or h1 <= h2:
            continue
        xo = F(-0.5) * (h2 - h0) / (h0 - F(2.0) * h1 + h2)
        out.append(F(2.0 * PI * np.float64(xo + F(i) + F(0.5)) / np.float64(nbins)))
    return out, margin


def descriptor(kp, orientation, grad, ori, opts, dtype):
    """float [128], or None where the window leaves the image."""
    F = dtype
    PXB, OHB = 4, 8
    x, y, sample = f32(kp[2]), f32(kp[3]), f32(kp[1])
    ix, iy = int(x + f32(0.5)), int(y + f32(0.5))
    dxf, dyf = F(x - f32(ix)), F(y - f32(iy))
    sigma = relative_scale(sample, opts)
    h, w = grad.shape
    o = F(orientation)
    sino, coso = np.sin(o), np.cos(o)
    binsize = f32(3.0) * sigma
    win = int(SQRT2 * np.float64(binsize) * 5.0 * 0.5)
    if ix < win or ix + win >= w or iy < win or iy + win >= h:
        return None
    binsize = F(binsize)
    d = np.arange(-win, win + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    mod = grad[iy - win:iy + win + 1, ix - win:ix + win + 1].ravel()
    angle = ori[iy - win:iy + win + 1, ix - win:ix + win + 1].ravel()
    theta = angle - o
    theta = np.where(theta < 0, (theta.astype(np.float64) + 2.0 * PI).astype(F), theta)
    winx, winy = dx.ravel().astype(F) - dxf, dy.ravel().astype(F) - dyf
    binoff = F(1.5)
    binx = (coso * winx + sino * winy) / binsize + binoff
    biny = (-sino * winx + coso * winy) / binsize + binoff
    bint = ((theta * F(OHB)).astype(np.float64) / (2.0 * PI) - 0.5).astype(F)
    gw = np.exp(-(((binx - binoff) ** 2 + (biny - binoff) ** 2) / (F(2.0) * F(2.0) * F(2.0))))
    contrib = mod * gw
    bx0, by0, bt0 = np.floor(binx).astype(np.int64), np.floor(biny).astype(np.int64), np.floor(bint).astype(np.int64)
    bxi, byi, bti = [bx0, bx0 + 1], [by0, by0 + 1], [bt0, bt0 + 1]
    wx = [bxi[1].astype(F) - binx, F(1.0) - (bxi[1].astype(F) - binx)]
    wy = [byi[1].astype(F) - biny, F(1.0) - (byi[1].astype(F) - biny)]
    wt = [bti[1].astype(F) - bint, F(1.0) - (bti[1].astype(F) - bint)]
    bti = [np.where(bti[0] < 0, bti[0] + OHB, bti[0]), np.where(bti[1] >= OHB, bti[1] - OHB, bti[1])]
    idx, val, ok = [], [], []
    for yy in range(2):
        for xx in range(2):
            for tt in range(2):
                ok.append((bxi[xx] >= 0) & (bxi[xx] < PXB) & (byi[yy] >= 0) & (byi[yy] < PXB))
                idx.append(bti[tt] + bxi[xx] * OHB + byi[yy] * OHB * PXB)
                val.append(contrib * wx[xx] * wy[yy] * wt[tt])
    idx, val, ok = np.stack(idx, 1).ravel(), np.stack(val, 1).ravel(), np.stack(ok, 1).ravel()
    data = np.zeros(128, dtype=F)
    np.add.at(data, idx[ok], val[ok])

    def normalize(v):
        sq = F(0.0)
        for e in v:
            sq = sq + e * e
        return v / np.sqrt(sq)
    with np.errstate(all="ignore"):
        data = normalize(data)
        data = np.minimum(data, F(f32(0.2)))
        data = normalize(data)
    return data


def describe(octaves, keypoints, opts, dtype):
    """Per keypoint: (orientations, margin, [descriptor or None per orientation])."""
    by_index = {o[0]: o for o in octaves}
    cache = {}
    out = []
    for kp in keypoints:
        oi = int(kp[0])
        i = int(mve_round(f32(kp[1]))) + 1
        if (oi, i) not in cache:
            cache[(oi, i)] = grad_ori(by_index[oi][1][i], dtype)
        grad, ori = cache[(oi, i)]
        oris, margin = orientations(kp, grad, ori, opts, dtype)
        out.append((oris, margin, [descriptor(kp, f32(o), grad, ori, opts, dtype) for o in oris]))
    return out


def generation_meta(kp, orientation, opts):
    """x, y, scale, orientation of Sift::Descriptor, float32."""
    sf = f32(2.0 ** int(kp[0]))
    return (sf * (f32(kp[2]) + f32(0.5)) - f32(0.5), sf * (f32(kp[3]) + f32(0.5)) - f32(0.5),
            absolute_scale(int(kp[0]), kp[1], opts), f32(orientation))


def linear_at_u8(img, x, y):
    """Image<unsigned char>::linear_at with interpolate<unsigned char>'s + 0.5f truncation; [channels]."""
    im = img if img.ndim == 3 else img[:, :, None]
    h, w, _ = im.shape
    x = max(f32(0.0), min(f32(w - 1), f32(x)))
    y = max(f32(0.0), min(f32(h - 1), f32(y)))
    fx, fy = int(x), int(y)
    fx1, fy1 = min(fx + 1, w - 1), min(fy + 1, h - 1)
    w1 = x - f32(fx)
    w0 = f32(1.0) - w1
    w3 = y - f32(fy)
    w2 = f32(1.0) - w3
    a, b, c, d = (im[fy, fx].astype(f32), im[fy, fx1].astype(f32), im[fy1, fx].astype(f32), im[fy1, fx1].astype(f32))
    v = a * (w0 * w2) + b * (w1 * w2) + c * (w0 * w3) + d * (w1 * w3) + f32(0.5)
    return v.astype(np.uint8)


def normalized_position(x, y, width, height):
    fw, fh = f32(width), f32(height)
    fn = max(fw, fh)
    return (f32(x) + f32(0.5) - fw * f32(0.5)) / fn, (f32(y) + f32(0.5) - fh * f32(0.5)) / fn
