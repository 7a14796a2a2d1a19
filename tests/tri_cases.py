"""Cases, reference, bound and check of the ray triangulation (ba_triangulate_kernel in ba_kernels.hip, reached through
osfm_ba_triangulate, osfm_filter_reprojection and osfm_scene_triangulate).

The reference is written from the reference project's camera accessors and intersectRays
(OrthoQuaternionCamera.cpp:45-59, OrthographicCamera.cpp:55-61, 78-95, 128-139, 183-193, triangulation.cpp:11-42),
not from the kernel or from oracle_ba_triangulate (oracle/ba_oracle.c), which is the kernel's line-for-line twin.
It is evaluated with mpmath at 200 bits on the float64 inputs:
  quaternion model   the rotation is Eigen's q * v expression, v + w t + u x t with t = 2 u x v, q as stored and NOT
                     normalised; origin = q * (s xn, s yn, -10), direction = q * (0, 0, 1),
                     xn = -2 (x / W - 1/2) + offX, yn likewise;
  Euler model        S = (Rz(phi) Rx(theta + pi/2)) Ry(rho), toCameraSpace(v) = T^T S v;
                     origin = toCameraSpace(0, 0, -10) + xn s X + yn s Y, direction = toCameraSpace(0, 0, 1);
  per track          d normalised, R = sum (I - d d^T), q = sum (I - d d^T) o, the symmetric eigendecomposition of R,
                     eigenvalues with |lambda| <= 3 * 2^-52 * lambda_max dropped (Eigen's default rank cut of
                     bdcSvd().solve), x = sum v (v^T q) / lambda over the rest.
The generator tests/golden/make_tri_golden.py stores its results in tests/golden/tri_reference.npz; load() rebuilds a
case's inputs, asserts their SHA-256 against the stored one and returns both, so that the GPU tests need neither
mpmath nor the oracle.

Bound.  With n_j rays, lambda+min the smallest retained eigenvalue and o_k the origins of track j,
  A_j = n_j (max_k |o_k|_2 + |x_ref|_2) / lambda+min,      |x - x_ref|_inf <= tau 2^-53 A_j     for EVERY valid track.
q has n_j terms of size |o_k|, and the pseudo-inverse amplifies an error in q or in R x by 1 / lambda+min, so A_j
follows each track's conditioning.  oracle_ba_triangulate (plain double arithmetic) stays below 1.8 of 2^-53 A_j on
every case here, from benign scenes (errors of 1e-15) to rays spread by 1e-4 rad (errors of 1e-4): tau = 4 for it
(test_tri_cases_cpu.py).  TAU is the kernel's, measured on MI355X against the golden (test_triangulation_gpu.py).

Inputs are the same on any machine.  Pixel positions are float32 values widened, as synth.make_ba_scene stores
them.  Whatever else went through sin, cos or log -- camera parameters, start points -- is rounded to float32 and
widened as well (a quaternion is normalised again afterwards: +, *, / and sqrt round the same everywhere), so that a
last-bit difference between two libms cannot move an input and with it the hash.

Cases (both camera models unless said otherwise):
  benign               make_ba_scene(model, 9, 200, config_id=32, noise_px=0.3): the scene of test_ba_gpu.py
  lengths              260 ring cameras, 33 tracks: lengths 260, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 128,
                       129, 250 with a track of 0 or 1 observations between each two -- two workgroups of 16 octets
                       and one that holds a single octet; octets that return at once beside octets that loop 33 times
  single               M = 1, two rays
  near_parallel_1e-2, near_parallel_1e-4
                       8 cameras, copies of camera 0 rotated by that many radians of noise; 64 tracks of 2..5 views
  parallel_axis        6 cameras with one look direction, offsets, rolls and scales differ; 48 tracks of 2..5 views.
                       R has rank 2 and the answer is the minimum-norm point.  The direction is an exact axis --
                       quaternion (0, 0, sin a/2, cos a/2), Euler phi = 0, theta = 0 -- so that I - d d^T is exact in
                       double on any hardware
  non_unit_quat        (quaternion) 6 cameras x 64 tracks, every q scaled by a factor in [0.97, 1.03]: pins Eigen's
                       unnormalised expression and the normalisation of d
  intrinsics           6 cameras x 64 tracks, images of 1920 x 1080 and 3 x 5, offsets +-0.3, scales 0.37, 1 and 4,
                       pixel positions 0, negative and out of frame, points centred at (5, -3, 2)
  angles               (Euler) 6 cameras x 64 tracks, phi and rho up to +-100 rad, theta within 1e-3 of +-pi/2
For every valid track each reference eigenvalue ratio lambda_i / lambda_max is >= 1e-10 or < 1e-30 (the latter in
parallel_axis only): nothing sits where the rank decision is made at rounding level.

Why there is no case with exactly parallel rays in a generic direction: there the third eigenvalue of the double R is
rounding noise that sits AT the cut.  Over 20000 random orientations with 2..5 identical directions each, the noise
eigenvalue reached 1.00 x the cut 3 * 2^-52 * lambda_max when the products of d d^T are rounded separately and 1.07 x
with singly rounded (FMA-like) ones.  The kernel, the oracle and Eigen may each decide rank 2 or rank 3 on such a
track, and none would be wrong.  The cut is the reference project's; changing it is not this file's business.
"""
import hashlib
import os

import numpy as np

from orthosfm_amd import synth

U = 2.0 ** -53
TAU = 8                      # the kernel's: 4 x 1.62, the largest ratio seen on MI355X, rounded up to a power of two
TAU_TWIN = 4                 # oracle_ba_triangulate's (largest ratio seen: 1.71)
BITS = 200
BAND_LO, BAND_HI = 1e-30, 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_reference.npz")
SEED = synth.BASE_SEED
_ST = 0x7A1 << 32            # streams of synth's counter-based generator used here

Q, E = synth.MODEL_QUATERNION, synth.MODEL_EULER
CASES = {"benign": (Q, E), "lengths": (Q, E), "single": (Q, E), "near_parallel_1e-2": (Q, E),
         "near_parallel_1e-4": (Q, E), "parallel_axis": (Q, E), "non_unit_quat": (Q,), "intrinsics": (Q, E),
         "angles": (E,)}
ALL = [(name, model) for name, models in CASES.items() for model in models]
LENGTHS = (260, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 128, 129, 250)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _snap_cams(model, cams):
    """Camera parameters on the float32 grid; quaternions normalised again (sum of squares in a fixed order)."""
    cams = _f32(cams)
    if model == Q:
        q = cams[:, :4]
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        cams[:, :4] = q / n[:, None]
    return cams


def _const(model, C):
    """The constant masks of synth.make_ba_scene (they do not enter the triangulation)."""
    const = np.zeros((C, 7), dtype=np.uint8)
    if model == Q:
        const[:, 6] = 1
    else:
        const[:, 5:] = 1
    const[0, :] = 1
    return const


def _cams_from_euler(model, angles, off, scale):
    """(C, 7) parameters of cameras with the given (phi, theta, rho), offsets and scales, in either model."""
    C = len(angles)
    cams = np.zeros((C, 7))
    for c, (phi, theta, rho) in enumerate(angles):
        if model == Q:
            cams[c, :4] = synth.euler_to_quat(phi, theta, rho)
            cams[c, 4:6], cams[c, 6] = off[c], scale[c]
        else:
            cams[c, :3] = (phi, theta, rho)
            cams[c, 3:5], cams[c, 5] = off[c], scale[c]
    return _snap_cams(model, cams)


def _ring(model, C, stream, nphi=None):
    ang = synth.uniform(SEED, _ST | stream, 2 * C).reshape(C, 2)
    angles = [(2.0 * np.pi * c / (nphi or C), np.deg2rad(-30.0 + 60.0 * ang[c, 0]), np.deg2rad(-30.0 + 60.0 * ang[c, 1]))
              for c in range(C)]
    return _cams_from_euler(model, angles, np.zeros((C, 2)), np.ones(C))


def _ball(M, stream, centre=(0.0, 0.0, 0.0)):
    d = synth.normal(SEED, _ST | stream, 3 * M).reshape(M, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (0.5 * np.cbrt(synth.uniform(SEED, _ST | (stream + 1), M)))[:, None] + np.asarray(centre)


def _arcs(lengths, C, stream):
    """Per track a contiguous arc of cameras on the ring of C, starting at a drawn camera."""
    first = np.floor(synth.uniform(SEED, _ST | stream, len(lengths)) * C).astype(np.int64)
    return [(first[j] + np.arange(n)) % C for j, n in enumerate(lengths)]


def _scene(model, cams, img_w, img_h, pts, track_cams, noise_px, stream, proj_cams=None):
    """Observations: the points projected by proj_cams (default: cams) plus noise, through float32; tracks in order.
    Start points are distinct per track and never a result, so that a point that must keep its bytes shows it."""
    C, M = cams.shape[0], pts.shape[0]
    proj = cams if proj_cams is None else proj_cams
    ln = np.array([len(t) for t in track_cams], dtype=np.int64)
    obs_point = np.repeat(np.arange(M), ln)
    obs_camera = np.concatenate([np.asarray(t, dtype=np.int64) for t in track_cams] + [np.zeros(0, dtype=np.int64)])
    O = obs_point.size
    xy = np.zeros((O, 2))
    for c in range(C):
        sel = np.nonzero(obs_camera == c)[0]
        if sel.size:
            xy[sel] = synth._project(model, proj[c], pts[obs_point[sel]], int(img_w[c]), int(img_h[c]))
    if noise_px and O:
        xy += noise_px * synth.normal(SEED, _ST | stream, 2 * O).reshape(O, 2)
    xy = _f32(xy)
    P = np.empty((M, 4))
    j = np.arange(M, dtype=np.float64)
    P[:, 0], P[:, 1], P[:, 2], P[:, 3] = 100.5 + j, -0.25 * j - 7.0, 3.0, 1.5
    return synth.BaScene(model, cams.copy(), _const(model, C), np.asarray(img_w, dtype=np.int32),
                         np.asarray(img_h, dtype=np.int32), P, xy, obs_camera.astype(np.int32),
                         obs_point.astype(np.int32), cams.copy(), pts.copy())


def _sizes(C, w=2048, h=2048):
    return np.full(C, w, dtype=np.int32), np.full(C, h, dtype=np.int32)


def _benign(model):
    sc = synth.make_ba_scene(model, 9, 200, config_id=32, noise_px=0.3)
    sc.cam_params = _snap_cams(model, sc.cam_params)
    sc.points = _f32(sc.points)
    return sc


def _lengths(model):
    C = 260
    cams = _ring(model, C, 0x10)
    ln = []
    for i, n in enumerate(LENGTHS):
        ln.append(n)
        if i + 1 < len(LENGTHS):
            ln.append(i % 2)                 # a track of 0 or of 1 observations between each two
    assert len(ln) == 33
    return _scene(model, cams, *_sizes(C), _ball(len(ln), 0x12), _arcs(ln, C, 0x14), 0.3, 0x15)


def _single(model):
    cams = _ring(model, 2, 0x20, nphi=5)
    return _scene(model, cams, *_sizes(2), _ball(1, 0x22), [np.array([0, 1])], 0.3, 0x25)


def _near_parallel(model, spread, stream):
    C, M = 8, 64
    base = (0.3, 0.2, -0.1)
    nz = synth.normal(SEED, _ST | stream, 3 * C).reshape(C, 3) * spread
    cams = np.zeros((C, 7))
    if model == Q:
        q0 = synth.euler_to_quat(*base)
        for c in range(C):
            a = np.linalg.norm(nz[c])
            dq = np.array([*(np.sin(a / 2) * nz[c] / a), np.cos(a / 2)])
            cams[c, :4] = synth.quat_mul(dq, q0) if c else q0
        cams[:, 6] = 1.0
    else:
        for c in range(C):
            cams[c, :3] = np.array(base) + (nz[c] if c else 0.0)
        cams[:, 5] = 1.0
    cams = _snap_cams(model, cams)
    ln = [2 + j % 4 for j in range(M)]
    return _scene(model, cams, *_sizes(C), _ball(M, stream + 1), _arcs(ln, C, stream + 3), 0.3, stream + 4)


def _parallel_axis(model):
    C, M = 6, 48
    roll = np.array([0.0, 0.7, -1.3, 2.9, 0.2, -2.2])
    off = np.array([[0.0, 0.0], [0.2, -0.1], [-0.15, 0.05], [0.1, 0.2], [-0.2, -0.2], [0.05, 0.15]])
    scale = np.array([1.0, 0.8, 1.25, 1.0, 1.25, 0.8])
    cams = np.zeros((C, 7))
    if model == Q:
        cams[:, 2], cams[:, 3] = np.sin(roll / 2), np.cos(roll / 2)
        cams[:, 4:6], cams[:, 6] = off, scale
    else:
        cams[:, 2] = roll                    # phi = 0, theta = 0
        cams[:, 3:5], cams[:, 5] = off, scale
    cams = _snap_cams(model, cams)
    ln = [2 + j % 4 for j in range(M)]
    return _scene(model, cams, *_sizes(C), _ball(M, 0x52), _arcs(ln, C, 0x54), 0.3, 0x55)


def _non_unit_quat(model):
    assert model == Q
    C, M = 6, 64
    unit = _ring(model, C, 0x60)
    f = _f32(0.97 + 0.06 * synth.uniform(SEED, _ST | 0x61, C))
    f[0], f[1] = _f32(0.97), _f32(1.03)
    cams = unit.copy()
    cams[:, :4] = unit[:, :4] * f[:, None]
    ln = [2 + j % 5 for j in range(M)]
    return _scene(model, cams, *_sizes(C), _ball(M, 0x62), _arcs(ln, C, 0x64), 0.3, 0x65, proj_cams=unit)


def _intrinsics(model):
    C, M = 6, 64
    ang = synth.uniform(SEED, _ST | 0x70, 2 * C).reshape(C, 2)
    angles = [(2.0 * np.pi * c / C, np.deg2rad(-30.0 + 60.0 * ang[c, 0]), np.deg2rad(-30.0 + 60.0 * ang[c, 1]))
              for c in range(C)]
    off = 0.3 * np.array([[1, -1], [-1, 1], [1, 1], [-1, -1], [1, 0], [0, -1]], dtype=np.float64)
    scale = np.array([0.37, 1.0, 4.0, 4.0, 0.37, 1.0])
    cams = _cams_from_euler(model, angles, off, scale)
    w = np.array([1920, 3, 1920, 3, 3, 1920], dtype=np.int32)
    h = np.array([1080, 5, 1080, 5, 5, 1080], dtype=np.int32)
    ln = [2 + j % 5 for j in range(M)]
    sc = _scene(model, cams, w, h, _ball(M, 0x72, centre=(5.0, -3.0, 2.0)), _arcs(ln, C, 0x74), 0.3, 0x75)
    # positions a detector never gives: the origin, negative, far out of frame
    fixed = np.array([[0.0, 0.0], [-7.5, 3.0], [2500.0, -40.0], [0.0, 1079.0], [-0.0, 5.0], [1e6, 1e6]])
    sc.obs_xy[3:3 + 6 * 7:7] = fixed
    return sc


def _angles(model):
    assert model == E
    C, M = 6, 64
    u = synth.uniform(SEED, _ST | 0x80, 4 * C).reshape(C, 4)
    cams = np.zeros((C, 7))
    cams[:, 0] = -100.0 + 200.0 * u[:, 0]
    cams[:, 2] = -100.0 + 200.0 * u[:, 1]
    cams[0, 0], cams[1, 2] = 100.0, -100.0
    sign = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    cams[:, 1] = sign * 0.5 * np.pi + 1e-3 * (2.0 * u[:, 2] - 1.0)
    cams[:, 5] = 1.0
    cams = _snap_cams(model, cams)
    assert (np.abs(np.abs(cams[:, 1]) - 0.5 * np.pi) <= 1e-3).all()
    ln = [2 + j % 5 for j in range(M)]
    return _scene(model, cams, *_sizes(C), _ball(M, 0x82), _arcs(ln, C, 0x84), 0.3, 0x85)


_BUILDERS = {"benign": _benign, "lengths": _lengths, "single": _single,
             "near_parallel_1e-2": lambda m: _near_parallel(m, 1e-2, 0x30),
             "near_parallel_1e-4": lambda m: _near_parallel(m, 1e-4, 0x40),
             "parallel_axis": _parallel_axis, "non_unit_quat": _non_unit_quat, "intrinsics": _intrinsics,
             "angles": _angles}


def build(name, model):
    """The inputs of a case as a synth.BaScene (observations grouped by track, tracks in order)."""
    assert model in CASES[name], (name, model)
    sc = _BUILDERS[name](model)
    assert (np.diff(sc.obs_point) >= 0).all()
    return sc


def input_hash(sc):
    h = hashlib.sha256()
    h.update(np.array([sc.model, sc.cam_params.shape[0], sc.points.shape[0], sc.obs_xy.shape[0]], dtype=np.int64).tobytes())
    for a, t in ((sc.cam_params, np.float64), (sc.img_w, np.int32), (sc.img_h, np.int32), (sc.points, np.float64),
                 (sc.obs_xy, np.float64), (sc.obs_camera, np.int32), (sc.obs_point, np.int32)):
        h.update(np.ascontiguousarray(a, dtype=t).tobytes())
    return h.hexdigest()


def track_lengths(sc):
    return np.bincount(sc.obs_point, minlength=sc.points.shape[0])


# ---------------------------------------------------------------------------
# reference (mpmath)
# ---------------------------------------------------------------------------

def _mp():
    import mpmath
    return mpmath


def _camera_frames(sc, mp):
    """Per camera, in mpmath: the images X, Y, Z of the local axes (origin = s xn X + s yn Y - 10 Z, direction = Z),
    offsets, scale and image size."""
    f = mp.mpf
    out = []
    for c in range(sc.cam_params.shape[0]):
        p = [f(float(v)) for v in sc.cam_params[c]]
        if sc.model == Q:
            u, w = p[:3], p[3]

            def cross(a, b):
                return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

            def rot(v):
                t = [2 * x for x in cross(u, v)]
                ut = cross(u, t)
                return [v[i] + w * t[i] + ut[i] for i in range(3)]
            X, Y, Z = rot([f(1), f(0), f(0)]), rot([f(0), f(1), f(0)]), rot([f(0), f(0), f(1)])
            off, s = (p[4], p[5]), p[6]
        else:
            phi, om, rho = p[0], p[1] + f(0.5 * np.pi), p[2]
            Ry = mp.matrix([[mp.cos(rho), -mp.sin(rho), 0], [mp.sin(rho), mp.cos(rho), 0], [0, 0, 1]])
            Rx = mp.matrix([[1, 0, 0], [0, mp.cos(om), -mp.sin(om)], [0, mp.sin(om), mp.cos(om)]])
            Rz = mp.matrix([[mp.cos(phi), -mp.sin(phi), 0], [mp.sin(phi), mp.cos(phi), 0], [0, 0, 1]])
            S = (Rz * Rx) * Ry

            def tcs(k):                      # T^T S e_k with T = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
                return [S[0, k], S[2, k], -S[1, k]]
            X, Y, Z = tcs(0), tcs(1), tcs(2)
            off, s = (p[3], p[4]), p[5]
        out.append((X, Y, Z, off, s, f(int(sc.img_w[c])), f(int(sc.img_h[c]))))
    return out


def _ray(fr, x, y, mp):
    X, Y, Z, off, s, W, H = fr
    xn = -2 * (mp.mpf(float(x)) / W - mp.mpf(0.5)) + off[0]
    yn = -2 * (mp.mpf(float(y)) / H - mp.mpf(0.5)) + off[1]
    return [s * xn * X[i] + s * yn * Y[i] - 10 * Z[i] for i in range(3)], Z


def rays(sc, ks, bits=BITS):
    """The reference's origin and (unnormalised) direction of the observations ks, rounded to float64."""
    mp = _mp()
    with mp.workprec(bits):
        fr = _camera_frames(sc, mp)
        o = np.zeros((len(ks), 3))
        d = np.zeros((len(ks), 3))
        for i, k in enumerate(ks):
            oo, dd = _ray(fr[int(sc.obs_camera[k])], sc.obs_xy[k, 0], sc.obs_xy[k, 1], mp)
            o[i], d[i] = [float(v) for v in oo], [float(v) for v in dd]
    return o, d


def reference(sc, bits=BITS):
    """points (M, 3) float64, A (M,), ratios (M, 3) = |lambda_i| / lambda_max in descending order, valid (M,) uint8.
    Rows of tracks with fewer than two rays are zero."""
    mp = _mp()
    M = sc.points.shape[0]
    pts, A, ratios, valid = np.zeros((M, 3)), np.zeros(M), np.zeros((M, 3)), np.zeros(M, dtype=np.uint8)
    start = np.concatenate([[0], np.cumsum(track_lengths(sc))])
    with mp.workprec(bits):
        fr = _camera_frames(sc, mp)
        proj = []
        for X, Y, Z, *_ in fr:
            n = mp.sqrt(Z[0] * Z[0] + Z[1] * Z[1] + Z[2] * Z[2])
            d = [z / n for z in Z]
            proj.append([[(1 if a == b else 0) - d[a] * d[b] for b in range(3)] for a in range(3)])
        cut = 3 * mp.mpf(2) ** -52
        for j in range(M):
            k0, k1 = int(start[j]), int(start[j + 1])
            if k1 - k0 < 2:
                continue
            R = mp.zeros(3, 3)
            q = [mp.mpf(0)] * 3
            omax = mp.mpf(0)
            for k in range(k0, k1):
                c = int(sc.obs_camera[k])
                o, _ = _ray(fr[c], sc.obs_xy[k, 0], sc.obs_xy[k, 1], mp)
                P = proj[c]
                for a in range(3):
                    for b in range(3):
                        R[a, b] += P[a][b]
                    q[a] = q[a] + P[a][0] * o[0] + P[a][1] * o[1] + P[a][2] * o[2]
                omax = max(omax, mp.sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]))
            lam, V = mp.eigsy(R)
            lmax = max(abs(lam[i]) for i in range(3))
            x = [mp.mpf(0)] * 3
            lmin = None
            for i in range(3):
                if abs(lam[i]) <= cut * lmax:
                    continue
                cf = (V[0, i] * q[0] + V[1, i] * q[1] + V[2, i] * q[2]) / lam[i]
                x = [x[a] + cf * V[a, i] for a in range(3)]
                lmin = abs(lam[i]) if lmin is None else min(lmin, abs(lam[i]))
            xn = mp.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
            pts[j] = [float(v) for v in x]
            A[j] = float((k1 - k0) * (omax + xn) / lmin)
            ratios[j] = sorted((float(abs(lam[i]) / lmax) for i in range(3)), reverse=True)
            valid[j] = 1
    return {"points": pts, "A": A, "ratios": ratios, "valid": valid}


# ---------------------------------------------------------------------------
# golden and check
# ---------------------------------------------------------------------------

def key(name, model):
    return f"{name}/{'quat' if model == Q else 'euler'}"


_golden = None


def golden(name, model):
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    k = key(name, model)
    g = {f: _golden[f"{k}/{f}"] for f in ("points", "A", "ratios", "valid")}
    g["sha256"] = str(_golden[f"{k}/sha256"])
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def load(name, model):
    """(scene, golden) of a case; the scene is rebuilt and must hash to what the golden was made from."""
    sc = build(name, model)
    g = golden(name, model)
    assert input_hash(sc) == g["sha256"], f"{key(name, model)}: inputs differ from those of tests/golden/tri_reference.npz"
    return sc, g


def ratios(points, g):
    """|x - x_ref|_inf / (2^-53 A_j) per track; 0 on invalid tracks, inf where a valid point is not finite."""
    x = np.asarray(points, dtype=np.float64)[:, :3]
    err = np.abs(x - g["points"]).max(axis=1)
    r = np.where(err == 0, 0.0, err / (U * np.where(g["A"] > 0, g["A"], 1.0)))
    r = np.where(np.isfinite(x).all(axis=1), r, np.inf)
    return np.where(g["valid"].astype(bool), r, 0.0)


def worst(points, g):
    """(largest ratio, its track)."""
    r = ratios(points, g)
    j = int(np.argmax(r)) if r.size else 0
    return (float(r[j]) if r.size else 0.0), j


def check(points, g, tau=None):
    """True when every valid track is within tau 2^-53 A_j of the reference."""
    return worst(points, g)[0] <= (TAU if tau is None else tau)


def scene_from_ba_scene(sc, device=0):
    """A device-resident scene whose track table is the case's observation list (as test_e2e_gpu.py builds one)."""
    from orthosfm_amd.scene import Scene
    offs = np.concatenate([[0], np.cumsum(track_lengths(sc))]).astype(np.int64)
    return Scene(sc.model, sc.img_w, sc.img_h, offs, sc.obs_camera, sc.obs_xy.astype(np.float32), device)
