"""A reference of one linearisation of the bundle adjustment, in extended precision, and the checker that holds what
the solve's kernels computed (ba.debug_linearization: the first LM iteration of osfm_ba_solve) against it.

The reference starts from the oracle's evaluate() (oracle/ba_oracle.c, oracle_lib.oracle_ba_linearize): per
observation the Huber-corrected residual r and the tangent Jacobian blocks Jc (2 x 6) and Jp (2 x 3), unscaled, from
the oracle's jets -- independent of the kernels' hand-derived Jacobians.  From there everything is np.longdouble
(64-bit mantissa): the Jacobi scales, the LM diagonals clamped to [min_lm_diagonal, max_lm_diagonal] and divided by
the radius, V_j and V_j^-1, S = U + D^2 - sum_j W_j V_j^-1 W_j^T and its rhs, then -- from the GPU's own camera step
y_c, so that the factorisation's error does not enter -- the point steps, the candidate points and cameras (through
the oracle's homog_plus / quat_plus), the model cost change -(g^T h + h^T J^T J h / 2), the candidate cost and the
relative decrease.  The Schur products are formed per track, tracks grouped by length.

Every quantity q is checked componentwise: |q_gpu - q_ref| <= tau_q u A_q, u = 2^-53, A_q the same expression
evaluated on absolute values.  The Jacobian both sides start from is a float64 value computed by another formula
(jets against hand-derived derivatives, with cancellations in the rotation columns), so |J| is taken with a floor:
an entry counts as at least its observation's largest camera (point) entry times its column's scale, and a residual
as at least sqrt(rho') (|x_obs| + 1) -- a residual is the difference of two pixel positions.  Where V_j^-1 enters,
|V_j^-1| is replaced by |V_j^-1| + |V_j^-1| A_V |V_j^-1|, the first-order error of the inverse (kappa(V_j) in it).
The camera step is checked by its residual: |S y - rhs| <= tau u ((A_S + |S|)|y| + A_rhs + |rhs| + n max(|S||y|)).

What this can see in S: the floor and the kappa term make A_S much larger than |S|.  tau u A_S / |S| is about 5e-10
on the diagonal and 3e-9 (median; 2e-8 at the 90th percentile) off it for a 3-camera problem with 2500 tracks, 3e-9
and 2e-8 (up to 2e-6 for the smallest entries) for a ring of 200 cameras with 20000 tracks.  So a relative error of
1e-10 in one block of S passes unseen; one entry of a pair list dropped, a chunk lost or added twice, a missing or
one-sided scale, a missing D^2 -- errors of 1e-4 and more of the entries they touch -- do not (test_lin_cases_cpu.py).
V_j^-1 itself is checked on its own to 64 u |V_j^-1| A_V |V_j^-1|: an error of 1e-9 there is seen directly.

One tau per quantity, for every case (TAU below):
  ge, vinv                       64        S, rhs             256
  diag                           256       scale              1024
  y_c (residual)                 256       candidate points   256, candidate cameras 64
  model cost change              1024      costs (initial, candidate), gradient norm, relative decrease  1024
The Jacobi scales 1 / (1 + |column|) and, without Jacobi scaling, the LM diagonals are the only quantities made from
the unscaled column sums of squares; there the two Jacobian formulas differ by more than the floor allows for (on
MI355X the point columns' sums of squares differed from the oracle's by up to 3e-13 relative: scale_p reached 533 u A
where every other quantity stayed below 60 u A), hence their larger taus.
"""
import numpy as np

import oracle_lib

U = 2.0 ** -53
LD = np.longdouble
TAU = {"scale_c": 1024, "scale_p": 1024, "diag_c": 256, "diag_p": 256, "ge": 64, "vinv": 64, "S": 256, "rhs": 256,
       "y_c": 256, "cand_points": 256, "cand_cams": 64, "model_cost_change": 1024, "initial_cost": 1024,
       "cand_cost": 1024, "grad_max": 1024, "relative_decrease": 1024}
OPTION_DEFAULTS = {"huber_delta": 1.0, "optimize_points": 1, "initial_trust_region_radius": 1e4, "min_lm_diagonal": 1e-6,
                   "max_lm_diagonal": 1e32, "jacobi_scaling": 1, "min_relative_decrease": 1e-3, "function_tolerance": 1e-6}
_BATCH = 1 << 18          # Schur products formed per batch (blocks of 6 x 6)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def options(**kw):
    o = dict(OPTION_DEFAULTS)
    o.update(kw)
    return o


def inv3(V):
    """Inverses of a stack of 3 x 3 matrices by the adjugate (any float type, longdouble included)."""
    a, b, c = V[..., 0, 0], V[..., 0, 1], V[..., 0, 2]
    d, e, f = V[..., 1, 0], V[..., 1, 1], V[..., 1, 2]
    g, h, i = V[..., 2, 0], V[..., 2, 1], V[..., 2, 2]
    A = e * i - f * h
    B = -(d * i - f * g)
    Cc = d * h - e * g
    det = a * A + b * B + c * Cc
    adj = np.stack([np.stack([A, -(b * i - c * h), b * f - c * e], -1),
                    np.stack([B, a * i - c * g, -(a * f - c * d)], -1),
                    np.stack([Cc, -(a * h - b * g), a * e - b * d], -1)], -2)
    return adj / det[..., None, None]


class Layout:
    """The cameras' tangent columns and the tracks of a scene."""

    def __init__(self, sc, lin):
        self.C, self.M, self.O = sc.cam_params.shape[0], sc.points.shape[0], sc.obs_camera.shape[0]
        self.off, self.ldim = lin["cam_off"], lin["cam_ldim"]
        self.nc = int(self.ldim.sum())
        self.cam = sc.obs_camera.astype(np.int64)
        self.pt = sc.obs_point.astype(np.int64)
        t = np.arange(6)
        self.mask = t[None, :] < self.ldim[self.cam][:, None]                      # (O, 6)
        self.cols = np.where(self.mask, self.off[self.cam][:, None] + t[None, :], 0)
        self.col_cam = np.repeat(np.arange(self.C), self.ldim)                   # (nc,)
        self.col_t = np.arange(self.nc) - self.off[self.col_cam]
        self.pt_start = np.zeros(self.M + 1, dtype=np.int64)
        np.add.at(self.pt_start, self.pt + 1, 1)
        self.pt_start = np.cumsum(self.pt_start)
        self.length = np.diff(self.pt_start)


def _col_sum(L, v):
    """(O, 6) per-observation values -> (nc,) sums over the camera columns."""
    out = np.zeros(L.nc, dtype=v.dtype)
    np.add.at(out, L.cols[L.mask], v[L.mask])
    return out


def _pt_sum(L, v):
    out = np.zeros((L.M,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, L.pt, v)
    return out


def _schur_blocks(L, Jc, Jp, Mid, out, sign=-1):
    """out (C, C, 6, 6) += sign * sum over tracks j and observation pairs (a, b) of j of Jc_a^T Jp_a Mid_j Jp_b^T Jc_b, the
    tracks grouped by length and the products of a batch reduced per camera pair (sorted keys, reduceat)."""
    C = L.C
    flat = out.reshape(C * C, 6, 6)
    for ln in np.unique(L.length[L.length > 0]):
        tracks = np.nonzero(L.length == ln)[0]
        step = max(1, _BATCH // int(ln * ln))
        for t0 in range(0, tracks.size, step):
            tr = tracks[t0:t0 + step]
            K = L.pt_start[tr][:, None] + np.arange(ln)[None, :]                 # (B, ln)
            jc, jp = Jc[K], Jp[K]                                                 # (B, ln, 2, 6), (B, ln, 2, 3)
            Q = np.einsum("blrx,bxy->blry", jp, Mid[tr])                          # Jp_a Mid
            Mab = np.einsum("blrx,bmsx->blmrs", Q, jp)                            # Jp_a Mid Jp_b^T (2 x 2)
            T = np.einsum("blmrs,bmsy->blmry", Mab, jc)
            blk = np.einsum("blrx,blmry->blmxy", jc, T).reshape(-1, 6, 6)
            cams = L.cam[K]
            keys = (cams[:, :, None] * C + cams[:, None, :]).reshape(-1)
            order = np.argsort(keys, kind="stable")
            ks = keys[order]
            starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
            flat[ks[starts]] += sign * np.add.reduceat(blk[order], starts, axis=0)


def _assemble(L, blocks, dtype):
    """(C, C, 6, 6) blocks -> the nc x nc matrix of the free columns."""
    return blocks[L.col_cam[:, None], L.col_cam[None, :], L.col_t[:, None], L.col_t[None, :]].astype(dtype)


def _huber_cost(raw, huber):
    s = (raw.astype(LD) ** 2).sum(1)
    b = LD(huber) ** 2
    return LD(0.5) * np.where(s > b, 2 * LD(huber) * np.sqrt(s) - b, s).sum(), s


def _plus_cams(sc, L, dc):
    """The oracle's plus_all on the cameras: quaternion rotation block through quat_plus, other columns added."""
    cams = sc.cam_params
    out = cams.copy()
    ccols = np.zeros((L.C, 6))
    ccols[L.col_cam, L.col_t] = dc
    if sc.model == 0:
        rot = sc.cam_const[:, 0] == 0
        if rot.any():
            out[rot, :4] = oracle_lib.oracle_plus("quat", cams[rot, :4], ccols[rot, :3])
        slots = [[s for s in (4, 5, 6) if not sc.cam_const[c, s]] for c in range(L.C)]
        first = np.where(rot, 3, 0)
    else:
        slots = [[s for s in range(6) if not sc.cam_const[c, s]] for c in range(L.C)]
        first = np.zeros(L.C, dtype=np.int64)
    for c in range(L.C):
        for i, s in enumerate(slots[c]):
            out[c, s] = cams[c, s] + ccols[c, first[c] + i]
    return out


def _scaled_floor(sc, L, lin, scale_c, scale_p):
    """|J| with the floor of the module docstring (float64), scaled; and the residual magnitudes."""
    Jc, Jp, r = lin["Jc"], lin["Jp"], lin["r"]
    mc = np.abs(Jc).max(axis=(1, 2))
    mp = np.abs(Jp).max(axis=(1, 2))
    sc_obs = np.where(L.mask, scale_c.astype(np.float64)[L.cols], 0.0)            # (O, 6)
    sp_obs = scale_p.astype(np.float64)[L.pt]                                     # (O, 3)
    Jch = (np.abs(Jc) + mc[:, None, None]) * sc_obs[:, None, :] * L.mask[:, None, :]
    Jph = (np.abs(Jp) + mp[:, None, None]) * sp_obs[:, None, :]
    raw, _ = oracle_lib.oracle_ba_residuals(sc)
    nraw = np.sqrt((raw ** 2).sum(1))
    nr = np.sqrt((r ** 2).sum(1))
    sq = np.where(nraw > 0, nr / np.where(nraw > 0, nraw, 1.0), 1.0)
    rh = np.abs(r) + sq[:, None] * (np.abs(sc.obs_xy) + 1.0)
    return Jch, Jph, rh


def reference(sc, opt, lin=None):
    """The linearisation at the scene's cameras and points (opt: options()); a dict of reference values (longdouble)
    and their bounds A (float64), in the cameras' own order."""
    o = options(**opt)
    if lin is None:
        lin = oracle_lib.oracle_ba_linearize(sc, huber_delta=o["huber_delta"], optimize_points=o["optimize_points"])
    L = Layout(sc, lin)
    pdim = 3 if o["optimize_points"] else 0
    R = LD(o["initial_trust_region_radius"])
    Jc0, Jp0, r = lin["Jc"].astype(LD), lin["Jp"].astype(LD), lin["r"].astype(LD)
    # Jacobi scales from the unscaled column norms
    colsq_c = _col_sum(L, (Jc0 ** 2).sum(1))
    colsq_p = _pt_sum(L, (Jp0 ** 2).sum(1))
    if o["jacobi_scaling"]:
        scale_c, scale_p = 1 / (1 + np.sqrt(colsq_c)), 1 / (1 + np.sqrt(colsq_p))
    else:
        scale_c, scale_p = np.ones(L.nc, dtype=LD), np.ones((L.M, 3), dtype=LD)
    if not pdim:
        scale_p = np.ones((L.M, 3), dtype=LD)
    Jc = Jc0 * np.where(L.mask, scale_c[L.cols], 0)[:, None, :]
    Jp = Jp0 * scale_p[L.pt][:, None, :]
    Jch, Jph, rh = _scaled_floor(sc, L, lin, scale_c, scale_p)
    ref, A = {}, {}
    colh_c = _col_sum(L, ((np.abs(lin["Jc"]) + np.abs(lin["Jc"]).max(axis=(1, 2))[:, None, None]) ** 2).sum(1) * L.mask)
    colh_p = _pt_sum(L, ((np.abs(lin["Jp"]) + np.abs(lin["Jp"]).max(axis=(1, 2))[:, None, None]) ** 2).sum(1))
    ref["scale_c"], ref["scale_p"] = scale_c, scale_p
    A["scale_c"] = f64(scale_c) + f64(scale_c) ** 2 * colh_c / (2 * np.sqrt(f64(colsq_c)) + 1e-300) * (f64(colsq_c) > 0)
    A["scale_p"] = f64(scale_p) + f64(scale_p) ** 2 * colh_p / (2 * np.sqrt(f64(colsq_p)) + 1e-300) * (f64(colsq_p) > 0)
    if not o["jacobi_scaling"]:
        A["scale_c"] = np.ones(L.nc)
    if not o["jacobi_scaling"] or not pdim:
        A["scale_p"] = np.ones((L.M, 3))
    # LM diagonals
    lo, hi = LD(o["min_lm_diagonal"]), LD(o["max_lm_diagonal"])
    dsum_c = _col_sum(L, (Jc ** 2).sum(1))
    dsum_p = _pt_sum(L, (Jp ** 2).sum(1))
    diag_c, diag_p = np.clip(dsum_c, lo, hi), np.clip(dsum_p, lo, hi)
    ref["diag_c"], ref["diag_p"] = diag_c, diag_p
    A["diag_c"] = _col_sum(L, (Jch ** 2).sum(1)) + f64(diag_c)
    A["diag_p"] = _pt_sum(L, (Jph ** 2).sum(1)) + f64(diag_p)
    # cameras' blocks U = sum Jc^T Jc (+ D^2 on the diagonal), rhs = sum Jc^T r
    blocks = np.zeros((L.C, L.C, 6, 6), dtype=LD)
    ablocks = np.zeros((L.C, L.C, 6, 6))
    ii = np.arange(L.C)
    dblk = _pt_sum_cam(L, np.einsum("krx,kry->kxy", Jc, Jc))
    blocks[ii, ii] += dblk
    ablocks[ii, ii] += _pt_sum_cam(L, np.einsum("krx,kry->kxy", Jch, Jch))
    rhs = _col_sum(L, np.einsum("krx,kr->kx", Jc, r))
    A_rhs = _col_sum(L, np.einsum("krx,kr->kx", Jch, rh))
    if pdim:
        V = _pt_sum(L, np.einsum("krx,kry->kxy", Jp, Jp))
        V[:, [0, 1, 2], [0, 1, 2]] += diag_p / R
        g = _pt_sum(L, np.einsum("krx,kr->kx", Jp, r))
        Vi = inv3(V)
        AV = _pt_sum(L, np.einsum("krx,kry->kxy", Jph, Jph))
        AV[:, [0, 1, 2], [0, 1, 2]] += f64(diag_p) / float(R)
        aVi = np.abs(f64(Vi))
        B = aVi + aVi @ AV @ aVi
        gh = _pt_sum(L, np.einsum("krx,kr->kx", Jph, rh))
        ref["vinv"], ref["ge"], A["vinv"], A["ge"] = Vi, g, B, gh
        _schur_blocks(L, Jc, Jp, Vi, blocks)
        _schur_blocks(L, Jch, Jph, B, ablocks, sign=1)
        qg = np.einsum("krx,kxy,ky->kr", Jp, Vi[L.pt], g[L.pt])                  # Q g per observation
        rhs -= _col_sum(L, np.einsum("krx,kr->kx", Jc, qg))
        A_rhs += _col_sum(L, np.einsum("krx,kr->kx", Jch, np.einsum("krx,kxy,ky->kr", Jph, B[L.pt], gh[L.pt])))
    S = _assemble(L, blocks, LD)
    AS = np.abs(_assemble(L, ablocks, np.float64))
    S[np.arange(L.nc), np.arange(L.nc)] += diag_c / R
    AS[np.arange(L.nc), np.arange(L.nc)] += f64(diag_c) / float(R)
    ref["S"], ref["rhs"], A["S"], A["rhs"] = S, rhs, AS, A_rhs
    # the cost and the gradient norm at the start
    raw, _ = oracle_lib.oracle_ba_residuals(sc)
    cost, s = _huber_cost(raw, o["huber_delta"])
    ref["initial_cost"] = cost
    A["initial_cost"] = float((s + 2 * np.sqrt(s) * (np.abs(sc.obs_xy).sum(1) + 1)).sum())
    gc = _col_sum(L, np.einsum("krx,kr->kx", Jc0, r))
    gp = _pt_sum(L, np.einsum("krx,kr->kx", Jp0, r))
    gm = np.abs(_plus_cams(sc, L, -f64(gc)) - sc.cam_params)
    gm = gm[_active_cam_slots(sc)].max(initial=0.0)
    if pdim and L.M:
        gm = max(gm, np.abs(oracle_lib.oracle_plus("homog", sc.points, -f64(gp)) - sc.points).max())
    ref["grad_max"] = LD(gm)
    agc = _col_sum(L, np.einsum("krx,kr->kx", np.abs(lin["Jc"]) + np.abs(lin["Jc"]).max(axis=(1, 2))[:, None, None], rh) * L.mask)
    A["grad_max"] = float(max(agc.max(initial=0.0), np.abs(sc.cam_params).max(initial=0.0), np.abs(sc.points).max(initial=0.0)))
    return {"ref": ref, "A": A, "L": L, "lin": lin, "opt": o, "Jc": Jc, "Jp": Jp, "r": r, "Jch": Jch, "Jph": Jph,
            "rh": rh, "pdim": pdim}


def _pt_sum_cam(L, v):
    out = np.zeros((L.C,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, L.cam, v)
    return out


def _active_cam_slots(sc):
    """Ambient camera coordinates of the non-constant blocks (the norms of the LM control)."""
    cc = sc.cam_const
    if sc.model == 0:
        act = np.zeros(cc.shape, dtype=bool)
        act[:, :4] = (cc[:, 0] == 0)[:, None]
        act[:, 4:] = cc[:, 4:] == 0
    else:
        act = np.zeros(cc.shape, dtype=bool)
        act[:, :6] = cc[:, :6] == 0
    return act


def step_reference(sc, R, y_c):
    """The step of the first iteration from the GPU's camera step y_c: point steps, candidates, model cost change,
    candidate cost (at the candidate given) -- appended to R["ref"] / R["A"]."""
    L, o, ref, A = R["L"], R["opt"], R["ref"], R["A"]
    y = y_c.astype(LD)
    yo = np.where(L.mask, y[L.cols], 0)                                          # (O, 6)
    u = np.einsum("krx,kx->kr", R["Jc"], yo)                                     # Jc y per observation
    uh = np.einsum("krx,kx->kr", R["Jch"], np.abs(f64(yo)))
    if R["pdim"]:
        t3 = ref["ge"] - _pt_sum(L, np.einsum("krx,kr->kx", R["Jp"], u))
        step_p = -np.einsum("jxy,jy->jx", ref["vinv"], t3)
        t3h = A["ge"] + _pt_sum(L, np.einsum("krx,kr->kx", R["Jph"], uh))
        A_step = np.einsum("jxy,jy->jx", A["vinv"], t3h)
        dl = step_p * ref["scale_p"]
        A_dl = A_step * f64(ref["scale_p"]) + np.abs(f64(step_p)) * A["scale_p"]
        ref["cand_points"] = oracle_lib.oracle_plus("homog", sc.points, f64(dl)) if L.M else sc.points.copy()
        A["cand_points"] = np.linalg.norm(sc.points, axis=1)[:, None] * (1 + A_dl.sum(1))[:, None] * np.ones((1, 4))
        m = -u + np.einsum("krx,kx->kr", R["Jp"], step_p[L.pt])
        mh = uh + np.einsum("krx,kx->kr", R["Jph"], np.abs(f64(step_p))[L.pt] + A_step[L.pt])
    else:
        step_p = np.zeros((L.M, 3), dtype=LD)
        ref["cand_points"] = sc.points.copy()
        A["cand_points"] = np.linalg.norm(sc.points, axis=1)[:, None] * np.ones((1, 4))
        m, mh = -u, uh
    ref["step_p"] = step_p
    ref["cand_cams"] = _plus_cams(sc, L, -f64(y * ref["scale_c"]))
    yc_mag = np.zeros(L.C)
    np.add.at(yc_mag, L.col_cam, np.abs(f64(y)) * (f64(ref["scale_c"]) + A["scale_c"]))
    A["cand_cams"] = (np.linalg.norm(sc.cam_params, axis=1) + yc_mag)[:, None] * np.ones((1, 7))
    ref["model_cost_change"] = -(m * (R["r"] + m / 2)).sum()
    A["model_cost_change"] = float((mh * (R["rh"] + mh)).sum())
    return ref, A


def candidate_cost(sc, cams, points, huber):
    """Cost at the given cameras and points (the oracle's residuals, Huber in longdouble) and its bound."""
    cand = sc.copy()
    cand.cam_params[:] = cams
    cand.points[:] = points
    raw, _ = oracle_lib.oracle_ba_residuals(cand)
    cost, s = _huber_cost(raw, huber)
    return cost, float((s + 2 * np.sqrt(s) * (np.abs(sc.obs_xy).sum(1) + 1)).sum())


def check(sc, R, cap, tau=TAU):
    """Worst |gpu - ref| / (tau u A) per quantity of the capture (a dict of ba.debug_linearization's form); every
    one must be <= 1.  The step quantities are taken from the GPU's y_c."""
    ref, A = step_reference(sc, R, cap["y_c"])
    o = R["opt"]
    ratios = {}

    def cmp(name, gpu, r, a):
        gpu = np.asarray(gpu, dtype=np.float64)
        err = np.abs(gpu.astype(LD) - np.asarray(r, dtype=LD)).astype(np.float64)
        bound = tau[name] * U * np.asarray(a, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bound)
        q = np.where(np.isnan(gpu), np.inf, q)
        ratios[name] = float(np.max(q, initial=0.0))

    for name in ("scale_c", "diag_c", "rhs"):
        cmp(name, cap[name], ref[name], A[name])
    cmp("S", np.tril(cap["S"]), np.tril(ref["S"]), A["S"])
    if R["pdim"]:
        cmp("scale_p", cap["scale_p"], ref["scale_p"], A["scale_p"])
        cmp("diag_p", cap["diag_p"], ref["diag_p"], A["diag_p"])
        cmp("ge", cap["ge"], ref["ge"], A["ge"])
        cmp("vinv", cap["vinv"], ref["vinv"], A["vinv"])
    cmp("initial_cost", cap["initial_cost"], ref["initial_cost"], A["initial_cost"])
    cmp("grad_max", cap["grad_max"], ref["grad_max"], A["grad_max"])
    # the camera step solves the reference system to its backward error
    y = cap["y_c"].astype(LD)
    Sf = ref["S"]
    Sfull = np.tril(Sf) + np.tril(Sf, -1).T
    res = Sfull @ y - ref["rhs"]
    ASf = np.tril(A["S"]) + np.tril(A["S"], -1).T
    ay = np.abs(cap["y_c"])
    aS = np.abs(np.asarray(Sfull, dtype=np.float64)) @ ay
    Ay = (ASf + np.abs(np.asarray(Sfull, dtype=np.float64))) @ ay + A["rhs"] + np.abs(np.asarray(ref["rhs"], dtype=np.float64)) + \
        y.size * aS.max(initial=0.0)
    cmp("y_c", np.asarray(res, dtype=np.float64), np.zeros_like(Ay), Ay)
    cmp("cand_cams", cap["cand_cams"], ref["cand_cams"], A["cand_cams"])
    cmp("cand_points", cap["cand_points"], ref["cand_points"], A["cand_points"])
    cmp("model_cost_change", cap["model_cost_change"], ref["model_cost_change"], A["model_cost_change"])
    cc, A_cc = candidate_cost(sc, cap["cand_cams"], cap["cand_points"], o["huber_delta"])
    cmp("cand_cost", cap["cand_cost"], cc, A_cc)
    mcc = ref["model_cost_change"]
    rel = (ref["initial_cost"] - cc) / mcc
    A_rel = (A["initial_cost"] + A_cc) / abs(float(mcc)) + abs(float(rel)) * A["model_cost_change"] / abs(float(mcc))
    cmp("relative_decrease", cap["relative_decrease"], rel, A_rel)
    # the decision, where the reference's relative decrease is clear of the threshold
    margin = TAU["relative_decrease"] * U * A_rel
    if abs(float(rel) - o["min_relative_decrease"]) > margin and \
            abs(float(ref["initial_cost"] - cc)) > o["function_tolerance"] * float(ref["initial_cost"]) * (1 + 1e-6):
        ratios["accepted"] = 0.0 if bool(cap["accepted"]) == bool(rel > o["min_relative_decrease"]) else np.inf
    return ratios
