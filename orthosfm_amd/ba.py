"""Host-side mirror of the reference's bundle-adjustment entry point on top of
the C ABI: orthosfm::runBundleAdjustment(cameras, tracks, algorithm,
optimizePoints, retriangulatePoints) (src/bundle_adjustment/bundle_adjustment.h:
18-20, .cpp:49-161) plus the two calls the pipeline makes around it,
ReconstructionAlgorithm::evaluateReprojectionError and ::triangulateTracks.

The classes below carry exactly the fields of the reference types that cross
the boundary (Feature, Track: src/data_structures/track.h:21-107; camera
parameter blocks: OrthoQuaternionCamera.h:83-91, OrthographicCamera.h:122-134).
All arithmetic happens in libosfm_hip.so; this module only flattens AoS to the
SoA arrays of osfm_ba_problem and scatters the results back.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi

MODEL_QUATERNION = 0
MODEL_EULER = 1
TERMINATION = {1: "CONVERGENCE (function tolerance)", 2: "CONVERGENCE (gradient tolerance)",
               3: "CONVERGENCE (parameter tolerance)", 4: "CONVERGENCE (trust region)",
               5: "NO_CONVERGENCE (max iterations)", 6: "FAILURE"}


@dataclass
class Feature:
    """orthosfm::Feature (track.h:21-31): x/y are float32 pixel coordinates."""
    viewID: int
    localFeatureID: int
    x: float
    y: float


@dataclass
class Track:
    """orthosfm::Track (track.h:69-107)."""
    features: list
    point: np.ndarray = field(default_factory=lambda: np.zeros(4))
    has_point: bool = False


@dataclass
class QuatCamera:
    """OrthoQuaternionCamera: rotation (x, y, z, w), offsets, scale; per-block
    fixed flags default to the reference's (rotation/offset free, scale fixed)."""
    view_id: int
    width: int
    height: int
    rotation: np.ndarray
    offset_x: float = 0.0
    offset_y: float = 0.0
    scale: float = 1.0
    fixed: bool = False
    fix_rotation: bool = False
    fix_offset: bool = False
    fix_scale: bool = True
    model = MODEL_QUATERNION

    def params(self):
        return np.array([*self.rotation, self.offset_x, self.offset_y, self.scale])

    def const_mask(self):
        f = self.fixed
        return np.array([f or self.fix_rotation] * 4 + [f or self.fix_offset] * 2 + [f or self.fix_scale],
                        dtype=np.uint8)

    def set_params(self, v):
        self.rotation = np.array(v[:4])
        self.offset_x, self.offset_y, self.scale = float(v[4]), float(v[5]), float(v[6])


@dataclass
class EulerCamera:
    """OrthographicCamera: phi, theta, roll, offsets, scale with the DoF mask of
    setDegreesOfFreedom (OrthographicCamera.cpp:195-207)."""
    view_id: int
    width: int
    height: int
    phi: float = 0.0
    theta: float = 0.0
    roll: float = 0.0
    offset_x: float = 0.0
    offset_y: float = 0.0
    scale: float = 1.0
    fixed: bool = False
    dof: int = 4            # solver 3 (ORTHO_EULER_ALL_DOF) -> 4
    model = MODEL_EULER

    def params(self):
        return np.array([self.phi, self.theta, self.roll, self.offset_x, self.offset_y, self.scale, 0.0])

    def const_mask(self):
        d = self.dof
        flags = [d < 1, d < 2, d < 3, d < 4, d < 4, d < 5, True]
        return np.array([self.fixed or f for f in flags], dtype=np.uint8)

    def set_params(self, v):
        self.phi, self.theta, self.roll = float(v[0]), float(v[1]), float(v[2])
        self.offset_x, self.offset_y, self.scale = float(v[3]), float(v[4]), float(v[5])


class FlatProblem:
    """The arrays of osfm_ba_problem (kept alive while the struct is in use)."""

    def __init__(self, model, cam_params, cam_const, img_w, img_h, points, obs_xy, obs_camera, obs_point):
        self.model = int(model)
        # always private copies: the solver updates cam_params / points in place
        self.cam_params = np.array(cam_params, dtype=np.float64, order="C").reshape(-1, 7)
        self.cam_const = np.array(cam_const, dtype=np.uint8, order="C").reshape(-1, 7)
        self.img_w = np.array(img_w, dtype=np.int32, order="C")
        self.img_h = np.array(img_h, dtype=np.int32, order="C")
        self.points = np.array(points, dtype=np.float64, order="C").reshape(-1, 4)
        self.obs_xy = np.array(obs_xy, dtype=np.float64, order="C").reshape(-1, 2)
        self.obs_camera = np.array(obs_camera, dtype=np.int32, order="C")
        self.obs_point = np.array(obs_point, dtype=np.int32, order="C")

    @classmethod
    def from_scene(cls, sc):
        return cls(sc.model, sc.cam_params, sc.cam_const, sc.img_w, sc.img_h, sc.points, sc.obs_xy,
                   sc.obs_camera, sc.obs_point)

    def struct(self):
        p = capi.BaProblem()
        p.model = self.model
        p.num_cameras = self.cam_params.shape[0]
        p.num_points = self.points.shape[0]
        p.num_observations = self.obs_camera.shape[0]
        p.cam_params = self.cam_params.ctypes.data
        p.cam_const = self.cam_const.ctypes.data
        p.img_width = self.img_w.ctypes.data
        p.img_height = self.img_h.ctypes.data
        p.points = self.points.ctypes.data
        p.obs_xy = self.obs_xy.ctypes.data
        p.obs_camera = self.obs_camera.ctypes.data
        p.obs_point = self.obs_point.ctypes.data
        return p


SMALL_FORM_GENERAL, SMALL_FORM_AUTO, SMALL_FORM_ONE_WORKGROUP = 0, 1, 2


def default_options(small_form: int = SMALL_FORM_GENERAL, **kw) -> capi.BaOptions:
    """osfm_ba_options_default with fields replaced.  small_form: 0 the general form, 1 the one-workgroup form where
    the problem is small enough (small_limits()), 2 the one-workgroup form or OsfmError(E_ARG)."""
    o = capi.BaOptions()
    capi.check(capi.lib.osfm_ba_options_default(C.byref(o)))
    o.small_form = small_form
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def small_limits():
    """osfm_ba_small_limits: (max_cameras, track_chunk, auto_max_observations) of the one-workgroup form."""
    v = [C.c_int32() for _ in range(3)]
    capi.check(capi.lib.osfm_ba_small_limits(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def solve(problem: FlatProblem, options: capi.BaOptions | None = None, **kw) -> capi.BaSummary:
    """osfm_ba_solve: in-place update of problem.cam_params / problem.points."""
    o = options if options is not None else default_options(**kw)
    s = capi.BaSummary()
    st = problem.struct()
    capi.check(capi.lib.osfm_ba_solve(C.byref(st), C.byref(o), C.byref(s)))
    return s


@dataclass
class Covariance:
    """What osfm_ba_covariance / osfm_scene_covariance return (include/osfm_hip.h): the cofactor matrices, unscaled --
    multiply by variance_factor for covariances in pixel units of the residuals.  An array that was not asked for
    (skip=...) or not computed (cam_cov_full without full=True, the point arrays with optimize_points=0) is None."""
    cam_cov: np.ndarray | None            # (C, 6, 6)
    cam_ldim: np.ndarray | None           # (C,)
    cam_cov_full: np.ndarray | None       # (nc, nc)
    point_cov: np.ndarray | None          # (M, 3, 3) of the Euclidean point
    point_valid: np.ndarray | None        # (M,) bool
    cost: float
    variance_factor: float
    num_residuals: int
    num_unknowns: int
    num_camera_unknowns: int
    num_valid_points: int
    gauge_camera: int
    gauge_axis: int
    min_pivot_seen: float
    rank_deficient: int
    dense_schur: int
    timings_ms: dict

    def point_sigma(self) -> np.ndarray:
        """sqrt(variance_factor * largest eigenvalue of point_cov) per point, NaN where the point is invalid."""
        out = np.full(self.point_cov.shape[0], np.nan)
        ok = self.point_valid
        if ok.any():
            out[ok] = np.sqrt(self.variance_factor * np.linalg.eigvalsh(self.point_cov[ok])[:, -1].clip(min=0.0))
        return out


def cov_options(**kw) -> capi.BaCovOptions:
    """osfm_ba_cov_options_default with fields replaced (huber_delta, min_pivot_ratio, optimize_points, depth_gauge,
    device)."""
    o = capi.BaCovOptions()
    capi.check(capi.lib.osfm_ba_cov_options_default(C.byref(o)))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _covariance_call(call, num_cameras, num_points, nc_guess, o, full, skip, fill=None):
    """Runs call(options, result) with arrays for num_cameras cameras / num_points points (skip: names of
    capi.BaCovResult.ARRAYS passed as NULL; fill: a value the arrays start with).  cam_cov_full is sized for nc_guess
    and, if the library's layout has another nc, for the one it reports."""
    Cn, M = int(num_cameras), int(num_points)
    with_points = bool(o.optimize_points)
    nc = int(nc_guess)
    for _ in range(2):
        arrays = {"cam_cov": np.zeros((Cn, 6, 6)), "cam_ldim": np.zeros(Cn, dtype=np.int32),
                  "cam_cov_full": np.zeros((nc, nc)) if full else None,
                  "point_cov": np.zeros((M, 3, 3)) if with_points else None,
                  "point_valid": np.zeros(M, dtype=np.uint8) if with_points else None}
        for k in skip:
            arrays[k] = None
        r = capi.BaCovResult()
        for k, a in arrays.items():
            if a is not None and fill is not None:
                a[...] = fill
            # (an empty array still gets a pointer: NULL means "not asked for")
            setattr(r, k, None if a is None else (a.ctypes.data if a.size else np.zeros(1).ctypes.data))
        r.nc = nc
        status = call(o, r)
        if status == capi.E_ARG and arrays["cam_cov_full"] is not None and r.num_camera_unknowns != nc:
            nc = int(r.num_camera_unknowns)
            continue
        break
    if status != capi.OK:
        err = capi.OsfmError(status, capi.last_error())
        err.rank_deficient = int(r.rank_deficient) if status == capi.E_NUMERIC else 0
        err.min_pivot_seen = float(r.min_pivot_seen)
        err.gauge_camera, err.gauge_axis = int(r.gauge_camera), int(r.gauge_axis)
        err.arrays = arrays
        raise err
    if arrays["point_valid"] is not None:
        arrays["point_valid"] = arrays["point_valid"].astype(bool)
    return Covariance(arrays["cam_cov"], arrays["cam_ldim"], arrays["cam_cov_full"], arrays["point_cov"], arrays["point_valid"],
                      r.cost, r.variance_factor, r.num_residuals, r.num_unknowns, r.num_camera_unknowns, r.num_valid_points,
                      r.gauge_camera, r.gauge_axis, r.min_pivot_seen, r.rank_deficient, r.dense_schur,
                      {"linearize": r.linearize_ms, "factor": r.factor_ms, "inverse": r.inverse_ms, "point": r.point_ms,
                       "total": r.total_ms})


def covariance(problem: FlatProblem, options: capi.BaCovOptions | None = None, full: bool = False, skip=(), fill=None,
               **kw) -> Covariance:
    """osfm_ba_covariance: the cofactor matrices of the cameras and points at the problem's values, which are not
    modified (include/osfm_hip.h: the gauge, the rank test, which points are invalid).  full: also the whole S^-1.
    Raises capi.OsfmError; on E_NUMERIC (an open gauge) the error carries rank_deficient = 1 and min_pivot_seen."""
    o = options if options is not None else cov_options(**kw)
    st = problem.struct()
    free = _free_columns(problem)
    held = bool(o.depth_gauge) and bool((free == 0).any()) and bool(_both_offsets_free(problem).any())
    return _covariance_call(lambda oo, r: capi.lib.osfm_ba_covariance(C.byref(st), C.byref(oo), C.byref(r)),
                            problem.cam_params.shape[0], problem.points.shape[0], int(free.sum()) - int(held), o, full, skip, fill)


def _both_offsets_free(problem: FlatProblem) -> np.ndarray:
    cc = problem.cam_const
    return (cc[:, 4:6] == 0).all(axis=1) if problem.model == 0 else (cc[:, 3:5] == 0).all(axis=1)


FORM_AS_SOLVE, FORM_PER_COLUMN = 0, 1
_LAUNCH_FIELDS = ("one_launch", "groups", "num_d", "num_p", "num_tiles", "arcs", "span", "nblk")


def debug_cholesky_solve(A, b, cam_ldim=None, pairs=None, form=FORM_AS_SOLVE, max_d=0, max_groups=0):
    """osfm_ba_debug_cholesky_solve (test hook): the reduced system's dense Cholesky solve of osfm_ba_solve applied to
    the batch A[r] x[r] = b[r] (A: (R, n, n), b: (R, n)), one system after the other on the same work arrays.
    cam_ldim / pairs: the cameras' unknowns and the camera pairs that share a track -- the elimination order is
    looked for as the solve does.  Returns (x (R, n), info (R,), launch: dict of _LAUNCH_FIELDS)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if A.ndim == 2:
        A, b = A[None], b.reshape(1, -1)
    R, n = A.shape[0], A.shape[1]
    if A.shape != (R, n, n) or b.shape != (R, n):
        raise ValueError(f"A {A.shape} and b {b.shape} are not a batch of systems")
    ldim = np.ascontiguousarray(cam_ldim if cam_ldim is not None else np.zeros(0), dtype=np.int32)
    pr = np.ascontiguousarray(pairs if pairs is not None else np.zeros((0, 2)), dtype=np.int32).reshape(-1, 2)
    x = np.empty((R, n))
    info = np.zeros(R, dtype=np.int32)
    launch = np.zeros(8, dtype=np.int32)
    capi.check(capi.lib.osfm_ba_debug_cholesky_solve(
        n, R, A, b, int(ldim.shape[0]), ldim.ctypes.data_as(C.c_void_p) if ldim.size else None,
        int(pr.shape[0]), pr.ctypes.data_as(C.c_void_p) if pr.size else None, int(form), int(max_d), int(max_groups), x, info, launch))
    return x, info, dict(zip(_LAUNCH_FIELDS, launch.tolist()))


def debug_linearization(problem: FlatProblem, options: capi.BaOptions | None = None, **kw):
    """osfm_ba_debug_linearization (test hook): osfm_ba_solve on the problem (updated in place as solve() does) with
    copies of its first LM iteration -- the Jacobi scales, LM diagonals, V^-1 and g of the points, the reduced camera
    system and rhs in the cameras' own order (lower triangle), then the camera step y_c, the candidate cameras and
    points and the step's cost figures -- and the regime the solve took.  Returns a dict."""
    o = options if options is not None else default_options(**kw)
    C_, M = problem.cam_params.shape[0], problem.points.shape[0]
    nc = int(_free_columns(problem).sum())
    shapes = {"scale_c": (nc,), "diag_c": (nc,), "S": (nc, nc), "rhs": (nc,), "scale_p": (M, 3), "diag_p": (M, 3),
              "vinv": (M, 3, 3), "ge": (M, 3), "y_c": (nc,), "cand_cams": (C_, 7), "cand_points": (M, 4)}
    out = {k: np.full(max(int(np.prod(v)), 1), np.nan) for k, v in shapes.items()}
    cap = capi.BaLinCapture()
    cap.nc = nc                 # (the library refuses a capture sized for another layout)
    for k in capi.BaLinCapture.ARRAYS:
        setattr(cap, k, out[k].ctypes.data)
    st = problem.struct()
    capi.check(capi.lib.osfm_ba_debug_linearization(C.byref(st), C.byref(o), C.byref(cap)))
    res = {k: out[k][:int(np.prod(v))].reshape(v) for k, v in shapes.items()}
    for name, _ in capi.BaLinCapture._fields_:
        if name not in capi.BaLinCapture.ARRAYS and name not in ("nc", "reserved"):
            res[name] = getattr(cap, name)
    return res


def _free_columns(problem: FlatProblem) -> np.ndarray:
    """Free tangent columns per camera (the layout of osfm_ba_solve: rotation as one block of 3 in the quaternion
    model)."""
    cc = problem.cam_const
    if problem.model == 0:
        return np.where(cc[:, 0] == 0, 3, 0) + (cc[:, 4:7] == 0).sum(axis=1)
    return (cc[:, :6] == 0).sum(axis=1)


def reprojection_errors(problem: FlatProblem, device: int = 0):
    """Batched ReconstructionAlgorithm::evaluateReprojectionError."""
    O = problem.obs_camera.shape[0]
    err = np.zeros(O)
    res = np.zeros((O, 2))
    st = problem.struct()
    capi.check(capi.lib.osfm_ba_reprojection_errors(C.byref(st), device, capi._ptr(err, C.c_double),
                                                    capi._ptr(res, C.c_double)))
    return err, res


def triangulate(problem: FlatProblem, device: int = 0) -> np.ndarray:
    """triangulateOrthographicTracks on the flattened tracks (in place);
    returns the per-point validity mask."""
    valid = np.zeros(max(problem.points.shape[0], 1), dtype=np.uint8)
    st = problem.struct()
    capi.check(capi.lib.osfm_ba_triangulate(C.byref(st), device, capi._ptr(valid, C.c_uint8)))
    return valid[:problem.points.shape[0]]


def _flatten(cameras, tracks):
    """bundle_adjustment.cpp:54-57,103-123: residual blocks for every feature
    of every track with a point whose view has a camera."""
    cam_index = {}
    for i, cam in enumerate(cameras):
        cam_index.setdefault(cam.view_id, i)          # std::map::insert keeps the first
    obs_xy, obs_cam, obs_pt, used, pts = [], [], [], [], []
    for ti, t in enumerate(tracks):
        if not t.has_point:
            continue
        j = len(used)
        n_before = len(obs_cam)
        for f in t.features:
            ci = cam_index.get(f.viewID)
            if ci is None:
                continue
            obs_xy.append((float(np.float32(f.x)), float(np.float32(f.y))))
            obs_cam.append(ci)
            obs_pt.append(j)
        # the parameter block exists even without residuals (AddParameterBlock, :88)
        used.append(ti)
        pts.append(np.asarray(t.point, dtype=np.float64))
        if len(obs_cam) == n_before:
            pass
    model = cameras[0].model if cameras else MODEL_QUATERNION
    fp = FlatProblem(model,
                     np.array([c.params() for c in cameras]).reshape(-1, 7),
                     np.array([c.const_mask() for c in cameras], dtype=np.uint8).reshape(-1, 7),
                     [c.width for c in cameras], [c.height for c in cameras],
                     np.array(pts).reshape(-1, 4), np.array(obs_xy).reshape(-1, 2), obs_cam, obs_pt)
    return fp, used


def filter_tracks_to_available_cameras(cameras, tracks):
    """filterTracksToAvailableCameras(cameras, tracks, false, false)
    (src/util/common.cpp:85-139): keeps tracks with >= 2 features in the given
    cameras, restricted to those features; the copies carry NO point."""
    ids = {c.view_id for c in cameras}
    out = []
    for t in tracks:
        fs = [f for f in t.features if f.viewID in ids]
        if len(fs) > 1:
            out.append(Track(fs))
    return out


def triangulate_tracks(cameras, tracks, reset_existing=True, device=0):
    """ReconstructionAlgorithm::triangulateTracks ->
    triangulateOrthographicTracks (triangulation.cpp:44-93)."""
    tmp = [Track(t.features, np.array([0.0, 0, 0, 1]), True) for t in tracks]
    fp, used = _flatten(cameras, tmp)
    valid = triangulate(fp, device) if fp.obs_camera.size else np.zeros(len(used), np.uint8)
    for j, ti in enumerate(used):
        t = tracks[ti]
        if valid[j]:
            if (not t.has_point) or reset_existing:
                t.point = fp.points[j].copy()
                t.has_point = True
        elif reset_existing:
            t.has_point = False


def run_bundle_adjustment(cameras, tracks, algorithm=None, optimize_points=True,
                          retriangulate_points=False, device=0, verbose=True):
    """orthosfm::runBundleAdjustment.  Cameras are updated in place; track points
    are updated in place only when retriangulate_points is False -- with True
    the reference optimises a filtered, re-triangulated COPY that it discards
    (bundle_adjustment.cpp:71-83,161), and so does this function."""
    work = tracks
    if retriangulate_points:
        work = filter_tracks_to_available_cameras(cameras, tracks)
        triangulate_tracks(cameras, work, True, device)
    fp, used = _flatten(cameras, work)
    s = solve(fp, optimize_points=1 if optimize_points else 0, device=device)
    for cam, v in zip(cameras, fp.cam_params):
        cam.set_params(v)
    for j, ti in enumerate(used):
        work[ti].point = fp.points[j].copy()
    if verbose:
        # summary.BriefReport() + the point-motion line (bundle_adjustment.cpp:148-160)
        print(f"Ceres-style Solver Report: Iterations: {s.num_iterations + 1}, Initial cost: {s.initial_cost:e}, "
              f"Final cost: {s.final_cost:e}, Termination: {TERMINATION.get(s.termination, '?')}")
        n = max(len(work), 1)
        print(f"Average point change: {s.mean_point_change * len(used) / n} (maximum change: {s.max_point_change})")
    return s


# ---------------------------------------------------------------------------
# bench helper
# ---------------------------------------------------------------------------

def bench_global_ba(num_cameras=200, num_points=100000, max_iterations=25, device=0):
    """BASELINE configs[3]: global BA, quaternion solver, 200 cameras, ~100k
    tracks.  Returns LM iterations/s of one solve from a perturbed start."""
    from . import synth
    sc = synth.make_ba_scene(synth.MODEL_QUATERNION, num_cameras, num_points, config_id=4)
    fp = FlatProblem.from_scene(sc)
    warm = FlatProblem.from_scene(sc)
    solve(warm, max_num_iterations=2, device=device)          # warm-up (allocator, code objects)
    # the call in its steady state: five identical calls, the MEDIAN one reported (by call time; the extremes beside it --
    # the CPU side of the comparison is a single measurement, so neither is the best of several)
    runs = [solve(FlatProblem.from_scene(sc), max_num_iterations=max_iterations, device=device) for _ in range(5)]
    runs.sort(key=lambda r: r.solve_ms)
    s = runs[len(runs) // 2]
    its = s.num_iterations
    # the per-family device times come from a second, instrumented solve (verbose = 1 records
    # an event pair around every kernel family of every iteration)
    prof = FlatProblem.from_scene(sc)
    sp = solve(prof, max_num_iterations=max_iterations, device=device, verbose=1)
    assert sp.num_iterations == its and sp.final_cost == s.final_cost
    s.point_pass_ms, s.pair_pass_ms, s.cholesky_ms, s.back_pass_ms = (sp.point_pass_ms, sp.pair_pass_ms,
                                                                      sp.cholesky_ms, sp.back_pass_ms)
    lm_ms = s.point_pass_ms + s.pair_pass_ms + s.cholesky_ms + s.back_pass_ms
    return {"workload": f"{num_cameras} quaternion cameras, {num_points} tracks, "
                        f"{fp.obs_camera.size} observations, Schur + dense Cholesky",
            "iterations": int(its), "iterations_per_s": its / (s.solve_ms * 1e-3), "calls_timed": len(runs), "reported": "median call",
            "iterations_per_s_min_max": [its / (runs[-1].solve_ms * 1e-3), its / (runs[0].solve_ms * 1e-3)],
            "lm_loop_iterations_per_s": its / max(s.lm_loop_ms * 1e-3, 1e-9),
            "lm_loop_iterations_per_s_min_max": [its / max(max(r.lm_loop_ms for r in runs) * 1e-3, 1e-9),
                                                 its / max(min(r.lm_loop_ms for r in runs) * 1e-3, 1e-9)],
            # elimination order of the reduced camera system (ba_order.hip): arcs factored side by side, the
            # chain of dependent diagonal blocks in the cameras' order and in the order used
            "order_arcs": int(s.order_arcs), "chain_blocks": [int(s.chain_blocks_natural), int(s.chain_blocks)],
            "solve_ms": s.solve_ms, "lm_loop_ms": s.lm_loop_ms, "initial_cost": s.initial_cost, "final_cost": s.final_cost,
            "termination": TERMINATION.get(s.termination, "?"),
            "kernel_ms": {"point_pass": s.point_pass_ms, "pair_pass": s.pair_pass_ms,
                          "cholesky": s.cholesky_ms, "back_pass": s.back_pass_ms,
                          "sum": lm_ms, "linearizations": int(s.linearizations)},
            "pair_entries": int(s.num_pair_entries),
            "observations": int(fp.obs_camera.size), "points": int(num_points),
            # tangent size of the free camera blocks: 3 per free rotation, 1 per free scalar
            "camera_unknowns": int(sum((0 if c[0] else 3) + int((c[4:] == 0).sum()) for c in fp.cam_const))}


def bench_local_ba(num_points=3000, num_cameras=3, device=0, repeats=5):
    """BASELINE configs[0] / the per-group call of the incremental reconstruction
    (reconstruct.cpp:219): a 3-camera quaternion BA.  Latency of one call and of one LM
    iteration inside it (the median of `repeats` calls)."""
    import time
    from . import synth
    sc = synth.make_ba_scene(synth.MODEL_QUATERNION, num_cameras, num_points, config_id=1)
    solve(FlatProblem.from_scene(sc), max_num_iterations=2, device=device)
    calls = []
    for _ in range(repeats):
        fp = FlatProblem.from_scene(sc)
        t0 = time.perf_counter()
        s = solve(fp, max_num_iterations=50, device=device)
        calls.append(((time.perf_counter() - t0) * 1e3, s))
    calls.sort(key=lambda c: c[0])
    call_ms, s = calls[len(calls) // 2]              # the median call (its extremes: call_ms_min_max)
    return {"workload": f"{num_cameras} quaternion cameras, {num_points} tracks, {fp.obs_camera.size} observations "
                        "(the local adjustment of one camera group)",
            "iterations": int(s.num_iterations), "call_ms": call_ms, "call_ms_min_max": [calls[0][0], calls[-1][0]], "reported": "median call",
            "lm_loop_ms": s.lm_loop_ms,
            "us_per_iteration": 1e3 * s.lm_loop_ms / max(s.num_iterations, 1),
            "iterations_per_s": s.num_iterations / max(s.lm_loop_ms * 1e-3, 1e-9),
            "final_cost": s.final_cost, "termination": TERMINATION.get(s.termination, "?")}
