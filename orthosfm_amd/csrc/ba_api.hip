// C-ABI implementation of the bundle-adjustment path (include/osfm_hip.h, section B): the checks, the uploads and the
// entry points.  The Levenberg-Marquardt solve they run is ba_solve.hip's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <future>
#include <numeric>
#include <string>
#include <vector>

#include "ba_solve.h"

using namespace osfm;

namespace {

// sizes, model, null pointers: what has to hold before any array is touched
int validate_header(const osfm_ba_problem *p, const char *what)
{
    if (!p) { set_error("%s: null problem", what); return OSFM_E_ARG; }
    if (p->model != OSFM_BA_MODEL_QUATERNION && p->model != OSFM_BA_MODEL_EULER) {
        set_error("%s: unknown camera model %d", what, p->model); return OSFM_E_ARG;
    }
    if (p->num_cameras < 0 || p->num_points < 0 || p->num_observations < 0) {
        set_error("%s: negative size", what); return OSFM_E_ARG;
    }
    if ((p->num_cameras && (!p->cam_params || !p->cam_const || !p->img_width || !p->img_height)) ||
        (p->num_points && !p->points) ||
        (p->num_observations && (!p->obs_xy || !p->obs_camera || !p->obs_point))) {
        set_error("%s: null array", what); return OSFM_E_ARG;
    }
    return OSFM_OK;
}

// The per-observation half of the checks; L->pt_start from the points' observation counts, taken in the same sweep over
// the caller's arrays
int validate_observations(const osfm_ba_problem *p, const char *what, Layout *L)
{
    int prev = 0;
    L->pt_start.assign((size_t)p->num_points + 2, 0);
    // A point is observed at most once per camera: the reference's tracks hold one feature per view (a track
    // with two is a conflict and dropped, bundler_tracks.cc:120-145), and the Schur-complement fast paths
    // (one slot per camera and track, ba_pairs.hip; the dense product, ba_dense.hip) rest on it.
    std::vector<int> seen_in((size_t)p->num_cameras, -1);
    for (int k = 0; k < p->num_observations; ++k) {
        const int c = p->obs_camera[k], j = p->obs_point[k];
        if (c < 0 || c >= p->num_cameras || j < 0 || j >= p->num_points) {
            set_error("%s: observation %d references camera %d / point %d out of range", what, k, c, j);
            return OSFM_E_ARG;
        }
        if (j < prev) {
            set_error("%s: obs_point must be non-decreasing (observation %d)", what, k);
            return OSFM_E_ARG;
        }
        if (seen_in[c] == j) {
            set_error("%s: point %d is observed twice by camera %d (observation %d); one observation per camera and point", what, j, c, k);
            return OSFM_E_ARG;
        }
        seen_in[c] = j;
        prev = j;
        L->pt_start[j + 1]++;
    }
    for (int j = 0; j < p->num_points; ++j) L->pt_start[j + 1] += L->pt_start[j];
    return OSFM_OK;
}

// all the checks, and the caller's layout
int validate_problem(const osfm_ba_problem *p, const char *what, Layout *L)
{
    OSFM_RETURN_IF(validate_header(p, what));
    OSFM_RETURN_IF(validate_observations(p, what, L));
    build_camera_layout(p->model, p->num_cameras, p->cam_const, L);
    return OSFM_OK;
}

// the caller's arrays: queued before the layout is derived on the host, so that the 24 bytes per observation
// cross PCIe while the host counts them
int upload_caller_arrays(const osfm_ba_problem *p, hipStream_t s, DeviceProblem *D)
{
    const int C = p->num_cameras, M = p->num_points, O = p->num_observations;
    OSFM_RETURN_IF(upload(D->obs_xy, p->obs_xy, (size_t)2 * O, s));
    OSFM_RETURN_IF(upload(D->obs_cam, p->obs_camera, (size_t)O, s));
    OSFM_RETURN_IF(upload(D->points[0], p->points, (size_t)4 * M, s));
    OSFM_RETURN_IF(upload(D->cams[0], p->cam_params, (size_t)7 * C, s));
    OSFM_RETURN_IF(upload(D->img_w, p->img_width, (size_t)C, s));
    OSFM_RETURN_IF(upload(D->img_h, p->img_height, (size_t)C, s));
    return OSFM_OK;
}

int upload_problem(const osfm_ba_problem *p, const Layout &L, double huber, int pdim, hipStream_t s,
    DeviceProblem *D, bool caller_arrays_queued = false)
{
    const int C = p->num_cameras, M = p->num_points, O = p->num_observations;
    if (!caller_arrays_queued) OSFM_RETURN_IF(upload_caller_arrays(p, s, D));
    OSFM_RETURN_IF(upload(D->pt_start, L.pt_start.data(), (size_t)M + 1, s));
    OSFM_RETURN_IF(upload(D->cam_ldim, L.cam_ldim.data(), (size_t)C, s));
    OSFM_RETURN_IF(upload(D->cam_off, L.cam_off.data(), (size_t)C, s));
    OSFM_RETURN_IF(upload(D->colmap, L.colmap.data(), (size_t)6 * C, s));
    // No synchronisation here: every source array (the caller's and the Layout's) outlives
    // the call, and what follows is ordered behind the copies on the same stream.
    return finish_device_problem(p->model, C, M, O, L.nc, huber, pdim, s, D);
}

// the caller's camera pairs (two camera indices each, in either order) as (larger, smaller)
int decode_pairs(const char *what, int C, int num_pairs, const int32_t *pairs, std::vector<std::pair<int, int>> *out)
{
    out->resize((size_t)num_pairs);
    for (int i = 0; i < num_pairs; ++i) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= C || b < 0 || b >= C) { set_error("%s: pair %d names camera %d / %d", what, i, a, b); return OSFM_E_ARG; }
        (*out)[i] = {std::max(a, b), std::min(a, b)};
    }
    return OSFM_OK;
}

}  // namespace

namespace osfm {

int select_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (this backend has no CPU fallback)");
        return OSFM_E_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("device %d out of range [0,%d)", device, ndev); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
    return OSFM_OK;
}


void build_camera_layout(int model, int C, const uint8_t *cam_const, Layout *L)
{
    L->cam_ldim.assign(C + 1, 0); L->cam_off.assign(C + 1, 0); L->colmap.assign((size_t)6 * (C + 1), 0);
    int tot = 0;
    for (int c = 0; c < C; ++c) {
        const uint8_t *cc = cam_const + 7 * c;
        int n = 0;
        int8_t *cm = L->colmap.data() + 6 * c;
        if (model == OSFM_BA_MODEL_QUATERNION) {
            if (!cc[0]) { cm[n++] = 0; cm[n++] = 1; cm[n++] = 2; }
            for (int s = 4; s < 7; ++s) if (!cc[s]) cm[n++] = (int8_t)(s - 1);   // full cols 3,4,5
        } else {
            for (int s = 0; s < 6; ++s) if (!cc[s]) cm[n++] = (int8_t)s;
        }
        L->cam_ldim[c] = n; L->cam_off[c] = tot; tot += n;
    }
    L->nc = tot;
}

int validate_ba_problem(const osfm_ba_problem *p, const char *what, Layout *L) { return validate_problem(p, what, L); }

int upload_ba_problem(const osfm_ba_problem *p, const Layout &L, double huber, int pdim, hipStream_t s, DeviceProblem *D)
{
    return upload_problem(p, L, huber, pdim, s, D);
}

int finish_device_problem(int model, int C, int M, int O, int nc, double huber, int pdim, hipStream_t s, DeviceProblem *D)
{
    OSFM_RETURN_IF(D->cams[1].alloc((size_t)7 * C * 8));
    OSFM_RETURN_IF(D->points[1].alloc((size_t)4 * M * 8));
    // obs_point is non-decreasing, i.e. it is the expansion of pt_start
    OSFM_RETURN_IF(D->obs_pt.alloc((size_t)O * sizeof(int32_t)));
    launch_expand_points(D->pt_start.as<int32_t>(), M, D->obs_pt.as<int32_t>(), s);
    BaDev &d = D->dev;
    memset(&d, 0, sizeof(d));          // lm == nullptr: the plain pointers below are used as they are (the solve's are its own)
    d.model = model; d.C = C; d.M = M; d.O = O; d.nc = nc; d.pdim = pdim;
    d.cams = D->cams[0].as<double>(); d.points = D->points[0].as<double>();
    d.obs_xy = D->obs_xy.as<double>(); d.obs_cam = D->obs_cam.as<int32_t>(); d.obs_pt = D->obs_pt.as<int32_t>();
    d.pt_start = D->pt_start.as<int32_t>(); d.img_w = D->img_w.as<int32_t>(); d.img_h = D->img_h.as<int32_t>();
    d.cam_ldim = D->cam_ldim.as<int32_t>(); d.cam_off = D->cam_off.as<int32_t>();
    d.cam_colmap = D->colmap.as<int8_t>();
    d.huber = huber;
    return OSFM_OK;
}

}  // namespace osfm

extern "C" {

int osfm_ba_debug_chol_trace(int enable, int64_t *stamps)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("ba_debug_chol_trace: no HIP device available"); return OSFM_E_DEVICE; }
    OSFM_HIP_CHECK(hipDeviceSynchronize());
    long long *buf = chol_flow_trace_buffer(1);
    if (!buf) { set_error("ba_debug_chol_trace: no memory for the trace"); return OSFM_E_DEVICE; }
    if (stamps) OSFM_HIP_CHECK(hipMemcpy(stamps, buf, 161 * 32 * 8, hipMemcpyDeviceToHost));
    if (!enable) chol_flow_trace_buffer(0);
    return OSFM_OK;
}

int osfm_ba_debug_flow_spin_limit(int limit)
{
    chol_flow_set_spin_limit(limit);
    return OSFM_OK;
}

int osfm_ba_debug_order(int num_cameras, const int32_t *cam_ldim, int num_pairs, const int32_t *pairs, int32_t *cam_off,
    uint64_t *blocks, int blocks_capacity, int32_t *info)
{
    if (num_cameras <= 0 || !cam_ldim || num_pairs < 0 || (num_pairs && !pairs) || !cam_off || !info) { set_error("ba_debug_order: bad arguments"); return OSFM_E_ARG; }
    std::vector<std::pair<int, int>> cp;
    OSFM_RETURN_IF(decode_pairs("ba_debug_order", num_cameras, num_pairs, pairs, &cp));
    ReducedOrder ord;
    const bool on = choose_reduced_order(num_cameras, cam_ldim, cp, &ord);
    unknown_positions(num_cameras, cam_ldim, ord, cam_off);
    const int tot = std::accumulate(cam_ldim, cam_ldim + num_cameras, 0);
    info[0] = on ? 1 : 0; info[1] = on ? ord.arcs : 0; info[2] = on ? ord.sep_cams : 0; info[3] = on ? ord.span : tot;
    info[4] = on ? ord.nblk : (tot + 31) / 32; info[5] = ord.chain_natural; info[6] = on ? ord.chain_ordered : ord.chain_natural;
    info[7] = on ? (int)ord.pad.size() : 0;
    if (blocks && on) {
        if (blocks_capacity < ord.nblk + 1) { set_error("ba_debug_order: %d rows of blocks, room for %d", ord.nblk + 1, blocks_capacity); return OSFM_E_CAPACITY; }
        for (size_t i = 0; i < ord.nz.size(); ++i) blocks[i] = ord.nz[i];
    }
    return OSFM_OK;
}

int osfm_ba_debug_cholesky_solve(int n, int num_systems, const double *A, const double *b, int num_cameras, const int32_t *cam_ldim,
    int num_pairs, const int32_t *pairs, int form, int max_d, int max_groups, double *x, int32_t *info, int32_t *launch)
{
    const char *what = "ba_debug_cholesky_solve";
    if (n <= 32) { set_error("%s: n = %d: systems of one block are chol_small_kernel's, not this path's", what, n); return OSFM_E_ARG; }
    if (n > 32 * 1024 || num_systems <= 0 || !A || !b || !x || !info) { set_error("%s: bad arguments", what); return OSFM_E_ARG; }
    if (form != 0 && form != 1) { set_error("%s: form %d (0: as the solve picks, 1: launch per column)", what, form); return OSFM_E_ARG; }
    if (max_d < 0 || max_groups < 0 || (form == 1 && (max_d || max_groups))) {
        set_error("%s: max_d %d / max_groups %d (only the one-launch form has them)", what, max_d, max_groups); return OSFM_E_ARG;
    }
    if (num_cameras < 0 || num_pairs < 0 || (num_cameras && !cam_ldim) || (num_pairs && (!pairs || !num_cameras))) {
        set_error("%s: bad camera arguments", what); return OSFM_E_ARG;
    }
    ReducedOrder ord;
    if (num_cameras) {
        int tot = 0;
        for (int c = 0; c < num_cameras; ++c) {
            if (cam_ldim[c] < 0) { set_error("%s: camera %d has %d unknowns", what, c, cam_ldim[c]); return OSFM_E_ARG; }
            tot += cam_ldim[c];
        }
        if (tot != n) { set_error("%s: the cameras hold %d unknowns, the system %d", what, tot, n); return OSFM_E_ARG; }
        std::vector<std::pair<int, int>> cp;
        OSFM_RETURN_IF(decode_pairs(what, num_cameras, num_pairs, pairs, &cp));
        choose_reduced_order(num_cameras, cam_ldim, cp, &ord);
    }
    // the caller's unknown u sits at pos[u] of the laid-out system, span unknowns in all (no cameras: one block of n)
    const std::vector<int32_t> pos = num_cameras ? unknown_positions(num_cameras, cam_ldim, ord) : unknown_positions(1, &n, ord);
    const int span = ord.active ? ord.span : n;
    OSFM_RETURN_IF(select_device(0));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    hipStream_t s = sg.s;
    DevArray ord_nz, ord_ptiles;
    FlowPattern pattern;
    if (ord.active) {
        OSFM_RETURN_IF(upload(ord_nz, ord.nz.data(), ord.nz.size(), s));
        OSFM_RETURN_IF(upload(ord_ptiles, ord.ptiles.data(), ord.ptiles.size(), s));
        pattern.nz = ord_nz.as<unsigned long long>(); pattern.ptiles = ord_ptiles.as<int32_t>(); pattern.num_ptiles = (int)ord.ptiles.size();
    }
    const FlowPlan pl = chol_flow_plan(span, form == 0, pattern, max_d, max_groups);
    if ((max_d || max_groups) && !pl.flow) {
        set_error("%s: the one-launch form cannot run with max_d %d / max_groups %d (%d groups for %d D's, %d P's for %d tiles)",
            what, max_d, max_groups, pl.groups, pl.num_d, pl.num_p, pl.num_tiles);
        return OSFM_E_ARG;
    }
    // the solve's buffers, one set for the whole batch: flags zeroed once, the factor's matrix filled with NaN once and
    // never cleared again -- a tile read before its producer wrote it is the previous system's, or NaN
    CholeskyBuffers ch;
    OSFM_RETURN_IF(ch.alloc(span, form == 0, s));
    const int N = ch.N;
    DevArray infod;
    OSFM_RETURN_IF(infod.alloc((size_t)num_systems * 4));
    OSFM_HIP_CHECK(hipMemsetAsync(ch.L.ptr, 0xff, ch.s_elems * 8, s));
    OSFM_HIP_CHECK(hipMemsetAsync(ch.Ldiag.ptr, 0xff, (size_t)N * 32 * 8, s));
    OSFM_HIP_CHECK(hipMemsetAsync(ch.y.ptr, 0xff, (size_t)N * 8, s));
    OSFM_HIP_CHECK(hipMemsetAsync(infod.ptr, 0, (size_t)num_systems * 4, s));
    // the laid-out system as the pair pass leaves it: lower triangle (the factorisation reads nothing else), the identity
    // on the padding diagonal -- interior (ordered layout) and tail (ba_reset_system_kernel) --, the right-hand side in row N
    std::vector<double> h(ch.s_elems), hx((size_t)N);
    int used = 0;
    for (int r = 0; r < num_systems; ++r) {
        std::fill(h.begin(), h.end(), 0.0);
        for (int i = 0; i < N; ++i) h[(size_t)i * N + i] = 1.0;      // (every unknown's diagonal is overwritten below)
        const double *Ar = A + (size_t)r * n * n, *br = b + (size_t)r * n;
        for (int u = 0; u < n; ++u) {
            for (int v = 0; v < n; ++v) {
                const int pu = pos[u], pv = pos[v];
                if (pv <= pu) h[(size_t)pu * N + pv] = Ar[(size_t)u * n + v];
            }
            h[(size_t)N * N + pos[u]] = br[u];
        }
        OSFM_HIP_CHECK(hipMemcpyAsync(ch.S.ptr, h.data(), ch.s_elems * 8, hipMemcpyHostToDevice, s));
        used = ch.solve(span, infod.as<int>() + r, nullptr, ch.flow, pattern, s, max_d, max_groups);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipMemcpyAsync(hx.data(), ch.y.ptr, (size_t)N * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(info + r, infod.as<int32_t>() + r, 4, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));            // (h and hx are reused by the next system)
        for (int u = 0; u < n; ++u) x[(size_t)r * n + u] = hx[pos[u]];
    }
    if (launch) {
        const int32_t v[8] = {used, pl.groups, pl.num_d, pl.num_p, pl.num_tiles, ord.active ? ord.arcs : 0, span, N / 32};
        memcpy(launch, v, sizeof(v));
    }
    return OSFM_OK;
}

int osfm_ba_options_default(osfm_ba_options *o)
{
    if (!o) { set_error("ba_options_default: null"); return OSFM_E_ARG; }
    o->huber_delta = 1.0;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-10;
    o->max_num_iterations = 100;
    o->optimize_points = 1;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->jacobi_scaling = 1;
    o->max_consecutive_invalid_steps = 5;
    o->device = 0;
    o->verbose = 0;
    o->retriangulate_points = 0;
    o->small_form = 0;
    return OSFM_OK;
}

int osfm_ba_small_limits(int32_t *max_cameras, int32_t *track_chunk, int32_t *auto_max_observations)
{
    if (max_cameras) *max_cameras = kSmallMaxCams;
    if (track_chunk) *track_chunk = kSmallTrackChunk;
    if (auto_max_observations) *auto_max_observations = kSmallAutoMaxObs;
    return OSFM_OK;
}

// osfm_ba_solve; cap: osfm_ba_debug_linearization's copies (null: none)
static int ba_solve_host(const osfm_ba_problem *p, const osfm_ba_options *opt, osfm_ba_summary *sum, osfm_ba_lin_capture *cap)
{
    if (!sum) { set_error("ba_solve: null summary"); return OSFM_E_ARG; }
    memset(sum, 0, sizeof(*sum));
    const auto t_begin = Clock::now();
    OSFM_RETURN_IF(validate_header(p, "ba_solve"));
    osfm_ba_options o;
    if (opt) o = *opt; else osfm_ba_options_default(&o);
    OSFM_RETURN_IF(check_small_form(o, p->num_cameras, cap != nullptr, cap ? "ba_debug_linearization" : "ba_solve"));
    // The sweep over the caller's observations (range / order / one-observation-per-camera checks, the points'
    // observation counts, the copy of the start points) takes as long as queueing the uploads does (0.4 ms each for
    // BASELINE config 4: pageable arrays are staged by the calling thread): for problems of that size it runs on a
    // thread of its own beside them.  What it finds is looked at before anything is computed.
    Layout L;
    const int C = p->num_cameras, M = p->num_points;
    std::vector<double> pts0;
    std::string sweep_error;
    auto sweep = [&]() -> int {
        const int rc = validate_observations(p, "ba_solve", &L);
        if (rc != OSFM_OK) { sweep_error = osfm_last_error(); return rc; }      // (the message is per thread)
        // the points the optimisation starts from (tracksBackup, bundle_adjustment.cpp:99)
        pts0.resize((size_t)4 * M);
        if (M) memcpy(pts0.data(), p->points, (size_t)4 * M * 8);
        return OSFM_OK;
    };
    bool beside = p->num_observations >= 100000;
    std::future<int> swept;
    if (beside) {
        // (no thread to be had: the sweep runs here, in front of the uploads, as for small problems)
        try { swept = std::async(std::launch::async, sweep); } catch (const std::exception &) { beside = false; }
    }
    if (!beside) OSFM_RETURN_IF(sweep());
    struct Joiner { std::future<int> &f; ~Joiner() { if (f.valid()) f.wait(); } } joiner{swept};     // never leave it running
    OSFM_RETURN_IF(select_device(o.device));

    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    hipStream_t s = sg.s;

    // (D is declared before L: the transfers queued from L's vectors are waited for before either goes)
    DeviceProblem D;
    OSFM_RETURN_IF(upload_caller_arrays(p, s, &D));
    lap(o.verbose, t_begin, "caller arrays queued");
    if (beside) {
        const int rc = swept.get();
        if (rc != OSFM_OK) {
            OSFM_HIP_CHECK(hipStreamSynchronize(s));       // the queued uploads, before their buffers go back to the pool
            set_error("%s", sweep_error.c_str());
            return rc;
        }
    }
    build_camera_layout(p->model, C, p->cam_const, &L);
    const int pdim = o.optimize_points ? 3 : 0;
    lap(o.verbose, t_begin, "layout");
    OSFM_RETURN_IF(upload_problem(p, L, o.huber_delta, pdim, s, &D, true));
    if (o.retriangulate_points && M > 0) {
        // triangulateTracks(cameras, localTracks, true) in front of the solve (bundle_adjustment.cpp:77-83)
        OSFM_HIP_CHECK(hipMemcpyAsync(D.points[1].ptr, D.points[0].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToDevice, s));
        launch_triangulate(D.dev, D.points[1].as<double>(), nullptr, s);
        OSFM_HIP_CHECK(hipMemcpyAsync(D.points[0].ptr, D.points[1].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToDevice, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(pts0.data(), D.points[1].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToHost, s));
    }
    lap(o.verbose, t_begin, "upload problem");

    int64_t bound = 0;
    for (int j = 0; j < M; ++j) {
        const int64_t l = L.pt_start[j + 1] - L.pt_start[j];
        bound += pdim ? l * l : l;
    }
    int cur = 0;
    OSFM_RETURN_IF(ba_solve_core(D, o, sg, bound, sum, &cur, cap));
    // ---- write back the current iterate --------------------------------------
    if (C) OSFM_HIP_CHECK(hipMemcpyAsync(p->cam_params, D.cams[cur].ptr, (size_t)7 * C * 8, hipMemcpyDeviceToHost, s));
    if (M) OSFM_HIP_CHECK(hipMemcpyAsync(p->points, D.points[cur].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    double mx = 0.0, acc = 0.0;
    for (int j = 0; j < M; ++j) {       // bundle_adjustment.cpp:150-160
        double dd = 0.0;
        for (int i = 0; i < 4; ++i) { const double e = pts0[4 * j + i] - p->points[4 * j + i]; dd += e * e; }
        dd = std::sqrt(dd); mx = std::max(mx, dd); acc += dd;
    }
    sum->mean_point_change = M ? acc / M : 0.0;
    sum->max_point_change = mx;
    sum->solve_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_begin).count();
    return OSFM_OK;
}

int osfm_ba_solve(const osfm_ba_problem *p, const osfm_ba_options *opt, osfm_ba_summary *sum)
{
    return ba_solve_host(p, opt, sum, nullptr);
}

int osfm_ba_debug_linearization(const osfm_ba_problem *p, const osfm_ba_options *opt, osfm_ba_lin_capture *cap)
{
    if (!cap) { set_error("ba_debug_linearization: null capture"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(validate_header(p, "ba_debug_linearization"));
    // the arrays are the caller's, sized for its nc: the layout's must be the same
    Layout L;
    build_camera_layout(p->model, p->num_cameras, p->cam_const, &L);
    if (cap->nc != L.nc) {
        set_error("ba_debug_linearization: the capture is sized for %d camera columns, the problem has %d", cap->nc, L.nc);
        return OSFM_E_ARG;
    }
    const bool any_c = p->num_cameras > 0, any_p = p->num_points > 0;
    if ((any_c && (!cap->scale_c || !cap->diag_c || !cap->S || !cap->rhs || !cap->y_c || !cap->cand_cams)) ||
        (any_p && (!cap->scale_p || !cap->diag_p || !cap->vinv || !cap->ge || !cap->cand_points))) {
        set_error("ba_debug_linearization: null capture array"); return OSFM_E_ARG;
    }
    osfm_ba_summary sum;
    return ba_solve_host(p, opt, &sum, cap);
}

int osfm_ba_reprojection_errors(const osfm_ba_problem *p, int device, double *err, double *residuals)
{
    Layout L;                 // declared before the stream lease: it must outlive the copies that read it
    OSFM_RETURN_IF(validate_problem(p, "ba_reprojection_errors", &L));
    if (!err && !residuals) { set_error("ba_reprojection_errors: no output"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(select_device(device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DeviceProblem D;
    OSFM_RETURN_IF(upload_problem(p, L, 1.0, 3, sg.s, &D));
    const int O = p->num_observations;
    DevArray d_err, d_res;
    OSFM_RETURN_IF(d_err.alloc((size_t)O * 8));
    OSFM_RETURN_IF(d_res.alloc((size_t)2 * O * 8));
    launch_reproj(D.dev, d_err.as<double>(), d_res.as<double>(), sg.s);
    OSFM_HIP_CHECK(hipGetLastError());
    if (err && O) OSFM_HIP_CHECK(hipMemcpyAsync(err, d_err.ptr, (size_t)O * 8, hipMemcpyDeviceToHost, sg.s));
    if (residuals && O) OSFM_HIP_CHECK(hipMemcpyAsync(residuals, d_res.ptr, (size_t)2 * O * 8, hipMemcpyDeviceToHost, sg.s));
    OSFM_HIP_CHECK(hipStreamSynchronize(sg.s));
    return OSFM_OK;
}

int osfm_ba_triangulate(const osfm_ba_problem *p, int device, uint8_t *point_valid)
{
    Layout L;                 // declared before the stream lease: it must outlive the copies that read it
    OSFM_RETURN_IF(validate_problem(p, "ba_triangulate", &L));
    OSFM_RETURN_IF(select_device(device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DeviceProblem D;
    OSFM_RETURN_IF(upload_problem(p, L, 1.0, 3, sg.s, &D));
    const int M = p->num_points;
    DevArray d_valid;
    OSFM_RETURN_IF(d_valid.alloc((size_t)std::max(M, 1)));
    // points of tracks with fewer than two rays keep their input value
    OSFM_HIP_CHECK(hipMemcpyAsync(D.points[1].ptr, D.points[0].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToDevice, sg.s));
    launch_triangulate(D.dev, D.points[1].as<double>(), d_valid.as<uint8_t>(), sg.s);
    OSFM_HIP_CHECK(hipGetLastError());
    if (M) OSFM_HIP_CHECK(hipMemcpyAsync(p->points, D.points[1].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToHost, sg.s));
    if (point_valid && M) OSFM_HIP_CHECK(hipMemcpyAsync(point_valid, d_valid.ptr, (size_t)M, hipMemcpyDeviceToHost, sg.s));
    OSFM_HIP_CHECK(hipStreamSynchronize(sg.s));
    return OSFM_OK;
}

int osfm_filter_reprojection(const osfm_ba_problem *p, int device, double max_error,
    uint8_t *obs_keep, uint8_t *point_valid, double *err)
{
    Layout L;                 // declared before the stream lease: it must outlive the copies that read it
    OSFM_RETURN_IF(validate_problem(p, "filter_reprojection", &L));
    if (!obs_keep && p->num_observations > 0) { set_error("filter_reprojection: obs_keep is null"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(select_device(device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DeviceProblem D;
    OSFM_RETURN_IF(upload_problem(p, L, 1.0, 3, sg.s, &D));
    const int M = p->num_points, O = p->num_observations;
    DevArray d_valid, d_err, d_res;
    OSFM_RETURN_IF(d_valid.alloc((size_t)std::max(M, 1)));
    OSFM_RETURN_IF(d_err.alloc((size_t)std::max(O, 1) * 8));
    OSFM_RETURN_IF(d_res.alloc((size_t)2 * std::max(O, 1) * 8));
    // triangulate into the spare point array (tracks with fewer than two rays
    // keep their input point), then evaluate against the triangulated points
    OSFM_HIP_CHECK(hipMemcpyAsync(D.points[1].ptr, D.points[0].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToDevice, sg.s));
    launch_triangulate(D.dev, D.points[1].as<double>(), d_valid.as<uint8_t>(), sg.s);
    OSFM_HIP_CHECK(hipMemcpyAsync(D.points[0].ptr, D.points[1].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToDevice, sg.s));
    launch_reproj(D.dev, d_err.as<double>(), d_res.as<double>(), sg.s);
    OSFM_HIP_CHECK(hipGetLastError());
    std::vector<double> herr((size_t)std::max(O, 1));
    if (O) OSFM_HIP_CHECK(hipMemcpyAsync(herr.data(), d_err.ptr, (size_t)O * 8, hipMemcpyDeviceToHost, sg.s));
    if (M) OSFM_HIP_CHECK(hipMemcpyAsync(p->points, D.points[1].ptr, (size_t)4 * M * 8, hipMemcpyDeviceToHost, sg.s));
    if (point_valid && M) OSFM_HIP_CHECK(hipMemcpyAsync(point_valid, d_valid.ptr, (size_t)M, hipMemcpyDeviceToHost, sg.s));
    OSFM_HIP_CHECK(hipStreamSynchronize(sg.s));
    for (int k = 0; k < O; ++k) {
        obs_keep[k] = herr[k] < max_error ? 1 : 0;
        if (err) err[k] = herr[k];
    }
    return OSFM_OK;
}

}  // extern "C"
