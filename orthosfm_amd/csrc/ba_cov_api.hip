// osfm_ba_covariance (include/osfm_hip.h, section B): the gauge choice, the layout, and the covariance computation on a
// finished DeviceProblem that the scene's entry (scene_api.hip) runs as well.  DESIGN.md "Covariances".
#include <cmath>
#include <cstring>
#include <vector>

#include "ba_cov.h"
#include "ba_cov_kernels.h"

using namespace osfm;

namespace {

// rows of R (l = R p, the camera's linear map of the inhomogeneous point: ba_device.h's quat_local / euler_local): rows
// 0 and 1 are the image axes in the scene, row 2 the viewing axis
void camera_rows(int model, const double *cam, double R[3][3])
{
    if (model == OSFM_BA_MODEL_QUATERNION) {
        const double qx = cam[0], qy = cam[1], qz = cam[2], qw = cam[3];
        const double n2 = qx * qx + qy * qy + qz * qz + qw * qw;
        const double a[3] = {-qx / n2, -qy / n2, -qz / n2}, b = qw / n2;
        for (int k = 0; k < 3; ++k) {
            double p[3] = {0, 0, 0};
            p[k] = 1.0;
            const double t2[3] = {2 * (a[1] * p[2] - a[2] * p[1]), 2 * (a[2] * p[0] - a[0] * p[2]), 2 * (a[0] * p[1] - a[1] * p[0])};
            const double at2[3] = {a[1] * t2[2] - a[2] * t2[1], a[2] * t2[0] - a[0] * t2[2], a[0] * t2[1] - a[1] * t2[0]};
            for (int i = 0; i < 3; ++i) R[i][k] = p[i] + b * t2[i] + at2[i];
        }
        return;
    }
    const double phi = cam[0], om = cam[1] + 1.57079632679489661923, rho = cam[2];
    const double so = std::sin(om), co = std::cos(om), sr = std::sin(rho), cr = std::cos(rho), sp = std::sin(phi), cp = std::cos(phi);
    const double Rx[3][3] = {{1, 0, 0}, {0, co, -so}, {0, so, co}};
    const double Ry[3][3] = {{cr, -sr, 0}, {sr, cr, 0}, {0, 0, 1}};
    const double Rz[3][3] = {{cp, -sp, 0}, {sp, cp, 0}, {0, 0, 1}};
    double A[3][3], S[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = Rz[i][0] * Rx[0][j] + Rz[i][1] * Rx[1][j] + Rz[i][2] * Rx[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[i][j] = A[i][0] * Ry[0][j] + A[i][1] * Ry[1][j] + A[i][2] * Ry[2][j];
    // l_i = S[0][i] p_0 - S[1][i] p_2 + S[2][i] p_1
    for (int i = 0; i < 3; ++i) { R[i][0] = S[0][i]; R[i][1] = S[2][i]; R[i][2] = -S[1][i]; }
}

inline int offset_slot(int model, int axis) { return (model == OSFM_BA_MODEL_QUATERNION ? 4 : 3) + axis; }

bool all_constant(int model, const uint8_t *cc)
{
    if (model == OSFM_BA_MODEL_QUATERNION) return cc[0] && cc[4] && cc[5] && cc[6];
    for (int s = 0; s < 6; ++s) if (!cc[s]) return false;
    return true;
}

int arg_error(const char *what, const char *msg) { set_error("%s: %s", what, msg); return OSFM_E_ARG; }

}  // namespace

namespace osfm {

void cov_choose_gauge(int model, int C, const double *cams, const uint8_t *cam_const, int32_t *camera, int32_t *axis)
{
    *camera = -1; *axis = -1;
    int c0 = -1;
    for (int c = 0; c < C && c0 < 0; ++c) if (all_constant(model, cam_const + 7 * c)) c0 = c;
    if (c0 < 0) return;
    double R0[3][3];
    camera_rows(model, cams + 7 * c0, R0);
    const double n0 = std::sqrt(R0[2][0] * R0[2][0] + R0[2][1] * R0[2][1] + R0[2][2] * R0[2][2]);
    double best = 2.0;
    for (int c = 0; c < C; ++c) {
        const uint8_t *cc = cam_const + 7 * c;
        if (cc[offset_slot(model, 0)] || cc[offset_slot(model, 1)]) continue;
        double R[3][3];
        camera_rows(model, cams + 7 * c, R);
        const double n = std::sqrt(R[2][0] * R[2][0] + R[2][1] * R[2][1] + R[2][2] * R[2][2]);
        const double cosine = std::fabs(R[2][0] * R0[2][0] + R[2][1] * R0[2][1] + R[2][2] * R0[2][2]) / (n * n0);
        if (!(cosine < best)) continue;              // the largest angle between the axes as lines; ties: the lowest index
        best = cosine;
        const double ax = std::fabs(R[0][0] * R0[2][0] + R[0][1] * R0[2][1] + R[0][2] * R0[2][2]);
        const double ay = std::fabs(R[1][0] * R0[2][0] + R[1][1] * R0[2][1] + R[1][2] * R0[2][2]);
        *camera = c; *axis = ay > ax ? 1 : 0;
    }
}

std::vector<uint8_t> cov_held_masks(int model, int C, const uint8_t *cam_const, int camera, int axis)
{
    std::vector<uint8_t> cc(cam_const, cam_const + (size_t)7 * C);
    if (camera >= 0) cc[(size_t)7 * camera + offset_slot(model, axis)] = 1;
    return cc;
}

int ba_cov_core(const DeviceProblem &D, const osfm_ba_cov_options &o, StreamLease &sg, bool want_blocks, bool want_full,
    bool want_points, osfm_ba_cov_result *res, CovHost *out)
{
    const auto t_begin = Clock::now();
    hipStream_t s = sg.s;
    const int C = D.dev.C, M = D.dev.M, O = D.dev.O, nc = D.dev.nc, pdim = D.dev.pdim;
    if (nc > OSFM_BA_COV_MAX_UNKNOWNS) {
        set_error("ba_covariance: %d camera unknowns, at most %d (three dense arrays of that square)", nc, OSFM_BA_COV_MAX_UNKNOWNS);
        return OSFM_E_CAPACITY;
    }
    if (!(o.min_pivot_ratio >= 0.0) || !(o.min_pivot_ratio < 1.0)) return arg_error("ba_covariance", "min_pivot_ratio outside [0, 1)");
    OSFM_RETURN_IF(sg.set->ensure_events(5));
    std::vector<hipEvent_t> &ev = sg.set->events;
    OSFM_HIP_CHECK(hipEventRecord(ev[0], s));

    // ---- the points that stay in the system (behind a first point pass over all of them) ----
    DevArray d_valid;
    OSFM_RETURN_IF(d_valid.alloc((size_t)std::max(M, 1)));
    std::vector<uint8_t> valid((size_t)M, 1);
    std::vector<int32_t> pt_start((size_t)M + 1, 0);
    constexpr int kRedo = 1;
    int dropped_obs = 0;
    auto check_points = [&](const PlainLin &lin) -> int {
        if (!pdim || !M) return 0;
        launch_cov_point_valid(D.dev, lin.obsrec, o.min_pivot_ratio, d_valid.as<uint8_t>(), s);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipMemcpyAsync(valid.data(), d_valid.ptr, (size_t)M, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        for (int j = 0; j < M; ++j) if (!valid[j]) dropped_obs += pt_start[j + 1] - pt_start[j];
        return dropped_obs ? kRedo : 0;
    };

    // ---- everything behind the pair pass, on the problem d that was linearised ----
    double h_ratio = 1.0, cost = 0.0;
    int32_t h_info = 0;
    DevArray sdiag, ratio, Z, Sinv, d_blocks, d_full, d_rows, d_pcov;
    auto finish = [&](const BaDev &d, const PlainLin &lin) -> int {
        CholeskyBuffers &ch = *lin.chol;
        const int N = ch.N;
        OSFM_HIP_CHECK(hipEventRecord(ev[1], s));
        OSFM_RETURN_IF(sdiag.alloc((size_t)N * 8));
        OSFM_RETURN_IF(ratio.alloc(16));
        launch_cov_save_diagonal(ch.S.as<double>(), N, sdiag.as<double>(), s);
        int32_t *info = reinterpret_cast<int32_t *>(ratio.as<double>() + 1);
        OSFM_HIP_CHECK(hipMemsetAsync(info, 0, 4, s));
        // the launch-per-column form: a one-off call gains nothing from the one-launch form, which waits on other workgroups
        ch.solve(std::max(nc, 1), info, nullptr, false, FlowPattern(), s);
        launch_cov_pivot_ratio(ch.Ldiag.as<double>(), sdiag.as<double>(), nc, ratio.as<double>(), s);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipEventRecord(ev[2], s));
        std::vector<double> parts((size_t)lin.num_windows);
        OSFM_HIP_CHECK(hipMemcpyAsync(parts.data(), lin.cost_partials, parts.size() * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(&h_ratio, ratio.ptr, 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(&h_info, info, 4, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        for (double v : parts) cost += v;
        if (h_info != 0) h_ratio = 0.0;
        if (!(h_ratio >= o.min_pivot_ratio)) return OSFM_OK;      // (reported by the caller of this lambda)
        // ---- S^-1 = Z^T Z, Z = L^-1 ----
        OSFM_RETURN_IF(Z.alloc((size_t)N * N * 8));
        OSFM_RETURN_IF(Sinv.alloc((size_t)N * N * 8));
        launch_cov_factor_inverse(ch.L.as<double>(), ch.Ldiag.as<double>(), N, Z.as<double>(), s);
        launch_cov_gram(Z.as<double>(), N, Sinv.as<double>(), s);
        if (want_blocks) OSFM_RETURN_IF(d_blocks.alloc((size_t)std::max(C, 1) * 36 * 8));
        if (want_full) OSFM_RETURN_IF(d_full.alloc((size_t)std::max(nc, 1) * std::max(nc, 1) * 8));
        launch_cov_camera_blocks(d, Sinv.as<double>(), N, want_blocks ? d_blocks.as<double>() : nullptr,
            want_full ? d_full.as<double>() : nullptr, s);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipEventRecord(ev[3], s));
        // ---- the points ----
        if (pdim && want_points && M) {
            OSFM_RETURN_IF(d_rows.alloc((size_t)std::max(d.O, 1) * 9 * 8));
            OSFM_RETURN_IF(d_pcov.alloc((size_t)M * 9 * 8));
            OSFM_HIP_CHECK(hipMemcpyAsync(d_valid.ptr, valid.data(), (size_t)M, hipMemcpyHostToDevice, s));
            if (nc > 0) launch_cov_point_rows(d, lin.obsrec, lin.obs_lay, Sinv.as<double>(), N, d_rows.as<double>(), s);
            launch_cov_point_finish(d, lin.vinv, nc > 0 ? d_rows.as<double>() : nullptr, d_valid.as<uint8_t>(), d_pcov.as<double>(), s);
            OSFM_HIP_CHECK(hipGetLastError());
        }
        OSFM_HIP_CHECK(hipEventRecord(ev[4], s));
        if (want_blocks && C) { out->cam_cov.resize((size_t)C * 36); OSFM_HIP_CHECK(hipMemcpyAsync(out->cam_cov.data(), d_blocks.ptr, (size_t)C * 36 * 8, hipMemcpyDeviceToHost, s)); }
        if (want_full && nc) { out->full.resize((size_t)nc * nc); OSFM_HIP_CHECK(hipMemcpyAsync(out->full.data(), d_full.ptr, (size_t)nc * nc * 8, hipMemcpyDeviceToHost, s)); }
        if (pdim && want_points && M) { out->point_cov.resize((size_t)M * 9); OSFM_HIP_CHECK(hipMemcpyAsync(out->point_cov.data(), d_pcov.ptr, (size_t)M * 9 * 8, hipMemcpyDeviceToHost, s)); }
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        res->dense_schur = lin.dense ? 1 : 0;
        return OSFM_OK;
    };

    int64_t bound = 0;
    OSFM_HIP_CHECK(hipMemcpyAsync(pt_start.data(), D.dev.pt_start, ((size_t)M + 1) * 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    auto pair_bound = [&](const std::vector<int32_t> &ps) {
        int64_t b = 0;
        for (int j = 0; j < M; ++j) { const int64_t l = ps[j + 1] - ps[j]; b += pdim ? l * l : l; }
        return b;
    };
    bound = pair_bound(pt_start);
    int used_obs = O;
    int rc = ba_linearize_plain(D, sg, bound, check_points, [&](const PlainLin &lin) { return finish(D.dev, lin); });
    // (the second problem's arrays: declared here so that they outlive the work queued on them)
    DeviceProblem D2;
    DevArray d_map;
    std::vector<int32_t> pt2, map;
    if (rc == kRedo) {
        // some point with observations is invalid: the same problem without those observations (the points keep their
        // numbers; an invalid one has no observation left and adds nothing)
        pt2.assign((size_t)M + 1, 0);
        map.reserve((size_t)O);
        for (int j = 0; j < M; ++j) {
            if (valid[j]) for (int k = pt_start[j]; k < pt_start[j + 1]; ++k) map.push_back(k);
            pt2[j + 1] = (int32_t)map.size();
        }
        const int O2 = (int)map.size();
        used_obs = O2;
        OSFM_RETURN_IF(upload(d_map, map.data(), map.size(), s));
        OSFM_RETURN_IF(upload(D2.pt_start, pt2.data(), pt2.size(), s));
        OSFM_RETURN_IF(D2.obs_xy.alloc((size_t)std::max(O2, 1) * 16));
        OSFM_RETURN_IF(D2.obs_cam.alloc((size_t)std::max(O2, 1) * 4));
        launch_cov_gather_obs(O2, d_map.as<int32_t>(), D.dev.obs_xy, D.dev.obs_cam, D2.obs_xy.as<double>(), D2.obs_cam.as<int32_t>(), s);
        OSFM_RETURN_IF(finish_device_problem(D.dev.model, C, M, O2, nc, D.dev.huber, pdim, s, &D2));
        D2.dev.cams = D.dev.cams; D2.dev.points = D.dev.points; D2.dev.img_w = D.dev.img_w; D2.dev.img_h = D.dev.img_h;
        D2.dev.cam_ldim = D.dev.cam_ldim; D2.dev.cam_off = D.dev.cam_off; D2.dev.cam_colmap = D.dev.cam_colmap;
        OSFM_HIP_CHECK(hipGetLastError());
        rc = ba_linearize_plain(D2, sg, pair_bound(pt2), [](const PlainLin &) { return 0; },
            [&](const PlainLin &lin) { return finish(D2.dev, lin); });
    }
    OSFM_RETURN_IF(rc);
    int num_valid = 0;
    if (pdim) for (int j = 0; j < M; ++j) num_valid += valid[j];
    res->cost = cost;
    res->num_residuals = 2 * used_obs;
    res->num_camera_unknowns = nc;
    res->num_valid_points = num_valid;
    res->num_unknowns = nc + 3 * num_valid;
    const int dof = res->num_residuals - res->num_unknowns;
    res->variance_factor = dof > 0 ? 2.0 * cost / dof : 0.0;
    res->min_pivot_seen = h_ratio;
    float ms[4] = {0, 0, 0, 0};
    const bool deficient = !(h_ratio >= o.min_pivot_ratio);
    for (int i = 0; i < (deficient ? 2 : 4); ++i) OSFM_HIP_CHECK(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    res->linearize_ms = ms[0]; res->factor_ms = ms[1]; res->inverse_ms = ms[2]; res->point_ms = ms[3];
    res->total_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_begin).count();
    if (deficient) {
        res->rank_deficient = 1;
        set_error("ba_covariance: the reduced camera system is rank deficient (smallest relative pivot %.3g < %.3g): a gauge freedom is open",
            h_ratio, o.min_pivot_ratio);
        return OSFM_E_NUMERIC;
    }
    if (pdim && want_points) out->valid = valid;
    return OSFM_OK;
}

}  // namespace osfm

extern "C" {

int osfm_ba_cov_options_default(osfm_ba_cov_options *o)
{
    if (!o) return arg_error("ba_cov_options_default", "null");
    o->huber_delta = 1.0;
    o->min_pivot_ratio = 1e-8;
    o->optimize_points = 1;
    o->depth_gauge = 1;
    o->device = 0;
    o->reserved = 0;
    return OSFM_OK;
}

int osfm_ba_covariance(const osfm_ba_problem *p, const osfm_ba_cov_options *opts, osfm_ba_cov_result *res)
{
    if (!res) return arg_error("ba_covariance", "null result");
    osfm_ba_cov_result r = *res;            // the caller's pointers and nc; the scalars are written back on every path behind the checks
    r.cost = r.variance_factor = r.min_pivot_seen = 0.0;
    r.num_residuals = r.num_unknowns = r.num_camera_unknowns = r.num_valid_points = 0;
    r.gauge_camera = r.gauge_axis = -1; r.rank_deficient = 0; r.dense_schur = 0;
    r.linearize_ms = r.factor_ms = r.inverse_ms = r.point_ms = r.total_ms = 0.0;
    osfm_ba_cov_options o;
    if (opts) o = *opts; else osfm_ba_cov_options_default(&o);
    Layout L;                 // declared before the stream lease: it must outlive the copies that read it
    OSFM_RETURN_IF(validate_ba_problem(p, "ba_covariance", &L));
    const int C = p->num_cameras, M = p->num_points;
    if (o.depth_gauge) cov_choose_gauge(p->model, C, p->cam_params, p->cam_const, &r.gauge_camera, &r.gauge_axis);
    const std::vector<uint8_t> masks = cov_held_masks(p->model, C, p->cam_const, r.gauge_camera, r.gauge_axis);
    build_camera_layout(p->model, C, masks.data(), &L);
    if (res->cam_cov_full && res->nc != L.nc) {
        res->num_camera_unknowns = L.nc; res->gauge_camera = r.gauge_camera; res->gauge_axis = r.gauge_axis;     // (what it should have been)
        set_error("ba_covariance: cam_cov_full is sized for %d camera columns, the problem has %d (the gauge column held)", res->nc, L.nc);
        return OSFM_E_ARG;
    }
    OSFM_RETURN_IF(select_device(o.device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DeviceProblem D;
    const int pdim = o.optimize_points ? 3 : 0;
    OSFM_RETURN_IF(upload_ba_problem(p, L, o.huber_delta, pdim, sg.s, &D));
    CovHost h;
    const int rc = ba_cov_core(D, o, sg, res->cam_cov != nullptr, res->cam_cov_full != nullptr,
        res->point_cov != nullptr || res->point_valid != nullptr, &r, &h);
    if (rc == OSFM_OK || rc == OSFM_E_NUMERIC) {
        const osfm_ba_cov_result keep = *res;
        *res = r;
        res->cam_cov = keep.cam_cov; res->cam_ldim = keep.cam_ldim; res->cam_cov_full = keep.cam_cov_full;
        res->point_cov = keep.point_cov; res->point_valid = keep.point_valid; res->nc = keep.nc; res->reserved = keep.reserved;
    }
    OSFM_RETURN_IF(rc);
    if (res->cam_ldim) for (int c = 0; c < C; ++c) res->cam_ldim[c] = L.cam_ldim[c];
    if (res->cam_cov && C) memcpy(res->cam_cov, h.cam_cov.data(), (size_t)C * 36 * 8);
    if (res->cam_cov_full && L.nc) memcpy(res->cam_cov_full, h.full.data(), (size_t)L.nc * L.nc * 8);
    if (pdim && M) {
        if (res->point_cov) memcpy(res->point_cov, h.point_cov.data(), (size_t)M * 9 * 8);
        if (res->point_valid) memcpy(res->point_valid, h.valid.data(), (size_t)M);
    }
    return OSFM_OK;
}

}  // extern "C"
