// ba_solve_core as stages: trust-region logic restated from the published Ceres 2.0/2.1 algorithm
// (TrustRegionMinimizer, LevenbergMarquardtStrategy) as runBundleAdjustment configures it (bundle_adjustment.cpp:126-145)
#include <cmath>
#include <limits>

#include "ba_solve.h"

namespace osfm {

namespace {

// the five OSFM_BA_* switches (A/B runs and tests), read where a solve makes its Switches: tests change them between solves
struct Switches {
    int order = getenv("OSFM_BA_ORDER") ? atoi(getenv("OSFM_BA_ORDER")) : 1;                   // 0: never order
    int dense = getenv("OSFM_BA_DENSE_SCHUR") ? atoi(getenv("OSFM_BA_DENSE_SCHUR")) : -1;      // -1: the cost model decides
    bool steps = getenv("OSFM_BA_CHOLESKY_STEPS"), separate_post = getenv("OSFM_BA_SEPARATE_POST"), separate_back = getenv("OSFM_BA_SEPARATE_BACK");
};

// The reduced camera system as laid out: observation windows, Schur pair lists, and the elimination order if one was chosen
struct SystemLayout {
    ObsWindows win;
    DevArray win_desc, win_over, win_ok, win_count, obs_lay;
    PairListsDev PL;
    ReducedOrder ord;
    DevArray cam_off, ord_nz, ord_ptiles, ord_pad;
    FlowPattern pattern;
    int span = 0, N = 0;        // unknowns laid out (interior padding included), padded to the Cholesky's blocks
};

// Windows, pair lists and the order, looked for where the system has at least eight block columns (ba_order.hip): it needs
// the camera pairs, so the pair lists come first then.  d.cam_off / d.nc become the solve's own.  Returns synchronised.
int lay_out_system(BaDev &d, const Switches &sw, int64_t pair_bound, int32_t *h_over, hipStream_t s, SystemLayout &y, osfm_ba_summary *sum)
{
    const int C = d.C;
    y.win.num = obs_windows_count(d.O);
    OSFM_RETURN_IF(y.win_desc.alloc((size_t)y.win.num * sizeof(WinDesc)));
    OSFM_RETURN_IF(y.win_over.alloc((size_t)y.win.num * 4));
    OSFM_RETURN_IF(y.win_ok.alloc((size_t)y.win.num * 4));
    OSFM_RETURN_IF(y.win_count.alloc(16));
    OSFM_RETURN_IF(y.obs_lay.alloc((size_t)std::max(d.O, 1) * 4));
    OSFM_HIP_CHECK(hipMemsetAsync(y.win_count.ptr, 0, 16, s));
    y.win.desc = y.win_desc.as<WinDesc>(); y.win.over_list = y.win_over.as<int32_t>(); y.win.ok_list = y.win_ok.as<int32_t>();
    y.win.obs_lay = y.obs_lay.as<int32_t>();
    // the observation windows (ba_kernels.h), behind the order where there is one: obs_lay holds the cameras' offsets;
    // the count of windows that need the other kernels comes back with the pair lists' synchronisation
    auto lay_out_windows = [&]() -> int {
        if (d.nc >= (1 << 24)) { set_error("ba_solve: more than 2^24 camera unknowns"); return OSFM_E_ARG; }
        launch_obs_windows(d, y.win.num, y.win_desc.as<WinDesc>(), y.win_over.as<int32_t>(), y.win_ok.as<int32_t>(),
            y.win_count.as<int32_t>(), y.obs_lay.as<int32_t>(), s);
        OSFM_HIP_CHECK(hipMemcpyAsync(h_over, y.win_count.ptr, 4, hipMemcpyDeviceToHost, s));
        return OSFM_OK;
    };
    const bool may_order = sw.order != 0 && d.pdim != 0 && cholesky_padded_dim(std::max(d.nc, 1)) / 32 >= 8 && !sw.steps;
    if (!may_order) OSFM_RETURN_IF(lay_out_windows());
    OSFM_RETURN_IF(pair_lists_build(d, d.pdim != 0, std::max<int64_t>(pair_bound, 1), &y.PL, s, sw.dense));
    const int num_pairs = y.PL.num_pairs;
    sum->num_pair_entries = y.PL.dense ? y.PL.num_entries_all : y.PL.num_entries;
    if (may_order && !y.PL.dense && num_pairs > 0) {
        // the camera pairs that share a track (the unique keys of the lists) and the cameras' block sizes
        std::vector<uint32_t> keys((size_t)num_pairs);
        std::vector<int32_t> ldim((size_t)C);
        OSFM_HIP_CHECK(hipMemcpyAsync(keys.data(), y.PL.unique.ptr, (size_t)num_pairs * 4, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(ldim.data(), d.cam_ldim, (size_t)C * 4, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        std::vector<std::pair<int, int>> cpairs((size_t)num_pairs);
        const uint32_t g = (uint32_t)y.PL.group, Cu = (uint32_t)C;
        for (int i = 0; i < num_pairs; ++i) cpairs[i] = {(int)((keys[i] / (Cu * g)) * g + keys[i] % g), (int)((keys[i] / g) % Cu)};
        if (choose_reduced_order(C, ldim.data(), cpairs, &y.ord)) {
            OSFM_RETURN_IF(upload(y.cam_off, y.ord.cam_off.data(), (size_t)C, s));
            d.cam_off = y.cam_off.as<int32_t>(); d.nc = y.ord.span;
            OSFM_RETURN_IF(upload(y.ord_nz, y.ord.nz.data(), y.ord.nz.size(), s));
            OSFM_RETURN_IF(upload(y.ord_ptiles, y.ord.ptiles.data(), y.ord.ptiles.size(), s));
            OSFM_RETURN_IF(upload(y.ord_pad, y.ord.pad.data(), y.ord.pad.size(), s));
            y.pattern = {y.ord_nz.as<unsigned long long>(), y.ord_ptiles.as<int32_t>(), (int)y.ord.ptiles.size()};
        }
    }
    if (may_order) OSFM_RETURN_IF(lay_out_windows());
    sum->order_arcs = y.ord.active ? y.ord.arcs : 0;
    sum->chain_blocks_natural = y.ord.chain_natural; sum->chain_blocks = y.ord.active ? y.ord.chain_ordered : y.ord.chain_natural;
    y.span = d.nc; y.N = cholesky_padded_dim(std::max(y.span, 1));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));     // (pair_lists_build has synchronised: this returns at once)
    y.win.num_over = *h_over;
    return OSFM_OK;
}

// The solve's work arrays.  What has to start at zero -- the cameras' partials and gradient norms, the Cholesky's info word,
// the tickets of the fused tails -- is one block and one memset (four were 30 us of a 3-camera adjustment's set-up)
struct Workspace {
    DevArray obsrec, diag_c, diag_p, vinv, ge, partA, partB, partC, zeros, scale_c, scale_p, camder[2], lm;
    DevArray dense_z, dense_w, dense_partial;    // dense visibility: S's point part as a product (ba_dense.hip)
    CholeskyBuffers chol;
    double *part_cam = nullptr, *gmax_cam = nullptr;     // pieces of zeros
    int32_t *info = nullptr, *tickets = nullptr;
};

// d (laid out): gets the scales and the camera tables; the tables of the start cameras are queued
int allocate_workspace(BaDev &d, const SystemLayout &y, const Switches &sw, hipStream_t s, Workspace &w)
{
    const int C = d.C, M = d.M, nc = y.span, blocksM = y.win.num;
    if (y.PL.dense) {
        const size_t zw = (size_t)schur_dense_rows(nc) * schur_dense_cols(M) * 8;
        OSFM_RETURN_IF(w.dense_z.alloc(zw)); OSFM_RETURN_IF(w.dense_w.alloc(zw));
        OSFM_RETURN_IF(w.dense_partial.alloc(schur_dense_partial_bytes(nc, M)));
    }
    OSFM_RETURN_IF(w.obsrec.alloc((size_t)std::max(d.O, 1) * kObsRec * 8));
    OSFM_RETURN_IF(w.diag_c.alloc((size_t)nc * 8));
    OSFM_RETURN_IF(w.diag_p.alloc((size_t)3 * M * 8));
    OSFM_RETURN_IF(w.vinv.alloc((size_t)9 * M * 8));
    OSFM_RETURN_IF(w.ge.alloc((size_t)3 * M * 8));
    OSFM_RETURN_IF(w.partA.alloc((size_t)3 * blocksM * 8));
    OSFM_RETURN_IF(w.partB.alloc((size_t)3 * blocksM * 8));
    OSFM_RETURN_IF(w.partC.alloc((size_t)blocksM * 8));
    // the Jacobi scales start at one (what stands without Jacobi scaling; the padding's stays so)
    OSFM_RETURN_IF(w.scale_c.alloc((size_t)nc * 8));
    launch_fill(w.scale_c.as<double>(), (size_t)nc, 1.0, s);
    OSFM_RETURN_IF(w.scale_p.alloc((size_t)3 * M * 8));
    launch_fill(w.scale_p.as<double>(), (size_t)3 * M, 1.0, s);
    d.scale_c = w.scale_c.as<double>(); d.scale_p = w.scale_p.as<double>();
    auto r256 = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t z_part = 0, z_gmax = z_part + r256((size_t)2 * std::max(C, 1) * 8), z_info = z_gmax + r256((size_t)std::max(C, 1) * 8),
                 z_tick = z_info + 256, z_end = z_tick + r256(2 * lm_ticket_bytes());
    OSFM_RETURN_IF(w.zeros.alloc(z_end));
    OSFM_HIP_CHECK(hipMemsetAsync(w.zeros.ptr, 0, z_end, s));
    char *z = w.zeros.as<char>();
    w.part_cam = reinterpret_cast<double *>(z + z_part); w.gmax_cam = reinterpret_cast<double *>(z + z_gmax);
    w.info = reinterpret_cast<int32_t *>(z + z_info); w.tickets = reinterpret_cast<int32_t *>(z + z_tick);
    OSFM_RETURN_IF(w.chol.alloc(nc, !sw.steps, s));
    // the cameras' derived tables, one per iterate buffer: whoever writes cameras writes their rows
    OSFM_RETURN_IF(w.camder[0].alloc((size_t)std::max(C, 1) * kCamDer * 8));
    OSFM_RETURN_IF(w.camder[1].alloc((size_t)std::max(C, 1) * kCamDer * 8));
    d.camder = d.camder2[0] = w.camder[0].as<double>(); d.camder2[1] = w.camder[1].as<double>();
    launch_cam_derive(d, d.cams, d.camder2[0], s);
    return OSFM_OK;
}

// kernel-family timing (o.verbose): event pairs from the events behind the iteration slots (out of them: untimed)
struct KernelTimer {
    std::vector<hipEvent_t> &evs;
    bool on;
    size_t next;                                   // the next free event
    std::vector<std::pair<size_t, int>> pairs;     // (first event of the pair, family)
    bool off() const { return !on || next + 1 >= evs.size(); }
    int tic(int family, hipStream_t s) { if (!off()) { OSFM_HIP_CHECK(hipEventRecord(evs[next], s)); pairs.push_back({next, family}); } return OSFM_OK; }
    int toc(hipStream_t s) { if (!off()) { OSFM_HIP_CHECK(hipEventRecord(evs[next + 1], s)); next += 2; } return OSFM_OK; }
};

enum { kPostNone = 0, kPostInitial = 1, kPostLoop = 2 };

// What every iteration launches with: the solve's BaDev, the passes' arguments over the workspace, the forms taken
struct LmRun {
    BaDev d;
    PointPassArgs pa;
    PairPassArgs qa;
    LmParams prm;
    LmScratch sc;
    LmDev *lm;                // the state on the device
    // post_fused / back_fused: the LM control rides in the tails of the pair / back pass (which also makes and evaluates
    // the candidate), DESIGN.md §3.3.  small: one block of unknowns -- the solve and the candidate cameras are one launch
    bool post_fused, back_fused, small, eager, dense_first;
    KernelTimer timer;
};

LmRun make_run(const BaDev &d, const osfm_ba_options &o, const Switches &sw, const SystemLayout &y, const Workspace &w,
    std::vector<hipEvent_t> &evs, size_t first_event)
{
    const int C = d.C, nc = y.span, N = y.N;
    const PairListsDev &PL = y.PL;
    LmRun r{d, {}, {}, {}, {}, w.lm.as<LmDev>(), PL.num_pairs > 0 && !sw.separate_post, C > 0 && !sw.separate_back,
        nc > 0 && N == 32, N / 32 <= 4, true, {evs, o.verbose != 0, first_event, {}}};
    double *S = w.chol.S.as<double>();
    PointPassArgs &pa = r.pa; PairPassArgs &qa = r.qa;
    pa.min_diag = o.min_lm_diagonal; pa.max_diag = o.max_lm_diagonal;
    pa.diag_p = w.diag_p.as<double>(); pa.vinv = w.vinv.as<double>(); pa.ge = w.ge.as<double>();
    pa.scale_p_out = w.scale_p.as<double>(); pa.partials = w.partA.as<double>(); pa.obsrec = w.obsrec.as<double>();
    qa.min_diag = o.min_lm_diagonal; qa.max_diag = o.max_lm_diagonal;
    qa.num_pairs = PL.num_pairs; qa.dense = PL.dense ? 1 : 0;
    qa.pair_key = PL.unique.as<uint32_t>(); qa.pair_start = PL.starts.as<int32_t>(); qa.entries = PL.entries.as<uint64_t>();
    qa.chunk_start = PL.chunk_start.as<int32_t>(); qa.max_chunks = PL.max_chunks; qa.chunk = PL.chunk;
    qa.chunk_pair = PL.chunk_pair.as<int32_t>(); qa.chunk_desc = PL.chunk_desc.as<PairChunkDesc>();
    qa.pair_ticket = PL.pair_ticket.as<int32_t>(); qa.chunk_partials = PL.chunk_partials.as<double>();
    qa.gmax_out = w.gmax_cam; qa.vinv = w.vinv.as<double>(); qa.ge = w.ge.as<double>(); qa.obsrec = w.obsrec.as<double>();
    qa.diag_c = w.diag_c.as<double>(); qa.scale_c_out = w.scale_c.as<double>();
    qa.S = S; qa.ldS = N; qa.rhs = S + (size_t)N * N;
    r.prm = {o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.min_relative_decrease, o.max_trust_region_radius,
             o.min_trust_region_radius, o.max_num_iterations, o.max_consecutive_invalid_steps};
    r.sc = {w.partA.as<double>(), w.partB.as<double>(), w.partC.as<double>(), w.part_cam, w.gmax_cam, w.info, y.win.num,
            std::max(C, 1), r.small ? S : nullptr, nc, N};     // (reset_S: a one-block system is cleared by the decide kernel)
    return r;
}

int linearize(LmRun &r, const SystemLayout &y, const Workspace &w, bool reset, int post, LmDev *host_out, hipStream_t s)
{
    const CholeskyBuffers &ch = w.chol;
    r.pa.mode = kPassNormal; r.qa.mode = kPassNormal;
    OSFM_RETURN_IF(r.timer.tic(0, s));
    launch_point_pass(r.d, r.pa, y.win, s);
    OSFM_RETURN_IF(r.timer.toc(s));
    if (reset) {
        launch_reset_system(ch.S.as<double>(), ch.s_elems, ch.N, y.span, ch.N, s);
        if (y.ord.active) launch_padding_diagonal(ch.S.as<double>(), ch.N, y.ord_pad.as<int32_t>(), (int)y.ord.pad.size(), s);
    }
    if (y.PL.dense) {
        launch_schur_dense(r.d, w.obsrec.as<double>(), y.win.obs_lay, w.dense_z.as<double>(), w.dense_w.as<double>(),
            w.dense_partial.as<double>(), ch.S.as<double>(), ch.N, r.dense_first, s);
        r.dense_first = false;
    }
    memset(&r.qa.post, 0, sizeof(r.qa.post));
    if (post != kPostNone && r.post_fused) {
        r.qa.post.lm = r.lm; r.qa.post.prm = r.prm; r.qa.post.sc = r.sc; r.qa.post.host_out = host_out;
        r.qa.post.ticket = w.tickets + lm_ticket_bytes() / 4; r.qa.post.initial = post == kPostInitial; r.qa.post.enabled = 1;
    }
    OSFM_RETURN_IF(r.timer.tic(1, s));
    launch_pair_pass(r.d, r.qa, s);
    OSFM_RETURN_IF(r.timer.toc(s));
    if (post != kPostNone && !r.post_fused) launch_lm_post(r.lm, r.prm, r.sc, post == kPostInitial, host_out, s);
    return OSFM_OK;
}

// One iteration's Cholesky (one-launch form while one_launch), candidate and decision (state into host_out, may be null).
// *consumed: the launch-per-column form ran in place, so the system is cleared before it is accumulated again
int lm_step(LmRun &r, const SystemLayout &y, Workspace &w, bool one_launch, LmDev *host_out, hipStream_t s, bool *consumed)
{
    const int nc = y.span;
    double *y_c = w.chol.y.as<double>();
    OSFM_RETURN_IF(r.timer.tic(2, s));
    *consumed = false;
    if (r.small) launch_small_solve(w.chol.S.as<double>(), nc, w.chol.Ldiag.as<double>(), y_c, w.info, r.d, w.part_cam, s);
    else if (nc > 0) *consumed = w.chol.solve(nc, w.info, r.lm, one_launch, y.pattern, s) == 0;
    OSFM_RETURN_IF(r.timer.toc(s));
    OSFM_RETURN_IF(r.timer.tic(3, s));
    BackPassArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.y_c = y_c; ba.vinv = w.vinv.as<double>(); ba.ge = w.ge.as<double>(); ba.obsrec = w.obsrec.as<double>(); ba.partials = w.partB.as<double>();
    if (r.back_fused) {
        ba.fused = 1; ba.cost_partials = w.partC.as<double>();
        ba.decide.lm = r.lm; ba.decide.prm = r.prm; ba.decide.sc = r.sc; ba.decide.host_out = host_out;
        ba.decide.ticket = w.tickets; ba.decide.enabled = 1;
    }
    if (!r.small) launch_cam_update(r.d, y_c, nullptr, nullptr, w.part_cam, s);
    launch_back_pass(r.d, ba, y.win, s);
    OSFM_RETURN_IF(r.timer.toc(s));
    if (!r.back_fused) {
        launch_cost_pass(r.d, nullptr, nullptr, w.partC.as<double>(), y.win, s);
        // the kernels write the state they leave straight into the host's slot
        launch_lm_decide(r.lm, r.prm, r.sc, host_out, s);
    }
    return OSFM_OK;
}

// test hook (osfm_ba_debug_linearization): the first iteration in the cameras' own order; *pos: unknown_positions
int capture_linearization(const LmRun &r, const SystemLayout &y, const Workspace &w, hipStream_t s, osfm_ba_lin_capture *cap,
    std::vector<int32_t> *pos)
{
    const BaDev &d = r.d;
    const PairListsDev &PL = y.PL;
    const int C = d.C, M = d.M, nc = y.span, N = y.N, num_pairs = PL.num_pairs;
    const size_t s_elems = w.chol.s_elems;
    std::vector<int32_t> ldim((size_t)C);
    std::vector<double> hS(s_elems), hdiag((size_t)nc), hscale((size_t)nc);
    std::vector<PairChunkDesc> desc((size_t)std::max(PL.max_chunks, 1));
    LmDev st;
    if (C) OSFM_HIP_CHECK(hipMemcpyAsync(ldim.data(), d.cam_ldim, (size_t)C * 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(hS.data(), w.chol.S.ptr, s_elems * 8, hipMemcpyDeviceToHost, s));
    if (nc) {
        OSFM_HIP_CHECK(hipMemcpyAsync(hdiag.data(), w.diag_c.ptr, (size_t)nc * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(hscale.data(), w.scale_c.ptr, (size_t)nc * 8, hipMemcpyDeviceToHost, s));
    }
    if (M) {
        OSFM_HIP_CHECK(hipMemcpyAsync(cap->scale_p, w.scale_p.ptr, (size_t)3 * M * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(cap->diag_p, w.diag_p.ptr, (size_t)3 * M * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(cap->vinv, w.vinv.ptr, (size_t)9 * M * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(cap->ge, w.ge.ptr, (size_t)3 * M * 8, hipMemcpyDeviceToHost, s));
    }
    if (num_pairs > 0 && PL.max_chunks > 0)
        OSFM_HIP_CHECK(hipMemcpyAsync(desc.data(), PL.chunk_desc.ptr, (size_t)PL.max_chunks * sizeof(PairChunkDesc), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(&st, r.lm, sizeof(LmDev), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    *pos = unknown_positions(C, ldim.data(), y.ord);
    const size_t n = pos->size();
    std::vector<char> taken((size_t)N, 0);
    for (size_t u = 0; u < n; ++u) {
        const size_t pu = (size_t)(*pos)[u];
        taken[pu] = 1;
        for (size_t v = 0; v < n; ++v) {
            const size_t pv = (size_t)(*pos)[v];
            cap->S[u * n + v] = v > u ? 0.0 : hS[std::max(pu, pv) * N + std::min(pu, pv)];
        }
        cap->rhs[u] = hS[(size_t)N * N + pu];
        cap->diag_c[u] = hdiag[pu];
        cap->scale_c[u] = hscale[pu];
    }
    cap->num_pad = 0; cap->pad_diag_min = INFINITY; cap->pad_diag_max = -INFINITY; cap->pad_off_max = 0.0;
    for (size_t q = 0; q < (size_t)N; ++q) {
        if (taken[q]) continue;
        cap->num_pad++;
        cap->pad_diag_min = std::min(cap->pad_diag_min, hS[q * N + q]);
        cap->pad_diag_max = std::max(cap->pad_diag_max, hS[q * N + q]);
        double off = std::fabs(hS[(size_t)N * N + q]);
        for (size_t p = 0; p < (size_t)N; ++p)
            if (p != q) off = std::max(off, std::fabs(p < q ? hS[q * N + p] : hS[p * N + q]));
        cap->pad_off_max = std::max(cap->pad_off_max, off);
    }
    cap->initial_cost = st.initial_cost; cap->grad_max = st.grad_max; cap->radius = st.radius; cap->stopped = st.stop;
    cap->win_num = y.win.num; cap->win_over = y.win.num_over;
    cap->small_lists = PL.small; cap->dense = PL.dense;
    cap->dense_splits = PL.dense ? schur_dense_splits(nc, M) : 0;
    cap->num_pairs = num_pairs; cap->pair_chunk = PL.chunk; cap->max_chunks = PL.max_chunks;
    std::vector<char> multi((size_t)std::max(num_pairs, 1), 0);     // pairs of more than one chunk
    cap->multi_chunk_pairs = 0;
    if (num_pairs > 0)
        for (int i = 0; i < PL.max_chunks; ++i)
            if (desc[i].nchunks > 1 && desc[i].pi >= 0 && desc[i].pi < num_pairs && !multi[desc[i].pi]) { multi[desc[i].pi] = 1; cap->multi_chunk_pairs++; }
    cap->order_arcs = y.ord.active ? y.ord.arcs : 0;
    cap->span = nc; cap->N = N; cap->small_solve = r.small; cap->post_fused = r.post_fused; cap->back_fused = r.back_fused;
    return OSFM_OK;
}

// behind the first iteration's decision, before the linearisation that follows it overwrites anything
int capture_step(const LmRun &r, const SystemLayout &y, const Workspace &w, const std::vector<int32_t> &pos, bool one_launch,
    hipStream_t s, osfm_ba_lin_capture *cap)
{
    const int C = r.d.C, M = r.d.M, nc = y.span;
    std::vector<double> hy((size_t)std::max(nc, 1));
    LmDev st;
    if (nc) OSFM_HIP_CHECK(hipMemcpyAsync(hy.data(), w.chol.y.ptr, (size_t)nc * 8, hipMemcpyDeviceToHost, s));
    // (the first candidate goes to the iterate buffers 1 whatever the decision: buffers 0 are current)
    if (C) OSFM_HIP_CHECK(hipMemcpyAsync(cap->cand_cams, r.d.cams2[1], (size_t)7 * C * 8, hipMemcpyDeviceToHost, s));
    if (M) OSFM_HIP_CHECK(hipMemcpyAsync(cap->cand_points, r.d.points2[1], (size_t)4 * M * 8, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(&st, r.lm, sizeof(LmDev), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t u = 0; u < pos.size(); ++u) cap->y_c[u] = hy[pos[u]];
    cap->model_cost_change = st.model_cost_change; cap->cand_cost = st.cand_cost;
    cap->relative_decrease = (st.x_cost - (std::isfinite(st.cand_cost) ? st.cand_cost : std::numeric_limits<double>::max())) / st.model_cost_change;
    cap->accepted = st.cur == 1; cap->flow_aborted = st.flow_aborted; cap->one_launch = one_launch;
    return OSFM_OK;
}

// ---- Levenberg-Marquardt, control on the device: every iteration is the same fixed sequence of launches, what they do is
// read from the LmDev state that ba_lm_decide / ba_lm_post keep.  Small systems are bound by launch latency: the host
// (eager) enqueues iteration i + 1 before it looks at the state iteration i left, and pays one row of do-nothing kernels
// at the end.  Large ones are bound by the device: the host waits for the decision of iteration i (the linearisation of i
// is queued behind it) and never enqueues a Cholesky that will not happen.  h_state[slot]: the state iteration slot - 1
// leaves, evs[slot] behind it.  Returns the final state in *fin.
int run_loop(LmRun &r, const SystemLayout &y, Workspace &w, int max_slots, LmDev *h_state, hipStream_t s, osfm_ba_summary *sum,
    osfm_ba_lin_capture *cap, const std::vector<int32_t> &cap_pos, LmDev *fin)
{
    std::vector<hipEvent_t> &evs = r.timer.evs;
    bool one_launch = w.chol.flow;       // the one-launch Cholesky, until a launch of it had to be given up
    int restarts = 0;
    for (int it = 0; it < max_slots - 2; ++it) {
        const int slot = it + 1;
        bool consumed = false;
        OSFM_RETURN_IF(lm_step(r, y, w, one_launch, r.eager ? nullptr : &h_state[slot], s, &consumed));
        if (cap && it == 0 && !cap->stopped) OSFM_RETURN_IF(capture_step(r, y, w, cap_pos, !r.small && y.span > 0 && !consumed, s, cap));
        if (!r.eager) OSFM_HIP_CHECK(hipEventRecord(evs[slot], s));
        OSFM_RETURN_IF(linearize(r, y, w, consumed, kPostLoop, r.eager ? &h_state[slot] : nullptr, s));
        OSFM_HIP_CHECK(hipGetLastError());
        int seen = -1;                    // the slot whose state the host has read in this round
        if (r.eager) {
            OSFM_HIP_CHECK(hipEventRecord(evs[slot], s));
            if (it >= 1) {
                // what iteration it - 1 left behind (this iteration is already queued after it)
                OSFM_HIP_CHECK(hipEventSynchronize(evs[slot - 1]));
                seen = slot - 1;
            }
        } else {
            OSFM_HIP_CHECK(hipEventSynchronize(evs[slot]));
            seen = slot;
        }
        if (seen >= 0 && h_state[seen].flow_aborted) {
            // The one-launch factorisation of iteration seen - 1 gave up (its workgroups were not all resident) and nothing
            // was decided from it: the system is linearised again at the same iterate and diagonal (no second finalisation:
            // that is the iteration's, still to come), and the iteration repeats in the launch-per-column form, as the rest.
            if (!one_launch || ++restarts > 1) { set_error("ba_solve: the Cholesky launch was given up twice (device busy?)"); return OSFM_E_DEVICE; }
            one_launch = false;
            sum->flow_fallbacks++;
            OSFM_HIP_CHECK(hipStreamSynchronize(s));
            launch_lm_clear_abort(r.lm, s);
            OSFM_RETURN_IF(linearize(r, y, w, !r.small, kPostNone, nullptr, s));
            it = seen - 2;                // the loop's increment makes it seen - 1: that iteration again
            continue;
        }
        if (seen >= 0 && h_state[seen].stop) break;
    }
    OSFM_HIP_CHECK(hipMemcpyAsync(&h_state[max_slots - 1], r.lm, sizeof(LmDev), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    *fin = h_state[max_slots - 1];
    if (fin->nonfinite) { set_error("ba_solve: non-finite initial cost"); return OSFM_E_NUMERIC; }
    return OSFM_OK;
}

int fill_summary(const LmDev &fin, const KernelTimer &t, Clock::time_point t_loop, osfm_ba_summary *sum)
{
    double ms_of[4] = {0, 0, 0, 0};       // point pass, pair pass, Cholesky, back pass
    for (auto &pr : t.pairs) {
        float ms = 0.f;
        if (pr.first >= t.next) continue;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, t.evs[pr.first], t.evs[pr.first + 1]));
        ms_of[pr.second] += ms;
    }
    sum->lm_loop_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_loop).count();
    sum->initial_cost = fin.initial_cost; sum->final_cost = fin.x_cost;
    sum->num_successful_steps = fin.num_success; sum->num_unsuccessful_steps = fin.num_unsuccess;
    sum->num_iterations = fin.iteration; sum->termination = fin.term;
    sum->point_pass_ms = ms_of[0]; sum->pair_pass_ms = ms_of[1]; sum->cholesky_ms = ms_of[2]; sum->back_pass_ms = ms_of[3];
    sum->linearizations = fin.num_success + fin.num_unsuccess + 1;   // the speculative ones past the end do nothing
    return OSFM_OK;
}

// The one-workgroup form (ba_small.hip): no observation windows, pair lists, elimination order or Cholesky buffers --
// the per-observation records and per-point blocks, one launch, one read of the state it leaves.  The summary's
// per-kernel-family times and list / order fields stay 0; lm_loop_ms is the device's own time between the first
// linearisation and the end of the launch.
int small_solve(const DeviceProblem &D, const osfm_ba_options &o, StreamLease &sg, osfm_ba_summary *sum, int *cur_out)
{
    const auto t_begin = Clock::now();
    hipStream_t s = sg.s;
    BaDev d = D.dev;
    const size_t M = (size_t)d.M, O = (size_t)d.O;
    if (d.nc > 6 * kSmallMaxCams) { set_error("ba_solve: %d camera unknowns in the one-workgroup form", d.nc); return OSFM_E_ARG; }
    DevArray obsrec, diag_p, vinv, ge, scale_p, state;
    OSFM_RETURN_IF(obsrec.alloc(O * kObsRec * 8));
    OSFM_RETURN_IF(diag_p.alloc(3 * M * 8));
    OSFM_RETURN_IF(vinv.alloc(9 * M * 8));
    OSFM_RETURN_IF(ge.alloc(3 * M * 8));
    OSFM_RETURN_IF(scale_p.alloc(3 * M * 8));
    constexpr size_t kStampsAt = (sizeof(LmDev) + 15) / 16 * 16, kStateBytes = kStampsAt + 3 * sizeof(long long);
    OSFM_RETURN_IF(state.alloc(kStateBytes));
    OSFM_RETURN_IF(sg.set->ensure_pinned(kStateBytes));
    d.cams2[0] = D.cams[0].as<double>(); d.cams2[1] = D.cams[1].as<double>();
    d.points2[0] = D.points[0].as<double>(); d.points2[1] = D.points[1].as<double>();
    SmallBaArgs a;
    memset(&a, 0, sizeof(a));
    a.prm = {o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.min_relative_decrease, o.max_trust_region_radius,
             o.min_trust_region_radius, o.max_num_iterations, o.max_consecutive_invalid_steps};
    a.radius0 = o.initial_trust_region_radius; a.min_diag = o.min_lm_diagonal; a.max_diag = o.max_lm_diagonal;
    a.jacobi_scaling = o.jacobi_scaling ? 1 : 0;
    a.obsrec = obsrec.as<double>(); a.diag_p = diag_p.as<double>(); a.vinv = vinv.as<double>(); a.ge = ge.as<double>();
    a.scale_p = scale_p.as<double>();
    a.lm = state.as<LmDev>(); a.stamps = reinterpret_cast<long long *>(state.as<char>() + kStampsAt);
    launch_small_ba(d, a, s);
    OSFM_HIP_CHECK(hipGetLastError());
    char *h = static_cast<char *>(sg.set->pinned);
    OSFM_HIP_CHECK(hipMemcpyAsync(h, state.ptr, kStateBytes, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    LmDev fin;
    long long stamps[3];
    memcpy(&fin, h, sizeof(fin));
    memcpy(stamps, h + kStampsAt, sizeof(stamps));
    if (fin.nonfinite) { set_error("ba_solve: non-finite initial cost"); return OSFM_E_NUMERIC; }
    sum->lm_loop_ms = (double)(stamps[2] - stamps[1]) * 1e-5;       // 100 MHz
    sum->initial_cost = fin.initial_cost; sum->final_cost = fin.x_cost;
    sum->num_successful_steps = fin.num_success; sum->num_unsuccessful_steps = fin.num_unsuccess;
    sum->num_iterations = fin.iteration; sum->termination = fin.term;
    sum->linearizations = fin.num_success + fin.num_unsuccess + 1;
    lap(o.verbose, t_begin, "  one-workgroup solve");
    *cur_out = fin.cur;
    return OSFM_OK;
}

}  // namespace

int check_small_form(const osfm_ba_options &o, int num_cameras, bool capture, const char *what)
{
    if (o.small_form < 0 || o.small_form > 2) { set_error("%s: small_form %d (0: general form, 1: by size, 2: one-workgroup form)", what, o.small_form); return OSFM_E_ARG; }
    if (o.small_form != 2) return OSFM_OK;
    if (capture) { set_error("%s: the capture is of the general form, small_form is 2", what); return OSFM_E_ARG; }
    if (num_cameras > kSmallMaxCams) {
        set_error("%s: small_form 2 with %d cameras: the one-workgroup form takes at most %d", what, num_cameras, kSmallMaxCams);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

int ba_linearize_plain(const DeviceProblem &D, StreamLease &sg, int64_t pair_bound,
    const std::function<int(const PlainLin &)> &after_points, const std::function<int(const PlainLin &)> &after_system)
{
    Switches sw{};
    sw.order = 0; sw.steps = true;       // the cameras' own order; no hand-off flags (the launch-per-column Cholesky)
    hipStream_t s = sg.s;
    BaDev d = D.dev;                     // (lm stays null: the kernels read the plain pointers and these arguments)
    OSFM_RETURN_IF(sg.set->ensure_pinned(sizeof(LmDev)));
    osfm_ba_summary sum;
    memset(&sum, 0, sizeof(sum));
    SystemLayout y;
    OSFM_RETURN_IF(lay_out_system(d, sw, pair_bound, static_cast<int32_t *>(sg.set->pinned), s, y, &sum));
    Workspace w;
    OSFM_RETURN_IF(allocate_workspace(d, y, sw, s, w));
    osfm_ba_options o;
    osfm_ba_options_default(&o);
    LmRun r = make_run(d, o, sw, y, w, sg.set->events, 0);
    const double inf = std::numeric_limits<double>::infinity();
    r.pa.mode = kPassNormal; r.pa.update_diag = 1; r.pa.want_gradient = 0; r.pa.radius = inf;
    r.qa.mode = kPassNormal; r.qa.update_diag = 1; r.qa.want_gradient = 0; r.qa.radius = inf;
    launch_point_pass(r.d, r.pa, y.win, s);
    OSFM_HIP_CHECK(hipGetLastError());
    const PlainLin lin{w.obsrec.as<double>(), w.vinv.as<double>(), y.win.obs_lay, w.partA.as<double>(), y.win.num, &w.chol, y.PL.dense};
    const int rc = after_points(lin);
    if (rc != 0) return rc;
    launch_reset_system(w.chol.S.as<double>(), w.chol.s_elems, w.chol.N, y.span, w.chol.N, s);
    if (y.PL.dense)
        launch_schur_dense(r.d, w.obsrec.as<double>(), y.win.obs_lay, w.dense_z.as<double>(), w.dense_w.as<double>(),
            w.dense_partial.as<double>(), w.chol.S.as<double>(), w.chol.N, true, s);
    memset(&r.qa.post, 0, sizeof(r.qa.post));
    launch_pair_pass(r.d, r.qa, s);
    OSFM_HIP_CHECK(hipGetLastError());
    return after_system(lin);
}

int ba_solve_core(const DeviceProblem &D, const osfm_ba_options &o, StreamLease &sg, int64_t pair_bound, osfm_ba_summary *sum,
    int *cur_out, osfm_ba_lin_capture *cap)
{
    OSFM_RETURN_IF(check_small_form(o, D.dev.C, cap != nullptr, "ba_solve"));
    if (!cap && (o.small_form == 2 || (o.small_form == 1 && D.dev.C <= kSmallMaxCams && D.dev.O <= kSmallAutoMaxObs)))
        return small_solve(D, o, sg, sum, cur_out);
    const auto t_begin = Clock::now();
    const Switches sw{};
    hipStream_t s = sg.s;
    BaDev d = D.dev;
    const int max_slots = o.max_num_iterations + 3;
    OSFM_RETURN_IF(sg.set->ensure_pinned((size_t)max_slots * sizeof(LmDev)));
    LmDev *h_state = static_cast<LmDev *>(sg.set->pinned);
    SystemLayout y;
    OSFM_RETURN_IF(lay_out_system(d, sw, pair_bound, reinterpret_cast<int32_t *>(&h_state[max_slots - 1]), s, y, sum));
    lap(o.verbose, t_begin, "  pair lists (device)");
    Workspace w;
    OSFM_RETURN_IF(allocate_workspace(d, y, sw, s, w));
    OSFM_RETURN_IF(w.lm.alloc(sizeof(LmDev)));
    // verbose: 8 timing events per iteration slot, three slots of slack for a given-up Cholesky launch's repeat (20 events)
    OSFM_RETURN_IF(sg.set->ensure_events((size_t)max_slots + (o.verbose ? 8 * ((size_t)max_slots + 3) : 0)));
    LmDev &init = h_state[0];
    memset(&init, 0, sizeof(init));
    init.radius = o.initial_trust_region_radius; init.decrease_factor = 2.0;
    init.update_diag = 1; init.want_gradient = 1; init.term = OSFM_BA_NO_CONVERGENCE;
    OSFM_HIP_CHECK(hipMemcpyAsync(w.lm.ptr, &init, sizeof(LmDev), hipMemcpyHostToDevice, s));
    d.cams2[0] = D.cams[0].as<double>(); d.cams2[1] = D.cams[1].as<double>();
    d.points2[0] = D.points[0].as<double>(); d.points2[1] = D.points[1].as<double>();
    LmRun r = make_run(d, o, sw, y, w, sg.set->events, (size_t)max_slots);
    // iteration 0: the Jacobi scaling from the unscaled column norms, on the plain pointers; the state comes after it
    if (o.jacobi_scaling) {
        r.pa.mode = kPassScaleInit; r.qa.mode = kPassScaleInit;
        r.pa.radius = r.qa.radius = o.initial_trust_region_radius;
        launch_point_pass(r.d, r.pa, y.win, s);
        launch_pair_pass(r.d, r.qa, s);
        OSFM_HIP_CHECK(hipGetLastError());
    }
    r.d.lm = r.lm;
    lap(o.verbose, t_begin, "  alloc + lists up");
    OSFM_RETURN_IF(linearize(r, y, w, true, kPostInitial, nullptr, s));
    OSFM_HIP_CHECK(hipGetLastError());
    lap(o.verbose, t_begin, "  first linearize");
    std::vector<int32_t> cap_pos;
    if (cap) OSFM_RETURN_IF(capture_linearization(r, y, w, s, cap, &cap_pos));
    const auto t_loop = Clock::now();
    LmDev fin;
    OSFM_RETURN_IF(run_loop(r, y, w, max_slots, h_state, s, sum, cap, cap_pos, &fin));
    OSFM_RETURN_IF(fill_summary(fin, r.timer, t_loop, sum));
    lap(o.verbose, t_begin, "  LM loop");
    *cur_out = fin.cur;
    return OSFM_OK;
}

}  // namespace osfm
