// osfm_match_guided: validation, the per-pair job records, the four launches of guided_kernels.hip and the lists'
// way back.  Scratch is the matcher's, grow-only like its other work arrays (booked through DeviceBuffer).
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "match_internal.h"
#include "guided_kernels.h"

using namespace osfm;

namespace {

// OSFM_GUIDED_TRACE: the time since the call began, at its steps (tools/guided_timing.py reads the split off it)
struct GuidedLap {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what) const
    {
        static const bool trace = getenv("OSFM_GUIDED_TRACE") != nullptr;
        if (trace) fprintf(stderr, "[osfm guided] %-22s %9.3f ms\n", what,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

}  // namespace

extern "C" {

int osfm_guided_options_default(osfm_guided_options *o)
{
    if (!o) { set_error("guided_options_default: null argument"); return OSFM_E_ARG; }
    memset(o, 0, sizeof(*o));
    o->threshold = 0.0015;
    o->sift_lowe_ratio = 0.8f;
    o->surf_lowe_ratio = 0.7f;
    o->cap_from_seeds = 1;
    return OSFM_OK;
}

int osfm_guided_limits(int32_t *queries_per_workgroup, int32_t *positions_per_chunk, int32_t *candidates_per_pass)
{
    if (queries_per_workgroup) *queries_per_workgroup = kGuidedQueries;
    if (positions_per_chunk) *positions_per_chunk = kGuidedChunk;
    if (candidates_per_pass) *candidates_per_pass = kGuidedPass;
    return OSFM_OK;
}

int osfm_match_guided(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, const int64_t *seed_offsets,
    const int32_t *seed_corr, const double *F, const osfm_guided_options *opts, osfm_guided_result *results,
    int32_t *corr, int64_t capacity, int64_t *total, double *F_out)
{
    if (!m || num_pairs < 0 || (num_pairs > 0 && (!pairs || !results || !seed_offsets)) || capacity < 0 || (capacity > 0 && !corr)) {
        set_error("match_guided: bad arguments");
        return OSFM_E_ARG;
    }
    if (!m->shards.empty())
        return osfm_match_guided(m->shards[0], pairs, num_pairs, seed_offsets, seed_corr, F, opts, results, corr, capacity, total, F_out);
    osfm_guided_options o;
    osfm_guided_options_default(&o);
    if (opts) o = *opts;
    if (!(o.threshold > 0.0)) { set_error("match_guided: threshold %g is not > 0", o.threshold); return OSFM_E_ARG; }
    if (num_pairs == 0) { if (total) *total = 0; return OSFM_OK; }

    std::lock_guard<std::mutex> lock(m->mu);
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const GuidedLap lap{};

    // ---- validation: nothing is written before all of it has passed ----
    if (seed_offsets[0] < 0) { set_error("match_guided: seed_offsets[0] = %lld", (long long)seed_offsets[0]); return OSFM_E_ARG; }
    for (int p = 0; p < num_pairs; ++p)
        if (seed_offsets[p + 1] < seed_offsets[p]) { set_error("match_guided: seed offsets decrease at pair %d", p); return OSFM_E_ARG; }
    if (seed_offsets[num_pairs] > seed_offsets[0] && !seed_corr) { set_error("match_guided: seeds without seed_corr"); return OSFM_E_ARG; }
    std::vector<int32_t> stamp1, stamp2;
    int64_t u_total = 0, list_total = 0;
    for (int p = 0; p < num_pairs; ++p) {
        if (check_view(m, pairs[p].view_1, "match_guided") != OSFM_OK || check_view(m, pairs[p].view_2, "match_guided") != OSFM_OK)
            return OSFM_E_ARG;        // (a view that was never set is an argument error here, as one without positions)
        const ViewData &a = m->views[pairs[p].view_1], &b = m->views[pairs[p].view_2];
        const int n1 = a.ns + a.nu, n2 = b.ns + b.nu;
        if (a.n_positions != n1 || b.n_positions != n2) {
            set_error("match_guided: views %d and %d need osfm_match_set_positions", pairs[p].view_1, pairs[p].view_2);
            return OSFM_E_ARG;
        }
        if (seed_offsets[p + 1] - seed_offsets[p] > std::min(n1, n2)) {
            set_error("match_guided: pair %d has more seeds than features", p);
            return OSFM_E_ARG;
        }
        if ((int)stamp1.size() < n1) stamp1.resize(n1, -1);
        if ((int)stamp2.size() < n2) stamp2.resize(n2, -1);
        for (int64_t t = seed_offsets[p]; t < seed_offsets[p + 1]; ++t) {
            const int f1 = seed_corr[2 * t], f2 = seed_corr[2 * t + 1];
            if (f1 < 0 || f1 >= n1 || f2 < 0 || f2 >= n2) {
                set_error("match_guided: pair %d, seed (%d, %d) outside its views (%d, %d features)", p, f1, f2, n1, n2);
                return OSFM_E_ARG;
            }
            if (stamp1[f1] == p || stamp2[f2] == p) {
                set_error("match_guided: pair %d names a feature of seed (%d, %d) twice", p, f1, f2);
                return OSFM_E_ARG;
            }
            if ((f1 < a.ns) != (f2 < b.ns)) {
                set_error("match_guided: pair %d, seed (%d, %d) joins a SIFT row to a SURF row", p, f1, f2);
                return OSFM_E_ARG;
            }
            stamp1[f1] = p; stamp2[f2] = p;
        }
        u_total += n1 + n2;
        list_total += std::min(n1, n2);
    }

    lap("validated");

    // ---- job records ----
    const int64_t seed0 = seed_offsets[0], num_seeds = seed_offsets[num_pairs] - seed0;
    OSFM_RETURN_IF(m->g_jobs.reserve((size_t)num_pairs * sizeof(GuidedJob)));
    OSFM_RETURN_IF(m->g_prep.reserve((size_t)num_pairs * sizeof(GuidedPrep)));
    OSFM_RETURN_IF(m->g_seeds.reserve((size_t)std::max<int64_t>(num_seeds, 1) * 8));
    OSFM_RETURN_IF(m->g_u.reserve((size_t)std::max<int64_t>(u_total, 1) * 8));
    OSFM_RETURN_IF(m->g_m.reserve((size_t)std::max<int64_t>(u_total, 1) * 4));
    OSFM_RETURN_IF(m->g_list.reserve((size_t)std::max<int64_t>(list_total, 1) * 8));
    OSFM_RETURN_IF(m->g_off.reserve((size_t)num_pairs * 8));
    std::vector<GuidedJob> jobs((size_t)num_pairs);
    std::vector<char> seen(m->views.size(), 0);
    int64_t u_at = 0, list_at = 0, blocks = 0;
    auto cdiv = [](int n) { return (int64_t)((n + kGuidedQueries - 1) / kGuidedQueries); };
    for (int p = 0; p < num_pairs; ++p) {
        const int v1 = pairs[p].view_1, v2 = pairs[p].view_2;
        const ViewData &a = m->views[v1], &b = m->views[v2];
        for (int v : {v1, v2})
            if (!seen[v]) { seen[v] = 1; if (m->views[v].ready) OSFM_HIP_CHECK(hipStreamWaitEvent(s, m->views[v].ready, 0)); }
        const int n1 = a.ns + a.nu, n2 = b.ns + b.nu;
        GuidedJob &j = jobs[p];
        memset(&j, 0, sizeof(j));
        j.pos1 = a.positions.as<float>(); j.pos2 = b.positions.as<float>();
        j.sift1 = a.sift.as<int8_t>(); j.sift2 = b.sift.as<int8_t>();
        j.surf1 = a.surf.as<int8_t>(); j.surf2 = b.surf.as<int8_t>();
        j.seeds = m->g_seeds.as<int32_t>() + 2 * (seed_offsets[p] - seed0);
        j.u1 = m->g_u.as<double>() + u_at; j.u2 = j.u1 + n1;
        j.m12 = m->g_m.as<int32_t>() + u_at; j.m21 = j.m12 + n1;
        j.list = m->g_list.as<int32_t>() + 2 * list_at;
        j.ns1 = a.ns; j.nu1 = a.nu; j.ns2 = b.ns; j.nu2 = b.nu;
        j.num_seeds = (int32_t)(seed_offsets[p + 1] - seed_offsets[p]);
        j.has_F = F ? 1 : 0;
        if (F) { const double *f = F + (size_t)p * 9; j.F[0] = f[2]; j.F[1] = f[5]; j.F[2] = f[6]; j.F[3] = f[7]; j.F[4] = f[8]; }
        j.block_start = (int32_t)blocks;
        blocks += cdiv(a.ns) + cdiv(a.nu) + cdiv(b.ns) + cdiv(b.nu);
        if (blocks > 0x7fffffff) { set_error("match_guided: too many queries for one call; split the pairs"); return OSFM_E_ARG; }
        j.block_end = (int32_t)blocks;
        u_at += n1 + n2; list_at += std::min(n1, n2);
    }
    OSFM_HIP_CHECK(hipMemcpyAsync(m->g_jobs.ptr, jobs.data(), jobs.size() * sizeof(GuidedJob), hipMemcpyHostToDevice, s));
    if (num_seeds > 0)
        OSFM_HIP_CHECK(hipMemcpyAsync(m->g_seeds.ptr, seed_corr + 2 * seed0, (size_t)num_seeds * 8, hipMemcpyHostToDevice, s));

    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    lap("jobs and seeds up");

    // ---- the pairs on the device ----
    const GuidedJob *d_jobs = m->g_jobs.as<GuidedJob>();
    GuidedPrep *d_prep = m->g_prep.as<GuidedPrep>();
    launch_guided_prepare(d_jobs, num_pairs, d_prep, o.threshold, o.cap_from_seeds, s);
    launch_guided_match(d_jobs, num_pairs, (int)blocks, d_prep, o.sift_lowe_ratio * o.sift_lowe_ratio,
        o.surf_lowe_ratio * o.surf_lowe_ratio, s);
    launch_guided_finish(d_jobs, num_pairs, d_prep, s);
    OSFM_HIP_CHECK(hipGetLastError());
    std::vector<GuidedPrep> prep((size_t)num_pairs);
    OSFM_HIP_CHECK(hipMemcpyAsync(prep.data(), d_prep, prep.size() * sizeof(GuidedPrep), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    lap("kernels done");

    // ---- records, then the lists back to back ----
    std::vector<int64_t> dst((size_t)num_pairs);
    int64_t written = 0;
    for (int p = 0; p < num_pairs; ++p) {
        osfm_guided_result &r = results[p];
        r.status = prep[p].status;
        r.num_seeds = jobs[p].num_seeds;
        r.num_added = prep[p].count - jobs[p].num_seeds;
        r.max_candidates = prep[p].max_candidates;
        r.offset = written;
        dst[p] = written;
        written += prep[p].count;
        if (F_out) {
            double *f = F_out + (size_t)p * 9;
            for (int i = 0; i < 9; ++i) f[i] = 0.0;
            f[2] = prep[p].v[0]; f[5] = prep[p].v[1]; f[6] = prep[p].v[2]; f[7] = prep[p].v[3]; f[8] = prep[p].v[4];
        }
    }
    if (total) *total = written;
    if (written > capacity) {
        set_error("match_guided: %lld correspondences need more than the given capacity %lld", (long long)written, (long long)capacity);
        return OSFM_E_CAPACITY;
    }
    if (written > 0) {
        OSFM_RETURN_IF(m->g_out.reserve((size_t)written * 8));
        OSFM_HIP_CHECK(hipMemcpyAsync(m->g_off.ptr, dst.data(), dst.size() * 8, hipMemcpyHostToDevice, s));
        launch_guided_gather(d_jobs, num_pairs, d_prep, m->g_off.as<int64_t>(), m->g_out.as<int32_t>(), s);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipMemcpyAsync(corr, m->g_out.ptr, (size_t)written * 8, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
    }
    lap("lists on the host");
    return OSFM_OK;
}

}  // extern "C"
