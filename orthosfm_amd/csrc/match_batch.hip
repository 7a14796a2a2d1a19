// One batch of pairs on the device: the plan of match_plan.hip reserved, launched and read back.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "match_internal.h"
#include "cashash_kernels.h"

namespace osfm {

int check_view(const osfm_matcher *m, int v, const char *what) { return check_view(m->views, v, what); }

void reset_stats(osfm_matcher *m) { memset(&m->stats, 0, sizeof(m->stats)); }

// Runs one batch of pairs through the device pipeline (BatchMode says which entry's semantics).
int run_batch(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, const BatchMode &mode,
    BatchResult *res)
{
    const bool cascade = cascade_batch(m->opts, mode);
    if (cascade) OSFM_RETURN_IF(ensure_cashash(m));
    static const int forced_seg_tiles = [] { const char *e = getenv("OSFM_SEG_TILES"); return e ? atoi(e) : 0; }();
    // OSFM_FINISH_RESCAN=wave: every refinement of the finish through its per-query rescan (read per batch)
    const char *rescan_env = getenv("OSFM_FINISH_RESCAN");
    PlanKnobs knobs;
    knobs.seg_tiles = forced_seg_tiles;
    knobs.rescan_wave = rescan_env && strcmp(rescan_env, "wave") == 0;
    BatchPlan &plan = m->plan;
    res->counts.assign(num_pairs, 0);
    OSFM_RETURN_IF(plan_batch(m->views, m->opts, m->special_max, knobs, pairs, num_pairs, mode, &plan));
    // the caller reads the pairs' places and lengths from the result
    res->plans = plan.plans;
    res->out_ints = plan.out_ints;
    const std::vector<PairPlan> &plans = plan.plans;
    std::vector<MatchProblem> *probs = plan.probs;
    const std::vector<SpecialJob> &spjobs = plan.spjobs, &spjobs_wide = plan.spjobs_wide;
    const int64_t out_ints = plan.out_ints, total_queries = plan.total_queries, rs_buckets = plan.rs_buckets;
    const int *total_blocks = plan.total_blocks, *max_n = plan.max_n;

    // --- scratch ---------------------------------------------------------
    // (a smaller call than the largest the caller has announced: the arrays in proportion, once -- the parts of a
    //  large call are bounded by batch_size_for, and so is the proportion)
    double grow = 1.0;
    if (mode.expect > num_pairs && num_pairs > 0) grow = 1.02 * (double)mode.expect / num_pairs;
    auto grown = [&](int64_t n) { return (size_t)((double)std::max<int64_t>(n, 1) * std::max(grow, 1.0)); };
    OSFM_RETURN_IF(m->out.reserve(grown(std::max<int64_t>(out_ints, 4)) * 4));
    OSFM_RETURN_IF(m->rowparts.reserve(grown(plan.rowpart_recs) * sizeof(RowPart)));
    OSFM_RETURN_IF(m->colparts.reserve(grown(plan.colpart_recs) * sizeof(ColPart)));
    OSFM_RETURN_IF(m->keep.reserve(grown(std::max<int64_t>(plan.keep_bytes, 16))));
    OSFM_RETURN_IF(m->exact_items.reserve(grown(total_queries) * sizeof(ExactItem)));
    OSFM_RETURN_IF(m->exact_count.reserve(16));
    if (plan.bucketed) {
        OSFM_RETURN_IF(m->rs_count.reserve(grown(rs_buckets) * sizeof(int32_t)));
        OSFM_RETURN_IF(m->rs_items.reserve(grown(plan.rs_items) * sizeof(RescoreItem)));
    }
    OSFM_RETURN_IF(m->sp_parts.reserve((size_t)std::max<int64_t>(plan.sp_recs, 1) * sizeof(RowPart)));
    hipStream_t s = m->stream;
    {
        // the views this batch names: their uploads (own stream) before anything of the batch
        std::vector<uint8_t> seen(m->views.size(), 0);
        for (int p = 0; p < num_pairs; ++p)
            for (int v : {plans[p].v1, plans[p].v2})
                if (!seen[v]) { seen[v] = 1; if (m->views[v].ready) OSFM_HIP_CHECK(hipStreamWaitEvent(s, m->views[v].ready, 0)); }
    }
    OSFM_RETURN_IF(m->sp_col.reserve((size_t)std::max<int64_t>(plan.sp_cols, 1) * 4));
    OSFM_RETURN_IF(m->d_spjobs.reserve(std::max<size_t>(spjobs.size() + spjobs_wide.size(), 1) * sizeof(SpecialJob)));
    if (!spjobs.empty())
        OSFM_HIP_CHECK(hipMemcpyAsync(m->d_spjobs.ptr, spjobs.data(), spjobs.size() * sizeof(SpecialJob),
            hipMemcpyHostToDevice, s));
    if (!spjobs_wide.empty())
        OSFM_HIP_CHECK(hipMemcpyAsync(m->d_spjobs.as<SpecialJob>() + spjobs.size(), spjobs_wide.data(),
            spjobs_wide.size() * sizeof(SpecialJob), hipMemcpyHostToDevice, s));
    int32_t *d_out = m->out.as<int32_t>();
    OSFM_HIP_CHECK(hipMemsetAsync(d_out, 0xff, (size_t)std::max<int64_t>(out_ints, 4) * 4, s));

    OSFM_HIP_CHECK(hipMemsetAsync(m->exact_count.ptr, 0, 16, s));
    bool timed[2] = {false, false};
    bool probed = false;
    for (int type = 0; type < 2; ++type) {
        const int np = (int)probs[type].size();
        if (np == 0) continue;
        for (int i = 0; i < np; ++i) {
            probs[type][i].m12 = d_out + plan.m12_off[type][i];
            probs[type][i].m21 = d_out + plan.m21_off[type][i];
        }
        OSFM_RETURN_IF(m->d_problems[type].reserve(np * sizeof(MatchProblem)));
        OSFM_RETURN_IF(m->mark_off[type].reserve(np * 2 * sizeof(int64_t)));
        OSFM_RETURN_IF(m->counts[type].reserve(np * sizeof(int32_t)));
        OSFM_HIP_CHECK(hipMemcpyAsync(m->d_problems[type].ptr, probs[type].data(),
            np * sizeof(MatchProblem), hipMemcpyHostToDevice, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(m->mark_off[type].ptr, plan.mark_off[type].data(),
            np * 2 * sizeof(int64_t), hipMemcpyHostToDevice, s));
        OSFM_HIP_CHECK(hipMemsetAsync(m->counts[type].ptr, 0, np * sizeof(int32_t), s));
        const MatchProblem *dp = m->d_problems[type].as<MatchProblem>();
        const LoweTable tab = type == 0 ? m->tab_sift : m->tab_surf;
        const int ecap = (int)std::min<int64_t>(total_queries, 0x7fffffff);
        int32_t *ecount = m->exact_count.as<int32_t>() + type;

        if (cascade) {
            OSFM_HIP_CHECK(hipEventRecord(m->ev[type][0], s));
            timed[type] = true;
            OSFM_RETURN_IF(m->cas_state.reserve((size_t)std::max<int64_t>(plan.cas_queries[type], 1) * kCasMaxCand * 4));
            launch_cashash_match(type == 0 ? 128 : 64, dp, np, max_n[type], m->cas_state.as<int32_t>(), tab, s);
            OSFM_HIP_CHECK(hipEventRecord(m->ev[type][1], s));
        } else {
            if (total_blocks[type] > 0) { OSFM_HIP_CHECK(hipEventRecord(m->ev[type][0], s)); timed[type] = true; }
            unsigned long long *probe = nullptr;
            if (type == 0 && mode.limit == 0) {
                OSFM_RETURN_IF(m->clock_probe.reserve(16));
                OSFM_HIP_CHECK(hipMemsetAsync(m->clock_probe.ptr, 0, 16, s));
                probe = m->clock_probe.as<unsigned long long>();
                probed = true;
            }
            if (!m->zero_tile.ptr) {
                OSFM_RETURN_IF(m->zero_tile.reserve((size_t)kTileCols * 128));
                OSFM_HIP_CHECK(hipMemsetAsync(m->zero_tile.ptr, 0, (size_t)kTileCols * 128, s));
            }
            launch_match_tiles(type == 0 ? 8 : 4, plan.needs_mask[type], plan.any_special[type], plan.any_c0[type],
                plan.any_corrected[type], dp, np, total_blocks[type],
                m->rowparts.as<RowPart>(), m->colparts.as<ColPart>(), s, probe, m->zero_tile.as<int8_t>());
            if (timed[type]) OSFM_HIP_CHECK(hipEventRecord(m->ev[type][1], s));
            if (type == 0 && !(spjobs.empty() && spjobs_wide.empty())) {
                OSFM_HIP_CHECK(hipEventRecord(m->ev_sp[0], s));
                launch_match_special(dp, m->d_spjobs.as<SpecialJob>(), (int)spjobs.size(), m->sp_parts.as<RowPart>(),
                    m->sp_col.as<int32_t>(), s);
                launch_match_special_wide(dp, m->d_spjobs.as<SpecialJob>() + spjobs.size(), (int)spjobs_wide.size(),
                    m->sp_parts.as<RowPart>(), m->sp_col.as<int32_t>(), s);
                OSFM_HIP_CHECK(hipEventRecord(m->ev_sp[1], s));
            }
            const bool rs = type == 0 && plan.bucketed;
            if (rs) OSFM_HIP_CHECK(hipMemsetAsync(m->rs_count.ptr, 0, (size_t)rs_buckets * sizeof(int32_t), s));
            launch_match_finish(dp, np, max_n[type], m->rowparts.as<RowPart>(),
                m->colparts.as<ColPart>(), m->sp_parts.as<RowPart>(), m->sp_col.as<int32_t>(), tab, 0,
                m->exact_items.as<ExactItem>(), ecount, ecap, rs ? m->rs_count.as<int32_t>() : nullptr,
                rs ? m->rs_items.as<RescoreItem>() : nullptr, s);
            if (rs)
                launch_match_rescore(dp, np, m->rs_count.as<int32_t>(), m->rs_items.as<RescoreItem>(), rs_buckets, tab,
                    m->exact_items.as<ExactItem>(), ecount, ecap, s);
            launch_exact_scan(type == 0 ? 128 : 64, dp, m->exact_items.as<ExactItem>(), ecount, ecap,
                tab, s);
        }
        launch_cross_check_mark(dp, np, max_n[type], m->keep.as<uint8_t>(), m->keep.as<uint8_t>(),
            m->mark_off[type].as<int64_t>(), m->counts[type].as<int32_t>(), s);
        if (mode.apply)
            launch_cross_check_apply(dp, np, max_n[type], m->keep.as<uint8_t>(),
                m->keep.as<uint8_t>(), m->mark_off[type].as<int64_t>(), s);
        OSFM_HIP_CHECK(hipGetLastError());
    }

    // --- counts back -------------------------------------------------------
    std::vector<int32_t> hc[2];
    int32_t hexact[4] = {0, 0, 0, 0};
    for (int type = 0; type < 2; ++type) {
        hc[type].resize(probs[type].size());
        if (!hc[type].empty())
            OSFM_HIP_CHECK(hipMemcpyAsync(hc[type].data(), m->counts[type].ptr,
                hc[type].size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    OSFM_HIP_CHECK(hipMemcpyAsync(hexact, m->exact_count.ptr, 16, hipMemcpyDeviceToHost, s));
    unsigned long long hprobe[2] = {0, 0};
    if (probed) OSFM_HIP_CHECK(hipMemcpyAsync(hprobe, m->clock_probe.ptr, 16, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    m->stats.tile_shader_cycles += (double)hprobe[0];
    m->stats.tile_refclk_ticks += (double)hprobe[1];
    for (int p = 0; p < num_pairs; ++p) {
        int c = 0;
        for (int type = 0; type < 2; ++type)
            if (plans[p].prob_index[type] >= 0) c += hc[type][plans[p].prob_index[type]];
        res->counts[p] = c;
    }
    for (int type = 0; type < 2; ++type) {
        if (!timed[type]) continue;
        float ms = 0.f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, m->ev[type][0], m->ev[type][1]));
        if (cascade) {
            m->stats.cashash_kernel_ms += ms;
            m->stats.cashash_kernel_launches += 1;
        } else if (mode.limit > 0) {
            m->stats.lowres_kernel_ms += ms;
            m->stats.lowres_kernel_launches += 1;
        } else {
            m->stats.tile_kernel_ms += ms;
            m->stats.tile_kernel_launches += 1;
            m->stats.tile_workgroups += total_blocks[type];
            if (type == 1) { m->stats.surf_tile_kernel_ms += ms; m->stats.surf_tile_kernel_launches += 1; }
        }
    }
    if (!(spjobs.empty() && spjobs_wide.empty())) {
        float ms = 0.f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, m->ev_sp[0], m->ev_sp[1]));
        m->stats.special_kernel_ms += ms;
        m->stats.special_kernel_launches += 1;
    }
    m->stats.exact_scan_queries += hexact[0] + hexact[1];
    if (cascade) {
        // no dense products in this mode
    } else if (mode.limit > 0) {
        m->stats.lowres_mac_count += plan.macs;
    } else {
        m->stats.mac_count += plan.macs;
        m->stats.surf_mac_count += plan.macs_surf;
        m->stats.algorithmic_bytes += plan.alg_bytes;
    }
    return OSFM_OK;
}

}  // namespace osfm
