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
    BatchResult *res, const SliceSink *sink, bool *sliced)
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
    if (sliced) *sliced = false;
    OSFM_RETURN_IF(plan_batch(m->views, m->opts, m->special_max, knobs, pairs, num_pairs, mode, &plan));
    // the caller reads the pairs' places and lengths from the result
    res->plans = plan.plans;
    res->out_ints = plan.out_ints;
    const std::vector<PairPlan> &plans = plan.plans;
    std::vector<MatchProblem> *probs = plan.probs;
    const std::vector<SpecialJob> &spjobs = plan.spjobs, &spjobs_wide = plan.spjobs_wide;
    const int64_t out_ints = plan.out_ints, total_queries = plan.total_queries, rs_buckets = plan.rs_buckets;
    const int *total_blocks = plan.total_blocks, *max_n = plan.max_n;
    const int np_of[2] = {(int)probs[0].size(), (int)probs[1].size()};

    // --- slices of the post-work ------------------------------------------
    // slice k: the pairs [bounds[k], bounds[k + 1]) and with them the problems [first[type][k], first[type][k + 1])
    // of either type (the problems of a type are in pair order)
    std::vector<int> bounds;
    int nslices = 1;
    if (sink && !cascade && num_pairs > 0) nslices = post_slice_bounds(num_pairs, sink->requested, &bounds);
    if (nslices <= 1) { bounds.assign({0, num_pairs}); nslices = 1; }
    std::vector<int> first[2];
    for (int type = 0; type < 2; ++type) {
        first[type].assign(nslices + 1, np_of[type]);
        int k = 0, seen = 0;
        for (int p = 0; p < num_pairs; ++p) {
            while (k < nslices && bounds[k] <= p) first[type][k++] = seen;
            if (plans[p].prob_index[type] >= 0) ++seen;
        }
    }
    // a slice's rescore launch walks its own buckets from 0: the bucket and item offsets of its problems count
    // from the slice's first (a batch of one slice keeps them as planned)
    std::vector<int64_t> bucket0(nslices + 1, rs_buckets), item0(nslices + 1, plan.rs_items);
    for (int k = 0; k < nslices; ++k) {
        const int f = first[0][k];
        if (f < np_of[0]) { bucket0[k] = probs[0][f].rs_bucket_off; item0[k] = probs[0][f].rs_item_off; }
    }
    for (int k = nslices - 1; k >= 0; --k) {       // (a slice without SIFT problems: empty, at the next one's start)
        bucket0[k] = std::min(bucket0[k], bucket0[k + 1]);
        item0[k] = std::min(item0[k], item0[k + 1]);
    }
    for (int k = 1; k < nslices; ++k)
        for (int i = first[0][k]; i < first[0][k + 1]; ++i) {
            probs[0][i].rs_bucket_off -= bucket0[k];
            probs[0][i].rs_item_off -= item0[k];
        }

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
    if (plan.bucketed) OSFM_RETURN_IF(m->rs_items.reserve(grown(plan.rs_items) * sizeof(RescoreItem)));
    OSFM_RETURN_IF(m->sp_parts.reserve((size_t)std::max<int64_t>(plan.sp_recs, 1) * sizeof(RowPart)));
    OSFM_RETURN_IF(m->sp_col.reserve((size_t)std::max<int64_t>(plan.sp_cols, 1) * 4));
    // (every batch ends with a wait for the stream: nothing still reads the two blocks when a reserve frees them)
    const ControlLayout cl = control_layout(np_of[0], np_of[1], plan.bucketed ? rs_buckets : 0);
    const StagingLayout sl = staging_layout(np_of[0], np_of[1], spjobs.size(), spjobs_wide.size());
    OSFM_RETURN_IF(m->d_control.reserve(grown((int64_t)cl.bytes)));
    OSFM_RETURN_IF(m->d_batch.reserve(grown((int64_t)sl.bytes)));
    OSFM_RETURN_IF(m->h_read.reserve(cl.read_bytes * nslices));
    hipStream_t s = m->stream;
    {
        // the views this batch names: their uploads (own stream) before anything of the batch
        std::vector<uint8_t> seen(m->views.size(), 0);
        for (int p = 0; p < num_pairs; ++p)
            for (int v : {plans[p].v1, plans[p].v2})
                if (!seen[v]) { seen[v] = 1; if (m->views[v].ready) OSFM_HIP_CHECK(hipStreamWaitEvent(s, m->views[v].ready, 0)); }
    }
    int32_t *d_out = m->out.as<int32_t>();
    char *d_ctl = m->d_control.as<char>(), *d_up = m->d_batch.as<char>();

    // --- one upload -------------------------------------------------------
    {
        // (the upload that last read this block is over: every batch ends with a wait for the stream)
        PinnedBlock &stage = m->h_batch;
        OSFM_RETURN_IF(stage.reserve(sl.bytes));
        for (int type = 0; type < 2; ++type) {
            for (int i = 0; i < np_of[type]; ++i) {
                probs[type][i].m12 = d_out + plan.m12_off[type][i];
                probs[type][i].m21 = d_out + plan.m21_off[type][i];
            }
            if (np_of[type] == 0) continue;
            memcpy(stage.ptr + sl.probs_off[type], probs[type].data(), (size_t)np_of[type] * sizeof(MatchProblem));
            memcpy(stage.ptr + sl.mark_off[type], plan.mark_off[type].data(), (size_t)np_of[type] * 2 * sizeof(int64_t));
        }
        if (!spjobs.empty()) memcpy(stage.ptr + sl.sp_off, spjobs.data(), spjobs.size() * sizeof(SpecialJob));
        if (!spjobs_wide.empty())
            memcpy(stage.ptr + sl.sp_off + spjobs.size() * sizeof(SpecialJob), spjobs_wide.data(),
                spjobs_wide.size() * sizeof(SpecialJob));
        OSFM_HIP_CHECK(hipMemcpyAsync(d_up, stage.ptr, sl.bytes, hipMemcpyHostToDevice, s));
    }
    const SpecialJob *d_spjobs = reinterpret_cast<const SpecialJob *>(d_up + sl.sp_off);
    OSFM_HIP_CHECK(hipMemsetAsync(d_out, 0xff, (size_t)std::max<int64_t>(out_ints, 4) * 4, s));
    // --- one memset: exact-scan counters, clock probe, counts, rescore bucket counts ---
    OSFM_HIP_CHECK(hipMemsetAsync(d_ctl, 0, cl.bytes, s));
    int32_t *d_rs_count = reinterpret_cast<int32_t *>(d_ctl + cl.rs_off);
    const int ecap = (int)std::min<int64_t>(total_queries, 0x7fffffff);

    // finish, rescore, exact scan and cross-check of the problems of slice k of a type (exhaustive matching)
    auto post_work = [&](int type, int k) -> int {
        const int f = first[type][k], np = first[type][k + 1] - f;
        if (np <= 0) return OSFM_OK;
        const MatchProblem *dp = reinterpret_cast<const MatchProblem *>(d_up + sl.probs_off[type]) + f;
        const int64_t *d_mark = reinterpret_cast<const int64_t *>(d_up + sl.mark_off[type]) + 2 * (size_t)f;
        int32_t *d_counts = reinterpret_cast<int32_t *>(d_ctl + cl.counts_off[type]) + f;
        const LoweTable tab = type == 0 ? m->tab_sift : m->tab_surf;
        // (every slice of a type has a counter of its own; the item list is shared: a slice's scan has read it
        //  before the next slice's finish, behind it on the stream, writes it)
        int32_t *ecount = reinterpret_cast<int32_t *>(d_ctl + cl.exact_off) + type * kMaxPostSlices + k;
        const bool rs = type == 0 && plan.bucketed;
        int32_t *rsc = rs ? d_rs_count + bucket0[k] : nullptr;
        RescoreItem *rsi = rs ? m->rs_items.as<RescoreItem>() + item0[k] : nullptr;
        launch_match_finish(dp, np, max_n[type], m->rowparts.as<RowPart>(),
            m->colparts.as<ColPart>(), m->sp_parts.as<RowPart>(), m->sp_col.as<int32_t>(), tab, 0,
            m->exact_items.as<ExactItem>(), ecount, ecap, rsc, rsi, s);
        if (rs)
            launch_match_rescore(dp, np, rsc, rsi, bucket0[k + 1] - bucket0[k], tab,
                m->exact_items.as<ExactItem>(), ecount, ecap, s);
        launch_exact_scan(type == 0 ? 128 : 64, dp, m->exact_items.as<ExactItem>(), ecount, ecap, tab, s);
        launch_cross_check_mark(dp, np, max_n[type], m->keep.as<uint8_t>(), m->keep.as<uint8_t>(), d_mark, d_counts, s);
        if (mode.apply)
            launch_cross_check_apply(dp, np, max_n[type], m->keep.as<uint8_t>(), m->keep.as<uint8_t>(), d_mark, s);
        OSFM_HIP_CHECK(hipGetLastError());
        return OSFM_OK;
    };

    bool timed[2] = {false, false};
    bool probed = false;
    for (int type = 0; type < 2; ++type) {
        const int np = np_of[type];
        if (np == 0) continue;
        const MatchProblem *dp = reinterpret_cast<const MatchProblem *>(d_up + sl.probs_off[type]);
        const LoweTable tab = type == 0 ? m->tab_sift : m->tab_surf;

        if (cascade) {
            OSFM_HIP_CHECK(hipEventRecord(m->ev[type][0], s));
            timed[type] = true;
            OSFM_RETURN_IF(m->cas_state.reserve((size_t)std::max<int64_t>(plan.cas_queries[type], 1) * kCasMaxCand * 4));
            launch_cashash_match(type == 0 ? 128 : 64, dp, np, max_n[type], m->cas_state.as<int32_t>(), tab, s);
            OSFM_HIP_CHECK(hipEventRecord(m->ev[type][1], s));
            launch_cross_check_mark(dp, np, max_n[type], m->keep.as<uint8_t>(), m->keep.as<uint8_t>(),
                reinterpret_cast<const int64_t *>(d_up + sl.mark_off[type]),
                reinterpret_cast<int32_t *>(d_ctl + cl.counts_off[type]), s);
            if (mode.apply)
                launch_cross_check_apply(dp, np, max_n[type], m->keep.as<uint8_t>(), m->keep.as<uint8_t>(),
                    reinterpret_cast<const int64_t *>(d_up + sl.mark_off[type]), s);
            OSFM_HIP_CHECK(hipGetLastError());
            continue;
        }
        if (total_blocks[type] > 0) { OSFM_HIP_CHECK(hipEventRecord(m->ev[type][0], s)); timed[type] = true; }
        unsigned long long *probe = nullptr;
        if (type == 0 && mode.limit == 0) {
            probe = reinterpret_cast<unsigned long long *>(d_ctl + cl.probe_off);
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
            launch_match_special(dp, d_spjobs, (int)spjobs.size(), m->sp_parts.as<RowPart>(),
                m->sp_col.as<int32_t>(), s);
            launch_match_special_wide(dp, d_spjobs + spjobs.size(), (int)spjobs_wide.size(),
                m->sp_parts.as<RowPart>(), m->sp_col.as<int32_t>(), s);
            OSFM_HIP_CHECK(hipEventRecord(m->ev_sp[1], s));
        }
        // one slice: a type's post-work straight behind its tiles; more: behind the tiles of both types, below
        if (nslices == 1) OSFM_RETURN_IF(post_work(type, 0));
        else OSFM_HIP_CHECK(hipGetLastError());
    }

    // --- counts back -------------------------------------------------------
    // the head of the control block, once per slice, each into a place of its own in h_read
    const char *h_last = m->h_read.ptr + (size_t)(nslices - 1) * cl.read_bytes;
    auto counts_of = [&](const char *h, int p0, int p1) {
        for (int p = p0; p < p1; ++p) {
            int c = 0;
            for (int type = 0; type < 2; ++type)
                if (plans[p].prob_index[type] >= 0)
                    c += reinterpret_cast<const int32_t *>(h + cl.counts_off[type])[plans[p].prob_index[type]];
            res->counts[p] = c;
        }
    };
    if (nslices == 1) {
        OSFM_HIP_CHECK(hipMemcpyAsync(m->h_read.ptr, d_ctl, cl.read_bytes, hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        counts_of(h_last, 0, num_pairs);
    } else {
        for (int k = 0; k < nslices; ++k) {
            for (int type = 0; type < 2; ++type) OSFM_RETURN_IF(post_work(type, k));
            OSFM_RETURN_IF(m->ev_slice[k].make());
            OSFM_HIP_CHECK(hipMemcpyAsync(m->h_read.ptr + (size_t)k * cl.read_bytes, d_ctl, cl.read_bytes,
                hipMemcpyDeviceToHost, s));
            OSFM_HIP_CHECK(hipEventRecord(m->ev_slice[k].e, s));
        }
        // every slice is queued: the stream works through them while the host hands out the finished ones
        for (int k = 0; k < nslices; ++k) {
            OSFM_HIP_CHECK(hipEventSynchronize(m->ev_slice[k].e));
            counts_of(m->h_read.ptr + (size_t)k * cl.read_bytes, bounds[k], bounds[k + 1]);
            OSFM_RETURN_IF(sink->on_slice(bounds[k], bounds[k + 1]));
        }
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        if (sliced) *sliced = true;
    }
    unsigned long long hprobe[2] = {0, 0};
    if (probed) memcpy(hprobe, h_last + cl.probe_off, sizeof(hprobe));
    long long hexact = 0;
    for (int type = 0; type < 2; ++type)
        for (int k = 0; k < nslices; ++k)
            hexact += reinterpret_cast<const int32_t *>(h_last + cl.exact_off)[type * kMaxPostSlices + k];
    m->stats.tile_shader_cycles += (double)hprobe[0];
    m->stats.tile_refclk_ticks += (double)hprobe[1];
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
    if (!cascade && !(spjobs.empty() && spjobs_wide.empty())) {
        float ms = 0.f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, m->ev_sp[0], m->ev_sp[1]));
        m->stats.special_kernel_ms += ms;
        m->stats.special_kernel_launches += 1;
    }
    m->stats.exact_scan_queries += hexact;
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
