// The matcher's host arithmetic (match_plan.h).  A wrong offset or block count here is an out-of-bounds access in a
// kernel, so nothing in this file needs a device: tests/host/match_plan_check.cc checks it on a CPU.
#include <algorithm>
#include <climits>
#include <cstring>
#include <queue>

#include "match_plan.h"

namespace osfm {

int check_view(const std::vector<ViewData> &views, int v, const char *what)
{
    if (v < 0 || v >= (int)views.size()) {
        set_error("%s: view id %d out of range [0, %zu)", what, v, views.size());
        return OSFM_E_ARG;
    }
    if (!views[v].set) {
        set_error("%s: view %d has not been set", what, v);
        return OSFM_E_STATE;
    }
    return OSFM_OK;
}

void BatchPlan::clear()
{
    BatchPlan fresh;
    auto keep = [](auto &to, auto &from) { from.clear(); to.swap(from); };
    keep(fresh.plans, plans);
    keep(fresh.spjobs, spjobs);
    keep(fresh.spjobs_wide, spjobs_wide);
    for (int type = 0; type < 2; ++type) {
        keep(fresh.probs[type], probs[type]);
        keep(fresh.m12_off[type], m12_off[type]);
        keep(fresh.m21_off[type], m21_off[type]);
        keep(fresh.mark_off[type], mark_off[type]);
    }
    *this = std::move(fresh);
}

int plan_batch(const std::vector<ViewData> &views, const osfm_match_options &opts, int special_max, const PlanKnobs &knobs,
    const osfm_pair *pairs, int num_pairs, const BatchMode &mode, BatchPlan *out)
{
    BatchPlan &bp = *out;
    bp.clear();
    const int lowres_limit = mode.limit;
    const bool cascade = bp.cascade = cascade_batch(opts, mode);
    bp.plans.assign(num_pairs, PairPlan());
    struct SpEntry { int problem, side, view, units, nchunk; };
    std::vector<SpEntry> spentries;

    // Segment length of the correction-free problems: a workgroup walks seg_cols columns for its 256 rows.
    // Every segment costs a prologue (A fragments, two tiles), a row merge and a set of row partials, so a
    // launch with enough row blocks to fill the chip several times over takes one segment per row block (up to
    // kSegColsMax columns); a small launch (the per-pair entries) is cut into more, shorter ones.
    int64_t rb_estimate = 0;
    for (int p = 0; p < num_pairs; ++p) {
        const int v1 = pairs[p].view_1;
        if (v1 >= 0 && v1 < (int)views.size())
            rb_estimate += (std::max(views[v1].ns, views[v1].nu) + kRowsPerBlock - 1) / kRowsPerBlock;
    }
    auto choose_seg_cols = [&](int n2) {
        const int ncyc = (n2 + kCycleCols - 1) / kCycleCols;
        int cyc;                                                   // cycles per segment
        if (knobs.seg_tiles > 0) cyc = std::max(1, knobs.seg_tiles / 16);     // measurements (tools/seg_intercept.sh)
        else {
            constexpr int64_t kWantBlocks = 2048;                  // four rounds of the 512 resident workgroups
            const int64_t want = (kWantBlocks + std::max<int64_t>(rb_estimate, 1) - 1) / std::max<int64_t>(rb_estimate, 1);
            const int nseg = (int)std::min<int64_t>(std::max<int64_t>(want, 1), ncyc);
            cyc = (ncyc + nseg - 1) / nseg;
        }
        cyc = std::min(cyc, kSegColsMax / kCycleCols);
        return cyc * kCycleCols;
    };

    for (int p = 0; p < num_pairs; ++p) {
        PairPlan &pl = bp.plans[p];
        pl.v1 = pairs[p].view_1; pl.v2 = pairs[p].view_2;
        OSFM_RETURN_IF(check_view(views, pl.v1, "match"));
        OSFM_RETURN_IF(check_view(views, pl.v2, "match"));
        const ViewData &a = views[pl.v1], &b = views[pl.v2];
        pl.ns1 = a.ns; pl.nu1 = a.nu; pl.ns2 = b.ns; pl.nu2 = b.nu;
        pl.has_sift = a.ns > 0 && (mode.type_mask & 1);
        pl.has_surf = a.nu > 0 && (mode.type_mask & 2);
        // sfm::CascadeHashing leaves a type out of the Result altogether when view_2 lacks it
        // (cascade_hashing.h:341-342; ExhaustiveMatching keeps the -1 filled block)
        if (cascade && !opts.cascade_keep_empty_blocks) {
            if (b.ns == 0) pl.has_sift = false;
            if (b.nu == 0) pl.has_surf = false;
        }
        // exhaustive_matching.cc:153-177: SIFT takes precedence
        if (mode.lowres && pl.has_sift) pl.has_surf = false;
        if (lowres_limit > 0) {
            pl.ns1 = std::min(pl.ns1, lowres_limit); pl.ns2 = std::min(pl.ns2, lowres_limit);
            pl.nu1 = std::min(pl.nu1, lowres_limit); pl.nu2 = std::min(pl.nu2, lowres_limit);
        }
        const int e1 = pl.has_sift ? pl.ns1 : 0;      // sift entries on side 1 / 2
        const int e2 = pl.has_sift ? pl.ns2 : 0;
        pl.len12 = e1 + (pl.has_surf ? pl.nu1 : 0);
        pl.len21 = e2 + (pl.has_surf ? pl.nu2 : 0);
        pl.off12 = bp.out_ints; bp.out_ints += round_up(pl.len12, 4);
        pl.off21 = bp.out_ints; bp.out_ints += round_up(pl.len21, 4);
        pl.prob_index[0] = pl.prob_index[1] = -1;
        for (int type = 0; type < 2; ++type) {
            if (type == 0 ? !pl.has_sift : !pl.has_surf) continue;
            MatchProblem pr;
            memset(&pr, 0, sizeof(pr));
            pr.n1 = type == 0 ? pl.ns1 : pl.nu1;
            pr.n2 = type == 0 ? pl.ns2 : pl.nu2;
            pr.A = (type == 0 ? a.sift : a.surf).as<int8_t>();
            pr.B = (type == 0 ? b.sift : b.surf).as<int8_t>();
            pr.corrA = (type == 0 ? a.sift_corr : a.surf_corr).as<int32_t>();
            pr.corrB = (type == 0 ? b.sift_corr : b.surf_corr).as<int32_t>();
            // raw row operand: SURF bytes are the values already
            pr.A_raw = (type == 0 ? a.sift_raw : a.surf).as<int8_t>();
            pr.corrA_raw = (type == 0 ? a.sift_raw_corr : a.surf_corr).as<int32_t>();
            // a num_features-limited batch runs the masked kernel, which keeps every
            // row on the keyed (value-128) path
            const bool limited = lowres_limit > 0;
            const int n_special = (type == 0 && !limited) ? a.n_special : 0;
            pr.n_special = n_special;
            pr.A_special = a.special.as<int8_t>();
            pr.corrA_special = a.special_corr.as<int32_t>();
            pr.special_map = a.special_map.as<int32_t>();
            pr.special_slot = n_special > 0 ? a.special_slot.as<int32_t>() : nullptr;
            const bool empty = pr.n1 == 0 || pr.n2 == 0;
            if (limited) bp.needs_mask[type] = true;
            // correction-free column operand: SURF bytes are the values; SIFT views
            // without a value > 127 (the raw copy then holds every descriptor)
            pr.B_raw = (type == 0 ? b.sift_raw : b.surf).as<int8_t>();
            pr.c0 = (type == 1 || b.n_special == 0) ? 1 : 0;
            // Few special descriptors on either side (the case real SIFT data produces,
            // sift.cc:830-839): they go through match_special_kernel and every other
            // descriptor of both views stays on the correction-free form.
            if (type == 0 && !limited && !cascade && !empty && (a.n_special > 0 || b.n_special > 0) &&
                a.n_special <= special_max && b.n_special <= special_max) {
                pr.sp = 1; pr.c0 = 1;
                pr.nsA = a.n_special; pr.nsB = b.n_special;
                pr.n_special = 0;                          // no special row blocks in the tile launch
                pr.special_slot = a.n_special > 0 ? a.special_slot.as<int32_t>() : nullptr;
                pr.B_special = b.special.as<int8_t>();
                pr.corrB_special = b.special_corr.as<int32_t>();
                pr.special_map_B = b.special_map.as<int32_t>();
                pr.special_slot_B = b.n_special > 0 ? b.special_slot.as<int32_t>() : nullptr;
                for (int side = 0; side < 2; ++side) {
                    const int ns = side == 0 ? pr.nsA : pr.nsB, no = side == 0 ? pr.n2 : pr.n1;
                    if (ns == 0) continue;
                    // more than kSpSlots units: the wide kernel (smaller chunks, shared through LDS)
                    const int units = (ns + 31) / 32;
                    pr.sp_wide[side] = units > kSpSlots ? 1 : 0;
                    const int chunk_cols = pr.sp_wide[side] ? kSpWideChunk : kSpChunk;
                    const int nchunk = (no + chunk_cols - 1) / chunk_cols;
                    pr.sp_row_off[side] = bp.sp_recs; bp.sp_recs += (int64_t)nchunk * round_up(ns, 32);
                    pr.sp_col_off[side] = bp.sp_cols; bp.sp_cols += round_up(no, 32);
                    spentries.push_back({(int)bp.probs[type].size(), side, side == 0 ? pl.v2 : pl.v1, units, nchunk});
                }
            }
            if (!empty && !limited) (pr.c0 ? bp.any_c0 : bp.any_corrected)[type] = true;
            if (!empty && pr.n_special > 0) bp.any_special[type] = true;
            pr.nrb_main = empty ? 0 : (pr.n1 + kRowsPerBlock - 1) / kRowsPerBlock;
            pr.nrb = pr.nrb_main + (empty ? 0 : (pr.n_special + kRowsPerBlock - 1) / kRowsPerBlock);
            // (only the RAW row blocks of a c0 problem run the correction-free kernel; its special row blocks, if
            //  any, run the keyed kernel, whose keys hold kSegCols / 32 fragment indices: such a problem keeps kSegCols)
            pr.seg_cols = (pr.c0 && !limited && pr.n_special == 0 && !empty) ? choose_seg_cols(pr.n2) : kSegCols;
            pr.nseg = empty ? 0 : (pr.n2 + pr.seg_cols - 1) / pr.seg_cols;
            pr.n2stride = round_up(pr.n2, kCycleCols);
            pr.block_start = bp.total_blocks[type];
            pr.rs_bucket_off = bp.rs_buckets;
            pr.rs_item_off = bp.rs_items;
            if (type == 0 && !cascade && !empty) {
                bp.rs_buckets += rescore_buckets(pr.nrb_main, pr.n2);
                bp.rs_items += rescore_items(pr.nrb_main, pr.n2);
            }
            if (cascade) {
                // no score tiles: the candidate search works on the hash data of the two views
                const ViewData *vd[2] = {&a, &b};
                for (int side = 0; side < 2; ++side) {
                    pr.cas_rec[side] = vd[side]->cas_rec[type].ptr;
                    pr.cas_start[side] = vd[side]->cas_start[type].as<int32_t>();
                    pr.cas_items[side] = vd[side]->cas_items[type].as<int32_t>();
                }
                pr.cas_state_off[0] = bp.cas_queries[type]; bp.cas_queries[type] += pr.n1;
                pr.cas_state_off[1] = bp.cas_queries[type]; bp.cas_queries[type] += pr.n2;
            } else {
                bp.total_blocks[type] += pr.nrb * pr.nseg;
                pr.rowpart_off = bp.rowpart_recs;
                bp.rowpart_recs += (int64_t)pr.nseg * pr.nrb * kRowsPerBlock;
                pr.colpart_off = bp.colpart_recs;              // nrb * n2stride records = two int32 planes of that many entries
                bp.colpart_recs += (int64_t)pr.nrb * pr.n2stride;
            }
            // the lists' places in the combined output buffer (m12 / m21 follow once it is allocated)
            bp.m12_off[type].push_back(pl.off12 + (type == 0 ? 0 : e1));
            bp.m21_off[type].push_back(pl.off21 + (type == 0 ? 0 : e2));
            // combine_results offsets (matching.cc:74-86) -- SURF entries only
            pr.out_off12 = (type == 1 && mode.apply) ? e2 : 0;
            pr.out_off21 = (type == 1 && mode.apply) ? e1 : 0;
            if (type == 1) {
                // exactness of the int32 fast path needs every 16-bit lane sum
                // in range: guaranteed when |q|^2 * |c|^2 <= 32767^2
                const long long bound = (long long)a.surf_norm2_max * (long long)b.surf_norm2_max;
                pr.force_exact = bound > 32767LL * 32767LL ? 1 : 0;
            }
            pl.prob_index[type] = (int)bp.probs[type].size();
            bp.mark_off[type].push_back(bp.keep_bytes); bp.keep_bytes += round_up(pr.n1, 16);
            bp.mark_off[type].push_back(bp.keep_bytes); bp.keep_bytes += round_up(pr.n2, 16);
            bp.max_n[type] = std::max(bp.max_n[type], std::max(pr.n1, pr.n2));
            bp.total_queries += pr.n1 + pr.n2;
            bp.probs[type].push_back(pr);
            if (!empty) {
                const int dim = type == 0 ? 128 : 64;
                bp.macs += (int64_t)pr.n1 * pr.n2 * dim;
                if (type == 1) bp.macs_surf += (int64_t)pr.n1 * pr.n2 * dim;
                bp.alg_bytes += (int64_t)(pr.n1 + pr.n2) * (dim + 4);
            }
        }
    }
    bp.bucketed = bp.rs_buckets > 0 && bp.rs_buckets <= INT_MAX && bp.max_n[0] < (1 << 26) && !knobs.rescan_wave;

    // Workgroups that stream the same 4096 descriptors of the same view run next to each other:
    // the chunk (512 KB) is then fetched from HBM once per L2 instead of once per pair (in
    // pair order the streamed view of side 0 changes with every pair: 3 GB of HBM reads per
    // 1225 pairs for 128 MB of distinct descriptors).
    // Jobs of match_special_kernel: the entries (one side of one problem) grouped by the view they
    // stream -- up to kSpSlots one-unit entries share a workgroup, an entry with more units has workgroups of
    // its own -- and, per group, one job per chunk; groups of one view next to each other, so that a chunk
    // (512 KB) is fetched from HBM once per L2 and not once per pair.
    std::stable_sort(spentries.begin(), spentries.end(), [](const SpEntry &x, const SpEntry &y) {
        return x.view != y.view ? x.view < y.view : x.units < y.units;
    });
    for (size_t e = 0; e < spentries.size();) {
        SpecialJob j;
        memset(&j, 0, sizeof(j));
        const SpEntry &f = spentries[e];
        if (f.units > kSpSlots) {
            // the wide kernel: one job per chunk of kSpWideChunk candidates
            j.problem[0] = f.problem; j.side[0] = f.side; j.count = 0;
            for (int c = 0; c < f.nchunk; ++c) { j.chunk = c; bp.spjobs_wide.push_back(j); }
            ++e;
            continue;
        }
        if (f.units > 1) {
            j.problem[0] = f.problem; j.side[0] = f.side; j.count = 0;
            ++e;
        } else {
            int c = 0;
            while (c < kSpSlots && e < spentries.size() && spentries[e].view == f.view && spentries[e].units == 1) {
                j.problem[c] = spentries[e].problem; j.side[c] = spentries[e].side; ++c; ++e;
            }
            j.count = c;
        }
        for (int c = 0; c < f.nchunk; ++c) { j.chunk = c; bp.spjobs.push_back(j); }
    }
    return OSFM_OK;
}

// per-pair workspace estimate -> batch size
// pairs per launch group: bounded by the partial-result workspace
// (column partials dominate: nrb * n2 * 8 B per pair) -- 24 GB of the 288 GB
int batch_size_for(const std::vector<ViewData> &views, const osfm_match_options &o, bool lowres)
{
    if (o.pairs_per_batch > 0) return o.pairs_per_batch;
    if (lowres) return 16384;
    size_t worst = 1;
    for (const auto &v : views) {
        const size_t n = (size_t)std::max(v.ns, v.nu) + 256;
        worst = std::max(worst, (n / kRowsPerBlock + 1) * n * sizeof(ColPart) + n * 64);
    }
    const size_t budget = (size_t)24 << 30;
    return (int)std::max<size_t>(1, std::min<size_t>(budget / worst, 4096));
}

// A call that fits one batch is still cut in three when it is large: the lists of one part then leave
// the device (63 MB per 1225 pairs: 2.5 ms of an otherwise idle device) while the next part is matched.
int full_batch_size(const std::vector<ViewData> &views, const osfm_match_options &o, size_t n_full)
{
    int bs = batch_size_for(views, o, false);
    // (not in cascade-hashing mode: its bucket kernels want the large launch)
    if (o.pairs_per_batch <= 0 && !o.geometric_verification && o.matcher_type != OSFM_MATCHER_CASCADE_HASHING && n_full >= 768)
        bs = std::min<int>(bs, (int)((n_full + 2) / 3));
    // parts of equal size: a call of 3898 pairs at 1875 per part ran 1875 + 1875 + 148, and the short part took
    // 17.5 ms where its pairs are worth 8 (a launch's fixed costs and tail): 0.3 s of a 500-view job
    if (o.pairs_per_batch <= 0 && n_full > (size_t)bs) {
        const size_t parts = (n_full + bs - 1) / bs;
        bs = (int)((n_full + parts - 1) / parts);
    }
    return bs;
}

// A slice adds four or five launches and a read-back and hides the copy of the slices before it (63 MB of lists per
// 1225 pairs of 20 000 features).  Neither number here is settled by measurement: one run of the headline step per
// value put 2, 3 and 4 slices 0.4 - 0.8 ms below the parent and within noise of one another
// (profiles/r11_step_ab.txt), and the 96 pairs below which a part stays one sequence are an estimate (a slice's
// launches against the copy time of some tens of pairs).
int default_post_slices(int pairs) { return pairs >= 96 ? 3 : 1; }

int post_slice_bounds(int pairs, int requested, std::vector<int> *bounds)
{
    bounds->clear();
    if (pairs <= 0) return 0;
    if (requested <= 0) requested = default_post_slices(pairs);
    const int n = std::max(1, std::min(std::min(requested, pairs), kMaxPostSlices));
    for (int k = 0; k <= n; ++k) bounds->push_back((int)((int64_t)pairs * k / n));      // n <= pairs: strictly rising
    return n;
}

namespace {
constexpr size_t kBlockAlign = 64;
size_t take(size_t *at, size_t bytes)
{
    const size_t off = *at;
    *at = (off + bytes + kBlockAlign - 1) / kBlockAlign * kBlockAlign;
    return off;
}
}  // namespace

ControlLayout control_layout(size_t np_sift, size_t np_surf, int64_t rs_buckets)
{
    ControlLayout l;
    size_t at = 0;
    l.exact_off = take(&at, (size_t)2 * kMaxPostSlices * sizeof(int32_t));
    l.probe_off = take(&at, 2 * sizeof(unsigned long long));
    l.counts_off[0] = take(&at, np_sift * sizeof(int32_t));
    l.counts_off[1] = take(&at, np_surf * sizeof(int32_t));
    l.read_bytes = at;
    l.rs_off = take(&at, (size_t)std::max<int64_t>(rs_buckets, 0) * sizeof(int32_t));
    l.bytes = at;
    return l;
}

StagingLayout staging_layout(size_t np_sift, size_t np_surf, size_t spjobs, size_t spjobs_wide)
{
    StagingLayout l;
    size_t at = 0;
    l.probs_off[0] = take(&at, np_sift * sizeof(MatchProblem));
    l.probs_off[1] = take(&at, np_surf * sizeof(MatchProblem));
    l.mark_off[0] = take(&at, np_sift * 2 * sizeof(int64_t));
    l.mark_off[1] = take(&at, np_surf * 2 * sizeof(int64_t));
    l.sp_off = take(&at, (spjobs + spjobs_wide) * sizeof(SpecialJob));
    l.bytes = std::max(at, kBlockAlign);
    return l;
}

CompactLayout compact_layout(size_t n)
{
    CompactLayout l;
    size_t at = 0;
    l.m12_off = take(&at, n * sizeof(int64_t));
    l.corr_off = take(&at, n * sizeof(int64_t));
    l.len12_off = take(&at, n * sizeof(int32_t));
    l.keep_off = take(&at, n);
    l.bytes = std::max(at, kBlockAlign);
    return l;
}

// Longest processing time first on N1 * N2 over the pairs `cand` (ascending pair indices); ties go to the lower
// shard.  Equal work everywhere degenerates to round robin, as in distributed.py.
void deal_pairs_lpt(const std::vector<ViewData> &views, int num_shards, const osfm_pair *pairs, const std::vector<int> &cand,
    std::vector<std::vector<int>> *owner)
{
    const int n = num_shards;
    owner->assign(n, {});
    const int nc = (int)cand.size();
    std::vector<int64_t> w(nc);
    bool uniform = true;
    for (int i = 0; i < nc; ++i) {
        const ViewData &a = views[pairs[cand[i]].view_1], &b = views[pairs[cand[i]].view_2];
        w[i] = (int64_t)(a.ns + a.nu) * (int64_t)(b.ns + b.nu);
        uniform &= w[i] == w[0];
    }
    if (uniform) {
        for (int i = 0; i < nc; ++i) (*owner)[i % n].push_back(cand[i]);
        return;
    }
    std::vector<int> order(nc);
    for (int i = 0; i < nc; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return w[x] > w[y]; });
    typedef std::pair<int64_t, int> Load;
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    for (int k = 0; k < n; ++k) heap.push({0, k});
    std::vector<int> own(nc);
    for (int i : order) {
        Load l = heap.top(); heap.pop();
        own[i] = l.second;
        heap.push({l.first + w[i], l.second});
    }
    for (int i = 0; i < nc; ++i) (*owner)[own[i]].push_back(cand[i]);      // ascending inside a shard
}

// Host twin of matching.h:126-127,138-143 for every (d1, d2): the smallest
// (even) d1 that the float ratio test rejects for a given d2.
void build_lowe_table(float lowe, bool is_signed, std::vector<int32_t> *tab)
{
    const volatile float sq = lowe * lowe;     // MATH_POW2 in float
    const float sq_lowe = sq;
    const int dmax = is_signed ? 32258 : 65534;
    tab->assign(32768, 0x7fffffff);
    for (int d2 = 0; d2 <= dmax; d2 += 2) {
        // float(d1)/float(d2) is monotone in d1: binary search on even d1
        int lo = 0, hi = dmax / 2 + 1;   // in units of 2; hi = "never rejected"
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            const float ratio = static_cast<float>(2 * mid) / static_cast<float>(d2);
            if (ratio > sq_lowe) hi = mid; else lo = mid + 1;
        }
        (*tab)[d2 / 2] = lo > dmax / 2 ? 0x7fffffff : 2 * lo;
    }
}

int max_d1_for(float dist_thres, bool is_signed)
{
    const volatile float sq = dist_thres * dist_thres;
    const float sq_dist = sq;
    const int dmax = is_signed ? 32258 : 65534;
    int best = -1;
    // largest d with !(float(d) > sq_dist); monotone
    int lo = 0, hi = dmax;
    if (!(static_cast<float>(0) > sq_dist)) {
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (static_cast<float>(mid) > sq_dist) hi = mid - 1; else lo = mid;
        }
        best = lo;
    }
    return best;
}

}  // namespace osfm
