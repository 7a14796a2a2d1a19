// Checks the matcher's batch plan (orthosfm_amd/csrc/match_plan.hip) on the host: views are sizes only (every buffer
// null), plan_batch runs over the sizes and modes at which the plan changes path, and every range a kernel is handed
// must lie inside the plan's totals and apart from every other.  Nothing is compared against what the code under test
// produced.  Built with AddressSanitizer and UBSan (tests/host/Makefile); prints "ok <cases> cases" when all held.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../orthosfm_amd/csrc/match_plan.h"

namespace osfm {
static char g_error[1024];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace osfm

using namespace osfm;

static const char *g_case = "";
static long g_cases = 0;
#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            fprintf(stderr, "match_plan_check: %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_case); \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)

static int64_t up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static int64_t cdiv(int64_t x, int64_t m) { return (x + m - 1) / m; }

// half-open ranges of one scratch array: inside [0, total), pairwise disjoint (empty ranges own nothing)
struct Ranges {
    std::vector<std::pair<int64_t, int64_t>> r;
    void add(int64_t off, int64_t len) { CHECK(off >= 0 && len >= 0); if (len) r.push_back({off, off + len}); }
    void check(int64_t total)
    {
        std::sort(r.begin(), r.end());
        for (size_t i = 0; i < r.size(); ++i) {
            CHECK(r[i].second <= total);
            if (i) CHECK(r[i - 1].second <= r[i].first);
        }
    }
};

struct Case {
    osfm_match_options opts;
    int special_max = 512;
    PlanKnobs knobs;
    BatchMode mode;
};

static void check_plan(const std::vector<ViewData> &views, const Case &c, const std::vector<osfm_pair> &pairs)
{
    ++g_cases;
    BatchPlan bp;
    CHECK(plan_batch(views, c.opts, c.special_max, c.knobs, pairs.data(), (int)pairs.size(), c.mode, &bp) == OSFM_OK);
    const BatchMode &mode = c.mode;
    const bool limited = mode.limit > 0;
    const bool cascade = c.opts.matcher_type == OSFM_MATCHER_CASCADE_HASHING && !limited;
    CHECK(bp.cascade == cascade);
    CHECK(bp.plans.size() == pairs.size());

    Ranges out, rowparts, colparts, keep, sp_row, sp_col, rs_bucket, rs_item, cas[2];
    struct Side { int view, ns, no, nchunk, units; std::vector<int> seen; };
    std::map<std::pair<int, int>, Side> sp_sides;          // (SIFT problem, side) with special rows on the sp path
    int64_t blocks[2] = {0, 0}, queries = 0, macs = 0, macs_surf = 0, alg_bytes = 0;
    int max_n[2] = {0, 0};
    bool needs_mask[2] = {false, false}, any_special[2] = {false, false}, any_c0[2] = {false, false}, any_corr[2] = {false, false};
    size_t next_prob[2] = {0, 0};
    Ranges pair_out;

    for (size_t p = 0; p < pairs.size(); ++p) {
        const PairPlan &pl = bp.plans[p];
        const ViewData &a = views[pairs[p].view_1], &b = views[pairs[p].view_2];
        CHECK(pl.v1 == pairs[p].view_1 && pl.v2 == pairs[p].view_2);
        // the types of the pair, as the reference's matchers decide them
        bool has[2] = {a.ns > 0 && (mode.type_mask & 1), a.nu > 0 && (mode.type_mask & 2)};
        if (cascade && !c.opts.cascade_keep_empty_blocks) { if (b.ns == 0) has[0] = false; if (b.nu == 0) has[1] = false; }
        if (mode.lowres && has[0]) has[1] = false;
        auto lim = [&](int n) { return limited ? std::min(n, mode.limit) : n; };
        const int n1[2] = {lim(a.ns), lim(a.nu)}, n2[2] = {lim(b.ns), lim(b.nu)};
        const int e1 = has[0] ? n1[0] : 0, e2 = has[0] ? n2[0] : 0;
        CHECK(pl.has_sift == has[0] && pl.has_surf == has[1]);
        CHECK(pl.len12 == e1 + (has[1] ? n1[1] : 0));
        CHECK(pl.len21 == e2 + (has[1] ? n2[1] : 0));
        pair_out.add(pl.off12, pl.len12);
        pair_out.add(pl.off21, pl.len21);
        for (int type = 0; type < 2; ++type) {
            CHECK((pl.prob_index[type] >= 0) == has[type]);
            if (!has[type]) continue;
            const int i = pl.prob_index[type];
            CHECK((size_t)i == next_prob[type]++ && (size_t)i < bp.probs[type].size());
            const MatchProblem &pr = bp.probs[type][i];
            CHECK(pr.n1 == n1[type] && pr.n2 == n2[type]);
            const bool empty = pr.n1 == 0 || pr.n2 == 0;
            // output lists: inside the pair's blocks, SIFT entries first
            CHECK(pr.m12 == nullptr && pr.m21 == nullptr);
            const int64_t o12 = bp.m12_off[type][i], o21 = bp.m21_off[type][i];
            CHECK(o12 == pl.off12 + (type ? e1 : 0) && o21 == pl.off21 + (type ? e2 : 0));
            out.add(o12, pr.n1);
            out.add(o21, pr.n2);
            CHECK(pr.out_off12 == ((type == 1 && mode.apply) ? e2 : 0));
            CHECK(pr.out_off21 == ((type == 1 && mode.apply) ? e1 : 0));
            // keep bytes: owned by empty problems too
            keep.add(bp.mark_off[type][2 * i], pr.n1);
            keep.add(bp.mark_off[type][2 * i + 1], pr.n2);
            // the kernel form (comments of MatchProblem)
            const bool want_sp = type == 0 && !limited && !cascade && !empty && (a.n_special > 0 || b.n_special > 0) &&
                                 a.n_special <= c.special_max && b.n_special <= c.special_max;
            CHECK((pr.sp != 0) == want_sp);
            if (type == 1) CHECK(pr.c0 == 1 && pr.n_special == 0 && pr.sp == 0);
            if (pr.sp) {
                CHECK(pr.c0 == 1 && pr.n_special == 0 && pr.nsA == a.n_special && pr.nsB == b.n_special);
            } else {
                CHECK(pr.nsA == 0 && pr.nsB == 0 && pr.sp_wide[0] == 0 && pr.sp_wide[1] == 0);
                if (type == 0) {
                    CHECK(pr.n_special == (limited ? 0 : a.n_special));
                    CHECK(pr.c0 == (b.n_special == 0 ? 1 : 0));
                }
            }
            if (type == 1) {
                const long long bound = (long long)a.surf_norm2_max * (long long)b.surf_norm2_max;
                CHECK(pr.force_exact == (bound > 32767LL * 32767LL ? 1 : 0));
            } else {
                CHECK(pr.force_exact == 0);
            }
            // row blocks and column segments
            CHECK(pr.n2stride % kCycleCols == 0 && pr.n2stride >= pr.n2);
            CHECK(pr.seg_cols % kCycleCols == 0 && pr.seg_cols >= kCycleCols && pr.seg_cols <= kSegColsMax);
            if (empty) {
                CHECK(pr.nrb == 0 && pr.nseg == 0 && pr.nrb_main == 0);
            } else {
                CHECK((int64_t)pr.nrb_main * kRowsPerBlock >= pr.n1 && (int64_t)(pr.nrb_main - 1) * kRowsPerBlock < pr.n1);
                CHECK(pr.nrb >= pr.nrb_main && (int64_t)(pr.nrb - pr.nrb_main) * kRowsPerBlock >= pr.n_special);
                CHECK((pr.nrb > pr.nrb_main) == (pr.n_special > 0));
                CHECK((int64_t)pr.nseg * pr.seg_cols >= pr.n2 && (int64_t)(pr.nseg - 1) * pr.seg_cols < pr.n2);
            }
            if (pr.n_special > 0 || limited || !pr.c0) CHECK(pr.seg_cols == kSegCols);
            if (c.knobs.seg_tiles > 0 && pr.c0 && !limited && pr.n_special == 0 && !empty)
                CHECK(pr.seg_cols == std::min(std::max(1, c.knobs.seg_tiles / 16) * kCycleCols, kSegColsMax));
            if (cascade) {
                cas[type].add(pr.cas_state_off[0], pr.n1);
                cas[type].add(pr.cas_state_off[1], pr.n2);
            } else {
                CHECK(pr.block_start == blocks[type]);
                blocks[type] += (int64_t)pr.nrb * pr.nseg;
                rowparts.add(pr.rowpart_off, (int64_t)pr.nseg * pr.nrb * kRowsPerBlock);
                colparts.add(pr.colpart_off, (int64_t)pr.nrb * pr.n2stride);
            }
            if (type == 0 && !cascade && !empty) {
                rs_bucket.add(pr.rs_bucket_off, rescore_buckets(pr.nrb_main, pr.n2));
                rs_item.add(pr.rs_item_off, rescore_items(pr.nrb_main, pr.n2));
            }
            for (int side = 0; side < 2 && pr.sp; ++side) {
                const int ns = side == 0 ? pr.nsA : pr.nsB, no = side == 0 ? pr.n2 : pr.n1;
                if (ns == 0) { CHECK(pr.sp_wide[side] == 0); continue; }
                const int units = (int)cdiv(ns, 32);
                CHECK(pr.sp_wide[side] == (units > kSpSlots ? 1 : 0));
                const int nchunk = (int)cdiv(no, units > kSpSlots ? kSpWideChunk : kSpChunk);
                sp_row.add(pr.sp_row_off[side], (int64_t)nchunk * up(ns, 32));
                sp_col.add(pr.sp_col_off[side], up(no, 32));
                sp_sides[{i, side}] = Side{side == 0 ? pairs[p].view_2 : pairs[p].view_1, ns, no, nchunk, units, std::vector<int>(nchunk, 0)};
            }
            // totals, launch flags, statistics
            queries += pr.n1 + pr.n2;
            max_n[type] = std::max(max_n[type], std::max(pr.n1, pr.n2));
            if (limited) needs_mask[type] = true;
            if (!empty && pr.n_special > 0) any_special[type] = true;
            if (!empty && !limited) (pr.c0 ? any_c0 : any_corr)[type] = true;
            if (!empty) {
                const int dim = type == 0 ? 128 : 64;
                macs += (int64_t)pr.n1 * pr.n2 * dim;
                if (type == 1) macs_surf += (int64_t)pr.n1 * pr.n2 * dim;
                alg_bytes += (int64_t)(pr.n1 + pr.n2) * (dim + 4);
            }
        }
    }
    for (int type = 0; type < 2; ++type) {
        CHECK(next_prob[type] == bp.probs[type].size());
        CHECK(bp.m12_off[type].size() == bp.probs[type].size() && bp.m21_off[type].size() == bp.probs[type].size());
        CHECK(bp.mark_off[type].size() == 2 * bp.probs[type].size());
        CHECK(bp.total_blocks[type] == blocks[type] && bp.max_n[type] == max_n[type]);
        CHECK(bp.needs_mask[type] == needs_mask[type] && bp.any_special[type] == any_special[type]);
        CHECK(bp.any_c0[type] == any_c0[type] && bp.any_corrected[type] == any_corr[type]);
        cas[type].check(bp.cas_queries[type]);
    }
    pair_out.check(bp.out_ints);
    out.check(bp.out_ints);
    rowparts.check(bp.rowpart_recs);
    colparts.check(bp.colpart_recs);
    keep.check(bp.keep_bytes);
    sp_row.check(bp.sp_recs);
    sp_col.check(bp.sp_cols);
    rs_bucket.check(bp.rs_buckets);
    rs_item.check(bp.rs_items);
    CHECK(bp.total_queries == queries && bp.macs == macs && bp.macs_surf == macs_surf && bp.alg_bytes == alg_bytes);
    CHECK(bp.bucketed == (bp.rs_buckets > 0 && !c.knobs.rescan_wave));       // (no case is near the 2^31 / 2^26 limits)

    // jobs of match_special_kernel and of its wide form
    const int nprob0 = (int)bp.probs[0].size();
    for (const SpecialJob &j : bp.spjobs_wide) {
        CHECK(j.count == 0 && j.problem[0] >= 0 && j.problem[0] < nprob0 && (j.side[0] == 0 || j.side[0] == 1));
        auto it = sp_sides.find({j.problem[0], j.side[0]});
        CHECK(it != sp_sides.end() && it->second.units > kSpSlots);
        CHECK(j.chunk >= 0 && j.chunk < it->second.nchunk);
        it->second.seen[j.chunk]++;
    }
    for (const SpecialJob &j : bp.spjobs) {
        CHECK(j.count >= 0 && j.count <= kSpSlots);
        const int entries = j.count == 0 ? 1 : j.count;
        int view = -1;
        for (int e = 0; e < entries; ++e) {
            CHECK(j.problem[e] >= 0 && j.problem[e] < nprob0 && (j.side[e] == 0 || j.side[e] == 1));
            auto it = sp_sides.find({j.problem[e], j.side[e]});
            CHECK(it != sp_sides.end());
            Side &sd = it->second;
            CHECK(sd.units <= kSpSlots);
            if (j.count > 0) CHECK(sd.units == 1); else CHECK(sd.units > 1);
            if (e == 0) view = sd.view; else CHECK(sd.view == view);      // a shared job streams one view
            CHECK(j.chunk >= 0 && j.chunk < sd.nchunk);
            sd.seen[j.chunk]++;
        }
    }
    for (const auto &kv : sp_sides)
        for (int n : kv.second.seen) CHECK(n == 1);
}

static void set_view(ViewData &v, int ns, int nu, int n_special, int norm2 = 1000)
{
    v.set = true;
    v.ns = ns; v.nu = nu;
    v.ns_pad = (int)up(std::max(ns, 1), kRowsPerBlock); v.nu_pad = (int)up(std::max(nu, 1), kRowsPerBlock);
    v.n_special = n_special; v.surf_norm2_max = norm2;
}

static std::vector<Case> modes(int special_max)
{
    std::vector<Case> cs;
    Case base;
    osfm_match_options &o = base.opts;
    o = osfm_match_options();
    o.matcher_type = OSFM_MATCHER_EXHAUSTIVE;
    base.special_max = special_max;
    cs.push_back(base);                                                                  // full
    for (int lowres = 0; lowres < 2; ++lowres) {
        Case c = base; c.mode.limit = 500; c.mode.lowres = lowres; c.mode.apply = !lowres; cs.push_back(c);
    }
    { Case c = base; c.mode.apply = false; cs.push_back(c); }
    for (int mask = 1; mask <= 2; ++mask) {                                              // (3 is the default)
        Case c = base; c.mode.type_mask = mask; cs.push_back(c);
        c.mode.limit = 500; c.mode.apply = false; cs.push_back(c);                       // the twoway entry
    }
    for (int keep = 0; keep < 2; ++keep) {
        Case c = base; c.opts.matcher_type = OSFM_MATCHER_CASCADE_HASHING; c.opts.cascade_keep_empty_blocks = keep; cs.push_back(c);
        c.mode.limit = 500; c.mode.lowres = true; c.mode.apply = false; cs.push_back(c);   // limited: exhaustive in this mode too
    }
    { Case c = base; c.knobs.rescan_wave = true; cs.push_back(c); }
    return cs;
}

static void check_batches()
{
    const int sizes[] = {0, 1, 255, 256, 257, 1023, 1024, 1025, 8192, 8193};
    for (int special_max : {512, 40}) {
        const int specials[] = {0, 1, 32, 33, 64, 65, special_max, special_max + 1};
        // a view per SIFT size and number of special rows -- every count at two sizes (one of them past a segment), none
        // and one at the others --; its SURF part has another of the sizes
        std::vector<std::pair<int, int>> shape;
        for (int i = 0; i < 10; ++i)
            for (int k = 0; k < 8; ++k) {
                const bool every = special_max == 512 ? (sizes[i] == 1025 || sizes[i] == 8193) : (sizes[i] == 257 || sizes[i] == 1025);
                if (special_max != 512 && !every && sizes[i] != 0) continue;
                if (specials[k] <= sizes[i] && (every || k < 2)) shape.push_back({i, specials[k]});
            }
        std::vector<ViewData> views(shape.size());
        for (size_t v = 0; v < shape.size(); ++v)
            set_view(views[v], sizes[shape[v].first], sizes[(shape[v].first + 3 + v) % 10], shape[v].second);
        std::vector<osfm_pair> all;
        for (int a = 0; a < (int)views.size(); ++a)
            for (int b = 0; b < (int)views.size(); ++b) all.push_back({a, b});     // (a, a) included
        for (const Case &c0 : modes(special_max)) {
            // one pair: a small rb_estimate, many short segments
            g_case = "one pair";
            for (const osfm_pair &pr : all) check_plan(views, c0, {pr});
            // all pairs: rb_estimate >= 2048, one segment per row block; and the forced segment lengths
            for (int tiles : {0, 16, 512}) {
                g_case = tiles == 0 ? "all pairs" : tiles == 16 ? "all pairs, OSFM_SEG_TILES=16" : "all pairs, OSFM_SEG_TILES=512";
                Case c = c0;
                c.knobs.seg_tiles = tiles;
                check_plan(views, c, all);
                check_plan(views, c, {all[all.size() / 2], all[all.size() / 2]});      // the same pair twice
            }
        }
        if (special_max != 512) continue;
        g_case = "rb_estimate";
        int64_t rb = 0;
        for (const osfm_pair &pr : all) rb += cdiv(std::max(views[pr.view_1].ns, views[pr.view_1].nu), kRowsPerBlock);
        CHECK(rb >= 2048);
    }
}

static void check_surf_norms()
{
    g_case = "surf norms";
    const int norms[] = {0, 32766, 32767, 32768, 1 << 20, 0x7fffffff};
    std::vector<ViewData> views(6);
    for (int v = 0; v < 6; ++v) set_view(views[v], 10, 300, 0, norms[v]);
    std::vector<osfm_pair> all;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) all.push_back({a, b});
    // 32767 * 32767 is the last product of the fast path, 32767 * 32768 the first beyond it (check_plan compares)
    check_plan(views, modes(512)[0], all);
}

static void check_view_errors()
{
    g_case = "view errors";
    std::vector<ViewData> views(2);
    set_view(views[0], 10, 10, 0);
    BatchPlan bp;
    const Case c = modes(512)[0];
    const osfm_pair unset = {0, 1}, range = {0, 2}, neg = {-1, 0};
    CHECK(plan_batch(views, c.opts, 512, c.knobs, &unset, 1, c.mode, &bp) == OSFM_E_STATE);
    CHECK(plan_batch(views, c.opts, 512, c.knobs, &range, 1, c.mode, &bp) == OSFM_E_ARG);
    CHECK(plan_batch(views, c.opts, 512, c.knobs, &neg, 1, c.mode, &bp) == OSFM_E_ARG);
    CHECK(plan_batch(views, c.opts, 512, c.knobs, nullptr, 0, c.mode, &bp) == OSFM_OK && bp.out_ints == 0 && bp.plans.empty());
    g_cases += 4;
}

// The parts of a call's full matching.  full_batch_size is the even share of its number of parts, rounded up: dealt
// evenly the parts differ by at most one pair.  (The chunk loop of match_all_single takes full parts first, so its last
// part is the one that is short: 3898 pairs run as 1300 + 1300 + 1298.)
static void check_batch_sizes()
{
    g_case = "batch sizes";
    for (int big : {300, 3000, 20000, 100000}) {
        std::vector<ViewData> views(3);
        set_view(views[0], big, 50, 0); set_view(views[1], 10, big / 2, 0); set_view(views[2], 0, 0, 0);
        for (int variant = 0; variant < 4; ++variant) {
            osfm_match_options o = osfm_match_options();
            o.geometric_verification = variant == 1;
            o.matcher_type = variant == 2 ? OSFM_MATCHER_CASCADE_HASHING : OSFM_MATCHER_EXHAUSTIVE;
            o.pairs_per_batch = variant == 3 ? 100 : 0;
            const int cap = batch_size_for(views, o, false);
            CHECK(cap >= 1 && cap <= 4096);
            CHECK(batch_size_for(views, o, true) == (variant == 3 ? 100 : 16384));
            if (variant == 3) CHECK(cap == 100);
            for (size_t n = 1; n <= 20000; n += (n < 1200 ? 1 : 37)) {
                const int bs = full_batch_size(views, o, n);
                ++g_cases;
                CHECK(bs >= 1 && bs <= cap);
                if (variant == 3) { CHECK(bs == 100); continue; }
                const size_t parts = cdiv(n, bs);
                if (parts > 1) CHECK((size_t)bs == (size_t)cdiv(n, parts));       // the even share: parts of bs or bs - 1 pairs
                else CHECK(n <= (size_t)cap);
                // a large call overlaps the copies of one part with the matching of the next
                if (variant == 0 && n >= 768) CHECK(parts >= 3);
            }
        }
    }
}

static void check_deal()
{
    g_case = "deal";
    std::vector<ViewData> views(40);
    for (int v = 0; v < 40; ++v) set_view(views[v], 100 + 977 * v % 3000, 13 * v % 700, 0);
    std::vector<osfm_pair> pairs;
    for (int a = 1; a < 40; ++a)
        for (int b = 0; b < a; ++b) pairs.push_back({a, b});
    for (int uniform = 0; uniform < 2; ++uniform) {
        if (uniform) for (int v = 0; v < 40; ++v) set_view(views[v], 500, 200, 0);
        for (int shards : {1, 2, 3, 8}) {
            for (int stride : {1, 3, 7}) {
                ++g_cases;
                std::vector<int> cand;
                for (int p = stride - 1; p < (int)pairs.size(); p += stride) cand.push_back(p);
                std::vector<std::vector<int>> owner;
                deal_pairs_lpt(views, shards, pairs.data(), cand, &owner);
                CHECK((int)owner.size() == shards);
                std::vector<int> got;
                std::vector<int64_t> load(shards, 0);
                int64_t heaviest = 0;
                for (int k = 0; k < shards; ++k) {
                    CHECK(std::is_sorted(owner[k].begin(), owner[k].end()));
                    for (int p : owner[k]) {
                        const ViewData &a = views[pairs[p].view_1], &b = views[pairs[p].view_2];
                        const int64_t w = (int64_t)(a.ns + a.nu) * (b.ns + b.nu);
                        load[k] += w; heaviest = std::max(heaviest, w);
                        got.push_back(p);
                    }
                }
                std::sort(got.begin(), got.end());
                CHECK(got == cand);                                               // every candidate, once
                // longest first to the least loaded shard: no two loads further apart than one pair's work
                CHECK(*std::max_element(load.begin(), load.end()) - *std::min_element(load.begin(), load.end()) <= heaviest);
                if (uniform)
                    for (size_t i = 0; i < cand.size(); ++i)
                        CHECK(std::find(owner[i % shards].begin(), owner[i % shards].end(), cand[i]) != owner[i % shards].end());
            }
        }
    }
}

int main()
{
    check_batches();
    check_surf_norms();
    check_view_errors();
    check_batch_sizes();
    check_deal();
    printf("ok %ld cases\n", g_cases);
    return 0;
}
