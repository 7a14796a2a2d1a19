// Checks, on the host, the two pure decisions behind a batch's passes over the device (orthosfm_amd/csrc/match_plan.h):
// the slices the post-work of a call's last part is cut into, and the layouts of the blocks a batch zeroes, uploads
// and reads back in one operation each.  Nothing is compared against what the code under test produced: the slices
// must tile the pairs, the fields must lie inside their block, aligned and apart.  Built with AddressSanitizer and
// UBSan (orthosfm_amd/csrc/Makefile); prints "ok <cases> cases" when all held.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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

static char g_case[256] = "";
static long g_cases = 0;
#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            fprintf(stderr, "match_pass_check: %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_case); \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)

struct Field { size_t off, bytes, align; };

// every field inside [0, total), at a multiple of its alignment, and apart from every other
static void check_fields(std::vector<Field> f, size_t total)
{
    for (const Field &x : f) {
        CHECK(x.off % x.align == 0);
        CHECK(x.off <= total && x.bytes <= total - x.off);
    }
    std::sort(f.begin(), f.end(), [](const Field &a, const Field &b) { return a.off < b.off; });
    for (size_t i = 1; i < f.size(); ++i)
        if (f[i].bytes) CHECK(f[i - 1].off + f[i - 1].bytes <= f[i].off);
}

static void check_slices()
{
    for (int pairs = 1; pairs <= 70; ++pairs)
        for (int req = 1; req <= 9; ++req) {
            snprintf(g_case, sizeof(g_case), "slices: %d pairs, %d requested", pairs, req);
            std::vector<int> b;
            const int n = post_slice_bounds(pairs, req, &b);
            CHECK(n >= 1 && n <= req && n <= pairs && n <= kMaxPostSlices);
            CHECK(n == std::min(req, pairs));                 // as many as asked for wherever every slice can have a pair
            CHECK((int)b.size() == n + 1);
            CHECK(b.front() == 0 && b.back() == pairs);
            std::vector<int> hits(pairs, 0);
            for (int k = 0; k < n; ++k) {
                CHECK(b[k] < b[k + 1]);                       // in order, none empty
                for (int p = b[k]; p < b[k + 1]; ++p) hits[p]++;
            }
            for (int p = 0; p < pairs; ++p) CHECK(hits[p] == 1);
            // slices of even size: none more than one pair longer than another
            int lo = pairs, hi = 0;
            for (int k = 0; k < n; ++k) { lo = std::min(lo, b[k + 1] - b[k]); hi = std::max(hi, b[k + 1] - b[k]); }
            CHECK(hi - lo <= 1);
            ++g_cases;
        }
    // the default and the bounds of the knob
    for (int pairs : {1, 2, 95, 96, 408, 4096, 100000}) {
        snprintf(g_case, sizeof(g_case), "slices: %d pairs, default and extremes", pairs);
        std::vector<int> b;
        for (int req : {0, -3}) {
            const int n = post_slice_bounds(pairs, req, &b);
            CHECK(n == std::min(std::max(default_post_slices(pairs), 1), pairs) && (int)b.size() == n + 1 && b.back() == pairs);
        }
        const int n = post_slice_bounds(pairs, 1 << 30, &b);
        CHECK(n == std::min(pairs, (int)kMaxPostSlices) && (int)b.size() == n + 1 && b.front() == 0 && b.back() == pairs);
        for (int k = 0; k < n; ++k) CHECK(b[k] < b[k + 1]);
        ++g_cases;
    }
    std::vector<int> b{1, 2, 3};
    CHECK(post_slice_bounds(0, 3, &b) == 0 && b.empty());
    ++g_cases;
}

static void check_layouts()
{
    for (size_t np : {(size_t)1, (size_t)2, (size_t)407, (size_t)4096})
        for (int with_surf = 0; with_surf < 2; ++with_surf)
            for (int64_t rs : {(int64_t)0, (int64_t)1, (int64_t)924 * (int64_t)np})
                for (size_t nsp : {(size_t)0, (size_t)3})
                    for (size_t nspw : {(size_t)0, (size_t)5}) {
                        const size_t np_surf = with_surf ? np : 0;
                        snprintf(g_case, sizeof(g_case), "layout: %zu sift, %zu surf, %lld buckets, %zu + %zu jobs", np, np_surf,
                            (long long)rs, nsp, nspw);
                        const ControlLayout c = control_layout(np, np_surf, rs);
                        check_fields({{c.exact_off, (size_t)2 * kMaxPostSlices * 4, 16}, {c.probe_off, 16, 16},
                                         {c.counts_off[0], np * 4, 16}, {c.counts_off[1], np_surf * 4, 16},
                                         {c.rs_off, (size_t)rs * 4, 16}},
                            c.bytes);
                        // what comes back: the counters, the probe and the counts, and nothing of the bucket counts
                        for (size_t end : {c.exact_off + (size_t)2 * kMaxPostSlices * 4, c.probe_off + 16, c.counts_off[0] + np * 4,
                                 c.counts_off[1] + np_surf * 4})
                            CHECK(end <= c.read_bytes);
                        CHECK(c.read_bytes <= c.rs_off && c.read_bytes <= c.bytes && c.read_bytes > 0);

                        const StagingLayout s = staging_layout(np, np_surf, nsp, nspw);
                        check_fields({{s.probs_off[0], np * sizeof(MatchProblem), alignof(MatchProblem) < 16 ? 16 : alignof(MatchProblem)},
                                         {s.probs_off[1], np_surf * sizeof(MatchProblem), 16},
                                         {s.mark_off[0], np * 16, 16}, {s.mark_off[1], np_surf * 16, 16},
                                         {s.sp_off, (nsp + nspw) * sizeof(SpecialJob), 16}},
                            s.bytes);
                        CHECK(s.bytes > 0);

                        const CompactLayout k = compact_layout(np);
                        check_fields({{k.m12_off, np * 8, 16}, {k.corr_off, np * 8, 16}, {k.len12_off, np * 4, 16},
                                         {k.keep_off, np, 16}},
                            k.bytes);
                        CHECK(k.bytes > 0);
                        ++g_cases;
                    }
    // a batch without problems still has a block to clear and to copy
    snprintf(g_case, sizeof(g_case), "layout: empty batch");
    CHECK(control_layout(0, 0, 0).bytes > 0 && control_layout(0, 0, 0).read_bytes > 0);
    CHECK(staging_layout(0, 0, 0, 0).bytes > 0 && compact_layout(0).bytes > 0);
    ++g_cases;
}

int main()
{
    check_slices();
    check_layouts();
    printf("ok %ld cases\n", g_cases);
    return 0;
}
