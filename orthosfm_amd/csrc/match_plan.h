// The pure host decisions of the matcher: what a batch of pairs is cut into (kernel forms, segment lengths, every
// offset into the shared scratch arrays, the jobs of match_special_kernel), how a call is cut into batches and dealt
// over shards, the accept / reject tables.  Plain C++: no HIP call, no kernel, no getenv.
#pragma once
#include <cstdint>
#include <vector>

#include "match_kernels.h"
#include "osfm_common.h"

namespace osfm {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct ViewData {
    bool set = false;
    int ns = 0, nu = 0;
    int ns_pad = 0, nu_pad = 0;
    DeviceBuffer sift, sift_corr, surf, surf_corr;
    // raw form of the SIFT rows (rows with a value > 127 blanked) and the
    // gathered "special" rows that need the value-128 form on the row side
    DeviceBuffer sift_raw, sift_raw_corr, special, special_corr, special_map, special_slot;
    int n_special = 0;
    int surf_norm2_max = 0;
    // cascade hashing data per descriptor type (0: SIFT, 1: SURF), see cashash_kernels.h
    DeviceBuffer cas_hash[2], cas_bucket[2], cas_start[2], cas_items[2], cas_rec[2];
    DeviceBuffer positions;      // [ns + nu][2] floats (geometric verification only)
    int n_positions = -1;
    // recorded on the upload stream behind the view's transfer and conversion kernels; the matching
    // stream waits for it before a batch that names the view (uploads do not wait for matching and
    // matching does not wait for uploads of views it does not use)
    hipEvent_t ready = nullptr;
    ~ViewData() { event_destroy(ready); }
    ViewData() = default;
    ViewData(const ViewData &) = delete;
    ViewData &operator=(const ViewData &) = delete;
};

struct PairPlan {
    int v1, v2;
    int ns1, nu1, ns2, nu2;      // (possibly low-res limited) sizes used
    bool has_sift, has_surf;     // problems generated
    int64_t off12, off21;        // into the combined output buffer (ints)
    int len12, len21;
    int prob_index[2];           // index into the per-type problem list or -1
};

struct BatchResult {
    std::vector<PairPlan> plans;
    std::vector<int32_t> counts;     // mutual matches per pair (sift + surf)
    int64_t out_ints = 0;
};

// One batch of pairs through the device pipeline.
//   limit > 0 : pairwise_match_lowres semantics (SIFT if view_1 has
//               SIFT, else SURF; first `limit` descriptors; count only)
//   limit == 0: pairwise_match semantics (both types, cross-check
//               applied, combined lists left in the matcher's output buffer)
struct BatchMode {
    int limit = 0;            // > 0: only the first `limit` descriptors of each view
    bool lowres = false;      // pairwise_match_lowres: SIFT if view_1 has SIFT, else SURF
    bool apply = true;        // remove_inconsistent_matches + combine offsets
    int type_mask = 3;        // bit 0: SIFT, bit 1: SURF
    int expect = 0;           // pairs of the largest batch to come (osfm_match_expect_pairs): the work arrays are sized for it
};

// CascadeHashing overrides pairwise_match only (cascade_hashing.h:49-56): limited
// (low-res / num_features) matching stays exhaustive
inline bool cascade_batch(const osfm_match_options &opts, const BatchMode &mode)
{
    return opts.matcher_type == OSFM_MATCHER_CASCADE_HASHING && mode.limit == 0;
}

// The environment knobs that reach the plan; the caller reads them.
struct PlanKnobs {
    int seg_tiles = 0;            // OSFM_SEG_TILES > 0: tiles per segment of the correction-free problems (measurements)
    bool rescan_wave = false;     // OSFM_FINISH_RESCAN=wave: every refinement of the finish through its per-query rescan
};

// Everything run_batch decides before it touches the device.  probs[type][i].m12 / m21 are null: the lists of
// problem i of a type start at m12_off[type][i] / m21_off[type][i] ints into the combined output buffer.
struct BatchPlan {
    std::vector<PairPlan> plans;
    std::vector<MatchProblem> probs[2];
    std::vector<int64_t> m12_off[2], m21_off[2];
    std::vector<int64_t> mark_off[2];          // per problem: first keep byte of its rows, of its columns
    std::vector<SpecialJob> spjobs, spjobs_wide;
    int64_t out_ints = 0, rowpart_recs = 0, colpart_recs = 0, keep_bytes = 0, total_queries = 0;
    int64_t sp_recs = 0, sp_cols = 0;
    int64_t rs_buckets = 0, rs_items = 0;      // bucketed rescoring (SIFT problems of the tile path)
    int64_t cas_queries[2] = {0, 0};
    int total_blocks[2] = {0, 0}, max_n[2] = {0, 0};
    bool needs_mask[2] = {false, false};       // some problem is limited below its view size
    bool any_special[2] = {false, false};      // some problem has gathered special rows
    bool any_c0[2] = {false, false}, any_corrected[2] = {false, false};
    bool bucketed = false, cascade = false;
    int64_t macs = 0, macs_surf = 0, alg_bytes = 0;
    void clear();      // an empty plan that keeps the memory of its vectors (a matcher plans batch after batch into one)
};

// OSFM_E_ARG / OSFM_E_STATE (with the error text) for a view id out of range / a view that has not been set.
int check_view(const std::vector<ViewData> &views, int v, const char *what);

int plan_batch(const std::vector<ViewData> &views, const osfm_match_options &opts, int special_max, const PlanKnobs &knobs,
    const osfm_pair *pairs, int num_pairs, const BatchMode &mode, BatchPlan *out);

// Pairs per batch of osfm_match_all, and the (equal) parts a call's full matching is cut into.
int batch_size_for(const std::vector<ViewData> &views, const osfm_match_options &o, bool lowres);
int full_batch_size(const std::vector<ViewData> &views, const osfm_match_options &o, size_t n_full);

// The post-work of a call's last part (finish, rescore, exact scan, cross-check, count read-back) is issued per
// slice of its pairs, so that a slice's lists leave the device while the next slice is finished.
// requested <= 0: default_post_slices(pairs).  bounds: the slices are the pairs [bounds[k], bounds[k + 1]);
// at most min(pairs, kMaxPostSlices) of them, none empty.  Returns their number (0 for no pairs).
constexpr int kMaxPostSlices = 64;
int default_post_slices(int pairs);
int post_slice_bounds(int pairs, int requested, std::vector<int> *bounds);

// One device block per batch for everything that is zeroed before the batch runs, cleared by one memset; its
// first read_bytes (the exact-scan counters of every slice and type, the clock probe, the counts of both types)
// come back in one copy.  The rescore bucket counts lie behind them.
struct ControlLayout {
    size_t exact_off = 0;          // int32[2][kMaxPostSlices]: exact-scan items of (type, slice)
    size_t probe_off = 0;          // unsigned long long[2]
    size_t counts_off[2] = {0, 0}; // int32[problems of the type]
    size_t read_bytes = 0;
    size_t rs_off = 0;             // int32[rs_buckets]
    size_t bytes = 0;
};
ControlLayout control_layout(size_t np_sift, size_t np_surf, int64_t rs_buckets);

// One block for everything a batch uploads (staged page-locked on the host, one copy): the problems and the
// mark offsets of both types, the jobs of the two special kernels.
struct StagingLayout {
    size_t probs_off[2] = {0, 0};  // MatchProblem[problems of the type]
    size_t mark_off[2] = {0, 0};   // int64[2 * problems of the type]
    size_t sp_off = 0;             // SpecialJob[spjobs], then SpecialJob[spjobs_wide] back to back
    size_t bytes = 0;
};
StagingLayout staging_layout(size_t np_sift, size_t np_surf, size_t spjobs, size_t spjobs_wide);

// The four per-pair arrays of the list compaction in one block.
struct CompactLayout {
    size_t m12_off = 0, corr_off = 0;      // int64[n]
    size_t len12_off = 0;                  // int32[n]
    size_t keep_off = 0;                   // uint8[n]
    size_t bytes = 0;
};
CompactLayout compact_layout(size_t n);

void deal_pairs_lpt(const std::vector<ViewData> &views, int num_shards, const osfm_pair *pairs, const std::vector<int> &cand,
    std::vector<std::vector<int>> *owner);

void build_lowe_table(float lowe, bool is_signed, std::vector<int32_t> *tab);
int max_d1_for(float dist_thres, bool is_signed);

}  // namespace osfm
