// The matcher's handle and the functions its host files share.  Not part of the C ABI.
//   match_plan.hip   what a batch is cut into (pure host arithmetic)      match_batch.hip  run_batch: one batch on the device
//   match_views.hip  view upload, hand-off, copies, cascade-hash build    match_all.hip    osfm_match_all on one device
//   match_multi.hip  the multi-device front                               match_pair.hip   request combiner of the per-pair entries
//   match_api.hip    set_error and every extern "C" entry               guided_api.hip   osfm_match_guided
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "match_plan.h"

namespace osfm {

// Page-locked host memory that only grows (contents not kept); whoever grows it has waited for the transfer that
// still reads it.  Freed with the matcher.
struct PinnedBlock {
    char *ptr = nullptr;
    size_t bytes = 0;
    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock &) = delete;
    PinnedBlock &operator=(const PinnedBlock &) = delete;
    ~PinnedBlock() { pinned_free(ptr, bytes); }
    int reserve(size_t need)
    {
        if (need <= bytes) return OSFM_OK;
        pinned_free(ptr, bytes);
        ptr = nullptr; bytes = 0;
        const size_t want = need + need / 8 + 256;
        void *p = nullptr;
        OSFM_HIP_CHECK(pinned_alloc(&p, want, hipHostMallocDefault));
        ptr = static_cast<char *>(p); bytes = want;
        return OSFM_OK;
    }
};

// An event without timing, made on first use and destroyed with the matcher.
struct LazyEvent {
    hipEvent_t e = nullptr;
    LazyEvent() = default;
    LazyEvent(const LazyEvent &) = delete;
    LazyEvent &operator=(const LazyEvent &) = delete;
    ~LazyEvent() { event_destroy(e); }
    int make()
    {
        if (!e) OSFM_HIP_CHECK(event_create(&e, false));
        return OSFM_OK;
    }
};

// What run_batch hands out per slice of a batch whose post-work runs in slices (match_plan.h: post_slice_bounds):
// the pairs [p0, p1) of the batch are finished and their counts are in res->counts.  The main stream is busy
// with the later slices meanwhile.
struct SliceSink {
    int requested = 1;          // slices asked for (<= 0: the default for the batch's size)
    std::function<int(int p0, int p1)> on_slice;
};

}  // namespace osfm

struct osfm_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    osfm_match_options opts;
    std::vector<osfm::ViewData> views;
    osfm::DeviceBuffer lowe_sift, lowe_surf;
    osfm::LoweTable tab_sift, tab_surf;
    std::mutex mu;
    // uploads (osfm_match_set_view) have a stream and a lock of their own: a view can be uploaded while a
    // batch that does not name it is being matched
    hipStream_t up_stream = nullptr;
    std::mutex up_mu;

    // scratch (grow-only)
    osfm::DeviceBuffer rowparts, colparts, out, keep;
    osfm::DeviceBuffer exact_items, stage_in, flags;
    osfm::DeviceBuffer rs_items;                // bucketed rescoring of the SIFT finish: the buckets' items
    osfm::DeviceBuffer sp_parts, sp_col;        // match_special_kernel: row results, column results
    // Per batch one upload, one memset, one read-back (match_plan.h: StagingLayout, ControlLayout):
    //   d_batch    problems, mark offsets and special jobs, uploaded in one copy from h_batch.  Every batch ends
    //              with a wait for the stream, so the upload that read h_batch is over before it is refilled (or
    //              regrown); planning a batch while the one before it runs would need a second block or an event.
    //   d_control  every counter the kernels add to, cleared by one memset; its head comes back into h_read in one
    //              copy.  h_read is read by the host behind the wait for that copy and before the next one is queued.
    osfm::DeviceBuffer d_batch, d_control;
    osfm::PinnedBlock h_batch, h_read;
    osfm::LazyEvent ev_slice[osfm::kMaxPostSlices];      // behind the count read-back of a slice
    osfm::BatchPlan plan;                 // run_batch's plan (under mu): its vectors keep their memory from batch to batch
    osfm::DeviceBuffer zero_tile;         // kTileCols blank descriptors: what the correction-free tile loop prefetches past a segment's end
    int special_max = 512;                // views with more special descriptors take the per-view operand forms
    int expect_pairs = 0;                 // osfm_match_expect_pairs: the largest call to come (work arrays sized for it)
    // the four per-pair arrays of the compaction in one block (CompactLayout), uploaded in one copy from the host
    // block of the list buffer the compaction fills: ev_copied of that list buffer lies behind the upload too
    osfm::DeviceBuffer d_compact[2], d_corr;
    osfm::PinnedBlock h_compact[2];
    // osfm_match_all without verification: the lists of chunk k leave the device on a copy stream while
    // chunk k + 1 is matched (two list buffers alternate)
    osfm::DeviceBuffer d_corr_alt;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_compact[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    bool copied_used[2] = {false, false};
    osfm::DeviceBuffer d_jobs, d_inl, d_inl_count, d_corr2, d_gather_off;
    // osfm_match_guided (guided_api.hip): job and result records, seeds, band scalars, one-way results, padded and packed lists
    osfm::DeviceBuffer g_jobs, g_prep, g_seeds, g_u, g_m, g_list, g_out, g_off;
    hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    hipEvent_t ev_sp[2] = {nullptr, nullptr};
    // page-locked staging of the view uploads (two blocks alternate; the event says a block's transfer is done)
    char *pin_ptr[2] = {nullptr, nullptr};
    size_t pin_bytes[2] = {0, 0};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_used[2] = {false, false};
    unsigned pin_next = 0;

    // cascade hashing: projection matrices (transposed), running sums, average; the
    // hashes depend on the average over ALL views, hence the dirty flag
    osfm::DeviceBuffer cas_proj[2], cas_sum[2], cas_avg[2], cas_state;
    std::atomic<bool> cas_dirty{true};

    osfm_match_stats stats;

    // Concurrent callers of the per-pair entries (the reference drives MatchingBase from an
    // OpenMP loop, bundler_matching.cc:86-88) are combined: whoever finds no leader at work
    // takes every request that is waiting, runs them as ONE batch and hands the results out.
    // A pair alone costs 0.26 ms of launch and synchronisation latency for 60 us of GPU work.
    struct Staging { int32_t *ptr = nullptr; size_t ints = 0; int users = 0; };
    struct PairRequest {
        int kind;                       // 0: pairwise_match, 1: pairwise_match_lowres
        int v1, v2, num_features;
        int32_t *m12, *m21, *len12, *len21, *count;
        int status = OSFM_OK;
        bool done = false;
        std::string error;
        // where the leader left this request's lists: in a page-locked staging block that the
        // requester copies from itself (the copies of a batch run in parallel, one per thread)
        Staging *stage = nullptr;
        int64_t src12 = 0, src21 = 0;
        int32_t n12 = 0, n21 = 0;
    };
    std::vector<Staging *> comb_staging;      // guarded by comb_mu; blocks live as long as the matcher

    // Multi-device front (osfm_match_create_multi): no device state of its own, one complete
    // matcher per entry of device_ids (the same device may appear more than once: logical
    // shards).  Every view goes to every shard; osfm_match_all deals its pairs over them.
    std::vector<osfm_matcher *> shards;
    std::vector<Staging> shard_stage;         // page-locked list buffer per shard (grow-only)
    std::atomic<unsigned> next_shard{0};      // per-pair entries: round robin
    std::mutex multi_mu;                      // one osfm_match_all at a time on the front
    std::mutex comb_mu;
    std::condition_variable comb_cv;
    std::deque<PairRequest *> comb_queue;
    bool comb_leader = false;
};

namespace osfm {

// match_batch.hip
int check_view(const osfm_matcher *m, int v, const char *what);
// sink: the post-work of the batch in slices (exhaustive matching only), each handed to sink->on_slice when its
// counts have arrived; without it, or with one slice, the batch is one sequence and on_slice is not called
int run_batch(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, const BatchMode &mode, BatchResult *res,
    const SliceSink *sink = nullptr, bool *sliced = nullptr);
void reset_stats(osfm_matcher *m);

// match_views.hip
int upload_view(osfm_matcher *m, int view, const uint16_t *sift, int n_sift, const int16_t *surf, int n_surf);
int handoff_all(osfm_matcher *m, int view, int device, const float *d_sift, const int32_t *sift_map, int n_sift,
    const float *d_surf, const int32_t *surf_map, int n_surf, const float *d_positions,
    const std::function<int(hipStream_t)> &begin, const std::function<int(hipStream_t)> &end);
int ensure_cashash(osfm_matcher *m);

// match_all.hip
enum { kPhaseBoth = 0, kPhaseGate = 1, kPhaseFull = 2 };
int match_all_single(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, osfm_pair_result *results,
    int32_t *corr, int64_t capacity, int64_t *total, int phase);

// match_multi.hip
int for_each_shard(osfm_matcher *m, const std::function<int(size_t)> &fn);
int multi_match_all(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, osfm_pair_result *results,
    int32_t *corr, int64_t capacity, int64_t *total);

// match_pair.hip
int combine(osfm_matcher *m, osfm_matcher::PairRequest &rq);

}  // namespace osfm
