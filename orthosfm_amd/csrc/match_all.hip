// osfm_match_all on one device: classification, the low-res gate, full matching in chunks, the ordered
// correspondence lists and (optionally) RANSAC-F on them.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "match_internal.h"
#include "ransac_kernels.h"
#include "ransac_affine.h"

namespace osfm {

namespace {

// OSFM_MATCH_TRACE: the time since the chunk began, at the steps of a chunk
struct Lap {
    std::chrono::steady_clock::time_point t_chunk = std::chrono::steady_clock::now();
    void operator()(const char *what) const
    {
        static const bool trace = getenv("OSFM_MATCH_TRACE") != nullptr;
        if (trace) fprintf(stderr, "[osfm match] %-18s %9.3f ms\n", what,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_chunk).count());
    }
};

// What the host decides about the pairs of one chunk (entry k: pair full_idx[start + k]).
struct ChunkLists {
    std::vector<int64_t> m12_off, corr_off;     // a kept pair's m12 list in m->out; its correspondences in the chunk's list
    std::vector<int32_t> len12;
    std::vector<uint8_t> keep;
};

// The kept pairs' mutual matches of a chunk of n pairs, as chunk_corr (id 1, id 2) records back to back on the
// device; without verification they go on to corr + 2 * written on the copy stream.  cs: the stream the compaction
// runs on -- the main stream, or the copy stream itself for a slice whose counts the host has waited for.
int compact_chunk(osfm_matcher *m, const ChunkLists &h, int n, int64_t chunk_corr, int32_t *corr, int64_t written, int *chunk_no,
    hipStream_t cs)
{
    const osfm_match_options &o = m->opts;
    // without verification two list buffers alternate: the copy of the one is in flight on the
    // copy stream while the next chunk is matched and compacted into the other
    const int cb = o.geometric_verification ? 0 : ((*chunk_no)++ & 1);
    DeviceBuffer &dcorr = cb ? m->d_corr_alt : m->d_corr;
    // before a reserve may free it -- and before the host block of this list buffer, whose upload lies in front of
    // that copy, is refilled (with verification the chunk before this one has ended with a wait for the stream)
    if (m->copied_used[cb]) OSFM_HIP_CHECK(hipEventSynchronize(m->ev_copied[cb]));
    OSFM_RETURN_IF(dcorr.reserve((size_t)chunk_corr * 8));
    const CompactLayout cl = compact_layout((size_t)n);
    OSFM_RETURN_IF(m->d_compact[cb].reserve(cl.bytes));
    OSFM_RETURN_IF(m->h_compact[cb].reserve(cl.bytes));
    char *hp = m->h_compact[cb].ptr, *dp = m->d_compact[cb].as<char>();
    memcpy(hp + cl.m12_off, h.m12_off.data(), (size_t)n * 8);
    memcpy(hp + cl.corr_off, h.corr_off.data(), (size_t)n * 8);
    memcpy(hp + cl.len12_off, h.len12.data(), (size_t)n * 4);
    memcpy(hp + cl.keep_off, h.keep.data(), (size_t)n);
    OSFM_HIP_CHECK(hipMemcpyAsync(dp, hp, cl.bytes, hipMemcpyHostToDevice, cs));
    launch_compact_pairs(n, m->out.as<int32_t>(), reinterpret_cast<const int64_t *>(dp + cl.m12_off),
        reinterpret_cast<const int32_t *>(dp + cl.len12_off), reinterpret_cast<const int64_t *>(dp + cl.corr_off),
        reinterpret_cast<const uint8_t *>(dp + cl.keep_off), dcorr.as<int32_t>(), cs);
    OSFM_HIP_CHECK(hipGetLastError());
    if (!o.geometric_verification) {
        if (cs != m->copy_stream) {
            OSFM_HIP_CHECK(hipEventRecord(m->ev_compact[cb], cs));
            OSFM_HIP_CHECK(hipStreamWaitEvent(m->copy_stream, m->ev_compact[cb], 0));
        }
        OSFM_HIP_CHECK(hipMemcpyAsync(corr + 2 * written, dcorr.ptr, (size_t)chunk_corr * 8,
            hipMemcpyDeviceToHost, m->copy_stream));
        OSFM_HIP_CHECK(hipEventRecord(m->ev_copied[cb], m->copy_stream));
        m->copied_used[cb] = true;
    }
    return OSFM_OK;
}

// RANSAC-F (or, with ransac_model OSFM_RANSAC_AFFINE, the affine RANSAC of ransac_affine.hip) on the device-resident
// lists of a chunk (bundler_matching.cc:194-219): entry k of the chunk is pair
// idx[k] with counts[k] correspondences.  Pairs with enough inliers keep them, at corr + 2 * *written_out on.
int verify_chunk(osfm_matcher *m, const osfm_pair *pairs, const int *idx, int n, const std::vector<int32_t> &counts,
    const ChunkLists &h, int64_t chunk_corr, osfm_pair_result *results, int32_t *corr, int64_t capacity,
    int64_t *written_out, bool *overflow, const Lap &lap)
{
    const osfm_match_options &o = m->opts;
    hipStream_t s = m->stream;
    std::vector<RansacJob> jobs;
    std::vector<int> job_pair;
    OSFM_RETURN_IF(m->d_inl.reserve((size_t)chunk_corr * 4));
    OSFM_RETURN_IF(m->d_inl_count.reserve((size_t)n * 4));
    for (int k = 0; k < n; ++k) {
        if (!h.keep[k]) continue;
        const int p = idx[k];
        const ViewData &a = m->views[pairs[p].view_1], &b = m->views[pairs[p].view_2];
        if (a.n_positions < 0 || b.n_positions < 0) {
            set_error("match_all: geometric verification needs osfm_match_set_positions for views %d and %d",
                pairs[p].view_1, pairs[p].view_2);
            return OSFM_E_STATE;
        }
        RansacJob j;
        memset(&j, 0, sizeof(j));
        j.pos1 = a.positions.as<float>(); j.pos2 = b.positions.as<float>();
        j.corr = m->d_corr.as<int32_t>() + 2 * h.corr_off[k];
        j.k = counts[k];
        // stream id = linear index of the pair in the reference's enumeration
        const int64_t hi = std::max(pairs[p].view_1, pairs[p].view_2), lo = std::min(pairs[p].view_1, pairs[p].view_2);
        j.pair_id = (uint64_t)(hi * (hi - 1) / 2 + lo);
        j.inliers_out = m->d_inl.as<int32_t>() + h.corr_off[k];
        j.count_out = m->d_inl_count.as<int32_t>() + (int)jobs.size();
        j.F_out = nullptr;
        jobs.push_back(j); job_pair.push_back(k);
    }
    const size_t jobs_bytes = (jobs.size() * sizeof(RansacJob) + 255) / 256 * 256;
    const bool affine = o.ransac_model == OSFM_RANSAC_AFFINE;
    OSFM_RETURN_IF(m->d_jobs.reserve(jobs_bytes + (affine ? affine_scratch_bytes((int)jobs.size()) : ransac_scratch_bytes((int)jobs.size()))));
    OSFM_HIP_CHECK(hipMemcpyAsync(m->d_jobs.ptr, jobs.data(), jobs.size() * sizeof(RansacJob), hipMemcpyHostToDevice, s));
    if (affine)
        launch_ransac_affine(m->d_jobs.as<RansacJob>(), (int)jobs.size(), o.ransac_max_iterations, o.ransac_threshold,
            o.ransac_refit, o.ransac_seed, static_cast<char *>(m->d_jobs.ptr) + jobs_bytes, nullptr, s);
    else
        launch_ransac(m->d_jobs.as<RansacJob>(), (int)jobs.size(), o.ransac_max_iterations, o.ransac_threshold,
            o.ransac_seed, static_cast<char *>(m->d_jobs.ptr) + jobs_bytes, s);
    OSFM_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> h_cnt(jobs.size());
    OSFM_HIP_CHECK(hipMemcpyAsync(h_cnt.data(), m->d_inl_count.ptr, jobs.size() * 4, hipMemcpyDeviceToHost, s));
    lap("ransac queued");
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    lap("ransac done");
    // keep pairs with enough inliers; gather their inlier correspondences
    const int min_inl = std::max(8, o.min_matching_inliers);
    std::vector<int64_t> g_src, g_dst;     // per job: source offset (corr / inlier ids), destination
    std::vector<int32_t> g_cnt;
    int64_t chunk_out = 0;
    for (size_t jx = 0; jx < jobs.size(); ++jx) {
        const int k = job_pair[jx];
        osfm_pair_result &r = results[idx[k]];
        r.num_inliers = h_cnt[jx];
        if (h_cnt[jx] < min_inl) { r.status = OSFM_PAIR_REJECTED_INLIERS; r.offset = 0; continue; }
        r.offset = *written_out + chunk_out;
        g_src.push_back(h.corr_off[k]); g_dst.push_back(chunk_out); g_cnt.push_back(h_cnt[jx]);
        chunk_out += h_cnt[jx];
    }
    if (*written_out + chunk_out > capacity) *overflow = true;
    if (!*overflow && chunk_out > 0) {
        const int ng = (int)g_cnt.size();
        OSFM_RETURN_IF(m->d_gather_off.reserve((size_t)ng * 20));
        OSFM_RETURN_IF(m->d_corr2.reserve((size_t)chunk_out * 8));
        char *gb = m->d_gather_off.as<char>();
        OSFM_HIP_CHECK(hipMemcpyAsync(gb, g_src.data(), (size_t)ng * 8, hipMemcpyHostToDevice, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(gb + (size_t)ng * 8, g_dst.data(), (size_t)ng * 8, hipMemcpyHostToDevice, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(gb + (size_t)ng * 16, g_cnt.data(), (size_t)ng * 4, hipMemcpyHostToDevice, s));
        launch_gather_inliers(ng, m->d_corr.as<int32_t>(), m->d_inl.as<int32_t>(),
            reinterpret_cast<const int64_t *>(gb), reinterpret_cast<const int64_t *>(gb + (size_t)ng * 8),
            reinterpret_cast<const int32_t *>(gb + (size_t)ng * 16), m->d_corr2.as<int32_t>(), s);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipMemcpyAsync(corr + 2 * *written_out, m->d_corr2.ptr, (size_t)chunk_out * 8,
            hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        lap("lists on the host");
    }
    *written_out += chunk_out;
    return OSFM_OK;
}

}  // namespace

// bundler::Matching::compute on one device.  phase: kPhaseBoth -- the whole of it; kPhaseGate -- classification and
// the low-res gate only (a pair that goes on to full matching is left at OSFM_PAIR_MATCHED with its lowres_matches);
// kPhaseFull -- full matching (and RANSAC-F) of the pairs whose result arrives as OSFM_PAIR_MATCHED, everything else
// is left as it is.  The multi-device front runs the two halves as two rounds with a deal of their own each.
int match_all_single(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, osfm_pair_result *results,
    int32_t *corr, int64_t capacity, int64_t *total, int phase)
{
    std::lock_guard<std::mutex> lock(m->mu);
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    if (phase != kPhaseFull) reset_stats(m);
    const osfm_match_options &o = m->opts;
    // whatever way this call ends, no copy into the caller's buffer is still in flight afterwards
    struct CopyDrain { hipStream_t s; ~CopyDrain() { if (s) (void)hipStreamSynchronize(s); } } copy_drain{m->copy_stream};

    // ---- classify (bundler_matching.cc:96-99, 146-158) ---------------------
    std::vector<int> lowres_idx, full_idx;
    for (int p = 0; p < num_pairs; ++p) {
        OSFM_RETURN_IF(check_view(m, pairs[p].view_1, "match_all"));
        OSFM_RETURN_IF(check_view(m, pairs[p].view_2, "match_all"));
        const ViewData &a = m->views[pairs[p].view_1], &b = m->views[pairs[p].view_2];
        osfm_pair_result &r = results[p];
        if (phase == kPhaseFull) {
            if (r.status == OSFM_PAIR_MATCHED) full_idx.push_back(p);
            continue;
        }
        r.status = OSFM_PAIR_MATCHED; r.lowres_matches = -1; r.num_matches = 0; r.num_inliers = -1; r.offset = 0;
        const size_t np1 = (size_t)a.ns + a.nu, np2 = (size_t)b.ns + b.nu;
        if (np1 == 0 || np2 == 0) { r.status = OSFM_PAIR_SKIPPED_EMPTY; continue; }
        if (o.use_lowres_matching && np1 * np2 > 1000000) lowres_idx.push_back(p);
        else full_idx.push_back(p);
    }

    // ---- low-res gate -------------------------------------------------------
    {
        const int bs = batch_size_for(m->views, o, true);
        std::vector<osfm_pair> chunk;
        for (size_t start = 0; start < lowres_idx.size(); start += bs) {
            const size_t end = std::min(lowres_idx.size(), start + bs);
            chunk.clear();
            for (size_t k = start; k < end; ++k) chunk.push_back(pairs[lowres_idx[k]]);
            BatchResult res;
            BatchMode mode;
            mode.limit = o.num_lowres_features; mode.lowres = true; mode.apply = false;
            OSFM_RETURN_IF(run_batch(m, chunk.data(), (int)chunk.size(), mode, &res));
            for (size_t k = start; k < end; ++k) {
                const int p = lowres_idx[k];
                results[p].lowres_matches = res.counts[k - start];
                if (res.counts[k - start] < o.min_lowres_matches)
                    results[p].status = OSFM_PAIR_REJECTED_LOWRES;
                else
                    full_idx.push_back(p);
            }
        }
        std::sort(full_idx.begin(), full_idx.end());
    }
    if (phase == kPhaseGate) { if (total) *total = 0; return OSFM_OK; }

    // ---- full matching + ordered correspondence lists -----------------------
    const int min_matches = std::max(8, o.min_feature_matches);
    int64_t written = 0, written_out = 0;     // pre-RANSAC / post-RANSAC correspondence counts
    bool overflow = false;
    {
        const int bs = full_batch_size(m->views, o, full_idx.size());
        const char *slices_env = getenv("OSFM_POST_SLICES");
        const int post_slices_env = slices_env ? atoi(slices_env) : 0;      // 0: default_post_slices of the part
        int chunk_no = 0;
        std::vector<osfm_pair> chunk;
        ChunkLists h;
        for (size_t start = 0; start < full_idx.size(); start += bs) {
            const size_t end = std::min(full_idx.size(), start + bs);
            const int n = (int)(end - start);
            chunk.clear();
            for (size_t k = start; k < end; ++k) chunk.push_back(pairs[full_idx[k]]);
            const Lap lap{};
            // ---- match ----
            BatchResult res;
            BatchMode full_mode;
            // (the largest part of the largest call announced: what the work arrays are sized for from the first call on)
            if (m->expect_pairs > 0)
                full_mode.expect = std::min<int>(full_batch_size(m->views, o, (size_t)m->expect_pairs), m->expect_pairs);
            // ---- keep / reject by count, compact ----
            // of the pairs [k0, k1) of the chunk, whose counts are in res; the compaction on stream cs
            int64_t chunk_corr = 0;
            auto emit = [&](int k0, int k1, hipStream_t cs) -> int {
                const int ns = k1 - k0;
                h.m12_off.assign(ns, 0); h.corr_off.assign(ns, 0); h.len12.assign(ns, 0); h.keep.assign(ns, 0);
                chunk_corr = 0;
                for (int k = k0; k < k1; ++k) {
                    const int p = full_idx[start + k];
                    osfm_pair_result &r = results[p];
                    r.num_matches = res.counts[k];
                    if (res.counts[k] < min_matches) { r.status = OSFM_PAIR_REJECTED_COUNT; continue; }
                    r.status = OSFM_PAIR_MATCHED;
                    r.offset = written + chunk_corr;
                    h.keep[k - k0] = 1;
                    h.m12_off[k - k0] = res.plans[k].off12;
                    h.len12[k - k0] = res.plans[k].len12;
                    h.corr_off[k - k0] = chunk_corr;
                    chunk_corr += res.counts[k];
                }
                if (!o.geometric_verification && written + chunk_corr > capacity) overflow = true;
                // With verification the pre-RANSAC lists are device scratch (d_corr) that the
                // RANSAC jobs of THIS chunk read: they are built whatever the state of the
                // caller's buffer; only the copies to the host stop after an overflow.
                if (chunk_corr > 0 && (o.geometric_verification || !overflow))
                    OSFM_RETURN_IF(compact_chunk(m, h, ns, chunk_corr, corr, written, &chunk_no, cs));
                return OSFM_OK;
            };
            // Nothing is matched behind a call's last part, so its lists would leave the device with nothing else
            // running: its post-work runs in slices (OSFM_POST_SLICES, read per call; 1: one sequence as for every
            // other part), and a slice's lists are compacted and copied on the copy stream while the main stream
            // finishes the next slice.  With verification the RANSAC jobs want the whole chunk's lists: no slices.
            SliceSink sink;
            sink.requested = post_slices_env;
            sink.on_slice = [&](int k0, int k1) -> int {
                OSFM_RETURN_IF(emit(k0, k1, m->copy_stream));
                written += chunk_corr;
                return OSFM_OK;
            };
            const bool last = end == full_idx.size();
            bool sliced = false;
            OSFM_RETURN_IF(run_batch(m, chunk.data(), n, full_mode, &res,
                last && !o.geometric_verification ? &sink : nullptr, &sliced));
            lap("matched");
            if (sliced) continue;
            OSFM_RETURN_IF(emit(0, n, m->stream));
            // ---- verify ----
            if (o.geometric_verification && chunk_corr > 0)
                OSFM_RETURN_IF(verify_chunk(m, pairs, full_idx.data() + start, n, res.counts, h, chunk_corr, results, corr,
                    capacity, &written_out, &overflow, lap));
            written += chunk_corr;
        }
    }
    if (!o.geometric_verification) OSFM_HIP_CHECK(hipStreamSynchronize(m->copy_stream));      // every list has arrived
    if (o.geometric_verification) written = written_out;
    if (total) *total = written;
    if (overflow) {
        set_error("match_all: %lld correspondences need more than the given capacity %lld",
            (long long)written, (long long)capacity);
        return OSFM_E_CAPACITY;
    }
    return OSFM_OK;
}

}  // namespace osfm
