// ---------------------------------------------------------------------------
// Multi-device front.  The reference's caller is ONE C++ process
// (bundler::Matching::compute, bundler_matching.cc:58-136), so the sharding over the GPUs of
// a node has to live behind the C ABI: one worker thread per shard for the duration of a
// call, every shard a complete single-device matcher holding the full descriptor bank, the
// pairs of osfm_match_all dealt by work (N1 * N2, longest first, to the least loaded shard:
// the rule of orthosfm_amd/distributed.py::deal_pairs), no data-path exchange between
// devices.  Each shard leaves its lists in its own page-locked block; once every count is
// known the offsets follow in pair order and the shard threads copy their lists to their
// places in the caller's buffer -- records and bytes are those of a single-device call.
// ---------------------------------------------------------------------------
#include <algorithm>
#include <cstring>
#include <thread>

#include "match_internal.h"

namespace osfm {

int for_each_shard(osfm_matcher *m, const std::function<int(size_t)> &fn)
{
    const size_t n = m->shards.size();
    std::vector<int> st(n, OSFM_OK);
    std::vector<std::string> msg(n);
    auto run = [&](size_t k) {
        st[k] = fn(k);
        if (st[k] != OSFM_OK) msg[k] = osfm_last_error();      // the error text is per thread
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < n; ++k) th.emplace_back(run, k);
    run(0);
    for (auto &t : th) t.join();
    // a failure is reported once: the first failing shard's status and text
    for (size_t k = 0; k < n; ++k)
        if (st[k] != OSFM_OK) {
            set_error("device %d (shard %zu of %zu): %s", m->shards[k]->device, k, n, msg[k].c_str());
            return st[k];
        }
    return OSFM_OK;
}

// Two rounds, each dealt by what it costs.  The low-res gate (bundler_matching.cc:146-158: 500 x 500 features per
// pair, 1 / 1600 of a full match) goes round robin over ALL pairs; what it lets through -- on real image sets the
// survivors follow the scene, not the pair index: views of another scene reject whole rows of the pair matrix --
// is then dealt longest-first on N1 * N2 for the full matching.  (One deal before the gate balanced the weights
// of pairs of which a structured third was never matched.)  The shard threads live through both rounds and the
// copy of the lists: a barrier between the rounds (the survivors of all shards are dealt together) and one behind
// the counts (a list's place in the caller's buffer follows from the counts of every pair before it).
int multi_match_all(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, osfm_pair_result *results,
    int32_t *corr, int64_t capacity, int64_t *total)
{
    std::lock_guard<std::mutex> lock(m->multi_mu);
    const int n = (int)m->shards.size();
    for (int p = 0; p < num_pairs; ++p) {
        OSFM_RETURN_IF(check_view(m->shards[0], pairs[p].view_1, "match_all"));
        OSFM_RETURN_IF(check_view(m->shards[0], pairs[p].view_2, "match_all"));
    }
    const auto &views = m->shards[0]->views;
    const bool verify = m->opts.geometric_verification != 0;
    std::vector<std::vector<int>> owner(n);                   // round 2: pairs of each shard, ascending
    std::vector<std::vector<osfm_pair>> sub_pairs(n);
    std::vector<std::vector<osfm_pair_result>> sub_res(n);
    std::vector<int64_t> sub_total(n, 0), sub_cap(n, 0);
    std::vector<int> sub_status(n, OSFM_OK);
    std::vector<int64_t> goff(num_pairs, 0);                  // a pair's list inside its shard's block
    int64_t run = 0;
    bool overflow = false;

    // a barrier for the n shard threads; the last one to arrive runs `serial` before anyone leaves
    std::mutex bmu;
    std::condition_variable bcv;
    int waiting = 0, generation = 0;
    bool failed = false;                                      // a shard has failed: the others stop at the next barrier
    auto barrier = [&](bool ok, const std::function<void()> &serial) -> bool {
        std::unique_lock<std::mutex> lk(bmu);
        if (!ok) failed = true;
        if (++waiting == n) {
            if (!failed) serial();
            waiting = 0; ++generation;
            bcv.notify_all();
        } else {
            const int gen = generation;
            bcv.wait(lk, [&] { return generation != gen; });
        }
        return !failed;
    };

    const int st = for_each_shard(m, [&](size_t k) -> int {
        // ---- round 1: the gate of every n-th pair ----
        std::vector<osfm_pair> gp;
        std::vector<int> gidx;
        for (int p = (int)k; p < num_pairs; p += n) { gp.push_back(pairs[p]); gidx.push_back(p); }
        std::vector<osfm_pair_result> gres(gp.size());
        int r = match_all_single(m->shards[k], gp.data(), (int)gp.size(), gres.data(), nullptr, 0, nullptr, kPhaseGate);
        if (r == OSFM_OK) for (size_t i = 0; i < gidx.size(); ++i) results[gidx[i]] = gres[i];
        if (!barrier(r == OSFM_OK, [&] {
                // the survivors of all shards, dealt by the work they are
                std::vector<int> cand;
                for (int p = 0; p < num_pairs; ++p) if (results[p].status == OSFM_PAIR_MATCHED) cand.push_back(p);
                deal_pairs_lpt(views, n, pairs, cand, &owner);
                for (int q = 0; q < n; ++q) {
                    int64_t bound = 0;      // a pair has at most min(features of either view) mutual matches
                    for (int p : owner[q]) {
                        sub_pairs[q].push_back(pairs[p]);
                        sub_res[q].push_back(results[p]);
                        const ViewData &a = views[pairs[p].view_1], &b = views[pairs[p].view_2];
                        bound += std::min(a.ns + a.nu, b.ns + b.nu);
                    }
                    sub_cap[q] = std::min(bound, capacity);
                }
            }))
            return r;
        // ---- round 2: full matching (and RANSAC-F) of this shard's survivors into its own page-locked block ----
        osfm_matcher::Staging &sg = m->shard_stage[k];
        const size_t need = (size_t)std::max<int64_t>(sub_cap[k], 1) * 2;
        r = OSFM_OK;
        if (sg.ints < need) {
            pinned_free(sg.ptr, sg.ints * 4);
            sg.ptr = nullptr; sg.ints = 0;
            if (pinned_alloc(reinterpret_cast<void **>(&sg.ptr), (need + need / 8) * 4, hipHostMallocPortable) != hipSuccess) {
                set_error("match_all: no page-locked memory for the lists of device %d", m->shards[k]->device);
                r = OSFM_E_DEVICE;
            } else sg.ints = need + need / 8;
        }
        if (r == OSFM_OK) {
            r = match_all_single(m->shards[k], sub_pairs[k].data(), (int)sub_pairs[k].size(), sub_res[k].data(),
                sg.ptr, sub_cap[k], &sub_total[k], kPhaseFull);
            // a shard that runs out of room has still classified and counted every pair
            sub_status[k] = r;
            if (r == OSFM_E_CAPACITY) r = OSFM_OK;
        }
        if (!barrier(r == OSFM_OK, [&] {
                // every count is known: the lists' places in the caller's buffer, in pair order
                std::vector<size_t> pos(n, 0);
                std::vector<int> own(num_pairs, -1);
                for (int q = 0; q < n; ++q) for (int p : owner[q]) own[p] = q;
                for (int p = 0; p < num_pairs; ++p) {
                    const int q = own[p];
                    if (q < 0) continue;                       // stopped at the gate (or empty): as round 1 left it
                    results[p] = sub_res[q][pos[q]++];
                    const int64_t local = results[p].offset;
                    results[p].offset = 0;
                    if (results[p].status == OSFM_PAIR_MATCHED) {
                        results[p].offset = run;
                        goff[p] = local;
                        run += verify ? results[p].num_inliers : results[p].num_matches;
                    }
                }
                overflow = run > capacity;
                for (int q = 0; q < n; ++q) overflow |= sub_status[q] == OSFM_E_CAPACITY;
            }))
            return r;
        if (overflow) return OSFM_OK;
        // ---- this shard's lists to their places ----
        const int32_t *src = sg.ptr;
        for (int p : owner[k]) {
            if (results[p].status != OSFM_PAIR_MATCHED) continue;
            const int64_t cnt = verify ? results[p].num_inliers : results[p].num_matches;
            if (cnt > 0) memcpy(corr + 2 * results[p].offset, src + 2 * goff[p], (size_t)cnt * 8);
        }
        return OSFM_OK;
    });
    if (st != OSFM_OK) return st;
    if (total) {
        // on overflow every shard reports what it needs: the required total
        int64_t need = 0;
        for (int k = 0; k < n; ++k) need += sub_total[k];
        *total = overflow ? need : run;
    }
    if (overflow) {
        set_error("match_all: %lld correspondences need more than the given capacity %lld",
            (long long)(total ? *total : run), (long long)capacity);
        return OSFM_E_CAPACITY;
    }
    return OSFM_OK;
}

}  // namespace osfm
