// The request combiner of the per-pair entries (osfm_match_pair, osfm_match_pair_lowres): concurrent callers
// become one batch (see osfm_matcher::PairRequest).
#include <algorithm>
#include <cstring>

#include "match_internal.h"

namespace osfm {

namespace {

constexpr size_t kCombineMax = 64;       // requests per combined batch

// One combined batch: requests of one kind (and, for the low-res kind, one feature limit).
void serve_requests(osfm_matcher *m, const std::vector<osfm_matcher::PairRequest *> &batch)
{
    auto fail_all = [&](int status) {
        const std::string msg = osfm_last_error();
        for (auto *r : batch) { r->status = status; r->error = msg; }
    };
    std::lock_guard<std::mutex> lock(m->mu);
    if (hipSetDevice(m->device) != hipSuccess) { set_error("match_pair: hipSetDevice failed"); fail_all(OSFM_E_DEVICE); return; }
    reset_stats(m);
    std::vector<osfm_pair> pairs(batch.size());
    for (size_t k = 0; k < batch.size(); ++k) pairs[k] = {batch[k]->v1, batch[k]->v2};
    BatchResult res;
    BatchMode mode;
    if (batch[0]->kind == 1) { mode.limit = batch[0]->num_features; mode.lowres = true; mode.apply = false; }
    int st = run_batch(m, pairs.data(), (int)pairs.size(), mode, &res);
    if (st != OSFM_OK) { fail_all(st); return; }
    if (batch[0]->kind == 1) {
        for (size_t k = 0; k < batch.size(); ++k) *batch[k]->count = res.counts[k];
        return;
    }
    // all lists of the batch lie back to back in m->out: ONE copy into a page-locked block (two
    // pageable copies per pair were most of a batch's time); every requester then takes its own
    osfm_matcher::Staging *stage = nullptr;
    {
        std::lock_guard<std::mutex> q(m->comb_mu);
        for (auto *sg : m->comb_staging)
            if (sg->users == 0 && (!stage || sg->ints > stage->ints)) stage = sg;
        if (!stage) { stage = new osfm_matcher::Staging; m->comb_staging.push_back(stage); }
        stage->users = (int)batch.size();
    }
    const size_t need = (size_t)std::max<int64_t>(res.out_ints, 4);
    hipError_t e = hipSuccess;
    if (stage->ints < need) {
        pinned_free(stage->ptr, stage->ints * 4);
        stage->ptr = nullptr; stage->ints = 0;
        e = pinned_alloc(reinterpret_cast<void **>(&stage->ptr), (need + need / 4) * 4, hipHostMallocDefault);
        if (e == hipSuccess) stage->ints = need + need / 4;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(stage->ptr, m->out.ptr, need * 4, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) {
        set_error("match_pair: copy of the lists failed: %s", hipGetErrorString(e));
        fail_all(OSFM_E_DEVICE);
        std::lock_guard<std::mutex> q(m->comb_mu);
        stage->users = 0;
        return;
    }
    for (size_t k = 0; k < batch.size(); ++k) {
        const PairPlan &pl = res.plans[k];
        batch[k]->stage = stage;
        batch[k]->src12 = pl.off12; batch[k]->n12 = pl.len12;
        batch[k]->src21 = pl.off21; batch[k]->n21 = pl.len21;
    }
}

}  // namespace

int combine(osfm_matcher *m, osfm_matcher::PairRequest &rq)
{
    std::unique_lock<std::mutex> lk(m->comb_mu);
    m->comb_queue.push_back(&rq);
    while (!rq.done) {
        if (m->comb_leader) { m->comb_cv.wait(lk); continue; }
        m->comb_leader = true;
        while (!rq.done && !m->comb_queue.empty()) {
            // everything of the kind at the head of the queue, in arrival order
            std::vector<osfm_matcher::PairRequest *> batch;
            const osfm_matcher::PairRequest *head = m->comb_queue.front();
            for (auto it = m->comb_queue.begin(); it != m->comb_queue.end() && batch.size() < kCombineMax;) {
                if ((*it)->kind == head->kind && (*it)->num_features == head->num_features) {
                    batch.push_back(*it);
                    it = m->comb_queue.erase(it);
                } else {
                    ++it;
                }
            }
            lk.unlock();
            // The leader must not leave the others waiting for ever, and no exception may cross the C ABI into
            // the caller's OpenMP loop: a failure inside the batch (an allocation, say) fails the batch.
            try {
                serve_requests(m, batch);
            } catch (const std::exception &e) {
                for (auto *r : batch) { r->status = OSFM_E_STATE; r->error = std::string("match_pair: ") + e.what(); r->stage = nullptr; }
            } catch (...) {
                for (auto *r : batch) { r->status = OSFM_E_STATE; r->error = "match_pair: unknown failure in the combined batch"; r->stage = nullptr; }
            }
            lk.lock();
            for (auto *r : batch) r->done = true;
            m->comb_cv.notify_all();
        }
        m->comb_leader = false;
        m->comb_cv.notify_all();             // a waiter whose request is still queued takes over
    }
    lk.unlock();
    if (rq.stage) {
        if (rq.n12) memcpy(rq.m12, rq.stage->ptr + rq.src12, (size_t)rq.n12 * 4);
        if (rq.n21) memcpy(rq.m21, rq.stage->ptr + rq.src21, (size_t)rq.n21 * 4);
        if (rq.len12) *rq.len12 = rq.n12;
        if (rq.len21) *rq.len21 = rq.n21;
        lk.lock();
        rq.stage->users--;
        lk.unlock();
    }
    if (rq.status != OSFM_OK) set_error("%s", rq.error.c_str());
    return rq.status;
}

}  // namespace osfm
