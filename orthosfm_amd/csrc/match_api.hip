// C-ABI implementation of the matching path (include/osfm_hip.h, section A).
// Host orchestration only: every inner product, reduction, ratio test,
// cross-check and compaction runs in the kernels of match_kernels.hip.
// This file holds the entries; what they call lives in the files match_internal.h lists.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "match_internal.h"
#include "cashash_kernels.h"
#include "ransac_kernels.h"
#include "ransac_affine.h"
#include "view_front.h"

namespace osfm {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

}  // namespace osfm

using namespace osfm;

extern "C" {

const char *osfm_last_error(void) { return g_last_error.c_str(); }
int osfm_version(void) { return OSFM_ABI_VERSION; }

int osfm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int osfm_ransac_selfcheck(int mode, uint64_t *counters)
{
    if (mode < 0 || mode > 2) { set_error("ransac_selfcheck: mode %d", mode); return OSFM_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("ransac_selfcheck: no HIP device available");
        return OSFM_E_DEVICE;
    }
    unsigned long long c[3] = {0, 0, 0};
    OSFM_RETURN_IF(ransac_set_mode(mode, c));
    if (counters) for (int i = 0; i < 3; ++i) counters[i] = c[i];
    return OSFM_OK;
}

int osfm_trim_device_memory(int device, uint64_t *released_bytes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("trim_device_memory: no HIP device available");
        return OSFM_E_DEVICE;
    }
    if (device < -1 || device >= ndev) { set_error("trim_device_memory: device %d out of range [-1,%d)", device, ndev); return OSFM_E_ARG; }
    const size_t b = g_device_pool.trim(device);
    if (released_bytes) *released_bytes = b;
    return OSFM_OK;
}

int osfm_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("device_memory: no HIP device available");
        return OSFM_E_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("device_memory: device %d out of range [0,%d)", device, ndev); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
    size_t f = 0, t = 0;
    OSFM_HIP_CHECK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return OSFM_OK;
}

int osfm_library_memory(osfm_memory_report *out)
{
    if (!out) { set_error("library_memory: null"); return OSFM_E_ARG; }
    out->device_buffer_bytes = g_ledger.device_buffer_bytes.load();
    out->pool_live_bytes = g_ledger.pool_live_bytes.load();
    out->pool_cached_bytes = g_ledger.pool_cached_bytes.load();
    out->pinned_host_bytes = g_ledger.pinned_host_bytes.load();
    out->live_matchers = g_ledger.live_matchers.load();
    out->live_streams = g_ledger.live_streams.load();
    out->live_events = g_ledger.live_events.load();
    out->reserved = 0;
    return OSFM_OK;
}

int osfm_match_options_default(osfm_match_options *o)
{
    if (!o) { set_error("options_default: null"); return OSFM_E_ARG; }
    o->sift_lowe_ratio = 0.8f;
    o->sift_distance_threshold = FLT_MAX;
    o->surf_lowe_ratio = 0.7f;
    o->surf_distance_threshold = FLT_MAX;
    o->use_lowres_matching = 1;
    o->num_lowres_features = 500;
    o->min_lowres_matches = 5;
    o->min_feature_matches = 50;
    o->pairs_per_batch = 0;
    o->geometric_verification = 0;
    o->ransac_max_iterations = 1000;
    o->ransac_threshold = 0.0015;
    o->min_matching_inliers = 30;
    o->matcher_type = OSFM_MATCHER_EXHAUSTIVE;
    o->ransac_seed = 0;
    o->cascade_keep_empty_blocks = 0;
    o->special_kernel_max = 0;
    o->ransac_model = OSFM_RANSAC_FUNDAMENTAL;
    o->ransac_refit = 1;
    return OSFM_OK;
}

int osfm_match_create(int device, int num_views, const osfm_match_options *opts, osfm_matcher **out)
{
    if (!out || num_views < 0) { set_error("match_create: bad arguments"); return OSFM_E_ARG; }
    *out = nullptr;
    if (opts && opts->ransac_model != OSFM_RANSAC_FUNDAMENTAL && opts->ransac_model != OSFM_RANSAC_AFFINE) {
        set_error("match_create: ransac_model %d", opts->ransac_model);
        return OSFM_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("match_create: no HIP device available (this backend has no CPU fallback)");
        return OSFM_E_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_error("match_create: device %d out of range [0,%d)", device, ndev);
        return OSFM_E_ARG;
    }
    OSFM_HIP_CHECK(hipSetDevice(device));
    // owned until the last step succeeded: an error return frees everything made so far
    struct Owner { osfm_matcher *p; ~Owner() { if (p) osfm_match_destroy(p); } } owner{(g_ledger.live_matchers++, new osfm_matcher())};
    osfm_matcher *m = owner.p;
    m->device = device;
    if (opts) m->opts = *opts; else osfm_match_options_default(&m->opts);
    m->views = std::vector<ViewData>(num_views);
    reset_stats(m);
    OSFM_HIP_CHECK(stream_create(&m->stream));
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) OSFM_HIP_CHECK(event_create(&m->ev[i][j], true));
    for (int j = 0; j < 2; ++j) OSFM_HIP_CHECK(event_create(&m->ev_sp[j], true));
    for (int j = 0; j < 2; ++j) OSFM_HIP_CHECK(event_create(&m->pin_ev[j], false));
    OSFM_HIP_CHECK(stream_create(&m->copy_stream));
    OSFM_HIP_CHECK(stream_create(&m->up_stream));
    for (int j = 0; j < 2; ++j) {
        OSFM_HIP_CHECK(event_create(&m->ev_compact[j], false));
        OSFM_HIP_CHECK(event_create(&m->ev_copied[j], false));
    }
    // at most 512: the finish kernel's scan of the special rows keys them with nine bits
    if (m->opts.special_kernel_max != 0) m->special_max = std::min(std::max(m->opts.special_kernel_max, 0), 512);
    // The finish kernel skips work for a query whose ratio test fails against a lower bound of its second best
    // (match_finish_kernel): that needs thresholds that never rise as the second distance falls.
    const auto monotone = [](const std::vector<int32_t> &tab) { return std::is_sorted(tab.begin(), tab.end()); };
    std::vector<int32_t> t;
    build_lowe_table(m->opts.sift_lowe_ratio, false, &t);
    if (!monotone(t)) { set_error("match_create: the SIFT ratio table is not monotone"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(m->lowe_sift.reserve(t.size() * 4));
    OSFM_HIP_CHECK(hipMemcpy(m->lowe_sift.ptr, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    build_lowe_table(m->opts.surf_lowe_ratio, true, &t);
    if (!monotone(t)) { set_error("match_create: the SURF ratio table is not monotone"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(m->lowe_surf.reserve(t.size() * 4));
    OSFM_HIP_CHECK(hipMemcpy(m->lowe_surf.ptr, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    m->tab_sift.reject_from = m->lowe_sift.as<int32_t>();
    m->tab_sift.max_d1 = max_d1_for(m->opts.sift_distance_threshold, false);
    m->tab_sift.is_signed = 0;
    m->tab_surf.reject_from = m->lowe_surf.as<int32_t>();
    m->tab_surf.max_d1 = max_d1_for(m->opts.surf_distance_threshold, true);
    m->tab_surf.is_signed = 1;
    owner.p = nullptr;
    *out = m;
    return OSFM_OK;
}

int osfm_match_create_multi(const int *device_ids, int num_devices, int num_views,
    const osfm_match_options *opts, osfm_matcher **out)
{
    if (!out || !device_ids || num_devices < 1 || num_views < 0) { set_error("match_create_multi: bad arguments"); return OSFM_E_ARG; }
    *out = nullptr;
    if (opts && opts->ransac_model != OSFM_RANSAC_FUNDAMENTAL && opts->ransac_model != OSFM_RANSAC_AFFINE) {
        set_error("match_create_multi: ransac_model %d", opts->ransac_model);
        return OSFM_E_ARG;
    }
    struct Owner { osfm_matcher *p; ~Owner() { if (p) osfm_match_destroy(p); } } owner{(g_ledger.live_matchers++, new osfm_matcher())};
    osfm_matcher *m = owner.p;
    m->device = device_ids[0];
    if (opts) m->opts = *opts; else osfm_match_options_default(&m->opts);
    reset_stats(m);
    for (int k = 0; k < num_devices; ++k) {
        osfm_matcher *sh = nullptr;
        OSFM_RETURN_IF(osfm_match_create(device_ids[k], num_views, &m->opts, &sh));
        m->shards.push_back(sh);
    }
    m->shard_stage.resize(num_devices);
    owner.p = nullptr;
    *out = m;
    return OSFM_OK;
}

int osfm_match_get_devices(const osfm_matcher *m, int32_t *device_ids, int capacity, int32_t *num_devices)
{
    if (!m || !num_devices || capacity < 0 || (capacity > 0 && !device_ids)) { set_error("match_get_devices: bad arguments"); return OSFM_E_ARG; }
    const int n = m->shards.empty() ? 1 : (int)m->shards.size();
    *num_devices = n;
    for (int k = 0; k < std::min(n, capacity); ++k) device_ids[k] = m->shards.empty() ? m->device : m->shards[k]->device;
    return OSFM_OK;
}

int osfm_match_destroy(osfm_matcher *m)
{
    if (!m) return OSFM_OK;
    if (!m->shards.empty() || !m->shard_stage.empty()) {
        for (auto *sh : m->shards) osfm_match_destroy(sh);
        for (auto &sg : m->shard_stage) pinned_free(sg.ptr, sg.ints * 4);
        g_ledger.live_matchers--;
        delete m;
        return OSFM_OK;
    }
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) event_destroy(m->ev[i][j]);
    for (int j = 0; j < 2; ++j) event_destroy(m->ev_sp[j]);
    for (int j = 0; j < 2; ++j) {
        event_destroy(m->pin_ev[j]);
        pinned_free(m->pin_ptr[j], m->pin_bytes[j]);
    }
    stream_destroy(m->copy_stream);
    stream_destroy(m->up_stream);
    for (int j = 0; j < 2; ++j) {
        event_destroy(m->ev_compact[j]);
        event_destroy(m->ev_copied[j]);
    }
    stream_destroy(m->stream);
    for (auto *sg : m->comb_staging) { pinned_free(sg->ptr, sg->ints * 4); delete sg; }
    g_ledger.live_matchers--;
    delete m;       // every DeviceBuffer (views, scratch, cascade-hashing data) frees itself
    return OSFM_OK;
}

// exhaustive_matching.cc:17-27 with math::clamp / math::round in float.
int osfm_quantize_sift(const float *src, int n, uint16_t *dst)
{
    if (n < 0 || (n > 0 && (!src || !dst))) { set_error("quantize_sift: bad arguments"); return OSFM_E_ARG; }
    for (size_t i = 0; i < (size_t)n * 128; ++i) {
        float v = src[i];
        v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        v *= 255.0f;
        v = v > 0.0f ? floorf(v + 0.5f) : ceilf(v - 0.5f);
        dst[i] = (uint16_t)(unsigned char)v;
    }
    return OSFM_OK;
}

// exhaustive_matching.cc:29-38.
int osfm_quantize_surf(const float *src, int n, int16_t *dst)
{
    if (n < 0 || (n > 0 && (!src || !dst))) { set_error("quantize_surf: bad arguments"); return OSFM_E_ARG; }
    for (size_t i = 0; i < (size_t)n * 64; ++i) {
        float v = src[i];
        v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
        v *= 127.0f;
        v = v > 0.0f ? floorf(v + 0.5f) : ceilf(v - 0.5f);
        dst[i] = (int16_t)(signed char)v;
    }
    return OSFM_OK;
}

int osfm_match_set_view(osfm_matcher *m, int view, const uint16_t *sift, int n_sift,
    const int16_t *surf, int n_surf)
{
    if (!m) { set_error("set_view: null matcher"); return OSFM_E_ARG; }
    if (!m->shards.empty())        // every shard holds the full bank: one host-to-device copy per device, side by side
        return for_each_shard(m, [&](size_t k) { return osfm_match_set_view(m->shards[k], view, sift, n_sift, surf, n_surf); });
    std::lock_guard<std::mutex> lock(m->up_mu);
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    return upload_view(m, view, sift, n_sift, surf, n_surf);
}

int osfm_match_set_view_float(osfm_matcher *m, int view, const float *sift, int n_sift,
    const float *surf, int n_surf)
{
    if (!m) { set_error("set_view_float: null matcher"); return OSFM_E_ARG; }
    if (n_sift < 0 || n_surf < 0) { set_error("set_view_float: negative count"); return OSFM_E_ARG; }
    std::vector<uint16_t> qs((size_t)n_sift * 128);
    std::vector<int16_t> qu((size_t)n_surf * 64);
    OSFM_RETURN_IF(osfm_quantize_sift(sift, n_sift, qs.data()));
    OSFM_RETURN_IF(osfm_quantize_surf(surf, n_surf, qu.data()));
    return osfm_match_set_view(m, view, qs.data(), n_sift, qu.data(), n_surf);
}

int osfm_match_expect_pairs(osfm_matcher *m, int32_t pairs_per_call)
{
    if (!m || pairs_per_call < 0) { set_error("match_expect_pairs: bad arguments"); return OSFM_E_ARG; }
    if (!m->shards.empty()) {
        for (auto *sh : m->shards) sh->expect_pairs = (pairs_per_call + (int)m->shards.size() - 1) / (int)m->shards.size();
        return OSFM_OK;
    }
    std::lock_guard<std::mutex> lock(m->mu);
    m->expect_pairs = pairs_per_call;
    return OSFM_OK;
}

int osfm_match_view_size(const osfm_matcher *m, int view, int *n_sift, int *n_surf)
{
    if (!m) { set_error("view_size: null matcher"); return OSFM_E_ARG; }
    if (!m->shards.empty()) return osfm_match_view_size(m->shards[0], view, n_sift, n_surf);
    OSFM_RETURN_IF(check_view(m, view, "view_size"));
    if (n_sift) *n_sift = m->views[view].ns;
    if (n_surf) *n_surf = m->views[view].nu;
    return OSFM_OK;
}

int osfm_match_set_positions(osfm_matcher *m, int view, const float *xy, int n)
{
    if (!m || n < 0 || (n > 0 && !xy)) { set_error("set_positions: bad argument"); return OSFM_E_ARG; }
    if (!m->shards.empty())
        return for_each_shard(m, [&](size_t k) { return osfm_match_set_positions(m->shards[k], view, xy, n); });
    std::lock_guard<std::mutex> lock(m->mu);
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    OSFM_RETURN_IF(check_view(m, view, "set_positions"));
    ViewData &v = m->views[view];
    if (n != v.ns + v.nu) {
        set_error("set_positions: view %d has %d features, got %d positions", view, v.ns + v.nu, n);
        return OSFM_E_ARG;
    }
    OSFM_RETURN_IF(v.positions.reserve((size_t)std::max(n, 1) * 8));
    if (n) OSFM_HIP_CHECK(hipMemcpy(v.positions.ptr, xy, (size_t)n * 8, hipMemcpyHostToDevice));
    v.n_positions = n;
    return OSFM_OK;
}

int osfm_match_set_view_from_front(osfm_matcher *m, int view, osfm_view_front *front)
{
    if (!m || !front) { set_error("set_view_from_front: null argument"); return OSFM_E_ARG; }
    FrontResult r;
    OSFM_RETURN_IF(view_front_result(front, &r));
    return handoff_all(m, view, r.device, r.sift_desc, r.sift_map, r.n_sift, r.surf_desc, r.surf_map, r.n_surf, r.normalized,
        [&](hipStream_t s) { return view_front_begin_read(front, s); }, [&](hipStream_t s) { return view_front_end_read(front, s); });
}

int osfm_match_debug_set_view_device(osfm_matcher *m, int view, const float *sift, int n_sift, const int32_t *sift_order,
    const float *surf, int n_surf, const int32_t *surf_order, const float *positions)
{
    if (!m || n_sift < 0 || n_surf < 0 || (n_sift > 0 && !sift) || (n_surf > 0 && !surf) || (n_sift + n_surf > 0 && !positions)) {
        set_error("debug_set_view_device: bad arguments");
        return OSFM_E_ARG;
    }
    for (int i = 0; i < n_sift; ++i)
        if (sift_order && (sift_order[i] < 0 || sift_order[i] >= n_sift)) { set_error("debug_set_view_device: sift_order[%d] out of range", i); return OSFM_E_ARG; }
    for (int i = 0; i < n_surf; ++i)
        if (surf_order && (surf_order[i] < 0 || surf_order[i] >= n_surf)) { set_error("debug_set_view_device: surf_order[%d] out of range", i); return OSFM_E_ARG; }
    const int device = m->shards.empty() ? m->device : m->shards[0]->device;
    OSFM_HIP_CHECK(hipSetDevice(device));
    DeviceBuffer d_sift, d_surf, d_so, d_uo, d_pos;
    auto put = [](DeviceBuffer &b, const void *src, size_t bytes) -> int {
        if (!src || !bytes) return OSFM_OK;
        OSFM_RETURN_IF(b.reserve(bytes));
        OSFM_HIP_CHECK(hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice));
        return OSFM_OK;
    };
    OSFM_RETURN_IF(put(d_sift, sift, (size_t)n_sift * 128 * 4));
    OSFM_RETURN_IF(put(d_surf, surf, (size_t)n_surf * 64 * 4));
    OSFM_RETURN_IF(put(d_so, sift_order, (size_t)n_sift * 4));
    OSFM_RETURN_IF(put(d_uo, surf_order, (size_t)n_surf * 4));
    OSFM_RETURN_IF(put(d_pos, positions, (size_t)(n_sift + n_surf) * 8));
    hipStream_t used = nullptr;
    const int rc = handoff_all(m, view, device, d_sift.as<float>(), d_so.as<int32_t>(), n_sift, d_surf.as<float>(), d_uo.as<int32_t>(),
        n_surf, d_pos.as<float>(), [&](hipStream_t s) -> int { used = s; return OSFM_OK; }, [](hipStream_t) -> int { return OSFM_OK; });
    if (used) (void)hipStreamSynchronize(used);      // the source arrays go with this call
    return rc;
}

int osfm_match_debug_view_bank(osfm_matcher *m, int view, int shard, osfm_view_bank *b)
{
    if (!m || !b) { set_error("debug_view_bank: null argument"); return OSFM_E_ARG; }
    if (!m->shards.empty()) {
        if (shard < 0 || shard >= (int)m->shards.size()) { set_error("debug_view_bank: shard %d of %zu", shard, m->shards.size()); return OSFM_E_ARG; }
        return osfm_match_debug_view_bank(m->shards[(size_t)shard], view, 0, b);
    }
    std::lock_guard<std::mutex> lock(m->up_mu);
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    OSFM_RETURN_IF(check_view(m, view, "debug_view_bank"));
    const ViewData &v = m->views[view];
    OSFM_HIP_CHECK(hipStreamSynchronize(m->up_stream));
    const int sp_pad = v.n_special > 0 ? round_up(v.n_special, kRowsPerBlock) : 0;
    b->n_sift = v.ns; b->n_surf = v.nu; b->n_sift_pad = v.ns_pad; b->n_surf_pad = v.nu_pad;
    b->n_special = v.n_special; b->n_special_pad = sp_pad; b->surf_norm2_max = v.surf_norm2_max; b->n_positions = v.n_positions;
    struct { void *to; const DeviceBuffer *from; size_t bytes; } arrays[] = {
        {b->sift, &v.sift, (size_t)v.ns_pad * 128}, {b->sift_corr, &v.sift_corr, (size_t)v.ns_pad * 4},
        {b->sift_raw, &v.sift_raw, (size_t)v.ns_pad * 128}, {b->sift_raw_corr, &v.sift_raw_corr, (size_t)v.ns_pad * 4},
        {b->surf, &v.surf, (size_t)v.nu_pad * 64}, {b->surf_corr, &v.surf_corr, (size_t)v.nu_pad * 4},
        {b->special, &v.special, (size_t)sp_pad * 128}, {b->special_corr, &v.special_corr, (size_t)sp_pad * 4},
        {b->special_map, &v.special_map, sp_pad ? (size_t)v.n_special * 4 : 0},
        {b->special_slot, &v.special_slot, sp_pad ? (size_t)v.ns * 4 : 0},
        {b->positions, &v.positions, (size_t)std::max(v.n_positions, 0) * 8},
    };
    for (auto &r : arrays)
        if (r.to && r.bytes) OSFM_HIP_CHECK(hipMemcpy(r.to, r.from->ptr, r.bytes, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

int osfm_ransac_options_default(osfm_ransac_options *o)
{
    if (!o) { set_error("ransac_options_default: null"); return OSFM_E_ARG; }
    o->max_iterations = 1000; o->reserved = 0; o->threshold = 0.0015; o->seed = 0;
    return OSFM_OK;
}

}  // extern "C"

// One pair through a pair-RANSAC kernel, for the two single-pair entries: the checks, the upload, the job record, the
// launch (launch(job, scratch, result record), all on the device), the wait and the results.  name: the entry in
// error messages; min_k: the matches a sample of the model needs; result: the model's own record, if it has one.
template <class Launch>
static int ransac_single_pair(const char *name, int min_k, size_t scratch_bytes, int device, const float *pos1, int n1,
    const float *pos2, int n2, const int32_t *corr, int k, uint64_t pair_id, int32_t *inliers, int32_t *num_inliers,
    double *F, void *result, size_t result_bytes, Launch launch)
{
    if (n1 < 0 || n2 < 0 || k < 0 || !num_inliers || (k > 0 && (!pos1 || !pos2 || !corr || !inliers))) {
        set_error("%s: bad argument", name); return OSFM_E_ARG;
    }
    for (int i = 0; i < k; ++i)
        if (corr[2 * i] < 0 || corr[2 * i] >= n1 || corr[2 * i + 1] < 0 || corr[2 * i + 1] >= n2) {
            set_error("%s: correspondence %d out of range", name, i); return OSFM_E_ARG;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("%s: no HIP device available (this backend has no CPU fallback)", name);
        return OSFM_E_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("%s: bad device", name); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
    if (k < min_k) { *num_inliers = -1; return OSFM_OK; }
    DeviceBuffer d1, d2, dc, di, dn, df, dj, dr;
    struct Rel { DeviceBuffer *b[8]; ~Rel() { for (auto *x : b) x->release(); } } rel{{&d1, &d2, &dc, &di, &dn, &df, &dj, &dr}};
    OSFM_RETURN_IF(d1.reserve((size_t)n1 * 8)); OSFM_RETURN_IF(d2.reserve((size_t)n2 * 8));
    OSFM_RETURN_IF(dc.reserve((size_t)k * 8)); OSFM_RETURN_IF(di.reserve((size_t)k * 4));
    OSFM_RETURN_IF(dn.reserve(16)); OSFM_RETURN_IF(df.reserve(72));
    if (result_bytes) OSFM_RETURN_IF(dr.reserve(result_bytes));
    OSFM_RETURN_IF(dj.reserve(256 + scratch_bytes));                 // the job, then the kernel's scratch
    OSFM_HIP_CHECK(hipMemcpy(d1.ptr, pos1, (size_t)n1 * 8, hipMemcpyHostToDevice));
    OSFM_HIP_CHECK(hipMemcpy(d2.ptr, pos2, (size_t)n2 * 8, hipMemcpyHostToDevice));
    OSFM_HIP_CHECK(hipMemcpy(dc.ptr, corr, (size_t)k * 8, hipMemcpyHostToDevice));
    RansacJob job;
    memset(&job, 0, sizeof(job));
    job.pos1 = d1.as<float>(); job.pos2 = d2.as<float>(); job.corr = dc.as<int32_t>(); job.k = k;
    job.pair_id = pair_id; job.inliers_out = di.as<int32_t>(); job.count_out = dn.as<int32_t>();
    job.F_out = df.as<double>();
    OSFM_HIP_CHECK(hipMemcpy(dj.ptr, &job, sizeof(job), hipMemcpyHostToDevice));
    launch(dj.as<RansacJob>(), static_cast<char *>(dj.ptr) + 256, dr.ptr);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipDeviceSynchronize());
    int32_t cnt = 0;
    OSFM_HIP_CHECK(hipMemcpy(&cnt, dn.ptr, 4, hipMemcpyDeviceToHost));
    *num_inliers = cnt;
    if (cnt > 0) OSFM_HIP_CHECK(hipMemcpy(inliers, di.ptr, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    if (F) OSFM_HIP_CHECK(hipMemcpy(F, df.ptr, 72, hipMemcpyDeviceToHost));
    if (result) OSFM_HIP_CHECK(hipMemcpy(result, dr.ptr, result_bytes, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

extern "C" {

int osfm_ransac_fundamental(int device, const float *pos1, int n1, const float *pos2, int n2,
    const int32_t *corr, int k, const osfm_ransac_options *opts, uint64_t pair_id,
    int32_t *inliers, int32_t *num_inliers, double *F)
{
    osfm_ransac_options o;
    if (opts) o = *opts; else osfm_ransac_options_default(&o);
    return ransac_single_pair("ransac_fundamental", 8, ransac_scratch_bytes(1), device, pos1, n1, pos2, n2, corr, k, pair_id,
        inliers, num_inliers, F, nullptr, 0, [&](const RansacJob *d_job, void *scratch, void *) {
            launch_ransac(d_job, 1, o.max_iterations, o.threshold, o.seed, scratch, nullptr);
        });
}

int osfm_ransac_affine_options_default(osfm_ransac_affine_options *o)
{
    if (!o) { set_error("ransac_affine_options_default: null"); return OSFM_E_ARG; }
    o->max_iterations = 1000; o->refit = 1; o->threshold = 0.0015; o->seed = 0;
    return OSFM_OK;
}

int osfm_ransac_affine(int device, const float *pos1, int n1, const float *pos2, int n2,
    const int32_t *corr, int k, const osfm_ransac_affine_options *opts, uint64_t pair_id,
    int32_t *inliers, int32_t *num_inliers, double *F, osfm_ransac_affine_result *result)
{
    osfm_ransac_affine_options o;
    if (opts) o = *opts; else osfm_ransac_affine_options_default(&o);
    return ransac_single_pair("ransac_affine", 4, affine_scratch_bytes(1), device, pos1, n1, pos2, n2, corr, k, pair_id,
        inliers, num_inliers, F, result, sizeof(*result), [&](const RansacJob *d_job, void *scratch, void *d_result) {
            launch_ransac_affine(d_job, 1, o.max_iterations, o.threshold, o.refit, o.seed, scratch,
                static_cast<osfm_ransac_affine_result *>(d_result), nullptr);
        });
}

int osfm_match_pair(osfm_matcher *m, int view_1, int view_2, int32_t *m12, int32_t *len12,
    int32_t *m21, int32_t *len21)
{
    if (!m || !m12 || !m21) { set_error("match_pair: null argument"); return OSFM_E_ARG; }
    if (!m->shards.empty())        // concurrent callers spread over the devices; each shard combines its own arrivals
        return osfm_match_pair(m->shards[m->next_shard++ % m->shards.size()], view_1, view_2, m12, len12, m21, len21);
    // a bad view id fails its own call, not the batch it would have joined
    OSFM_RETURN_IF(check_view(m, view_1, "match"));
    OSFM_RETURN_IF(check_view(m, view_2, "match"));
    osfm_matcher::PairRequest rq;
    rq.kind = 0; rq.v1 = view_1; rq.v2 = view_2; rq.num_features = 0;
    rq.m12 = m12; rq.m21 = m21; rq.len12 = len12; rq.len21 = len21; rq.count = nullptr;
    return combine(m, rq);
}

int osfm_match_pair_lowres(osfm_matcher *m, int view_1, int view_2, int num_features, int32_t *count)
{
    if (!m || !count) { set_error("match_pair_lowres: null argument"); return OSFM_E_ARG; }
    if (!m->shards.empty())
        return osfm_match_pair_lowres(m->shards[m->next_shard++ % m->shards.size()], view_1, view_2, num_features, count);
    if (num_features <= 0) { *count = 0; return OSFM_OK; }
    OSFM_RETURN_IF(check_view(m, view_1, "match"));
    OSFM_RETURN_IF(check_view(m, view_2, "match"));
    osfm_matcher::PairRequest rq;
    rq.kind = 1; rq.v1 = view_1; rq.v2 = view_2; rq.num_features = num_features;
    rq.m12 = rq.m21 = rq.len12 = rq.len21 = nullptr; rq.count = count;
    return combine(m, rq);
}

int osfm_match_twoway(osfm_matcher *m, int view_1, int view_2, int descriptor_type, int num_features,
    int32_t *m12, int32_t *m21)
{
    if (!m || !m12 || !m21 || (descriptor_type != 0 && descriptor_type != 1) || num_features < 0) {
        set_error("match_twoway: bad argument");
        return OSFM_E_ARG;
    }
    if (!m->shards.empty()) return osfm_match_twoway(m->shards[0], view_1, view_2, descriptor_type, num_features, m12, m21);
    std::lock_guard<std::mutex> lock(m->mu);
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    reset_stats(m);
    osfm_pair pr = {view_1, view_2};
    BatchResult res;
    BatchMode mode;
    mode.limit = num_features; mode.apply = false; mode.type_mask = 1 << descriptor_type;
    OSFM_RETURN_IF(run_batch(m, &pr, 1, mode, &res));
    const PairPlan &pl = res.plans[0];
    // With an empty set 1 Matching::twoway_match yields matches_1_2 of size 0
    // and matches_2_1 of size n2 filled with -1 (matching.h:121-124).
    const ViewData &a = m->views[view_1], &b = m->views[view_2];
    int n1 = descriptor_type == 0 ? a.ns : a.nu, n2 = descriptor_type == 0 ? b.ns : b.nu;
    if (num_features > 0) { n1 = std::min(n1, num_features); n2 = std::min(n2, num_features); }
    if (n1 == 0) { for (int i = 0; i < n2; ++i) m21[i] = -1; return OSFM_OK; }
    const int32_t *d_out = m->out.as<int32_t>();
    if (pl.len12) OSFM_HIP_CHECK(hipMemcpy(m12, d_out + pl.off12, (size_t)pl.len12 * 4, hipMemcpyDeviceToHost));
    if (pl.len21) OSFM_HIP_CHECK(hipMemcpy(m21, d_out + pl.off21, (size_t)pl.len21 * 4, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

int osfm_pair_from_index(int64_t index, int32_t *view_1, int32_t *view_2)
{
    if (index < 0 || !view_1 || !view_2) { set_error("pair_from_index: bad arguments"); return OSFM_E_ARG; }
    // bundler_matching.cc:92-93
    const int a = (int)(0.5 + std::sqrt(0.25 + 2.0 * (double)index));
    *view_1 = a;
    *view_2 = (int)index - a * (a - 1) / 2;
    return OSFM_OK;
}

int osfm_match_all(osfm_matcher *m, const osfm_pair *pairs, int num_pairs, osfm_pair_result *results,
    int32_t *corr, int64_t capacity, int64_t *total)
{
    if (!m || (num_pairs > 0 && (!pairs || !results)) || num_pairs < 0 || capacity < 0 ||
        (capacity > 0 && !corr)) {
        set_error("match_all: bad arguments");
        return OSFM_E_ARG;
    }
    if (!m->shards.empty()) return multi_match_all(m, pairs, num_pairs, results, corr, capacity, total);
    return match_all_single(m, pairs, num_pairs, results, corr, capacity, total, kPhaseBoth);
}

int osfm_match_get_cascade_hashes(osfm_matcher *m, int view, int type, uint64_t *hashes,
    uint8_t *bucket_ids)
{
    if (!m || type < 0 || type > 1) { set_error("get_cascade_hashes: bad arguments"); return OSFM_E_ARG; }
    if (!m->shards.empty()) return osfm_match_get_cascade_hashes(m->shards[0], view, type, hashes, bucket_ids);
    std::lock_guard<std::mutex> lock(m->mu);
    OSFM_RETURN_IF(check_view(m, view, "get_cascade_hashes"));
    OSFM_HIP_CHECK(hipSetDevice(m->device));
    OSFM_RETURN_IF(ensure_cashash(m));
    const ViewData &v = m->views[view];
    const int n = type == 0 ? v.ns : v.nu;
    const int words = type == 0 ? 2 : 1;
    if (n > 0 && hashes)
        OSFM_HIP_CHECK(hipMemcpy(hashes, v.cas_hash[type].ptr, (size_t)n * words * 8, hipMemcpyDeviceToHost));
    if (n > 0 && bucket_ids)
        OSFM_HIP_CHECK(hipMemcpy(bucket_ids, v.cas_bucket[type].ptr, (size_t)n * kCasGroups, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

int osfm_match_get_shard_stats(const osfm_matcher *m, int shard, osfm_match_stats *out)
{
    if (!m || !out) { set_error("get_shard_stats: null argument"); return OSFM_E_ARG; }
    const int n = m->shards.empty() ? 1 : (int)m->shards.size();
    if (shard < 0 || shard >= n) { set_error("get_shard_stats: shard %d of %d", shard, n); return OSFM_E_ARG; }
    *out = m->shards.empty() ? m->stats : m->shards[shard]->stats;
    return OSFM_OK;
}

int osfm_match_get_stats(const osfm_matcher *m, osfm_match_stats *out)
{
    if (!m || !out) { set_error("get_stats: null argument"); return OSFM_E_ARG; }
    if (!m->shards.empty()) {
        // sums over the shards' most recent calls (times are device times: they ran side by side)
        memset(out, 0, sizeof(*out));
        for (const auto *sh : m->shards) {
            const osfm_match_stats &t = sh->stats;
            out->tile_kernel_ms += t.tile_kernel_ms; out->tile_kernel_launches += t.tile_kernel_launches;
            out->exact_scan_queries += t.exact_scan_queries; out->mac_count += t.mac_count;
            out->algorithmic_bytes += t.algorithmic_bytes; out->lowres_kernel_ms += t.lowres_kernel_ms;
            out->lowres_kernel_launches += t.lowres_kernel_launches; out->lowres_mac_count += t.lowres_mac_count;
            out->cashash_kernel_ms += t.cashash_kernel_ms; out->cashash_kernel_launches += t.cashash_kernel_launches;
            out->special_kernel_launches += t.special_kernel_launches; out->special_kernel_ms += t.special_kernel_ms;
            out->tile_shader_cycles += t.tile_shader_cycles; out->tile_refclk_ticks += t.tile_refclk_ticks;
            out->surf_tile_kernel_ms += t.surf_tile_kernel_ms; out->surf_tile_kernel_launches += t.surf_tile_kernel_launches;
            out->surf_mac_count += t.surf_mac_count; out->tile_workgroups += t.tile_workgroups;
        }
        return OSFM_OK;
    }
    *out = m->stats;
    return OSFM_OK;
}

// The symbols a binary built against the header before osfm_match_options grew (ransac_model, ransac_refit) binds: the
// struct as it was then, up to special_kernel_max; the rest takes its defaults.  The header binds today's callers to
// the *_v2 definitions above.
#undef osfm_match_options_default
#undef osfm_match_create
#undef osfm_match_create_multi
static constexpr size_t kOptionsBytesBefore = offsetof(osfm_match_options, ransac_model);
static_assert(kOptionsBytesBefore == 80, "the layout binaries built against the earlier header pass");

static osfm_match_options options_from_before(const void *opts)
{
    osfm_match_options o;
    memset(&o, 0, sizeof(o));                 // its padding too: osfm_match_options_default copies it out
    osfm_match_options_default_v2(&o);
    if (opts) memcpy(&o, opts, kOptionsBytesBefore);
    return o;
}

OSFM_API int osfm_match_options_default(void *opts)
{
    if (!opts) { set_error("options_default: null"); return OSFM_E_ARG; }
    const osfm_match_options o = options_from_before(nullptr);
    memcpy(opts, &o, kOptionsBytesBefore);
    return OSFM_OK;
}

OSFM_API int osfm_match_create(int device, int num_views, const void *opts, osfm_matcher **out)
{
    const osfm_match_options o = options_from_before(opts);
    return osfm_match_create_v2(device, num_views, &o, out);
}

OSFM_API int osfm_match_create_multi(const int *device_ids, int num_devices, int num_views, const void *opts, osfm_matcher **out)
{
    const osfm_match_options o = options_from_before(opts);
    return osfm_match_create_multi_v2(device_ids, num_devices, num_views, &o, out);
}

}  // extern "C"
