// How a view's descriptors reach a matcher: upload from the host, the hand-off from a view front end on the device,
// copies between shards -- and the cascade-hash build over the whole bank.
#include <algorithm>
#include <cstdlib>
#include <random>
#include <thread>

#include "match_internal.h"
#include "cashash_kernels.h"
#include "view_kernels.h"

namespace osfm {

namespace {

// A view of n_sift + n_surf descriptors, not set yet: its sizes and the six operand arrays.
int size_view(ViewData &v, int n_sift, int n_surf)
{
    v.set = false;
    v.ns = n_sift; v.nu = n_surf;
    v.ns_pad = round_up(std::max(n_sift, 1), kRowsPerBlock);
    v.nu_pad = round_up(std::max(n_surf, 1), kRowsPerBlock);
    OSFM_RETURN_IF(v.sift.reserve((size_t)v.ns_pad * 128));
    OSFM_RETURN_IF(v.sift_corr.reserve((size_t)v.ns_pad * 4));
    OSFM_RETURN_IF(v.sift_raw.reserve((size_t)v.ns_pad * 128));
    OSFM_RETURN_IF(v.sift_raw_corr.reserve((size_t)v.ns_pad * 4));
    OSFM_RETURN_IF(v.surf.reserve((size_t)v.nu_pad * 64));
    OSFM_RETURN_IF(v.surf_corr.reserve((size_t)v.nu_pad * 4));
    return OSFM_OK;
}

// The rows special_map names, gathered into the view's special set (v.n_special > 0, the map is on the device).
int gather_special(ViewData &v, hipStream_t s)
{
    const int sp_pad = round_up(v.n_special, kRowsPerBlock);
    OSFM_RETURN_IF(v.special.reserve((size_t)sp_pad * 128));
    OSFM_RETURN_IF(v.special_corr.reserve((size_t)sp_pad * 4));
    // zero-vector padding in the value-128 form: bytes -128, correction -2^20 - 2^22
    launch_gather_rows(v.sift.as<int8_t>(), v.sift_corr.as<int32_t>(), v.special_map.as<int32_t>(),
        v.n_special, sp_pad, 128, -(1 << 20) - (1 << 22), (int8_t)-128, v.special.as<int8_t>(),
        v.special_corr.as<int32_t>(), s);
    return OSFM_OK;
}

}  // namespace

int upload_view(osfm_matcher *m, int view, const uint16_t *sift, int n_sift, const int16_t *surf,
    int n_surf)
{
    if (view < 0 || view >= (int)m->views.size()) {
        set_error("set_view: view id %d out of range", view);
        return OSFM_E_ARG;
    }
    if (n_sift < 0 || n_surf < 0 || (n_sift > 0 && !sift) || (n_surf > 0 && !surf)) {
        set_error("set_view: null descriptors / negative count");
        return OSFM_E_ARG;
    }
    ViewData &v = m->views[view];
    hipStream_t s = m->up_stream;
    OSFM_RETURN_IF(size_view(v, n_sift, n_surf));
    // One pass over the caller's descriptors on the host: range check (an error leaves the view
    // unset before anything is queued), the list of special rows, the largest SURF norm -- while
    // copying them into a page-locked block (two alternate, guarded by events).  Everything behind
    // that is queued on the stream and NOT waited for: the next view's host pass runs while this
    // view's transfer and conversion kernels do (200 views x 20k: 0.29 -> 0.12 s).
    const size_t b_sift = (size_t)n_sift * 128 * 2, b_surf = (size_t)n_surf * 64 * 2;
    const size_t b_ints = (size_t)n_sift * 4 * 2;                       // special list + slot map behind the descriptors
    const size_t need = std::max<size_t>(b_sift + b_surf + b_ints, 64);
    const int ps = m->pin_next++ & 1;
    if (m->pin_used[ps]) OSFM_HIP_CHECK(hipEventSynchronize(m->pin_ev[ps]));
    if (m->pin_bytes[ps] < need) {
        pinned_free(m->pin_ptr[ps], m->pin_bytes[ps]);
        m->pin_ptr[ps] = nullptr; m->pin_bytes[ps] = 0;
        OSFM_HIP_CHECK(pinned_alloc(reinterpret_cast<void **>(&m->pin_ptr[ps]), need + need / 4, hipHostMallocDefault));
        m->pin_bytes[ps] = need + need / 4;
    }
    char *pin = m->pin_ptr[ps];
    uint16_t *p_sift = reinterpret_cast<uint16_t *>(pin);
    int16_t *p_surf = reinterpret_cast<int16_t *>(pin + b_sift);
    int32_t *p_special = reinterpret_cast<int32_t *>(pin + b_sift + b_surf), *p_slot = p_special + n_sift;
    int n_special = 0;
    bool bad = false;
    {
        // copy + row maxima on a few threads (the pass is memory bound: 5 MB per 20k-feature view), then the
        // special rows numbered in ascending order: the same gathered set on every run
        auto rows = [&](int lo, int hi, int *bad_out) {
            int b = 0;
            for (int i = lo; i < hi; ++i) {
                const uint16_t *d = sift + (size_t)i * 128;
                uint16_t *o = p_sift + (size_t)i * 128;
                unsigned mx = 0;
                for (int k = 0; k < 128; ++k) { o[k] = d[k]; mx = std::max<unsigned>(mx, d[k]); }
                b |= mx > 255;
                p_slot[i] = mx > 127 ? 1 : 0;
            }
            *bad_out = b;
        };
        static const int max_thr = getenv("OSFM_UPLOAD_THREADS") ? std::max(1, std::min(4, atoi(getenv("OSFM_UPLOAD_THREADS")))) : 4;
        const int nthr = n_sift >= 8192 ? max_thr : 1;
        int bad_t[4] = {0, 0, 0, 0};
        std::vector<std::thread> th;
        for (int t = 1; t < nthr; ++t)
            th.emplace_back(rows, (int)((int64_t)n_sift * t / nthr), (int)((int64_t)n_sift * (t + 1) / nthr), &bad_t[t]);
        rows(0, (int)((int64_t)n_sift / nthr), &bad_t[0]);
        for (auto &t : th) t.join();
        for (int t = 0; t < nthr; ++t) bad |= bad_t[t] != 0;
        for (int i = 0; i < n_sift; ++i) {
            if (p_slot[i]) { p_slot[i] = n_special; p_special[n_special++] = i; }
            else p_slot[i] = -1;
        }
    }
    long long norm2_max = 0;
    for (int i = 0; i < n_surf; ++i) {
        const int16_t *d = surf + (size_t)i * 64;
        int16_t *o = p_surf + (size_t)i * 64;
        long long n2 = 0;
        for (int k = 0; k < 64; ++k) { o[k] = d[k]; bad |= d[k] > 127 || d[k] < -128; n2 += (long long)d[k] * d[k]; }
        norm2_max = std::max(norm2_max, n2);
    }
    if (bad) {
        set_error("set_view: descriptor value outside the quantised range "
                  "(SIFT 0..255, SURF -128..127) in view %d", view);
        return OSFM_E_RANGE;
    }
    OSFM_RETURN_IF(m->stage_in.reserve(std::max<size_t>(b_sift + b_surf, 16)));
    OSFM_RETURN_IF(m->flags.reserve(16));
    char *stage = m->stage_in.as<char>();
    if (b_sift + b_surf) OSFM_HIP_CHECK(hipMemcpyAsync(stage, pin, b_sift + b_surf, hipMemcpyHostToDevice, s));
    int32_t *flags = m->flags.as<int32_t>();       // written by the kernels' own range checks; the host pass above has decided
    launch_prepare_sift(reinterpret_cast<const uint16_t *>(stage), n_sift, v.ns_pad,
        v.sift.as<int8_t>(), v.sift_corr.as<int32_t>(), v.sift_raw.as<int8_t>(),
        v.sift_raw_corr.as<int32_t>(), flags + 0, s);
    v.n_special = n_special;
    if (v.n_special > 0) {
        OSFM_RETURN_IF(v.special_map.reserve((size_t)v.n_special * 4));
        OSFM_RETURN_IF(v.special_slot.reserve((size_t)n_sift * 4));
        OSFM_HIP_CHECK(hipMemcpyAsync(v.special_map.ptr, p_special, (size_t)v.n_special * 4, hipMemcpyHostToDevice, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(v.special_slot.ptr, p_slot, (size_t)n_sift * 4, hipMemcpyHostToDevice, s));
        OSFM_RETURN_IF(gather_special(v, s));
    }
    launch_prepare_surf(reinterpret_cast<const int16_t *>(stage + b_sift), n_surf, v.nu_pad,
        v.surf.as<int8_t>(), v.surf_corr.as<int32_t>(), flags + 1, flags + 2, s);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(m->pin_ev[ps], s));
    m->pin_used[ps] = true;
    if (!v.ready) OSFM_HIP_CHECK(event_create(&v.ready, false));
    OSFM_HIP_CHECK(hipEventRecord(v.ready, s));
    v.surf_norm2_max = (int)std::min<long long>(norm2_max, 0x7fffffff);
    v.set = true;
    m->cas_dirty = true;           // the cascade hashes depend on the average over all views
    return OSFM_OK;
}

// upload_view's result from float rows that are on this matcher's device already (the view front end's hand-off):
// row i of the view is row sift_map[i] of d_sift (NULL: row i), likewise SURF; d_positions holds ns + nu rows.
// Queued on the upload stream like upload_view; the host waits once, for the number of special rows (which sizes
// their gathered set) and the largest SURF norm.  The caller has made the stream wait for the source arrays.
static int handoff_view(osfm_matcher *m, int view, const float *d_sift, const int32_t *sift_map, int n_sift, const float *d_surf,
    const int32_t *surf_map, int n_surf, const float *d_positions)
{
    ViewData &v = m->views[view];
    hipStream_t s = m->up_stream;
    OSFM_RETURN_IF(size_view(v, n_sift, n_surf));
    // the scan writes both before the number of special rows is known: sized for every row
    OSFM_RETURN_IF(v.special_slot.reserve((size_t)std::max(n_sift, 1) * 4));
    OSFM_RETURN_IF(v.special_map.reserve((size_t)std::max(n_sift, 1) * 4));
    OSFM_RETURN_IF(v.positions.reserve((size_t)std::max(n_sift + n_surf, 1) * 8));
    OSFM_RETURN_IF(m->flags.reserve(16));
    int32_t *scalars = m->flags.as<int32_t>();     // [0]: special rows, [1]: largest SURF norm
    OSFM_HIP_CHECK(hipMemsetAsync(scalars, 0, 8, s));
    view::launch_handoff_sift(s, d_sift, sift_map, n_sift, v.ns_pad, v.sift.as<int8_t>(), v.sift_corr.as<int32_t>(),
        v.sift_raw.as<int8_t>(), v.sift_raw_corr.as<int32_t>(), v.special_slot.as<int32_t>());
    view::launch_special_scan(s, v.special_slot.as<int32_t>(), n_sift, v.special_map.as<int32_t>(), scalars + 0);
    view::launch_handoff_surf(s, d_surf, surf_map, n_surf, v.nu_pad, v.surf.as<int8_t>(), v.surf_corr.as<int32_t>(), scalars + 1);
    if (n_sift + n_surf)
        OSFM_HIP_CHECK(hipMemcpyAsync(v.positions.ptr, d_positions, (size_t)(n_sift + n_surf) * 8, hipMemcpyDeviceToDevice, s));
    OSFM_HIP_CHECK(hipGetLastError());
    int32_t h_scalars[2] = {0, 0};
    OSFM_HIP_CHECK(hipMemcpyAsync(h_scalars, scalars, 8, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    v.n_special = h_scalars[0];
    if (v.n_special > 0) {
        OSFM_RETURN_IF(gather_special(v, s));
        OSFM_HIP_CHECK(hipGetLastError());
    }
    if (!v.ready) OSFM_HIP_CHECK(event_create(&v.ready, false));
    OSFM_HIP_CHECK(hipEventRecord(v.ready, s));
    v.surf_norm2_max = h_scalars[1];
    v.n_positions = n_sift + n_surf;
    v.set = true;
    m->cas_dirty = true;
    return OSFM_OK;
}

// View `view` of `src` (prepared, possibly on another device) into the same view of `dst`, array for array.
static int copy_view(osfm_matcher *dst, osfm_matcher *src, int view)
{
    std::lock_guard<std::mutex> lock(dst->up_mu);
    OSFM_HIP_CHECK(hipSetDevice(dst->device));
    const ViewData &a = src->views[view];
    ViewData &v = dst->views[view];
    hipStream_t s = dst->up_stream;
    v.set = false;
    v.ns = a.ns; v.nu = a.nu; v.ns_pad = a.ns_pad; v.nu_pad = a.nu_pad;
    v.n_special = a.n_special; v.surf_norm2_max = a.surf_norm2_max; v.n_positions = a.n_positions;
    OSFM_HIP_CHECK(hipStreamWaitEvent(s, a.ready, 0));
    const int sp_pad = a.n_special > 0 ? round_up(a.n_special, kRowsPerBlock) : 0;
    struct { DeviceBuffer *to; const DeviceBuffer *from; size_t bytes; } arrays[] = {
        {&v.sift, &a.sift, (size_t)a.ns_pad * 128}, {&v.sift_corr, &a.sift_corr, (size_t)a.ns_pad * 4},
        {&v.sift_raw, &a.sift_raw, (size_t)a.ns_pad * 128}, {&v.sift_raw_corr, &a.sift_raw_corr, (size_t)a.ns_pad * 4},
        {&v.surf, &a.surf, (size_t)a.nu_pad * 64}, {&v.surf_corr, &a.surf_corr, (size_t)a.nu_pad * 4},
        {&v.special, &a.special, (size_t)sp_pad * 128}, {&v.special_corr, &a.special_corr, (size_t)sp_pad * 4},
        {&v.special_map, &a.special_map, sp_pad ? (size_t)a.n_special * 4 : 0},
        {&v.special_slot, &a.special_slot, sp_pad ? (size_t)a.ns * 4 : 0},
        {&v.positions, &a.positions, (size_t)std::max(a.n_positions, 0) * 8},
    };
    for (auto &r : arrays) {
        if (!r.bytes) continue;
        OSFM_RETURN_IF(r.to->reserve(r.bytes));
        OSFM_HIP_CHECK(hipMemcpyAsync(r.to->ptr, r.from->ptr, r.bytes, hipMemcpyDefault, s));
    }
    if (!v.ready) OSFM_HIP_CHECK(event_create(&v.ready, false));
    OSFM_HIP_CHECK(hipEventRecord(v.ready, s));
    v.set = true;
    dst->cas_dirty = true;
    return OSFM_OK;
}

// The device hand-off on a matcher of one or several shards: prepared once, on the first shard on `device`, and
// copied to the others.  begin / end bracket the reads of the source arrays on that shard's upload stream.
int handoff_all(osfm_matcher *m, int view, int device, const float *d_sift, const int32_t *sift_map, int n_sift,
    const float *d_surf, const int32_t *surf_map, int n_surf, const float *d_positions,
    const std::function<int(hipStream_t)> &begin, const std::function<int(hipStream_t)> &end)
{
    osfm_matcher *first = m;
    if (!m->shards.empty()) {
        first = nullptr;
        for (auto *sh : m->shards)
            if (sh->device == device) { first = sh; break; }
    }
    if (!first || first->device != device) {
        set_error("set_view_from_front: the descriptors are on device %d, which is none of the matcher's", device);
        return OSFM_E_ARG;
    }
    if (view < 0 || view >= (int)first->views.size()) {
        set_error("set_view_from_front: view id %d out of range", view);
        return OSFM_E_ARG;
    }
    {
        std::lock_guard<std::mutex> lock(first->up_mu);
        OSFM_HIP_CHECK(hipSetDevice(first->device));
        OSFM_RETURN_IF(begin(first->up_stream));
        const int rc = handoff_view(first, view, d_sift, sift_map, n_sift, d_surf, surf_map, n_surf, d_positions);
        OSFM_RETURN_IF(end(first->up_stream));
        OSFM_RETURN_IF(rc);
    }
    for (auto *sh : m->shards)
        if (sh != first) OSFM_RETURN_IF(copy_view(sh, first, view));
    return OSFM_OK;
}

// CascadeHashing::init (cascade_hashing.cc:33-70) for the views set so far.
// The projection matrices are drawn on the host with the same standard-library
// facilities the reference uses (std::mt19937(0) + std::normal_distribution<>,
// cascade_hashing.h:225-254): the distribution's algorithm is the library's,
// so the values equal the reference's when both are built against libstdc++.
static int build_cashash(osfm_matcher *m)
{
    OSFM_HIP_CHECK(hipStreamSynchronize(m->up_stream));       // the hashes are built from every view
    hipStream_t s = m->stream;
    for (int type = 0; type < 2; ++type) {
        const int dim = type == 0 ? 128 : 64;
        const int np = dim + kCasSecBits;
        if (!m->cas_proj[type].ptr) {
            std::mt19937 prng(0);
            std::normal_distribution<> dis(0, 1);
            std::vector<float> projT((size_t)dim * np);
            for (int i = 0; i < dim; ++i)                    // primary: prim_hash[i][j]
                for (int j = 0; j < dim; ++j) projT[(size_t)j * np + i] = (float)dis(prng);
            for (int g = 0; g < kCasGroups; ++g)             // secondary: sec_hash[g][i][j]
                for (int i = 0; i < kCasBits; ++i)
                    for (int j = 0; j < dim; ++j) projT[(size_t)j * np + dim + g * kCasBits + i] = (float)dis(prng);
            OSFM_RETURN_IF(m->cas_proj[type].reserve(projT.size() * 4));
            OSFM_HIP_CHECK(hipMemcpy(m->cas_proj[type].ptr, projT.data(), projT.size() * 4, hipMemcpyHostToDevice));
            OSFM_RETURN_IF(m->cas_sum[type].reserve(128 * 4));
            OSFM_RETURN_IF(m->cas_avg[type].reserve(128 * 4));
        }
        // compute_avg_descriptors: one running float sum per dimension over all views in order
        OSFM_HIP_CHECK(hipMemsetAsync(m->cas_sum[type].ptr, 0, 128 * 4, s));
        int64_t total = 0;
        for (auto &v : m->views) {
            if (!v.set) continue;
            const int n = type == 0 ? v.ns : v.nu;
            total += n;
            launch_cashash_accumulate((type == 0 ? v.sift : v.surf).as<int8_t>(), n, dim, type == 0 ? 128 : 0,
                type == 0 ? 255.0f : 127.0f, m->cas_sum[type].as<float>(), s);
        }
        launch_cashash_average(m->cas_sum[type].as<float>(), dim, total, m->cas_avg[type].as<float>(), s);
        for (auto &v : m->views) {
            if (!v.set) continue;
            const int n = type == 0 ? v.ns : v.nu;
            if (n >= (1 << 17)) {
                // candidate keys hold the position inside a bucket list in 17 bits
                set_error("cascade hashing: %d descriptors of one type in a view, at most %d supported", n, (1 << 17) - 1);
                return OSFM_E_RANGE;
            }
            OSFM_RETURN_IF(v.cas_hash[type].reserve((size_t)std::max(n, 1) * (dim / 64) * 8));
            OSFM_RETURN_IF(v.cas_bucket[type].reserve((size_t)std::max(n, 1) * kCasGroups));
            OSFM_RETURN_IF(v.cas_start[type].reserve((size_t)kCasGroups * (kCasBuckets + 1) * 4));
            OSFM_RETURN_IF(v.cas_items[type].reserve((size_t)std::max(n, 1) * kCasGroups * 4));
            launch_cashash_hash((type == 0 ? v.sift : v.surf).as<int8_t>(), n, dim, type == 0 ? 128 : 0,
                type == 0 ? 255.0f : 127.0f, m->cas_avg[type].as<float>(), m->cas_proj[type].as<float>(),
                v.cas_hash[type].as<uint64_t>(), v.cas_bucket[type].as<uint8_t>(), s);
            launch_cashash_buckets(v.cas_bucket[type].as<uint8_t>(), n, v.cas_start[type].as<int32_t>(),
                v.cas_items[type].as<int32_t>(), s);
            OSFM_RETURN_IF(v.cas_rec[type].reserve((size_t)std::max(n, 1) * sizeof(CasRecord)));
            launch_cashash_pack(v.cas_hash[type].as<uint64_t>(), v.cas_bucket[type].as<uint8_t>(), n, dim / 64,
                static_cast<CasRecord *>(v.cas_rec[type].ptr), s);
        }
    }
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    return OSFM_OK;
}

// The average descriptor -- and with it every hash -- is taken over ALL views (CascadeHashing::init receives the whole
// viewport list, cascade_hashing.cc:33-70), so a cascade batch needs the complete bank: a slot that was never set
// is an error, not an empty view, and no upload may run beside the build (uploads mutate the views under up_mu; the
// flag is cleared BEFORE the build so that an upload that follows raises it again and is not lost).
int ensure_cashash(osfm_matcher *m)
{
    std::lock_guard<std::mutex> lock(m->up_mu);
    for (size_t v = 0; v < m->views.size(); ++v)
        if (!m->views[v].set) {
            set_error("cascade hashing: view %d of %d has not been set (the hashes depend on the average descriptor of ALL views)",
                (int)v, (int)m->views.size());
            return OSFM_E_STATE;
        }
    if (!m->cas_dirty.exchange(false)) return OSFM_OK;
    const int rc = build_cashash(m);
    if (rc != OSFM_OK) m->cas_dirty = true;
    return rc;
}

}  // namespace osfm
