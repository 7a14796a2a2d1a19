// C ABI of the view front end (include/osfm_hip.h, "View front end"): owns the image buffers of the halving chain,
// a SIFT and a SURF context and the arrays of one view, and runs bundler::Features::compute's steps on them.
#include <cstring>
#include <memory>

#include "detector_context.h"
#include "feature_device.h"
#include "feature_view.h"
#include "view_front.h"
#include "view_kernels.h"

using namespace osfm;

struct osfm_view_front {
    int device = 0, max_w = 0, max_h = 0;
    osfm_view_options opts{};
    osfm_sift *sift = nullptr;
    osfm_surf *surf = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};                 // timing: chain begin / end, view kernel begin / end (the end: the load is ready)
    hipEvent_t read_done = nullptr;        // recorded by a reader of the arrays (view_front_end_read)
    bool read_pending = false;
    size_t max_features = 0;
    DeviceBuffer img[2], positions, normalized, colors, sift_map, surf_map;
    // osfm_view_front_load_marked: reserved by the first call that needs them.  img_keep: the third image buffer of
    // a chain that would overwrite the import image; kept: the second set of arrays of OSFM_MARK_FEATURES
    DeviceBuffer img_keep, mask, pixel_xy, pixel_rgb, mark, mark_counts, kept_index;
    DeviceBuffer kept[8];                  // positions, normalized, colors, sift_map, surf_map, pixel_xy, pixel_rgb, mark
    // the last load
    bool have = false;
    int import_w = 0, import_h = 0, feat_w = 0, feat_h = 0, channels = 0, n_sift = 0, n_surf = 0;
    const uint8_t *d_image = nullptr;
    bool have_marks = false, compacted = false;
    bool host_rows_stale = false;          // compacted: the host arrays below still hold every row of the detectors
    const DetectorContext *fs = nullptr, *fu = nullptr;     // the detectors' results (NULL: no such detector)
    std::vector<float> h_positions, h_scale, h_orientation;     // FeatureSet's order, SIFT rows first
    std::vector<int32_t> h_sift_map, h_surf_map;
    ~osfm_view_front()
    {
        (void)osfm_sift_destroy(sift);
        (void)osfm_surf_destroy(surf);
        for (auto &e : ev) event_destroy(e);
        event_destroy(read_done);
        stream_destroy(stream);
    }
};

namespace {

void half(int *w, int *h) { *w = (*w + 1) >> 1; *h = (*h + 1) >> 1; }

const float *desc_of(const DetectorContext *f) { return f ? f->desc.as<float>() : nullptr; }

// bundler::Features::compute's chain on a size: downscale_factor - 1 halvings (downscale_image), then halvings
// while width * height > max_image_size, in int as in the reference.  False where rescale_half_size throws.
bool plan_chain(const osfm_view_options &o, int w, int h, int *import_w, int *import_h, int *out_w, int *out_h, int *halvings)
{
    int n = 0;
    for (int i = 1; i < o.downscale_factor; ++i, ++n) {
        if (w < 2 || h < 2) return false;
        half(&w, &h);
    }
    *import_w = w; *import_h = h;
    while (o.max_image_size > 0 && w * h > o.max_image_size) {
        if (w < 2 || h < 2) return false;
        half(&w, &h);
        ++n;
    }
    *out_w = w; *out_h = h; *halvings = n;
    return true;
}

// What osfm_view_front_load_marked adds to a load.
struct MarkRequest {
    const uint8_t *mask;
    int mask_w, mask_h;
    osfm_view_mark_options opts;
    osfm_view_mark_summary *out;
};

view::ViewRows rows_of(osfm_view_front *c, bool kept)
{
    view::ViewRows r;
    if (kept) {
        r.positions = c->kept[0].as<float>(); r.normalized = c->kept[1].as<float>(); r.colors = c->kept[2].as<uint8_t>();
        r.sift_map = c->kept[3].as<int32_t>(); r.surf_map = c->kept[4].as<int32_t>(); r.pixel_xy = c->kept[5].as<float>();
        r.pixel_rgb = c->kept[6].as<uint8_t>(); r.mark = c->kept[7].as<uint8_t>();
    } else {
        r.positions = c->positions.as<float>(); r.normalized = c->normalized.as<float>(); r.colors = c->colors.as<uint8_t>();
        r.sift_map = c->sift_map.as<int32_t>(); r.surf_map = c->surf_map.as<int32_t>(); r.pixel_xy = c->pixel_xy.as<float>();
        r.pixel_rgb = c->pixel_rgb.as<uint8_t>(); r.mark = c->mark.as<uint8_t>();
    }
    return r;
}

int load(osfm_view_front *c, const uint8_t *pixels, int width, int height, int channels, osfm_view_summary *sum_out,
    const MarkRequest *marks)
{
    int iw, ih, fw, fh, halvings;
    if (!plan_chain(c->opts, width, height, &iw, &ih, &fw, &fh, &halvings)) {
        set_error("osfm_view_front_load: the halving chain of a %d x %d image reaches a side below 2, which the reference "
            "refuses to halve", width, height);
        return OSFM_E_ARG;
    }
    hipStream_t s = c->stream;
    // the marks read the import image after the detectors have run: where the chain goes on for two or more
    // halvings behind it, these alternate between the other buffer and a third one
    const int import_at = c->opts.downscale_factor - 1;
    const bool keep_import = marks && halvings - import_at >= 2;
    if (marks) {
        const size_t K = c->max_features;
        const bool features = marks->opts.mode == OSFM_MARK_FEATURES;
        if (keep_import) OSFM_RETURN_IF(c->img_keep.reserve((size_t)((iw + 3) >> 2) * ((ih + 3) >> 2) * channels));
        if (marks->mask) OSFM_RETURN_IF(c->mask.reserve((size_t)marks->mask_w * marks->mask_h));
        OSFM_RETURN_IF(c->pixel_xy.reserve(K * 8));
        OSFM_RETURN_IF(c->pixel_rgb.reserve(K * 3));
        OSFM_RETURN_IF(c->mark.reserve(K));
        OSFM_RETURN_IF(c->mark_counts.reserve(32));
        if (features && marks->mask) {
            const size_t row_bytes[8] = {8, 8, 3, 4, 4, 8, 3, 1};
            for (int k = 0; k < 8; ++k) OSFM_RETURN_IF(c->kept[k].reserve(K * row_bytes[k]));
            OSFM_RETURN_IF(c->kept_index.reserve(K * 4));
        }
    }
    // a hand-off that still reads the previous load's arrays: this load's work queues behind it, the host does not wait
    if (c->read_pending) {
        OSFM_HIP_CHECK(hipStreamWaitEvent(s, c->read_done, 0));
        c->read_pending = false;
    }
    OSFM_HIP_CHECK(hipMemcpyAsync(c->img[0].ptr, pixels, (size_t)width * height * channels, hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipEventRecord(c->ev[0], s));
    if (marks && marks->mask)
        OSFM_HIP_CHECK(hipMemcpyAsync(c->mask.ptr, marks->mask, (size_t)marks->mask_w * marks->mask_h, hipMemcpyHostToDevice, s));
    uint8_t *bufs[3] = {c->img[0].as<uint8_t>(), c->img[1].as<uint8_t>(), c->img_keep.as<uint8_t>()};
    int cur = 0, w = width, h = height;
    const uint8_t *d_import = bufs[0];
    for (int i = 0; i < halvings; ++i) {
        // without keep_import: the two buffers in turn.  With it, from the second halving behind the import image
        // on, the buffer that is neither the import image's nor the current one
        int to = cur ^ 1;
        if (keep_import && i > import_at) to = 3 - (import_at & 1) - cur;
        view::launch_halve(s, bufs[cur], w, h, channels, bufs[to]);
        half(&w, &h);
        cur = to;
        if (i + 1 == import_at) d_import = bufs[cur];
    }
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(c->ev[1], s));
    const uint8_t *d_image = bufs[cur];

    osfm_view_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    if (c->sift) OSFM_RETURN_IF(sift_extract_device(c->sift, d_image, c->ev[1], fw, fh, channels, &sum.sift));
    if (c->surf) OSFM_RETURN_IF(surf_extract_device(c->surf, d_image, c->ev[1], fw, fh, channels, &sum.surf));
    OSFM_HIP_CHECK(hipSetDevice(c->device));

    // FeatureSet's order on the host (the detectors keep the order by scale there): a few bytes per feature go up,
    // the descriptors stay where they are
    const int ns = c->fs ? c->fs->n_desc : 0, nu = c->fu ? c->fu->n_desc : 0, n = ns + nu;
    if ((size_t)n > c->max_features) { set_error("osfm_view_front_load: internal: %d features exceed the arrays", n); return OSFM_E_STATE; }
    c->h_positions.resize((size_t)n * 2); c->h_scale.resize((size_t)n); c->h_orientation.resize((size_t)n);
    c->h_sift_map.resize((size_t)ns); c->h_surf_map.resize((size_t)nu);
    auto rows = [&](const DetectorContext *f, int base, std::vector<int32_t> *map) {
        for (size_t i = 0; i < map->size(); ++i) {
            const size_t g = (size_t)f->order[i], o = (size_t)base + i;
            c->h_positions[2 * o] = f->positions[2 * g]; c->h_positions[2 * o + 1] = f->positions[2 * g + 1];
            c->h_scale[o] = f->scale[g]; c->h_orientation[o] = f->orientation[g];
            (*map)[i] = f->desc_row(g);
        }
    };
    rows(c->fs, 0, &c->h_sift_map);
    rows(c->fu, ns, &c->h_surf_map);
    if (n) OSFM_HIP_CHECK(hipMemcpyAsync(c->positions.ptr, c->h_positions.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (ns) OSFM_HIP_CHECK(hipMemcpyAsync(c->sift_map.ptr, c->h_sift_map.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
    if (nu) OSFM_HIP_CHECK(hipMemcpyAsync(c->surf_map.ptr, c->h_surf_map.data(), (size_t)nu * 4, hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipEventRecord(c->ev[2], s));
    view::launch_view_rows(s, d_image, fw, fh, channels, c->positions.as<float>(), n, c->colors.as<uint8_t>(),
        c->normalized.as<float>());
    OSFM_HIP_CHECK(hipGetLastError());
    int32_t h_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // [0..2]: the marks kernel's, [4..5]: the compaction's
    bool compacted = false;
    int pixel_width = 0;
    if (marks) {
        const osfm_view_mark_options &mo = marks->opts;
        pixel_width = mo.pixel_width > 0 ? mo.pixel_width : iw;
        int32_t *counts = c->mark_counts.as<int32_t>();
        OSFM_HIP_CHECK(hipMemsetAsync(counts, 0, 32, s));
        view::launch_view_marks(s, c->normalized.as<float>(), n, ns, (double)pixel_width, d_import, iw, ih, channels,
            marks->mask ? c->mask.as<uint8_t>() : nullptr, marks->mask_w, marks->mask_h, mo.clamp, mo.threshold,
            c->pixel_xy.as<float>(), c->pixel_rgb.as<uint8_t>(), c->mark.as<uint8_t>(), counts);
        // a view without a mask keeps every row: nothing to move
        compacted = mo.mode == OSFM_MARK_FEATURES && marks->mask && n > 0;
        if (compacted) view::launch_compact_rows(s, rows_of(c, false), ns, nu, rows_of(c, true), c->kept_index.as<int32_t>(), counts + 4);
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipMemcpyAsync(h_counts, counts, 32, hipMemcpyDeviceToHost, s));
    }
    OSFM_HIP_CHECK(hipEventRecord(c->ev[3], s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));

    float chain_ms = 0.0f, view_ms = 0.0f;
    OSFM_HIP_CHECK(hipEventElapsedTime(&chain_ms, c->ev[0], c->ev[1]));
    OSFM_HIP_CHECK(hipEventElapsedTime(&view_ms, c->ev[2], c->ev[3]));
    sum.import_width = iw; sum.import_height = ih; sum.feature_width = fw; sum.feature_height = fh;
    sum.num_halvings = halvings; sum.num_sift = ns; sum.num_surf = nu;
    sum.halving_ms = chain_ms; sum.view_ms = view_ms;
    sum.total_ms = (double)chain_ms + view_ms + sum.sift.total_ms + sum.surf.total_ms;
    c->import_w = iw; c->import_h = ih; c->feat_w = fw; c->feat_h = fh; c->channels = channels;
    c->n_sift = ns; c->n_surf = nu; c->d_image = d_image;
    c->have_marks = marks != nullptr; c->compacted = compacted; c->host_rows_stale = compacted;
    if (marks) {
        osfm_view_mark_summary ms;
        std::memset(&ms, 0, sizeof(ms));
        ms.masked_out_sift = h_counts[0]; ms.masked_out_surf = h_counts[1]; ms.outside = h_counts[2];
        ms.kept_sift = compacted ? h_counts[4] : ns; ms.kept_surf = compacted ? h_counts[5] : nu;
        ms.has_mask = marks->mask != nullptr; ms.pixel_width = pixel_width;
        if (compacted && (ms.kept_sift != ns - ms.masked_out_sift || ms.kept_surf != nu - ms.masked_out_surf)) {
            set_error("osfm_view_front_load_marked: internal: %d + %d rows kept, %d + %d of %d + %d masked out", ms.kept_sift,
                ms.kept_surf, ms.masked_out_sift, ms.masked_out_surf, ns, nu);
            return OSFM_E_STATE;
        }
        c->n_sift = ms.kept_sift; c->n_surf = ms.kept_surf;
        sum.num_sift = ms.kept_sift; sum.num_surf = ms.kept_surf;
        if (marks->out) *marks->out = ms;
    }
    c->have = true;
    if (sum_out) *sum_out = sum;
    return OSFM_OK;
}

// After a load that moved the kept rows together on the device, the host's arrays follow on the first download: the
// load itself waits for the two counts alone.
int refresh_host_rows(osfm_view_front *c)
{
    if (!c->host_rows_stale) return OSFM_OK;
    const size_t ns = (size_t)c->n_sift, nu = (size_t)c->n_surf, n = ns + nu;
    std::vector<int32_t> index(n), sift_map(ns), surf_map(nu);
    if (n) OSFM_HIP_CHECK(hipMemcpyAsync(index.data(), c->kept_index.ptr, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (ns) OSFM_HIP_CHECK(hipMemcpyAsync(sift_map.data(), c->kept[3].ptr, ns * 4, hipMemcpyDeviceToHost, c->stream));
    if (nu) OSFM_HIP_CHECK(hipMemcpyAsync(surf_map.data(), c->kept[4].ptr, nu * 4, hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {            // index ascends and index[i] >= i: in place
        const size_t r = (size_t)index[i];
        c->h_positions[2 * i] = c->h_positions[2 * r]; c->h_positions[2 * i + 1] = c->h_positions[2 * r + 1];
        c->h_scale[i] = c->h_scale[r]; c->h_orientation[i] = c->h_orientation[r];
    }
    c->h_positions.resize(n * 2); c->h_scale.resize(n); c->h_orientation.resize(n);
    c->h_sift_map.swap(sift_map); c->h_surf_map.swap(surf_map);
    c->host_rows_stale = false;
    return OSFM_OK;
}

int check_load_args(osfm_view_front *c, const uint8_t *pixels, int width, int height, int channels, const char *who)
{
    if (!c || !pixels) { set_error("%s: null argument", who); return OSFM_E_ARG; }
    c->have = false;          // whatever comes of this call, the previous result is gone
    c->have_marks = false;
    return check_image(who, "front end", c->max_w, c->max_h, width, height, channels);
}

}  // namespace

namespace osfm {

int view_front_result(osfm_view_front *c, FrontResult *out)
{
    if (!c || !out) { set_error("osfm_view_front: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_view_front: no load to hand off"); return OSFM_E_STATE; }
    out->device = c->device;
    const view::ViewRows rows = rows_of(c, c->compacted);
    out->sift_desc = desc_of(c->fs); out->surf_desc = desc_of(c->fu); out->normalized = rows.normalized;
    out->sift_map = rows.sift_map; out->surf_map = rows.surf_map;
    out->n_sift = c->n_sift; out->n_surf = c->n_surf;
    return OSFM_OK;
}

int view_front_image(osfm_view_front *c, FrontImage *out)
{
    if (!c || !out) { set_error("osfm_view_front: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_view_front: no load whose image could be handed off"); return OSFM_E_STATE; }
    out->device = c->device; out->pixels = c->d_image;
    out->width = c->feat_w; out->height = c->feat_h; out->channels = c->channels;
    return OSFM_OK;
}

int view_front_begin_read(osfm_view_front *c, hipStream_t reader)
{
    OSFM_HIP_CHECK(hipStreamWaitEvent(reader, c->ev[3], 0));
    // one event serves every reader: a second one queues behind the first, so that the last record covers both
    if (c->read_pending) OSFM_HIP_CHECK(hipStreamWaitEvent(reader, c->read_done, 0));
    return OSFM_OK;
}

int view_front_end_read(osfm_view_front *c, hipStream_t reader)
{
    OSFM_HIP_CHECK(hipEventRecord(c->read_done, reader));
    c->read_pending = true;
    return OSFM_OK;
}

}  // namespace osfm

extern "C" {

int osfm_view_options_default(osfm_view_options *o)
{
    if (!o) { set_error("osfm_view_options_default: null argument"); return OSFM_E_ARG; }
    o->downscale_factor = 1;
    o->max_image_size = 6000000;
    o->feature_types = OSFM_FEATURE_ALL;
    return OSFM_OK;
}

int osfm_view_front_create(int device, int max_width, int max_height, const osfm_view_options *view_opts,
    const osfm_sift_options *sift_opts, const osfm_surf_options *surf_opts, osfm_view_front **out)
{
    if (!out) { set_error("osfm_view_front_create: null argument"); return OSFM_E_ARG; }
    *out = nullptr;
    osfm_view_options vo;
    (void)osfm_view_options_default(&vo);
    if (view_opts) vo = *view_opts;
    OSFM_RETURN_IF(check_bounds("osfm_view_front_create", max_width, max_height));
    if (vo.downscale_factor < 1 || vo.downscale_factor > 16 || vo.feature_types < 1 || vo.feature_types > OSFM_FEATURE_ALL) {
        set_error("osfm_view_front_create: invalid options (downscale_factor 1..16, feature_types 1..3)");
        return OSFM_E_ARG;
    }
    OSFM_RETURN_IF(select_device("osfm_view_front_create", device));
    std::unique_ptr<osfm_view_front> c(new osfm_view_front);
    c->device = device; c->max_w = max_width; c->max_h = max_height; c->opts = vo;
    // the detectors' bound: the input bound after the fixed halvings (an image under max_image_size passes the loop
    // unhalved, so the loop lowers no bound)
    int dw = max_width, dh = max_height;
    for (int i = 1; i < vo.downscale_factor; ++i) half(&dw, &dh);
    osfm_sift_options so;
    osfm_surf_options uo;
    (void)osfm_sift_options_default(&so);
    (void)osfm_surf_options_default(&uo);
    if (sift_opts) so = *sift_opts;
    if (surf_opts) uo = *surf_opts;
    if (vo.feature_types & OSFM_FEATURE_SIFT) {
        OSFM_RETURN_IF(osfm_sift_create(device, dw, dh, &so, &c->sift));
        c->max_features += (size_t)so.max_keypoints;
        c->fs = detector_of(c->sift);
    }
    if (vo.feature_types & OSFM_FEATURE_SURF) {
        OSFM_RETURN_IF(osfm_surf_create(device, dw, dh, &uo, &c->surf));
        c->max_features += (size_t)uo.max_keypoints;
        c->fu = detector_of(c->surf);
    }
    const size_t K = c->max_features;
    OSFM_RETURN_IF(c->img[0].reserve((size_t)max_width * max_height * 3));
    OSFM_RETURN_IF(c->img[1].reserve((size_t)((max_width + 1) >> 1) * ((max_height + 1) >> 1) * 3));
    OSFM_RETURN_IF(c->positions.reserve(K * 8));
    OSFM_RETURN_IF(c->normalized.reserve(K * 8));
    OSFM_RETURN_IF(c->colors.reserve(K * 3));
    OSFM_RETURN_IF(c->sift_map.reserve(K * 4));
    OSFM_RETURN_IF(c->surf_map.reserve(K * 4));
    OSFM_HIP_CHECK(stream_create(&c->stream));
    for (auto &e : c->ev) OSFM_HIP_CHECK(event_create(&e, true));
    OSFM_HIP_CHECK(event_create(&c->read_done, false));
    *out = c.release();
    return OSFM_OK;
}

int osfm_view_front_destroy(osfm_view_front *c)
{
    if (!c) return OSFM_OK;
    (void)hipSetDevice(c->device);
    if (c->read_pending) (void)hipEventSynchronize(c->read_done);   // a hand-off may still read the arrays
    delete c;
    return OSFM_OK;
}

int osfm_view_front_load(osfm_view_front *c, const uint8_t *pixels, int width, int height, int channels, osfm_view_summary *summary)
{
    OSFM_RETURN_IF(check_load_args(c, pixels, width, height, channels, "osfm_view_front_load"));
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const int rc = load(c, pixels, width, height, channels, summary, nullptr);
    if (rc != OSFM_OK) (void)hipStreamSynchronize(c->stream);   // nothing of a failed call may still run
    return rc;
}

int osfm_view_mark_options_default(osfm_view_mark_options *o)
{
    if (!o) { set_error("osfm_view_mark_options_default: null argument"); return OSFM_E_ARG; }
    o->mode = OSFM_MARK_TRACKS;
    o->clamp = OSFM_CLAMP_REFERENCE;
    o->threshold = 16;
    o->pixel_width = 0;
    return OSFM_OK;
}

static int check_mark_args(const uint8_t *mask, int mask_w, int mask_h, const osfm_view_mark_options &o, const char *who)
{
    if (mask && (mask_w < 1 || mask_h < 1)) { set_error("%s: mask size %d x %d", who, mask_w, mask_h); return OSFM_E_ARG; }
    if ((o.mode != OSFM_MARK_TRACKS && o.mode != OSFM_MARK_FEATURES) || (o.clamp != OSFM_CLAMP_REFERENCE && o.clamp != OSFM_CLAMP_IMAGE) ||
        o.pixel_width < 0) {
        set_error("%s: invalid options (mode 0..1, clamp 0..1, pixel_width >= 0)", who);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

int osfm_view_front_load_marked(osfm_view_front *c, const uint8_t *pixels, int width, int height, int channels, const uint8_t *mask,
    int mask_width, int mask_height, const osfm_view_mark_options *opts, osfm_view_summary *summary, osfm_view_mark_summary *mark_summary)
{
    OSFM_RETURN_IF(check_load_args(c, pixels, width, height, channels, "osfm_view_front_load_marked"));
    MarkRequest req;
    (void)osfm_view_mark_options_default(&req.opts);
    if (opts) req.opts = *opts;
    req.mask = mask; req.mask_w = mask ? mask_width : 0; req.mask_h = mask ? mask_height : 0; req.out = mark_summary;
    OSFM_RETURN_IF(check_mark_args(mask, mask_width, mask_height, req.opts, "osfm_view_front_load_marked"));
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const int rc = load(c, pixels, width, height, channels, summary, &req);
    if (rc != OSFM_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}

int osfm_view_front_download_marks(osfm_view_front *c, float *pixel_xy, uint8_t *pixel_rgb, uint8_t *mark)
{
    if (!c) { set_error("osfm_view_front_download_marks: null argument"); return OSFM_E_ARG; }
    if (!c->have || !c->have_marks) {
        set_error("osfm_view_front_download_marks: no osfm_view_front_load_marked to download");
        return OSFM_E_STATE;
    }
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_sift + c->n_surf;
    const view::ViewRows rows = rows_of(c, c->compacted);
    if (pixel_xy && n) OSFM_HIP_CHECK(hipMemcpyAsync(pixel_xy, rows.pixel_xy, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (pixel_rgb && n) OSFM_HIP_CHECK(hipMemcpyAsync(pixel_rgb, rows.pixel_rgb, n * 3, hipMemcpyDeviceToHost, c->stream));
    if (mark && n) OSFM_HIP_CHECK(hipMemcpyAsync(mark, rows.mark, n, hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OSFM_OK;
}

int osfm_view_debug_mark_rows(int64_t n, const float *normalized, const uint8_t *pixels, int width, int height, int channels,
    const uint8_t *mask, int mask_width, int mask_height, const osfm_view_mark_options *opts, float *pixel_xy, uint8_t *pixel_rgb,
    uint8_t *mark)
{
    if (n < 0 || !pixels || (n > 0 && (!normalized || !pixel_xy || !pixel_rgb || !mark))) {
        set_error("osfm_view_debug_mark_rows: null argument / negative count");
        return OSFM_E_ARG;
    }
    if ((channels != 1 && channels != 3) || width < 1 || height < 1) {
        set_error("osfm_view_debug_mark_rows: a %d x %d image of %d channels", width, height, channels);
        return OSFM_E_ARG;
    }
    osfm_view_mark_options o;
    (void)osfm_view_mark_options_default(&o);
    if (opts) o = *opts;
    OSFM_RETURN_IF(check_mark_args(mask, mask_width, mask_height, o, "osfm_view_debug_mark_rows"));
    const double pixel_width = o.pixel_width > 0 ? o.pixel_width : width;
    for (int64_t i = 0; i < n; ++i)
        view_mark_row(normalized[2 * i], normalized[2 * i + 1], pixel_width, pixels, width, height, channels, mask, mask_width,
            mask_height, o.clamp, o.threshold, pixel_xy + 2 * i, mark + i, pixel_rgb + 3 * i);
    return OSFM_OK;
}

int osfm_view_front_download(osfm_view_front *c, float *positions, float *normalized, uint8_t *colors, float *scale,
    float *orientation, float *sift_descriptors, float *surf_descriptors)
{
    if (!c) { set_error("osfm_view_front_download: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_view_front_download: no load to download"); return OSFM_E_STATE; }
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    OSFM_RETURN_IF(refresh_host_rows(c));
    const size_t n = (size_t)c->n_sift + c->n_surf;
    const view::ViewRows rows = rows_of(c, c->compacted);
    if (positions && n) std::memcpy(positions, c->h_positions.data(), n * 8);
    if (scale && n) std::memcpy(scale, c->h_scale.data(), n * 4);
    if (orientation && n) std::memcpy(orientation, c->h_orientation.data(), n * 4);
    if (normalized && n) OSFM_HIP_CHECK(hipMemcpyAsync(normalized, rows.normalized, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (colors && n) OSFM_HIP_CHECK(hipMemcpyAsync(colors, rows.colors, n * 3, hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (sift_descriptors) OSFM_RETURN_IF(gather_descriptors(c->stream, desc_of(c->fs), c->h_sift_map, 128, sift_descriptors));
    if (surf_descriptors) OSFM_RETURN_IF(gather_descriptors(c->stream, desc_of(c->fu), c->h_surf_map, 64, surf_descriptors));
    return OSFM_OK;
}

int osfm_view_front_debug_image(osfm_view_front *c, uint8_t *out, int32_t *width, int32_t *height, int32_t *channels)
{
    if (!c) { set_error("osfm_view_front_debug_image: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_view_front_debug_image: no load"); return OSFM_E_STATE; }
    if (width) *width = c->feat_w;
    if (height) *height = c->feat_h;
    if (channels) *channels = c->channels;
    if (!out) return OSFM_OK;
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    OSFM_HIP_CHECK(hipMemcpyAsync(out, c->d_image, (size_t)c->feat_w * c->feat_h * c->channels, hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OSFM_OK;
}

}  // extern "C"
