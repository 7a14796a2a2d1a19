// C ABI of the view front end (include/osfm_hip.h, "View front end"): owns the image buffers of the halving chain,
// a SIFT and a SURF context and the arrays of one view, and runs bundler::Features::compute's steps on them.
#include <cstring>
#include <memory>

#include "feature_device.h"
#include "osfm_common.h"
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
    // the last load
    bool have = false;
    int import_w = 0, import_h = 0, feat_w = 0, feat_h = 0, channels = 0, n_sift = 0, n_surf = 0;
    const uint8_t *d_image = nullptr;
    DeviceFeatures fs, fu;
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

int load(osfm_view_front *c, const uint8_t *pixels, int width, int height, int channels, osfm_view_summary *sum_out)
{
    int iw, ih, fw, fh, halvings;
    if (!plan_chain(c->opts, width, height, &iw, &ih, &fw, &fh, &halvings)) {
        set_error("osfm_view_front_load: the halving chain of a %d x %d image reaches a side below 2, which the reference "
            "refuses to halve", width, height);
        return OSFM_E_ARG;
    }
    hipStream_t s = c->stream;
    // a hand-off that still reads the previous load's arrays: this load's work queues behind it, the host does not wait
    if (c->read_pending) {
        OSFM_HIP_CHECK(hipStreamWaitEvent(s, c->read_done, 0));
        c->read_pending = false;
    }
    OSFM_HIP_CHECK(hipMemcpyAsync(c->img[0].ptr, pixels, (size_t)width * height * channels, hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipEventRecord(c->ev[0], s));
    int cur = 0, w = width, h = height;
    for (int i = 0; i < halvings; ++i) {
        view::launch_halve(s, c->img[cur].as<uint8_t>(), w, h, channels, c->img[cur ^ 1].as<uint8_t>());
        half(&w, &h);
        cur ^= 1;
    }
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(c->ev[1], s));
    const uint8_t *d_image = c->img[cur].as<uint8_t>();

    osfm_view_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    c->fs = DeviceFeatures(); c->fu = DeviceFeatures();
    if (c->sift) {
        OSFM_RETURN_IF(sift_extract_device(c->sift, d_image, c->ev[1], fw, fh, channels, &sum.sift));
        OSFM_RETURN_IF(sift_device_features(c->sift, &c->fs));
    }
    if (c->surf) {
        OSFM_RETURN_IF(surf_extract_device(c->surf, d_image, c->ev[1], fw, fh, channels, &sum.surf));
        OSFM_RETURN_IF(surf_device_features(c->surf, &c->fu));
    }
    OSFM_HIP_CHECK(hipSetDevice(c->device));

    // FeatureSet's order on the host (the detectors keep the order by scale there): a few bytes per feature go up,
    // the descriptors stay where they are
    const int ns = c->fs.n, nu = c->fu.n, n = ns + nu;
    if ((size_t)n > c->max_features) { set_error("osfm_view_front_load: internal: %d features exceed the arrays", n); return OSFM_E_STATE; }
    c->h_positions.resize((size_t)n * 2); c->h_scale.resize((size_t)n); c->h_orientation.resize((size_t)n);
    c->h_sift_map.resize((size_t)ns); c->h_surf_map.resize((size_t)nu);
    auto rows = [&](const DeviceFeatures &f, int base, std::vector<int32_t> *map) {
        for (int i = 0; i < f.n; ++i) {
            const size_t g = (size_t)(*f.order)[(size_t)i], o = (size_t)(base + i);
            c->h_positions[2 * o] = (*f.positions)[2 * g]; c->h_positions[2 * o + 1] = (*f.positions)[2 * g + 1];
            c->h_scale[o] = (*f.scale)[g]; c->h_orientation[o] = (*f.orientation)[g];
            (*map)[(size_t)i] = f.rows ? (*f.rows)[g] : (int32_t)g;
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
    c->have = true;
    if (sum_out) *sum_out = sum;
    return OSFM_OK;
}

// rows map[0..n) of a detector's descriptor array, `dim` floats each, into out
int download_rows(osfm_view_front *c, const float *desc, const std::vector<int32_t> &map, int dim, float *out)
{
    if (map.empty()) return OSFM_OK;
    const size_t last = (size_t)*std::max_element(map.begin(), map.end()) + 1;
    std::vector<float> gen(last * dim);
    OSFM_HIP_CHECK(hipMemcpyAsync(gen.data(), desc, gen.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < map.size(); ++i) std::memcpy(out + i * dim, gen.data() + (size_t)map[i] * dim, (size_t)dim * sizeof(float));
    return OSFM_OK;
}

}  // namespace

namespace osfm {

int view_front_result(osfm_view_front *c, FrontResult *out)
{
    if (!c || !out) { set_error("osfm_view_front: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_view_front: no load to hand off"); return OSFM_E_STATE; }
    out->device = c->device;
    out->sift_desc = c->fs.desc; out->surf_desc = c->fu.desc; out->normalized = c->normalized.as<float>();
    out->sift_map = c->sift_map.as<int32_t>(); out->surf_map = c->surf_map.as<int32_t>();
    out->n_sift = c->n_sift; out->n_surf = c->n_surf;
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
    if (max_width < 1 || max_height < 1 || max_width > 16384 || max_height > 16384) {
        set_error("osfm_view_front_create: image size %d x %d outside 1..16384", max_width, max_height);
        return OSFM_E_ARG;
    }
    if (vo.downscale_factor < 1 || vo.downscale_factor > 16 || vo.feature_types < 1 || vo.feature_types > OSFM_FEATURE_ALL) {
        set_error("osfm_view_front_create: invalid options (downscale_factor 1..16, feature_types 1..3)");
        return OSFM_E_ARG;
    }
    int ndev = 0;
    OSFM_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("osfm_view_front_create: device %d of %d", device, ndev); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
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
    }
    if (vo.feature_types & OSFM_FEATURE_SURF) {
        OSFM_RETURN_IF(osfm_surf_create(device, dw, dh, &uo, &c->surf));
        c->max_features += (size_t)uo.max_keypoints;
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
    if (!c || !pixels) { set_error("osfm_view_front_load: null argument"); return OSFM_E_ARG; }
    c->have = false;          // whatever comes of this call, the previous result is gone
    if (channels != 1 && channels != 3) {
        set_error("osfm_view_front_load: %d channels: a grey (1) or colour (3) image is expected", channels);
        return OSFM_E_ARG;
    }
    if (width < 1 || height < 1) { set_error("osfm_view_front_load: image size %d x %d", width, height); return OSFM_E_ARG; }
    if (width > c->max_w || height > c->max_h) {
        set_error("osfm_view_front_load: a %d x %d image exceeds the front end's %d x %d", width, height, c->max_w, c->max_h);
        return OSFM_E_RANGE;
    }
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const int rc = load(c, pixels, width, height, channels, summary);
    if (rc != OSFM_OK) (void)hipStreamSynchronize(c->stream);   // nothing of a failed call may still run
    return rc;
}

int osfm_view_front_download(osfm_view_front *c, float *positions, float *normalized, uint8_t *colors, float *scale,
    float *orientation, float *sift_descriptors, float *surf_descriptors)
{
    if (!c) { set_error("osfm_view_front_download: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_view_front_download: no load to download"); return OSFM_E_STATE; }
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_sift + c->n_surf;
    if (positions && n) std::memcpy(positions, c->h_positions.data(), n * 8);
    if (scale && n) std::memcpy(scale, c->h_scale.data(), n * 4);
    if (orientation && n) std::memcpy(orientation, c->h_orientation.data(), n * 4);
    if (normalized && n) OSFM_HIP_CHECK(hipMemcpyAsync(normalized, c->normalized.ptr, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (colors && n) OSFM_HIP_CHECK(hipMemcpyAsync(colors, c->colors.ptr, n * 3, hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (sift_descriptors) OSFM_RETURN_IF(download_rows(c, c->fs.desc, c->h_sift_map, 128, sift_descriptors));
    if (surf_descriptors) OSFM_RETURN_IF(download_rows(c, c->fu.desc, c->h_surf_map, 64, surf_descriptors));
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
