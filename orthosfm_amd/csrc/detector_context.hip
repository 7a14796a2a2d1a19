// The detector-independent steps of the SIFT and the SURF context (see detector_context.h).
#include <cstring>

#include "detector_context.h"
#include "feature_view.h"

namespace osfm {

using detect::kBlock;
using detect::Keypoint;

int check_bounds(const char *api, int max_width, int max_height)
{
    if (max_width < 1 || max_height < 1 || max_width > 16384 || max_height > 16384) {
        set_error("%s: image size %d x %d outside 1..16384", api, max_width, max_height);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

int select_device(const char *api, int device)
{
    int ndev = 0;
    OSFM_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("%s: device %d of %d", api, device, ndev); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
    return OSFM_OK;
}

int init_detector(DetectorContext *c, int device, int max_width, int max_height, int max_keypoints, int extrema_blocks,
    int num_events)
{
    c->device = device; c->max_w = max_width; c->max_h = max_height; c->max_keypoints = max_keypoints;
    const size_t K = (size_t)max_keypoints;
    c->max_blocks = std::max(extrema_blocks, (int)((K + kBlock - 1) / kBlock)) + 1;
    OSFM_RETURN_IF(c->pixels.reserve((size_t)max_width * max_height * 3));
    OSFM_RETURN_IF(c->cand.reserve(K * sizeof(Keypoint)));
    OSFM_RETURN_IF(c->moved.reserve(K * sizeof(Keypoint)));
    OSFM_RETURN_IF(c->kps.reserve(K * sizeof(Keypoint)));
    OSFM_RETURN_IF(c->keep.reserve(K));
    OSFM_RETURN_IF(c->counts.reserve((size_t)c->max_blocks * sizeof(int32_t)));
    OSFM_RETURN_IF(c->total.reserve(sizeof(int32_t)));
    OSFM_HIP_CHECK(stream_create(&c->stream));
    for (c->num_events = 0; c->num_events < num_events; ++c->num_events) OSFM_HIP_CHECK(event_create(&c->ev[c->num_events], true));
    return OSFM_OK;
}

int check_image(const char *api, const char *owner, int max_w, int max_h, int width, int height, int channels)
{
    if (channels != 1 && channels != 3) {
        set_error("%s: %d channels: a grey (1) or colour (3) image is expected", api, channels);
        return OSFM_E_ARG;
    }
    if (width < 1 || height < 1) { set_error("%s: image size %d x %d", api, width, height); return OSFM_E_ARG; }
    if (width > max_w || height > max_h) {
        set_error("%s: a %d x %d image exceeds the %s's %d x %d", api, width, height, owner, max_w, max_h);
        return OSFM_E_RANGE;
    }
    return OSFM_OK;
}

int stage_image(DetectorContext *c, const uint8_t *pixels, size_t bytes, hipEvent_t image_ready, const uint8_t **d_pixels)
{
    if (pixels) {
        OSFM_HIP_CHECK(hipMemcpyAsync(c->pixels.ptr, pixels, bytes, hipMemcpyHostToDevice, c->stream));
        *d_pixels = c->pixels.as<uint8_t>();
    } else if (image_ready) OSFM_HIP_CHECK(hipStreamWaitEvent(c->stream, image_ready, 0));
    return OSFM_OK;
}

int compact_keypoints(DetectorContext *c, std::vector<Keypoint> *h_kps)
{
    c->n_kp = 0;
    h_kps->clear();
    if (c->n_cand <= 0) return OSFM_OK;
    hipStream_t s = c->stream;
    int32_t *counts = c->counts.as<int32_t>(), *total = c->total.as<int32_t>();
    detect::launch_scan(s, counts, (c->n_cand + kBlock - 1) / kBlock, total);
    detect::launch_compact(s, c->moved.as<Keypoint>(), c->keep.as<uint8_t>(), counts, c->n_cand, c->kps.as<Keypoint>());
    OSFM_HIP_CHECK(hipMemcpyAsync(&c->n_kp, total, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    h_kps->resize((size_t)c->n_kp);
    if (c->n_kp) {
        OSFM_HIP_CHECK(hipMemcpyAsync(h_kps->data(), c->kps.ptr, (size_t)c->n_kp * sizeof(Keypoint), hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
    }
    return OSFM_OK;
}

void begin_rows(DetectorContext *c, int n_desc)
{
    const size_t n = (size_t)n_desc;
    c->n_desc = n_desc;
    c->positions.resize(n * 2); c->normalized.resize(n * 2);
    c->scale.resize(n); c->orientation.resize(n); c->colors.resize(n * 3);
}

int finish_rows(DetectorContext *c, const uint8_t *pixels, int width, int height, int channels, float *ms, double *total_ms)
{
    for (size_t j = 0; pixels && j < (size_t)c->n_desc; ++j)
        feature_view_row(pixels, width, height, channels, c->positions[2 * j], c->positions[2 * j + 1], &c->colors[3 * j],
            &c->normalized[2 * j]);
    feature_view_order(c->scale, &c->order);
    *total_ms = 0.0;
    for (int i = 0; i + 1 < c->num_events; ++i) {
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
        *total_ms += ms[i];
    }
    return OSFM_OK;
}

int gather_descriptors(hipStream_t s, const float *d_desc, const std::vector<int32_t> &map, int dim, float *out)
{
    if (map.empty()) return OSFM_OK;
    const size_t last = (size_t)*std::max_element(map.begin(), map.end()) + 1;
    std::vector<float> gen(last * dim);
    OSFM_HIP_CHECK(hipMemcpyAsync(gen.data(), d_desc, gen.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < map.size(); ++i) std::memcpy(out + i * dim, gen.data() + (size_t)map[i] * dim, (size_t)dim * sizeof(float));
    return OSFM_OK;
}

int download_features(DetectorContext *c, const char *api, int dim, float *descriptors, float *positions, float *scale,
    float *orientation, uint8_t *colors, float *normalized_positions)
{
    if (!c) { set_error("%s: null argument", api); return OSFM_E_ARG; }
    if (!c->have) { set_error("%s: no extraction to download", api); return OSFM_E_STATE; }
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_desc;
    if (descriptors) {
        std::vector<int32_t> map(n);
        for (size_t i = 0; i < n; ++i) map[i] = c->desc_row((size_t)c->order[i]);
        OSFM_RETURN_IF(gather_descriptors(c->stream, c->desc.as<float>(), map, dim, descriptors));
    }
    for (size_t i = 0; i < n; ++i) {
        const size_t g = (size_t)c->order[i];
        if (positions) { positions[2 * i] = c->positions[2 * g]; positions[2 * i + 1] = c->positions[2 * g + 1]; }
        if (scale) scale[i] = c->scale[g];
        if (orientation) orientation[i] = c->orientation[g];
        if (colors) std::memcpy(colors + 3 * i, c->colors.data() + 3 * g, 3);
        if (normalized_positions) {
            normalized_positions[2 * i] = c->normalized[2 * g];
            normalized_positions[2 * i + 1] = c->normalized[2 * g + 1];
        }
    }
    return OSFM_OK;
}

int debug_keypoints(DetectorContext *c, const char *api, int after_localisation, float *out, int32_t *count)
{
    if (!c) { set_error("%s: null argument", api); return OSFM_E_ARG; }
    if (!c->have) { set_error("%s: no extraction", api); return OSFM_E_STATE; }
    const int n = after_localisation ? c->n_kp : c->n_cand;
    if (count) *count = n;
    if (!out || !n) return OSFM_OK;
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    OSFM_HIP_CHECK(hipMemcpyAsync(out, after_localisation ? c->kps.ptr : c->cand.ptr, (size_t)n * sizeof(Keypoint),
        hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OSFM_OK;
}

}  // namespace osfm
