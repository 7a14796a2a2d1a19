// C entries of the observation refinement (include/osfm_hip.h, "Sub-pixel refinement"): a handle that owns one grey
// image per view, and the call that refines the observations of tracks against them (refine_kernels.hip).
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "refine_kernels.h"
#include "view_front.h"

using namespace osfm;

struct osfm_refiner {
    int device = 0, num_views = 0;
    hipStream_t stream = nullptr;          // image uploads and conversions
    std::vector<DeviceBuffer> grey;        // float32 [h][w] per view
    std::vector<refine::Image> images;     // what the kernel sees of them
    DeviceBuffer staging, table;           // the 8-bit upload of set_image; the images array on the device
    ~osfm_refiner() { stream_destroy(stream); }
};

namespace {

int use_device(const char *api, int device)
{
    int ndev = 0;
    OSFM_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("%s: device %d of %d", api, device, ndev); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
    return OSFM_OK;
}

int check_view(const osfm_refiner *r, int view, int width, int height, int channels, const char *api)
{
    if (view < 0 || view >= r->num_views) { set_error("%s: view %d of %d", api, view, r->num_views); return OSFM_E_RANGE; }
    if (channels != 1 && channels != 3) { set_error("%s: %d channels: a grey (1) or colour (3) image is expected", api, channels); return OSFM_E_ARG; }
    if (width < 1 || height < 1 || width > 16384 || height > 16384) {
        set_error("%s: image size %d x %d outside 1..16384", api, width, height);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

int check_options(const osfm_refine_options &o)
{
    const bool ok = o.radius >= 2 && o.radius <= refine::kMaxRadius && o.max_iterations >= 1 && o.max_iterations <= 100 &&
        std::isfinite(o.step) && o.step > 0.0 && std::isfinite(o.eps) && o.eps >= 0.0 && std::isfinite(o.min_contrast) &&
        std::isfinite(o.max_shift) && o.max_shift >= 0.0 && std::isfinite(o.max_deform) && o.max_deform >= 1.0 &&
        o.min_score >= -1.0 && o.min_score <= 1.0 && o.min_pivot > 0.0 && o.min_pivot < 1.0;
    if (!ok) {
        set_error("osfm_refine_tracks: invalid options (radius 2..%d, max_iterations 1..100, step > 0, eps >= 0, max_shift >= 0, "
            "max_deform >= 1, min_score -1..1, 0 < min_pivot < 1)", refine::kMaxRadius);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

}  // namespace

extern "C" {

int osfm_refine_options_default(osfm_refine_options *o)
{
    if (!o) { set_error("osfm_refine_options_default: null argument"); return OSFM_E_ARG; }
    o->radius = 7;
    o->max_iterations = 10;
    o->step = 1.0;
    o->eps = 1e-3;
    o->min_contrast = 2.0;
    o->max_shift = 3.0;
    o->max_deform = 2.0;
    o->min_score = 0.9;
    o->min_pivot = 0.034;
    return OSFM_OK;
}

int osfm_refine_create(int device, int num_views, osfm_refiner **out)
{
    if (!out) { set_error("osfm_refine_create: null argument"); return OSFM_E_ARG; }
    *out = nullptr;
    if (num_views < 1) { set_error("osfm_refine_create: %d views", num_views); return OSFM_E_ARG; }
    OSFM_RETURN_IF(use_device("osfm_refine_create", device));
    std::unique_ptr<osfm_refiner> r(new osfm_refiner);
    r->device = device; r->num_views = num_views;
    r->grey.resize((size_t)num_views);
    r->images.assign((size_t)num_views, refine::Image{nullptr, 0, 0});
    OSFM_RETURN_IF(r->table.reserve((size_t)num_views * sizeof(refine::Image)));
    OSFM_HIP_CHECK(stream_create(&r->stream));
    *out = r.release();
    return OSFM_OK;
}

int osfm_refine_destroy(osfm_refiner *r)
{
    if (!r) return OSFM_OK;
    (void)hipSetDevice(r->device);
    delete r;
    return OSFM_OK;
}

int osfm_refine_set_image(osfm_refiner *r, int view, const uint8_t *pixels, int width, int height, int channels)
{
    if (!r || !pixels) { set_error("osfm_refine_set_image: null argument"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(check_view(r, view, width, height, channels, "osfm_refine_set_image"));
    OSFM_HIP_CHECK(hipSetDevice(r->device));
    const size_t n = (size_t)width * height;
    r->images[view] = refine::Image{nullptr, 0, 0};
    OSFM_RETURN_IF(r->staging.reserve(n * channels));
    OSFM_RETURN_IF(r->grey[view].reserve(n * sizeof(float)));
    OSFM_HIP_CHECK(hipMemcpyAsync(r->staging.ptr, pixels, n * channels, hipMemcpyHostToDevice, r->stream));
    refine::launch_grey(r->stream, r->staging.as<uint8_t>(), width, height, channels, r->grey[view].as<float>());
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipStreamSynchronize(r->stream));      // the staging buffer serves the next call
    r->images[view] = refine::Image{r->grey[view].as<float>(), width, height};
    return OSFM_OK;
}

int osfm_refine_set_image_from_front(osfm_refiner *r, int view, osfm_view_front *front)
{
    if (!r || !front) { set_error("osfm_refine_set_image_from_front: null argument"); return OSFM_E_ARG; }
    FrontImage im;
    OSFM_RETURN_IF(view_front_image(front, &im));
    if (im.device != r->device) {
        set_error("osfm_refine_set_image_from_front: the front end is on device %d, the refiner on %d", im.device, r->device);
        return OSFM_E_ARG;
    }
    OSFM_RETURN_IF(check_view(r, view, im.width, im.height, im.channels, "osfm_refine_set_image_from_front"));
    OSFM_HIP_CHECK(hipSetDevice(r->device));
    r->images[view] = refine::Image{nullptr, 0, 0};
    OSFM_RETURN_IF(r->grey[view].reserve((size_t)im.width * im.height * sizeof(float)));
    OSFM_RETURN_IF(view_front_begin_read(front, r->stream));
    refine::launch_grey(r->stream, im.pixels, im.width, im.height, im.channels, r->grey[view].as<float>());
    const hipError_t launched = hipGetLastError();
    OSFM_RETURN_IF(view_front_end_read(front, r->stream));
    OSFM_HIP_CHECK(launched);
    r->images[view] = refine::Image{r->grey[view].as<float>(), im.width, im.height};
    return OSFM_OK;
}

int osfm_refine_tracks(osfm_refiner *r, int64_t num_tracks, const int64_t *offsets, const int32_t *view, const double *xy,
    const uint8_t *alive, const double *init_affine, const osfm_refine_options *opts, double *out_xy, double *out_affine,
    double *score, int32_t *status, int32_t *iterations, osfm_refine_stats *stats)
{
    if (!r || num_tracks < 0 || !offsets) { set_error("osfm_refine_tracks: null argument / negative count"); return OSFM_E_ARG; }
    osfm_refine_options o;
    (void)osfm_refine_options_default(&o);
    if (opts) o = *opts;
    OSFM_RETURN_IF(check_options(o));
    if (offsets[0] != 0) { set_error("osfm_refine_tracks: offsets[0] is %lld", (long long)offsets[0]); return OSFM_E_ARG; }
    for (int64_t t = 0; t < num_tracks; ++t)
        if (offsets[t + 1] < offsets[t]) { set_error("osfm_refine_tracks: offsets decrease at track %lld", (long long)t); return OSFM_E_ARG; }
    const int64_t F = offsets[num_tracks];
    if (F > 0 && (!view || !xy || !out_xy || !status)) { set_error("osfm_refine_tracks: null array"); return OSFM_E_ARG; }
    for (int64_t f = 0; f < F; ++f) {
        bool finite = std::isfinite(xy[2 * f]) && std::isfinite(xy[2 * f + 1]);
        if (finite && init_affine) {
            const double *a = init_affine + 4 * f;
            finite = std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && std::isfinite(a[3]) &&
                a[0] * a[3] - a[1] * a[2] != 0.0;
        }
        if (!finite) {
            set_error("osfm_refine_tracks: observation %lld: a position or init_affine that is not finite, or a singular init_affine", (long long)f);
            return OSFM_E_ARG;
        }
    }
    for (int64_t f = 0; f < F; ++f)
        if (view[f] < 0 || view[f] >= r->num_views) {
            set_error("osfm_refine_tracks: observation %lld names view %d of %d", (long long)f, view[f], r->num_views);
            return OSFM_E_RANGE;
        }
    for (int64_t f = 0; f < F; ++f)
        if ((!alive || alive[f]) && !r->images[view[f]].px) {
            set_error("osfm_refine_tracks: observation %lld lies in view %d, which has no image", (long long)f, view[f]);
            return OSFM_E_STATE;
        }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (F == 0) return OSFM_OK;

    OSFM_HIP_CHECK(hipSetDevice(r->device));
    OSFM_HIP_CHECK(hipStreamSynchronize(r->stream));       // images handed over from a front end are complete
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    const size_t T = (size_t)num_tracks, n = (size_t)F;
    PooledBuffer d_off, d_view, d_xy, d_alive, d_aff, d_ref, d_count, d_track, o_xy, o_aff, o_score, o_status, o_iter;
    OSFM_RETURN_IF(d_off.reserve((T + 1) * 8));
    OSFM_RETURN_IF(d_view.reserve(n * 4));
    OSFM_RETURN_IF(d_xy.reserve(n * 16));
    if (alive) OSFM_RETURN_IF(d_alive.reserve(n));
    if (init_affine) OSFM_RETURN_IF(d_aff.reserve(n * 32));
    OSFM_RETURN_IF(d_ref.reserve(T * 8));
    OSFM_RETURN_IF(d_count.reserve(T * 4));
    OSFM_RETURN_IF(d_track.reserve(n * 4));
    OSFM_RETURN_IF(o_xy.reserve(n * 16));
    OSFM_RETURN_IF(o_aff.reserve(n * 32));
    OSFM_RETURN_IF(o_score.reserve(n * 8));
    OSFM_RETURN_IF(o_status.reserve(n * 4));
    OSFM_RETURN_IF(o_iter.reserve(n * 4));
    hipStream_t s = sg.s;
    OSFM_HIP_CHECK(hipMemcpyAsync(r->table.ptr, r->images.data(), r->images.size() * sizeof(refine::Image), hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(d_off.ptr, offsets, (T + 1) * 8, hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(d_view.ptr, view, n * 4, hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(d_xy.ptr, xy, n * 16, hipMemcpyHostToDevice, s));
    if (alive) OSFM_HIP_CHECK(hipMemcpyAsync(d_alive.ptr, alive, n, hipMemcpyHostToDevice, s));
    if (init_affine) OSFM_HIP_CHECK(hipMemcpyAsync(d_aff.ptr, init_affine, n * 32, hipMemcpyHostToDevice, s));
    const refine::Tracks tr{num_tracks, F, d_off.as<int64_t>(), d_view.as<int32_t>(), d_xy.as<double>(),
        alive ? d_alive.as<uint8_t>() : nullptr, init_affine ? d_aff.as<double>() : nullptr};
    const refine::Work wk{d_ref.as<int64_t>(), d_count.as<int32_t>(), d_track.as<int32_t>()};
    const refine::Out out{o_xy.as<double>(), o_aff.as<double>(), o_score.as<double>(), o_status.as<int32_t>(), o_iter.as<int32_t>()};
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].a, s));
    refine::launch_track_pass(s, tr, wk);
    refine::launch_refine(s, r->table.as<refine::Image>(), tr, wk, o, out);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].b, s));
    // status and iterations always come down: the statistics are counted from them.  The caller's arrays are written
    // only once everything has arrived
    std::vector<int32_t> h_status(n), h_iter(n);
    std::vector<double> h_xy(n * 2);
    OSFM_HIP_CHECK(hipMemcpyAsync(h_status.data(), o_status.ptr, n * 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(h_iter.data(), o_iter.ptr, n * 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(h_xy.data(), o_xy.ptr, n * 16, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    if (out_affine) OSFM_HIP_CHECK(hipMemcpy(out_affine, o_aff.ptr, n * 32, hipMemcpyDeviceToHost));
    if (score) OSFM_HIP_CHECK(hipMemcpy(score, o_score.ptr, n * 8, hipMemcpyDeviceToHost));
    std::memcpy(out_xy, h_xy.data(), n * 16);
    std::memcpy(status, h_status.data(), n * 4);
    if (iterations) std::memcpy(iterations, h_iter.data(), n * 4);
    if (stats) {
        for (size_t f = 0; f < n; ++f) {
            if (h_status[f] >= 0 && h_status[f] < OSFM_REFINE_NUM_STATUS) stats->status_count[h_status[f]]++;
            stats->iterations += h_iter[f];
        }
        float ms = 0.0f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, sg.ev[0].a, sg.ev[0].b));
        stats->device_ms = ms;
    }
    return OSFM_OK;
}

}  // extern "C"
