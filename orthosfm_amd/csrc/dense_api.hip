// C entries of the dense plane sweep (include/osfm_hip.h, "Dense depth maps"): a handle that owns one grey image per
// view, the cameras and the depth maps swept so far; the sweep of one view, and the fusion of all (dense_kernels.hip).
#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "dense_handle.h"
#include "view_front.h"

using namespace osfm;
using osfm::dense::drop_map;

namespace {

int use_device(const char *api, int device)
{
    int ndev = 0;
    OSFM_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { set_error("%s: device %d of %d", api, device, ndev); return OSFM_E_ARG; }
    OSFM_HIP_CHECK(hipSetDevice(device));
    return OSFM_OK;
}

int check_view(const osfm_dense *d, int view, int width, int height, int channels, const char *api)
{
    if (view < 0 || view >= d->num_views) { set_error("%s: view %d of %d", api, view, d->num_views); return OSFM_E_RANGE; }
    if (channels != 1 && channels != 3) { set_error("%s: %d channels: a grey (1) or colour (3) image is expected", api, channels); return OSFM_E_ARG; }
    if (width < 1 || height < 1 || width > 16384 || height > 16384) {
        set_error("%s: image size %d x %d outside 1..16384", api, width, height);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

int check_options(const char *api, const osfm_dense_options &o)
{
    const bool ok = o.radius >= 1 && o.radius <= dense::kMaxRadius && o.min_sources >= 1 && o.min_sources <= dense::kMaxSources &&
        o.min_consistent >= 0 && std::isfinite(o.min_contrast) && o.min_contrast > 0.0 && o.min_score >= -1.0 && o.min_score <= 1.0 &&
        std::isfinite(o.consistency_tol) && o.consistency_tol >= 0.0;
    if (!ok) {
        set_error("%s: invalid options (radius 1..%d, min_sources 1..%d, min_consistent >= 0, min_contrast > 0, min_score -1..1, "
            "consistency_tol >= 0)", api, dense::kMaxRadius, dense::kMaxSources);
        return OSFM_E_ARG;
    }
    return OSFM_OK;
}

void count_status(const std::vector<uint8_t> &st, osfm_dense_stats *stats)
{
    for (uint8_t s : st)
        if (s < OSFM_DENSE_NUM_STATUS) stats->status_count[s]++;
}

}  // namespace

extern "C" {

int osfm_dense_options_default(osfm_dense_options *o)
{
    if (!o) { set_error("osfm_dense_options_default: null argument"); return OSFM_E_ARG; }
    o->radius = 3;
    o->min_sources = 2;
    o->min_consistent = 2;
    o->reserved = 0;
    o->min_contrast = 2.0;
    o->min_score = 0.8;
    o->consistency_tol = 2.0;
    return OSFM_OK;
}

int osfm_dense_limits(int32_t *tile_w, int32_t *tile_h, int32_t *max_radius, int32_t *max_sources, int32_t *max_depths)
{
    if (tile_w) *tile_w = dense::kTileW;
    if (tile_h) *tile_h = dense::kTileH;
    if (max_radius) *max_radius = dense::kMaxRadius;
    if (max_sources) *max_sources = dense::kMaxSources;
    if (max_depths) *max_depths = dense::kMaxDepths;
    return OSFM_OK;
}

int osfm_dense_debug_ablation(int mode)
{
    return dense::set_ablation(mode);
}

int osfm_dense_create(int device, int num_views, osfm_dense **out)
{
    if (!out) { set_error("osfm_dense_create: null argument"); return OSFM_E_ARG; }
    *out = nullptr;
    if (num_views < 1) { set_error("osfm_dense_create: %d views", num_views); return OSFM_E_ARG; }
    OSFM_RETURN_IF(use_device("osfm_dense_create", device));
    std::unique_ptr<osfm_dense> d(new osfm_dense);
    const size_t V = (size_t)num_views;
    d->device = device; d->num_views = num_views;
    d->grey.resize(V); d->depth.resize(V); d->score.resize(V); d->status.resize(V); d->final_status.resize(V);
    d->images.assign(V, refine::Image{nullptr, 0, 0});
    d->geo.resize(V);
    d->refine_status.resize(V); d->refine_gradient.resize(V); d->refine_normal.resize(V);
    d->refined.assign(V, 0);
    d->swept.assign(V, 0);
    d->dz.assign(V, 0.0);
    OSFM_RETURN_IF(d->table.reserve(V * sizeof(dense::FuseView)));
    OSFM_HIP_CHECK(stream_create(&d->stream));
    *out = d.release();
    return OSFM_OK;
}

int osfm_dense_destroy(osfm_dense *d)
{
    if (!d) return OSFM_OK;
    (void)hipSetDevice(d->device);
    delete d;
    return OSFM_OK;
}

int osfm_dense_set_image(osfm_dense *d, int view, const uint8_t *pixels, int width, int height, int channels)
{
    if (!d || !pixels) { set_error("osfm_dense_set_image: null argument"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(check_view(d, view, width, height, channels, "osfm_dense_set_image"));
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    const size_t n = (size_t)width * height;
    d->images[view] = refine::Image{nullptr, 0, 0};
    drop_map(d, view);
    OSFM_RETURN_IF(d->staging.reserve(n * channels));
    OSFM_RETURN_IF(d->grey[view].reserve(n * sizeof(float)));
    OSFM_HIP_CHECK(hipMemcpyAsync(d->staging.ptr, pixels, n * channels, hipMemcpyHostToDevice, d->stream));
    refine::launch_grey(d->stream, d->staging.as<uint8_t>(), width, height, channels, d->grey[view].as<float>());
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipStreamSynchronize(d->stream));      // the staging buffer serves the next call
    d->images[view] = refine::Image{d->grey[view].as<float>(), width, height};
    return OSFM_OK;
}

int osfm_dense_set_image_from_front(osfm_dense *d, int view, osfm_view_front *front)
{
    if (!d || !front) { set_error("osfm_dense_set_image_from_front: null argument"); return OSFM_E_ARG; }
    FrontImage im;
    OSFM_RETURN_IF(view_front_image(front, &im));
    if (im.device != d->device) {
        set_error("osfm_dense_set_image_from_front: the front end is on device %d, the handle on %d", im.device, d->device);
        return OSFM_E_ARG;
    }
    OSFM_RETURN_IF(check_view(d, view, im.width, im.height, im.channels, "osfm_dense_set_image_from_front"));
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    d->images[view] = refine::Image{nullptr, 0, 0};
    drop_map(d, view);
    OSFM_RETURN_IF(d->grey[view].reserve((size_t)im.width * im.height * sizeof(float)));
    OSFM_RETURN_IF(view_front_begin_read(front, d->stream));
    refine::launch_grey(d->stream, im.pixels, im.width, im.height, im.channels, d->grey[view].as<float>());
    const hipError_t launched = hipGetLastError();
    OSFM_RETURN_IF(view_front_end_read(front, d->stream));
    OSFM_HIP_CHECK(launched);
    d->images[view] = refine::Image{d->grey[view].as<float>(), im.width, im.height};
    return OSFM_OK;
}

int osfm_dense_set_cameras(osfm_dense *d, const double *P)
{
    if (!d || !P) { set_error("osfm_dense_set_cameras: null argument"); return OSFM_E_ARG; }
    std::vector<dense::ViewGeo> geo((size_t)d->num_views);
    for (int v = 0; v < d->num_views; ++v)
        if (!dense::make_geo(P + 8 * (size_t)v, &geo[v])) {
            set_error("osfm_dense_set_cameras: view %d: a value that is not finite, or rows of A that are not independent", v);
            return OSFM_E_ARG;
        }
    d->geo = geo;
    d->cameras = true;
    for (int v = 0; v < d->num_views; ++v) drop_map(d, v);
    return OSFM_OK;
}

int osfm_dense_sweep(osfm_dense *d, int ref, int num_sources, const int32_t *sources, double z_min, double dz, int num_depths,
    const osfm_dense_options *opts, double *depth, float *score, uint8_t *status, osfm_dense_stats *stats)
{
    if (!d || !sources) { set_error("osfm_dense_sweep: null argument"); return OSFM_E_ARG; }
    osfm_dense_options o;
    (void)osfm_dense_options_default(&o);
    if (opts) o = *opts;
    OSFM_RETURN_IF(check_options("osfm_dense_sweep", o));
    if (num_depths < 3 || num_depths > dense::kMaxDepths) {
        set_error("osfm_dense_sweep: %d depths outside 3..%d", num_depths, dense::kMaxDepths);
        return OSFM_E_ARG;
    }
    if (!std::isfinite(z_min) || !std::isfinite(dz) || !(dz > 0.0) || !std::isfinite(z_min + dz * num_depths)) {
        set_error("osfm_dense_sweep: z_min %g, dz %g: finite values and dz > 0 are expected", z_min, dz);
        return OSFM_E_ARG;
    }
    if (num_sources < 1 || num_sources > dense::kMaxSources || num_sources < o.min_sources) {
        set_error("osfm_dense_sweep: %d sources outside 1..%d, or fewer than min_sources %d", num_sources, dense::kMaxSources, o.min_sources);
        return OSFM_E_ARG;
    }
    if (ref < 0 || ref >= d->num_views) { set_error("osfm_dense_sweep: view %d of %d", ref, d->num_views); return OSFM_E_RANGE; }
    for (int i = 0; i < num_sources; ++i)
        if (sources[i] < 0 || sources[i] >= d->num_views) {
            set_error("osfm_dense_sweep: source %d is view %d of %d", i, sources[i], d->num_views);
            return OSFM_E_RANGE;
        }
    for (int i = 0; i < num_sources; ++i) {
        bool twice = sources[i] == ref;
        for (int j = 0; j < i; ++j) twice = twice || sources[j] == sources[i];
        if (twice) { set_error("osfm_dense_sweep: source %d (view %d) is the reference or named twice", i, sources[i]); return OSFM_E_ARG; }
    }
    if (!d->cameras) { set_error("osfm_dense_sweep: no cameras (osfm_dense_set_cameras)"); return OSFM_E_STATE; }
    if (!d->images[ref].px) { set_error("osfm_dense_sweep: view %d has no image", ref); return OSFM_E_STATE; }
    for (int i = 0; i < num_sources; ++i)
        if (!d->images[sources[i]].px) { set_error("osfm_dense_sweep: view %d has no image", sources[i]); return OSFM_E_STATE; }

    OSFM_HIP_CHECK(hipSetDevice(d->device));
    OSFM_HIP_CHECK(hipStreamSynchronize(d->stream));       // images handed over from a front end are complete
    const refine::Image &ir = d->images[ref];
    const size_t n = (size_t)ir.w * ir.h;
    drop_map(d, ref);
    OSFM_RETURN_IF(d->depth[ref].reserve(n * sizeof(double)));
    OSFM_RETURN_IF(d->score[ref].reserve(n * sizeof(float)));
    OSFM_RETURN_IF(d->status[ref].reserve(n));
    OSFM_RETURN_IF(d->final_status[ref].reserve(n));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    hipStream_t s = sg.s;

    dense::SweepArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ref = ir.px; a.w = ir.w; a.h = ir.h;
    a.num_sources = num_sources; a.num_depths = num_depths; a.radius = o.radius; a.min_sources = o.min_sources;
    a.z_min = z_min; a.dz = dz;
    const int side = 2 * o.radius + 1;
    a.min_var = (float)((double)(side * side) * o.min_contrast * o.min_contrast);
    a.min_score = (float)o.min_score;
    a.depth = d->depth[ref].as<double>(); a.score = d->score[ref].as<float>(); a.status = d->status[ref].as<uint8_t>();
    for (int i = 0; i < num_sources; ++i) {
        const refine::Image &is = d->images[sources[i]];
        a.src[i].px = is.px; a.src[i].w = is.w; a.src[i].h = is.h;
        dense::make_source(d->geo[ref], d->geo[sources[i]], &a.src[i]);
    }
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].a, s));
    dense::launch_sweep(s, a);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].b, s));
    // the status always comes down: the statistics are counted from it.  The caller's arrays are written only once
    // everything has arrived
    std::vector<uint8_t> h_status(n);
    OSFM_HIP_CHECK(hipMemcpyAsync(h_status.data(), a.status, n, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    if (depth) OSFM_HIP_CHECK(hipMemcpy(depth, a.depth, n * sizeof(double), hipMemcpyDeviceToHost));
    if (score) OSFM_HIP_CHECK(hipMemcpy(score, a.score, n * sizeof(float), hipMemcpyDeviceToHost));
    if (status) std::memcpy(status, h_status.data(), n);
    d->swept[ref] = 1;
    d->dz[ref] = dz;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        count_status(h_status, stats);
        const int64_t tiles = (int64_t)((ir.w + dense::kTileW - 1) / dense::kTileW) * ((ir.h + dense::kTileH - 1) / dense::kTileH);
        stats->samples = tiles * (dense::kTileW + 2 * o.radius) * (dense::kTileH + 2 * o.radius) * (int64_t)num_depths * num_sources;
        float ms = 0.0f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, sg.ev[0].a, sg.ev[0].b));
        stats->device_ms = ms;
    }
    return OSFM_OK;
}

int osfm_dense_fuse(osfm_dense *d, const osfm_dense_options *opts, int64_t *num_points, osfm_dense_stats *stats)
{
    if (!d) { set_error("osfm_dense_fuse: null argument"); return OSFM_E_ARG; }
    osfm_dense_options o;
    (void)osfm_dense_options_default(&o);
    if (opts) o = *opts;
    OSFM_RETURN_IF(check_options("osfm_dense_fuse", o));
    if (!d->cameras) { set_error("osfm_dense_fuse: no cameras (osfm_dense_set_cameras)"); return OSFM_E_STATE; }
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    const int V = d->num_views;
    std::vector<dense::FuseView> views((size_t)V);
    int64_t total = 0;
    for (int v = 0; v < V; ++v) {
        dense::FuseView &f = views[v];
        std::memset(&f, 0, sizeof(f));
        f.swept = d->swept[v];
        f.geo = d->geo[v];
        if (!f.swept) continue;
        f.depth = d->depth[v].as<double>(); f.status = d->status[v].as<uint8_t>(); f.final_status = d->final_status[v].as<uint8_t>();
        f.w = d->images[v].w; f.h = d->images[v].h;
        f.offset = total;
        f.dz = d->dz[v];
        total += (int64_t)f.w * f.h;
    }
    if (total + 1 > (int64_t)0x7fffffff) { set_error("osfm_dense_fuse: %lld pixels in all: more than one scan takes", (long long)total); return OSFM_E_ARG; }
    d->fused = false;
    OSFM_RETURN_IF(d->flags.reserve((size_t)(total + 1) * 4));
    OSFM_RETURN_IF(d->scan.reserve((size_t)(total + 1) * 4));
    size_t temp = 0;
    OSFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, d->flags.as<int32_t>(), d->scan.as<int32_t>(), (int)(total + 1), nullptr));
    OSFM_RETURN_IF(d->scan_temp.reserve(temp));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    hipStream_t s = sg.s;
    OSFM_HIP_CHECK(hipMemcpyAsync(d->table.ptr, views.data(), (size_t)V * sizeof(dense::FuseView), hipMemcpyHostToDevice, s));
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].a, s));
    OSFM_HIP_CHECK(hipMemsetAsync(d->flags.as<int32_t>() + total, 0, 4, s));
    for (int v = 0; v < V; ++v)
        if (views[v].swept)
            dense::launch_consistency(s, d->table.as<dense::FuseView>(), V, v, (int64_t)views[v].w * views[v].h, o.consistency_tol,
                o.min_consistent, d->flags.as<int32_t>());
    OSFM_HIP_CHECK(hipGetLastError());
    size_t have = d->scan_temp.bytes;
    OSFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d->scan_temp.ptr, have, d->flags.as<int32_t>(), d->scan.as<int32_t>(), (int)(total + 1), s));
    int32_t count = 0;
    OSFM_HIP_CHECK(hipMemcpyAsync(&count, d->scan.as<int32_t>() + total, 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    const size_t N = (size_t)count;
    OSFM_RETURN_IF(d->cloud_points.reserve(N * 24 + 8));
    OSFM_RETURN_IF(d->cloud_view.reserve(N * 4 + 8));
    OSFM_RETURN_IF(d->cloud_pixel.reserve(N * 8 + 8));
    const dense::Cloud cloud{d->cloud_points.as<double>(), d->cloud_view.as<int32_t>(), d->cloud_pixel.as<int32_t>()};
    for (int v = 0; v < V; ++v)
        if (views[v].swept)
            dense::launch_emit(s, d->table.as<dense::FuseView>(), v, (int64_t)views[v].w * views[v].h, d->flags.as<int32_t>(),
                d->scan.as<int32_t>(), cloud);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].b, s));
    std::vector<uint8_t> h_status;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (int v = 0; v < V; ++v) {
            if (!views[v].swept) continue;
            h_status.resize((size_t)views[v].w * views[v].h);
            OSFM_HIP_CHECK(hipMemcpyAsync(h_status.data(), views[v].final_status, h_status.size(), hipMemcpyDeviceToHost, s));
            OSFM_HIP_CHECK(hipStreamSynchronize(s));
            count_status(h_status, stats);
        }
    }
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    if (stats) {
        float ms = 0.0f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, sg.ev[0].a, sg.ev[0].b));
        stats->device_ms = ms;
    }
    d->cloud_size = count;
    d->fused = true;
    if (num_points) *num_points = count;
    return OSFM_OK;
}

int osfm_dense_download_status(osfm_dense *d, int view, uint8_t *status)
{
    if (!d || !status) { set_error("osfm_dense_download_status: null argument"); return OSFM_E_ARG; }
    if (view < 0 || view >= d->num_views) { set_error("osfm_dense_download_status: view %d of %d", view, d->num_views); return OSFM_E_RANGE; }
    if (!d->fused || !d->swept[view]) { set_error("osfm_dense_download_status: view %d has no fused depth map", view); return OSFM_E_STATE; }
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    OSFM_HIP_CHECK(hipMemcpy(status, d->final_status[view].ptr, (size_t)d->images[view].w * d->images[view].h, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

int osfm_dense_download_cloud(osfm_dense *d, int64_t capacity, double *points, int32_t *view, int32_t *pixel)
{
    if (!d) { set_error("osfm_dense_download_cloud: null argument"); return OSFM_E_ARG; }
    if (!d->fused) { set_error("osfm_dense_download_cloud: no fusion (osfm_dense_fuse)"); return OSFM_E_STATE; }
    if (capacity < d->cloud_size) {
        set_error("osfm_dense_download_cloud: capacity %lld, the cloud has %lld points", (long long)capacity, (long long)d->cloud_size);
        return OSFM_E_CAPACITY;
    }
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    const size_t N = (size_t)d->cloud_size;
    if (N == 0) return OSFM_OK;
    if (points) OSFM_HIP_CHECK(hipMemcpy(points, d->cloud_points.ptr, N * 24, hipMemcpyDeviceToHost));
    if (view) OSFM_HIP_CHECK(hipMemcpy(view, d->cloud_view.ptr, N * 4, hipMemcpyDeviceToHost));
    if (pixel) OSFM_HIP_CHECK(hipMemcpy(pixel, d->cloud_pixel.ptr, N * 8, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

int osfm_dense_cloud_write(const char *path, int64_t n, const double *points, const uint8_t *rgb)
{
    if (!path || n < 0 || (n > 0 && !points)) { set_error("osfm_dense_cloud_write: null argument / negative count"); return OSFM_E_ARG; }
    std::ofstream f(path, std::ios::out | std::ios::trunc | std::ios::binary);
    if (!f) { set_error("osfm_dense_cloud_write: cannot open %s", path); return OSFM_E_IO; }
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << (long long)n << "\n"
      << "property float x\nproperty float y\nproperty float z\n"
      << "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
    std::vector<char> rows((size_t)n * 15);
    for (int64_t i = 0; i < n; ++i) {
        char *row = rows.data() + 15 * (size_t)i;
        const float xyz[3] = {(float)points[3 * i], (float)points[3 * i + 1], (float)points[3 * i + 2]};
        std::memcpy(row, xyz, 12);                      // the hosts this library runs on are little-endian
        for (int c = 0; c < 3; ++c) row[12 + c] = rgb ? (char)rgb[3 * i + c] : 0;
    }
    f.write(rows.data(), (std::streamsize)rows.size());
    f.close();
    if (!f) { set_error("osfm_dense_cloud_write: write to %s failed", path); return OSFM_E_IO; }
    return OSFM_OK;
}

}  // extern "C"
