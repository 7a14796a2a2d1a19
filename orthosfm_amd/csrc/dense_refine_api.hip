// C entries of the slanted-plane refinement (include/osfm_hip.h, "Slanted-plane refinement of a depth map"): the
// refinement of one view's map in place (dense_refine_kernels.hip) and the download of what it left.
#include <cmath>
#include <cstring>
#include <vector>

#include "dense_handle.h"
#include "dense_refine_kernels.h"

using namespace osfm;

extern "C" {

int osfm_dense_refine_options_default(osfm_dense_refine_options *o)
{
    if (!o) { set_error("osfm_dense_refine_options_default: null argument"); return OSFM_E_ARG; }
    o->radius = 3;
    o->min_sources = 2;
    o->max_iterations = 10;
    o->reserved = 0;
    o->eps = 1e-3;
    o->max_shift = 1.5;
    o->max_deform = 2.0;
    o->min_score = 0.8;
    o->min_pivot = 0.035;
    return OSFM_OK;
}

int osfm_dense_refine_view(osfm_dense *d, int view, int num_sources, const int32_t *sources, const osfm_dense_refine_options *opts,
    double *depth, double *gradient, double *normal, float *score, uint8_t *rstatus, osfm_dense_refine_stats *stats)
{
    const char *api = "osfm_dense_refine_view";
    if (!d || !sources) { set_error("%s: null argument", api); return OSFM_E_ARG; }
    osfm_dense_refine_options o;
    (void)osfm_dense_refine_options_default(&o);
    if (opts) o = *opts;
    const bool ok = o.radius >= 1 && o.radius <= dense::kMaxRadius && o.min_sources >= 1 && o.min_sources <= dense::kMaxSources &&
        o.max_iterations >= 1 && o.max_iterations <= dense::kRefineMaxIterations && std::isfinite(o.eps) && o.eps > 0.0 &&
        std::isfinite(o.max_shift) && o.max_shift >= 0.0 && std::isfinite(o.max_deform) && o.max_deform >= 1.0 &&
        o.min_score >= -1.0 && o.min_score <= 1.0 && o.min_pivot > 0.0 && o.min_pivot < 1.0;
    if (!ok) {
        set_error("%s: invalid options (radius 1..%d, min_sources 1..%d, max_iterations 1..%d, eps > 0, max_shift >= 0, max_deform >= 1, "
            "min_score -1..1, 0 < min_pivot < 1)", api, dense::kMaxRadius, dense::kMaxSources, dense::kRefineMaxIterations);
        return OSFM_E_ARG;
    }
    if (num_sources < 1 || num_sources > dense::kMaxSources || num_sources < o.min_sources) {
        set_error("%s: %d sources outside 1..%d, or fewer than min_sources %d", api, num_sources, dense::kMaxSources, o.min_sources);
        return OSFM_E_ARG;
    }
    if (view < 0 || view >= d->num_views) { set_error("%s: view %d of %d", api, view, d->num_views); return OSFM_E_RANGE; }
    for (int i = 0; i < num_sources; ++i)
        if (sources[i] < 0 || sources[i] >= d->num_views) {
            set_error("%s: source %d is view %d of %d", api, i, sources[i], d->num_views);
            return OSFM_E_RANGE;
        }
    for (int i = 0; i < num_sources; ++i) {
        bool twice = sources[i] == view;
        for (int j = 0; j < i; ++j) twice = twice || sources[j] == sources[i];
        if (twice) { set_error("%s: source %d (view %d) is the view itself or named twice", api, i, sources[i]); return OSFM_E_ARG; }
    }
    if (!d->cameras) { set_error("%s: no cameras (osfm_dense_set_cameras)", api); return OSFM_E_STATE; }
    if (!d->swept[view] || !d->images[view].px) { set_error("%s: view %d has no depth map", api, view); return OSFM_E_STATE; }
    for (int i = 0; i < num_sources; ++i)
        if (!d->images[sources[i]].px) { set_error("%s: view %d has no image", api, sources[i]); return OSFM_E_STATE; }

    OSFM_HIP_CHECK(hipSetDevice(d->device));
    OSFM_HIP_CHECK(hipStreamSynchronize(d->stream));       // images handed over from a front end are complete
    const refine::Image &ir = d->images[view];
    const size_t n = (size_t)ir.w * ir.h;
    OSFM_RETURN_IF(d->refine_status[view].reserve(n));
    OSFM_RETURN_IF(d->refine_gradient[view].reserve(n * 2 * sizeof(double)));
    OSFM_RETURN_IF(d->refine_normal[view].reserve(n * 3 * sizeof(double)));
    const size_t counter_bytes = (size_t)dense::kRefineCounterSlots * dense::kRefineSlotStride * sizeof(unsigned long long);
    OSFM_RETURN_IF(d->refine_counters.reserve(counter_bytes));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    hipStream_t s = sg.s;
    // the map changes: what was made of it is gone, and until the kernel has run the planes mean nothing
    d->refined[view] = 0;
    d->fused = false;
    if (d->mesh_view == view) d->mesh_view = -1;

    dense::RefineArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ref = ir.px; a.w = ir.w; a.h = ir.h;
    a.num_sources = num_sources; a.radius = o.radius; a.min_sources = o.min_sources; a.max_iterations = o.max_iterations;
    a.dz = d->dz[view];
    a.converged = o.eps * a.dz;
    a.max_shift = o.max_shift; a.max_deform = o.max_deform; a.min_score = o.min_score; a.min_pivot = o.min_pivot;
    const dense::ViewGeo &g = d->geo[view];
    for (int j = 0; j < 3; ++j) { a.B[j][0] = g.B[j][0]; a.B[j][1] = g.B[j][1]; a.d[j] = g.d[j]; }
    a.status = d->status[view].as<uint8_t>();
    a.depth = d->depth[view].as<double>();
    a.score = d->score[view].as<float>();
    a.rstatus = d->refine_status[view].as<uint8_t>();
    a.gradient = d->refine_gradient[view].as<double>();
    a.normal = d->refine_normal[view].as<double>();
    a.counters = d->refine_counters.as<unsigned long long>();
    for (int i = 0; i < num_sources; ++i) {
        const refine::Image &is = d->images[sources[i]];
        a.src[i].px = is.px; a.src[i].w = is.w; a.src[i].h = is.h;
        dense::make_source(g, d->geo[sources[i]], &a.src[i]);
    }
    OSFM_HIP_CHECK(hipMemsetAsync(a.counters, 0, counter_bytes, s));
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].a, s));
    dense::launch_refine(s, a);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].b, s));
    // the status always comes down: the statistics are counted from it.  The caller's arrays are written only once
    // everything has arrived
    std::vector<uint8_t> h_status(n);
    std::vector<unsigned long long> h_counters((size_t)dense::kRefineCounterSlots * dense::kRefineSlotStride);
    OSFM_HIP_CHECK(hipMemcpyAsync(h_status.data(), a.rstatus, n, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(h_counters.data(), a.counters, counter_bytes, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    d->refined[view] = 1;
    if (depth) OSFM_HIP_CHECK(hipMemcpy(depth, a.depth, n * sizeof(double), hipMemcpyDeviceToHost));
    if (gradient) OSFM_HIP_CHECK(hipMemcpy(gradient, a.gradient, n * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (normal) OSFM_HIP_CHECK(hipMemcpy(normal, a.normal, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (score) OSFM_HIP_CHECK(hipMemcpy(score, a.score, n * sizeof(float), hipMemcpyDeviceToHost));
    if (rstatus) std::memcpy(rstatus, h_status.data(), n);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (uint8_t st : h_status)
            if (st < OSFM_DENSE_REFINE_NUM_STATUS) stats->status_count[st]++;
        int64_t passes = 0;
        for (int slot = 0; slot < dense::kRefineCounterSlots; ++slot) {
            stats->iterations += (int64_t)h_counters[(size_t)slot * dense::kRefineSlotStride];
            passes += (int64_t)h_counters[(size_t)slot * dense::kRefineSlotStride + 1];
        }
        const int side = 2 * o.radius + 1;
        stats->samples = passes * side * side;
        float ms = 0.0f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, sg.ev[0].a, sg.ev[0].b));
        stats->device_ms = ms;
    }
    return OSFM_OK;
}

int osfm_dense_download_refined(osfm_dense *d, int view, double *gradient, double *normal, uint8_t *rstatus)
{
    const char *api = "osfm_dense_download_refined";
    if (!d) { set_error("%s: null argument", api); return OSFM_E_ARG; }
    if (view < 0 || view >= d->num_views) { set_error("%s: view %d of %d", api, view, d->num_views); return OSFM_E_RANGE; }
    if (!d->refined[view]) { set_error("%s: the map of view %d was not refined (osfm_dense_refine_view)", api, view); return OSFM_E_STATE; }
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    const size_t n = (size_t)d->images[view].w * d->images[view].h;
    if (gradient) OSFM_HIP_CHECK(hipMemcpy(gradient, d->refine_gradient[view].ptr, n * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (normal) OSFM_HIP_CHECK(hipMemcpy(normal, d->refine_normal[view].ptr, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (rstatus) OSFM_HIP_CHECK(hipMemcpy(rstatus, d->refine_status[view].ptr, n, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

}  // extern "C"
