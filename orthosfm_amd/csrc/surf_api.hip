// C ABI of the SURF extraction (include/osfm_hip.h, "SURF feature extraction"): owns the summed-area table and
// the response maps, runs the stages of surf_kernels.hip in the reference's order, and keeps
// FeatureSet::compute_surf's view of the result.  What an extraction shares with SIFT's is detector_context.h's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "detector_context.h"
#include "feature_device.h"
#include "surf_kernels.h"

using namespace osfm;
using namespace osfm::surf;

struct osfm_surf : DetectorContext {
    osfm_surf_options opts{};
    DeviceBuffer sat, maps, table, weights, ori_jobs, ori_out, desc_jobs, status;
    size_t map_floats = 0;
    // the last extraction (rows: generation row j is descriptor job rows[j])
    int width = 0, height = 0;
    MapsView view{};
};

namespace {

// Filter sizes (a third of the kernel's side): fs = 2^(o + 1) (k + 1) + 1
int filter_size(int o, int k) { return (2 << o) * (k + 1) + 1; }

// The response maps of a w x h image: per octave ceil(w / 2^o) x ceil(h / 2^o), four planes.
size_t plan_maps(int w, int h, MapsView *mv, int *blocks)
{
    size_t n = 0;
    int total_blocks = 0;
    for (int o = 0; o < kOctaves; ++o) {
        if (mv) { mv->ow[o] = w; mv->oh[o] = h; mv->offset[o] = n; }
        n += (size_t)kSamples * w * h;
        total_blocks += 2 * extrema_blocks(w, h);
        w = (w + 1) >> 1; h = (h + 1) >> 1;
    }
    if (blocks) *blocks = total_blocks;
    return n;
}

// Surf::descriptor_assignment's scale of a keypoint, by the reference's float expression.
float keypoint_scale(const Keypoint &k)
{
    const int sample = (int)(k.sample + 0.5f);
    return 3 * filter_size((int)k.octave, sample) * 1.2f / 9.0f;
}

int describe(osfm_surf *c, const std::vector<DescJob> &jobs, std::vector<int32_t> *status)
{
    const size_t n = jobs.size();
    status->assign(n, 0);
    if (!n) return OSFM_OK;
    hipStream_t s = c->stream;
    OSFM_HIP_CHECK(hipMemcpyAsync(c->desc_jobs.ptr, jobs.data(), n * sizeof(DescJob), hipMemcpyHostToDevice, s));
    launch_descriptor(s, c->sat.as<Sat>(), c->width, c->height, c->weights.as<float>(), c->desc_jobs.as<DescJob>(), (int)n,
        c->desc.as<float>(), c->status.as<int32_t>());
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipMemcpyAsync(status->data(), c->status.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    return OSFM_OK;
}

// pixels: the image in host memory, uploaded here; or NULL with d_pixels, the image on the device, read once
// image_ready has happened (the colours and normalised positions then stay with the caller).
int extract(osfm_surf *c, const uint8_t *pixels, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height,
    int channels, osfm_surf_summary *sum_out)
{
    const osfm_surf_options &o = c->opts;
    hipStream_t s = c->stream;
    MapsView mv{};
    int total_blocks = 0;
    if (plan_maps(width, height, &mv, &total_blocks) > c->map_floats || total_blocks > c->max_blocks) {
        set_error("osfm_surf_extract: internal: the maps of %d x %d exceed the context's", width, height);
        return OSFM_E_STATE;
    }
    mv.maps = c->maps.as<float>();
    Sat *sat = c->sat.as<Sat>();

    // ---- summed-area table
    OSFM_HIP_CHECK(hipEventRecord(c->ev[0], s));
    OSFM_RETURN_IF(stage_image(c, pixels, (size_t)width * height * channels, image_ready, &d_pixels));
    launch_sat(s, d_pixels, width, height, channels, sat);

    // ---- response maps
    OSFM_HIP_CHECK(hipEventRecord(c->ev[1], s));
    for (int oi = 0; oi < kOctaves; ++oi) {
        OctaveFilters f;
        for (int k = 0; k < kSamples; ++k) {
            const int fs = filter_size(oi, k);
            f.fs[k] = fs;
            f.inv_karea[k] = 1.0 / (fs * (2 * fs - 1));
        }
        launch_response(s, sat, width, height, oi, f, mv.maps + mv.offset[oi], mv.ow[oi], mv.oh[oi]);
    }
    OSFM_HIP_CHECK(hipGetLastError());

    // ---- extrema: count per workgroup, scan, write in (octave, sample, y, x) order
    OSFM_HIP_CHECK(hipEventRecord(c->ev[2], s));
    Keypoint *cand = c->cand.as<Keypoint>();
    OSFM_RETURN_IF(find_candidates(c, "osfm_surf_extract", kOctaves, 1, 3, [&](int oi, int si, int base, const int32_t *offsets) {
        const size_t plane = (size_t)mv.ow[oi] * mv.oh[oi];
        const float *m1 = mv.maps + mv.offset[oi] + (size_t)si * plane;
        launch_extrema(s, m1 - plane, m1, m1 + plane, mv.ow[oi], mv.oh[oi], base, c->counts.as<int32_t>(), offsets, cand,
            o.max_keypoints, (float)oi, (float)si);
        return extrema_blocks(mv.ow[oi], mv.oh[oi]);
    }));
    const int n_cand = c->n_cand;

    // ---- localisation and compaction
    OSFM_HIP_CHECK(hipEventRecord(c->ev[3], s));
    std::vector<Keypoint> h_kps;
    if (n_cand > 0)
        launch_localise(s, mv, o.contrast_threshold, width, height, cand, n_cand, c->moved.as<Keypoint>(), c->keep.as<uint8_t>(),
            c->counts.as<int32_t>());
    OSFM_RETURN_IF(compact_keypoints(c, &h_kps));
    const int n_kp = c->n_kp;

    // ---- orientation: the windows on the device, atan2 / sinf / cosf of the winner from the C library
    OSFM_HIP_CHECK(hipEventRecord(c->ev[4], s));
    std::vector<float> kp_scale((size_t)n_kp);
    std::vector<OriJob> ori_jobs((size_t)n_kp);
    std::vector<OriResult> ori((size_t)n_kp);
    for (int i = 0; i < n_kp; ++i) {
        const Keypoint &k = h_kps[(size_t)i];
        kp_scale[(size_t)i] = keypoint_scale(k);
        ori_jobs[(size_t)i] = OriJob{(int)(k.x + 0.5f), (int)(k.y + 0.5f), (int)kp_scale[(size_t)i]};
    }
    if (n_kp) {
        OSFM_HIP_CHECK(hipMemcpyAsync(c->ori_jobs.ptr, ori_jobs.data(), (size_t)n_kp * sizeof(OriJob), hipMemcpyHostToDevice, s));
        launch_orientation(s, sat, width, height, c->table.as<OriTable>(), c->ori_jobs.as<OriJob>(), n_kp, c->ori_out.as<OriResult>());
        OSFM_HIP_CHECK(hipGetLastError());
        OSFM_HIP_CHECK(hipMemcpyAsync(ori.data(), c->ori_out.ptr, (size_t)n_kp * sizeof(OriResult), hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
    }
    std::vector<DescJob> jobs;
    std::vector<int32_t> job_kp;
    std::vector<float> job_ori;
    for (int i = 0; i < n_kp; ++i) {
        if (!ori[(size_t)i].ok) continue;
        const Keypoint &k = h_kps[(size_t)i];
        const float orientation = std::atan2(ori[(size_t)i].best_dy, ori[(size_t)i].best_dx);
        DescJob j{k.x, k.y, (int)kp_scale[(size_t)i], 0.0f, 1.0f};
        if (!o.use_upright_descriptor) {
            j.sin_ori = std::sin(orientation);
            j.cos_ori = std::cos(orientation);
        }
        jobs.push_back(j);
        job_kp.push_back(i);
        job_ori.push_back(orientation);
    }

    // ---- descriptors
    OSFM_HIP_CHECK(hipEventRecord(c->ev[5], s));
    c->width = width; c->height = height;        // describe() reads them
    std::vector<int32_t> status;
    OSFM_RETURN_IF(describe(c, jobs, &status));
    OSFM_HIP_CHECK(hipEventRecord(c->ev[6], s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));

    // ---- FeatureSet::compute_surf's view: positions, colours, the order by scale
    osfm_surf_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    sum.num_candidates = n_cand; sum.num_keypoints = n_kp;
    for (const Keypoint &k : h_kps) sum.keypoints_per_octave[(int)k.octave]++;
    std::vector<int32_t> rows;
    for (size_t j = 0; j < jobs.size(); ++j)
        if (status[j]) rows.push_back((int32_t)j);
    const int n_desc = (int)rows.size();     // <= n_kp <= n_cand <= max_keypoints: one per keypoint at most
    sum.num_descriptors = n_desc;
    begin_rows(c, n_desc);
    for (int r = 0; r < n_desc; ++r) {
        const size_t j = (size_t)rows[(size_t)r];
        const Keypoint &k = h_kps[(size_t)job_kp[j]];
        sum.descriptors_per_octave[(int)k.octave]++;
        sum.num_guarded += status[j] == 2;
        c->positions[2 * (size_t)r] = k.x; c->positions[2 * (size_t)r + 1] = k.y;
        c->scale[(size_t)r] = kp_scale[(size_t)job_kp[j]];
        c->orientation[(size_t)r] = job_ori[j];
    }
    float ms[6] = {};
    OSFM_RETURN_IF(finish_rows(c, pixels, width, height, channels, ms, &sum.total_ms));
    sum.sat_ms = ms[0]; sum.response_ms = ms[1]; sum.extrema_ms = ms[2]; sum.localisation_ms = ms[3]; sum.orientation_ms = ms[4];
    sum.descriptor_ms = ms[5];
    c->view = mv;
    c->rows.swap(rows);
    c->have = true;
    if (sum_out) *sum_out = sum;
    return OSFM_OK;
}

}  // namespace

namespace osfm {

int surf_extract_device(osfm_surf *c, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height, int channels,
    osfm_surf_summary *summary)
{
    return run_extract(c, "osfm_surf_extract", d_pixels, width, height, channels,
        [&] { return extract(c, nullptr, d_pixels, image_ready, width, height, channels, summary); });
}

const DetectorContext *detector_of(const osfm_surf *c) { return c; }

}  // namespace osfm

extern "C" {

int osfm_surf_options_default(osfm_surf_options *o)
{
    if (!o) { set_error("osfm_surf_options_default: null argument"); return OSFM_E_ARG; }
    o->contrast_threshold = 500.0f;
    o->use_upright_descriptor = 0;
    o->max_keypoints = 65536;
    return OSFM_OK;
}

int osfm_surf_create(int device, int max_width, int max_height, const osfm_surf_options *opts, osfm_surf **out)
{
    if (!out) { set_error("osfm_surf_create: null argument"); return OSFM_E_ARG; }
    *out = nullptr;
    osfm_surf_options o;
    (void)osfm_surf_options_default(&o);
    if (opts) o = *opts;
    OSFM_RETURN_IF(check_bounds("osfm_surf_create", max_width, max_height));
    if (o.max_keypoints < 1) { set_error("osfm_surf_create: invalid options (max_keypoints >= 1)"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(select_device("osfm_surf_create", device));
    std::unique_ptr<osfm_surf> c(new osfm_surf);
    c->opts = o;
    int blocks = 0;
    c->map_floats = plan_maps(max_width, max_height, nullptr, &blocks);
    OSFM_RETURN_IF(init_detector(c.get(), device, max_width, max_height, o.max_keypoints, blocks, 7));
    const size_t K = (size_t)o.max_keypoints;
    OSFM_RETURN_IF(c->sat.reserve((size_t)max_width * max_height * sizeof(Sat)));
    OSFM_RETURN_IF(c->maps.reserve(c->map_floats * sizeof(float)));
    OSFM_RETURN_IF(c->table.reserve(sizeof(OriTable)));
    OSFM_RETURN_IF(c->weights.reserve(400 * sizeof(float)));
    OSFM_RETURN_IF(c->ori_jobs.reserve(K * sizeof(OriJob)));
    OSFM_RETURN_IF(c->ori_out.reserve(K * sizeof(OriResult)));
    // one slot more than descriptors: osfm_surf_debug_describe's
    OSFM_RETURN_IF(c->desc_jobs.reserve((K + 1) * sizeof(DescJob)));
    OSFM_RETURN_IF(c->desc.reserve((K + 1) * 64 * sizeof(float)));
    OSFM_RETURN_IF(c->status.reserve((K + 1) * sizeof(int32_t)));
    // the orientation window's Gaussian (sigma 2.5) as the reference spells it: six significant digits
    OriTable table;
    int index = 0;
    for (int ry = -5; ry <= 5; ++ry)
        for (int rx = -5; rx <= 5; ++rx) {
            if (rx * rx + ry * ry >= 36) continue;
            char text[32];
            std::snprintf(text, sizeof(text), "%.6g", std::exp(-(double)(rx * rx + ry * ry) / 12.5));
            table.gauss[index] = (float)std::strtod(text, nullptr);
            table.rx[index] = (signed char)rx;
            table.ry[index] = (signed char)ry;
            ++index;
        }
    // the descriptor's Gaussian (sigma 3.3 s) by the reference's float expression with the C library's expf
    float weights[400];
    const float six = 2.0f * 3.3f, sq = six * six;
    for (int y = -10; y < 10; ++y)
        for (int x = -10; x < 10; ++x) weights[(y + 10) * 20 + (x + 10)] = std::exp(-(float)(x * x + y * y) / sq);
    OSFM_HIP_CHECK(hipMemcpyAsync(c->table.ptr, &table, sizeof(table), hipMemcpyHostToDevice, c->stream));
    OSFM_HIP_CHECK(hipMemcpyAsync(c->weights.ptr, weights, sizeof(weights), hipMemcpyHostToDevice, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    *out = c.release();
    return OSFM_OK;
}

int osfm_surf_destroy(osfm_surf *c) { return destroy_context(c); }

int osfm_surf_extract(osfm_surf *c, const uint8_t *pixels, int width, int height, int channels, osfm_surf_summary *summary)
{
    return run_extract(c, "osfm_surf_extract", pixels, width, height, channels,
        [&] { return extract(c, pixels, nullptr, nullptr, width, height, channels, summary); });
}

int osfm_surf_download(osfm_surf *c, float *descriptors, float *positions, float *scale, float *orientation, uint8_t *colors,
    float *normalized_positions)
{
    return download_features(c, "osfm_surf_download", 64, descriptors, positions, scale, orientation, colors, normalized_positions);
}

int osfm_surf_debug_image(osfm_surf *c, int octave, int sample, float *out, int32_t *width, int32_t *height)
{
    if (!c) { set_error("osfm_surf_debug_image: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_surf_debug_image: no extraction"); return OSFM_E_STATE; }
    if (octave < 0 || octave >= kOctaves || sample < 0 || sample >= kSamples) {
        set_error("osfm_surf_debug_image: octave %d sample %d out of range", octave, sample);
        return OSFM_E_ARG;
    }
    const int w = c->view.ow[octave], h = c->view.oh[octave];
    if (width) *width = w;
    if (height) *height = h;
    if (!out) return OSFM_OK;
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const size_t plane = (size_t)w * h;
    OSFM_HIP_CHECK(hipMemcpyAsync(out, c->view.maps + c->view.offset[octave] + (size_t)sample * plane, plane * sizeof(float),
        hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OSFM_OK;
}

int osfm_surf_debug_keypoints(osfm_surf *c, int after_localisation, float *out, int32_t *count)
{
    return debug_keypoints(c, "osfm_surf_debug_keypoints", after_localisation, out, count);
}

int osfm_surf_debug_describe(osfm_surf *c, float x, float y, float scale, float orientation, int upright, float *out,
    int32_t *status)
{
    if (!c || !out || !status) { set_error("osfm_surf_debug_describe: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_surf_debug_describe: no extraction"); return OSFM_E_STATE; }
    // the largest scale of the detector is 26.0; the bound keeps the kernel's int products of the scale small
    if (!(scale >= 1.0f && scale < 65.0f)) {
        set_error("osfm_surf_debug_describe: scale %g outside [1, 65)", (double)scale);
        return OSFM_E_ARG;
    }
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    DescJob j{x, y, (int)scale, 0.0f, 1.0f};
    if (!upright) {
        j.sin_ori = std::sin(orientation);
        j.cos_ori = std::cos(orientation);
    }
    // the hook borrows the slot behind the last extraction's descriptors, so that a download still returns those
    const size_t slot = c->rows.empty() ? 0 : (size_t)c->rows.back() + 1;
    hipStream_t s = c->stream;
    DescJob *d_job = c->desc_jobs.as<DescJob>() + slot;
    OSFM_HIP_CHECK(hipMemcpyAsync(d_job, &j, sizeof(j), hipMemcpyHostToDevice, s));
    launch_descriptor(s, c->sat.as<Sat>(), c->width, c->height, c->weights.as<float>(), d_job, 1, c->desc.as<float>() + slot * 64,
        c->status.as<int32_t>() + slot);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipMemcpyAsync(out, c->desc.as<float>() + slot * 64, 64 * sizeof(float), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(status, c->status.as<int32_t>() + slot, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    return OSFM_OK;
}

}  // extern "C"
