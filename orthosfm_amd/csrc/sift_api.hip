// C ABI of the SIFT extraction (include/osfm_hip.h, "SIFT feature extraction"): owns the pyramid, runs the
// stages of sift_kernels.hip in the reference's order, and keeps FeatureSet::compute_sift's view of the result.
// What an extraction shares with SURF's is detector_context.h's.
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>

#include "detector_context.h"
#include "feature_device.h"
#include "sift_kernels.h"

using namespace osfm;
using namespace osfm::sift;

namespace {

// Kernel weights of blur_gaussian, by the reference's float expression with the C library's expf; ks = 0: a copy.
BlurWeights gaussian_weights(float sigma)
{
    BlurWeights wt;
    std::memset(&wt, 0, sizeof(wt));
    if ((0.0f - 0.1f) <= sigma && sigma <= (0.0f + 0.1f)) return wt;
    wt.ks = (int)std::ceil(sigma * 2.884f);
    for (int i = 0; i <= wt.ks && i <= kMaxRadius; ++i) {
        const float x = (float)i;
        wt.w[i] = std::exp(-((x * x) / (2.0f * sigma * sigma)));
    }
    return wt;
}

struct OctavePlan {
    int index;
    bool blur_base;           // the first image is blurred (false: copied)
    BlurWeights base, step[kMaxImages];
};

// The blur of every image of the pyramid, as Sift::create_octaves / add_octave compute it.
void plan_octave(const osfm_sift_options &o, float has_sigma, OctavePlan *p)
{
    const float target = o.base_blur_sigma;
    p->blur_base = target > has_sigma;
    if (p->blur_base) p->base = gaussian_weights(std::sqrt(target * target - has_sigma * has_sigma));
    const float k = std::pow(2.0f, 1.0f / o.num_samples_per_octave);
    float sigma = target;
    for (int i = 1; i < o.num_samples_per_octave + 3; ++i) {
        const float sigmak = sigma * k;
        p->step[i] = gaussian_weights(std::sqrt(sigmak * sigmak - sigma * sigma));
        sigma = sigmak;
    }
}

}  // namespace

struct osfm_sift : DetectorContext {
    osfm_sift_options opts{};
    std::vector<OctavePlan> plan;          // blur weights per octave
    DeviceBuffer pyramid, sigma, num_ori, oris, jobs;
    size_t pyramid_floats = 0;
    PyramidView view{};                    // of the last extraction
};

namespace {

// Octave sizes for an image of w x h (min_octave is -1 or 0); false where the reference throws: it halves the image
// once after every octave, the last included, and halving needs 2 pixels a side.
bool octave_sizes(const osfm_sift_options &o, int w, int h, std::vector<std::pair<int, int>> *sizes)
{
    if (o.min_octave < 0) sizes->push_back({2 * w, 2 * h});
    for (int i = 0; i <= o.max_octave; ++i) {
        sizes->push_back({w, h});
        if (w < 2 || h < 2) return false;
        w = (w + 1) >> 1; h = (h + 1) >> 1;
    }
    return true;
}

// Floats of the pyramid for an image of w x h: the float image, the doubled image, the chain of halved images,
// one scratch plane of the largest octave, and per octave S + 3 images and S + 2 DoG images.
size_t pyramid_size(const osfm_sift_options &o, int w, int h)
{
    std::vector<std::pair<int, int>> sizes;
    (void)octave_sizes(o, w, h, &sizes);
    size_t n = (size_t)w * h;
    int ww = w, hh = h;
    for (int i = 0; i < o.max_octave + 1; ++i) { ww = (ww + 1) >> 1; hh = (hh + 1) >> 1; n += (size_t)ww * hh; }
    size_t largest = 0;
    for (auto &s : sizes) {
        const size_t plane = (size_t)s.first * s.second;
        largest = std::max(largest, plane);
        n += plane * (2 * o.num_samples_per_octave + 5);
    }
    if (o.min_octave < 0) n += (size_t)4 * w * h;
    return n + largest;
}

int copy_image(osfm_sift *c, const float *src, int w, int h, float *out)
{
    OSFM_HIP_CHECK(hipMemcpyAsync(out, src, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    OSFM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OSFM_OK;
}

// pixels: the image in host memory, uploaded here; or NULL with d_pixels, the image on the device, read once
// image_ready has happened (the colours and normalised positions then stay with the caller).
int extract(osfm_sift *c, const uint8_t *pixels, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height,
    int channels, osfm_sift_summary *sum_out)
{
    const osfm_sift_options &o = c->opts;
    const int S = o.num_samples_per_octave;
    std::vector<std::pair<int, int>> sizes;
    if (!octave_sizes(o, width, height, &sizes)) {
        set_error("osfm_sift_extract: a %d x %d image is too small for octaves %d..%d: the reference halves it once per "
            "octave, the last included, and halving needs 2 pixels a side", width, height, o.min_octave, o.max_octave);
        return OSFM_E_ARG;
    }
    hipStream_t s = c->stream;

    // ---- where everything lies in the context's pyramid, checked before the first launch
    float *p = c->pyramid.as<float>();
    auto take = [&p](size_t n) { float *r = p; p += n; return r; };
    float *orig = take((size_t)width * height);
    size_t largest = 0;
    for (auto &z : sizes) largest = std::max(largest, (size_t)z.first * z.second);
    float *sep = take(largest);
    PyramidView pv{};
    pv.num_octaves = (int)sizes.size();
    pv.S = S;
    pv.min_octave = o.min_octave;
    std::vector<float *> halves;           // the chain of halved inputs, in the order they are made
    float *dbl = nullptr;
    int total_blocks = 0;
    {
        int sw = width, sh = height;
        auto halve = [&]() { sw = (sw + 1) >> 1; sh = (sh + 1) >> 1; halves.push_back(take((size_t)sw * sh)); };
        for (int oi = 0; oi < pv.num_octaves; ++oi) {
            OctaveView &ov = pv.oct[oi];
            ov.w = sizes[oi].first; ov.h = sizes[oi].second;
            const size_t plane = (size_t)ov.w * ov.h;
            ov.img = take(plane * (S + 3));
            ov.dog = take(plane * (S + 2));
            if (c->plan[oi].index < 0) dbl = take(plane);
            else halve();
            total_blocks += S * extrema_blocks(ov.w, ov.h);
        }
    }
    if ((size_t)(p - c->pyramid.as<float>()) > c->pyramid_floats || total_blocks > c->max_blocks) {
        set_error("osfm_sift_extract: internal: the pyramid of %d x %d exceeds the context's", width, height);
        return OSFM_E_STATE;
    }

    // ---- scale space
    OSFM_HIP_CHECK(hipEventRecord(c->ev[0], s));
    OSFM_RETURN_IF(stage_image(c, pixels, (size_t)width * height * channels, image_ready, &d_pixels));
    launch_to_float(s, d_pixels, width, height, channels, orig);
    const float hs = 0.866025403784439f;       // rescale_half_size_gaussian's default sigma
    const float hw1 = std::exp(-0.5f / (2.0f * (hs * hs))), hw2 = std::exp(-2.5f / (2.0f * (hs * hs))),
                hw3 = std::exp(-4.5f / (2.0f * (hs * hs)));
    const float *seed = orig;
    int sw = width, sh = height;
    size_t next_half = 0;
    auto halve = [&]() {
        float *half = halves[next_half++];
        launch_half_size(s, seed, sw, sh, half, hw1, hw2, hw3);
        seed = half; sw = (sw + 1) >> 1; sh = (sh + 1) >> 1;
    };
    for (int oi = 0; oi < pv.num_octaves; ++oi) {
        const OctavePlan &pl = c->plan[oi];
        const OctaveView &ov = pv.oct[oi];
        const int w = ov.w, h = ov.h;
        const size_t plane = (size_t)w * h;
        const float *src = seed;
        if (pl.index < 0) {
            launch_double_size(s, orig, width, height, dbl);
            src = dbl;
        }
        if (pl.blur_base && pl.base.ks > 0) launch_blur(s, src, sep, ov.img, nullptr, nullptr, w, h, pl.base);
        else OSFM_HIP_CHECK(hipMemcpyAsync(ov.img, src, plane * sizeof(float), hipMemcpyDeviceToDevice, s));
        for (int i = 1; i < S + 3; ++i) {
            float *prev = ov.img + (size_t)(i - 1) * plane, *cur = ov.img + (size_t)i * plane;
            float *dog = ov.dog + (size_t)(i - 1) * plane;
            if (pl.step[i].ks > 0) launch_blur(s, prev, sep, cur, prev, dog, w, h, pl.step[i]);
            else {   // blur_gaussian returns a copy for sigma < 0.1: the DoG image is zero
                OSFM_HIP_CHECK(hipMemcpyAsync(cur, prev, plane * sizeof(float), hipMemcpyDeviceToDevice, s));
                OSFM_HIP_CHECK(hipMemsetAsync(dog, 0, plane * sizeof(float), s));
            }
        }
        if (pl.index >= 0) halve();   // the next octave starts from the halved input of this one, not from its blurred image
    }
    OSFM_HIP_CHECK(hipGetLastError());

    // ---- extrema: count per workgroup, scan, write in (octave, sample, y, x) order
    OSFM_HIP_CHECK(hipEventRecord(c->ev[1], s));
    Keypoint *cand = c->cand.as<Keypoint>();
    OSFM_RETURN_IF(find_candidates(c, "osfm_sift_extract", pv.num_octaves, 0, S, [&](int oi, int si, int base, const int32_t *offsets) {
        const OctaveView &ov = pv.oct[oi];
        const size_t plane = (size_t)ov.w * ov.h;
        const float *d0 = ov.dog + (size_t)si * plane;
        launch_extrema(s, d0, d0 + plane, d0 + 2 * plane, ov.w, ov.h, base, c->counts.as<int32_t>(), offsets, cand, o.max_keypoints,
            (float)(oi + o.min_octave), (float)si);
        return extrema_blocks(ov.w, ov.h);
    }));
    const int n_cand = c->n_cand;

    // ---- localisation, compaction, and sigma / scale from the C library's powf on the host
    OSFM_HIP_CHECK(hipEventRecord(c->ev[2], s));
    std::vector<Keypoint> h_kps;
    if (n_cand > 0) {
        LocaliseParams prm;
        prm.contrast_threshold = o.contrast_threshold;
        prm.score_threshold = ((o.edge_ratio_threshold + 1.0f) * (o.edge_ratio_threshold + 1.0f)) / o.edge_ratio_threshold;
        launch_localise(s, pv, prm, cand, n_cand, c->moved.as<Keypoint>(), c->keep.as<uint8_t>(), c->counts.as<int32_t>());
    }
    OSFM_RETURN_IF(compact_keypoints(c, &h_kps));
    const int n_kp = c->n_kp;
    std::vector<float> sigma((size_t)n_kp), abs_scale((size_t)n_kp);
    for (int i = 0; i < n_kp; ++i) {
        const Keypoint &k = h_kps[(size_t)i];
        // Sift::keypoint_relative_scale / keypoint_absolute_scale
        sigma[(size_t)i] = o.base_blur_sigma * std::pow(2.0f, (k.sample + 1.0f) / S);
        abs_scale[(size_t)i] = o.base_blur_sigma * std::pow(2.0f, (int)k.octave + (k.sample + 1.0f) / S);
    }

    // ---- orientation assignment
    OSFM_HIP_CHECK(hipEventRecord(c->ev[3], s));
    std::vector<int32_t> num_ori((size_t)n_kp);
    std::vector<float> oris((size_t)n_kp * kMaxOrientations);
    std::vector<DescriptorJob> jobs;
    if (n_kp) {
        OSFM_HIP_CHECK(hipMemcpyAsync(c->sigma.ptr, sigma.data(), (size_t)n_kp * sizeof(float), hipMemcpyHostToDevice, s));
        launch_orientation(s, pv, c->kps.as<Keypoint>(), c->sigma.as<float>(), n_kp, c->num_ori.as<int32_t>(), c->oris.as<float>());
        OSFM_HIP_CHECK(hipMemcpyAsync(num_ori.data(), c->num_ori.ptr, (size_t)n_kp * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipMemcpyAsync(oris.data(), c->oris.ptr, oris.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        OSFM_HIP_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < n_kp; ++i)
            for (int j = 0; j < num_ori[(size_t)i]; ++j) jobs.push_back({i, oris[(size_t)i * kMaxOrientations + j]});
    }
    const int n_desc = (int)jobs.size();
    if (n_desc > o.max_keypoints) {
        set_error("osfm_sift_extract: %d descriptors exceed max_keypoints %d", n_desc, o.max_keypoints);
        return OSFM_E_CAPACITY;
    }

    // ---- descriptors
    OSFM_HIP_CHECK(hipEventRecord(c->ev[4], s));
    if (n_desc) {
        OSFM_HIP_CHECK(hipMemcpyAsync(c->jobs.ptr, jobs.data(), (size_t)n_desc * sizeof(DescriptorJob), hipMemcpyHostToDevice, s));
        launch_descriptor(s, pv, c->kps.as<Keypoint>(), c->sigma.as<float>(), c->jobs.as<DescriptorJob>(), n_desc, c->desc.as<float>());
    }
    OSFM_HIP_CHECK(hipEventRecord(c->ev[5], s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    OSFM_HIP_CHECK(hipGetLastError());

    // ---- FeatureSet::compute_sift's view: positions, colours, the order by scale
    osfm_sift_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    sum.num_candidates = n_cand; sum.num_keypoints = n_kp; sum.num_descriptors = n_desc; sum.num_octaves = pv.num_octaves;
    for (const Keypoint &k : h_kps) sum.keypoints_per_octave[(int)k.octave - o.min_octave]++;
    begin_rows(c, n_desc);
    for (int j = 0; j < n_desc; ++j) {
        const Keypoint &k = h_kps[(size_t)jobs[(size_t)j].keypoint];
        sum.descriptors_per_octave[(int)k.octave - o.min_octave]++;
        const float factor = (float)std::pow(2.0, (double)(int)k.octave);
        c->positions[2 * (size_t)j] = factor * (k.x + 0.5f) - 0.5f;
        c->positions[2 * (size_t)j + 1] = factor * (k.y + 0.5f) - 0.5f;
        c->scale[(size_t)j] = abs_scale[(size_t)jobs[(size_t)j].keypoint];
        c->orientation[(size_t)j] = jobs[(size_t)j].orientation;
    }
    float ms[5] = {};
    OSFM_RETURN_IF(finish_rows(c, pixels, width, height, channels, ms, &sum.total_ms));
    sum.scale_space_ms = ms[0]; sum.extrema_ms = ms[1]; sum.localisation_ms = ms[2]; sum.orientation_ms = ms[3];
    sum.descriptor_ms = ms[4];
    c->view = pv;
    c->have = true;
    if (sum_out) *sum_out = sum;
    return OSFM_OK;
}

}  // namespace

namespace osfm {

int sift_extract_device(osfm_sift *c, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height, int channels,
    osfm_sift_summary *summary)
{
    return run_extract(c, "osfm_sift_extract", d_pixels, width, height, channels,
        [&] { return extract(c, nullptr, d_pixels, image_ready, width, height, channels, summary); });
}

const DetectorContext *detector_of(const osfm_sift *c) { return c; }

}  // namespace osfm

extern "C" {

int osfm_sift_options_default(osfm_sift_options *o)
{
    if (!o) { set_error("osfm_sift_options_default: null argument"); return OSFM_E_ARG; }
    o->num_samples_per_octave = 3;
    o->min_octave = 0;
    o->max_octave = 4;
    o->contrast_threshold = -1.0f;
    o->edge_ratio_threshold = 10.0f;
    o->base_blur_sigma = 1.6f;
    o->inherent_blur_sigma = 0.5f;
    o->max_keypoints = 65536;
    return OSFM_OK;
}

int osfm_sift_create(int device, int max_width, int max_height, const osfm_sift_options *opts, osfm_sift **out)
{
    if (!out) { set_error("osfm_sift_create: null argument"); return OSFM_E_ARG; }
    *out = nullptr;
    osfm_sift_options o;
    (void)osfm_sift_options_default(&o);
    if (opts) o = *opts;
    const int S = o.num_samples_per_octave;
    OSFM_RETURN_IF(check_bounds("osfm_sift_create", max_width, max_height));
    if (o.min_octave > 0) {
        set_error("osfm_sift_create: min_octave %d: the first octave is the image (0) or the doubled image (-1)", o.min_octave);
        return OSFM_E_ARG;
    }
    if (S < 1 || S + 3 > kMaxImages || o.min_octave < -1 || o.min_octave > o.max_octave
        || o.max_octave - o.min_octave + 1 > kMaxOctaves || o.max_octave - o.min_octave + 1 > OSFM_SIFT_MAX_OCTAVES
        || o.max_keypoints < 1 || !(o.edge_ratio_threshold > 0.0f) || !(o.base_blur_sigma > 0.0f)
        || !(o.inherent_blur_sigma >= 0.0f)) {
        set_error("osfm_sift_create: invalid options (samples per octave 1..%d, octaves -1 <= min <= max, at most %d of them, "
            "max_keypoints >= 1, positive sigmas)", kMaxImages - 3, kMaxOctaves);
        return OSFM_E_ARG;
    }
    // Sift::Sift: a negative contrast threshold means the default
    if (o.contrast_threshold < 0.0f) o.contrast_threshold = 0.02f / (float)S;
    OSFM_RETURN_IF(select_device("osfm_sift_create", device));
    std::unique_ptr<osfm_sift> c(new osfm_sift);
    c->opts = o;
    // the blur of every octave: the doubled image has twice the inherent blur, octave 0 the inherent blur, every
    // later octave the base blur
    for (int i = o.min_octave; i <= o.max_octave; ++i) {
        OctavePlan pl;
        std::memset(&pl, 0, sizeof(pl));
        pl.index = i;
        plan_octave(o, i < 0 ? o.inherent_blur_sigma * 2.0f : i == 0 ? o.inherent_blur_sigma : o.base_blur_sigma, &pl);
        int ks = pl.blur_base ? pl.base.ks : 0;
        for (int k = 1; k < S + 3; ++k) ks = std::max(ks, pl.step[k].ks);
        if (ks > kMaxRadius) {
            set_error("osfm_sift_create: these sigmas need a blur radius of %d, the kernels hold %d", ks, kMaxRadius);
            return OSFM_E_ARG;
        }
        c->plan.push_back(pl);
    }
    std::vector<std::pair<int, int>> sizes;
    (void)octave_sizes(o, max_width, max_height, &sizes);
    int blocks = 0;
    for (auto &z : sizes) blocks += S * extrema_blocks(z.first, z.second);
    OSFM_RETURN_IF(init_detector(c.get(), device, max_width, max_height, o.max_keypoints, blocks, 6));
    c->pyramid_floats = pyramid_size(o, max_width, max_height);
    const size_t K = (size_t)o.max_keypoints;
    OSFM_RETURN_IF(c->pyramid.reserve(c->pyramid_floats * sizeof(float)));
    OSFM_RETURN_IF(c->sigma.reserve(K * sizeof(float)));
    OSFM_RETURN_IF(c->num_ori.reserve(K * sizeof(int32_t)));
    OSFM_RETURN_IF(c->oris.reserve(K * kMaxOrientations * sizeof(float)));
    OSFM_RETURN_IF(c->jobs.reserve(K * sizeof(DescriptorJob)));
    OSFM_RETURN_IF(c->desc.reserve(K * 128 * sizeof(float)));
    *out = c.release();
    return OSFM_OK;
}

int osfm_sift_destroy(osfm_sift *c) { return destroy_context(c); }

int osfm_sift_extract(osfm_sift *c, const uint8_t *pixels, int width, int height, int channels, osfm_sift_summary *summary)
{
    return run_extract(c, "osfm_sift_extract", pixels, width, height, channels,
        [&] { return extract(c, pixels, nullptr, nullptr, width, height, channels, summary); });
}

int osfm_sift_download(osfm_sift *c, float *descriptors, float *positions, float *scale, float *orientation, uint8_t *colors,
    float *normalized_positions)
{
    return download_features(c, "osfm_sift_download", 128, descriptors, positions, scale, orientation, colors, normalized_positions);
}

int osfm_sift_debug_image(osfm_sift *c, int octave, int kind, int index, float *out, int32_t *width, int32_t *height)
{
    if (!c) { set_error("osfm_sift_debug_image: null argument"); return OSFM_E_ARG; }
    if (!c->have) { set_error("osfm_sift_debug_image: no extraction"); return OSFM_E_STATE; }
    const int oi = octave - c->opts.min_octave, S = c->opts.num_samples_per_octave;
    if (oi < 0 || oi >= c->view.num_octaves || kind < 0 || kind > 1 || index < 0 || index >= S + 3 - kind) {
        set_error("osfm_sift_debug_image: octave %d kind %d index %d out of range", octave, kind, index);
        return OSFM_E_ARG;
    }
    const OctaveView &ov = c->view.oct[oi];
    if (width) *width = ov.w;
    if (height) *height = ov.h;
    if (!out) return OSFM_OK;
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    return copy_image(c, (kind ? ov.dog : ov.img) + (size_t)index * ov.w * ov.h, ov.w, ov.h, out);
}

int osfm_sift_debug_keypoints(osfm_sift *c, int after_localisation, float *out, int32_t *count)
{
    return debug_keypoints(c, "osfm_sift_debug_keypoints", after_localisation, out, count);
}

}  // extern "C"
