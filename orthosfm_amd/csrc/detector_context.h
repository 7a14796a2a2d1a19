// What the SIFT and the SURF context (sift_api.hip, surf_api.hip) have in common: the stream and stage events, the
// buffers of the candidate search and the compaction (detect_kernels.hip), FeatureSet's view of the last extraction,
// and the steps of an extraction that do not depend on the detector.  Each step takes the API's name for its error
// messages.  The view front end (view_api.hip) shares the argument checks and the descriptor gather, and reads the
// detectors' results here.  Not part of the C ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "detect_kernels.h"
#include "osfm_common.h"

namespace osfm {

struct DetectorContext {
    int device = 0, max_w = 0, max_h = 0, max_keypoints = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {};                 // the stage boundaries of an extraction; num_events of them exist
    int num_events = 0;
    DeviceBuffer pixels, cand, moved, kps, keep, counts, total;
    DeviceBuffer desc;                     // [.][128] (SIFT) or [.][64] (SURF); reserved by the detector
    int max_blocks = 0;
    // the last extraction
    bool have = false;
    int n_cand = 0, n_kp = 0, n_desc = 0;
    std::vector<int32_t> rows;             // SURF: generation row j is row rows[j] of desc; SIFT: empty, row j itself
    std::vector<float> positions, scale, orientation, normalized;   // in generation order
    std::vector<uint8_t> colors;
    std::vector<int32_t> order;            // FeatureSet's order: row i is generation row order[i]
    ~DetectorContext()
    {
        for (auto &e : ev) event_destroy(e);
        stream_destroy(stream);
    }
    // row of desc that holds generation row g
    int32_t desc_row(size_t g) const { return rows.empty() ? (int32_t)g : rows[g]; }
};

// ---- create
int check_bounds(const char *api, int max_width, int max_height);          // 1..16384 a side
int select_device(const char *api, int device);                            // checks the index, makes it current
// The bounds, the seven common buffers for max_keypoints candidates and `extrema_blocks` workgroups of the candidate
// search, the stream and `num_events` timing events.
int init_detector(DetectorContext *c, int device, int max_width, int max_height, int max_keypoints, int extrema_blocks,
    int num_events);
template <class Context> int destroy_context(Context *c)
{
    if (!c) return OSFM_OK;
    (void)hipSetDevice(c->device);
    delete c;
    return OSFM_OK;
}

// ---- extract
// owner: whose bound the image exceeds ("context", "front end")
int check_image(const char *api, const char *owner, int max_w, int max_h, int width, int height, int channels);
// The body of every extract entry around `run`, the detector's extraction.  image: the caller's pointer, host or device.
template <class Run> int run_extract(DetectorContext *c, const char *api, const void *image, int width, int height, int channels, Run run)
{
    if (!c || !image) { set_error("%s: null argument", api); return OSFM_E_ARG; }
    c->have = false;          // whatever comes of this call, the previous result is gone
    OSFM_RETURN_IF(check_image(api, "context", c->max_w, c->max_h, width, height, channels));
    OSFM_HIP_CHECK(hipSetDevice(c->device));
    const int rc = run();
    if (rc != OSFM_OK) (void)hipStreamSynchronize(c->stream);   // nothing of a failed call may still run
    return rc;
}
// pixels: the image in host memory, uploaded here; or NULL with *d_pixels, the image on the device, read once
// image_ready has happened.  *d_pixels: where the stream's kernels read the image.
int stage_image(DetectorContext *c, const uint8_t *pixels, size_t bytes, hipEvent_t image_ready, const uint8_t **d_pixels);

// Candidates in (octave, sample, y, x) order: count per workgroup, scan, ranked write; n_cand, refused over
// max_keypoints.  plane(octave, sample, block_base, offsets) launches the detector's extrema pass of one plane
// (offsets NULL: the count pass) and returns its number of workgroups.
template <class Plane> int find_candidates(DetectorContext *c, const char *api, int octaves, int sample_begin, int sample_end, Plane plane)
{
    hipStream_t s = c->stream;
    int32_t *counts = c->counts.as<int32_t>(), *total = c->total.as<int32_t>();
    for (int pass = 0; pass < 2; ++pass) {
        int base = 0;
        for (int oi = 0; oi < octaves; ++oi)
            for (int si = sample_begin; si < sample_end; ++si) base += plane(oi, si, base, pass ? counts : nullptr);
        if (!pass) detect::launch_scan(s, counts, base, total);
    }
    OSFM_HIP_CHECK(hipMemcpyAsync(&c->n_cand, total, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    if (c->n_cand > c->max_keypoints) {
        set_error("%s: %d candidates exceed max_keypoints %d", api, c->n_cand, c->max_keypoints);
        return OSFM_E_CAPACITY;
    }
    return OSFM_OK;
}
// After the detector's localisation of the n_cand candidates into moved / keep / counts: the kept ones, in order, in
// kps and on the host; n_kp.  Without candidates nothing is launched.
int compact_keypoints(DetectorContext *c, std::vector<detect::Keypoint> *h_kps);
// The closing step, in two halves around the detector's loop that fills positions / scale / orientation:
// begin_rows sizes the host arrays for n_desc rows; finish_rows adds colours and normalised positions (pixels: the
// image in host memory, or NULL), the order by scale, and ms[num_events - 1], the stage times, with their sum.
void begin_rows(DetectorContext *c, int n_desc);
int finish_rows(DetectorContext *c, const uint8_t *pixels, int width, int height, int channels, float *ms, double *total_ms);

// ---- results
// out[i] = row map[i] of d_desc, `dim` floats each
int gather_descriptors(hipStream_t s, const float *d_desc, const std::vector<int32_t> &map, int dim, float *out);
// osfm_sift_download / osfm_surf_download: the descriptors of `dim` floats and the per-row arrays, in FeatureSet's order
int download_features(DetectorContext *c, const char *api, int dim, float *descriptors, float *positions, float *scale,
    float *orientation, uint8_t *colors, float *normalized_positions);
int debug_keypoints(DetectorContext *c, const char *api, int after_localisation, float *out, int32_t *count);

}  // namespace osfm
