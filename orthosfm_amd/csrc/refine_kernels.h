// Sub-pixel refinement of track observations by affine least-squares matching (DESIGN.md "Observation refinement").
// tests/refine_restatement.py is the definition in numpy; this header holds what the kernels (refine_kernels.hip) and
// the C entries (refine_api.hip) share.
#pragma once
#include "osfm_common.h"

namespace osfm {
namespace refine {

constexpr int kWavesPerGroup = 4;                              // one wave per observation, 256 threads a workgroup
constexpr int kMaxRadius = 15;
constexpr int kMaxSamples = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);      // 961: 16 strides of 64 lanes
constexpr int kParams = 8;                                     // px, py, a00, a01, a10, a11, gain, bias
constexpr int kSums = kParams * (kParams + 1) / 2 + kParams + 1;    // 36 + 8 + the cost

// A view's grey image on the device: float32, row-major, no padding.  px == nullptr: no image.
struct Image {
    const float *px;
    int32_t w, h;
};

struct Tracks {
    int64_t num_tracks, num_obs;
    const int64_t *offsets;       // [T + 1]
    const int32_t *view;          // [F]
    const double *xy;             // [F][2]
    const uint8_t *alive;         // [F] or nullptr
    const double *init_affine;    // [F][4] or nullptr
};

// the small pass's output, then the main kernel's
struct Work {
    int64_t *ref_obs;             // [T]: the first alive observation, -1 without one
    int32_t *alive_count;         // [T]
    int32_t *track_of;            // [F]
};
struct Out {
    double *xy, *affine, *score;  // [F][2], [F][4], [F]
    int32_t *status, *iterations; // [F]
};

// uint8 [h][w][channels] -> float32 [h][w]: the byte, or (float)(r + g + b) / 3.0f
void launch_grey(hipStream_t s, const uint8_t *pixels, int w, int h, int channels, float *out);
void launch_track_pass(hipStream_t s, const Tracks &t, const Work &w);
void launch_refine(hipStream_t s, const Image *images, const Tracks &t, const Work &w, const osfm_refine_options &o, const Out &out);

}  // namespace refine
}  // namespace osfm
