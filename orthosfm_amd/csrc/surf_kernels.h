// SURF extraction kernels (surf_kernels.hip) as the C ABI (surf_api.hip) launches them.  The detector is MVE's
// sfm/surf.cc: an integer summed-area table, Hessian response maps, extrema, one Newton step, a sliding-window
// orientation and a 4 x 4 x 4 descriptor.  Every stage keeps the reference's operation order and types, and the
// values of C-library functions come from the host, so that every stage's result equals the reference's bytes
// (DESIGN.md 3u names the one decision that cannot be pinned).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "detect_kernels.h"

namespace osfm {
namespace surf {

using detect::kBlock;
using detect::Keypoint;             // rows (octave, sample, x, y), as the SIFT stages keep them

constexpr int kOctaves = 4, kSamples = 4;
constexpr int kOriSamples = 109;    // grid points of a circle of radius 6
constexpr int kWindows = 16;        // for (deg = -pi; deg < pi; deg += pi / 8)
constexpr int kDescBlock = 448;     // 400 sample lanes in whole waves

// The table is modular: every filter is a sum of box sums far below 2^31 in magnitude, so 32-bit wrap-around
// arithmetic returns the exact integer the reference's int64 table gives.
using Sat = uint32_t;

struct MapsView {                   // the 4 x 4 response maps: plane k of octave o at maps + offset[o] + k * ow * oh
    float *maps;
    int ow[kOctaves], oh[kOctaves];
    unsigned long long offset[kOctaves];
};

struct OctaveFilters {              // kernel_sizes[o][*] and float(1.0 / (fs * (2 fs - 1)))
    int fs[kSamples];
    float inv_karea[kSamples];
};

struct OriTable {                   // the 109 samples in (ry, rx) order with their Gaussian weights
    float gauss[kOriSamples];
    signed char rx[kOriSamples], ry[kOriSamples];
};

struct OriJob {                     // descriptor_orientation's integer view of a keypoint
    int32_t x, y, scale;
};

struct OriResult {
    double best_dx, best_dy;
    int32_t ok, reserved;           // 0: rejected by the margin test
};

struct DescJob {                    // descriptor_computation's input; sin / cos from the host's C library
    float x, y;
    int32_t scale;
    float sin_ori, cos_ori;
};

// Inclusive integral image of the desaturated bytes (1 channel: the bytes; 3: DESATURATE_LIGHTNESS).
void launch_sat(hipStream_t s, const uint8_t *pixels, int w, int h, int channels, Sat *sat);
void launch_response(hipStream_t s, const Sat *sat, int w, int h, int octave, OctaveFilters f, float *maps, int ow, int oh);
// Per workgroup of kBlock pixels (x in 1 .. ow - 2, every row) of sample `sample` (1 or 2): the number of maxima;
// with offsets given they are written at offsets[block_base + b] + rank, rows below `capacity` only.
void launch_extrema(hipStream_t s, const float *m0, const float *m1, const float *m2, int ow, int oh, int block_base,
    int32_t *counts, const int32_t *offsets, Keypoint *out, int capacity, float octave, float sample);
void launch_localise(hipStream_t s, MapsView maps, float contrast_threshold, int width, int height, const Keypoint *cand,
    int n, Keypoint *out, uint8_t *keep, int32_t *counts);
void launch_orientation(hipStream_t s, const Sat *sat, int w, int h, const OriTable *table, const OriJob *jobs, int n,
    OriResult *out);
// out[n][64]; status[n]: 0 rejected, 1 ok, 2 ok with taps outside the table read as zero.  weights: the 20 x 20 expf table.
void launch_descriptor(hipStream_t s, const Sat *sat, int w, int h, const float *weights, const DescJob *jobs, int n,
    float *out, int32_t *status);

inline int extrema_blocks(int ow, int oh)
{
    if (ow < 3 || oh < 1) return 0;
    const long long n = (long long)(ow - 2) * oh;
    return (int)((n + kBlock - 1) / kBlock);
}

}  // namespace surf
}  // namespace osfm
