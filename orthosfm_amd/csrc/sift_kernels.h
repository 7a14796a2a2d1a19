// SIFT extraction kernels (sift_kernels.hip) as the C ABI (sift_api.hip) launches them.  The detector is MVE's
// sfm/sift.cc: scale space, extrema and localisation keep its float32 operation order, so that their results
// are equal to its bytes; orientation assignment and the descriptor are evaluated in double.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "detect_kernels.h"

namespace osfm {
namespace sift {

using detect::kBlock;
using detect::Keypoint;

constexpr int kMaxRadius = 32;      // largest blur radius ceil(sigma * 2.884) a context accepts
constexpr int kMaxOctaves = 16;
constexpr int kMaxImages = 16;      // S + 3 images per octave
constexpr int kMaxOrientations = 18;  // strict local maxima of 36 circular bins

struct BlurWeights {
    int ks;
    float w[kMaxRadius + 1];
};

struct OctaveView {
    float *img;      // S + 3 planes of w * h
    float *dog;      // S + 2 planes
    int w, h;
};

struct PyramidView {
    int num_octaves, S, min_octave;
    OctaveView oct[kMaxOctaves];
};

struct LocaliseParams {
    float contrast_threshold, score_threshold;
};

struct DescriptorJob {
    int32_t keypoint;
    float orientation;
};

void launch_to_float(hipStream_t s, const uint8_t *pixels, int w, int h, int channels, float *out);
void launch_double_size(hipStream_t s, const float *in, int w, int h, float *out);
void launch_half_size(hipStream_t s, const float *in, int w, int h, float *out, float w1, float w2, float w3);
// out = blur(in); dog = out - base where dog is given.  sep: scratch of w * h.
void launch_blur(hipStream_t s, const float *in, float *sep, float *out, const float *base, float *dog, int w, int h,
    const BlurWeights &wt);
// Per workgroup of kBlock interior pixels of DoG triple (d0, d1, d2): the number of extrema (counts[block_base + b]);
// with offsets given the extrema are written at offsets[block_base + b] + rank, rows below `capacity` only.
void launch_extrema(hipStream_t s, const float *d0, const float *d1, const float *d2, int w, int h, int block_base,
    int32_t *counts, const int32_t *offsets, Keypoint *out, int capacity, float octave, float sample);
void launch_localise(hipStream_t s, PyramidView pyr, LocaliseParams prm, const Keypoint *cand, int n, Keypoint *out,
    uint8_t *keep, int32_t *counts);
void launch_orientation(hipStream_t s, PyramidView pyr, const Keypoint *kps, const float *sigma, int n, int32_t *num,
    float *orientations);
void launch_descriptor(hipStream_t s, PyramidView pyr, const Keypoint *kps, const float *sigma, const DescriptorJob *jobs,
    int n, float *out);

inline int extrema_blocks(int w, int h)
{
    if (w < 3 || h < 3) return 0;
    const long long n = (long long)(w - 2) * (h - 2);
    return (int)((n + kBlock - 1) / kBlock);
}

}  // namespace sift
}  // namespace osfm
