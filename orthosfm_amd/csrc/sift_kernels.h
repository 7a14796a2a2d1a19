// SIFT extraction kernels (sift_kernels.hip) as the C ABI (sift_api.hip) launches them.  The detector is MVE's
// sfm/sift.cc: scale space, extrema and localisation keep its float32 operation order, so that their results
// are equal to its bytes; orientation assignment and the descriptor are evaluated in double.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace osfm {
namespace sift {

constexpr int kMaxRadius = 32;      // largest blur radius ceil(sigma * 2.884) a context accepts
constexpr int kMaxOctaves = 16;
constexpr int kMaxImages = 16;      // S + 3 images per octave
constexpr int kMaxOrientations = 18;  // strict local maxima of 36 circular bins
constexpr int kBlock = 256;         // threads per workgroup of the per-pixel and per-candidate kernels

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

struct Keypoint {    // Sift::Keypoint with the octave as a float: 16 bytes
    float octave, sample, x, y;
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
// exclusive scan of counts[n] in place; *total receives the sum
void launch_scan(hipStream_t s, int32_t *counts, int n, int32_t *total);
void launch_localise(hipStream_t s, PyramidView pyr, LocaliseParams prm, const Keypoint *cand, int n, Keypoint *out,
    uint8_t *keep, int32_t *counts);
void launch_compact(hipStream_t s, const Keypoint *in, const uint8_t *keep, const int32_t *offsets, int n, Keypoint *out);
void launch_orientation(hipStream_t s, PyramidView pyr, const Keypoint *kps, const float *sigma, int n, int32_t *num,
    float *orientations);
void launch_descriptor(hipStream_t s, PyramidView pyr, const Keypoint *kps, const float *sigma, const DescriptorJob *jobs,
    int n, float *out);

// Rank of this thread among the flagged threads of its workgroup (kBlock threads), in thread order, and their
// number: the ranked write of the count / scan / write scheme, shared with the SURF kernels.
__device__ inline int block_rank(bool flag, int *block_total)
{
    __shared__ int wave_count[kBlock / 64];
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < kBlock / 64; ++i) {
        if (i < wave) before += wave_count[i];
        total += wave_count[i];
    }
    *block_total = total;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

inline int extrema_blocks(int w, int h)
{
    if (w < 3 || h < 3) return 0;
    const long long n = (long long)(w - 2) * (h - 2);
    return (int)((n + kBlock - 1) / kBlock);
}

}  // namespace sift
}  // namespace osfm
