// The ordered compaction that the SIFT and the SURF detector share (detect_kernels.hip): a kernel counts the rows it
// would write per workgroup, a scan turns the counts into offsets, and a second pass writes every row at its
// workgroup's offset plus its rank, so that the rows come out in thread order whatever order the workgroups run in.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace osfm {
namespace detect {

constexpr int kBlock = 256;         // threads per workgroup of the per-pixel and per-candidate kernels

struct Keypoint {    // Sift::Keypoint with the octave as a float: 16 bytes
    float octave, sample, x, y;
};

// exclusive scan of counts[n] in place; *total receives the sum
void launch_scan(hipStream_t s, int32_t *counts, int n, int32_t *total);
void launch_compact(hipStream_t s, const Keypoint *in, const uint8_t *keep, const int32_t *offsets, int n, Keypoint *out);

// Rank of this thread among the flagged threads of its workgroup (kBlock threads), in thread order, and their
// number: the ranked write of the count / scan / write scheme.
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

}  // namespace detect
}  // namespace osfm
