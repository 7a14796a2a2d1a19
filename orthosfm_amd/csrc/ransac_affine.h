// Batched RANSAC over affine fundamental matrices (geometric verification of orthographic view pairs).
#pragma once
#include "ransac_kernels.h"
#include "../../include/osfm_hip.h"

namespace osfm {

constexpr int kAffineHyp = 2;          // hypotheses per thread and pass
constexpr int kAffineChunk = 1024;     // matches staged in LDS at a time

// scratch: affine_scratch_bytes(num_jobs) of device memory (best-of-part slots and the per-pair completion
// counters), 16-byte aligned.  The jobs are the RansacJob records of launch_ransac; count_out is -1 below 4 matches.
// results: one record per job, or null.
size_t affine_scratch_bytes(int num_jobs);
void launch_ransac_affine(const RansacJob *d_jobs, int num_jobs, int max_iterations, double threshold, int refit,
    uint64_t seed, void *scratch, osfm_ransac_affine_result *d_results, hipStream_t s);

}  // namespace osfm
