// Guided matching inside the affine epipolar band of verified pairs (osfm_match_guided): device records and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/osfm_hip.h"

namespace osfm {

constexpr int kGuidedQueries = 16;     // queries per workgroup: four per wave, one after the other
constexpr int kGuidedChunk = 2048;     // band scalars of the other view staged in LDS at a time (16 KB)
constexpr int kGuidedPass = 64;        // candidates a query collects before the wave scores them, one per lane

// One pair of a call.  u1 / u2 / m12 / m21 / list are the pair's own pieces of the matcher's scratch.
struct GuidedJob {
    const float *pos1, *pos2;                      // [n][2] normalised positions of view_1 / view_2
    const int8_t *sift1, *sift2, *surf1, *surf2;   // the bank's rows: SIFT value - 128, SURF value
    const int32_t *seeds;                          // (feature_1, feature_2) pairs, validated on the host
    double *u1, *u2;                               // band scalars: (x1 c + y1 d) + e per feature of view_1, x2 a + y2 b of view_2; NaN: in a seed
    int32_t *m12, *m21;                            // one-way results in combined indices, -1: none
    int32_t *list;                                 // the pair's correspondences, at most min(n1, n2)
    int32_t ns1, nu1, ns2, nu2;
    int32_t num_seeds, has_F;
    int32_t block_start, block_end;                // the pair's workgroups in the matching launch
    double F[5];                                   // (a, b, c, d, e) when has_F
};

// What the preparation leaves for the kernels behind it and for the host.
struct GuidedPrep {
    double v[5], s, s_lo, s_hi, thr2;
    int32_t cap[2];                                // per type: largest dist_1st a result may have
    int32_t status, count, max_candidates, pad;
};

void launch_guided_prepare(const GuidedJob *d_jobs, int num_jobs, GuidedPrep *d_prep, double threshold, int cap_from_seeds, hipStream_t s);
void launch_guided_match(const GuidedJob *d_jobs, int num_jobs, int total_blocks, GuidedPrep *d_prep, float sq_sift, float sq_surf, hipStream_t s);
void launch_guided_finish(const GuidedJob *d_jobs, int num_jobs, GuidedPrep *d_prep, hipStream_t s);
void launch_guided_gather(const GuidedJob *d_jobs, int num_jobs, const GuidedPrep *d_prep, const int64_t *d_dst_off, int32_t *d_out, hipStream_t s);

}  // namespace osfm
