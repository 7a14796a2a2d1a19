// Placing one view against triangulated points: RANSAC over affine cameras (resect_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/osfm_hip.h"

namespace osfm {

constexpr int kResectSample = 4;        // points per hypothesis: four non-coplanar points fix an affine camera
constexpr int kResectTile = 256;        // points per scoring workgroup: the unit of the fixed-order sums
constexpr int kResectChunk = 16;        // hypotheses whose tables a scoring workgroup stages in LDS
constexpr int kResectMaxIterations = 1 << 20;

// opts with the defaults filled in and checked (OSFM_E_ARG otherwise); *iterations: the number of hypotheses
int resect_check_options(const osfm_resect_options *opts, osfm_resect_options *out, int *iterations);

// fewer correspondences than a sample and its support: OSFM_RESECT_TOO_FEW, nothing is launched
inline bool resect_too_few(int N, const osfm_resect_options &o) { return (int64_t)N < (int64_t)kResectSample + o.min_consensus; }

// points [N][3], xy [N][2] pixels (device) -> data [5][N]: rows X, Y, Z, u, v (u, v by tk_normalise)
void launch_resect_pack(const double *points, const double *xy, int N, int W, int H, double *data, hipStream_t s);

// The whole call on data [5][N] (device): eight launches on s and ONE read-back.  ev_a / ev_b: timing events around
// the scoring kernel.  Outputs are host pointers (inlier may be null; it is written for min(N, inlier_capacity)
// points).  The current device is the one data lives on.
int resect_core(const double *data, int N, int W, int H, const osfm_resect_options &o, int iterations, uint64_t stream_id,
    hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b, double *rotation, double *scale, double *offsets, uint8_t *inlier,
    int inlier_capacity, osfm_resect_result *result);

}  // namespace osfm
