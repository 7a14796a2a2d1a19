// Initial alignment of a camera group: RANSAC over Tomasi-Kanade factorisations (tk_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/osfm_hip.h"

namespace osfm {

constexpr int kTkMinCameras = 3, kTkMaxCameras = 8;
constexpr int kTkMinSample = 4, kTkMaxSample = 32;
constexpr int kTkTile = 256;        // tracks per scoring workgroup: the unit of the fixed-order error sums
constexpr int kTkChunk = 16;        // hypotheses whose tables a scoring workgroup stages in LDS

// Row of the measurement matrix from a pixel coordinate: the value getPointOnCameraPlane uses.  One function for
// the per-call form and the scene's gather, so that both hand the core the same bits.
__host__ __device__ __forceinline__ double tk_normalise(double px, int size)
{
    return -2.0 * (px / (double)size - 0.5);
}

// opts with the defaults filled in and checked (OSFM_E_ARG otherwise); *iterations: the number of hypotheses
int tk_check_options(const osfm_tk_options *opts, int num_cameras, osfm_tk_options *out, int *iterations);

// xy [N][C][2] pixels (device) -> rows [2C][N]: the x rows of the cameras, then their y rows
void launch_tk_rows(const double *xy, int N, int C, int W, int H, double *rows, hipStream_t s);

// The whole call on rows [2C][N] (device, normalised coordinates): a handful of launches on s and ONE read-back.
// ev_a / ev_b: timing events around the scoring kernel.  Outputs are host pointers (offsets / inlier may be null;
// inlier is written for min(N, inlier_capacity) tracks).  The current device is the one rows lives on.
int tk_align_core(const double *rows, int N, int C, int W, int H, const osfm_tk_options &o, int iterations, uint64_t group_id,
    hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b, double *basis_1, double *basis_2, double *offsets, uint8_t *inlier,
    int inlier_capacity, osfm_tk_result *result);

}  // namespace osfm
