// Slanted-plane refinement of a depth map (DESIGN.md "Slanted-plane refinement").  tests/dense_refine_restatement.py is
// the definition in numpy; this header holds what the kernel (dense_refine_kernels.hip) and the C entries
// (dense_refine_api.hip) share.
#pragma once
#include "dense_kernels.h"

namespace osfm {
namespace dense {

constexpr int kRefineLanes = 16;                               // lanes that own a pixel: four pixels a wave
constexpr int kRefineBlock = 4;                                // a workgroup owns kRefineBlock x kRefineBlock pixels, a wave one row of them
constexpr int kRefineThreads = kRefineLanes * kRefineBlock * kRefineBlock;
constexpr int kRefineMaxIterations = 100;
constexpr int kRefineCounterSlots = 64, kRefineSlotStride = 8;      // per slot: iterations, source passes
constexpr double kRefineBlockEps = 1e-12;                      // BLOCK_EPS of the restatement

struct RefineArgs {
    const float *ref;             // float32 [h][w]
    int32_t w, h;
    int32_t num_sources, radius, min_sources, max_iterations;
    double dz, converged, max_shift, max_deform, min_score, min_pivot;      // converged: eps dz
    double B[3][2], d[3];         // of the view's ViewGeo
    const uint8_t *status;        // [h][w], the sweep's
    double *depth;                // [h][w]: REFINED pixels take the new depth
    float *score;                 // [h][w]: and the new score
    uint8_t *rstatus;             // [h][w]
    double *gradient, *normal;    // [h][w][2], [h][w][3]: NaN where the pixel is not REFINED
    unsigned long long *counters; // [kRefineCounterSlots][kRefineSlotStride], zeroed
    Source src[kMaxSources];
};
void launch_refine(hipStream_t s, const RefineArgs &a);

}  // namespace dense
}  // namespace osfm
