// Dense depth maps by orthographic plane sweep and their fusion (DESIGN.md "Dense plane sweep").
// tests/dense_restatement.py is the definition in numpy; this header holds what the kernels (dense_kernels.hip) and
// the C entries (dense_api.hip) share.
#pragma once
#include "osfm_common.h"

namespace osfm {
namespace dense {

constexpr int kTileW = 32, kTileH = 16;                        // reference pixels a workgroup owns: two per thread
constexpr int kThreads = 256;
constexpr int kMaxRadius = 7;
constexpr int kMaxSources = 8;
constexpr int kMaxDepths = 256;
constexpr int kHaloW = kTileW + 2 * kMaxRadius, kHaloH = kTileH + 2 * kMaxRadius;      // 46 x 30
constexpr int kHalo = kHaloW * kHaloH;                          // 1380 texels
constexpr int kSlots = (kHalo + kThreads - 1) / kThreads;       // halo texels a thread warps: 6

// The geometry of a view, made on the host in double in the order of tests/dense_restatement.py (Geometry):
// pixel = A X + t, viewing axis d, B = A^T (A A^T)^-1.
struct ViewGeo {
    double A[2][3], t[2], d[3], B[3][2];
};
// false: P has a value that is not finite, or A has no rank 2
bool make_geo(const double *P, ViewGeo *g);

// a source as the sweep kernel sees it: where reference pixel x at depth z falls, G x + g + z e
struct Source {
    const float *px;
    int32_t w, h;
    double G[2][2], g[2], e[2];
};
void make_source(const ViewGeo &ref, const ViewGeo &src, Source *s);

struct SweepArgs {
    const float *ref;             // float32 [h][w], the refiner's grey image
    int32_t w, h;
    int32_t num_sources, num_depths, radius, min_sources;
    double z_min, dz;
    float min_var, min_score;     // (2 radius + 1)^2 min_contrast^2
    double *depth;                // [h][w], NaN where the status is not OSFM_DENSE_OK
    float *score;                 // [h][w], 0 there
    uint8_t *status;              // [h][w]
    Source src[kMaxSources];
};
void launch_sweep(hipStream_t s, const SweepArgs &a);

// What osfm_dense_debug_ablation leaves out of the sweeps that follow: the texel gather (a sample made of the
// position instead), the double arithmetic of the positions (float32 instead), all taps of the box sums but one.
enum { kAblateNone = 0, kAblateGather = 1, kAblateDouble = 2, kAblateBoxSums = 3 };
int set_ablation(int mode);       // returns the mode before

// a view as the fusion sees it
struct FuseView {
    const double *depth;
    const uint8_t *status;
    uint8_t *final_status;
    int32_t w, h, swept, reserved;
    int64_t offset;               // of its first pixel in the flags of all swept views
    double dz;
    ViewGeo geo;
};
struct Cloud {
    double *points;               // [N][3]
    int32_t *view, *pixel;        // [N], [N][2] (x, y)
};
// final_status and flags[offset + i] (1: the pixel's point is emitted) of view r
void launch_consistency(hipStream_t s, const FuseView *views, int num_views, int r, int64_t pixels, double tol, int min_consistent,
    int32_t *flags);
// scan: the exclusive sum of flags
void launch_emit(hipStream_t s, const FuseView *views, int r, int64_t pixels, const int32_t *flags, const int32_t *scan, Cloud cloud);

}  // namespace dense
}  // namespace osfm
