// A mesh per depth map (DESIGN.md "Depth-map meshes"): islands, triangles, vertex classes, normals, scales and
// confidences on the image grid of an orthographic view.  tests/mesh_restatement.py is the definition in numpy, on
// general vertex and face lists; this header holds what the kernels (mesh_kernels.hip) and the C entries
// (mesh_api.hip) share.
#pragma once
#include "dense_kernels.h"

namespace osfm {
namespace mesh {

constexpr int kLabelTileW = 32, kLabelTileH = 16;               // pixels a workgroup labels in LDS: one per thread
constexpr int kLabelThreads = kLabelTileW * kLabelTileH;
constexpr int kMaxConfidenceIterations = 16;
// Steps a walk towards a root, and retries of a union, may take.  Parents only ever decrease, so every walk ends; the
// bound turns a defect into an error code (kError) instead of a hang.  A chain is as long as the tile-local roots it
// threads, far below this.
constexpr int kMaxHops = 1 << 16;

// Counters of one call, uint64 on the device: kCounterSlots sets of them, kSlotStride words (a cache line) apart;
// a workgroup counts into the set of its index, the sum over the sets is the count.
enum { kSolid = 0, kIslandPixels, kComponents, kDropped, kSimple, kBorder, kComplex, kError, kNumCounters };
constexpr int kCounterSlots = 64, kSlotStride = 16;
constexpr size_t kCounterWords = (size_t)kCounterSlots * kSlotStride;

struct View {
    const double *depth;          // [h][w]
    const uint8_t *status;        // the sweep's
    const uint8_t *final_status;  // the fusion's, or null
    const uint8_t *refine_status; // of the slanted-plane refinement, or null: its REFINED pixels take refine_normal [h][w][3]
    const double *refine_normal;
    int32_t w, h;
    dense::ViewGeo geo;
};

// solid[i] = 1: sweep status OK, and with a final status that one OK or DUPLICATE
void launch_solid(hipStream_t s, const View &v, uint8_t *solid, unsigned long long *counters);

// Component labelling of the solid pixels, four launches: the kernel boundaries publish one phase to the next.
//   tile:  union-find in LDS over a kLabelTileW x kLabelTileH tile; local[i] = parent[i] = the tile-local root of
//          pixel i (a pixel index; -1 where not solid), tile_size[root] = its pixels
//   seam:  unions across the tile seams on parent[], through agent-scope atomics only
//   root:  every tile-local root finds its root, adds its pixels to size[root] and leaves the root in local[]
//   clear: a pixel whose component has fewer than min_island pixels stops being solid
void launch_label(hipStream_t s, int w, int h, int min_island, uint8_t *solid, int32_t *parent, int32_t *local, int32_t *tile_size,
    int32_t *size, unsigned long long *counters);

// blocks[i]: bits 0..3 say which of T1..T4 the 2 x 2 block with its first pixel at i emits (0 in the last column and
// row); tflags[i]: how many
void launch_blocks(hipStream_t s, const View &v, const uint8_t *solid, double thr, double thr_diag, uint8_t *blocks, int32_t *tflags,
    unsigned long long *counters);

// Per pixel, from the four blocks around it: vflags[i] (a triangle names it), cls[i] (OSFM_MESH_VERTEX_*), links[i]
// (bit k: a mesh edge to the k-th of its 8 neighbours, row-major), dist[i] (0 on a BORDER vertex, else 255)
void launch_vertices(hipStream_t s, int w, int h, const uint8_t *blocks, int32_t *vflags, uint8_t *cls, uint8_t *links, uint8_t *dist,
    unsigned long long *counters);

// one round of the distance to the border: out[i] = min(in[i], 1 + in[n] over the linked n)
void launch_distance_round(hipStream_t s, int w, int h, const uint8_t *links, const uint8_t *in, uint8_t *out);

struct Mesh {
    double *points, *normals, *scale;     // [V][3], [V][3], [V]
    float *confidence;                    // [V]
    int32_t *pixel;                       // [V][2]
    uint8_t *vclass;                      // [V]
    int32_t *triangles;                   // [T][3]
};
// vscan, tscan: the exclusive sums of vflags and tflags
void launch_emit(hipStream_t s, const View &v, const uint8_t *blocks, const int32_t *vflags, const int32_t *vscan, const int32_t *tscan,
    const uint8_t *cls, const uint8_t *dist, int iterations, Mesh mesh);

// sqrt(|b0 x b1|) of the columns of B, in the restatement's order
double footprint(const dense::ViewGeo &g);

}  // namespace mesh
}  // namespace osfm
