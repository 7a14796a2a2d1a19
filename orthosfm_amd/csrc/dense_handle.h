// The handle behind osfm_dense, shared by the entries of the sweep and the fusion (dense_api.hip), those of the
// slanted-plane refinement (dense_refine_api.hip) and those of the depth-map meshes (mesh_api.hip).
#pragma once
#include <vector>

#include "dense_kernels.h"
#include "refine_kernels.h"

struct osfm_dense {
    int device = 0, num_views = 0;
    hipStream_t stream = nullptr;                  // image uploads and conversions
    std::vector<osfm::DeviceBuffer> grey;          // float32 [h][w] per view
    std::vector<osfm::refine::Image> images;
    std::vector<osfm::DeviceBuffer> depth, score, status, final_status;      // per swept view
    // of osfm_dense_refine_view (dense_refine_api.hip), per refined view: status [h][w], gradient [h][w][2], normal [h][w][3]
    std::vector<osfm::DeviceBuffer> refine_status, refine_gradient, refine_normal;
    std::vector<uint8_t> refined;
    osfm::DeviceBuffer refine_counters;
    std::vector<osfm::dense::ViewGeo> geo;
    std::vector<uint8_t> swept;
    std::vector<double> dz;
    bool cameras = false, fused = false;
    int64_t cloud_size = 0;
    osfm::DeviceBuffer staging, table, flags, scan, scan_temp, cloud_points, cloud_view, cloud_pixel;
    // the mesh of the last osfm_dense_mesh_view (mesh_api.hip): mesh_view < 0 without one
    int mesh_view = -1;
    int64_t mesh_vertices = 0, mesh_triangles = 0;
    osfm::DeviceBuffer mesh_solid, mesh_parent, mesh_local, mesh_tile_size, mesh_size, mesh_blocks, mesh_tflags, mesh_tscan,
        mesh_vflags, mesh_vscan, mesh_class, mesh_links, mesh_dist[2], mesh_counters, mesh_scan_temp, mesh_points, mesh_normals,
        mesh_confidence, mesh_scale, mesh_pixel, mesh_vclass, mesh_tris;
    ~osfm_dense() { osfm::stream_destroy(stream); }
};

namespace osfm {
namespace dense {

// a new image, new cameras or a new map: what was made of the old ones is gone
inline void drop_map(osfm_dense *d, int view)
{
    d->swept[view] = 0;
    d->refined[view] = 0;
    d->fused = false;
    if (d->mesh_view == view) d->mesh_view = -1;
}

}  // namespace dense
}  // namespace osfm
