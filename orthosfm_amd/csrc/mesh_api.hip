// C entries of the depth-map meshes (include/osfm_hip.h, "A mesh per depth map"): the upload of a depth map, the mesh
// of one view (mesh_kernels.hip), its download, and the PLY file of a mesh or a point set.
#include <cmath>
#include <cstring>
#include <fstream>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "dense_handle.h"
#include "mesh_kernels.h"

using namespace osfm;

namespace {

int check_mesh_view(const osfm_dense *d, int view, const char *api)
{
    if (view < 0 || view >= d->num_views) { set_error("%s: view %d of %d", api, view, d->num_views); return OSFM_E_RANGE; }
    return OSFM_OK;
}

}  // namespace

extern "C" {

int osfm_dense_set_map(osfm_dense *d, int view, const double *depth, const float *score, const uint8_t *status, double dz)
{
    if (!d || !depth || !status) { set_error("osfm_dense_set_map: null argument"); return OSFM_E_ARG; }
    OSFM_RETURN_IF(check_mesh_view(d, view, "osfm_dense_set_map"));
    if (!d->cameras) { set_error("osfm_dense_set_map: no cameras (osfm_dense_set_cameras)"); return OSFM_E_STATE; }
    if (!d->images[view].px) { set_error("osfm_dense_set_map: view %d has no image", view); return OSFM_E_STATE; }
    if (!std::isfinite(dz) || !(dz > 0.0)) { set_error("osfm_dense_set_map: dz %g: a finite value > 0 is expected", dz); return OSFM_E_ARG; }
    const size_t n = (size_t)d->images[view].w * d->images[view].h;
    for (size_t i = 0; i < n; ++i) {
        if (status[i] > OSFM_DENSE_RANGE_EDGE) {
            set_error("osfm_dense_set_map: pixel %zu has status %d: a status of the sweep (0..%d) is expected", i, (int)status[i], OSFM_DENSE_RANGE_EDGE);
            return OSFM_E_ARG;
        }
        if (status[i] == OSFM_DENSE_OK && !std::isfinite(depth[i])) {
            set_error("osfm_dense_set_map: pixel %zu is OK and its depth is not finite", i);
            return OSFM_E_ARG;
        }
    }
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    OSFM_HIP_CHECK(hipStreamSynchronize(d->stream));
    dense::drop_map(d, view);
    OSFM_RETURN_IF(d->depth[view].reserve(n * sizeof(double)));
    OSFM_RETURN_IF(d->score[view].reserve(n * sizeof(float)));
    OSFM_RETURN_IF(d->status[view].reserve(n));
    OSFM_RETURN_IF(d->final_status[view].reserve(n));
    OSFM_HIP_CHECK(hipMemcpy(d->depth[view].ptr, depth, n * sizeof(double), hipMemcpyHostToDevice));
    if (score) OSFM_HIP_CHECK(hipMemcpy(d->score[view].ptr, score, n * sizeof(float), hipMemcpyHostToDevice));
    else OSFM_HIP_CHECK(hipMemset(d->score[view].ptr, 0, n * sizeof(float)));
    OSFM_HIP_CHECK(hipMemcpy(d->status[view].ptr, status, n, hipMemcpyHostToDevice));
    OSFM_HIP_CHECK(hipDeviceSynchronize());
    d->swept[view] = 1;
    d->dz[view] = dz;
    return OSFM_OK;
}

int osfm_dense_mesh_options_default(osfm_dense_mesh_options *o)
{
    if (!o) { set_error("osfm_dense_mesh_options_default: null argument"); return OSFM_E_ARG; }
    o->dd_factor = 5.0;
    o->confidence_iterations = 3;
    o->min_island = 0;
    o->use_fused = 0;
    o->refined_normals = 0;
    return OSFM_OK;
}

int osfm_dense_mesh_limits(int32_t *label_tile_w, int32_t *label_tile_h, int32_t *max_confidence_iterations)
{
    if (label_tile_w) *label_tile_w = mesh::kLabelTileW;
    if (label_tile_h) *label_tile_h = mesh::kLabelTileH;
    if (max_confidence_iterations) *max_confidence_iterations = mesh::kMaxConfidenceIterations;
    return OSFM_OK;
}

int osfm_dense_mesh_view(osfm_dense *d, int view, const osfm_dense_mesh_options *opts, int64_t *num_vertices, int64_t *num_triangles,
    osfm_dense_mesh_stats *stats)
{
    if (!d) { set_error("osfm_dense_mesh_view: null argument"); return OSFM_E_ARG; }
    osfm_dense_mesh_options o;
    (void)osfm_dense_mesh_options_default(&o);
    if (opts) o = *opts;
    if (!std::isfinite(o.dd_factor) || o.dd_factor < 0.0 || o.confidence_iterations < 0 ||
        o.confidence_iterations > mesh::kMaxConfidenceIterations || o.min_island < 0) {
        set_error("osfm_dense_mesh_view: invalid options (dd_factor >= 0, confidence_iterations 0..%d, min_island >= 0)",
            mesh::kMaxConfidenceIterations);
        return OSFM_E_ARG;
    }
    OSFM_RETURN_IF(check_mesh_view(d, view, "osfm_dense_mesh_view"));
    if (!d->cameras || !d->swept[view]) { set_error("osfm_dense_mesh_view: view %d has no depth map", view); return OSFM_E_STATE; }
    if (o.use_fused && !d->fused) { set_error("osfm_dense_mesh_view: use_fused without a fusion (osfm_dense_fuse)"); return OSFM_E_STATE; }
    if (o.refined_normals && !d->refined[view]) {
        set_error("osfm_dense_mesh_view: refined_normals, and the map of view %d was not refined (osfm_dense_refine_view)", view);
        return OSFM_E_STATE;
    }

    OSFM_HIP_CHECK(hipSetDevice(d->device));
    mesh::View v;
    std::memset(&v, 0, sizeof(v));
    v.depth = d->depth[view].as<double>(); v.status = d->status[view].as<uint8_t>();
    v.final_status = o.use_fused ? d->final_status[view].as<uint8_t>() : nullptr;
    v.refine_status = o.refined_normals ? d->refine_status[view].as<uint8_t>() : nullptr;
    v.refine_normal = o.refined_normals ? d->refine_normal[view].as<double>() : nullptr;
    v.w = d->images[view].w; v.h = d->images[view].h;
    v.geo = d->geo[view];
    const size_t n = (size_t)v.w * v.h;                        // at most 2^28: the counts fit the scans' int32
    const bool label = o.min_island > 0;
    const double f = mesh::footprint(v.geo);
    const double thr = o.dd_factor * f, thr_diag = thr * std::sqrt(2.0);

    d->mesh_view = -1;
    OSFM_RETURN_IF(d->mesh_solid.reserve(n));
    if (label) {
        OSFM_RETURN_IF(d->mesh_parent.reserve(n * 4));
        OSFM_RETURN_IF(d->mesh_local.reserve(n * 4));
        OSFM_RETURN_IF(d->mesh_tile_size.reserve(n * 4));
        OSFM_RETURN_IF(d->mesh_size.reserve(n * 4));
    }
    OSFM_RETURN_IF(d->mesh_blocks.reserve(n));
    OSFM_RETURN_IF(d->mesh_tflags.reserve((n + 1) * 4));
    OSFM_RETURN_IF(d->mesh_tscan.reserve((n + 1) * 4));
    OSFM_RETURN_IF(d->mesh_vflags.reserve((n + 1) * 4));
    OSFM_RETURN_IF(d->mesh_vscan.reserve((n + 1) * 4));
    OSFM_RETURN_IF(d->mesh_class.reserve(n));
    OSFM_RETURN_IF(d->mesh_links.reserve(n));
    OSFM_RETURN_IF(d->mesh_dist[0].reserve(n));
    OSFM_RETURN_IF(d->mesh_dist[1].reserve(n));
    OSFM_RETURN_IF(d->mesh_counters.reserve(mesh::kCounterWords * sizeof(unsigned long long)));
    size_t temp = 0;
    OSFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, d->mesh_tflags.as<int32_t>(), d->mesh_tscan.as<int32_t>(), (int)(n + 1), nullptr));
    OSFM_RETURN_IF(d->mesh_scan_temp.reserve(temp));

    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    hipStream_t s = sg.s;
    hipEvent_t marks[OSFM_MESH_NUM_STAGES + 1] = {sg.ev[0].a, sg.ev[0].b, sg.ev[1].a, sg.ev[1].b, sg.ev[2].a, sg.ev[2].b};
    unsigned long long *counters = d->mesh_counters.as<unsigned long long>();
    uint8_t *solid = d->mesh_solid.as<uint8_t>();
    OSFM_HIP_CHECK(hipMemsetAsync(counters, 0, mesh::kCounterWords * sizeof(unsigned long long), s));
    OSFM_HIP_CHECK(hipMemsetAsync(d->mesh_tflags.as<int32_t>() + n, 0, 4, s));
    OSFM_HIP_CHECK(hipMemsetAsync(d->mesh_vflags.as<int32_t>() + n, 0, 4, s));
    OSFM_HIP_CHECK(hipEventRecord(marks[0], s));
    mesh::launch_solid(s, v, solid, counters);
    if (label)
        mesh::launch_label(s, v.w, v.h, o.min_island, solid, d->mesh_parent.as<int32_t>(), d->mesh_local.as<int32_t>(),
            d->mesh_tile_size.as<int32_t>(), d->mesh_size.as<int32_t>(), counters);
    OSFM_HIP_CHECK(hipEventRecord(marks[1], s));
    mesh::launch_blocks(s, v, solid, thr, thr_diag, d->mesh_blocks.as<uint8_t>(), d->mesh_tflags.as<int32_t>(), counters);
    OSFM_HIP_CHECK(hipEventRecord(marks[2], s));
    mesh::launch_vertices(s, v.w, v.h, d->mesh_blocks.as<uint8_t>(), d->mesh_vflags.as<int32_t>(), d->mesh_class.as<uint8_t>(),
        d->mesh_links.as<uint8_t>(), d->mesh_dist[0].as<uint8_t>(), counters);
    OSFM_HIP_CHECK(hipEventRecord(marks[3], s));
    // a vertex at distance k < K has it after k rounds; min(distance, K) needs no more than K - 1
    int cur = 0;
    for (int k = 1; k < o.confidence_iterations; ++k, cur ^= 1)
        mesh::launch_distance_round(s, v.w, v.h, d->mesh_links.as<uint8_t>(), d->mesh_dist[cur].as<uint8_t>(), d->mesh_dist[cur ^ 1].as<uint8_t>());
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(marks[4], s));
    size_t have = d->mesh_scan_temp.bytes;
    OSFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d->mesh_scan_temp.ptr, have, d->mesh_tflags.as<int32_t>(), d->mesh_tscan.as<int32_t>(), (int)(n + 1), s));
    have = d->mesh_scan_temp.bytes;
    OSFM_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d->mesh_scan_temp.ptr, have, d->mesh_vflags.as<int32_t>(), d->mesh_vscan.as<int32_t>(), (int)(n + 1), s));
    int32_t T = 0, V = 0;
    unsigned long long h_slots[mesh::kCounterWords], h_counters[mesh::kNumCounters] = {};
    OSFM_HIP_CHECK(hipMemcpyAsync(&T, d->mesh_tscan.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(&V, d->mesh_vscan.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipMemcpyAsync(h_slots, counters, sizeof(h_slots), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    for (int slot = 0; slot < mesh::kCounterSlots; ++slot)
        for (int k = 0; k < mesh::kNumCounters; ++k) h_counters[k] += h_slots[(size_t)slot * mesh::kSlotStride + k];
    if (h_counters[mesh::kError]) {
        set_error("osfm_dense_mesh_view: the component labelling ran into its bound of %d steps", mesh::kMaxHops);
        return OSFM_E_NUMERIC;
    }
    OSFM_RETURN_IF(d->mesh_points.reserve((size_t)V * 24 + 8));
    OSFM_RETURN_IF(d->mesh_normals.reserve((size_t)V * 24 + 8));
    OSFM_RETURN_IF(d->mesh_scale.reserve((size_t)V * 8 + 8));
    OSFM_RETURN_IF(d->mesh_confidence.reserve((size_t)V * 4 + 8));
    OSFM_RETURN_IF(d->mesh_pixel.reserve((size_t)V * 8 + 8));
    OSFM_RETURN_IF(d->mesh_vclass.reserve((size_t)V + 8));
    OSFM_RETURN_IF(d->mesh_tris.reserve((size_t)T * 12 + 8));
    const mesh::Mesh out{d->mesh_points.as<double>(), d->mesh_normals.as<double>(), d->mesh_scale.as<double>(), d->mesh_confidence.as<float>(),
        d->mesh_pixel.as<int32_t>(), d->mesh_vclass.as<uint8_t>(), d->mesh_tris.as<int32_t>()};
    mesh::launch_emit(s, v, d->mesh_blocks.as<uint8_t>(), d->mesh_vflags.as<int32_t>(), d->mesh_vscan.as<int32_t>(), d->mesh_tscan.as<int32_t>(),
        d->mesh_class.as<uint8_t>(), d->mesh_dist[cur].as<uint8_t>(), o.confidence_iterations, out);
    OSFM_HIP_CHECK(hipGetLastError());
    OSFM_HIP_CHECK(hipEventRecord(marks[5], s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    d->mesh_view = view;
    d->mesh_vertices = V;
    d->mesh_triangles = T;
    if (num_vertices) *num_vertices = V;
    if (num_triangles) *num_triangles = T;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels_solid = (int64_t)h_counters[mesh::kSolid];
        stats->pixels_island = (int64_t)h_counters[mesh::kIslandPixels];
        stats->components = (int64_t)h_counters[mesh::kComponents];
        stats->triangles_dropped = (int64_t)h_counters[mesh::kDropped];
        stats->vertices_simple = (int64_t)h_counters[mesh::kSimple];
        stats->vertices_border = (int64_t)h_counters[mesh::kBorder];
        stats->vertices_complex = (int64_t)h_counters[mesh::kComplex];
        stats->threshold_steps = thr / d->dz[view];
        for (int k = 0; k < OSFM_MESH_NUM_STAGES; ++k) {
            float ms = 0.0f;
            OSFM_HIP_CHECK(hipEventElapsedTime(&ms, marks[k], marks[k + 1]));
            stats->stage_ms[k] = ms;
        }
        float ms = 0.0f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, marks[0], marks[OSFM_MESH_NUM_STAGES]));
        stats->device_ms = ms;
    }
    return OSFM_OK;
}

int osfm_dense_download_mesh(osfm_dense *d, int64_t capacity_vertices, int64_t capacity_triangles, double *points, double *normals,
    float *confidence, double *scale, int32_t *pixel, uint8_t *vclass, int32_t *triangles)
{
    if (!d) { set_error("osfm_dense_download_mesh: null argument"); return OSFM_E_ARG; }
    if (d->mesh_view < 0) { set_error("osfm_dense_download_mesh: no mesh (osfm_dense_mesh_view)"); return OSFM_E_STATE; }
    if (capacity_vertices < d->mesh_vertices || capacity_triangles < d->mesh_triangles) {
        set_error("osfm_dense_download_mesh: capacity %lld vertices, %lld triangles; the mesh has %lld and %lld", (long long)capacity_vertices,
            (long long)capacity_triangles, (long long)d->mesh_vertices, (long long)d->mesh_triangles);
        return OSFM_E_CAPACITY;
    }
    OSFM_HIP_CHECK(hipSetDevice(d->device));
    const size_t V = (size_t)d->mesh_vertices, T = (size_t)d->mesh_triangles;
    if (V > 0) {
        if (points) OSFM_HIP_CHECK(hipMemcpy(points, d->mesh_points.ptr, V * 24, hipMemcpyDeviceToHost));
        if (normals) OSFM_HIP_CHECK(hipMemcpy(normals, d->mesh_normals.ptr, V * 24, hipMemcpyDeviceToHost));
        if (confidence) OSFM_HIP_CHECK(hipMemcpy(confidence, d->mesh_confidence.ptr, V * 4, hipMemcpyDeviceToHost));
        if (scale) OSFM_HIP_CHECK(hipMemcpy(scale, d->mesh_scale.ptr, V * 8, hipMemcpyDeviceToHost));
        if (pixel) OSFM_HIP_CHECK(hipMemcpy(pixel, d->mesh_pixel.ptr, V * 8, hipMemcpyDeviceToHost));
        if (vclass) OSFM_HIP_CHECK(hipMemcpy(vclass, d->mesh_vclass.ptr, V, hipMemcpyDeviceToHost));
    }
    if (T > 0 && triangles) OSFM_HIP_CHECK(hipMemcpy(triangles, d->mesh_tris.ptr, T * 12, hipMemcpyDeviceToHost));
    return OSFM_OK;
}

int osfm_dense_mesh_write(const char *path, int64_t V, const double *points, const double *normals, const uint8_t *rgb,
    const float *confidence, const double *scale, int64_t T, const int32_t *triangles)
{
    if (!path || V < 0 || T < 0 || (V > 0 && !points) || (T > 0 && !triangles)) {
        set_error("osfm_dense_mesh_write: null argument / negative count");
        return OSFM_E_ARG;
    }
    for (int64_t i = 0; i < 3 * T; ++i)
        if (triangles[i] < 0 || triangles[i] >= V) { set_error("osfm_dense_mesh_write: triangle %lld names vertex %d of %lld", (long long)(i / 3), triangles[i], (long long)V); return OSFM_E_RANGE; }
    std::ofstream f(path, std::ios::out | std::ios::trunc | std::ios::binary);
    if (!f) { set_error("osfm_dense_mesh_write: cannot open %s", path); return OSFM_E_IO; }
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << (long long)V << "\n"
      << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
      << "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float confidence\nproperty float value\n";
    if (T > 0) f << "element face " << (long long)T << "\nproperty list uchar int vertex_indices\n";
    f << "end_header\n";
    constexpr size_t kRow = 35, kFace = 13;
    std::vector<char> rows((size_t)V * kRow);
    for (int64_t i = 0; i < V; ++i) {
        char *row = rows.data() + kRow * (size_t)i;
        float v[6] = {(float)points[3 * i], (float)points[3 * i + 1], (float)points[3 * i + 2], 0.0f, 0.0f, 0.0f};
        if (normals)
            for (int c = 0; c < 3; ++c) v[3 + c] = (float)normals[3 * i + c];
        std::memcpy(row, v, 24);                            // the hosts this library runs on are little-endian
        for (int c = 0; c < 3; ++c) row[24 + c] = rgb ? (char)rgb[3 * i + c] : 0;
        const float cs[2] = {confidence ? confidence[i] : 1.0f, scale ? (float)scale[i] : 0.0f};
        std::memcpy(row + 27, cs, 8);
    }
    f.write(rows.data(), (std::streamsize)rows.size());
    std::vector<char> faces((size_t)T * kFace);
    for (int64_t i = 0; i < T; ++i) {
        char *row = faces.data() + kFace * (size_t)i;
        row[0] = 3;
        std::memcpy(row + 1, triangles + 3 * i, 12);
    }
    f.write(faces.data(), (std::streamsize)faces.size());
    f.close();
    if (!f) { set_error("osfm_dense_mesh_write: write to %s failed", path); return OSFM_E_IO; }
    return OSFM_OK;
}

}  // extern "C"
