// Kernels of the view front end (view_kernels.hip): the halving chain of bundler::Features::compute on byte
// images, FeatureSet's colours and normalised positions read from the device image, and the hand-off that turns
// a detector's float descriptors into the matcher's bank without leaving the device.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace osfm {
namespace view {

// mve::image::rescale_half_size<uint8_t>: dst is ((w + 1) >> 1) x ((h + 1) >> 1) x c; w, h >= 2.
void launch_halve(hipStream_t s, const uint8_t *src, int w, int h, int c, uint8_t *dst);

// feature_view_row (feature_view.h) per feature: positions [n][2] in pixels of img; colors [n][3], normalized [n][2].
void launch_view_rows(hipStream_t s, const uint8_t *img, int w, int h, int c, const float *positions, int n, uint8_t *colors,
    float *normalized);

// view_mark_row (feature_view.h) per row of normalized [n][2]: pixel_xy [n][2], pixel_rgb [n][3], mark [n].  img is
// the import image, mask [mask_h][mask_w] or NULL.  counts[0..2] (zeroed by the caller) take the masked-out rows
// among the first n_sift, among the rest, and the rows outside the mask: integer sums, the same on every run.
void launch_view_marks(hipStream_t s, const float *normalized, int n, int n_sift, double pixel_width, const uint8_t *img, int w,
    int h, int c, const uint8_t *mask, int mask_w, int mask_h, int clamp, int threshold, float *pixel_xy, uint8_t *pixel_rgb,
    uint8_t *mark, int32_t *counts);

// The rows of a view whose mark carries kMarkIn, moved to the front of a second set of arrays: the first n_sift rows
// among themselves, then the others, each in their order.  One workgroup that walks the rows in passes of
// kCompactPassRows and numbers the kept ones from a running sum: the same result on every run.
struct ViewRows {
    int32_t *sift_map, *surf_map;           // [n_sift], [n_surf]
    float *positions, *normalized, *pixel_xy;       // [n][2]
    uint8_t *colors, *pixel_rgb, *mark;     // [n][3], [n][3], [n]
};
constexpr int kCompactPassRows = 1024;
// index [kept]: the row of `from` that each row of `to` was; counts[0..1]: kept among the first n_sift, among the rest.
void launch_compact_rows(hipStream_t s, const ViewRows &from, int n_sift, int n_surf, const ViewRows &to, int32_t *index,
    int32_t *counts);

// osfm_quantize_sift + prepare_sift_kernel (match_kernels.hip) in one pass: view row i is row map[i] of desc (map
// NULL: row i).  flag[i] (i < n) is 1 where the row holds a value above 127, else 0.
void launch_handoff_sift(hipStream_t s, const float *desc, const int32_t *map, int n, int npad, int8_t *dst, int32_t *corr,
    int8_t *dst_raw, int32_t *corr_raw, int32_t *flag);

// flag[0..n) in place into the slot of every row among the special rows (-1: none), their ascending list in
// special_map, their number in *count.  One workgroup, the same result on every run.
void launch_special_scan(hipStream_t s, int32_t *flag_to_slot, int n, int32_t *special_map, int32_t *count);

// osfm_quantize_surf + prepare_surf_kernel in one pass; *norm2max (zeroed by the caller) takes the largest
// squared norm of the quantised rows.
void launch_handoff_surf(hipStream_t s, const float *desc, const int32_t *map, int n, int npad, int8_t *dst, int32_t *corr,
    int32_t *norm2max);

}  // namespace view
}  // namespace osfm
