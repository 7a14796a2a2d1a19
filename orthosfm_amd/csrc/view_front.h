// What the matcher's hand-off (match_views.hip) sees of a view front end (view_api.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/osfm_hip.h"

namespace osfm {

// The last load on the front end's device.  Row i of the view's SIFT part is row sift_map[i] of sift_desc, and
// likewise for SURF; normalized holds the SIFT rows, then the SURF rows.
struct FrontResult {
    int device = 0;
    const float *sift_desc = nullptr, *surf_desc = nullptr, *normalized = nullptr;
    const int32_t *sift_map = nullptr, *surf_map = nullptr;
    int n_sift = 0, n_surf = 0;
};

// OSFM_E_STATE without a load.
int view_front_result(osfm_view_front *front, FrontResult *out);
// Brackets of a reader of those arrays on `reader`, a stream of any device: begin makes it wait for the load (and
// for an earlier reader that has not finished), end records what the front end's next load waits for.
int view_front_begin_read(osfm_view_front *front, hipStream_t reader);
int view_front_end_read(osfm_view_front *front, hipStream_t reader);

// The feature image of the last load (what osfm_view_front_debug_image copies out), for a reader inside the same
// brackets: 8-bit, row-major, `channels` interleaved.  OSFM_E_STATE without a load.
struct FrontImage {
    int device = 0;
    const uint8_t *pixels = nullptr;
    int width = 0, height = 0, channels = 0;
};
int view_front_image(osfm_view_front *front, FrontImage *out);

}  // namespace osfm
