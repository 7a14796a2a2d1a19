// Internal entries of the SIFT and SURF contexts for the view front end (view_api.hip): extraction from a byte
// image that is already on the context's device, and where the result lies there.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/osfm_hip.h"

namespace osfm {

struct DetectorContext;

// osfm_sift_extract / osfm_surf_extract on d_pixels (width x height x channels bytes on the context's device),
// which the context's stream reads once `image_ready` has happened.  Same errors; colours and normalised
// positions are not computed (the front end's kernel does that from the device image).
int sift_extract_device(osfm_sift *ctx, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height, int channels,
    osfm_sift_summary *summary);
int surf_extract_device(osfm_surf *ctx, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height, int channels,
    osfm_surf_summary *summary);
// The context's shared part (detector_context.h), where the last extraction lies: desc and n_desc on the device, the
// per-row arrays in generation order on the host.
const DetectorContext *detector_of(const osfm_sift *ctx);
const DetectorContext *detector_of(const osfm_surf *ctx);

}  // namespace osfm
