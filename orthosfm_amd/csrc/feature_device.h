// Internal entries of the SIFT and SURF contexts for the view front end (view_api.hip): extraction from a byte
// image that is already on the context's device, and where the result lies there.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "../../include/osfm_hip.h"

namespace osfm {

// The last extraction of a context as the hand-off reads it.  Everything is in generation order; row i of
// FeatureSet's view is generation row order[i], whose descriptor is row (rows ? rows[order[i]] : order[i]) of desc.
struct DeviceFeatures {
    const float *desc = nullptr;                    // device: [.][128] (SIFT) or [.][64] (SURF)
    int n = 0;
    const std::vector<float> *positions = nullptr, *scale = nullptr, *orientation = nullptr;
    const std::vector<int32_t> *order = nullptr, *rows = nullptr;
};

// osfm_sift_extract / osfm_surf_extract on d_pixels (width x height x channels bytes on the context's device),
// which the context's stream reads once `image_ready` has happened.  Same errors; colours and normalised
// positions are not computed (the front end's kernel does that from the device image).
int sift_extract_device(osfm_sift *ctx, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height, int channels,
    osfm_sift_summary *summary);
int surf_extract_device(osfm_surf *ctx, const uint8_t *d_pixels, hipEvent_t image_ready, int width, int height, int channels,
    osfm_surf_summary *summary);
int sift_device_features(osfm_sift *ctx, DeviceFeatures *out);
int surf_device_features(osfm_surf *ctx, DeviceFeatures *out);

}  // namespace osfm
