// The covariance computation on a finished DeviceProblem (ba_cov_api.hip): what osfm_ba_covariance (host arrays in)
// and osfm_scene_covariance (the device-resident scene's selection) both run, so the two agree to the bit.
#pragma once
#include <vector>

#include "ba_solve.h"

namespace osfm {

// The gauge rule of osfm_ba_cov_options::depth_gauge (osfm_hip.h) on the host's copy of the cameras: *camera / *axis
// = -1 when no camera is all constant or none has both offsets free.  cam_const: [C][7].
void cov_choose_gauge(int model, int C, const double *cams, const uint8_t *cam_const, int32_t *camera, int32_t *axis);
// cam_const with the gauge column held (the byte of the chosen offset set)
std::vector<uint8_t> cov_held_masks(int model, int C, const uint8_t *cam_const, int camera, int axis);

// what the core brings back to the host (the arrays the caller did not ask for stay empty)
struct CovHost {
    std::vector<double> cam_cov, full, point_cov;
    std::vector<uint8_t> valid;
};

// D: the problem under the layout with the gauge column held (D.dev.nc, cam_ldim, cam_off), pdim = 3 optimize_points.
// Fills the scalar fields of *res (cost .. total_ms but the gauge's); OSFM_E_NUMERIC with rank_deficient = 1 and nothing in
// *out when S fails the pivot test.  Returns synchronised.
int ba_cov_core(const DeviceProblem &D, const osfm_ba_cov_options &o, StreamLease &sg, bool want_blocks, bool want_full,
    bool want_points, osfm_ba_cov_result *res, CovHost *out);

}  // namespace osfm
