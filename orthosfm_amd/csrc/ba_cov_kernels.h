// Kernels of the covariance entry (osfm_ba_covariance, ba_cov_api.hip): the inverse of the reduced camera system from
// its Cholesky factor on the f64 matrix cores, and the fold of that inverse into the points' covariances.  None of
// them waits on another workgroup; every sum has a fixed order, so a call repeats to the bit.
#pragma once
#include "ba_kernels.h"

namespace osfm {

// valid[j] = 1: the track has at least two observations, |w| >= 1e-12 |x|, and the pivots of V_j = sum Jp^T Jp (from
// the point pass's records) are at least min_ratio of V_j's diagonal
void launch_cov_point_valid(const BaDev &d, const double *obsrec, double min_ratio, uint8_t *valid, hipStream_t s);
// dst[k] = src[map[k]] for the kept observations' positions and cameras
void launch_cov_gather_obs(int n, const int32_t *map, const double *xy_in, const int32_t *cam_in, double *xy_out, int32_t *cam_out,
    hipStream_t s);
// sdiag[i] = S[i][i], i < N: S's own diagonal, before the factorisation consumes it
void launch_cov_save_diagonal(const double *S, int N, double *sdiag, hipStream_t s);
// out[0] = min_{i < n} L_ii^2 / sdiag[i] (1 for n == 0; 0 where a pivot is not a positive number), L_ii = 1 / inv(L_kk)_ii
// from the inverses the factorisation leaves in Ldiag.  One workgroup.
void launch_cov_pivot_ratio(const double *Ldiag, const double *sdiag, int n, double *out, hipStream_t s);
// Z = L^-1 (N x N, lower block triangle; the blocks above the diagonal are not written): a workgroup per block
// column, forward substitution down the column with the diagonal blocks' inverses of Ldiag.  Lmat: the factor's
// off-diagonal blocks as launch_cholesky_solve's launch-per-column form leaves them.
void launch_cov_factor_inverse(const double *Lmat, const double *Ldiag, int N, double *Z, hipStream_t s);
// Sinv = Z^T Z (N x N, both triangles, exactly symmetric): a workgroup per tile of the lower triangle, mirrored on store
void launch_cov_gram(const double *Z, int N, double *Sinv, hipStream_t s);
// cam_cov[c][x][y] = Sinv[off_c + x][off_c + y] for x, y < ldim_c, else 0; full (may be null) [nc][nc] = Sinv's leading part
void launch_cov_camera_blocks(const BaDev &d, const double *Sinv, int N, double *cam_cov, double *full, hipStream_t s);
// rows[k] (9 doubles) = Y_a^T sum_b Sinv[a][b] Y_b over the observations b of k's track in order, Y = Jc^T Q: a lane per
// observation
void launch_cov_point_rows(const BaDev &d, const double *obsrec, const int32_t *obs_lay, const double *Sinv, int N, double *rows,
    hipStream_t s);
// point_cov[j] = G (V_j^-1 + sum_a rows[a]) G^T, the rows added in observation order; zero for an invalid point.
// rows == nullptr: no camera is free (the first term alone)
void launch_cov_point_finish(const BaDev &d, const double *vinv, const double *rows, const uint8_t *valid, double *point_cov,
    hipStream_t s);

}  // namespace osfm
