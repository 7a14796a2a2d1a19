// Initial alignment of a camera group on the GPU: a RANSAC over Tomasi-Kanade factorisations
// (robustlyEstimateTomasiKanadeFactorization, src/algorithms/tomasi_kanade.cpp:193-370; what it keeps of the
// reference and where it departs from it: INTEGRATION.md section 3).
//
// The tracks are N columns of a 2C x N matrix of normalised coordinates (x rows of the C cameras, then y rows).
//
//   tk_hypothesis_kernel   one wave per hypothesis: sample, centred rows, 2C x 2C Gram matrix, its eigenvectors by
//                          cyclic Jacobi in LDS, the metric upgrade in closed form, rotations, the usability test
//                          and the hypothesis' scoring table.
//   tk_score_kernel        the hot path, H x N x C: track tiles x hypothesis chunks.  A workgroup stages the tables
//                          of its chunk in LDS, every thread holds one track's 2C coordinates in registers and
//                          runs it through each table; per (tile, hypothesis) an integer count and an error sum
//                          reduced in a fixed order.
//   tk_select_kernel       sums the tile partials in tile order and applies the selection rule.
//   tk_fallback_*          only when no hypothesis is supported: the Gram matrix over all N columns as fixed-order
//                          tile partials, and the same factorisation on it.
//   tk_mask_kernel         one more scoring pass with the winner's table: the inlier mask.
//   tk_finish_kernel       the fallback's inlier count and mean error from the mask pass' tile partials.
//
// Scoring: the bases are orthonormal, so the least-squares intersection of a track's C rays is
// p = R^-1 sum_c (a_c x_c + b_c y_c) with R = sum_c (I - z_c z_c^T), where (a_c, b_c) are the track's coordinates
// plus the camera's offsets; R depends on the hypothesis alone and is inverted once.  A table holds the 2C x 3
// matrix A of the x and y axes, K = R^-1 A^T and the offsets: p = K a, residual = A p - a.
//
// Everything is double precision without contraction; no sum depends on arrival order (no floating-point
// atomics), so two calls return the same bytes.
#include <cmath>
#include <cstring>

#include "ba_solve.h"
#include "ransac_rand.h"
#include "tk_kernels.h"

namespace osfm {

namespace {

constexpr int kTkDim = 2 * kTkMaxCameras;           // rows of the measurement matrix at most
constexpr int kTkLd = kTkDim + 1;                   // padded leading dimension of the LDS matrices
constexpr int kTkBasis = 9 * kTkMaxCameras;
constexpr int kTkTable = 14 * kTkMaxCameras;        // a table's 14 C doubles at most

__host__ __device__ inline int tk_table_size(int C) { return 14 * C; }

// What the call leaves on the device for its one read-back; the inlier bytes follow it.
struct TkDeviceResult {
    int32_t status, iterations, usable_models, supported_models, best_iteration, num_inliers;
    double mean_error_px;
    double basis[kTkBasis];                         // solution 1
    double offsets[kTkDim];                         // by row of the measurement matrix
    // (not read back) the winner's scoring table and sample, for the mask pass
    double table[kTkTable];
    int32_t sample[kTkMaxSample];
    int32_t num_sample, pad_;
};

// LDS workspace of one factorisation
struct TkWork {
    double A[kTkDim][kTkLd];        // Gram matrix; the sweeps leave its eigenvalues on the diagonal
    double V[kTkDim][kTkLd];        // eigenvectors in columns
    double mean[kTkDim];
    double U[kTkDim][3];
    double M[6][7];                 // normal equations of the metric constraints, right-hand side in column 6
    double a6[3][6];
    double L[3][3], LV[3][3];
    double Rf[kTkDim][3];
    double axes[kTkMaxCameras][3][3];   // x, y, z axis per camera before the normalisation to camera 0
    int top[3];
    double B[kTkMaxCameras][9];     // solution 1, row-major
    double ang[kTkMaxCameras][2];
    double Rm[3][3], Ri[3][3];
    double table[kTkTable];
    int ok;
};

// Symmetric eigen-decomposition by cyclic Jacobi, cooperatively by one wave: A (n x n, LDS) ends diagonal, V holds
// the eigenvectors in its columns.  Every lane takes the same branches (they all read the same LDS words).
__device__ void tk_jacobi(double (*A)[kTkLd], double (*V)[kTkLd], int n, int lane)
{
    for (int e = lane; e < n * n; e += 64) V[e / n][e % n] = (e / n == e % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off += fabs(A[p][q]);
        if (off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (apq == 0.0) continue;
                __syncthreads();                                   // all lanes hold the three before anyone writes
                // an off-diagonal element that no longer changes either diagonal element is zero
                const double g = 100.0 * fabs(apq);
                if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    if (lane == 0) { A[p][q] = 0.0; A[q][p] = 0.0; }
                    __syncthreads();
                    continue;
                }
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                if (lane < n) {
                    const double akp = A[lane][p], akq = A[lane][q];
                    A[lane][p] = c * akp - s * akq; A[lane][q] = s * akp + c * akq;
                } else if (lane >= 32 && lane < 32 + n) {
                    const int k = lane - 32;
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
                __syncthreads();
                if (lane < n) {
                    const double apk = A[p][lane], aqk = A[q][lane];
                    A[p][lane] = c * apk - s * aqk; A[q][lane] = s * apk + c * aqk;
                }
                __syncthreads();
                if (lane == 0) { A[p][q] = 0.0; A[q][p] = 0.0; }
                __syncthreads();
            }
    }
}

// 3 x 3 version of the same on one lane (the metric L)
__device__ void tk_jacobi3(double (*A)[3], double (*V)[3])
{
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq);
                if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { A[p][q] = 0.0; A[q][p] = 0.0; continue; }
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
            }
    }
}

// row of the constraint u^T L v in the six unknowns (l00, l01, l02, l11, l12, l22)
__device__ void tk_sym_row(const double *u, const double *v, double *row)
{
    row[0] = u[0] * v[0];
    row[1] = u[0] * v[1] + u[1] * v[0];
    row[2] = u[0] * v[2] + u[2] * v[0];
    row[3] = u[1] * v[1];
    row[4] = u[1] * v[2] + u[2] * v[1];
    row[5] = u[2] * v[2];
}

// The serial part of a factorisation, on ONE lane, all arrays in LDS: from the eigen-decomposition of the Gram
// matrix (w.A diagonal, w.V) to the two-solution rotations w.B (solution 1).  false: no rank-3 measurement
// matrix (w3 <= 1e-12 w1), a singular constraint system or a metric that is not positive definite
// (lambda_min <= 1e-9 lambda_max).
__device__ bool tk_upgrade(TkWork &w, int C)
{
    const int n = 2 * C;
    // the three largest eigenvalues, descending
    w.top[0] = w.top[1] = w.top[2] = -1;
#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
        int best = -1;
        for (int i = 0; i < n; ++i) {
            if (i == w.top[0] || i == w.top[1]) continue;
            if (best < 0 || w.A[i][i] > w.A[best][best]) best = i;
        }
        w.top[m] = best;
    }
    const int *top = w.top;
    const double w1 = w.A[top[0]][top[0]], w3 = w.A[top[2]][top[2]];
    if (!(w3 > 1e-12 * w1)) return false;
    for (int r = 0; r < n; ++r) { w.U[r][0] = w.V[r][top[0]]; w.U[r][1] = w.V[r][top[1]]; w.U[r][2] = w.V[r][top[2]]; }
    // i^T L i = 1, j^T L j = 1, i^T L j = 0 per camera: linear in the symmetric L; their normal equations
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 7; ++j) w.M[i][j] = 0.0;
    for (int c = 0; c < C; ++c) {
        tk_sym_row(w.U[c], w.U[c], w.a6[0]);
        tk_sym_row(w.U[C + c], w.U[C + c], w.a6[1]);
        tk_sym_row(w.U[c], w.U[C + c], w.a6[2]);
#pragma unroll 1
        for (int e = 0; e < 3; ++e) {
            const double b = e < 2 ? 1.0 : 0.0;
#pragma unroll 1
            for (int i = 0; i < 6; ++i) {
                for (int j = 0; j < 6; ++j) w.M[i][j] += w.a6[e][i] * w.a6[e][j];
                w.M[i][6] += w.a6[e][i] * b;
            }
        }
    }
    // Gaussian elimination with partial pivoting
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        for (int i = k + 1; i < 6; ++i) if (fabs(w.M[i][k]) > fabs(w.M[piv][k])) piv = i;
        if (w.M[piv][k] == 0.0 || !isfinite(w.M[piv][k])) return false;
        if (piv != k) for (int j = k; j < 7; ++j) { const double t = w.M[k][j]; w.M[k][j] = w.M[piv][j]; w.M[piv][j] = t; }
        for (int i = k + 1; i < 6; ++i) {
            const double f = w.M[i][k] / w.M[k][k];
            for (int j = k; j < 7; ++j) w.M[i][j] -= f * w.M[k][j];
        }
    }
#pragma unroll 1
    for (int k = 5; k >= 0; --k) {
        double v = w.M[k][6];
        for (int j = k + 1; j < 6; ++j) v -= w.M[k][j] * w.M[j][6];
        w.M[k][6] = v / w.M[k][k];
    }
    w.L[0][0] = w.M[0][6]; w.L[0][1] = w.L[1][0] = w.M[1][6]; w.L[0][2] = w.L[2][0] = w.M[2][6];
    w.L[1][1] = w.M[3][6]; w.L[1][2] = w.L[2][1] = w.M[4][6]; w.L[2][2] = w.M[5][6];
    tk_jacobi3(w.L, w.LV);
    double lmin = w.L[0][0], lmax = w.L[0][0];
    for (int i = 1; i < 3; ++i) { lmin = fmin(lmin, w.L[i][i]); lmax = fmax(lmax, w.L[i][i]); }
    if (!(lmin > 1e-9 * lmax)) return false;
    // Q = V sqrt(Lambda); rows of U Q are the cameras' x and y axes up to scale
    for (int j = 0; j < 3; ++j) {
        const double sq = sqrt(w.L[j][j]);
        for (int i = 0; i < 3; ++i) w.LV[i][j] *= sq;
    }
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < 3; ++j)
            w.Rf[r][j] = w.U[r][0] * w.LV[0][j] + w.U[r][1] * w.LV[1][j] + w.U[r][2] * w.LV[2][j];
    // rotations: x normalised, y made orthogonal to it and normalised, z = x cross y
    for (int c = 0; c < C; ++c) {
        const double *x = w.Rf[c], *y = w.Rf[C + c];
        double *ax = w.axes[c][0], *ay = w.axes[c][1], *az = w.axes[c][2];
        const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        for (int i = 0; i < 3; ++i) ax[i] = x[i] / nx;
        const double d = y[0] * ax[0] + y[1] * ax[1] + y[2] * ax[2];
        for (int i = 0; i < 3; ++i) ay[i] = y[i] - d * ax[i];
        const double ny = sqrt(ay[0] * ay[0] + ay[1] * ay[1] + ay[2] * ay[2]);
        for (int i = 0; i < 3; ++i) ay[i] /= ny;
        az[0] = ax[1] * ay[2] - ax[2] * ay[1];
        az[1] = ax[2] * ay[0] - ax[0] * ay[2];
        az[2] = ax[0] * ay[1] - ax[1] * ay[0];
    }
    // B_c = B_0^T [x y z]_c: entry (i, j) is axis i of camera 0 times axis j of camera c
    bool finite = true;
#pragma unroll 1
    for (int c = 0; c < C; ++c)
#pragma unroll 1
        for (int e = 0; e < 9; ++e) {
            const double *u = w.axes[0][e / 3], *v = w.axes[c][e % 3];
            const double b = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
            w.B[c][e] = b;
            finite = finite && isfinite(b);
        }
    if (!finite) return false;
    // of the two mirror solutions B and T B T, T = diag(1, 1, -1), solution 1 has entry (0, 2) of camera 1 >= 0
    if (w.B[1][2] < 0.0)
        for (int c = 0; c < C; ++c) { w.B[c][2] = -w.B[c][2]; w.B[c][5] = -w.B[c][5]; w.B[c][6] = -w.B[c][6]; w.B[c][7] = -w.B[c][7]; }
    return true;
}

// isTomasiKanadeResultUsable (tomasi_kanade.cpp:446-470), literally: basisToPhiThetaRho(B, true)
// (OrthographicCamera.cpp:151-167) takes its angles from R B with R = [1 0 0; 0 0 -1; 0 1 0].
__device__ bool tk_usable(TkWork &w, int C)
{
    const double half_pi = 1.57079632679489661923;
    for (int c = 0; c < C; ++c) {
        const double b02 = w.B[c][2], b12 = -w.B[c][8], b22 = w.B[c][5];
        const double nrm = sqrt(b02 * b02 + b12 * b12 + b22 * b22);
        w.ang[c][0] = atan2(-b12, -b02) - half_pi;
        w.ang[c][1] = acos(b22 / nrm) - half_pi;
    }
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
            if (i == j) continue;
            if (fabs(w.ang[i][0] - w.ang[j][0]) < 0.1 && fabs(w.ang[i][1] - w.ang[j][1]) < 0.1) return false;
            double f = 0.0;
            for (int e = 0; e < 9; ++e) { const double d = w.B[i][e] - w.B[j][e]; f += d * d; }
            if (sqrt(f) < 0.1) return false;
        }
    return true;
}

// scoring table of the model w.B with the row means w.mean (one lane): A [2C][3], K = R^-1 A^T [3][2C], offsets [2C]
__device__ bool tk_make_table(TkWork &w, int C)
{
    const int n = 2 * C;
    double *A = w.table, *K = w.table + 6 * C, *off = w.table + 12 * C;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) w.Rm[i][j] = 0.0;
    for (int c = 0; c < C; ++c)
        for (int i = 0; i < 3; ++i) {
            A[3 * c + i] = w.B[c][3 * i];                     // x axis: column 0
            A[3 * (C + c) + i] = w.B[c][3 * i + 1];           // y axis: column 1
            for (int j = 0; j < 3; ++j)
                w.Rm[i][j] += (i == j ? 1.0 : 0.0) - w.B[c][3 * i + 2] * w.B[c][3 * j + 2];
        }
    const double (*m)[3] = w.Rm;
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2],
                 c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
    w.Ri[0][0] = c00 / det; w.Ri[1][0] = c01 / det; w.Ri[2][0] = c02 / det;
    w.Ri[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
    w.Ri[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
    w.Ri[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    w.Ri[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    w.Ri[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    w.Ri[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < n; ++r)
            K[i * n + r] = w.Ri[i][0] * A[3 * r] + w.Ri[i][1] * A[3 * r + 1] + w.Ri[i][2] * A[3 * r + 2];
    for (int r = 0; r < n; ++r) off[r] = -w.mean[r];
    return true;
}

// One track (its 2C coordinates d) under one table: true when every camera's reprojection error is <= thr pixels;
// *sum: the errors' sum over the cameras.  half_w / half_h: pixels per unit of the normalised coordinates.
template <int C>
__device__ __forceinline__ bool tk_track(const double *tbl, const double (&d)[2 * C], double half_w, double half_h, double thr,
    double *sum)
{
    constexpr int n = 2 * C;
    const double *A = tbl, *K = tbl + 6 * C, *off = tbl + 12 * C;
    double a[n];
#pragma unroll
    for (int r = 0; r < n; ++r) a[r] = d[r] + off[r];
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
#pragma unroll
    for (int r = 0; r < n; ++r) { p0 += K[r] * a[r]; p1 += K[n + r] * a[r]; p2 += K[2 * n + r] * a[r]; }
    bool pass = true;
    double es = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double rx = (A[3 * c] * p0 + A[3 * c + 1] * p1 + A[3 * c + 2] * p2) - a[c];
        const double ry = (A[3 * (C + c)] * p0 + A[3 * (C + c) + 1] * p1 + A[3 * (C + c) + 2] * p2) - a[C + c];
        const double ex = rx * half_w, ey = ry * half_h;
        const double e = sqrt(ex * ex + ey * ey);
        es += e;
        pass = pass && (e <= thr);
    }
    *sum = es;
    return pass;
}

// the same for a track whose coordinates lie in LDS / memory with a stride (sample tracks: C is a run-time value)
__device__ bool tk_track_dyn(const double *tbl, int C, const double *d, int stride, double half_w, double half_h, double thr,
    double *sum)
{
    const int n = 2 * C;
    const double *A = tbl, *K = tbl + 6 * C, *off = tbl + 12 * C;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    for (int r = 0; r < n; ++r) {
        const double a = d[r * stride] + off[r];
        p0 += K[r] * a; p1 += K[n + r] * a; p2 += K[2 * n + r] * a;
    }
    bool pass = true;
    double es = 0.0;
    for (int c = 0; c < C; ++c) {
        const double rx = (A[3 * c] * p0 + A[3 * c + 1] * p1 + A[3 * c + 2] * p2) - (d[c * stride] + off[c]);
        const double ry = (A[3 * (C + c)] * p0 + A[3 * (C + c) + 1] * p1 + A[3 * (C + c) + 2] * p2) - (d[(C + c) * stride] + off[C + c]);
        const double ex = rx * half_w, ey = ry * half_h;
        const double e = sqrt(ex * ex + ey * ey);
        es += e;
        pass = pass && (e <= thr);
    }
    *sum = es;
    return pass;
}

__global__ void tk_rows_kernel(const double *__restrict__ xy, int N, int C, int W, int H, double *__restrict__ rows)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    for (int c = 0; c < C; ++c) {
        rows[(size_t)c * N + t] = tk_normalise(xy[((size_t)t * C + c) * 2], W);
        rows[(size_t)(C + c) * N + t] = tk_normalise(xy[((size_t)t * C + c) * 2 + 1], H);
    }
}

// ---- one wave per hypothesis ----
__global__ __launch_bounds__(64) void tk_hypothesis_kernel(const double *__restrict__ rows, int N, int C, int S, uint64_t seed,
    uint64_t group, double half_w, double half_h, double thr, int32_t *__restrict__ valid, int32_t *__restrict__ fix_cnt,
    double *__restrict__ fix_err, int32_t *__restrict__ samples, double *__restrict__ bases, double *__restrict__ tables)
{
    __shared__ TkWork w;
    __shared__ double s_D[kTkDim][kTkMaxSample + 1];            // the sample's coordinates as read (not centred)
    __shared__ int32_t s_sample[kTkMaxSample];
    __shared__ double s_err[kTkMaxSample];
    __shared__ int32_t s_pass[kTkMaxSample];
    const int h = blockIdx.x, lane = threadIdx.x, n = 2 * C;
    if (lane == 0) {
        // the first S distinct values of ransac_rand(seed, group, h, k) % N, k = 0, 1, 2, ..., in draw order
        int have = 0;
        for (uint64_t k = 0; have < S; ++k) {
            const int32_t i = (int32_t)(ransac_rand(seed, group, (uint64_t)h, k) % (uint64_t)N);
            bool seen = false;
            for (int j = 0; j < have; ++j) seen = seen || s_sample[j] == i;
            if (!seen) s_sample[have++] = i;
        }
    }
    __syncthreads();
    for (int e = lane; e < n * S; e += 64) s_D[e / S][e % S] = rows[(size_t)(e / S) * N + s_sample[e % S]];
    if (lane < S) samples[(size_t)h * kTkMaxSample + lane] = s_sample[lane];
    __syncthreads();
    if (lane < n) {
        double m = 0.0;
        for (int k = 0; k < S; ++k) m += s_D[lane][k];
        w.mean[lane] = m / (double)S;
    }
    __syncthreads();
    for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e % n;
        const double mi = w.mean[i], mj = w.mean[j];
        double g = 0.0;
        for (int k = 0; k < S; ++k) g += (s_D[i][k] - mi) * (s_D[j][k] - mj);
        w.A[i][j] = g;
    }
    __syncthreads();
    tk_jacobi(w.A, w.V, n, lane);
    if (lane == 0) w.ok = (tk_upgrade(w, C) && tk_usable(w, C) && tk_make_table(w, C)) ? 1 : 0;
    __syncthreads();
    const bool ok = w.ok != 0;
    if (lane == 0) valid[h] = ok ? 1 : 0;
    if (!ok) {
        if (lane == 0) { fix_cnt[h] = 0; fix_err[h] = 0.0; }
        return;
    }
    for (int e = lane; e < 9 * C; e += 64) bases[(size_t)h * kTkBasis + e] = w.B[e / 9][e % 9];
    for (int e = lane; e < tk_table_size(C); e += 64) tables[(size_t)h * tk_table_size(C) + e] = w.table[e];
    // The sample's own tracks: the scoring kernel counts every track that passes, the consensus set leaves the
    // sample out, the error sum takes the whole sample in.  The difference is known here.
    if (lane < S) {
        double es = 0.0;
        const bool pass = tk_track_dyn(w.table, C, &s_D[0][lane], kTkMaxSample + 1, half_w, half_h, thr, &es);
        s_pass[lane] = pass ? 1 : 0;
        s_err[lane] = pass ? 0.0 : es;
    }
    __syncthreads();
    if (lane == 0) {
        int cnt = 0;
        double es = 0.0;
        for (int k = 0; k < S; ++k) { cnt += s_pass[k]; es += s_err[k]; }
        fix_cnt[h] = cnt; fix_err[h] = es;
    }
}

// fixed-order sum over the 256 threads of a workgroup: xor butterflies inside each wave (every lane ends with the
// same bits), then the caller adds the four waves' values in wave order
__device__ __forceinline__ double tk_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- the hot path: grid (track tiles, hypothesis chunks) ----
template <int C>
__global__ __launch_bounds__(kTkTile) void tk_score_kernel(const double *__restrict__ rows, int N, int H,
    const double *__restrict__ tables, const int32_t *__restrict__ valid, double half_w, double half_h, double thr,
    int32_t *__restrict__ part_cnt, double *__restrict__ part_err)
{
    constexpr int TS = 14 * C;
    __shared__ double s_tbl[kTkChunk * TS];
    __shared__ int32_t s_valid[kTkChunk];
    __shared__ double s_err[kTkChunk][4];
    __shared__ int32_t s_cnt[kTkChunk][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, h0 = blockIdx.y * kTkChunk;
    const int nh = min(kTkChunk, H - h0);
    if (tid < nh) s_valid[tid] = valid[h0 + tid];
    __syncthreads();
    for (int e = tid; e < nh * TS; e += kTkTile)
        s_tbl[e] = s_valid[e / TS] ? tables[(size_t)h0 * TS + e] : 0.0;          // (an invalid hypothesis wrote no table)
    const int t = tile * kTkTile + tid;
    const bool in = t < N;
    double d[2 * C];
#pragma unroll
    for (int r = 0; r < 2 * C; ++r) d[r] = in ? rows[(size_t)r * N + t] : 0.0;
    __syncthreads();
    for (int hh = 0; hh < nh; ++hh) {
        double v = 0.0;
        bool pass = false;
        if (s_valid[hh]) {
            double es;
            pass = tk_track<C>(s_tbl + hh * TS, d, half_w, half_h, thr, &es) && in;
            v = pass ? es : 0.0;
        }
        const unsigned long long bal = __ballot(pass);
        v = tk_wave_sum(v);
        if (lane == 0) { s_err[hh][wave] = v; s_cnt[hh][wave] = __popcll(bal); }
    }
    __syncthreads();
    if (tid < nh) {
        const size_t o = (size_t)tile * H + h0 + tid;
        part_cnt[o] = s_cnt[tid][0] + s_cnt[tid][1] + s_cnt[tid][2] + s_cnt[tid][3];
        part_err[o] = ((s_err[tid][0] + s_err[tid][1]) + s_err[tid][2]) + s_err[tid][3];
    }
}

// ---- the selection rule: among hypotheses with min_consensus tracks the most consensus tracks win, ties go to the
// lower mean error (over sample + consensus tracks and all cameras), further ties to the lower iteration ----
struct TkKey { int32_t cons; int32_t it; double mean; };
__device__ __forceinline__ bool tk_better(const TkKey &a, const TkKey &b)      // a beats b
{
    if (a.it < 0) return false;
    if (b.it < 0) return true;
    if (a.cons != b.cons) return a.cons > b.cons;
    if (a.mean != b.mean) return a.mean < b.mean;
    return a.it < b.it;
}

__global__ __launch_bounds__(256) void tk_select_kernel(int H, int tiles, int C, int S, int min_consensus,
    const int32_t *__restrict__ valid, const int32_t *__restrict__ fix_cnt, const double *__restrict__ fix_err,
    const int32_t *__restrict__ part_cnt, const double *__restrict__ part_err, const int32_t *__restrict__ samples,
    const double *__restrict__ bases, const double *__restrict__ tables, TkDeviceResult *__restrict__ res)
{
    __shared__ TkKey s_key[256];
    __shared__ int s_usable, s_supported;
    const int tid = threadIdx.x;
    if (tid == 0) { s_usable = 0; s_supported = 0; }
    __syncthreads();
    TkKey best = { 0, -1, 0.0 };
    for (int h = tid; h < H; h += 256) {
        if (!valid[h]) continue;
        atomicAdd(&s_usable, 1);
        int cnt = 0;
        double es = 0.0;
        for (int t = 0; t < tiles; ++t) { cnt += part_cnt[(size_t)t * H + h]; es += part_err[(size_t)t * H + h]; }
        const int cons = cnt - fix_cnt[h];
        if (cons < min_consensus) continue;
        atomicAdd(&s_supported, 1);
        es += fix_err[h];
        const TkKey k = { cons, h, es / ((double)(cons + S) * (double)C) };
        if (tk_better(k, best)) best = k;
    }
    s_key[tid] = best;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st && tk_better(s_key[tid + st], s_key[tid])) s_key[tid] = s_key[tid + st];
        __syncthreads();
    }
    const TkKey win = s_key[0];
    if (tid == 0) {
        res->iterations = H; res->usable_models = s_usable; res->supported_models = s_supported;
        res->best_iteration = win.it;
        res->status = win.it >= 0 ? OSFM_TK_RANSAC : OSFM_TK_FALLBACK;
        res->num_inliers = win.it >= 0 ? win.cons + S : 0;
        res->mean_error_px = win.it >= 0 ? win.mean : 0.0;
        res->num_sample = win.it >= 0 ? S : 0;
    }
    if (win.it < 0) return;
    const size_t h = (size_t)win.it;
    for (int e = tid; e < 9 * C; e += 256) res->basis[e] = bases[h * kTkBasis + e];
    for (int e = tid; e < tk_table_size(C); e += 256) res->table[e] = tables[h * tk_table_size(C) + e];
    for (int e = tid; e < 2 * C; e += 256) res->offsets[e] = tables[h * tk_table_size(C) + 12 * C + e];
    for (int e = tid; e < S; e += 256) res->sample[e] = samples[h * kTkMaxSample + e];
}

// ---- the fallback (no supported hypothesis): factorise ALL N tracks.  Row sums and the centred Gram matrix are
// tile partials summed in tile order. ----
__global__ __launch_bounds__(kTkTile) void tk_fallback_sums_kernel(const TkDeviceResult *__restrict__ res,
    const double *__restrict__ rows, int N, int C, double *__restrict__ part_sum)
{
    if (res->status != OSFM_TK_FALLBACK) return;
    __shared__ double s_w[kTkDim][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = 2 * C;
    const int t = blockIdx.x * kTkTile + tid;
    for (int r = 0; r < n; ++r) {
        const double v = tk_wave_sum(t < N ? rows[(size_t)r * N + t] : 0.0);
        if (lane == 0) s_w[r][wave] = v;
    }
    __syncthreads();
    if (tid < n) part_sum[(size_t)blockIdx.x * kTkDim + tid] = ((s_w[tid][0] + s_w[tid][1]) + s_w[tid][2]) + s_w[tid][3];
}

__global__ __launch_bounds__(kTkTile) void tk_fallback_gram_kernel(const TkDeviceResult *__restrict__ res,
    const double *__restrict__ rows, int N, int C, int tiles, const double *__restrict__ part_sum, double *__restrict__ part_gram)
{
    if (res->status != OSFM_TK_FALLBACK) return;
    __shared__ double s_mean[kTkDim];
    __shared__ double s_d[kTkDim][kTkTile + 1];
    const int tid = threadIdx.x, n = 2 * C;
    if (tid < n) {
        double m = 0.0;
        for (int b = 0; b < tiles; ++b) m += part_sum[(size_t)b * kTkDim + tid];
        s_mean[tid] = m / (double)N;
    }
    __syncthreads();
    const int t = blockIdx.x * kTkTile + tid;
    for (int r = 0; r < n; ++r) s_d[r][tid] = t < N ? rows[(size_t)r * N + t] - s_mean[r] : 0.0;
    __syncthreads();
    if (tid < n * n) {
        const int i = tid / n, j = tid % n;
        double g = 0.0;
        for (int k = 0; k < kTkTile; ++k) g += s_d[i][k] * s_d[j][k];
        part_gram[(size_t)blockIdx.x * (kTkDim * kTkDim) + tid] = g;
    }
}

__global__ __launch_bounds__(64) void tk_fallback_model_kernel(TkDeviceResult *__restrict__ res, int N, int C, int tiles,
    const double *__restrict__ part_sum, const double *__restrict__ part_gram)
{
    if (res->status != OSFM_TK_FALLBACK) return;
    __shared__ TkWork w;
    const int lane = threadIdx.x, n = 2 * C;
    if (lane < n) {
        double m = 0.0;
        for (int b = 0; b < tiles; ++b) m += part_sum[(size_t)b * kTkDim + lane];
        w.mean[lane] = m / (double)N;
    }
    for (int e = lane; e < n * n; e += 64) {
        double g = 0.0;
        for (int b = 0; b < tiles; ++b) g += part_gram[(size_t)b * (kTkDim * kTkDim) + e];
        w.A[e / n][e % n] = g;
    }
    __syncthreads();
    tk_jacobi(w.A, w.V, n, lane);
    if (lane == 0) w.ok = (tk_upgrade(w, C) && tk_make_table(w, C)) ? 1 : 0;      // (no usability test: :361-365)
    __syncthreads();
    if (!w.ok) {
        if (lane == 0) res->status = OSFM_TK_DEGENERATE;
        for (int e = lane; e < 9 * C; e += 64) res->basis[e] = (e % 9) % 4 == 0 ? 1.0 : 0.0;
        for (int e = lane; e < n; e += 64) res->offsets[e] = 0.0;
        return;
    }
    for (int e = lane; e < 9 * C; e += 64) res->basis[e] = w.B[e / 9][e % 9];
    for (int e = lane; e < tk_table_size(C); e += 64) res->table[e] = w.table[e];
    for (int e = lane; e < n; e += 64) res->offsets[e] = w.table[12 * C + e];
}

// ---- the winner once more over all tracks: the inlier mask (the sample's tracks are inliers); the tile partials
// serve the fallback's count and mean ----
template <int C>
__global__ __launch_bounds__(kTkTile) void tk_mask_kernel(const TkDeviceResult *__restrict__ res, const double *__restrict__ rows,
    int N, double half_w, double half_h, double thr, uint8_t *__restrict__ inlier, int32_t *__restrict__ part_cnt,
    double *__restrict__ part_err)
{
    constexpr int TS = 14 * C;
    __shared__ double s_tbl[TS];
    __shared__ int32_t s_sample[kTkMaxSample];
    __shared__ double s_err[4];
    __shared__ int32_t s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x * kTkTile + tid;
    const int status = res->status;
    if (status != OSFM_TK_RANSAC && status != OSFM_TK_FALLBACK) {
        if (t < N) inlier[t] = 0;
        if (tid == 0) { part_cnt[blockIdx.x] = 0; part_err[blockIdx.x] = 0.0; }
        return;
    }
    const int ns = res->num_sample;
    if (tid < TS) s_tbl[tid] = res->table[tid];
    if (tid < ns) s_sample[tid] = res->sample[tid];
    double d[2 * C];
#pragma unroll
    for (int r = 0; r < 2 * C; ++r) d[r] = t < N ? rows[(size_t)r * N + t] : 0.0;
    __syncthreads();
    double es;
    const bool pass = tk_track<C>(s_tbl, d, half_w, half_h, thr, &es) && t < N;
    bool member = pass;
    for (int k = 0; k < ns; ++k) member = member || s_sample[k] == t;
    if (t < N) inlier[t] = member ? 1 : 0;
    const unsigned long long bal = __ballot(pass);
    const double v = tk_wave_sum(pass ? es : 0.0);
    if (lane == 0) { s_err[wave] = v; s_cnt[wave] = __popcll(bal); }
    __syncthreads();
    if (tid == 0) {
        part_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        part_err[blockIdx.x] = ((s_err[0] + s_err[1]) + s_err[2]) + s_err[3];
    }
}

__global__ void tk_finish_kernel(TkDeviceResult *__restrict__ res, int tiles, int C, const int32_t *__restrict__ part_cnt,
    const double *__restrict__ part_err)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || res->status != OSFM_TK_FALLBACK) return;
    int cnt = 0;
    double es = 0.0;
    for (int b = 0; b < tiles; ++b) { cnt += part_cnt[b]; es += part_err[b]; }
    res->num_inliers = cnt;
    res->mean_error_px = cnt > 0 ? es / ((double)cnt * (double)C) : 0.0;
}

template <int C>
void tk_launch_score(dim3 grid, hipStream_t s, const double *rows, int N, int H, const double *tables, const int32_t *valid,
    double half_w, double half_h, double thr, int32_t *part_cnt, double *part_err)
{
    hipLaunchKernelGGL(tk_score_kernel<C>, grid, dim3(kTkTile), 0, s, rows, N, H, tables, valid, half_w, half_h, thr, part_cnt, part_err);
}
template <int C>
void tk_launch_mask(int tiles, hipStream_t s, const TkDeviceResult *res, const double *rows, int N, double half_w, double half_h,
    double thr, uint8_t *inlier, int32_t *part_cnt, double *part_err)
{
    hipLaunchKernelGGL(tk_mask_kernel<C>, dim3(tiles), dim3(kTkTile), 0, s, res, rows, N, half_w, half_h, thr, inlier, part_cnt, part_err);
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

void identity_outputs(int C, double *basis_1, double *basis_2, double *offsets, uint8_t *inlier, int n_inlier)
{
    for (int c = 0; c < C; ++c)
        for (int e = 0; e < 9; ++e) basis_1[9 * c + e] = basis_2[9 * c + e] = (e % 4 == 0) ? 1.0 : 0.0;
    if (offsets) for (int e = 0; e < 2 * C; ++e) offsets[e] = 0.0;
    if (inlier && n_inlier > 0) memset(inlier, 0, (size_t)n_inlier);
}

}  // namespace

int tk_check_options(const osfm_tk_options *opts, int num_cameras, osfm_tk_options *out, int *iterations)
{
    if (opts) *out = *opts; else osfm_tk_options_default(out);
    if (num_cameras < kTkMinCameras || num_cameras > kTkMaxCameras) {
        set_error("tk_align: %d cameras (a group has %d..%d)", num_cameras, kTkMinCameras, kTkMaxCameras); return OSFM_E_ARG;
    }
    if (out->sample_size < kTkMinSample || out->sample_size > kTkMaxSample) {
        set_error("tk_align: sample_size %d outside %d..%d", out->sample_size, kTkMinSample, kTkMaxSample); return OSFM_E_ARG;
    }
    if (!(out->probability > 0.0 && out->probability < 1.0) || !(out->inlier_ratio > 0.0 && out->inlier_ratio < 1.0) ||
        !(out->max_error_px > 0.0) || out->min_consensus < 0 || out->max_iterations < 0 || out->max_iterations > (1 << 20)) {
        set_error("tk_align: bad options"); return OSFM_E_ARG;
    }
    int H = out->max_iterations;
    if (H == 0) {
        // the reference's count (:212), held to 1 .. 2^20 (point 11): a quotient below one
        // means that one sample already reaches the probability, not that none is needed
        const double h = floor(log(1.0 - out->probability) / log(1.0 - pow(out->inlier_ratio, (double)out->sample_size)));
        H = h < 1.0 ? 1 : (h > (double)(1 << 20) ? (1 << 20) : (int)h);
    }
    *iterations = H;
    return OSFM_OK;
}

void launch_tk_rows(const double *xy, int N, int C, int W, int H, double *rows, hipStream_t s)
{
    if (N <= 0) return;
    hipLaunchKernelGGL(tk_rows_kernel, dim3((N + 255) / 256), dim3(256), 0, s, xy, N, C, W, H, rows);
}

int tk_align_core(const double *rows, int N, int C, int W, int H, const osfm_tk_options &o, int iterations, uint64_t group_id,
    hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b, double *basis_1, double *basis_2, double *offsets, uint8_t *inlier,
    int inlier_capacity, osfm_tk_result *result)
{
    memset(result, 0, sizeof(*result));
    result->best_iteration = -1;
    const int n_inlier = inlier ? std::min(N, std::max(inlier_capacity, 0)) : 0;
    const int S = o.sample_size;
    if (N < std::max(10, S)) {                      // the reference throws (tomasi_kanade.cpp:202-205)
        result->status = OSFM_TK_TOO_FEW;
        identity_outputs(C, basis_1, basis_2, offsets, inlier, n_inlier);
        return OSFM_OK;
    }
    const int Hn = iterations, tiles = (N + kTkTile - 1) / kTkTile, chunks = (Hn + kTkChunk - 1) / kTkChunk, TS = tk_table_size(C);
    // one block of device memory, carved up
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o0 = at; at += align16(bytes); return o0; };
    const size_t o_res = carve(sizeof(TkDeviceResult) + (size_t)N);
    const size_t o_valid = carve((size_t)Hn * 4), o_fcnt = carve((size_t)Hn * 4), o_ferr = carve((size_t)Hn * 8);
    const size_t o_samp = carve((size_t)Hn * kTkMaxSample * 4), o_bases = carve((size_t)Hn * kTkBasis * 8);
    const size_t o_tables = carve((size_t)Hn * TS * 8);
    const size_t o_pcnt = carve((size_t)tiles * Hn * 4), o_perr = carve((size_t)tiles * Hn * 8);
    const size_t o_fsum = carve((size_t)tiles * kTkDim * 8), o_fgram = carve((size_t)tiles * kTkDim * kTkDim * 8);
    const size_t o_mcnt = carve((size_t)tiles * 4), o_merr = carve((size_t)tiles * 8);
    DevArray block;
    OSFM_RETURN_IF(block.alloc(at));
    char *base = block.as<char>();
    TkDeviceResult *res = reinterpret_cast<TkDeviceResult *>(base + o_res);
    uint8_t *d_inlier = reinterpret_cast<uint8_t *>(base + o_res + sizeof(TkDeviceResult));
    int32_t *valid = reinterpret_cast<int32_t *>(base + o_valid), *fcnt = reinterpret_cast<int32_t *>(base + o_fcnt);
    double *ferr = reinterpret_cast<double *>(base + o_ferr);
    int32_t *samp = reinterpret_cast<int32_t *>(base + o_samp);
    double *bases = reinterpret_cast<double *>(base + o_bases), *tables = reinterpret_cast<double *>(base + o_tables);
    int32_t *pcnt = reinterpret_cast<int32_t *>(base + o_pcnt);
    double *perr = reinterpret_cast<double *>(base + o_perr);
    double *fsum = reinterpret_cast<double *>(base + o_fsum), *fgram = reinterpret_cast<double *>(base + o_fgram);
    int32_t *mcnt = reinterpret_cast<int32_t *>(base + o_mcnt);
    double *merr = reinterpret_cast<double *>(base + o_merr);
    const double half_w = 0.5 * (double)W, half_h = 0.5 * (double)H, thr = o.max_error_px;

    hipLaunchKernelGGL(tk_hypothesis_kernel, dim3(Hn), dim3(64), 0, s, rows, N, C, S, (uint64_t)o.seed, group_id, half_w, half_h, thr,
        valid, fcnt, ferr, samp, bases, tables);
    OSFM_HIP_CHECK(hipEventRecord(ev_a, s));
    const dim3 grid(tiles, chunks);
    switch (C) {
    case 3: tk_launch_score<3>(grid, s, rows, N, Hn, tables, valid, half_w, half_h, thr, pcnt, perr); break;
    case 4: tk_launch_score<4>(grid, s, rows, N, Hn, tables, valid, half_w, half_h, thr, pcnt, perr); break;
    case 5: tk_launch_score<5>(grid, s, rows, N, Hn, tables, valid, half_w, half_h, thr, pcnt, perr); break;
    case 6: tk_launch_score<6>(grid, s, rows, N, Hn, tables, valid, half_w, half_h, thr, pcnt, perr); break;
    case 7: tk_launch_score<7>(grid, s, rows, N, Hn, tables, valid, half_w, half_h, thr, pcnt, perr); break;
    default: tk_launch_score<8>(grid, s, rows, N, Hn, tables, valid, half_w, half_h, thr, pcnt, perr); break;
    }
    OSFM_HIP_CHECK(hipEventRecord(ev_b, s));
    hipLaunchKernelGGL(tk_select_kernel, dim3(1), dim3(256), 0, s, Hn, tiles, C, S, (int)o.min_consensus, valid, fcnt, ferr, pcnt, perr,
        samp, bases, tables, res);
    // (these three return at once unless the selection found no supported model)
    hipLaunchKernelGGL(tk_fallback_sums_kernel, dim3(tiles), dim3(kTkTile), 0, s, res, rows, N, C, fsum);
    hipLaunchKernelGGL(tk_fallback_gram_kernel, dim3(tiles), dim3(kTkTile), 0, s, res, rows, N, C, tiles, fsum, fgram);
    hipLaunchKernelGGL(tk_fallback_model_kernel, dim3(1), dim3(64), 0, s, res, N, C, tiles, fsum, fgram);
    switch (C) {
    case 3: tk_launch_mask<3>(tiles, s, res, rows, N, half_w, half_h, thr, d_inlier, mcnt, merr); break;
    case 4: tk_launch_mask<4>(tiles, s, res, rows, N, half_w, half_h, thr, d_inlier, mcnt, merr); break;
    case 5: tk_launch_mask<5>(tiles, s, res, rows, N, half_w, half_h, thr, d_inlier, mcnt, merr); break;
    case 6: tk_launch_mask<6>(tiles, s, res, rows, N, half_w, half_h, thr, d_inlier, mcnt, merr); break;
    case 7: tk_launch_mask<7>(tiles, s, res, rows, N, half_w, half_h, thr, d_inlier, mcnt, merr); break;
    default: tk_launch_mask<8>(tiles, s, res, rows, N, half_w, half_h, thr, d_inlier, mcnt, merr); break;
    }
    hipLaunchKernelGGL(tk_finish_kernel, dim3(1), dim3(64), 0, s, res, tiles, C, mcnt, merr);
    OSFM_HIP_CHECK(hipGetLastError());
    // the one read-back: the result block up to its offsets, and the inlier bytes behind it
    std::vector<char> host(sizeof(TkDeviceResult) + (size_t)N);
    OSFM_HIP_CHECK(hipMemcpyAsync(host.data(), res, host.size(), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.0f;
    OSFM_HIP_CHECK(hipEventElapsedTime(&ms, ev_a, ev_b));
    const TkDeviceResult *r = reinterpret_cast<const TkDeviceResult *>(host.data());
    result->status = r->status; result->iterations = r->iterations; result->usable_models = r->usable_models;
    result->supported_models = r->supported_models; result->best_iteration = r->best_iteration;
    result->num_inliers = r->num_inliers; result->mean_error_px = r->mean_error_px; result->score_kernel_ms = ms;
    for (int c = 0; c < C; ++c)
        for (int e = 0; e < 9; ++e) {
            const double v = r->basis[9 * c + e];
            basis_1[9 * c + e] = v;
            // T B T with T = diag(1, 1, -1): entries (0,2), (1,2), (2,0), (2,1) change sign
            basis_2[9 * c + e] = (e == 2 || e == 5 || e == 6 || e == 7) ? -v : v;
        }
    if (offsets) for (int c = 0; c < C; ++c) { offsets[2 * c] = r->offsets[c]; offsets[2 * c + 1] = r->offsets[C + c]; }
    if (n_inlier > 0) memcpy(inlier, host.data() + sizeof(TkDeviceResult), (size_t)n_inlier);
    return OSFM_OK;
}

}  // namespace osfm

using namespace osfm;

int osfm_tk_options_default(osfm_tk_options *o)
{
    if (!o) { set_error("tk_options_default: null"); return OSFM_E_ARG; }
    o->sample_size = 10; o->max_iterations = 0; o->probability = 0.999; o->inlier_ratio = 0.7;
    o->min_consensus = 25; o->device = 0; o->max_error_px = 3.0; o->seed = 0;
    return OSFM_OK;
}

int osfm_tk_align(const double *xy, int32_t num_tracks, int32_t num_cameras, int32_t img_width, int32_t img_height,
    const osfm_tk_options *opts, uint64_t group_id, double *basis_1, double *basis_2, double *offsets, uint8_t *inlier,
    osfm_tk_result *result)
{
    if (!xy || num_tracks < 0 || img_width <= 0 || img_height <= 0 || !basis_1 || !basis_2 || !result) {
        set_error("tk_align: bad arguments"); return OSFM_E_ARG;
    }
    osfm_tk_options o;
    int iterations = 0;
    OSFM_RETURN_IF(tk_check_options(opts, num_cameras, &o, &iterations));
    const int N = num_tracks, C = num_cameras;
    OSFM_RETURN_IF(select_device(o.device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DevArray d_xy, d_rows;
    if (N >= std::max(10, (int)o.sample_size)) {
        OSFM_RETURN_IF(upload(d_xy, xy, (size_t)N * C * 2, sg.s));
        OSFM_RETURN_IF(d_rows.alloc((size_t)N * C * 2 * 8));
        launch_tk_rows(d_xy.as<double>(), N, C, img_width, img_height, d_rows.as<double>(), sg.s);
    }
    return tk_align_core(d_rows.as<double>(), N, C, img_width, img_height, o, iterations, group_id, sg.s, sg.ev[0].a, sg.ev[0].b,
        basis_1, basis_2, offsets, inlier, N, result);
}

int osfm_tk_resolve_ambiguity(int32_t num_cameras, const double *basis_1, const double *basis_2, const double *global_rotation,
    const uint8_t *has_global, int32_t *choice)
{
    if (num_cameras < 1 || !basis_1 || !basis_2 || !global_rotation || !has_global || !choice) {
        set_error("tk_resolve_ambiguity: bad arguments"); return OSFM_E_ARG;
    }
    *choice = 1;
    int a = -1, b = -1;
    for (int c = 0; c < num_cameras && b < 0; ++c)
        if (has_global[c]) { if (a < 0) a = c; else b = c; }
    if (b < 0) return OSFM_OK;
    // z_a - z_b in the frame where a is canonical: (0, 0, 1) - (R_a^T R_b) e_z, matrices row-major local -> world
    auto look_difference = [](const double *Ra, const double *Rb, double *out) {
        for (int i = 0; i < 3; ++i) {
            const double zb = Ra[i] * Rb[2] + Ra[3 + i] * Rb[5] + Ra[6 + i] * Rb[8];      // column i of R_a times column z of R_b
            out[i] = (i == 2 ? 1.0 : 0.0) - zb;
        }
    };
    double g[3], m1[3], m2[3];
    look_difference(global_rotation + 9 * a, global_rotation + 9 * b, g);
    look_difference(basis_1 + 9 * a, basis_1 + 9 * b, m1);
    look_difference(basis_2 + 9 * a, basis_2 + 9 * b, m2);
    const double s1 = g[0] * m1[0] + g[1] * m1[1] + g[2] * m1[2];
    const double s2 = g[0] * m2[0] + g[1] * m2[1] + g[2] * m2[2];
    *choice = s2 > s1 ? 2 : 1;
    return OSFM_OK;
}
