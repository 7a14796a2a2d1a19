// Covariance kernels (ba_cov_kernels.h; DESIGN.md "Covariances").
//
// The inverse.  launch_cholesky_solve's launch-per-column form leaves L's off-diagonal 32 x 32 blocks in Lmat and
// inv(L_kk) of every diagonal block in Ldiag.  Z = L^-1 is lower block triangular with Z_kk = inv(L_kk) and, down block
// column k,  Z_ik = - inv(L_ii) sum_{m = k}^{i - 1} L_im Z_mk:  the block columns do not depend on each other, so a
// workgroup takes one and walks down it, every product eight k-steps of v_mfma_f64_16x16x4_f64 per wave (four waves, a
// 16 x 16 quadrant of the tile each: the register layout of ba_cholesky.hip's flow_mma).  Then S^-1 = Z^T Z, tile (a, b)
// of the lower triangle = sum_{m >= a} Z_ma^T Z_mb by one workgroup, m ascending, stored with its mirror image.
#include "ba_cov_kernels.h"

namespace osfm {

namespace {

constexpr int NB = 32;
typedef double v4d __attribute__((ext_vector_type(4)));
typedef double (*TileLds)[NB + 1];

// this thread's place in a 32 x 32 tile held by four waves in the accumulator layout of v_mfma_f64_16x16x4_f64: wave w has
// quadrant (w >> 1, w & 1), register e of a lane is element (tr0 + 4 e, tc)
struct TilePos { int tr0, tc, ar, ak, qi, qj; };
__device__ __forceinline__ TilePos tile_pos()
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    TilePos p;
    p.qi = wave >> 1; p.qj = wave & 1;
    p.tr0 = 16 * p.qi + (lane >> 4);
    p.tc = 16 * p.qj + (lane & 15);
    p.ar = lane & 15; p.ak = lane >> 4;
    return p;
}

// acc (+/-)= X Y^T: D[i][j] += sum_m X[i][m] Y[j][m], the k-steps in ascending order (A operand: X[16 qi + (lane & 15)]
// [4 s + (lane >> 4)], B operand: Y[16 qj + (lane & 15)][same k])
template <bool NEG>
__device__ __forceinline__ void tile_mma(v4d &acc, const double (*X)[NB + 1], const double (*Y)[NB + 1], const TilePos &p)
{
    const int xi = 16 * p.qi + p.ar, yj = 16 * p.qj + p.ar;
    double a[8], b[8];
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) { a[s8] = X[xi][4 * s8 + p.ak]; b[s8] = Y[yj][4 * s8 + p.ak]; }
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG ? -a[s8] : a[s8], b[s8], acc, 0, 0, 0);
}

// a 32 x 32 tile of a row-major matrix into LDS, as it is or transposed; 256 threads, coalesced rows
template <bool TRANSPOSE>
__device__ __forceinline__ void load_tile(const double *G, int ld, TileLds dst)
{
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = G[(size_t)r * ld + c0 + c];
        if (TRANSPOSE) dst[c0 + c][r] = v; else dst[r][c0 + c] = v;
    }
}

// inv(L_kk) from Ldiag (row-major 32 x 32, lower triangular: what lies above the diagonal is taken as zero)
__device__ __forceinline__ void load_diag_inverse(const double *Lk, TileLds dst)
{
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[r][c0 + c] = c0 + c <= r ? Lk[r * NB + c0 + c] : 0.0;
}

__global__ __launch_bounds__(256) void
cov_factor_inverse_kernel(const double *__restrict__ Lmat, const double *__restrict__ Ldiag, int N, double *Z)
{
    __shared__ __attribute__((aligned(16))) double X[NB][NB + 1];     // L_im, then inv(L_ii)
    __shared__ __attribute__((aligned(16))) double Y[NB][NB + 1];     // Z_mk transposed, then the sum transposed
    const int nblk = N / NB, k = blockIdx.x;
    const TilePos p = tile_pos();
    // Z_kk = inv(L_kk)
    load_diag_inverse(Ldiag + (size_t)k * NB * NB, X);
    __syncthreads();
    {
        double *Zkk = Z + (size_t)(k * NB) * N + k * NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) Zkk[(size_t)(p.tr0 + 4 * e) * N + p.tc] = X[p.tr0 + 4 * e][p.tc];
    }
    for (int i = k + 1; i < nblk; ++i) {
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int m = k; m < i; ++m) {
            // (the barrier also orders this workgroup's own stores of Z_mk in front of the loads of them)
            __threadfence_block();
            __syncthreads();
            load_tile<false>(Lmat + (size_t)(i * NB) * N + m * NB, N, X);
            load_tile<true>(Z + (size_t)(m * NB) * N + k * NB, N, Y);
            __syncthreads();
            tile_mma<false>(acc, X, Y, p);          // += L_im Z_mk
        }
        __syncthreads();
        // Z_ik = - inv(L_ii) T: T goes to LDS transposed, as the B operand's rows
        load_diag_inverse(Ldiag + (size_t)i * NB * NB, X);
#pragma unroll
        for (int e = 0; e < 4; ++e) Y[p.tc][p.tr0 + 4 * e] = acc[e];
        __syncthreads();
        v4d z = {0.0, 0.0, 0.0, 0.0};
        tile_mma<true>(z, X, Y, p);
        double *Zik = Z + (size_t)(i * NB) * N + k * NB;
#pragma unroll
        for (int e = 0; e < 4; ++e) Zik[(size_t)(p.tr0 + 4 * e) * N + p.tc] = z[e];
    }
}

__global__ __launch_bounds__(256) void
cov_gram_kernel(const double *__restrict__ Z, int N, double *__restrict__ Sinv)
{
    const int nblk = N / NB, a = blockIdx.y, b = blockIdx.x;
    if (b > a) return;
    __shared__ __attribute__((aligned(16))) double X[NB][NB + 1];     // Z_ma transposed
    __shared__ __attribute__((aligned(16))) double Y[NB][NB + 1];     // Z_mb transposed
    const TilePos p = tile_pos();
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int m = a; m < nblk; ++m) {
        __syncthreads();
        load_tile<true>(Z + (size_t)(m * NB) * N + a * NB, N, X);
        load_tile<true>(Z + (size_t)(m * NB) * N + b * NB, N, Y);
        __syncthreads();
        tile_mma<false>(acc, X, Y, p);              // += Z_ma^T Z_mb
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = p.tr0 + 4 * e, j = p.tc;
        if (a == b && j > i) continue;              // a diagonal tile: its lower triangle, mirrored (exact symmetry)
        const double v = acc[e];
        Sinv[(size_t)(a * NB + i) * N + b * NB + j] = v;
        Sinv[(size_t)(b * NB + j) * N + a * NB + i] = v;
    }
}

__global__ __launch_bounds__(256) void
cov_save_diagonal_kernel(const double *__restrict__ S, int N, double *__restrict__ sdiag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) sdiag[i] = S[(size_t)i * N + i];
}

__global__ __launch_bounds__(256) void
cov_pivot_ratio_kernel(const double *__restrict__ Ldiag, const double *__restrict__ sdiag, int n, double *out)
{
    __shared__ double sh[256];
    double m = 1.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double li = Ldiag[(size_t)(i / NB) * NB * NB + (i % NB) * NB + (i % NB)];      // 1 / L_ii
        const double v = 1.0 / (li * li * sdiag[i]);
        m = v > 0.0 && v <= 1.7976931348623157e308 ? fmin(m, v) : 0.0;                       // (NaN, inf, <= 0: no pivot)
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = fmin(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

__global__ __launch_bounds__(256) void
cov_point_valid_kernel(BaDev d, const double *__restrict__ obsrec, double min_ratio, uint8_t *__restrict__ valid)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d.M) return;
    const int k0 = d.pt_start[j], k1 = d.pt_start[j + 1];
    const double *x = d.points + 4 * (size_t)j;
    const double xn = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
    bool ok = k1 - k0 >= 2 && fabs(x[3]) >= 1e-12 * xn && xn > 0.0;
    if (ok) {
        double V[6] = {0, 0, 0, 0, 0, 0};       // 00 10 11 20 21 22
        for (int k = k0; k < k1; ++k) {
            const double *jp = obsrec + (size_t)k * kObsRec + kRecJp;
            int q = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) V[q++] += jp[a] * jp[b] + jp[3 + a] * jp[3 + b];
        }
        // the pivots of V's Cholesky factorisation (squared diagonal of its factor) against V's own diagonal
        const double p0 = V[0];
        const double l10 = V[1] / p0, l20 = V[3] / p0;
        const double p1 = V[2] - l10 * V[1];
        const double t21 = V[4] - l20 * V[1];
        const double p2 = V[5] - l20 * V[3] - t21 * t21 / p1;
        ok = p0 > 0.0 && p1 >= min_ratio * V[2] && p2 >= min_ratio * V[5] && p1 > 0.0 && p2 > 0.0;
    }
    valid[j] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void
cov_gather_obs_kernel(int n, const int32_t *__restrict__ map, const double2 *__restrict__ xy_in, const int32_t *__restrict__ cam_in,
    double2 *__restrict__ xy_out, int32_t *__restrict__ cam_out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int src = map[k];
    xy_out[k] = xy_in[src];
    cam_out[k] = cam_in[src];
}

__global__ __launch_bounds__(256) void
cov_camera_blocks_kernel(BaDev d, const double *__restrict__ Sinv, int N, double *__restrict__ cam_cov)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 36 * d.C) return;
    const int c = t / 36, x = (t % 36) / 6, y = t % 6;
    const int n = d.cam_ldim[c], off = d.cam_off[c];
    cam_cov[t] = x < n && y < n ? Sinv[(size_t)(off + x) * N + off + y] : 0.0;
}

__global__ __launch_bounds__(256) void
cov_pack_full_kernel(const double *__restrict__ Sinv, int N, int nc, double *__restrict__ full)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)nc * nc) return;
    const size_t i = t / nc, j = t % nc;
    full[t] = Sinv[i * N + j];
}

// t = Jc^T Q of a record (6 x 3; the camera's unused columns are zero in the record)
__device__ __forceinline__ void record_y(const double *rec, double (&t)[6][3])
{
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int c = 0; c < 3; ++c) t[x][c] = rec[kRecJc + x] * rec[kRecQ + c] + rec[kRecJc + 6 + x] * rec[kRecQ + 3 + c];
}

__global__ __launch_bounds__(256) void
cov_point_rows_kernel(BaDev d, const double *__restrict__ obsrec, const int32_t *__restrict__ obs_lay, const double *__restrict__ Sinv,
    int N, double *__restrict__ rows)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.O) return;
    const int j = d.obs_pt[k];
    const int k0 = d.pt_start[j], k1 = d.pt_start[j + 1];
    const int la = obs_lay[k], oa = la & 0xffffff, na = la >> 24;
    double U[6][3];                 // sum_b Sinv[a][b] Y_b
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int c = 0; c < 3; ++c) U[x][c] = 0.0;
    for (int kb = k0; kb < k1; ++kb) {
        const int lb = obs_lay[kb], ob = lb & 0xffffff, nb = lb >> 24;
        double tb[6][3];
        record_y(obsrec + (size_t)kb * kObsRec, tb);
#pragma unroll
        for (int x = 0; x < 6; ++x) {
            if (x >= na) continue;
            const double *srow = Sinv + (size_t)(oa + x) * N + ob;
#pragma unroll
            for (int y = 0; y < 6; ++y) {
                if (y >= nb) continue;
                const double sv = srow[y];
#pragma unroll
                for (int c = 0; c < 3; ++c) U[x][c] += sv * tb[y][c];
            }
        }
    }
    double ta[6][3];
    record_y(obsrec + (size_t)k * kObsRec, ta);
    double *out = rows + (size_t)k * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
#pragma unroll
            for (int x = 0; x < 6; ++x) v += x < na ? ta[x][r] * U[x][c] : 0.0;
            out[3 * r + c] = v;
        }
}

__global__ __launch_bounds__(256) void
cov_point_finish_kernel(BaDev d, const double *__restrict__ vinv, const double *__restrict__ rows, const uint8_t *__restrict__ valid,
    double *__restrict__ point_cov)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d.M) return;
    double *out = point_cov + (size_t)j * 9;
    if (!valid[j]) {
        for (int i = 0; i < 9; ++i) out[i] = 0.0;
        return;
    }
    double P[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) P[r][c] = vinv[(size_t)9 * j + 3 * r + c];
    if (rows)
        for (int k = d.pt_start[j]; k < d.pt_start[j + 1]; ++k)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) P[r][c] += rows[(size_t)9 * k + 3 * r + c];
    // the sum is symmetric but for the rounding of its terms: its symmetric part
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < r; ++c) { const double v = 0.5 * (P[r][c] + P[c][r]); P[r][c] = v; P[c][r] = v; }
    // G = d (x_0..2 / x_3) / dx . HJ, HJ the tangent basis of the homogeneous point
    const double *x = d.points + 4 * (size_t)j;
    double HJ[4][3], G[3][3];
    homog_jacobian(x, HJ);
    const double iw = 1.0 / x[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) G[r][c] = (HJ[r][c] - x[r] * iw * HJ[3][c]) * iw;
    double T[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[r][c] = G[r][0] * P[0][c] + G[r][1] * P[1][c] + G[r][2] * P[2][c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c <= r; ++c) {
            const double v = T[r][0] * G[c][0] + T[r][1] * G[c][1] + T[r][2] * G[c][2];
            out[3 * r + c] = v; out[3 * c + r] = v;
        }
}

inline int blocks_of(size_t n) { return (int)((n + 255) / 256); }

}  // namespace

void launch_cov_point_valid(const BaDev &d, const double *obsrec, double min_ratio, uint8_t *valid, hipStream_t s)
{
    if (d.M > 0) hipLaunchKernelGGL(cov_point_valid_kernel, dim3(blocks_of(d.M)), dim3(256), 0, s, d, obsrec, min_ratio, valid);
}

void launch_cov_gather_obs(int n, const int32_t *map, const double *xy_in, const int32_t *cam_in, double *xy_out, int32_t *cam_out,
    hipStream_t s)
{
    if (n > 0)
        hipLaunchKernelGGL(cov_gather_obs_kernel, dim3(blocks_of(n)), dim3(256), 0, s, n, map, reinterpret_cast<const double2 *>(xy_in),
            cam_in, reinterpret_cast<double2 *>(xy_out), cam_out);
}

void launch_cov_save_diagonal(const double *S, int N, double *sdiag, hipStream_t s)
{
    hipLaunchKernelGGL(cov_save_diagonal_kernel, dim3(blocks_of(N)), dim3(256), 0, s, S, N, sdiag);
}

void launch_cov_pivot_ratio(const double *Ldiag, const double *sdiag, int n, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(cov_pivot_ratio_kernel, dim3(1), dim3(256), 0, s, Ldiag, sdiag, n, out);
}

void launch_cov_factor_inverse(const double *Lmat, const double *Ldiag, int N, double *Z, hipStream_t s)
{
    hipLaunchKernelGGL(cov_factor_inverse_kernel, dim3(N / NB), dim3(256), 0, s, Lmat, Ldiag, N, Z);
}

void launch_cov_gram(const double *Z, int N, double *Sinv, hipStream_t s)
{
    hipLaunchKernelGGL(cov_gram_kernel, dim3(N / NB, N / NB), dim3(256), 0, s, Z, N, Sinv);
}

void launch_cov_camera_blocks(const BaDev &d, const double *Sinv, int N, double *cam_cov, double *full, hipStream_t s)
{
    if (cam_cov && d.C > 0) hipLaunchKernelGGL(cov_camera_blocks_kernel, dim3(blocks_of((size_t)36 * d.C)), dim3(256), 0, s, d, Sinv, N, cam_cov);
    if (full && d.nc > 0)
        hipLaunchKernelGGL(cov_pack_full_kernel, dim3(blocks_of((size_t)d.nc * d.nc)), dim3(256), 0, s, Sinv, N, d.nc, full);
}

void launch_cov_point_rows(const BaDev &d, const double *obsrec, const int32_t *obs_lay, const double *Sinv, int N, double *rows,
    hipStream_t s)
{
    if (d.O > 0) hipLaunchKernelGGL(cov_point_rows_kernel, dim3(blocks_of(d.O)), dim3(256), 0, s, d, obsrec, obs_lay, Sinv, N, rows);
}

void launch_cov_point_finish(const BaDev &d, const double *vinv, const double *rows, const uint8_t *valid, double *point_cov,
    hipStream_t s)
{
    if (d.M > 0) hipLaunchKernelGGL(cov_point_finish_kernel, dim3(blocks_of(d.M)), dim3(256), 0, s, d, vinv, rows, valid, point_cov);
}

}  // namespace osfm
