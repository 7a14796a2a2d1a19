// Placing one view against triangulated points on the GPU: a RANSAC over affine cameras (what is computed, in
// full: INTEGRATION.md section 3b; layout and measurements: DESIGN.md section 3x).  The structure is that of
// tk_kernels.hip.
//
// The camera model u = x.p / s - o_x, v = y.p / s - o_y is linear in the point, so a view is the affine camera
// (u, v) = A X + (c, d).  The correspondences are five rows of N doubles: X, Y, Z, u, v.
//
//   resect_hypothesis_kernel  one lane per hypothesis: sample, the 3 x 3 elimination with two right-hand sides, the
//                             pivot and axis-ratio tests, the hypothesis' table (a, c, b, d: 8 doubles).
//   resect_score_kernel       the hot path, H x N: point tiles x hypothesis chunks.  A workgroup stages the tables
//                             of its chunk in LDS, every thread holds one point's five doubles in registers and
//                             runs it through each table; per (tile, hypothesis) an integer count and an error sum
//                             reduced in a fixed order.
//   resect_select_kernel      sums the tile partials in tile order and applies the selection rule.
//   resect_refit_*            the winner's inliers: centroid sums, then the 6 + 3 + 3 centred sums, as tile partials.
//   resect_model_kernel       one lane: the SPD solve, the projection onto the camera model, the final camera.
//   resect_mask_kernel        all points once more under the final camera: the inlier bytes and tile partials.
//   resect_finish_kernel      the final count and mean error.
//
// Everything is double precision without contraction; no sum depends on arrival order (no floating-point
// atomics), so two calls return the same bytes.
#include <cmath>
#include <cstring>

#include "ba_solve.h"
#include "ransac_rand.h"
#include "resect_kernels.h"
#include "tk_kernels.h"

namespace osfm {

namespace {

constexpr int kResectTable = 8;         // a[3], c, b[3], d

// What the call leaves on the device for its one read-back; the inlier bytes follow it.
struct ResectDeviceResult {
    int32_t status, iterations, usable_models, supported_models, best_iteration, ransac_inliers, num_inliers, refit_used;
    double mean_error_px;
    double rotation[9];
    double scale;
    double offsets[2];
    // (not read back) the winner's table and sample for the refit, the final camera's table for the mask pass
    double table[kResectTable];
    double final_table[kResectTable];
    int32_t sample[kResectSample];
};

// Error in pixels of one point under one table.  half_w / half_h: pixels per unit of the normalised coordinates.
__device__ __forceinline__ double resect_error(const double *t, double X, double Y, double Z, double u, double v, double half_w,
    double half_h)
{
    const double ru = (((t[0] * X + t[1] * Y) + t[2] * Z) + t[3]) - u;
    const double rv = (((t[4] * X + t[5] * Y) + t[6] * Z) + t[7]) - v;
    const double ex = ru * half_w, ey = rv * half_h;
    return sqrt(ex * ex + ey * ey);
}

// rows a and b change places when `swap` holds (selects, so that the rows stay in registers)
__device__ __forceinline__ void resect_swap_rows(bool swap, double (&a)[5], double (&b)[5])
{
#pragma unroll
    for (int j = 0; j < 5; ++j) { const double x = a[j], y = b[j]; a[j] = swap ? y : x; b[j] = swap ? x : y; }
}

// M = [D | r_u | r_v], D 3 x 3: Gaussian elimination with partial pivoting, both right-hand sides at once.
// false: a pivot is below min_pivot times the largest entry of D (or D is zero / not finite).
__device__ __forceinline__ bool resect_solve3(double (&M)[3][5], double min_pivot, double (&a)[3], double (&b)[3])
{
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) big = fmax(big, fabs(M[i][j]));
    if (!(big > 0.0) || !isfinite(big)) return false;
    const double least = min_pivot * big;
    {
        int piv = 0;
        double pv = fabs(M[0][0]);
        if (fabs(M[1][0]) > pv) { piv = 1; pv = fabs(M[1][0]); }
        if (fabs(M[2][0]) > pv) { piv = 2; pv = fabs(M[2][0]); }
        resect_swap_rows(piv == 1, M[0], M[1]);
        resect_swap_rows(piv == 2, M[0], M[2]);
        if (!(pv >= least)) return false;
        const double f1 = M[1][0] / M[0][0], f2 = M[2][0] / M[0][0];
#pragma unroll
        for (int j = 1; j < 5; ++j) { M[1][j] -= f1 * M[0][j]; M[2][j] -= f2 * M[0][j]; }
    }
    resect_swap_rows(fabs(M[2][1]) > fabs(M[1][1]), M[1], M[2]);
    if (!(fabs(M[1][1]) >= least)) return false;
    {
        const double f = M[2][1] / M[1][1];
#pragma unroll
        for (int j = 2; j < 5; ++j) M[2][j] -= f * M[1][j];
    }
    if (!(fabs(M[2][2]) >= least)) return false;
    a[2] = M[2][3] / M[2][2];
    a[1] = (M[1][3] - M[1][2] * a[2]) / M[1][1];
    a[0] = ((M[0][3] - M[0][1] * a[1]) - M[0][2] * a[2]) / M[0][0];
    b[2] = M[2][4] / M[2][2];
    b[1] = (M[1][4] - M[1][2] * b[2]) / M[1][1];
    b[0] = ((M[0][4] - M[0][1] * b[1]) - M[0][2] * b[2]) / M[0][0];
    return true;
}

// eigenvalues l1 >= l2 of G = A A^T for A = [a; b]; false when they are not positive and finite
__device__ __forceinline__ bool resect_axes(const double (&a)[3], const double (&b)[3], double *g00, double *g01, double *g11,
    double *l1, double *l2)
{
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const double mid = 0.5 * (aa + bb), hd = 0.5 * (aa - bb);
    const double r = sqrt(hd * hd + ab * ab);
    *g00 = aa; *g01 = ab; *g11 = bb;
    *l1 = mid + r; *l2 = mid - r;
    return isfinite(*l1) && *l2 > 0.0;
}

// ---- one lane per hypothesis ----
__global__ __launch_bounds__(64) void resect_hypothesis_kernel(const double *__restrict__ data, int N, int H, uint64_t seed,
    uint64_t stream, double half_w, double half_h, double thr, double min_pivot, double min_axis_ratio,
    int32_t *__restrict__ valid, int32_t *__restrict__ fix_cnt, double *__restrict__ fix_err, int32_t *__restrict__ samples,
    double *__restrict__ tables)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= H) return;
    // the first four distinct values of ransac_rand(seed, stream, h, k) % N, k = 0, 1, 2, ..., in draw order
    int32_t s0 = -1, s1 = -1, s2 = -1, s3 = -1;
    int have = 0;
    for (uint64_t k = 0; have < kResectSample; ++k) {
        const int32_t i = (int32_t)(ransac_rand(seed, stream, (uint64_t)h, k) % (uint64_t)N);
        if (i == s0 || i == s1 || i == s2) continue;
        if (have == 0) s0 = i; else if (have == 1) s1 = i; else if (have == 2) s2 = i; else s3 = i;
        ++have;
    }
    const int32_t smp[kResectSample] = { s0, s1, s2, s3 };
    double p[kResectSample][5];
#pragma unroll
    for (int k = 0; k < kResectSample; ++k) {
        samples[(size_t)h * kResectSample + k] = smp[k];
#pragma unroll
        for (int r = 0; r < 5; ++r) p[k][r] = data[(size_t)r * N + smp[k]];
    }
    double M[3][5];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 5; ++r) M[k][r] = p[k + 1][r] - p[0][r];
    double a[3], b[3];
    bool ok = resect_solve3(M, min_pivot, a, b);
    double g00, g01, g11, l1 = 0.0, l2 = 0.0;
    ok = ok && resect_axes(a, b, &g00, &g01, &g11, &l1, &l2);
    ok = ok && !(sqrt(l2 / l1) < min_axis_ratio);
    double t[kResectTable];
    t[0] = a[0]; t[1] = a[1]; t[2] = a[2];
    t[3] = p[0][3] - ((a[0] * p[0][0] + a[1] * p[0][1]) + a[2] * p[0][2]);
    t[4] = b[0]; t[5] = b[1]; t[6] = b[2];
    t[7] = p[0][4] - ((b[0] * p[0][0] + b[1] * p[0][1]) + b[2] * p[0][2]);
#pragma unroll
    for (int e = 0; e < kResectTable; ++e) ok = ok && isfinite(t[e]);
    valid[h] = ok ? 1 : 0;
    if (!ok) { fix_cnt[h] = 0; fix_err[h] = 0.0; return; }
#pragma unroll
    for (int e = 0; e < kResectTable; ++e) tables[(size_t)h * kResectTable + e] = t[e];
    // The sample's own points are inliers by construction: the scoring kernel counts every point below the
    // threshold, so what it counted of the sample is taken out again, and a sample point it did not count (an
    // error at rounding level against a tiny threshold) brings its error into the sum.
    int cnt = 0;
    double es = 0.0;
#pragma unroll
    for (int k = 0; k < kResectSample; ++k) {
        const double e = resect_error(t, p[k][0], p[k][1], p[k][2], p[k][3], p[k][4], half_w, half_h);
        const bool pass = e < thr;
        cnt += pass ? 1 : 0;
        es += pass ? 0.0 : e;
    }
    fix_cnt[h] = cnt; fix_err[h] = es;
}

// fixed-order sum over the 256 threads of a workgroup: xor butterflies inside each wave (every lane ends with the
// same bits), then the caller adds the four waves' values in wave order
__device__ __forceinline__ double resect_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- the hot path: grid (point tiles, hypothesis chunks) ----
__global__ __launch_bounds__(kResectTile) void resect_score_kernel(const double *__restrict__ data, int N, int H,
    const double *__restrict__ tables, const int32_t *__restrict__ valid, double half_w, double half_h, double thr,
    int32_t *__restrict__ part_cnt, double *__restrict__ part_err)
{
    __shared__ double s_tbl[kResectChunk * kResectTable];
    __shared__ int32_t s_valid[kResectChunk];
    __shared__ double s_err[kResectChunk][4];
    __shared__ int32_t s_cnt[kResectChunk][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, h0 = blockIdx.y * kResectChunk;
    const int nh = min(kResectChunk, H - h0);
    if (tid < nh) s_valid[tid] = valid[h0 + tid];
    __syncthreads();
    if (tid < nh * kResectTable)
        s_tbl[tid] = s_valid[tid / kResectTable] ? tables[(size_t)h0 * kResectTable + tid] : 0.0;   // (an unusable hypothesis wrote no table)
    const int t = tile * kResectTile + tid;
    const bool in = t < N;
    const double X = in ? data[t] : 0.0, Y = in ? data[(size_t)N + t] : 0.0, Z = in ? data[2 * (size_t)N + t] : 0.0;
    const double u = in ? data[3 * (size_t)N + t] : 0.0, v = in ? data[4 * (size_t)N + t] : 0.0;
    __syncthreads();
    for (int hh = 0; hh < nh; ++hh) {
        double e = 0.0;
        bool pass = false;
        if (s_valid[hh]) {
            e = resect_error(s_tbl + hh * kResectTable, X, Y, Z, u, v, half_w, half_h);
            pass = in && e < thr;
        }
        const unsigned long long bal = __ballot(pass);
        const double w = resect_wave_sum(pass ? e : 0.0);
        if (lane == 0) { s_err[hh][wave] = w; s_cnt[hh][wave] = __popcll(bal); }
    }
    __syncthreads();
    if (tid < nh) {
        const size_t o = (size_t)tile * H + h0 + tid;
        part_cnt[o] = s_cnt[tid][0] + s_cnt[tid][1] + s_cnt[tid][2] + s_cnt[tid][3];
        part_err[o] = ((s_err[tid][0] + s_err[tid][1]) + s_err[tid][2]) + s_err[tid][3];
    }
}

// ---- the selection rule: among hypotheses with min_consensus inliers outside the sample the most inliers win, ties
// go to the lower mean error over them, further ties to the lower iteration ----
struct ResectKey { int32_t inl; int32_t it; double mean; };
__device__ __forceinline__ bool resect_better(const ResectKey &a, const ResectKey &b)      // a beats b
{
    if (a.it < 0) return false;
    if (b.it < 0) return true;
    if (a.inl != b.inl) return a.inl > b.inl;
    if (a.mean != b.mean) return a.mean < b.mean;
    return a.it < b.it;
}

__global__ __launch_bounds__(256) void resect_select_kernel(int H, int tiles, int min_consensus, double scale,
    const int32_t *__restrict__ valid, const int32_t *__restrict__ fix_cnt, const double *__restrict__ fix_err,
    const int32_t *__restrict__ part_cnt, const double *__restrict__ part_err, const int32_t *__restrict__ samples,
    const double *__restrict__ tables, ResectDeviceResult *__restrict__ res)
{
    __shared__ ResectKey s_key[256];
    __shared__ int s_usable, s_supported;
    const int tid = threadIdx.x;
    if (tid == 0) { s_usable = 0; s_supported = 0; }
    __syncthreads();
    ResectKey best = { 0, -1, 0.0 };
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
        const ResectKey k = { cons + kResectSample, h, es / (double)(cons + kResectSample) };
        if (resect_better(k, best)) best = k;
    }
    s_key[tid] = best;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st && resect_better(s_key[tid + st], s_key[tid])) s_key[tid] = s_key[tid + st];
        __syncthreads();
    }
    const ResectKey win = s_key[0];
    if (tid == 0) {
        res->iterations = H; res->usable_models = s_usable; res->supported_models = s_supported;
        res->best_iteration = win.it;
        res->status = win.it >= 0 ? OSFM_RESECT_OK : OSFM_RESECT_NO_MODEL;
        res->ransac_inliers = win.it >= 0 ? win.inl : 0;
        res->num_inliers = 0; res->refit_used = 0; res->mean_error_px = 0.0;
    }
    if (win.it < 0) {
        if (tid < 9) res->rotation[tid] = tid % 4 == 0 ? 1.0 : 0.0;
        if (tid == 9) res->scale = scale;
        if (tid == 10 || tid == 11) res->offsets[tid - 10] = 0.0;
        return;
    }
    const size_t h = (size_t)win.it;
    if (tid < kResectTable) res->table[tid] = tables[h * kResectTable + tid];
    if (tid < kResectSample) res->sample[tid] = samples[h * kResectSample + tid];
}

// member of the winner's inlier set: below the threshold under its table, or one of its sample
__device__ __forceinline__ bool resect_member(const double *tbl, const int32_t *smp, int t, int N, double X, double Y, double Z,
    double u, double v, double half_w, double half_h, double thr)
{
    if (t >= N) return false;
    bool m = resect_error(tbl, X, Y, Z, u, v, half_w, half_h) < thr;
#pragma unroll
    for (int k = 0; k < kResectSample; ++k) m = m || smp[k] == t;
    return m;
}

// ---- the refit over the winner's inliers, pass 1: their number and the sums of X, Y, Z, u, v per tile ----
__global__ __launch_bounds__(kResectTile) void resect_refit_sums_kernel(const ResectDeviceResult *__restrict__ res,
    const double *__restrict__ data, int N, double half_w, double half_h, double thr, int32_t *__restrict__ part_n,
    double *__restrict__ part_sum)
{
    if (res->status != OSFM_RESECT_OK) return;
    __shared__ double s_tbl[kResectTable];
    __shared__ int32_t s_smp[kResectSample];
    __shared__ double s_w[5][4];
    __shared__ int32_t s_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kResectTable) s_tbl[tid] = res->table[tid];
    if (tid < kResectSample) s_smp[tid] = res->sample[tid];
    const int t = blockIdx.x * kResectTile + tid;
    const bool in = t < N;
    double d[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) d[r] = in ? data[(size_t)r * N + t] : 0.0;
    __syncthreads();
    const bool m = resect_member(s_tbl, s_smp, t, N, d[0], d[1], d[2], d[3], d[4], half_w, half_h, thr);
    const unsigned long long bal = __ballot(m);
    if (lane == 0) s_n[wave] = __popcll(bal);
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const double w = resect_wave_sum(m ? d[r] : 0.0);
        if (lane == 0) s_w[r][wave] = w;
    }
    __syncthreads();
    if (tid < 5) part_sum[(size_t)blockIdx.x * 5 + tid] = ((s_w[tid][0] + s_w[tid][1]) + s_w[tid][2]) + s_w[tid][3];
    if (tid == 5) part_n[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// ---- pass 2: the sums centred on the centroid: xx xy xz yy yz zz, xu yu zu, xv yv zv per tile ----
__global__ __launch_bounds__(kResectTile) void resect_refit_cov_kernel(const ResectDeviceResult *__restrict__ res,
    const double *__restrict__ data, int N, int tiles, double half_w, double half_h, double thr,
    const int32_t *__restrict__ part_n, const double *__restrict__ part_sum, double *__restrict__ part_cov)
{
    if (res->status != OSFM_RESECT_OK) return;
    __shared__ double s_tbl[kResectTable];
    __shared__ int32_t s_smp[kResectSample];
    __shared__ double s_mean[5];
    __shared__ double s_w[12][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kResectTable) s_tbl[tid] = res->table[tid];
    if (tid < kResectSample) s_smp[tid] = res->sample[tid];
    if (tid >= 64 && tid < 69) {
        const int r = tid - 64;
        int n = 0;
        double m = 0.0;
        for (int b = 0; b < tiles; ++b) { n += part_n[b]; m += part_sum[(size_t)b * 5 + r]; }
        s_mean[r] = m / (double)n;
    }
    const int t = blockIdx.x * kResectTile + tid;
    const bool in = t < N;
    double d[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) d[r] = in ? data[(size_t)r * N + t] : 0.0;
    __syncthreads();
    const bool m = resect_member(s_tbl, s_smp, t, N, d[0], d[1], d[2], d[3], d[4], half_w, half_h, thr);
#pragma unroll
    for (int r = 0; r < 5; ++r) d[r] = m ? d[r] - s_mean[r] : 0.0;
    const double prod[12] = { d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2],
                              d[0] * d[3], d[1] * d[3], d[2] * d[3], d[0] * d[4], d[1] * d[4], d[2] * d[4] };
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const double w = resect_wave_sum(prod[e]);
        if (lane == 0) s_w[e][wave] = w;
    }
    __syncthreads();
    if (tid < 12) part_cov[(size_t)blockIdx.x * 12 + tid] = ((s_w[tid][0] + s_w[tid][1]) + s_w[tid][2]) + s_w[tid][3];
}

// Cov x = r for the SPD 3 x 3 Cov (xx xy xz yy yz zz) and two right-hand sides, by Cholesky.  false: a pivot is not
// above min_pivot times the largest diagonal entry.
__device__ bool resect_spd_solve(const double *c, const double *ru, const double *rv, double min_pivot, double *a, double *b)
{
    const double big = fmax(c[0], fmax(c[3], c[5]));
    if (!(big > 0.0) || !isfinite(big)) return false;
    const double least = min_pivot * big;
    if (!(c[0] >= least)) return false;
    const double l00 = sqrt(c[0]), l10 = c[1] / l00, l20 = c[2] / l00;
    const double d1 = c[3] - l10 * l10;
    if (!(d1 >= least)) return false;
    const double l11 = sqrt(d1), l21 = (c[4] - l20 * l10) / l11;
    const double d2 = (c[5] - l20 * l20) - l21 * l21;
    if (!(d2 >= least)) return false;
    const double l22 = sqrt(d2);
    for (int k = 0; k < 2; ++k) {
        const double *r = k ? rv : ru;
        double *x = k ? b : a;
        const double y0 = r[0] / l00, y1 = (r[1] - l10 * y0) / l11, y2 = ((r[2] - l20 * y0) - l21 * y1) / l22;
        x[2] = y2 / l22;
        x[1] = (y1 - l21 * x[2]) / l11;
        x[0] = ((y0 - l10 * x[1]) - l20 * x[2]) / l00;
    }
    return true;
}

// ---- one lane: the refit's solve, the projection onto the camera model, the final camera ----
__global__ __launch_bounds__(64) void resect_model_kernel(ResectDeviceResult *__restrict__ res, int tiles, double min_pivot,
    int estimate_scale, double fixed_scale, const int32_t *__restrict__ part_n, const double *__restrict__ part_sum,
    const double *__restrict__ part_cov)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || res->status != OSFM_RESECT_OK) return;
    int n = 0;
    double mean[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 }, cov[12];
    for (int e = 0; e < 12; ++e) cov[e] = 0.0;
    for (int t = 0; t < tiles; ++t) {
        n += part_n[t];
        for (int r = 0; r < 5; ++r) mean[r] += part_sum[(size_t)t * 5 + r];
        for (int e = 0; e < 12; ++e) cov[e] += part_cov[(size_t)t * 12 + e];
    }
    for (int r = 0; r < 5; ++r) mean[r] /= (double)n;
    double a[3], b[3];
    double g00, g01, g11, l1, l2;
    bool refit = resect_spd_solve(cov, cov + 6, cov + 9, min_pivot, a, b);
    if (refit) {
        const double ra[3] = { a[0], a[1], a[2] }, rb[3] = { b[0], b[1], b[2] };
        refit = resect_axes(ra, rb, &g00, &g01, &g11, &l1, &l2);
    }
    if (!refit) {
        // the winner's own matrix (it passed the axis-ratio test)
        for (int i = 0; i < 3; ++i) { a[i] = res->table[i]; b[i] = res->table[4 + i]; }
        const double ra[3] = { a[0], a[1], a[2] }, rb[3] = { b[0], b[1], b[2] };
        resect_axes(ra, rb, &g00, &g01, &g11, &l1, &l2);
    }
    // Q = G^(-1/2) A: sqrt(G) = (G + sqrt(det G) I) / sqrt(tr G + 2 sqrt(det G)), inverted in closed form
    const double sd = sqrt(l1) * sqrt(l2);                 // sigma_1 sigma_2
    const double st = sqrt(l1) + sqrt(l2);                 // sigma_1 + sigma_2
    const double q00 = (g11 + sd) / (st * sd), q01 = -g01 / (st * sd), q11 = (g00 + sd) / (st * sd);
    double x[3], y[3], z[3];
    for (int i = 0; i < 3; ++i) { x[i] = q00 * a[i] + q01 * b[i]; y[i] = q01 * a[i] + q11 * b[i]; }
    z[0] = x[1] * y[2] - x[2] * y[1];
    z[1] = x[2] * y[0] - x[0] * y[2];
    z[2] = x[0] * y[1] - x[1] * y[0];
    const double s = estimate_scale ? 2.0 / st : fixed_scale;
    const double ox = ((x[0] * mean[0] + x[1] * mean[1]) + x[2] * mean[2]) / s - mean[3];
    const double oy = ((y[0] * mean[0] + y[1] * mean[1]) + y[2] * mean[2]) / s - mean[4];
    for (int i = 0; i < 3; ++i) { res->rotation[3 * i] = x[i]; res->rotation[3 * i + 1] = y[i]; res->rotation[3 * i + 2] = z[i]; }
    res->scale = s; res->offsets[0] = ox; res->offsets[1] = oy;
    res->refit_used = refit ? 1 : 0;
    for (int i = 0; i < 3; ++i) { res->final_table[i] = x[i] / s; res->final_table[4 + i] = y[i] / s; }
    res->final_table[3] = -ox; res->final_table[7] = -oy;
}

// ---- all points once more under the final camera: the inlier bytes, count and error sum per tile ----
__global__ __launch_bounds__(kResectTile) void resect_mask_kernel(const ResectDeviceResult *__restrict__ res,
    const double *__restrict__ data, int N, double half_w, double half_h, double thr, uint8_t *__restrict__ inlier,
    int32_t *__restrict__ part_cnt, double *__restrict__ part_err)
{
    __shared__ double s_tbl[kResectTable];
    __shared__ double s_err[4];
    __shared__ int32_t s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x * kResectTile + tid;
    const bool in = t < N;
    if (res->status != OSFM_RESECT_OK) {
        if (in) inlier[t] = 0;
        if (tid == 0) { part_cnt[blockIdx.x] = 0; part_err[blockIdx.x] = 0.0; }
        return;
    }
    if (tid < kResectTable) s_tbl[tid] = res->final_table[tid];
    double d[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) d[r] = in ? data[(size_t)r * N + t] : 0.0;
    __syncthreads();
    const double e = resect_error(s_tbl, d[0], d[1], d[2], d[3], d[4], half_w, half_h);
    const bool pass = in && e < thr;
    if (in) inlier[t] = pass ? 1 : 0;
    const unsigned long long bal = __ballot(pass);
    const double w = resect_wave_sum(pass ? e : 0.0);
    if (lane == 0) { s_err[wave] = w; s_cnt[wave] = __popcll(bal); }
    __syncthreads();
    if (tid == 0) {
        part_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        part_err[blockIdx.x] = ((s_err[0] + s_err[1]) + s_err[2]) + s_err[3];
    }
}

__global__ void resect_finish_kernel(ResectDeviceResult *__restrict__ res, int tiles, const int32_t *__restrict__ part_cnt,
    const double *__restrict__ part_err)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || res->status != OSFM_RESECT_OK) return;
    int cnt = 0;
    double es = 0.0;
    for (int b = 0; b < tiles; ++b) { cnt += part_cnt[b]; es += part_err[b]; }
    res->num_inliers = cnt;
    res->mean_error_px = cnt > 0 ? es / (double)cnt : 0.0;
}

__global__ void resect_pack_kernel(const double *__restrict__ points, const double *__restrict__ xy, int N, int W, int H,
    double *__restrict__ data)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    for (int r = 0; r < 3; ++r) data[(size_t)r * N + t] = points[(size_t)t * 3 + r];
    data[3 * (size_t)N + t] = tk_normalise(xy[(size_t)t * 2], W);
    data[4 * (size_t)N + t] = tk_normalise(xy[(size_t)t * 2 + 1], H);
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

void identity_outputs(const osfm_resect_options &o, double *rotation, double *scale, double *offsets, uint8_t *inlier, int n_inlier)
{
    for (int e = 0; e < 9; ++e) rotation[e] = e % 4 == 0 ? 1.0 : 0.0;
    *scale = o.scale;
    offsets[0] = offsets[1] = 0.0;
    if (inlier && n_inlier > 0) memset(inlier, 0, (size_t)n_inlier);
}

}  // namespace

int resect_check_options(const osfm_resect_options *opts, osfm_resect_options *out, int *iterations)
{
    if (opts) *out = *opts; else osfm_resect_options_default(out);
    if (!(out->probability > 0.0 && out->probability < 1.0) || !(out->inlier_ratio > 0.0 && out->inlier_ratio < 1.0) ||
        !(out->max_error_px > 0.0) || !std::isfinite(out->max_error_px) || out->min_consensus < 0 || out->max_iterations < 0 ||
        out->max_iterations > kResectMaxIterations || !(out->min_pivot > 0.0 && out->min_pivot < 1.0) ||
        !(out->min_axis_ratio >= 0.0 && out->min_axis_ratio <= 1.0) || !(out->scale > 0.0) || !std::isfinite(out->scale)) {
        set_error("resect: bad options"); return OSFM_E_ARG;
    }
    int H = out->max_iterations;
    if (H == 0) {
        // a quotient below one means that one sample already reaches the probability, not that none is needed
        const double h = floor(log(1.0 - out->probability) / log(1.0 - pow(out->inlier_ratio, (double)kResectSample)));
        H = !(h >= 1.0) ? 1 : (h > (double)kResectMaxIterations ? kResectMaxIterations : (int)h);
    }
    *iterations = H;
    return OSFM_OK;
}

void launch_resect_pack(const double *points, const double *xy, int N, int W, int H, double *data, hipStream_t s)
{
    if (N <= 0) return;
    hipLaunchKernelGGL(resect_pack_kernel, dim3((N + 255) / 256), dim3(256), 0, s, points, xy, N, W, H, data);
}

int resect_core(const double *data, int N, int W, int H, const osfm_resect_options &o, int iterations, uint64_t stream_id,
    hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b, double *rotation, double *scale, double *offsets, uint8_t *inlier,
    int inlier_capacity, osfm_resect_result *result)
{
    memset(result, 0, sizeof(*result));
    result->best_iteration = -1;
    const int n_inlier = inlier ? std::min(N, std::max(inlier_capacity, 0)) : 0;
    if (resect_too_few(N, o)) {
        result->status = OSFM_RESECT_TOO_FEW;
        identity_outputs(o, rotation, scale, offsets, inlier, n_inlier);
        return OSFM_OK;
    }
    const int Hn = iterations, tiles = (N + kResectTile - 1) / kResectTile, chunks = (Hn + kResectChunk - 1) / kResectChunk;
    // one block of device memory, carved up
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o0 = at; at += align16(bytes); return o0; };
    const size_t o_res = carve(sizeof(ResectDeviceResult) + (size_t)N);
    const size_t o_valid = carve((size_t)Hn * 4), o_fcnt = carve((size_t)Hn * 4), o_ferr = carve((size_t)Hn * 8);
    const size_t o_samp = carve((size_t)Hn * kResectSample * 4), o_tables = carve((size_t)Hn * kResectTable * 8);
    const size_t o_pcnt = carve((size_t)tiles * Hn * 4), o_perr = carve((size_t)tiles * Hn * 8);
    const size_t o_rn = carve((size_t)tiles * 4), o_rsum = carve((size_t)tiles * 5 * 8), o_rcov = carve((size_t)tiles * 12 * 8);
    const size_t o_mcnt = carve((size_t)tiles * 4), o_merr = carve((size_t)tiles * 8);
    DevArray block;
    OSFM_RETURN_IF(block.alloc(at));
    char *base = block.as<char>();
    ResectDeviceResult *res = reinterpret_cast<ResectDeviceResult *>(base + o_res);
    uint8_t *d_inlier = reinterpret_cast<uint8_t *>(base + o_res + sizeof(ResectDeviceResult));
    int32_t *valid = reinterpret_cast<int32_t *>(base + o_valid), *fcnt = reinterpret_cast<int32_t *>(base + o_fcnt);
    double *ferr = reinterpret_cast<double *>(base + o_ferr);
    int32_t *samp = reinterpret_cast<int32_t *>(base + o_samp);
    double *tables = reinterpret_cast<double *>(base + o_tables);
    int32_t *pcnt = reinterpret_cast<int32_t *>(base + o_pcnt);
    double *perr = reinterpret_cast<double *>(base + o_perr);
    int32_t *rn = reinterpret_cast<int32_t *>(base + o_rn);
    double *rsum = reinterpret_cast<double *>(base + o_rsum), *rcov = reinterpret_cast<double *>(base + o_rcov);
    int32_t *mcnt = reinterpret_cast<int32_t *>(base + o_mcnt);
    double *merr = reinterpret_cast<double *>(base + o_merr);
    const double half_w = 0.5 * (double)W, half_h = 0.5 * (double)H, thr = o.max_error_px;

    hipLaunchKernelGGL(resect_hypothesis_kernel, dim3((Hn + 63) / 64), dim3(64), 0, s, data, N, Hn, (uint64_t)o.seed, stream_id,
        half_w, half_h, thr, o.min_pivot, o.min_axis_ratio, valid, fcnt, ferr, samp, tables);
    OSFM_HIP_CHECK(hipEventRecord(ev_a, s));
    hipLaunchKernelGGL(resect_score_kernel, dim3(tiles, chunks), dim3(kResectTile), 0, s, data, N, Hn, tables, valid, half_w, half_h,
        thr, pcnt, perr);
    OSFM_HIP_CHECK(hipEventRecord(ev_b, s));
    hipLaunchKernelGGL(resect_select_kernel, dim3(1), dim3(256), 0, s, Hn, tiles, (int)o.min_consensus, o.scale, valid, fcnt, ferr,
        pcnt, perr, samp, tables, res);
    // (these return at once when the selection found no supported hypothesis)
    hipLaunchKernelGGL(resect_refit_sums_kernel, dim3(tiles), dim3(kResectTile), 0, s, res, data, N, half_w, half_h, thr, rn, rsum);
    hipLaunchKernelGGL(resect_refit_cov_kernel, dim3(tiles), dim3(kResectTile), 0, s, res, data, N, tiles, half_w, half_h, thr, rn,
        rsum, rcov);
    hipLaunchKernelGGL(resect_model_kernel, dim3(1), dim3(64), 0, s, res, tiles, o.min_pivot, (int)o.estimate_scale, o.scale, rn, rsum,
        rcov);
    hipLaunchKernelGGL(resect_mask_kernel, dim3(tiles), dim3(kResectTile), 0, s, res, data, N, half_w, half_h, thr, d_inlier, mcnt, merr);
    hipLaunchKernelGGL(resect_finish_kernel, dim3(1), dim3(64), 0, s, res, tiles, mcnt, merr);
    OSFM_HIP_CHECK(hipGetLastError());
    // the one read-back: the result block up to its offsets, and the inlier bytes behind it
    std::vector<char> host(sizeof(ResectDeviceResult) + (size_t)N);
    OSFM_HIP_CHECK(hipMemcpyAsync(host.data(), res, host.size(), hipMemcpyDeviceToHost, s));
    OSFM_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.0f;
    OSFM_HIP_CHECK(hipEventElapsedTime(&ms, ev_a, ev_b));
    const ResectDeviceResult *r = reinterpret_cast<const ResectDeviceResult *>(host.data());
    result->status = r->status; result->iterations = r->iterations; result->usable_models = r->usable_models;
    result->supported_models = r->supported_models; result->best_iteration = r->best_iteration;
    result->ransac_inliers = r->ransac_inliers; result->num_inliers = r->num_inliers; result->refit_used = r->refit_used;
    result->mean_error_px = r->mean_error_px; result->score_kernel_ms = ms;
    for (int e = 0; e < 9; ++e) rotation[e] = r->rotation[e];
    *scale = r->scale;
    offsets[0] = r->offsets[0]; offsets[1] = r->offsets[1];
    if (n_inlier > 0) memcpy(inlier, host.data() + sizeof(ResectDeviceResult), (size_t)n_inlier);
    return OSFM_OK;
}

}  // namespace osfm

using namespace osfm;

int osfm_resect_options_default(osfm_resect_options *o)
{
    if (!o) { set_error("resect_options_default: null"); return OSFM_E_ARG; }
    o->max_iterations = 0; o->min_consensus = 8; o->probability = 0.999; o->inlier_ratio = 0.5; o->max_error_px = 3.0;
    o->min_pivot = 1e-6; o->min_axis_ratio = 0.5; o->estimate_scale = 0; o->device = 0; o->scale = 1.0; o->seed = 0;
    return OSFM_OK;
}

int osfm_resect_limits(int32_t *tile, int32_t *chunk)
{
    if (tile) *tile = kResectTile;
    if (chunk) *chunk = kResectChunk;
    return OSFM_OK;
}

int osfm_resect_view(const double *points, const double *xy, int32_t n, int32_t img_width, int32_t img_height,
    const osfm_resect_options *opts, uint64_t stream_id, double *rotation, double *scale, double *offsets, uint8_t *inlier,
    osfm_resect_result *result)
{
    if (!points || !xy || n < 0 || img_width <= 0 || img_height <= 0 || !rotation || !scale || !offsets || !result) {
        set_error("resect_view: bad arguments"); return OSFM_E_ARG;
    }
    osfm_resect_options o;
    int iterations = 0;
    OSFM_RETURN_IF(resect_check_options(opts, &o, &iterations));
    OSFM_RETURN_IF(select_device(o.device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DevArray d_points, d_xy, d_data;
    if (!resect_too_few(n, o)) {
        OSFM_RETURN_IF(upload(d_points, points, (size_t)n * 3, sg.s));
        OSFM_RETURN_IF(upload(d_xy, xy, (size_t)n * 2, sg.s));
        OSFM_RETURN_IF(d_data.alloc((size_t)n * 5 * 8));
        launch_resect_pack(d_points.as<double>(), d_xy.as<double>(), n, img_width, img_height, d_data.as<double>(), sg.s);
    }
    return resect_core(d_data.as<double>(), n, img_width, img_height, o, iterations, stream_id, sg.s, sg.ev[0].a, sg.ev[0].b,
        rotation, scale, offsets, inlier, n, result);
}
