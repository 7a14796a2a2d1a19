// Kernel of the slanted-plane refinement (dense_refine_kernels.h; DESIGN.md "Slanted-plane refinement").
//
// dense_refine_kernel: 16 lanes own a pixel, four pixels share a wave, and the 16 pixels of a workgroup are a 4 x 4
// block of the image, so that their windows and their footprints in a source overlap in the caches.  Lane l of a pixel
// takes the samples k = l, l + 16, ... of the (2 radius + 1)^2 window in row-major order of the offsets u.  A pixel's
// state is the same in all its lanes: every branch is taken by all 16 of them or by none, and the shuffles stay inside
// the 16.  The waves of a workgroup never meet: there is no barrier and no LDS.
//
// One evaluation of a source is one pass over the window for 18 sums that do not depend on gain and bias; everything
// after the fold is closed form, computed by every lane alike.  What a source's back-substitution needs is kept by
// lane s (and s + 8) of the pixel, so the registers do not grow with the number of sources.
//
// Sums: a lane adds its samples in ascending k, then the 16 partial sums are folded by the butterfly 8, 4, 2, 1.
// a + b == b + a to the bit, so every lane ends with the same value and the order is that of folding the upper half
// of the lanes onto the lower half -- which is how tests/dense_refine_restatement.py adds.  The build has
// -ffp-contract=off.  Every loop has a fixed bound; a wave leaves the iterations when none of its pixels runs.
#include "dense_refine_kernels.h"

namespace osfm {
namespace dense {
namespace {

enum { kSW = 0, kSWW, kSWT, kA00, kA01, kA02, kA11, kA12, kA22, kP0, kP1, kP2, kQ0, kQ1, kQ2, kU0, kU1, kU2, kNumSums };

__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int m = kRefineLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kRefineLanes);
    return v;
}

__device__ inline bool group_any(bool b)
{
    int v = b ? 1 : 0;
#pragma unroll
    for (int m = kRefineLanes / 2; m >= 1; m >>= 1) v |= __shfl_xor(v, m, kRefineLanes);
    return v != 0;
}

// One evaluation of source S for the pixel (x, y) with depth z and tilt (zx, zy): this lane's samples, then the fold.
// False: a sample lies outside the source (the sums then mean nothing).
__device__ inline bool source_pass(const Source &S, const float *__restrict__ ref, int w, int x, int y, double z, double zx, double zy,
    int R, int l, double *sums)
{
    const int side = 2 * R + 1, N = side * side;
    const double m00 = S.G[0][0] + S.e[0] * zx, m01 = S.G[0][1] + S.e[0] * zy;
    const double m10 = S.G[1][0] + S.e[1] * zx, m11 = S.G[1][1] + S.e[1] * zy;
    const double cx = (S.G[0][0] * (double)x + S.G[0][1] * (double)y) + (S.g[0] + z * S.e[0]);
    const double cy = (S.G[1][0] * (double)x + S.G[1][1] * (double)y) + (S.g[1] + z * S.e[1]);
    const double xmax = (double)(S.w - 1), ymax = (double)(S.h - 1);
    double acc[kNumSums];
#pragma unroll
    for (int i = 0; i < kNumSums; ++i) acc[i] = 0.0;
    bool out = false;
    for (int k = l; k < N; k += kRefineLanes) {
        const int iux = k % side - R, iuy = k / side - R;
        const double ux = (double)iux, uy = (double)iuy;
        const double sx = cx + (m00 * ux + m01 * uy), sy = cy + (m10 * ux + m11 * uy);
        if (!(sx >= 0.0 && sx <= xmax && sy >= 0.0 && sy <= ymax)) { out = true; continue; }      // a NaN too
        // the bilinear interpolant and its derivative: a point on the last column (row) is interpolated in the cell to
        // its left (above) with weight 1, so that no pixel beyond the image is read
        int x0 = (int)floor(sx), y0 = (int)floor(sy);
        x0 = min(x0, max(S.w - 2, 0));
        y0 = min(y0, max(S.h - 2, 0));
        const int x1 = min(x0 + 1, S.w - 1), y1 = min(y0 + 1, S.h - 1);
        const double fx = sx - (double)x0, fy = sy - (double)y0;
        const float *r0 = S.px + (size_t)y0 * (size_t)S.w, *r1 = S.px + (size_t)y1 * (size_t)S.w;
        const double i00 = (double)r0[x0], i01 = (double)r0[x1], i10 = (double)r1[x0], i11 = (double)r1[x1];
        const double top = (1.0 - fx) * i00 + fx * i01, bot = (1.0 - fx) * i10 + fx * i11;
        const double W = (1.0 - fy) * top + fy * bot;
        const double gx = (1.0 - fy) * (i01 - i00) + fy * (i11 - i10);
        const double gy = (1.0 - fx) * (i10 - i00) + fx * (i11 - i01);
        const double T = (double)ref[(size_t)(y + iuy) * (size_t)w + (size_t)(x + iux)];
        const double a0 = gx * S.e[0] + gy * S.e[1];
        const double a1 = a0 * ux, a2 = a0 * uy;
        acc[kSW] += W; acc[kSWW] += W * W; acc[kSWT] += W * T;
        acc[kA00] += a0 * a0; acc[kA01] += a0 * a1; acc[kA02] += a0 * a2;
        acc[kA11] += a1 * a1; acc[kA12] += a1 * a2; acc[kA22] += a2 * a2;
        acc[kP0] += a0 * W; acc[kP1] += a1 * W; acc[kP2] += a2 * W;
        acc[kQ0] += a0; acc[kQ1] += a1; acc[kQ2] += a2;
        acc[kU0] += a0 * T; acc[kU1] += a1 * T; acc[kU2] += a2 * T;
    }
#pragma unroll
    for (int i = 0; i < kNumSums; ++i) sums[i] = group_sum(acc[i]);
    return !group_any(out);
}

// the zero-mean normalised correlation of W and T from their sums
__device__ inline double zncc(const double *S, double N, double sT, double sTT)
{
    const double cov = S[kSWT] - S[kSW] * sT / N;
    const double var_w = S[kSWW] - S[kSW] * S[kSW] / N;
    const double var_t = sTT - sT * sT / N;
    const double den = sqrt(var_t * var_w);
    return den > 0.0 ? cov / den : 0.0;
}

// Cholesky of the diagonally scaled 3 x 3 matrix H (upper triangle: 00 01 02 11 12 22) and the step for rhs.  False
// (ill conditioned): a diagonal entry that is not positive, or a pivot below min_pivot.
__device__ inline bool solve3(const double *Hu, const double *rhs, double min_pivot, double *delta)
{
    double H[3][3] = {{Hu[0], Hu[1], Hu[2]}, {Hu[1], Hu[3], Hu[4]}, {Hu[2], Hu[4], Hu[5]}};
    if (!(H[0][0] > 0.0 && H[1][1] > 0.0 && H[2][2] > 0.0)) return false;
    double d[3], L[3][3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = 1.0 / sqrt(H[i][i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = (H[j][j] * d[j]) * d[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s >= min_pivot)) ok = false;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 3; ++i) {
            double t = (H[i][j] * d[i]) * d[j];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    if (!ok) return false;
    double yv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double t = rhs[i] * d[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t = t - L[i][k] * yv[k];
        yv[i] = t / L[i][i];
    }
    double zv[3];
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        double t = yv[i];
#pragma unroll
        for (int k = i + 1; k < 3; ++k) t = t - L[k][i] * zv[k];
        zv[i] = t / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) delta[i] = zv[i] * d[i];
    return true;
}

__global__ __launch_bounds__(kRefineThreads) void dense_refine_kernel(RefineArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l = lane & (kRefineLanes - 1), mine = l & (kMaxSources - 1);
    const int x = (int)blockIdx.x * kRefineBlock + (lane >> 4), y = (int)blockIdx.y * kRefineBlock + wave;
    const bool in_image = x < a.w && y < a.h;
    const size_t pix = in_image ? (size_t)y * (size_t)a.w + (size_t)x : 0;
    const int R = a.radius, side = 2 * R + 1, NN = side * side;
    const double N = (double)NN;

    int status = OSFM_DENSE_REFINE_NOT_OK;
    bool run = in_image && a.status[pix] == OSFM_DENSE_OK;
    const double z0 = run ? a.depth[pix] : 0.0;
    double z = z0, zx = 0.0, zy = 0.0;
    double sT = 0.0, sTT = 0.0, score0 = 0.0, score1 = 0.0;
    int frozen = 0, iterations = 0, passes = 0;
    bool converged = false;
    // of this lane's source, the one with index `mine`: gain, bias and what its back-substitution needs
    double my_gain = 1.0, my_bias = 0.0, my_sW = 0.0, my_sWW = 0.0, my_det = 1.0, my_D[3][2] = {}, my_rc[2] = {};

    if (run) {
        // the template: its window inside the reference image, its sums
        if (x - R < 0 || x + R > a.w - 1 || y - R < 0 || y + R > a.h - 1) {
            status = OSFM_DENSE_REFINE_OUTSIDE;
            run = false;
        } else {
            double s1 = 0.0, s2 = 0.0;
            for (int k = l; k < NN; k += kRefineLanes) {
                const double T = (double)a.ref[(size_t)(y + k / side - R) * (size_t)a.w + (size_t)(x + k % side - R)];
                s1 += T;
                s2 += T * T;
            }
            sT = group_sum(s1);
            sTT = group_sum(s2);
        }
    }

    for (int it = 0; it < a.max_iterations; ++it) {
        if (!__any(run && !converged)) break;
        if (run && !converged) {
        double Ht[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rt[3] = {0.0, 0.0, 0.0};
        bool outside = false, ill = false;
        int count = 0;
        double total = 0.0;
        for (int s = 0; s < a.num_sources; ++s) {
            if (it > 0 && !((frozen >> s) & 1)) continue;
            double S[kNumSums];
            const bool inside = source_pass(a.src[s], a.ref, a.w, x, y, z, zx, zy, R, l, S);
            ++passes;
            if (it == 0) {
                if (!inside) continue;
                frozen |= 1 << s;
            } else if (!inside) {
                outside = true;
                continue;
            }
            const double det = S[kSWW] * N - S[kSW] * S[kSW];
            if (!(det > kRefineBlockEps * (S[kSWW] * N))) ill = true;
            double gain, bias;
            if (it == 0) {
                gain = (S[kSWT] * N - S[kSW] * sT) / det;
                bias = (S[kSWW] * sT - S[kSW] * S[kSWT]) / det;
                total = total + zncc(S, N, sT, sTT);
            } else {
                gain = __shfl(my_gain, s, kRefineLanes);
                bias = __shfl(my_bias, s, kRefineLanes);
            }
            // the 5 x 5 normal equations of (gain a m, W, 1) with the block of gain and bias eliminated
            const double D[3][2] = {{gain * S[kP0], gain * S[kQ0]}, {gain * S[kP1], gain * S[kQ1]}, {gain * S[kP2], gain * S[kQ2]}};
            const double rc0 = (gain * S[kSWW] + bias * S[kSW]) - S[kSWT], rc1 = (gain * S[kSW] + bias * N) - sT;
            double E[3][2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                E[i][0] = (D[i][0] * N - D[i][1] * S[kSW]) / det;
                E[i][1] = (D[i][1] * S[kSWW] - D[i][0] * S[kSW]) / det;
            }
            const double gg = gain * gain;
            Ht[0] = Ht[0] + (gg * S[kA00] - (E[0][0] * D[0][0] + E[0][1] * D[0][1]));
            Ht[1] = Ht[1] + (gg * S[kA01] - (E[0][0] * D[1][0] + E[0][1] * D[1][1]));
            Ht[2] = Ht[2] + (gg * S[kA02] - (E[0][0] * D[2][0] + E[0][1] * D[2][1]));
            Ht[3] = Ht[3] + (gg * S[kA11] - (E[1][0] * D[1][0] + E[1][1] * D[1][1]));
            Ht[4] = Ht[4] + (gg * S[kA12] - (E[1][0] * D[2][0] + E[1][1] * D[2][1]));
            Ht[5] = Ht[5] + (gg * S[kA22] - (E[2][0] * D[2][0] + E[2][1] * D[2][1]));
            rt[0] = rt[0] + (gain * ((gain * S[kP0] + bias * S[kQ0]) - S[kU0]) - (E[0][0] * rc0 + E[0][1] * rc1));
            rt[1] = rt[1] + (gain * ((gain * S[kP1] + bias * S[kQ1]) - S[kU1]) - (E[1][0] * rc0 + E[1][1] * rc1));
            rt[2] = rt[2] + (gain * ((gain * S[kP2] + bias * S[kQ2]) - S[kU2]) - (E[2][0] * rc0 + E[2][1] * rc1));
            ++count;
            if (mine == s) {
                my_gain = gain; my_bias = bias; my_sW = S[kSW]; my_sWW = S[kSWW]; my_det = det;
#pragma unroll
                for (int i = 0; i < 3; ++i) { my_D[i][0] = D[i][0]; my_D[i][1] = D[i][1]; }
                my_rc[0] = rc0; my_rc[1] = rc1;
            }
        }
        const double rhs[3] = {-rt[0], -rt[1], -rt[2]};
        double delta[3];
        if (outside || count < a.min_sources) {
            status = OSFM_DENSE_REFINE_OUTSIDE;
            run = false;
        } else if (ill || !solve3(Ht, rhs, a.min_pivot, delta)) {
            status = OSFM_DENSE_REFINE_ILL_CONDITIONED;
            run = false;
        } else {
            if (it == 0) score0 = total / (double)count;
            z = z + delta[0]; zx = zx + delta[1]; zy = zy + delta[2];
            const double t0 = my_rc[0] + ((my_D[0][0] * delta[0] + my_D[1][0] * delta[1]) + my_D[2][0] * delta[2]);
            const double t1 = my_rc[1] + ((my_D[0][1] * delta[0] + my_D[1][1] * delta[1]) + my_D[2][1] * delta[2]);
            my_gain += -((N * t0 - my_sW * t1) / my_det);
            my_bias += -((my_sWW * t1 - my_sW * t0) / my_det);
            iterations = it + 1;
            const double c0 = fabs(delta[0]), c1 = (double)R * (fabs(delta[1]) + fabs(delta[2]));
            converged = c0 <= a.converged && c1 <= a.converged;
        }
        }
    }

    if (run) {
        // behind the loop: the final windows and their scores, then the tests in their order
        bool outside = false;
        int count = 0;
        double total = 0.0;
        for (int s = 0; s < a.num_sources; ++s) {
            if (!((frozen >> s) & 1)) continue;
            double S[kNumSums];
            const bool inside = source_pass(a.src[s], a.ref, a.w, x, y, z, zx, zy, R, l, S);
            ++passes;
            if (!inside) { outside = true; continue; }
            total = total + zncc(S, N, sT, sTT);
            ++count;
        }
        score1 = total / (double)max(count, 1);
        bool slope = false;
        const double lo = 1.0 / a.max_deform, hi = a.max_deform;
        for (int s = 0; s < a.num_sources; ++s) {
            if (!((frozen >> s) & 1)) continue;
            const Source &S = a.src[s];
            const double m00 = S.G[0][0] + S.e[0] * zx, m01 = S.G[0][1] + S.e[0] * zy;
            const double m10 = S.G[1][0] + S.e[1] * zx, m11 = S.G[1][1] + S.e[1] * zy;
            // singular values of M: (E, H) and (F, G) are its rotation and its reflection part
            const double E = 0.5 * (m00 + m11), F = 0.5 * (m00 - m11), G = 0.5 * (m10 + m01), H = 0.5 * (m10 - m01);
            const double Q = sqrt(E * E + H * H), Sg = sqrt(F * F + G * G);
            const double smax = Q + Sg, smin = fabs(Q - Sg);
            if (smax > hi || smin < lo) slope = true;
        }
        if (outside) status = OSFM_DENSE_REFINE_OUTSIDE;
        else if (!converged) status = OSFM_DENSE_REFINE_NOT_CONVERGED;
        else if (fabs(z - z0) / a.dz > a.max_shift) status = OSFM_DENSE_REFINE_REJECT_SHIFT;
        else if (slope) status = OSFM_DENSE_REFINE_REJECT_SLOPE;
        else if (score1 < a.min_score || score1 < score0) status = OSFM_DENSE_REFINE_REJECT_SCORE;
        else status = OSFM_DENSE_REFINE_REFINED;
    }

    if (in_image && l == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double g0 = nan, g1 = nan, n0 = nan, n1 = nan, n2 = nan;
        if (status == OSFM_DENSE_REFINE_REFINED) {
            // cross(b1 + zy d, b0 + zx d) normalised: against the viewing axis, as the meshes' vertex normals
            const double u0 = a.B[0][0] + zx * a.d[0], u1 = a.B[1][0] + zx * a.d[1], u2 = a.B[2][0] + zx * a.d[2];
            const double v0 = a.B[0][1] + zy * a.d[0], v1 = a.B[1][1] + zy * a.d[1], v2 = a.B[2][1] + zy * a.d[2];
            const double c0 = v1 * u2 - v2 * u1, c1 = v2 * u0 - v0 * u2, c2 = v0 * u1 - v1 * u0;
            const double nn = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
            g0 = zx; g1 = zy; n0 = c0 / nn; n1 = c1 / nn; n2 = c2 / nn;
            a.depth[pix] = z;
            a.score[pix] = (float)score1;
        }
        a.rstatus[pix] = (uint8_t)status;
        a.gradient[2 * pix] = g0; a.gradient[2 * pix + 1] = g1;
        a.normal[3 * pix] = n0; a.normal[3 * pix + 1] = n1; a.normal[3 * pix + 2] = n2;
    }
    // the counters: one lane per pixel counts, the wave adds, its first lane books
    long long its = (in_image && l == 0) ? iterations : 0, ps = (in_image && l == 0) ? passes : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        its += __shfl_xor(its, m, 64);
        ps += __shfl_xor(ps, m, 64);
    }
    if (lane == 0 && (its | ps)) {
        unsigned long long *slot = a.counters + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) % kRefineCounterSlots) * kRefineSlotStride;
        atomicAdd(slot, (unsigned long long)its);
        atomicAdd(slot + 1, (unsigned long long)ps);
    }
}

}  // namespace

void launch_refine(hipStream_t s, const RefineArgs &a)
{
    if (a.w <= 0 || a.h <= 0) return;
    const dim3 grid((unsigned)((a.w + kRefineBlock - 1) / kRefineBlock), (unsigned)((a.h + kRefineBlock - 1) / kRefineBlock));
    hipLaunchKernelGGL(dense_refine_kernel, grid, dim3(kRefineThreads), 0, s, a);
}

}  // namespace dense
}  // namespace osfm
