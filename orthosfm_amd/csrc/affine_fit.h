// The affine fundamental matrix as device code shared by the kernels that test against it or fit it: the RANSAC of
// ransac_affine.hip and the guided matcher of guided_kernels.hip.  One operation order throughout (files that include
// this are built without FMA contraction); tests/affine_restatement.py restates it operation for operation.
#pragma once
#include "ransac_pair.h"

namespace osfm {

// One hypothesis as the kernel holds it: v = (a, b, c, d, e), s = a^2 + b^2 + c^2 + d^2 and the two bounds of the
// safe product tests, s times the band's (sampson_below in ransac_kernels.hip has the argument).
struct AffineHyp { double v[5], s, s_lo, s_hi; };

__device__ __forceinline__ void affine_bounds(AffineHyp &h, const RansacBand &band)
{
    h.s = ((h.v[0] * h.v[0] + h.v[1] * h.v[1]) + h.v[2] * h.v[2]) + h.v[3] * h.v[3];
    h.s_lo = h.s * band.thr_lo;
    h.s_hi = h.s * band.thr_hi;
}

// sampson(F_A, x1, y1, x2, y2) < thr2 of ransac_kernels.hip in its own order of operations, with the terms that F_A's
// zeros remove left out: n = (x2 a + y2 b) + ((x1 c + y1 d) + e), the sum of squares is s.
__device__ __forceinline__ bool
affine_below(const AffineHyp &h, double x1, double y1, double x2, double y2, double thr2)
{
    double n = (x2 * h.v[0] + y2 * h.v[1]) + ((x1 * h.v[2] + y1 * h.v[3]) + h.v[4]);
    n *= n;
    if (n < h.s_lo) return true;                     // strict: s == 0 never passes here
    if (n >= h.s_hi) return false;
    return n / h.s < thr2;                           // the sliver, and NaN operands
}

// Eigenvectors of a symmetric 4 x 4 matrix by cyclic Jacobi, eig3_fixed of ransac_kernels.hip with one more row.
__device__ __forceinline__ void eig4_fixed(double (&A)[4][4], double (&V)[4][4], double (&w)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = ((((fabs(A[0][1]) + fabs(A[0][2])) + fabs(A[0][3])) + fabs(A[1][2])) + fabs(A[1][3])) + fabs(A[2][3]);
        if (off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                if (A[p][q] == 0.0) continue;
                const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = A[i][i];
}

// red[q * 256 + tid], q < N, holds a partial sum per thread: the fixed tree that leaves the totals in red[q * 256]
template <int N>
__device__ __forceinline__ void tree_sum(double *red, int tid)
{
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int q = 0; q < N; ++q) red[q * 256 + tid] += red[q * 256 + tid + st];
        }
        __syncthreads();
    }
}

// The least-squares F_A of the matches i < k with in(i), `count` of them (>= 1), by the 256 threads of a workgroup:
// z = (x2, y2, x1, y1), the mean in a first pass, the scatter about it in a second, (a, b, c, d) the scatter's
// eigenvector of the smallest eigenvalue, e = -(a, b, c, d) . mean.  Thread t adds matches t, t + 256, ... in order (a
// match that is not in adds +0), then a fixed tree over the 256 partial sums: the order is a function of k alone.
// red: 2560 doubles of LDS that nothing else reads until the call returns; load(i): the match as (x1, y1, x2, y2).
// Every thread returns the same R.v; its bounds are the caller's to set.
template <class Load, class In>
__device__ __forceinline__ void affine_refit(double *red, int tid, int k, int count, Load load, In in_pred, AffineHyp &R)
{
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
    for (int i = tid; i < k; i += 256) {
        const double4 m = load(i);
        const bool in = in_pred(m);
        z0 += in ? m.z : 0.0; z1 += in ? m.w : 0.0; z2 += in ? m.x : 0.0; z3 += in ? m.y : 0.0;
    }
    __syncthreads();               // whatever the caller kept in red is not read again
    red[0 * 256 + tid] = z0; red[1 * 256 + tid] = z1; red[2 * 256 + tid] = z2; red[3 * 256 + tid] = z3;
    tree_sum<4>(red, tid);
    const double cn = (double)count;
    const double mu0 = red[0] / cn, mu1 = red[256] / cn, mu2 = red[512] / cn, mu3 = red[768] / cn;
    __syncthreads();
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c03 = 0.0, c11 = 0.0, c12 = 0.0, c13 = 0.0, c22 = 0.0, c23 = 0.0, c33 = 0.0;
    for (int i = tid; i < k; i += 256) {
        const double4 m = load(i);
        const bool in = in_pred(m);
        const double d0 = m.z - mu0, d1 = m.w - mu1, d2 = m.x - mu2, d3 = m.y - mu3;
        c00 += in ? d0 * d0 : 0.0; c01 += in ? d0 * d1 : 0.0; c02 += in ? d0 * d2 : 0.0; c03 += in ? d0 * d3 : 0.0;
        c11 += in ? d1 * d1 : 0.0; c12 += in ? d1 * d2 : 0.0; c13 += in ? d1 * d3 : 0.0;
        c22 += in ? d2 * d2 : 0.0; c23 += in ? d2 * d3 : 0.0; c33 += in ? d3 * d3 : 0.0;
    }
    red[0 * 256 + tid] = c00; red[1 * 256 + tid] = c01; red[2 * 256 + tid] = c02; red[3 * 256 + tid] = c03;
    red[4 * 256 + tid] = c11; red[5 * 256 + tid] = c12; red[6 * 256 + tid] = c13;
    red[7 * 256 + tid] = c22; red[8 * 256 + tid] = c23; red[9 * 256 + tid] = c33;
    tree_sum<10>(red, tid);
    // every thread runs the same Jacobi on the same totals
    double C[4][4], V[4][4], w[4];
    C[0][0] = red[0]; C[0][1] = C[1][0] = red[256]; C[0][2] = C[2][0] = red[512]; C[0][3] = C[3][0] = red[768];
    C[1][1] = red[1024]; C[1][2] = C[2][1] = red[1280]; C[1][3] = C[3][1] = red[1536];
    C[2][2] = red[1792]; C[2][3] = C[3][2] = red[2048]; C[3][3] = red[2304];
    eig4_fixed(C, V, w);
    int m = 0;
    if (w[1] < w[m]) m = 1;
    if (w[2] < w[m]) m = 2;
    if (w[3] < w[m]) m = 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) R.v[q] = m == 0 ? V[q][0] : m == 1 ? V[q][1] : m == 2 ? V[q][2] : V[q][3];
    R.v[4] = -(((R.v[0] * mu0 + R.v[1] * mu1) + R.v[2] * mu2) + R.v[3] * mu3);
}

}  // namespace osfm
