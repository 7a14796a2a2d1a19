// Geometric verification of a pair of ORTHOGRAPHIC views on the GPU: RANSAC over affine fundamental matrices
//
//         | 0 0 a |
//   F_A = | 0 0 b |      x2^T F_A x1 = a x2 + b y2 + c x1 + d y1 + e = 0
//         | c d e |
//
// from minimal samples of 4 matches, with the Sampson distance of the 8-point kernel (ransac_kernels.hip) as the
// inlier test -- for F_A its denominator is the constant a^2 + b^2 + c^2 + d^2, so the distance is exact -- and one
// least-squares refit on the winner's inliers.  The reference project has no such estimator (its RansacFundamental
// is the 8-point one); the mode is opt-in (osfm_match_options.ransac_model, osfm_ransac_affine).
//
// The job records, the split of a pair's hypotheses over kRansacSplit workgroups, the tie rule, the election of the
// winner and the inlier list are the scaffold of ransac_pair.h, shared with ransac_kernel; the sample stream is that
// of ransac_rand.h.  All arithmetic is double precision in ONE operation order (this file is built without FMA
// contraction), restated operation for operation in tests/affine_restatement.py, which the kernel equals bit for
// bit.  Everything a thread holds is statically indexed (the elimination, the sample, the 4 x 4 Jacobi are unrolled
// on scalars): no scratch memory.
#include "ransac_affine.h"
#include "affine_fit.h"
#include "ransac_rand.h"
#include "osfm_common.h"

namespace osfm {

using AffineSlot = RansacSlot<5>;

namespace {

__device__ __forceinline__ void swap_if(bool c, double &a, double &b)
{
    const double t = a;
    a = c ? b : a;
    b = c ? t : b;
}

__device__ __forceinline__ void sort2(int &a, int &b)
{
    const int lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}

// Null vector of the 4 x 5 system with rows (x2, y2, x1, y1, 1) by Gauss-Jordan elimination with full pivoting
// (eight_point's scheme: the first largest modulus in row-major order is the pivot), scaled to a^2 + b^2 + c^2 +
// d^2 = 1.  Row and column exchanges are selects over the statically indexed positions.  False, and v zero: a pivot
// that is not > 0, or a = b = c = d = 0.
__device__ __forceinline__ bool four_point(const double (&P)[4][4], double (&v)[5])
{
    double A[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) A[i][j] = P[i][j];
        A[i][4] = 1.0;
    }
    int perm[5] = {0, 1, 2, 3, 4};
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int pr = r, pc = r;
        double best = -1.0;
#pragma unroll
        for (int i = r; i < 4; ++i)
#pragma unroll
            for (int j = r; j < 5; ++j) {
                const double m = fabs(A[i][j]);
                if (m > best) { best = m; pr = i; pc = j; }
            }
        ok = ok && best > 0.0;
        // (columns left of r are not read again in rows r and below)
#pragma unroll
        for (int i = r + 1; i < 4; ++i)
#pragma unroll
            for (int j = r; j < 5; ++j) swap_if(pr == i, A[r][j], A[i][j]);
#pragma unroll
        for (int j = r + 1; j < 5; ++j) {
            const bool c = pc == j;
#pragma unroll
            for (int i = 0; i < 4; ++i) swap_if(c, A[i][r], A[i][j]);
            const int t = perm[r];
            perm[r] = c ? perm[j] : perm[r];
            perm[j] = c ? t : perm[j];
        }
        const double inv = 1.0 / A[r][r];
#pragma unroll
        for (int j = r + 1; j < 5; ++j) A[r][j] *= inv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i == r) continue;
            const double fct = A[i][r];
#pragma unroll
            for (int j = r + 1; j < 5; ++j) A[i][j] -= fct * A[r][j];
        }
    }
    double f[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        f[c] = 1.0;                                  // the free column, perm[4]
#pragma unroll
        for (int r = 0; r < 4; ++r) f[c] = perm[r] == c ? -A[r][4] : f[c];
    }
    const double s = ((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) + f[3] * f[3];
    ok = ok && s > 0.0;
    const double inv = 1.0 / sqrt(s);
#pragma unroll
    for (int c = 0; c < 5; ++c) v[c] = ok ? f[c] * inv : 0.0;
    return ok;
}

}  // namespace

__global__ __launch_bounds__(256) void
ransac_affine_kernel(const RansacJob *__restrict__ jobs, int num_jobs, int max_iterations, double thr2, int refit,
    uint64_t seed, AffineSlot *__restrict__ slots, int32_t *__restrict__ done, osfm_ransac_affine_result *__restrict__ results)
{
    __shared__ double4 mpt[kAffineChunk];     // (x1, y1, x2, y2) of the staged matches; the partial sums of the refit
    __shared__ RansacLds<5> lds;
    __shared__ int s_n;                       // inliers of the refit

    const int jid = blockIdx.x / kRansacSplit, part = blockIdx.x % kRansacSplit;
    const RansacJob job = jobs[jid];
    const int k = job.k, tid = threadIdx.x;
    if (k < 4) {
        if (tid == 0 && part == 0) *job.count_out = -1;
        return;
    }
    // this part's iterations: whole passes of 256 * kAffineHyp
    constexpr int kPass = 256 * kAffineHyp;
    const RansacRange its = ransac_part_range(max_iterations, part, kPass);
    const RansacBand band(thr2);
    int best_count = 0, best_iter = 0x7fffffff;
    double bestv[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

    for (int base = its.begin; base < its.end; base += kPass) {
        AffineHyp H[kAffineHyp];
        bool valid[kAffineHyp];
        int cnt[kAffineHyp];
#pragma unroll
        for (int h = 0; h < kAffineHyp; ++h) {
            const int it = base + h * 256 + tid;
            valid[h] = false; cnt[h] = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) H[h].v[i] = 0.0;
            if (it < its.end) {
                // the first 4 distinct draws mod k, ascending
                int i0 = -1, i1 = -1, i2 = -1, i3 = -1, n = 0;
                for (uint64_t d = 0; n < 4; ++d) {
                    const int v = (int)(ransac_rand(seed, job.pair_id, (uint64_t)it, d) % (uint64_t)k);
                    if (v == i0 || v == i1 || v == i2) continue;
                    if (n == 0) i0 = v; else if (n == 1) i1 = v; else if (n == 2) i2 = v; else i3 = v;
                    ++n;
                }
                sort2(i0, i1); sort2(i2, i3); sort2(i0, i2); sort2(i1, i3); sort2(i1, i2);
                const double4 m0 = load_match(job, i0), m1 = load_match(job, i1), m2 = load_match(job, i2), m3 = load_match(job, i3);
                const double P[4][4] = { { m0.z, m0.w, m0.x, m0.y }, { m1.z, m1.w, m1.x, m1.y },
                                         { m2.z, m2.w, m2.x, m2.y }, { m3.z, m3.w, m3.x, m3.y } };
                valid[h] = four_point(P, H[h].v);
            }
            affine_bounds(H[h], band);
        }
        // inlier counts of this thread's hypotheses over all matches; every lane reads the same match
        for (int c0 = 0; c0 < k; c0 += kAffineChunk) {
            __syncthreads();
            for (int i = tid; i < kAffineChunk && c0 + i < k; i += 256) mpt[i] = load_match(job, c0 + i);
            __syncthreads();
            const int lim = min(kAffineChunk, k - c0);
            // invalid hypotheses (v zero: n = 0, s = 0, never below) are evaluated too: no divergence in the loop.
            // Four matches per round: their LDS reads are issued together
            int i = 0;
            for (; i + 4 <= lim; i += 4) {
                const double4 a0 = mpt[i], a1 = mpt[i + 1], a2 = mpt[i + 2], a3 = mpt[i + 3];
#pragma unroll
                for (int h = 0; h < kAffineHyp; ++h) {
                    cnt[h] += affine_below(H[h], a0.x, a0.y, a0.z, a0.w, thr2) ? 1 : 0;
                    cnt[h] += affine_below(H[h], a1.x, a1.y, a1.z, a1.w, thr2) ? 1 : 0;
                    cnt[h] += affine_below(H[h], a2.x, a2.y, a2.z, a2.w, thr2) ? 1 : 0;
                    cnt[h] += affine_below(H[h], a3.x, a3.y, a3.z, a3.w, thr2) ? 1 : 0;
                }
            }
            for (; i < lim; ++i) {
                const double4 a0 = mpt[i];
#pragma unroll
                for (int h = 0; h < kAffineHyp; ++h) cnt[h] += affine_below(H[h], a0.x, a0.y, a0.z, a0.w, thr2) ? 1 : 0;
            }
        }
#pragma unroll
        for (int h = 0; h < kAffineHyp; ++h) {
            const int it = base + h * 256 + tid;
            if (valid[h] && ransac_better(cnt[h], it, best_count, best_iter)) {
                best_count = cnt[h]; best_iter = it;
#pragma unroll
                for (int i = 0; i < 5; ++i) bestv[i] = H[h].v[i];
            }
        }
    }
    int win_count, win_iter;
    AffineHyp W;
    if (!ransac_elect(lds, slots, done, jid, part, tid, best_count, best_iter, bestv, win_count, win_iter, W.v)) return;
    if (win_count == 0) {
        if (tid == 0) {
            ransac_no_winner(job);
            if (results) results[jid] = osfm_ransac_affine_result{-1, 0, 0, 0};
        }
        return;
    }
    affine_bounds(W, band);
    int ran = 0, accepted = 0;
    if (refit && win_count >= 5) {
        if (tid == 0) s_n = 0;         // added to behind the barriers of the tree sums
        // one least-squares refit on the winner's inliers (affine_refit in affine_fit.h)
        AffineHyp R;
        affine_refit(reinterpret_cast<double *>(mpt), tid, k, win_count, [&](int i) { return load_match(job, i); },
            [&](const double4 &m) { return affine_below(W, m.x, m.y, m.z, m.w, thr2); }, R);
        affine_bounds(R, band);
        // all matches counted again under the refit; it replaces the winner when it holds at least as many
        int mine = 0;
        for (int i = tid; i < k; i += 256) {
            const double4 mm = load_match(job, i);
            mine += affine_below(R, mm.x, mm.y, mm.z, mm.w, thr2) ? 1 : 0;
        }
        if (mine) atomicAdd(&s_n, mine);
        __syncthreads();
        ran = 1;
        if (s_n >= win_count) { accepted = 1; W = R; }
    }
    if (tid == 0) {
        if (job.F_out) {
            for (int i = 0; i < 9; ++i) job.F_out[i] = 0.0;
            job.F_out[2] = W.v[0]; job.F_out[5] = W.v[1]; job.F_out[6] = W.v[2]; job.F_out[7] = W.v[3]; job.F_out[8] = W.v[4];
        }
        if (results) results[jid] = osfm_ransac_affine_result{win_iter, win_count, ran, accepted};
    }
    // ordered list of the inlier ids under the final F_A
    ransac_list_inliers(lds, job, tid, [&](int i) {
        const double4 m = load_match(job, i);
        return affine_below(W, m.x, m.y, m.z, m.w, thr2);
    });
}

size_t affine_scratch_bytes(int num_jobs) { return ransac_scratch_bytes(num_jobs, sizeof(AffineSlot)); }

void launch_ransac_affine(const RansacJob *d_jobs, int num_jobs, int max_iterations, double threshold, int refit,
    uint64_t seed, void *scratch, osfm_ransac_affine_result *d_results, hipStream_t s)
{
    if (num_jobs <= 0) return;
    AffineSlot *slots = static_cast<AffineSlot *>(scratch);
    int32_t *done = ransac_scratch_done(scratch, num_jobs, sizeof(AffineSlot), s);
    hipLaunchKernelGGL(ransac_affine_kernel, dim3(num_jobs * kRansacSplit), dim3(256), 0, s, d_jobs, num_jobs, max_iterations,
        threshold * threshold, refit != 0 ? 1 : 0, seed, slots, done, d_results);
}

}  // namespace osfm
