// The scaffold that the pair-RANSAC kernels share (ransac_kernel, ransac_affine_kernel): what running one pair's
// hypotheses on kRansacSplit workgroups of 256 threads needs whatever the model.  A kernel draws, solves and scores
// its own hypotheses; its share of the iterations, the band of the safe product tests, the tie rule, the election of
// the pair's winner and the ordered inlier list are here.  N: the doubles of a model (9 for F, 5 for F_A).
#pragma once
#include "ransac_kernels.h"

#include <algorithm>

namespace osfm {

// best (count, iteration, model) of one part of a pair's hypotheses
template <int N> struct RansacSlot { int32_t count, iter; double m[N]; };

// what the scaffold keeps in LDS; a kernel declares one, __shared__
template <int N> struct RansacLds { int s_count[256], s_iter[256]; double m[N]; int s_wave[4], s_run, s_last; };

// scratch of a launch: the slots of all jobs, then one completion counter per job (16-byte aligned)
inline size_t ransac_scratch_bytes(int num_jobs, size_t slot_bytes)
{
    return (size_t)std::max(num_jobs, 1) * (kRansacSplit * slot_bytes + 16);
}

// the completion counters of a launch's scratch block, cleared on the launch's stream
inline int32_t *ransac_scratch_done(void *scratch, int num_jobs, size_t slot_bytes, hipStream_t s)
{
    int32_t *done = reinterpret_cast<int32_t *>(static_cast<char *>(scratch) + (size_t)num_jobs * kRansacSplit * slot_bytes);
    (void)hipMemsetAsync(done, 0, (size_t)num_jobs * sizeof(int32_t), s);
    return done;
}

// iterations [begin, end) of a part: whole passes of `pass` iterations (256 threads x hypotheses per thread)
struct RansacRange { int begin, end; };

__device__ __forceinline__ RansacRange ransac_part_range(int max_iterations, int part, int pass)
{
    const int per_part = ((max_iterations + kRansacSplit - 1) / kRansacSplit + pass - 1) / pass * pass;
    const int begin = part * per_part;
    return { begin, min(max_iterations, begin + per_part) };
}

// thr2 and the two bounds of the safe product tests, thr2 (1 -+ 2^-49): n < s thr_lo implies fl(n / s) < thr2 and
// n >= s thr_hi implies fl(n / s) >= thr2 (sampson_below in ransac_kernels.hip has the argument)
struct RansacBand {
    double thr2, thr_lo, thr_hi;
    __device__ __forceinline__ explicit RansacBand(double t2)
        : thr2(t2), thr_lo(t2 * (1.0 - 1.7763568394002505e-15)), thr_hi(t2 * (1.0 + 1.7763568394002505e-15)) {}
};

// strictly more inliers wins; equal non-zero counts keep the earlier iteration (ransac_fundamental.cc:47)
__device__ __forceinline__ bool ransac_better(int count, int iter, int best_count, int best_iter)
{
    return count > best_count || (count == best_count && count > 0 && iter < best_iter);
}

// (x1, y1, x2, y2) of match i of a job
__device__ __forceinline__ double4 load_match(const RansacJob &job, int i)
{
    const int a = job.corr[2 * i], b = job.corr[2 * i + 1];
    return make_double4(job.pos1[2 * a], job.pos1[2 * a + 1], job.pos2[2 * b], job.pos2[2 * b + 1]);
}

// From every thread's best (count, iteration, model) of this part to the pair's winner.  The block's argmax goes into
// the part's slot; the part that gets there last (the counter of the pair) picks the best of all slots, re-arms the
// counter for the next launch and returns true with the winner, win_count == 0 when no part had an inlier.  Every
// other part returns false and is done; no workgroup waits for another.  A thread with no inlier: (0, 0x7fffffff, 0).
template <int N>
__device__ __forceinline__ bool
ransac_elect(RansacLds<N> &lds, RansacSlot<N> *slots, int32_t *done, int jid, int part, int tid,
    int best_count, int best_iter, const double (&best)[N], int &win_count, int &win_iter, double (&win)[N])
{
    // block argmax: (count desc, iteration asc).  ransac_better's count > 0 term changes nothing here: a thread
    // with count 0 carries iteration 0x7fffffff, which is before no other
    lds.s_count[tid] = best_count; lds.s_iter[tid] = best_iter;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) {
            const int c2 = lds.s_count[tid + st], i2 = lds.s_iter[tid + st];
            if (ransac_better(c2, i2, lds.s_count[tid], lds.s_iter[tid])) { lds.s_count[tid] = c2; lds.s_iter[tid] = i2; }
        }
        __syncthreads();
    }
    win_count = lds.s_count[0]; win_iter = lds.s_iter[0];
    if (best_count == win_count && best_iter == win_iter && win_count > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds.m[i] = best[i];
    }
    __syncthreads();
    // this part's best into its slot; the last part to get here goes on with all of them
    if (tid == 0) {
        RansacSlot<N> &mine = slots[(size_t)jid * kRansacSplit + part];
        mine.count = win_count; mine.iter = win_iter;
        for (int i = 0; i < N; ++i) mine.m[i] = win_count > 0 ? lds.m[i] : 0.0;
        __threadfence();
        lds.s_last = atomicAdd(&done[jid], 1) == kRansacSplit - 1;
    }
    __syncthreads();
    if (!lds.s_last) return false;
    if (tid == 0) {
        __threadfence();
        int bc = 0, bi = 0x7fffffff, bp = -1;
        for (int p = 0; p < kRansacSplit; ++p) {
            const RansacSlot<N> &sl = slots[(size_t)jid * kRansacSplit + p];
            if (ransac_better(sl.count, sl.iter, bc, bi)) { bc = sl.count; bi = sl.iter; bp = p; }
        }
        lds.s_count[0] = bc; lds.s_iter[0] = bi;
        for (int i = 0; i < N; ++i) lds.m[i] = bp >= 0 ? slots[(size_t)jid * kRansacSplit + bp].m[i] : 0.0;
        done[jid] = 0;                 // ready for the next launch
        lds.s_run = 0;
    }
    __syncthreads();
    win_count = lds.s_count[0]; win_iter = lds.s_iter[0];
#pragma unroll
    for (int i = 0; i < N; ++i) win[i] = lds.m[i];
    return true;
}

// what thread 0 of the last part writes for a pair none of whose hypotheses has an inlier
__device__ __forceinline__ void ransac_no_winner(const RansacJob &job)
{
    *job.count_out = 0;
    if (job.F_out) for (int i = 0; i < 9; ++i) job.F_out[i] = 0.0;
}

// The ids of the matches with in_pred(i), in ascending order, into job.inliers_out and their number into job.count_out;
// after ransac_elect returned true (it zeroes the running offset).
template <int N, class Pred>
__device__ __forceinline__ void ransac_list_inliers(RansacLds<N> &lds, const RansacJob &job, int tid, Pred in_pred)
{
    const int lane = tid & 63, wave = tid >> 6;
    for (int c0 = 0; c0 < job.k; c0 += 256) {
        const int i = c0 + tid;
        const bool in = i < job.k && in_pred(i);
        const unsigned long long bal = __ballot(in);
        if (lane == 0) lds.s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = lds.s_run;
        for (int w = 0; w < wave; ++w) off += lds.s_wave[w];
        if (in) job.inliers_out[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        __syncthreads();
        if (tid == 0) lds.s_run += lds.s_wave[0] + lds.s_wave[1] + lds.s_wave[2] + lds.s_wave[3];
        __syncthreads();
    }
    if (tid == 0) *job.count_out = lds.s_run;
}

}  // namespace osfm
