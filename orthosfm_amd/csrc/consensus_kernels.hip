// Kernels of the per-track consensus triangulation (consensus_kernels.h).
//
//   consensus_prepare_kernel     per camera the affine projection pix = A X + b and the unit look direction; per
//                                observation the ray origin (camera_ray of the triangulation)
//   consensus_vote_short_kernel  tracks of 2..8 observations: eight neighbouring lanes per track, lane = observation,
//                                a loop over the at most 28 pairs, count and sum folded by xor-shuffles
//   consensus_vote_long_kernel   longer tracks: a wave per track, lane = hypothesis (at most 120: two rounds of 64),
//                                observations staged through LDS 64 at a time and read as broadcasts
//   consensus_refit_kernel       ba_triangulate_kernel over the observations of a mask
//   consensus_classify_kernel    the new mask from the reprojection errors at the refit point
//   consensus_verdict_kernel     status, keep flags, returned point, the counters of the statistics
//
// Nothing waits on another workgroup and nothing but the integer counters is accumulated atomically: every fold has a
// fixed order, and a track's result depends on that track's observations alone.
#include <cmath>

#include "consensus_kernels.h"
#include "ba_rays.h"

namespace osfm {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ double dot3(const double a[3], const double b[3])
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// midpoint of the common perpendicular of the rays (oa, da), (ob, db), unit directions; false: (nearly) parallel
__device__ __forceinline__ bool pair_midpoint(const double oa[3], const double da[3], const double ob[3], const double db[3],
    double X[3])
{
    const double c = dot3(da, db);
    const double den = 1.0 - c * c;
    if (!(den > 1e-12)) return false;
    const double w[3] = { oa[0] - ob[0], oa[1] - ob[1], oa[2] - ob[2] };
    const double p = dot3(da, w), q = dot3(db, w);
    const double sa = (c * q - p) / den, sb = (q - c * p) / den;
    for (int i = 0; i < 3; ++i) X[i] = 0.5 * ((oa[i] + sa * da[i]) + (ob[i] + sb * db[i]));
    return true;
}

// squared pixel distance of A X + b from (x, y)
__device__ __forceinline__ double pixel_dist2(const double A[6], double b0, double b1, double x, double y, const double X[3])
{
    const double rx = (((A[0] * X[0] + A[1] * X[1]) + A[2] * X[2]) + b0) - x;
    const double ry = (((A[3] * X[0] + A[4] * X[1]) + A[5] * X[2]) + b1) - y;
    return rx * rx + ry * ry;
}

// (count, sum, index): more inliers, then the smaller sum of squared inlier errors, then the earlier hypothesis
__device__ __forceinline__ bool vote_better(int c1, double s1, int i1, int c2, double s2, int i2)
{
    if (c1 != c2) return c1 > c2;
    if (s1 != s2) return s1 < s2;
    return i1 < i2;
}

// observation index (within the track) of sample position i
__device__ __forceinline__ int sample_index(int i, int n, int ns) { return n <= ns ? i : (int)(((long long)i * n) / ns); }

__global__ __launch_bounds__(kThreads) void
consensus_prepare_kernel(BaDev d, double *__restrict__ camtab, double *__restrict__ origin)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.C) {
        // the residual functor at the origin with a zero observation: r = b, d r / d X = A
        const double P0[4] = { 0.0, 0.0, 0.0, 1.0 };
        ObsFull e;
        if (d.model == kModelQuat) eval_quat(d.cams + 7 * i, P0, (double)d.img_w[i], (double)d.img_h[i], 0.0, 0.0, true, e);
        else eval_euler(d.cams + 7 * i, P0, (double)d.img_w[i], (double)d.img_h[i], 0.0, 0.0, true, e);
        double *t = camtab + (size_t)kConsensusCam * i;
        for (int k = 0; k < 3; ++k) { t[k] = e.JP[0][k]; t[3 + k] = e.JP[1][k]; }
        t[6] = e.r[0]; t[7] = e.r[1];
        double o3[3], dir[3];
        camera_ray(d, i, 0.0, 0.0, o3, dir);
        const double n = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
        t[8] = dir[0] / n; t[9] = dir[1] / n; t[10] = dir[2] / n; t[11] = 0.0;
    }
    if (i < d.O) {
        double o3[3], dir[3];
        camera_ray(d, d.obs_cam[i], d.obs_xy[2 * i], d.obs_xy[2 * i + 1], o3, dir);
        origin[3 * (size_t)i] = o3[0]; origin[3 * (size_t)i + 1] = o3[1]; origin[3 * (size_t)i + 2] = o3[2];
    }
}

// What the voting kernels leave per track: active (a winner exists: the refit works on it), the winner's point in
// points_work, its mask in mask, the number of hypotheses scored; tracks of fewer than two observations and tracks
// without a valid pair keep all their observations.
struct VoteArgs {
    const double *camtab, *origin;
    double max_error;
    int ns;                        // sample cap
    uint8_t *mask;                 // [O]
    uint8_t *active;               // [M] 0: untested, 1: voted, 2: degenerate
    int32_t *hyps;                 // [M]
    double *points_work;           // [M][4]
};

__global__ __launch_bounds__(kThreads) void
consensus_vote_short_kernel(BaDev d, VoteArgs a)
{
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = gt >> 3, sub = gt & 7;
    if (j >= d.M) return;                       // (an octet never straddles j < M)
    const int k0 = d.pt_start[j], n = d.pt_start[j + 1] - k0;
    if (n > kConsensusShortLen) return;         // the long kernel's
    if (n < 2) {
        if (sub < n) a.mask[k0 + sub] = 1;
        if (sub == 0) { a.active[j] = 0; a.hyps[j] = 0; }
        return;
    }
    // lane = observation
    const bool mine = sub < n;
    double o[3] = { 0, 0, 0 }, dr[3] = { 0, 0, 1 }, A[6] = { 0, 0, 0, 0, 0, 0 }, b0 = 0, b1 = 0, x = 0, y = 0;
    if (mine) {
        const int k = k0 + sub;
        const double *t = a.camtab + (size_t)kConsensusCam * d.obs_cam[k];
        for (int i = 0; i < 6; ++i) A[i] = t[i];
        b0 = t[6]; b1 = t[7];
        for (int i = 0; i < 3; ++i) { dr[i] = t[8 + i]; o[i] = a.origin[3 * (size_t)k + i]; }
        x = d.obs_xy[2 * k]; y = d.obs_xy[2 * k + 1];
    }
    const int ns = n < a.ns ? n : a.ns;
    const int lane0 = (threadIdx.x & 63) & ~7;          // first lane of the octet in its wave
    int best_c = -1, best_i = 0, scored = 0, hyp = 0;
    double best_s = 0.0, best_X[3] = { 0, 0, 0 };
    bool best_in = true;
    for (int ia = 0; ia < ns; ++ia) {
        const int la = lane0 + sample_index(ia, n, ns);
        double oa[3], da[3];
        for (int i = 0; i < 3; ++i) { oa[i] = __shfl(o[i], la); da[i] = __shfl(dr[i], la); }
        for (int ib = ia + 1; ib < ns; ++ib, ++hyp) {
            const int lb = lane0 + sample_index(ib, n, ns);
            double ob[3], db[3], X[3];
            for (int i = 0; i < 3; ++i) { ob[i] = __shfl(o[i], lb); db[i] = __shfl(dr[i], lb); }
            if (!pair_midpoint(oa, da, ob, db, X)) continue;          // (the same decision in all eight lanes)
            ++scored;
            const double e2 = pixel_dist2(A, b0, b1, x, y, X);
            const bool in = mine && sqrt(e2) < a.max_error;
            int c = in ? 1 : 0;
            double sum = in ? e2 : 0.0;
            for (int m = 1; m < 8; m <<= 1) { c += __shfl_xor(c, m); sum += __shfl_xor(sum, m); }
            if (vote_better(c, sum, hyp, best_c, best_s, best_i)) {
                best_c = c; best_s = sum; best_i = hyp; best_in = in;
                best_X[0] = X[0]; best_X[1] = X[1]; best_X[2] = X[2];
            }
        }
    }
    const bool voted = best_c >= 0;
    if (mine) a.mask[k0 + sub] = voted ? (best_in ? 1 : 0) : 1;
    if (sub == 0) {
        a.active[j] = voted ? 1 : 2;
        a.hyps[j] = scored;
        if (voted) {
            double *p = a.points_work + 4 * (size_t)j;
            p[0] = best_X[0]; p[1] = best_X[1]; p[2] = best_X[2]; p[3] = 1.0;
        }
    }
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void
consensus_vote_long_kernel(BaDev d, VoteArgs a)
{
    // per wave: the sampled rays (origin, direction) and a chunk of observations as rows (A, b, x), component-major
    // so that the staging writes neighbouring words and the scoring reads one word for the whole wave
    __shared__ double s_ray[kConsensusLongTracks][kConsensusMaxSample][6];
    __shared__ double s_obs[kConsensusLongTracks][10][kConsensusChunk];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * kConsensusLongTracks + wv;
    if (j >= d.M) return;
    const int k0 = d.pt_start[j], n = d.pt_start[j + 1] - k0;
    if (n <= kConsensusShortLen) return;        // the short kernel's
    const int ns = n < a.ns ? n : a.ns;
    if (lane < ns) {
        const int k = k0 + sample_index(lane, n, ns);
        const double *t = a.camtab + (size_t)kConsensusCam * d.obs_cam[k];
        for (int i = 0; i < 3; ++i) { s_ray[wv][lane][i] = a.origin[3 * (size_t)k + i]; s_ray[wv][lane][3 + i] = t[8 + i]; }
    }
    wave_lds_sync();
    const int nh = ns * (ns - 1) / 2;
    // lane = hypothesis lane + 64 r; its pair (ia, ib) in lexicographic order, its point
    bool ok[2] = { false, false };
    double X[2][3] = { { 0, 0, 0 }, { 0, 0, 0 } };
    for (int r = 0; r < 2; ++r) {
        int h = lane + 64 * r;
        if (h >= nh) continue;
        int ia = 0;
        while (h >= ns - 1 - ia) { h -= ns - 1 - ia; ++ia; }
        const int ib = ia + 1 + h;
        ok[r] = pair_midpoint(&s_ray[wv][ia][0], &s_ray[wv][ia][3], &s_ray[wv][ib][0], &s_ray[wv][ib][3], X[r]);
    }
    int cnt[2] = { 0, 0 };
    double sum[2] = { 0.0, 0.0 };
    for (int base = 0; base < n; base += kConsensusChunk) {
        const int m = n - base < kConsensusChunk ? n - base : kConsensusChunk;
        wave_lds_sync();                         // the previous chunk has been read
        if (lane < m) {
            const int k = k0 + base + lane;
            const double *t = a.camtab + (size_t)kConsensusCam * d.obs_cam[k];
            for (int i = 0; i < 8; ++i) s_obs[wv][i][lane] = t[i];
            s_obs[wv][8][lane] = d.obs_xy[2 * k]; s_obs[wv][9][lane] = d.obs_xy[2 * k + 1];
        }
        wave_lds_sync();
        for (int q = 0; q < m; ++q) {            // ascending observation order
            double A[6];
            for (int i = 0; i < 6; ++i) A[i] = s_obs[wv][i][q];
            const double b0 = s_obs[wv][6][q], b1 = s_obs[wv][7][q], x = s_obs[wv][8][q], y = s_obs[wv][9][q];
            for (int r = 0; r < 2; ++r) {
                if (!ok[r]) continue;
                const double e2 = pixel_dist2(A, b0, b1, x, y, X[r]);
                if (sqrt(e2) < a.max_error) { ++cnt[r]; sum[r] += e2; }
            }
        }
    }
    // the lane's better hypothesis, then the wave's: a total order, so the fold's shape does not matter
    int bc = ok[0] ? cnt[0] : -1, bi = lane;
    double bs = sum[0];
    if (ok[1] && vote_better(cnt[1], sum[1], lane + 64, bc, bs, bi)) { bc = cnt[1]; bs = sum[1]; bi = lane + 64; }
    for (int m = 1; m < 64; m <<= 1) {
        const int oc = __shfl_xor(bc, m), oi = __shfl_xor(bi, m);
        const double os = __shfl_xor(bs, m);
        if (vote_better(oc, os, oi, bc, bs, bi)) { bc = oc; bs = os; bi = oi; }
    }
    int scored = (ok[0] ? 1 : 0) + (ok[1] ? 1 : 0);
    for (int m = 1; m < 64; m <<= 1) scored += __shfl_xor(scored, m);
    const bool voted = bc >= 0;
    double Xw[3] = { 0, 0, 0 };
    if (voted) {
        // the winner's point again, in every lane (the same operations on the same rays: the same bits)
        int h = bi, ia = 0;
        while (h >= ns - 1 - ia) { h -= ns - 1 - ia; ++ia; }
        const int ib = ia + 1 + h;
        pair_midpoint(&s_ray[wv][ia][0], &s_ray[wv][ia][3], &s_ray[wv][ib][0], &s_ray[wv][ib][3], Xw);
    }
    // the winner's mask, lane = observation
    for (int q = lane; q < n; q += 64) {
        const int k = k0 + q;
        uint8_t in = 1;
        if (voted) {
            const double *t = a.camtab + (size_t)kConsensusCam * d.obs_cam[k];
            double A[6];
            for (int i = 0; i < 6; ++i) A[i] = t[i];
            const double e2 = pixel_dist2(A, t[6], t[7], d.obs_xy[2 * k], d.obs_xy[2 * k + 1], Xw);
            in = sqrt(e2) < a.max_error ? 1 : 0;
        }
        a.mask[k] = in;
    }
    if (lane == 0) {
        a.active[j] = voted ? 1 : 2;
        a.hyps[j] = scored;
        if (voted) {
            double *p = a.points_work + 4 * (size_t)j;
            p[0] = Xw[0]; p[1] = Xw[1]; p[2] = Xw[2]; p[3] = 1.0;
        }
    }
}

// ba_triangulate_kernel over the observations of the mask: eight neighbouring lanes per track, the partial sums folded
// in the same order.  fitted[j] = 1 where the round ran (an active track with two or more observations in its mask).
__global__ __launch_bounds__(128) void
consensus_refit_kernel(BaDev d, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ active, double *points_work,
    uint8_t *__restrict__ fitted)
{
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = gt >> 3, sub = gt & 7;
    if (j >= d.M) return;                       // (an octet never straddles j < M)
    const int k0 = d.pt_start[j], k1 = d.pt_start[j + 1];
    if (active[j] != 1) { if (sub == 0) fitted[j] = 0; return; }
    double R[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, q[3] = { 0, 0, 0 };
    int cnt = 0;
    for (int k = k0 + sub; k < k1; k += 8) {
        if (!mask[k]) continue;
        ++cnt;
        double o3[3], dir[3];
        camera_ray(d, d.obs_cam[k], d.obs_xy[2 * k], d.obs_xy[2 * k + 1], o3, dir);
        const double n = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
        dir[0] /= n; dir[1] /= n; dir[2] /= n;
        for (int a = 0; a < 3; ++a) {
            double row[3];
            for (int b = 0; b < 3; ++b) { row[b] = (a == b ? 1.0 : 0.0) - dir[a] * dir[b]; R[a][b] += row[b]; }
            q[a] += row[0] * o3[0] + row[1] * o3[1] + row[2] * o3[2];
        }
    }
    for (int m = 1; m < 8; m <<= 1) cnt += __shfl_xor(cnt, m);
    for (int a = 0; a < 3; ++a) {
        for (int m = 1; m < 8; m <<= 1) q[a] += __shfl_xor(q[a], m);
        for (int b = 0; b < 3; ++b)
            for (int m = 1; m < 8; m <<= 1) R[a][b] += __shfl_xor(R[a][b], m);
    }
    if (cnt < 2) { if (sub == 0) fitted[j] = 0; return; }
    double x[3];
    solve_ray_system(R, q, x);
    if (sub != 0) return;
    double *p = points_work + 4 * (size_t)j;
    p[0] = x[0]; p[1] = x[1]; p[2] = x[2]; p[3] = 1.0;
    fitted[j] = 1;
}

// mask[k] = err[k] < max_error on the tracks the round refitted; changed[j]: the round's mask differs from the one
// before it (what the last round that ran leaves is "the last two masks differ")
__global__ __launch_bounds__(kThreads) void
consensus_classify_kernel(BaDev d, const double *__restrict__ err, double max_error, const uint8_t *__restrict__ fitted,
    uint8_t *__restrict__ mask, uint8_t *__restrict__ changed)
{
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = gt >> 3, sub = gt & 7;
    if (j >= d.M) return;
    if (!fitted[j]) return;
    const int k0 = d.pt_start[j], k1 = d.pt_start[j + 1];
    int diff = 0;
    for (int k = k0 + sub; k < k1; k += 8) {
        const uint8_t m = err[k] < max_error ? 1 : 0;
        diff |= m != mask[k];
        mask[k] = m;
    }
    for (int m = 1; m < 8; m <<= 1) diff |= __shfl_xor(diff, m);
    if (sub == 0) changed[j] = diff ? 1 : 0;
}

struct VerdictArgs {
    const uint8_t *mask, *active, *changed;
    const int32_t *hyps;
    const double *points_work;
    int min_support;
    ConsensusOut out;
};

__global__ __launch_bounds__(kThreads) void
consensus_verdict_kernel(BaDev d, VerdictArgs a)
{
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = gt >> 3, sub = gt & 7;
    unsigned long long c[kCsCounters];
    for (int i = 0; i < kCsCounters; ++i) c[i] = 0;
    if (j < d.M) {
        const int k0 = d.pt_start[j], k1 = d.pt_start[j + 1], n = k1 - k0;
        const int act = a.active[j];
        int kept = 0;
        for (int k = k0 + sub; k < k1; k += 8) kept += a.mask[k] ? 1 : 0;
        for (int m = 1; m < 8; m <<= 1) kept += __shfl_xor(kept, m);
        int st;
        if (act == 0) st = OSFM_CONSENSUS_UNTESTED;
        else if (act == 2) st = OSFM_CONSENSUS_DEGENERATE;
        else if (kept == n) st = OSFM_CONSENSUS_CLEAN;
        else if (kept >= a.min_support) st = OSFM_CONSENSUS_REPAIRED;
        else st = OSFM_CONSENSUS_UNSUPPORTED;
        for (int k = k0 + sub; k < k1; k += 8) a.out.keep[k] = st == OSFM_CONSENSUS_UNSUPPORTED ? 0 : a.mask[k];
        if (sub == 0) {
            const bool has = st == OSFM_CONSENSUS_CLEAN || st == OSFM_CONSENSUS_REPAIRED;
            const double *src = has ? a.points_work + 4 * (size_t)j : d.points + 4 * (size_t)j;
            for (int i = 0; i < 4; ++i) a.out.points_out[4 * (size_t)j + i] = src[i];
            a.out.valid[j] = has ? 1 : 0;
            a.out.status[j] = st;
            if (act != 0) {
                c[kCsTested] = 1;
                c[kCsClean] = st == OSFM_CONSENSUS_CLEAN;
                c[kCsRepaired] = st == OSFM_CONSENSUS_REPAIRED;
                c[kCsUnsupported] = st == OSFM_CONSENSUS_UNSUPPORTED;
                c[kCsDegenerate] = st == OSFM_CONSENSUS_DEGENERATE;
                c[kCsUnsettled] = act == 1 && a.changed[j];
                c[kCsObsTested] = (unsigned long long)n;
                c[kCsObsDropped] = st == OSFM_CONSENSUS_UNSUPPORTED ? (unsigned long long)n : (unsigned long long)(n - kept);
                c[kCsHypotheses] = (unsigned long long)a.hyps[j];
            }
        }
    }
    // the statistics: integer sums, a wave's share folded first
    for (int i = 0; i < kCsCounters; ++i) {
        unsigned long long v = c[i];
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.out.counters + i, v);
    }
}

}  // namespace

int consensus_check_options(const osfm_consensus_options *o, const char *what)
{
    if (!o) { set_error("%s: null options", what); return OSFM_E_ARG; }
    if (!(o->max_error > 0.0) || !std::isfinite(o->max_error)) { set_error("%s: max_error %g is not a positive number", what, o->max_error); return OSFM_E_ARG; }
    if (o->min_support < 2) { set_error("%s: min_support %d below 2", what, o->min_support); return OSFM_E_ARG; }
    if (o->max_sample < 2 || o->max_sample > kConsensusMaxSample) {
        set_error("%s: max_sample %d outside [2, %d]", what, o->max_sample, kConsensusMaxSample); return OSFM_E_ARG;
    }
    if (o->refit_rounds < 0 || o->refit_rounds > OSFM_CONSENSUS_MAX_REFIT_ROUNDS) {
        set_error("%s: refit_rounds %d outside [0, %d]", what, o->refit_rounds, OSFM_CONSENSUS_MAX_REFIT_ROUNDS); return OSFM_E_ARG;
    }
    return OSFM_OK;
}

int consensus_run(const BaDev &d_in, const osfm_consensus_options &o, const ConsensusOut &out, hipStream_t s)
{
    BaDev d = d_in;
    d.lm = nullptr;
    const int C = d.C, M = d.M, O = d.O;
    OSFM_HIP_CHECK(hipMemsetAsync(out.counters, 0, sizeof(unsigned long long) * kCsCounters, s));
    if (M <= 0) return OSFM_OK;
    DevArray camtab, origin, mask, active, hyps, work, fitted, changed, err;
    OSFM_RETURN_IF(camtab.alloc((size_t)std::max(C, 1) * kConsensusCam * 8));
    OSFM_RETURN_IF(origin.alloc((size_t)std::max(O, 1) * 24));
    OSFM_RETURN_IF(mask.alloc((size_t)std::max(O, 1)));
    OSFM_RETURN_IF(active.alloc((size_t)M));
    OSFM_RETURN_IF(hyps.alloc((size_t)M * 4));
    OSFM_RETURN_IF(work.alloc((size_t)M * 32));
    OSFM_RETURN_IF(fitted.alloc((size_t)M));
    OSFM_RETURN_IF(changed.alloc((size_t)M));
    OSFM_RETURN_IF(err.alloc((size_t)std::max(O, 1) * 8));
    OSFM_HIP_CHECK(hipMemsetAsync(changed.ptr, 0, (size_t)M, s));
    // tracks that no refit reaches are evaluated at their input point
    OSFM_HIP_CHECK(hipMemcpyAsync(work.ptr, d.points, (size_t)M * 32, hipMemcpyDeviceToDevice, s));
    const int np = std::max(C, O);
    if (np > 0) hipLaunchKernelGGL(consensus_prepare_kernel, dim3((np + kThreads - 1) / kThreads), dim3(kThreads), 0, s, d,
        camtab.as<double>(), origin.as<double>());
    VoteArgs va;
    va.camtab = camtab.as<double>(); va.origin = origin.as<double>();
    va.max_error = o.max_error; va.ns = o.max_sample;
    va.mask = mask.as<uint8_t>(); va.active = active.as<uint8_t>(); va.hyps = hyps.as<int32_t>();
    va.points_work = work.as<double>();
    const unsigned g8 = (unsigned)(((int64_t)M * 8 + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(consensus_vote_short_kernel, dim3(g8), dim3(kThreads), 0, s, d, va);
    hipLaunchKernelGGL(consensus_vote_long_kernel, dim3((unsigned)((M + kConsensusLongTracks - 1) / kConsensusLongTracks)),
        dim3(kThreads), 0, s, d, va);
    BaDev dw = d;
    dw.points = work.as<double>();
    for (int r = 0; r < o.refit_rounds; ++r) {
        hipLaunchKernelGGL(consensus_refit_kernel, dim3((unsigned)(((int64_t)M * 8 + 127) / 128)), dim3(128), 0, s, d,
            mask.as<uint8_t>(), active.as<uint8_t>(), work.as<double>(), fitted.as<uint8_t>());
        launch_reproj(dw, err.as<double>(), nullptr, s);
        hipLaunchKernelGGL(consensus_classify_kernel, dim3(g8), dim3(kThreads), 0, s, d, err.as<double>(), o.max_error,
            fitted.as<uint8_t>(), mask.as<uint8_t>(), changed.as<uint8_t>());
    }
    VerdictArgs ve;
    ve.mask = mask.as<uint8_t>(); ve.active = active.as<uint8_t>(); ve.changed = changed.as<uint8_t>();
    ve.hyps = hyps.as<int32_t>(); ve.points_work = work.as<double>(); ve.min_support = o.min_support; ve.out = out;
    hipLaunchKernelGGL(consensus_verdict_kernel, dim3(g8), dim3(kThreads), 0, s, d, ve);
    BaDev dout = d;
    dout.points = out.points_out;
    launch_reproj(dout, out.err, nullptr, s);
    OSFM_HIP_CHECK(hipGetLastError());
    return OSFM_OK;
}

void consensus_fill_stats(const unsigned long long *c, float device_ms, osfm_consensus_stats *st)
{
    st->tracks_tested = (int64_t)c[kCsTested]; st->tracks_clean = (int64_t)c[kCsClean];
    st->tracks_repaired = (int64_t)c[kCsRepaired]; st->tracks_unsupported = (int64_t)c[kCsUnsupported];
    st->tracks_degenerate = (int64_t)c[kCsDegenerate]; st->tracks_unsettled = (int64_t)c[kCsUnsettled];
    st->obs_tested = (int64_t)c[kCsObsTested]; st->obs_dropped = (int64_t)c[kCsObsDropped];
    st->hypotheses_scored = (int64_t)c[kCsHypotheses];
    st->device_ms = (double)device_ms;
}

}  // namespace osfm
