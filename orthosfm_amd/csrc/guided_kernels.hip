// Guided matching of verified pairs of orthographic views: the nearest-neighbour search of the exhaustive matcher once
// more, over the candidates inside the band of the pair's affine fundamental matrix only (osfm_match_guided in
// include/osfm_hip.h has the semantics; tests/guided_restatement.py restates them in numpy, and the kernels equal it
// in every byte).  The reference project has no such step.
//
//   guided_prepare_kernel   one workgroup per pair: F_A (given, or affine_refit over all seeds -- the code the affine
//                           RANSAC refits with, affine_fit.h), the status, the band scalars of every feature
//                           (u1 = (x1 c + y1 d) + e, u2 = x2 a + y2 b; the verifier's residual of a match is u2 + u1 in
//                           its own order of operations), NaN for the features of a seed -- a NaN passes no branch of
//                           the three-way test, so a seed's feature is no candidate and has none --, and the caps.
//   guided_match_kernel     a workgroup per kGuidedQueries queries of one direction and type.  The other view's band
//                           scalars pass through LDS in chunks of kGuidedChunk; a wave takes its queries one after the
//                           other, tests 64 positions a step, appends the positions in the band to the query's list by
//                           ballot (ascending), and when kGuidedPass are waiting scores them one per lane with the
//                           reference's 16-bit lane sums and advances the T-typed (best, second, index) through them in
//                           list order.  EVERY query is scanned in index order, so the products that do not fit T need
//                           no path of their own.
//   guided_finish_kernel    one workgroup per pair: cross-check, seeds put back, the list in feature_1 order.
//   guided_gather_kernel    the pairs' lists back to back, once the host has their lengths.
// Four launches a call whatever the number of pairs; no workgroup waits for another; integer maxima are the only
// atomics.  Double-precision arithmetic is in the verifier's operation order (no FMA contraction in this build).
#include "guided_kernels.h"
#include "affine_fit.h"

#include <climits>

namespace osfm {

namespace {

// The reference's inner product of two rows as the bank holds them (nearest_neighbor.cc:75-84): lane l sums the
// products of elements 8 i + l modulo 2^16, the lanes are read back as T and added as int.
template <int DIM, bool SIGNED>
__device__ __forceinline__ int guided_product(const int8_t *q, const int8_t *c)
{
    unsigned lanes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < DIM; k += 16) {
        const int4 wq = *reinterpret_cast<const int4 *>(q + k), wc = *reinterpret_cast<const int4 *>(c + k);
        const int aq[4] = {wq.x, wq.y, wq.z, wq.w}, ac[4] = {wc.x, wc.y, wc.z, wc.w};
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int bq = (aq[t >> 2] >> (8 * (t & 3))) & 0xff, bc = (ac[t >> 2] >> (8 * (t & 3))) & 0xff;
            const int vq = SIGNED ? (int)(int8_t)bq : (bq ^ 0x80), vc = SIGNED ? (int)(int8_t)bc : (bc ^ 0x80);
            lanes[t & 7] += (unsigned)(vq * vc);
        }
    }
    int ip = 0;
#pragma unroll
    for (int l = 0; l < 8; ++l) ip += SIGNED ? (int)(short)(lanes[l] & 0xffffu) : (int)(lanes[l] & 0xffffu);
    return ip;
}

// a value as a T-typed field holds it
template <bool SIGNED> __device__ __forceinline__ int guided_as_t(int v) { return SIGNED ? (int)(short)v : (int)(unsigned short)v; }

// nearest_neighbor.cc:262-267 / :234-237: the distance a T-typed product becomes (itself T-typed)
template <bool SIGNED> __device__ __forceinline__ int guided_distance(int p)
{
    if (SIGNED) return (int)(short)(32258 - 2 * min(16129, max(0, p)));
    return min(32767, 65025 - min(65025, p)) * 2;
}

// dist_1st of a search over one candidate with product ip: the state takes it when ip >= 0, else it stays at 0
template <bool SIGNED> __device__ __forceinline__ int guided_seed_distance(int ip)
{
    return guided_distance<SIGNED>(ip >= 0 ? guided_as_t<SIGNED>(ip) : 0);
}

// what one lane wrote to LDS is read by another lane of its wave: LDS operations of a wave complete in order, the
// fences keep the compiler from moving them
__device__ __forceinline__ void guided_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct GuidedSide {
    const double *uq, *uc;       // band scalars of the queries' / the candidates' view
    const int8_t *Q, *C;         // rows of the type
    int32_t *out;
    int nq, nc, qoff, coff;      // rows of the type on either side; the type's first combined index
};

template <int DIM, bool SIGNED>
__device__ __forceinline__ void
guided_scan(const GuidedSide &sd, int q0, const GuidedPrep &pp, int cap, float sq_lowe, int32_t *max_candidates,
    double *s_u, int8_t *s_q, int32_t (*s_list)[kGuidedPass], int32_t (*s_state)[6])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = min(kGuidedQueries, sd.nq - q0);
    if (sd.nc == 0) {
        if (tid < nq) sd.out[sd.qoff + q0 + tid] = -1;
        return;
    }
    for (int e = tid; e < kGuidedQueries * DIM; e += 256) {
        const int qi = e / DIM;
        s_q[e] = qi < nq ? sd.Q[(size_t)(q0 + qi) * DIM + (e - qi * DIM)] : (int8_t)0;
    }
    if (tid < kGuidedQueries) {
        s_state[tid][0] = 0; s_state[tid][1] = 0;       // best, second: the reference's state starts at (0, 0)
        s_state[tid][2] = -1; s_state[tid][3] = -1;     // the best's candidate; the first candidate (index 0 of the reference's list)
        s_state[tid][4] = 0; s_state[tid][5] = 0;       // candidates waiting in the list; candidates so far
    }
    const double s_lo = pp.s_lo, s_hi = pp.s_hi, ss = pp.s, thr2 = pp.thr2;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    for (int c0 = 0;; c0 += kGuidedChunk) {
        // the pass behind the last chunk (c0 >= nc) scores what is still waiting and writes the results
        const bool last = c0 >= sd.nc;
        __syncthreads();
        if (!last)
            for (int i = tid; i < kGuidedChunk; i += 256) s_u[i] = c0 + i < sd.nc ? sd.uc[sd.coff + c0 + i] : nan;
        __syncthreads();
        const int lim = last ? 0 : min(kGuidedChunk, sd.nc - c0);
        for (int qq = 0; qq < kGuidedQueries / 4; ++qq) {
            const int qi = wave * (kGuidedQueries / 4) + qq;       // the same in every lane of the wave
            if (qi >= nq) break;
            const double uv = sd.uq[sd.qoff + q0 + qi];
            int best = s_state[qi][0], second = s_state[qi][1], idx = s_state[qi][2], first = s_state[qi][3];
            int count = s_state[qi][4], total = s_state[qi][5];
            const int8_t *qrow = s_q + qi * DIM;
            // the waiting candidates, one per lane; the state goes through them in list order
            auto score = [&]() {
                guided_wave_sync();
                int ip = 0, j = 0;
                if (lane < count) {
                    j = s_list[qi][lane];
                    ip = guided_product<DIM, SIGNED>(qrow, sd.C + (size_t)j * DIM);
                }
                int bl = -1;
                for (int l = 0; l < count; ++l) {
                    const int v = __shfl(ip, l);
                    if (v >= second) {
                        if (v >= best) { second = best; best = guided_as_t<SIGNED>(v); bl = l; }
                        else second = guided_as_t<SIGNED>(v);
                    }
                }
                if (bl >= 0) idx = __shfl(j, bl);
                count = 0;
                guided_wave_sync();
            };
            for (int j0 = 0; j0 < lim; j0 += 64) {
                double n = s_u[j0 + lane] + uv;
                n *= n;
                const bool in = n < s_lo ? true : (n >= s_hi ? false : n / ss < thr2);
                const unsigned long long bal = __ballot(in);
                if (bal == 0) continue;
                const int pc = __popcll(bal);
                if (count + pc > kGuidedPass) score();
                if (in) s_list[qi][count + __popcll(bal & ((1ull << lane) - 1ull))] = c0 + j0 + lane;
                if (first < 0) first = c0 + j0 + __ffsll((long long)bal) - 1;
                count += pc; total += pc;
            }
            if (last) {
                if (count > 0) score();
                if (lane == 0) {
                    int res = -1;
                    if (total > 0) {
                        const int d1 = guided_distance<SIGNED>(best), d2 = guided_distance<SIGNED>(second);
                        res = sd.coff + (idx >= 0 ? idx : first);
                        // matching.h:114-146 without a distance threshold; 0 / 0 is no number and compares false
                        if (d1 > cap || (float)d1 / (float)d2 > sq_lowe) res = -1;
                        atomicMax(max_candidates, total);
                    }
                    sd.out[sd.qoff + q0 + qi] = res;
                }
            } else if (lane == 0) {
                s_state[qi][0] = best; s_state[qi][1] = second; s_state[qi][2] = idx; s_state[qi][3] = first;
                s_state[qi][4] = count; s_state[qi][5] = total;
            }
        }
        if (last) break;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void
guided_prepare_kernel(const GuidedJob *__restrict__ jobs, GuidedPrep *__restrict__ prep, double thr2, int cap_from_seeds)
{
    __shared__ double red[2560];
    __shared__ int s_cap[2];
    const GuidedJob job = jobs[blockIdx.x];
    const int tid = threadIdx.x, k = job.num_seeds;
    const int n1 = job.ns1 + job.nu1, n2 = job.ns2 + job.nu2;
    if (tid < 2) s_cap[tid] = -1;
    AffineHyp H;
    int status = OSFM_GUIDED_OK;
#pragma unroll
    for (int i = 0; i < 5; ++i) H.v[i] = job.has_F ? job.F[i] : 0.0;
    if (!job.has_F) {
        if (k < 5) status = OSFM_GUIDED_TOO_FEW;
        else
            affine_refit(red, tid, k, k,
                [&](int i) {
                    const int a = job.seeds[2 * i], b = job.seeds[2 * i + 1];
                    return make_double4(job.pos1[2 * a], job.pos1[2 * a + 1], job.pos2[2 * b], job.pos2[2 * b + 1]);
                },
                [](const double4 &) { return true; }, H);
    }
    const RansacBand band(thr2);
    affine_bounds(H, band);
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) finite = finite && H.v[i] - H.v[i] == 0.0;
    if (status == OSFM_GUIDED_OK && (!finite || !(H.s > 0.0))) status = OSFM_GUIDED_DEGENERATE;
    __syncthreads();
    if (status == OSFM_GUIDED_OK) {
        for (int i = tid; i < n1; i += 256) {
            const double x = job.pos1[2 * i], y = job.pos1[2 * i + 1];
            job.u1[i] = (x * H.v[2] + y * H.v[3]) + H.v[4];
        }
        for (int i = tid; i < n2; i += 256) {
            const double x = job.pos2[2 * i], y = job.pos2[2 * i + 1];
            job.u2[i] = x * H.v[0] + y * H.v[1];
        }
        __syncthreads();
        // a seed's features leave the play; its own product bounds what its type may add
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int t = tid; t < k; t += 256) {
            const int f1 = job.seeds[2 * t], f2 = job.seeds[2 * t + 1];
            job.u1[f1] = nan; job.u2[f2] = nan;
            if (f1 < job.ns1)
                atomicMax(&s_cap[0], guided_seed_distance<false>(guided_product<128, false>(
                    job.sift1 + (size_t)f1 * 128, job.sift2 + (size_t)f2 * 128)));
            else
                atomicMax(&s_cap[1], guided_seed_distance<true>(guided_product<64, true>(
                    job.surf1 + (size_t)(f1 - job.ns1) * 64, job.surf2 + (size_t)(f2 - job.ns2) * 64)));
        }
    }
    __syncthreads();
    if (tid == 0) {
        GuidedPrep &pp = prep[blockIdx.x];
        for (int i = 0; i < 5; ++i) pp.v[i] = H.v[i];
        pp.s = H.s; pp.s_lo = H.s_lo; pp.s_hi = H.s_hi; pp.thr2 = thr2;
        pp.cap[0] = cap_from_seeds ? s_cap[0] : INT_MAX;
        pp.cap[1] = cap_from_seeds ? s_cap[1] : INT_MAX;
        pp.status = status; pp.count = 0; pp.max_candidates = 0; pp.pad = 0;
    }
}

__global__ __launch_bounds__(256) void
guided_match_kernel(const GuidedJob *__restrict__ jobs, int num_jobs, GuidedPrep *__restrict__ prep, float sq_sift, float sq_surf)
{
    __shared__ double s_u[kGuidedChunk];
    __shared__ __attribute__((aligned(16))) int8_t s_q[kGuidedQueries * 128];
    __shared__ int32_t s_list[kGuidedQueries][kGuidedPass];
    __shared__ int32_t s_state[kGuidedQueries][6];
    // the pair of this workgroup: the first whose workgroups end behind it
    const int bid = blockIdx.x;
    int lo = 0, hi = num_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].block_end > bid) hi = mid; else lo = mid + 1;
    }
    const GuidedJob &job = jobs[lo];
    GuidedPrep &pp = prep[lo];
    if (pp.status != OSFM_GUIDED_OK) return;        // the pair's list is its seeds; nothing reads m12 / m21
    int b = bid - job.block_start;
    if (b < 0 || bid >= job.block_end) return;
    const int ns1 = job.ns1, nu1 = job.nu1, ns2 = job.ns2, nu2 = job.nu2;
    const int nb0 = (ns1 + kGuidedQueries - 1) / kGuidedQueries, nb1 = (nu1 + kGuidedQueries - 1) / kGuidedQueries;
    const int nb2 = (ns2 + kGuidedQueries - 1) / kGuidedQueries;
    int dir = 0, type = 0;
    if (b >= nb0) { b -= nb0; type = 1;
        if (b >= nb1) { b -= nb1; dir = 1; type = 0;
            if (b >= nb2) { b -= nb2; type = 1; } } }
    GuidedSide sd;
    if (dir == 0) {
        sd.uq = job.u1; sd.uc = job.u2; sd.out = job.m12;
        sd.Q = type ? job.surf1 : job.sift1; sd.C = type ? job.surf2 : job.sift2;
        sd.nq = type ? nu1 : ns1; sd.nc = type ? nu2 : ns2; sd.qoff = type ? ns1 : 0; sd.coff = type ? ns2 : 0;
    } else {
        sd.uq = job.u2; sd.uc = job.u1; sd.out = job.m21;
        sd.Q = type ? job.surf2 : job.sift2; sd.C = type ? job.surf1 : job.sift1;
        sd.nq = type ? nu2 : ns2; sd.nc = type ? nu1 : ns1; sd.qoff = type ? ns2 : 0; sd.coff = type ? ns1 : 0;
    }
    const int q0 = b * kGuidedQueries;
    if (q0 >= sd.nq) return;
    if (type == 0) guided_scan<128, false>(sd, q0, pp, pp.cap[0], sq_sift, &pp.max_candidates, s_u, s_q, s_list, s_state);
    else guided_scan<64, true>(sd, q0, pp, pp.cap[1], sq_surf, &pp.max_candidates, s_u, s_q, s_list, s_state);
}

__global__ __launch_bounds__(256) void
guided_finish_kernel(const GuidedJob *__restrict__ jobs, GuidedPrep *__restrict__ prep)
{
    __shared__ int s_wave[4], s_run;
    const GuidedJob job = jobs[blockIdx.x];
    GuidedPrep &pp = prep[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = job.num_seeds;
    const int n1 = job.ns1 + job.nu1;
    if (pp.status != OSFM_GUIDED_OK) {
        for (int t = tid; t < 2 * k; t += 256) job.list[t] = job.seeds[t];
        if (tid == 0) pp.count = k;
        return;
    }
    // remove_inconsistent_matches (matching.cc:18-36) as far as the list needs it: i -> j stays when j -> i
    for (int i = tid; i < n1; i += 256) {
        const int j = job.m12[i];
        job.m12[i] = j >= 0 && job.m21[j] == i ? j : -1;
    }
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int t = tid; t < k; t += 256) job.m12[job.seeds[2 * t]] = job.seeds[2 * t + 1];
    __syncthreads();
    for (int c0 = 0; c0 < n1; c0 += 256) {
        const int i = c0 + tid;
        const int j = i < n1 ? job.m12[i] : -1;
        const bool in = j >= 0;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = s_run;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (in) {
            off += __popcll(bal & ((1ull << lane) - 1ull));
            job.list[2 * off] = i; job.list[2 * off + 1] = j;
        }
        __syncthreads();
        if (tid == 0) s_run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) pp.count = s_run;
}

__global__ __launch_bounds__(256) void
guided_gather_kernel(const GuidedJob *__restrict__ jobs, const GuidedPrep *__restrict__ prep,
    const int64_t *__restrict__ dst_off, int32_t *__restrict__ out)
{
    const int32_t *src = jobs[blockIdx.x].list;
    int32_t *dst = out + 2 * dst_off[blockIdx.x];
    const int n = 2 * prep[blockIdx.x].count;
    for (int t = threadIdx.x; t < n; t += 256) dst[t] = src[t];
}

void launch_guided_prepare(const GuidedJob *d_jobs, int num_jobs, GuidedPrep *d_prep, double threshold, int cap_from_seeds, hipStream_t s)
{
    if (num_jobs <= 0) return;
    hipLaunchKernelGGL(guided_prepare_kernel, dim3(num_jobs), dim3(256), 0, s, d_jobs, d_prep, threshold * threshold,
        cap_from_seeds != 0 ? 1 : 0);
}

void launch_guided_match(const GuidedJob *d_jobs, int num_jobs, int total_blocks, GuidedPrep *d_prep, float sq_sift, float sq_surf, hipStream_t s)
{
    if (num_jobs <= 0 || total_blocks <= 0) return;
    hipLaunchKernelGGL(guided_match_kernel, dim3(total_blocks), dim3(256), 0, s, d_jobs, num_jobs, d_prep, sq_sift, sq_surf);
}

void launch_guided_finish(const GuidedJob *d_jobs, int num_jobs, GuidedPrep *d_prep, hipStream_t s)
{
    if (num_jobs <= 0) return;
    hipLaunchKernelGGL(guided_finish_kernel, dim3(num_jobs), dim3(256), 0, s, d_jobs, d_prep);
}

void launch_guided_gather(const GuidedJob *d_jobs, int num_jobs, const GuidedPrep *d_prep, const int64_t *d_dst_off, int32_t *d_out, hipStream_t s)
{
    if (num_jobs <= 0) return;
    hipLaunchKernelGGL(guided_gather_kernel, dim3(num_jobs), dim3(256), 0, s, d_jobs, d_prep, d_dst_off, d_out);
}

}  // namespace osfm
