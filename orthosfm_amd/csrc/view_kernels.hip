// Kernels of the view front end, see view_kernels.h.  All of them are memory bound and make one pass over their
// input; the library is built with -ffp-contract=off, which the float expressions below rely on: they are the
// host's (feature_view.h, osfm_quantize_sift / osfm_quantize_surf) operation for operation.
#include "view_kernels.h"

#include "feature_view.h"

namespace osfm {
namespace view {

namespace {

constexpr int kThreads = 256;

// The reference computes (uchar)(0.25f a + 0.25f b + 0.25f c + 0.25f d + 0.5f).  Every term is a byte scaled by a
// power of two and every partial sum a multiple of 0.25 below 1024, so all of it is exact in float; the truncation
// of the non-negative sum is a floor, and floor((a + b + c + d) / 4 + 1 / 2) = (a + b + c + d + 2) >> 2.
__device__ __forceinline__ unsigned quarter(unsigned a, unsigned b, unsigned c, unsigned d) { return (a + b + c + d + 2u) >> 2; }

// One thread per output pixel, all its channels; the last column / row stands in for the missing one of an odd size.
__global__ void __launch_bounds__(kThreads)
halve_kernel(const uint8_t *__restrict__ src, int w, int h, int c, int ow, int oh, uint8_t *__restrict__ dst)
{
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= ow * oh) return;
    const int x = idx % ow, y = idx / ow;
    const int x1 = min(2 * x + 1, w - 1), y1 = min(2 * y + 1, h - 1);
    const size_t rs = (size_t)w * c;
    const uint8_t *r0 = src + (size_t)(2 * y) * rs, *r1 = src + (size_t)y1 * rs;
    const size_t c0 = (size_t)(2 * x) * c, c1 = (size_t)x1 * c;
    uint8_t *o = dst + (size_t)idx * c;
    for (int k = 0; k < c; ++k) o[k] = (uint8_t)quarter(r0[c0 + k], r0[c1 + k], r1[c0 + k], r1[c1 + k]);
}

// Grey images whose width is a multiple of 8: rows of both images start on 8 bytes, a thread reads 8 bytes of two
// rows and writes 4 pixels in one store.
__global__ void __launch_bounds__(kThreads)
halve_grey8_kernel(const uint8_t *__restrict__ src, int w, int h, int ow, int oh, uint8_t *__restrict__ dst)
{
    const int quads = ow >> 2;
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= quads * oh) return;
    const int q = idx % quads, y = idx / quads;
    const int y1 = min(2 * y + 1, h - 1);
    const uint2 a = *reinterpret_cast<const uint2 *>(src + (size_t)(2 * y) * w + (size_t)q * 8);
    const uint2 b = *reinterpret_cast<const uint2 *>(src + (size_t)y1 * w + (size_t)q * 8);
    const unsigned ra[2] = {a.x, a.y}, rb[2] = {b.x, b.y};
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned wa = ra[k >> 1] >> ((k & 1) * 16), wb = rb[k >> 1] >> ((k & 1) * 16);
        out |= quarter(wa & 255u, (wa >> 8) & 255u, wb & 255u, (wb >> 8) & 255u) << (8 * k);
    }
    *reinterpret_cast<unsigned *>(dst + (size_t)y * ow + (size_t)q * 4) = out;
}

// std::min / std::max of the host code, operand for operand
__device__ __forceinline__ float min_f(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max_f(float a, float b) { return a < b ? b : a; }

// linear_at and feature_view_row of feature_view.h: the same float operations in the same order.
__global__ void __launch_bounds__(kThreads)
view_rows_kernel(const uint8_t *__restrict__ img, int w, int h, int ch, const float *__restrict__ positions, int n,
    uint8_t *__restrict__ colors, float *__restrict__ normalized)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float2 p = reinterpret_cast<const float2 *>(positions)[i];
    const float px = p.x, py = p.y;
    const float x = max_f(0.0f, min_f((float)(w - 1), px));
    const float y = max_f(0.0f, min_f((float)(h - 1), py));
    const int fx = (int)x, fy = (int)y;
    const int fx1 = min(fx + 1, w - 1), fy1 = min(fy + 1, h - 1);
    const float w1 = x - (float)fx, w0 = 1.0f - w1, w3 = y - (float)fy, w2 = 1.0f - w3;
    const size_t rs = (size_t)w * ch, r1 = fy * rs, r2 = fy1 * rs, c1 = (size_t)fx * ch, c2 = (size_t)fx1 * ch;
    uint8_t v[3] = {0, 0, 0};
    for (int cc = 0; cc < ch; ++cc)
        v[cc] = (uint8_t)((float)img[r1 + c1 + cc] * (w0 * w2) + (float)img[r1 + c2 + cc] * (w1 * w2)
            + (float)img[r2 + c1 + cc] * (w0 * w3) + (float)img[r2 + c2 + cc] * (w1 * w3) + 0.5f);
    for (int k = 0; k < 3; ++k) colors[3 * (size_t)i + k] = ch == 3 ? v[k] : v[0];
    const float fw = (float)w, fh = (float)h, fnorm = max_f(fw, fh);
    float2 nrm;
    nrm.x = (px + 0.5f - fw * 0.5f) / fnorm;
    nrm.y = (py + 0.5f - fh * 0.5f) / fnorm;
    reinterpret_cast<float2 *>(normalized)[i] = nrm;
}

// view_mark_row of feature_view.h, one lane per row: three byte gathers (mask, pixel) and 12 bytes written.  A wave
// adds what it counted in one atomic per counter, and only where it counted something.
__global__ void __launch_bounds__(kThreads)
view_marks_kernel(const float *__restrict__ normalized, int n, int n_sift, double pixel_width, const uint8_t *__restrict__ img,
    int w, int h, int ch, const uint8_t *__restrict__ mask, int mask_w, int mask_h, int clamp, int threshold,
    float *__restrict__ pixel_xy, uint8_t *__restrict__ pixel_rgb, uint8_t *__restrict__ mark, int32_t *__restrict__ counts)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    uint8_t m = kMarkIn;
    if (i < n) {
        const float2 p = reinterpret_cast<const float2 *>(normalized)[i];
        float xy[2];
        uint8_t rgb[3];
        view_mark_row(p.x, p.y, pixel_width, img, w, h, ch, mask, mask_w, mask_h, clamp, threshold, xy, &m, rgb);
        float2 o;
        o.x = xy[0]; o.y = xy[1];
        reinterpret_cast<float2 *>(pixel_xy)[i] = o;
        for (int k = 0; k < 3; ++k) pixel_rgb[3 * (size_t)i + k] = rgb[k];
        mark[i] = m;
    }
    const bool out = !(m & kMarkIn);        // lanes past n carry kMarkIn and count nowhere
    const int c0 = __popcll(__ballot(out && i < n_sift)), c1 = __popcll(__ballot(out && i >= n_sift));
    const int c2 = __popcll(__ballot((m & kMarkOutside) != 0));
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(counts + 0, c0);
        if (c1) atomicAdd(counts + 1, c1);
        if (c2) atomicAdd(counts + 2, c2);
    }
}

// One workgroup.  A pass takes kCompactPassRows rows, a thread four neighbours of them; the kept rows of a pass are
// numbered by a scan over the threads (inside a wave by shuffles, across the four waves through LDS) on top of
// what the earlier passes kept, which every thread adds up for itself.  The SIFT rows come first and their passes
// end at n_sift, so that the SURF rows are numbered from the kept SIFT rows on.
constexpr int kCompactPerThread = kCompactPassRows / kThreads;

__global__ void __launch_bounds__(kThreads)
compact_rows_kernel(ViewRows from, int n_sift, int n_surf, ViewRows to, int32_t *__restrict__ index, int32_t *__restrict__ counts)
{
    __shared__ int32_t wave_sum[kThreads / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    int kept = 0, kept_sift = 0;
    for (int part = 0; part < 2; ++part) {
        const int lo = part ? n_sift : 0, hi = part ? n_sift + n_surf : n_sift;
        for (int pass = lo; pass < hi; pass += kCompactPassRows) {
            const int r0 = pass + t * kCompactPerThread;
            bool keep[kCompactPerThread];
            int mine = 0;
#pragma unroll
            for (int k = 0; k < kCompactPerThread; ++k) {
                keep[k] = r0 + k < hi && (from.mark[r0 + k] & kMarkIn);
                mine += keep[k];
            }
            int incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int v = 0; v < kThreads / 64; ++v) { before += v < wave ? wave_sum[v] : 0; total += wave_sum[v]; }
            int dst = kept + before + incl - mine;
#pragma unroll
            for (int k = 0; k < kCompactPerThread; ++k) {
                if (!keep[k]) continue;
                const size_t r = (size_t)(r0 + k), d = (size_t)dst++;
                if (part == 0) to.sift_map[d] = from.sift_map[r];
                else to.surf_map[d - kept_sift] = from.surf_map[r - n_sift];
                reinterpret_cast<float2 *>(to.positions)[d] = reinterpret_cast<const float2 *>(from.positions)[r];
                reinterpret_cast<float2 *>(to.normalized)[d] = reinterpret_cast<const float2 *>(from.normalized)[r];
                reinterpret_cast<float2 *>(to.pixel_xy)[d] = reinterpret_cast<const float2 *>(from.pixel_xy)[r];
                for (int q = 0; q < 3; ++q) { to.colors[3 * d + q] = from.colors[3 * r + q]; to.pixel_rgb[3 * d + q] = from.pixel_rgb[3 * r + q]; }
                to.mark[d] = from.mark[r];
                index[d] = (int32_t)r;
            }
            kept += total;
            __syncthreads();            // wave_sum is written again in the next pass
        }
        if (part == 0) kept_sift = kept;
    }
    if (t == 0) { counts[0] = kept_sift; counts[1] = kept - kept_sift; }
}

// osfm_quantize_sift / osfm_quantize_surf (match_api.hip) for one value
__device__ __forceinline__ int quantize_sift(float v)
{
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    v *= 255.0f;
    v = v > 0.0f ? floorf(v + 0.5f) : ceilf(v - 0.5f);
    return (int)(unsigned char)v;
}

__device__ __forceinline__ int quantize_surf(float v)
{
    v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    v *= 127.0f;
    v = v > 0.0f ? floorf(v + 0.5f) : ceilf(v - 0.5f);
    return (int)(signed char)v;
}

// One wave per row as in prepare_sift_kernel, a lane reads 8 bytes of the float row and writes what that kernel
// writes for the two quantised values.
__global__ void __launch_bounds__(kThreads)
handoff_sift_kernel(const float *__restrict__ desc, const int32_t *__restrict__ map, int n, int npad, int8_t *__restrict__ dst,
    int32_t *__restrict__ corr, int8_t *__restrict__ dst_raw, int32_t *__restrict__ corr_raw, int32_t *__restrict__ flag)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= npad) return;
    int vals[2] = {0, 0};              // pad rows: the zero vector
    if (row < n) {
        const size_t from = map ? (size_t)map[row] : (size_t)row;
        const float2 f = reinterpret_cast<const float2 *>(desc + from * 128)[lane];
        vals[0] = quantize_sift(f.x);
        vals[1] = quantize_sift(f.y);
    }
    int sum = vals[0] + vals[1], vmax = max(vals[0], vals[1]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { sum += __shfl_xor(sum, m); vmax = max(vmax, __shfl_xor(vmax, m)); }
    const bool raw_ok = row < n && vmax <= 127;
    char2 off, raw;
    off.x = (int8_t)(vals[0] - 128); off.y = (int8_t)(vals[1] - 128);
    raw.x = (int8_t)(raw_ok ? vals[0] : 0); raw.y = (int8_t)(raw_ok ? vals[1] : 0);
    reinterpret_cast<char2 *>(dst + (size_t)row * 128)[lane] = off;
    reinterpret_cast<char2 *>(dst_raw + (size_t)row * 128)[lane] = raw;
    if (lane == 0) {
        corr[row] = 128 * (sum - 128 * 128) + (1 << 20) - (row < n ? 0 : (1 << 22));
        corr_raw[row] = raw_ok ? 128 * sum : -(1 << 22);
        if (row < n) flag[row] = vmax > 127 ? 1 : 0;
    }
}

// One workgroup: thread t owns rows [t * seg, (t + 1) * seg); it counts its flags, the counts are summed in
// thread order, and it numbers its rows from its sum.  A row is read and written by its owner alone, so the slots
// may take the flags' place.  n is a view's SIFT rows (65536 at most by default): 256 kB that stay in cache.
__global__ void __launch_bounds__(kThreads)
special_scan_kernel(int32_t *__restrict__ flag_to_slot, int n, int32_t *__restrict__ special_map, int32_t *__restrict__ count)
{
    __shared__ int32_t before[kThreads + 1];
    const int t = threadIdx.x;
    const int seg = (n + kThreads - 1) / kThreads;
    const int lo = min(n, t * seg), hi = min(n, lo + seg);
    int32_t mine = 0;
    for (int i = lo; i < hi; ++i) mine += flag_to_slot[i] != 0;
    before[t + 1] = mine;
    __syncthreads();
    if (t == 0) {
        before[0] = 0;
        for (int k = 1; k <= kThreads; ++k) before[k] += before[k - 1];
        *count = before[kThreads];
    }
    __syncthreads();
    int32_t next = before[t];
    for (int i = lo; i < hi; ++i) {
        if (flag_to_slot[i]) { special_map[next] = i; flag_to_slot[i] = next++; }
        else flag_to_slot[i] = -1;
    }
}

// One wave per row as in prepare_surf_kernel, kSurfRowsPerWave rows in turn: the largest norm has one address, and an
// atomic per row on it took 240 us for 21k rows, all of it waiting in line.  A workgroup folds its 32 rows first and
// asks only if it has something to add (the maximum only grows).
constexpr int kSurfRowsPerWave = 8;

__global__ void __launch_bounds__(kThreads)
handoff_surf_kernel(const float *__restrict__ desc, const int32_t *__restrict__ map, int n, int npad, int8_t *__restrict__ dst,
    int32_t *__restrict__ corr, int32_t *__restrict__ norm2max)
{
    __shared__ int32_t wave_max[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + wave) * kSurfRowsPerWave;
    int best = 0;
    for (int row = row0; row < min(row0 + kSurfRowsPerWave, npad); ++row) {
        int v = 0;
        if (row < n) {
            const size_t from = map ? (size_t)map[row] : (size_t)row;
            v = quantize_surf(desc[from * 64 + lane]);
        }
        dst[(size_t)row * 64 + lane] = (int8_t)v;
        int sq = v * v;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sq += __shfl_xor(sq, m);
        if (lane == 0) corr[row] = row < n ? 0 : -(1 << 22);     // padding rows lose every comparison
        best = max(best, sq);                                    // padding rows: 0, which adds nothing
    }
    if (lane == 0) wave_max[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
        if (best > __atomic_load_n(norm2max, __ATOMIC_RELAXED)) atomicMax(norm2max, best);
    }
}

}  // namespace

void launch_halve(hipStream_t s, const uint8_t *src, int w, int h, int c, uint8_t *dst)
{
    const int ow = (w + 1) >> 1, oh = (h + 1) >> 1;
    if (c == 1 && (w & 7) == 0) {
        const int work = (ow >> 2) * oh;
        hipLaunchKernelGGL(halve_grey8_kernel, dim3((work + kThreads - 1) / kThreads), dim3(kThreads), 0, s, src, w, h, ow, oh, dst);
        return;
    }
    hipLaunchKernelGGL(halve_kernel, dim3((ow * oh + kThreads - 1) / kThreads), dim3(kThreads), 0, s, src, w, h, c, ow, oh, dst);
}

void launch_view_rows(hipStream_t s, const uint8_t *img, int w, int h, int c, const float *positions, int n, uint8_t *colors,
    float *normalized)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(view_rows_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, img, w, h, c, positions, n,
        colors, normalized);
}

void launch_view_marks(hipStream_t s, const float *normalized, int n, int n_sift, double pixel_width, const uint8_t *img, int w,
    int h, int c, const uint8_t *mask, int mask_w, int mask_h, int clamp, int threshold, float *pixel_xy, uint8_t *pixel_rgb,
    uint8_t *mark, int32_t *counts)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(view_marks_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, normalized, n, n_sift,
        pixel_width, img, w, h, c, mask, mask_w, mask_h, clamp, threshold, pixel_xy, pixel_rgb, mark, counts);
}

void launch_compact_rows(hipStream_t s, const ViewRows &from, int n_sift, int n_surf, const ViewRows &to, int32_t *index,
    int32_t *counts)
{
    hipLaunchKernelGGL(compact_rows_kernel, dim3(1), dim3(kThreads), 0, s, from, n_sift, n_surf, to, index, counts);
}

void launch_handoff_sift(hipStream_t s, const float *desc, const int32_t *map, int n, int npad, int8_t *dst, int32_t *corr,
    int8_t *dst_raw, int32_t *corr_raw, int32_t *flag)
{
    if (npad <= 0) return;
    hipLaunchKernelGGL(handoff_sift_kernel, dim3((npad + 3) / 4), dim3(kThreads), 0, s, desc, map, n, npad, dst, corr, dst_raw,
        corr_raw, flag);
}

void launch_special_scan(hipStream_t s, int32_t *flag_to_slot, int n, int32_t *special_map, int32_t *count)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(special_scan_kernel, dim3(1), dim3(kThreads), 0, s, flag_to_slot, n, special_map, count);
}

void launch_handoff_surf(hipStream_t s, const float *desc, const int32_t *map, int n, int npad, int8_t *dst, int32_t *corr,
    int32_t *norm2max)
{
    if (npad <= 0) return;
    const int rows_per_block = 4 * kSurfRowsPerWave;
    hipLaunchKernelGGL(handoff_surf_kernel, dim3((npad + rows_per_block - 1) / rows_per_block), dim3(kThreads), 0, s, desc, map, n,
        npad, dst, corr, norm2max);
}

}  // namespace view
}  // namespace osfm
