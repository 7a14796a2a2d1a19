// SURF extraction on the device, following MVE's sfm/surf.cc (see surf_kernels.h).
//
// Equality with the reference's bytes rests on the same things as the SIFT stages': every float and double
// operation below is the reference's, in its order and type (the library is built with -ffp-contract=off and
// without fast-math; HIP's division and square root are correctly rounded); whatever the reference takes from
// the C library arrives from the host; and candidates and keypoints are compacted by a scan, in the reference's
// order (octave, sample, y, x).  The summed-area table is integer, so it has no order to keep.  No atomics:
// the same bytes on every run.
#include "surf_kernels.h"

namespace osfm {
namespace surf {

namespace {

constexpr double kPi = 3.14159265358979323846264338327950288;

// ----------------------------------------------------------------------------- summed-area table

__device__ inline uint32_t grey_at(const uint8_t *px, size_t i, int channels)
{
    if (channels == 1) return px[i];
    // desaturate_lightness on bytes: (unsigned char)(max * 0.5f + min * 0.5f + 0.5f), exact in float
    const uint8_t *v = px + 3 * i;
    const int r = v[0], g = v[1], b = v[2];
    const int hi = max(max(r, g), b), lo = min(min(r, g), b);
    return (uint32_t)((float)hi * 0.5f + (float)lo * 0.5f + 0.5f);
}

// Row sums: one workgroup per row, kBlock pixels at a time with a carry.
__global__ __launch_bounds__(kBlock) void sat_rows_kernel(const uint8_t *px, int w, int channels, Sat *sat)
{
    __shared__ uint32_t wave_total[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.x * w;
    uint32_t carry = 0;
    for (int base = 0; base < w; base += kBlock) {
        const int x = base + (int)threadIdx.x;
        uint32_t v = x < w ? grey_at(px, row + x, channels) : 0u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(v, off);
            if (lane >= off) v += t;
        }
        if (lane == 63) wave_total[wave] = v;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i) {
            if (i < wave) before += wave_total[i];
            total += wave_total[i];
        }
        if (x < w) sat[row + x] = carry + before + v;
        carry += total;
        __syncthreads();
    }
}

// Column sums in place: one lane per column, eight rows' loads in flight ahead of their adds.
__global__ __launch_bounds__(kBlock) void sat_cols_kernel(Sat *sat, int w, int h)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= w) return;
    Sat *p = sat + x;
    uint32_t acc = 0;
    int y = 0;
    for (; y + 8 <= h; y += 8) {
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[(size_t)(y + i) * w];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc += v[i];
            p[(size_t)(y + i) * w] = acc;
        }
    }
    for (; y < h; ++y) {
        acc += p[(size_t)y * w];
        p[(size_t)y * w] = acc;
    }
}

// ----------------------------------------------------------------------------- response maps

// Surf::filter_dxx / filter_dyy / filter_dxy: modular sums of the reference's taps, exact as int32.
__device__ inline int32_t filter_dxx(const Sat *sat, int w, int fs, int x, int y)
{
    const int fs2 = fs / 2;
    const Sat *r1 = sat + ((x - fs - fs2 - 1) + (long long)w * (y - fs));
    const Sat *r2 = r1 + (long long)w * (fs + fs - 1);
    const uint32_t v0 = r1[0], v1 = r1[fs], v2 = r1[2 * fs], v3 = r1[3 * fs];
    const uint32_t v4 = r2[0], v5 = r2[fs], v6 = r2[2 * fs], v7 = r2[3 * fs];
    uint32_t ret = 0;
    ret += v5 + v0 - v4 - v1;
    ret -= 2u * (v6 + v1 - v5 - v2);
    ret += v7 + v2 - v6 - v3;
    return (int32_t)ret;
}

__device__ inline int32_t filter_dyy(const Sat *sat, int w, int fs, int x, int y)
{
    const int fs2 = fs / 2;
    const Sat *r1 = sat + ((x - fs) + (long long)w * (y - fs - fs2 - 1));
    const Sat *r2 = r1 + (long long)w * fs, *r3 = r2 + (long long)w * fs, *r4 = r3 + (long long)w * fs;
    const int e = fs + fs - 1;
    const uint32_t v0 = r1[0], v1 = r2[0], v2 = r3[0], v3 = r4[0];
    const uint32_t v4 = r1[e], v5 = r2[e], v6 = r3[e], v7 = r4[e];
    uint32_t ret = 0;
    ret += v5 + v0 - v1 - v4;
    ret -= 2u * (v6 + v1 - v2 - v5);
    ret += v7 + v2 - v3 - v6;
    return (int32_t)ret;
}

__device__ inline int32_t filter_dxy(const Sat *sat, int w, int fs, int x, int y)
{
    const Sat *r1 = sat + ((x - fs - 1) + (long long)w * (y - fs - 1));
    const Sat *r2 = r1 + (long long)w * fs, *r3 = r2 + w, *r4 = r3 + (long long)w * fs;
    uint32_t ret = 0;
    ret += r2[fs] + r1[0] - r2[0] - r1[fs];
    ret -= r2[fs + fs + 1] + r1[fs + 1] - r2[fs + 1] - r1[fs + fs + 1];
    ret -= r4[fs] + r3[0] - r4[0] - r3[fs];
    ret += r4[fs + fs + 1] + r3[fs + 1] - r4[fs + 1] - r3[fs + fs + 1];
    return (int32_t)ret;
}

// Surf::create_response_map for the four samples of one octave: one lane per sample position.
__global__ __launch_bounds__(kBlock) void response_kernel(const Sat *sat, int w, int h, int octave, OctaveFilters f,
    float *maps, int ow, int oh)
{
    const long long n = (long long)ow * oh;
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int x = (int)(p % ow) << octave, y = (int)(p / ow) << octave;
    const float weight = 0.912f;
#pragma unroll
    for (int k = 0; k < kSamples; ++k) {
        const int fs = f.fs[k];
        const int border = fs + fs / 2 + 1;
        float r = 0.0f;
        if (!(x < border || x + border >= w || y < border || y + border >= h)) {
            const float dxx_t = (float)filter_dxx(sat, w, fs, x, y) * f.inv_karea[k];
            const float dyy_t = (float)filter_dyy(sat, w, fs, x, y) * f.inv_karea[k];
            const float dxy_t = (float)filter_dxy(sat, w, fs, x, y) * f.inv_karea[k];
            r = dxx_t * dyy_t - weight * dxy_t * dxy_t;
        }
        maps[(size_t)k * n + p] = r;
    }
}

// ----------------------------------------------------------------------------- extrema

// Surf::extrema_detection / check_maximum: the strict row test first, then any of the 26 neighbours with >=
// rejects.  Rows 0 and oh - 1 of samples 1 and 2 are zero (the border exceeds the step), so the row test never
// passes there and the rows above and below are never read.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void extrema_kernel(const float *m0, const float *m1, const float *m2, int ow, int oh,
    int block_base, int32_t *counts, const int32_t *offsets, Keypoint *out, int capacity, float octave, float sample)
{
    const int iw = ow - 2;
    const long long n = (long long)iw * oh;
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool flag = false;
    int x = 0, y = 0;
    if (p < n) {
        y = (int)(p / iw);
        x = 1 + (int)(p % iw);
        const size_t idx = (size_t)y * ow + x;
        const float c = m1[idx];
        if (c > m1[idx - 1] && c > m1[idx + 1] && y > 0 && y < oh - 1) {
            const float *layer[3] = {m1, m0, m2};
            bool largest = true;
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (l == 0 && dy == 0 && dx == 0) continue;
                        if (layer[l][idx + (long long)dy * ow + dx] >= c) largest = false;
                    }
            flag = largest;
        }
    }
    int total;
    const int rank = detect::block_rank(flag, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[block_base + blockIdx.x] = total;
    } else if (flag) {
        const int slot = offsets[block_base + blockIdx.x] + rank;
        if (slot < capacity) out[slot] = Keypoint{octave, sample, (float)x, (float)y};
    }
}

// ----------------------------------------------------------------------------- localisation

// Surf::keypoint_localization for one candidate per lane: one Newton step in double from float neighbours.
__global__ __launch_bounds__(kBlock) void localise_kernel(MapsView mv, float contrast_threshold, int width, int height,
    const Keypoint *cand, int n, Keypoint *out, uint8_t *keep, int32_t *counts)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const Keypoint c = cand[i];
        const int o = (int)c.octave, sample = (int)c.sample;
        const int w = mv.ow[o];
        const size_t plane = (size_t)w * mv.oh[o];
        const long long off = (int)c.x + (long long)(int)c.y * w;
        const float *s0 = mv.maps + mv.offset[o] + (size_t)(sample - 1) * plane + off, *s1 = s0 + plane, *s2 = s1 + plane;
#define N9(S) const float S##_0 = S[-1 - w], S##_1 = S[-w], S##_2 = S[1 - w], S##_3 = S[-1], S##_4 = S[0], S##_5 = S[1], \
        S##_6 = S[w - 1], S##_7 = S[w], S##_8 = S[1 + w]
        N9(s0); N9(s1); N9(s2);
#undef N9
        (void)s0_0; (void)s0_2; (void)s0_6; (void)s0_8; (void)s2_0; (void)s2_2; (void)s2_6; (void)s2_8;
        const double b0 = -(s1_5 - s1_3) * 0.5;
        const double b1 = -(s1_7 - s1_1) * 0.5;
        const double b2 = -(s2_4 - s0_4) * 0.5;
        double m[9];
        m[0] = s1_3 - 2.0 * s1_4 + s1_5;
        m[1] = (s1_8 - s1_6 - s1_2 + s1_0) * 0.25;
        m[2] = (s2_5 - s2_3 - s0_5 + s0_3) * 0.25;
        m[3] = m[1];
        m[4] = s1_1 - 2.0 * s1_4 + s1_7;
        m[5] = (s2_7 - s2_1 - s0_7 + s0_1) * 0.25;
        m[6] = m[2];
        m[7] = m[5];
        m[8] = s0_4 - 2.0 * s1_4 + s2_4;
        // math::matrix_determinant / matrix_inverse, in their operation order
        const double det = m[0] * m[4] * m[8] + m[1] * m[5] * m[6] + m[2] * m[3] * m[7]
            - m[2] * m[4] * m[6] - m[1] * m[3] * m[8] - m[0] * m[5] * m[7];
        Keypoint k = c;
        if (!((0.0f - 1.0e-5f) <= det && det <= (0.0f + 1.0e-5f))) {
            double inv[9];
            inv[0] = m[4] * m[8] - m[5] * m[7];
            inv[1] = m[2] * m[7] - m[1] * m[8];
            inv[2] = m[1] * m[5] - m[2] * m[4];
            inv[3] = m[5] * m[6] - m[3] * m[8];
            inv[4] = m[0] * m[8] - m[2] * m[6];
            inv[5] = m[2] * m[3] - m[0] * m[5];
            inv[6] = m[3] * m[7] - m[4] * m[6];
            inv[7] = m[1] * m[6] - m[0] * m[7];
            inv[8] = m[0] * m[4] - m[1] * m[3];
#pragma unroll
            for (int j = 0; j < 9; ++j) inv[j] = inv[j] / det;
            const double x0 = 0.0 + inv[0] * b0 + inv[1] * b1 + inv[2] * b2;
            const double x1 = 0.0 + inv[3] * b0 + inv[4] * b1 + inv[5] * b2;
            const double x2 = 0.0 + inv[6] * b0 + inv[7] * b1 + inv[8] * b2;
            const double hi = fmax(fmax(x0, x1), x2), lo = fmin(fmin(x0, x1), x2);
            if (!(hi > 0.5 || lo < -0.5f)) {
                const float dog_value = (float)(s1_4 - 0.5 * (0.0 + b0 * x0 + b1 * x1 + b2 * x2));
                if (!(dog_value < contrast_threshold)) {
                    const float sampling = (float)(1 << o);
                    k.x = (float)((c.x + x0) * sampling);
                    k.y = (float)((c.y + x1) * sampling);
                    k.sample = (float)(c.sample + x2);
                    ok = !(k.x < 0.0f || k.x + 1.0f > (float)width || k.y < 0.0f || k.y + 1.0f > (float)height);
                }
            }
        }
        out[i] = k;
        keep[i] = ok ? 1 : 0;
    }
    int total;
    (void)detect::block_rank(ok, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ----------------------------------------------------------------------------- Haar responses

// Surf::filter_dx_dy: the numerators, exact as int32.  GUARD: a tap outside the table reads as zero and sets
// *guarded (only non-finite input of the describe hook gets there); otherwise every tap is inside.
template <bool GUARD>
__device__ inline void haar(const Sat *sat, int w, long long size, int x, int y, int fs, int32_t *dx, int32_t *dy,
    bool *guarded)
{
    const long long xb = (x - fs - 1) + (long long)(y - fs - 1) * w;
    const long long yb = (x - fs - 1) + (long long)(y - 1) * w;
    const long long lower = xb + (long long)w * (2 * fs + 1);
    auto tap = [&](long long i) -> uint32_t {
        if (GUARD && (i < 0 || i >= size)) {
            *guarded = true;
            return 0u;
        }
        return sat[i];
    };
    const uint32_t x1 = tap(xb), x2 = tap(xb + fs), x3 = tap(xb + fs + 1), x4 = tap(xb + 2 * fs + 1);
    const uint32_t x5 = tap(lower), x6 = tap(lower + fs), x7 = tap(lower + fs + 1), x8 = tap(lower + 2 * fs + 1);
    const uint32_t y1 = tap(yb), y2 = tap(yb + 2 * fs + 1), y3 = tap(yb + w), y4 = tap(yb + w + 2 * fs + 1);
    *dx = (int32_t)((x8 + x2 - x4 - x6) - (x7 + x1 - x3 - x5));
    *dy = (int32_t)((x8 + y1 - x5 - y2) - (y4 + x1 - y3 - x4));
}

// ----------------------------------------------------------------------------- orientation

// Surf::descriptor_orientation for one keypoint per workgroup: 109 lanes fetch the weighted Haar responses and
// their angles, 16 lanes add up one window each in sample order, lane 0 takes the first longest window.  The
// angle is atan2 in double rounded to float, where the reference calls the C library's atan2f.
__global__ __launch_bounds__(128) void orientation_kernel(const Sat *sat, int w, int h, const OriTable *table,
    const OriJob *jobs, OriResult *out)
{
    __shared__ float s_dx[kOriSamples], s_dy[kOriSamples], s_ang[kOriSamples];
    __shared__ double s_len[kWindows], s_sx[kWindows], s_sy[kWindows];
    const OriJob job = jobs[blockIdx.x];
    const int t = threadIdx.x;
    const int spacing = 8 * job.scale + 1;
    if (job.x < spacing || job.y < spacing || job.x + spacing >= w || job.y + spacing >= h) {
        if (t == 0) out[blockIdx.x] = OriResult{0.0, 0.0, 0, 0};
        return;
    }
    if (t < kOriSamples) {
        const int fs = 2 * job.scale;
        int32_t idx, idy;
        haar<false>(sat, w, 0, job.x + table->rx[t] * job.scale, job.y + table->ry[t] * job.scale, fs, &idx, &idy, nullptr);
        const float norm = (float)((2 * fs + 1) * fs * (fs + 1));
        float dx = (float)idx / norm, dy = (float)idy / norm;
        dx *= table->gauss[t];
        dy *= table->gauss[t];
        s_dx[t] = dx;
        s_dy[t] = dy;
        s_ang[t] = (float)atan2((double)dy, (double)dx);
    }
    __syncthreads();
    if (t < kWindows) {
        const double inc = kPi / 8.0, half = kPi / 6.0;
        double deg = -kPi;
        for (int j = 0; j < t; ++j) deg += inc;
        const double win_start = deg - half, win_end = deg + half;
        double sum_dx = 0.0, sum_dy = 0.0;
        for (int i = 0; i < kOriSamples; ++i) {
            const double a = s_ang[i], ap = a + 2.0 * kPi, am = a - 2.0 * kPi;
            if ((a > win_start && a < win_end) || (ap > win_start && ap < win_end) || (am > win_start && am < win_end)) {
                sum_dx += s_dx[i];
                sum_dy += s_dy[i];
            }
        }
        s_sx[t] = sum_dx;
        s_sy[t] = sum_dy;
        s_len[t] = sum_dx * sum_dx + sum_dy * sum_dy;
    }
    __syncthreads();
    if (t == 0) {
        OriResult r{0.0, 0.0, 1, 0};
        double best = 0.0;
        for (int k = 0; k < kWindows; ++k)
            if (s_len[k] > best) {
                r.best_dx = s_sx[k];
                r.best_dy = s_sy[k];
                best = s_len[k];
            }
        out[blockIdx.x] = r;
    }
}

// ----------------------------------------------------------------------------- descriptor

// Surf::descriptor_computation for one job per workgroup: 400 lanes compute the weighted, rotated responses of
// their sample, 64 lanes add the 25 terms of their (cell, bin) sequentially in float in (y, x) order, lane 0 sums
// the squares in order.
__global__ __launch_bounds__(kDescBlock) void descriptor_kernel(const Sat *sat, int w, int h, const float *weights,
    const DescJob *jobs, float *out, int32_t *status)
{
    __shared__ float s_v[4][400];
    __shared__ float s_d[64];
    __shared__ float s_norm;
    const DescJob job = jobs[blockIdx.x];
    const int t = threadIdx.x;
    const float spacing = (float)(15 * job.scale + 1);
    if (job.x < spacing || job.y < spacing || job.x + spacing >= (float)w || job.y + spacing > (float)h) {
        if (t == 0) status[blockIdx.x] = 0;
        if (t < 64) out[(size_t)blockIdx.x * 64 + t] = 0.0f;
        return;
    }
    bool guarded = false;
    if (t < 400) {
        const int y = t / 20 - 10, x = t % 20 - 10;
        const float fx = (float)x + 0.5f, fy = (float)y + 0.5f, fscale = (float)job.scale;
        const float px = job.x + (job.cos_ori * fx - job.sin_ori * fy) * fscale;
        const float py = job.y + (job.sin_ori * fx + job.cos_ori * fy) * fscale;
        // math::round
        const int rot_x = (int)(px > 0.0f ? floorf(px + 0.5f) : ceilf(px - 0.5f));
        const int rot_y = (int)(py > 0.0f ? floorf(py + 0.5f) : ceilf(py - 0.5f));
        int32_t idx, idy;
        haar<true>(sat, w, (long long)w * h, rot_x, rot_y, job.scale, &idx, &idy, &guarded);
        const float norm = (float)((2 * job.scale + 1) * job.scale * (job.scale + 1));
        const float dx = (float)idx / norm, dy = (float)idy / norm;
        const float ori_dx = job.cos_ori * dx + job.sin_ori * dy;
        const float ori_dy = -job.sin_ori * dx + job.cos_ori * dy;
        const float weight = weights[t];
        s_v[0][t] = weight * ori_dx;
        s_v[1][t] = weight * ori_dy;
        s_v[2][t] = weight * fabsf(ori_dx);
        s_v[3][t] = weight * fabsf(ori_dy);
    }
    const int any_guarded = __syncthreads_or(guarded ? 1 : 0);
    if (t < 64) {
        const int bin = t & 3, cx = (t >> 2) & 3, cy = t >> 4;
        float acc = 0.0f;
        for (int yy = 0; yy < 5; ++yy)
            for (int xx = 0; xx < 5; ++xx) acc += s_v[bin][(cy * 5 + yy) * 20 + cx * 5 + xx];
        s_d[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        float norm = 0.0f;
        for (int j = 0; j < 64; ++j) norm = norm + s_d[j] * s_d[j];
        s_norm = norm;
    }
    __syncthreads();
    const float norm = s_norm;
    const bool small = (0.0f - 1e-8) <= norm && norm <= (0.0f + 1e-8);
    if (t == 0) status[blockIdx.x] = small ? 0 : any_guarded ? 2 : 1;
    if (t < 64) out[(size_t)blockIdx.x * 64 + t] = small ? 0.0f : s_d[t] / sqrtf(norm);
}

}  // namespace

// ----------------------------------------------------------------------------- launchers

void launch_sat(hipStream_t s, const uint8_t *pixels, int w, int h, int channels, Sat *sat)
{
    hipLaunchKernelGGL(sat_rows_kernel, dim3(h), dim3(kBlock), 0, s, pixels, w, channels, sat);
    hipLaunchKernelGGL(sat_cols_kernel, dim3((w + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sat, w, h);
}

void launch_response(hipStream_t s, const Sat *sat, int w, int h, int octave, OctaveFilters f, float *maps, int ow, int oh)
{
    const long long n = (long long)ow * oh;
    hipLaunchKernelGGL(response_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, sat, w, h, octave, f,
        maps, ow, oh);
}

void launch_extrema(hipStream_t s, const float *m0, const float *m1, const float *m2, int ow, int oh, int block_base,
    int32_t *counts, const int32_t *offsets, Keypoint *out, int capacity, float octave, float sample)
{
    const int blocks = extrema_blocks(ow, oh);
    if (!blocks) return;
    if (!offsets)
        hipLaunchKernelGGL(extrema_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, m0, m1, m2, ow, oh, block_base, counts, offsets,
            out, capacity, octave, sample);
    else
        hipLaunchKernelGGL(extrema_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, m0, m1, m2, ow, oh, block_base, counts, offsets,
            out, capacity, octave, sample);
}

void launch_localise(hipStream_t s, MapsView maps, float contrast_threshold, int width, int height, const Keypoint *cand,
    int n, Keypoint *out, uint8_t *keep, int32_t *counts)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(localise_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, maps, contrast_threshold, width,
        height, cand, n, out, keep, counts);
}

void launch_orientation(hipStream_t s, const Sat *sat, int w, int h, const OriTable *table, const OriJob *jobs, int n,
    OriResult *out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(orientation_kernel, dim3(n), dim3(128), 0, s, sat, w, h, table, jobs, out);
}

void launch_descriptor(hipStream_t s, const Sat *sat, int w, int h, const float *weights, const DescJob *jobs, int n,
    float *out, int32_t *status)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(descriptor_kernel, dim3(n), dim3(kDescBlock), 0, s, sat, w, h, weights, jobs, out, status);
}

}  // namespace surf
}  // namespace osfm
