// SIFT extraction on the device, following MVE's sfm/sift.cc (see sift_kernels.h).
//
// Equality with the reference's bytes up to the localised keypoints rests on three things: every float32
// operation below is the reference's, in its order (the library is built with -ffp-contract=off and without
// fast-math, and HIP's float division and square root are correctly rounded); the Gaussian weights arrive
// from the host, where the C library's expf made them; and candidates are compacted by a scan, in the
// reference's order (octave, sample, y, x).  Orientation histograms and descriptors are accumulated in double,
// in per-lane partial bins that a fixed loop adds up: no atomics, the same bytes on every run.
#include "sift_kernels.h"

namespace osfm {
namespace sift {

using detect::block_rank;

namespace {

constexpr double kPi = 3.14159265358979323846264338327950288;
constexpr double kSqrt2 = 1.41421356237309504880168872420969808;

// ----------------------------------------------------------------------------- scale space

__global__ __launch_bounds__(kBlock) void to_float_kernel(const uint8_t *px, int n, int channels, float *out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (channels == 1) {
        out[i] = fminf(1.0f, fmaxf(0.0f, (float)px[i] / 255.0f));
        return;
    }
    // byte_to_float_image per channel, then desaturate_average: v0 * third + v1 * third + v2 * third
    const float third = 1.0f / 3.0f;
    const float v0 = fminf(1.0f, fmaxf(0.0f, (float)px[3 * (size_t)i] / 255.0f));
    const float v1 = fminf(1.0f, fmaxf(0.0f, (float)px[3 * (size_t)i + 1] / 255.0f));
    const float v2 = fminf(1.0f, fmaxf(0.0f, (float)px[3 * (size_t)i + 2] / 255.0f));
    out[i] = v0 * third + v1 * third + v2 * third;
}

// rescale_double_size_supersample: the four neighbours at a quarter each, the last row and column repeated
__global__ __launch_bounds__(kBlock) void double_size_kernel(const float *in, int iw, int ih, float *out)
{
    const int ow = iw << 1, oh = ih << 1;
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x >= ow || y >= oh) return;
    const int y0 = y >> 1, y1 = (y + (y + 1 < oh ? 1 : 0)) >> 1;
    const int x0 = x >> 1, x1 = (x + (x + 1 < ow ? 1 : 0)) >> 1;
    const float a = in[(size_t)y0 * iw + x0], b = in[(size_t)y0 * iw + x1];
    const float c = in[(size_t)y1 * iw + x0], d = in[(size_t)y1 * iw + x1];
    out[(size_t)y * ow + x] = a * 0.25f + b * 0.25f + c * 0.25f + d * 0.25f;
}

// rescale_half_size_gaussian: 4 x 4 taps with clamped indices, accumulated row by row
__global__ __launch_bounds__(kBlock) void half_size_kernel(const float *in, int iw, int ih, float *out, float w1, float w2,
    float w3)
{
    const int ow = (iw + 1) >> 1, oh = (ih + 1) >> 1;
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    if (x >= ow || y >= oh) return;
    const int y2 = y << 1, x2 = x << 1;
    const int ry[4] = {max(0, y2 - 1), y2, min(ih - 1, y2 + 1), min(ih - 1, y2 + 2)};
    const int cx[4] = {max(0, x2 - 1), x2, min(iw - 1, x2 + 1), min(iw - 1, x2 + 2)};
    const float wt[4][4] = {{w3, w2, w2, w3}, {w2, w1, w1, w2}, {w2, w1, w1, w2}, {w3, w2, w2, w3}};
    float v = 0.0f, ws = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v += in[(size_t)ry[r] * iw + cx[c]] * wt[r][c];
            ws += wt[r][c];
        }
    out[(size_t)y * ow + x] = v / ws;
}

// blur_gaussian, x pass: a row segment of kBlock pixels with its halo in LDS, the halo indices clamped to the row
// (a radius beyond the image repeats the border pixel, as the reference's clamp does)
__global__ __launch_bounds__(kBlock) void blur_rows_kernel(const float *in, float *out, int w, int h, BlurWeights wt)
{
    __shared__ float tile[kBlock + 2 * kMaxRadius];
    const int ks = wt.ks;
    const int x0 = blockIdx.x * kBlock, y = blockIdx.y;
    const float *row = in + (size_t)y * w;
    for (int t = threadIdx.x; t < kBlock + 2 * ks; t += kBlock) tile[t] = row[min(max(x0 - ks + t, 0), w - 1)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    float v = 0.0f, ws = 0.0f;
    for (int i = -ks; i <= ks; ++i) {
        const float k = wt.w[i < 0 ? -i : i];
        v += tile[threadIdx.x + ks + i] * k;
        ws += k;
    }
    out[(size_t)y * w + x] = v / ws;
}

// blur_gaussian, y pass, on a tile of 32 x 32 outputs with its halo rows in LDS; the DoG image is the result minus `base`
constexpr int kColTile = 32;
__global__ __launch_bounds__(kBlock) void blur_cols_kernel(const float *in, float *out, const float *base, float *dog, int w,
    int h, BlurWeights wt)
{
    __shared__ float tile[kColTile + 2 * kMaxRadius][kColTile + 1];
    const int ks = wt.ks;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = blockIdx.x * kColTile, y0 = blockIdx.y * kColTile;
    const int gx = min(x0 + tx, w - 1);
    for (int r = ty; r < kColTile + 2 * ks; r += kBlock / 32)
        tile[r][tx] = in[(size_t)min(max(y0 - ks + r, 0), h - 1) * w + gx];
    __syncthreads();
    const int x = x0 + tx;
    if (x >= w) return;
    for (int j = ty; j < kColTile; j += kBlock / 32) {
        const int y = y0 + j;
        if (y >= h) break;
        float v = 0.0f, ws = 0.0f;
        for (int i = -ks; i <= ks; ++i) {
            const float k = wt.w[i < 0 ? -i : i];
            v += tile[j + ks + i][tx] * k;
            ws += k;
        }
        const float r = v / ws;
        const size_t p = (size_t)y * w + x;
        out[p] = r;
        if (dog) dog[p] = r - base[p];
    }
}

// ----------------------------------------------------------------------------- extrema

// Strict 26-neighbour extrema of the interior pixels, one thread per pixel in (y, x) order.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void extrema_kernel(const float *d0, const float *d1, const float *d2, int w, int h,
    int block_base, int32_t *counts, const int32_t *offsets, Keypoint *out, int capacity, float octave, float sample)
{
    const int iw = w - 2;
    const long long n = (long long)iw * (h - 2);
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool flag = false;
    int x = 0, y = 0;
    if (p < n) {
        y = 1 + (int)(p / iw);
        x = 1 + (int)(p % iw);
        const size_t idx = (size_t)y * w + x;
        const float c = d1[idx];
        const float *layer[3] = {d0, d1, d2};
        bool largest = true, smallest = true;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (l == 1 && dy == 0 && dx == 0) continue;
                    const float v = layer[l][idx + (long long)dy * w + dx];
                    if (v >= c) largest = false;
                    if (v <= c) smallest = false;
                }
        flag = largest || smallest;
    }
    int total;
    const int rank = block_rank(flag, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[block_base + blockIdx.x] = total;
    } else if (flag) {
        const int slot = offsets[block_base + blockIdx.x] + rank;
        if (slot < capacity) out[slot] = Keypoint{octave, sample, (float)x, (float)y};
    }
}

// ----------------------------------------------------------------------------- localisation

// Sift::keypoint_localization for one candidate per lane.  keep[i] tells whether it passed the ten rejection tests;
// counts[block] is the number kept in the workgroup, for the compaction that follows.
__global__ __launch_bounds__(kBlock) void localise_kernel(PyramidView pyr, LocaliseParams prm, const Keypoint *cand, int n,
    Keypoint *out, uint8_t *keep, int32_t *counts)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const Keypoint c = cand[i];
        const int oi = (int)c.octave - pyr.min_octave;
        const OctaveView &o = pyr.oct[oi];
        const int w = o.w, h = o.h;
        const int is = (int)c.sample;
        const size_t plane = (size_t)w * h;
        const float *d0 = o.dog + (size_t)is * plane, *d1 = d0 + plane, *d2 = d1 + plane;
        int ix = (int)c.x, iy = (int)c.y;
        float fx = 0.0f, fy = 0.0f, fs = 0.0f;
        float Dx = 0.0f, Dy = 0.0f, Ds = 0.0f, Dxx = 0.0f, Dyy = 0.0f, Dss = 0.0f, Dxy = 0.0f, Dxs = 0.0f, Dys = 0.0f;
        for (int j = 0; j < 5; ++j) {
            const long long px = (long long)iy * w + ix;
#define AT(D, OFF) ((D)[px + (OFF)])
            Dx = (AT(d1, 1) - AT(d1, -1)) * 0.5f;
            Dy = (AT(d1, w) - AT(d1, -w)) * 0.5f;
            Ds = (AT(d2, 0) - AT(d0, 0)) * 0.5f;
            Dxx = AT(d1, 1) + AT(d1, -1) - 2.0f * AT(d1, 0);
            Dyy = AT(d1, w) + AT(d1, -w) - 2.0f * AT(d1, 0);
            Dss = AT(d2, 0) + AT(d0, 0) - 2.0f * AT(d1, 0);
            Dxy = (AT(d1, 1 + w) + AT(d1, -1 - w) - AT(d1, -1 + w) - AT(d1, 1 - w)) * 0.25f;
            Dxs = (AT(d2, 1) + AT(d0, -1) - AT(d2, -1) - AT(d0, 1)) * 0.25f;
            Dys = (AT(d2, w) + AT(d0, -w) - AT(d2, -w) - AT(d0, w)) * 0.25f;
#undef AT
            const float m[9] = {Dxx, Dxy, Dxs, Dxy, Dyy, Dys, Dxs, Dys, Dss};
            // math::matrix_determinant / matrix_inverse, in their operation order
            const float det = m[0] * m[4] * m[8] + m[1] * m[5] * m[6] + m[2] * m[3] * m[7]
                - m[2] * m[4] * m[6] - m[1] * m[3] * m[8] - m[0] * m[5] * m[7];
            if ((0.0f - 1e-15f) <= det && det <= (0.0f + 1e-15f)) {
                fx = fy = fs = 0.0f;
                break;
            }
            float inv[9];
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
            for (int k = 0; k < 9; ++k) inv[k] = inv[k] / det;
            const float b0 = -Dx, b1 = -Dy, b2 = -Ds;
            fx = 0.0f + inv[0] * b0 + inv[1] * b1 + inv[2] * b2;
            fy = 0.0f + inv[3] * b0 + inv[4] * b1 + inv[5] * b2;
            fs = 0.0f + inv[6] * b0 + inv[7] * b1 + inv[8] * b2;
            const int dx = (fx > 0.6f && ix < w - 2 ? 1 : 0) + (fx < -0.6f && ix > 1 ? -1 : 0);
            const int dy = (fy > 0.6f && iy < h - 2 ? 1 : 0) + (fy < -0.6f && iy > 1 ? -1 : 0);
            if (dx != 0 || dy != 0) {
                ix += dx;
                iy += dy;
                continue;
            }
            break;
        }
        const float val = d1[(size_t)iy * w + ix] + 0.5f * (Dx * fx + Dy * fy + Ds * fs);
        const float trace = Dxx + Dyy;
        const float hdet = Dxx * Dyy - Dxy * Dxy;
        const float score = (trace * trace) / hdet;
        Keypoint k;
        k.octave = c.octave;
        k.x = (float)ix + fx;
        k.y = (float)iy + fy;
        k.sample = (float)is + fs;
        const bool rejected = fabsf(val) < prm.contrast_threshold || score < 0.0f || score > prm.score_threshold
            || fabsf(fx) > 1.5f || fabsf(fy) > 1.5f || fabsf(fs) > 1.0f
            || k.sample < -1.0f || k.sample > (float)pyr.S
            || k.x < 0.0f || k.x > (float)(w - 1) || k.y < 0.0f || k.y > (float)(h - 1);
        ok = !rejected;
        out[i] = k;
        keep[i] = ok ? 1 : 0;
    }
    int total;
    (void)block_rank(ok, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ----------------------------------------------------------------------------- orientation and descriptor

// Gradient magnitude and orientation of Sift::generate_grad_ori_images at one pixel: interior pixels only, zero
// on the border; orientation in [0, 2 pi).
__device__ inline void grad_ori(const float *img, int w, int h, int x, int y, double *gm, double *go)
{
    if (x < 1 || y < 1 || x >= w - 1 || y >= h - 1) {
        *gm = 0.0;
        *go = 0.0;
        return;
    }
    const size_t p = (size_t)y * w + x;
    const double dx = 0.5 * ((double)img[p + 1] - (double)img[p - 1]);
    const double dy = 0.5 * ((double)img[p + w] - (double)img[p - w]);
    const double a = atan2(dy, dx);
    *gm = sqrt(dx * dx + dy * dy);
    *go = a < 0.0 ? a + kPi * 2.0 : a;
}

// What orientation assignment and the descriptor share: the keypoint's pixel, its image, and whether the
// descriptor window fits (it is the larger of the two; a keypoint whose descriptor window leaves the image
// yields no descriptor whatever its orientations).
struct KeypointFrame {
    const float *img;
    int w, h, ix, iy;
    float dxf, dyf;
    bool valid;
};

__device__ inline KeypointFrame keypoint_frame(const PyramidView &pyr, const Keypoint &k)
{
    KeypointFrame f;
    const OctaveView &o = pyr.oct[(int)k.octave - pyr.min_octave];
    // math::round: half away from zero
    const float r = k.sample > 0.0f ? floorf(k.sample + 0.5f) : ceilf(k.sample - 0.5f);
    const int ii = (int)r + 1;
    f.valid = ii >= 0 && ii < pyr.S + 3;
    f.img = o.img + (size_t)(f.valid ? ii : 0) * o.w * o.h;
    f.w = o.w;
    f.h = o.h;
    f.ix = (int)(k.x + 0.5f);
    f.iy = (int)(k.y + 0.5f);
    f.dxf = k.x - (float)f.ix;
    f.dyf = k.y - (float)f.iy;
    return f;
}

__device__ inline bool window_fits(const KeypointFrame &f, int win)
{
    return !(f.ix < win || f.ix + win >= f.w || f.iy < win || f.iy + win >= f.h);
}

__device__ inline int descriptor_window(float sigma)
{
    const float binsize = 3.0f * sigma;
    return (int)(kSqrt2 * (double)binsize * 5.0 * 0.5);
}

// Sift::orientation_assignment, one wave per keypoint.  Lane l adds the window's samples l, l + 64, ... into its
// own 36 bins; bin b is then the sum of the 64 partial bins in lane order; lane 0 smooths and finds the peaks.
constexpr int kOriBins = 36;
__global__ __launch_bounds__(64) void orientation_kernel(PyramidView pyr, const Keypoint *kps, const float *sigmas, int n,
    int32_t *num, float *orientations)
{
    __shared__ double part[64][kOriBins + 1];
    __shared__ double hist[kOriBins];
    const int k = blockIdx.x;
    if (k >= n) return;
    const int lane = threadIdx.x;
    const Keypoint kp = kps[k];
    const float sigma = sigmas[k];
    const KeypointFrame f = keypoint_frame(pyr, kp);
    const int win = (int)(sigma * 1.5f * 3.0f);
    if (!f.valid || !window_fits(f, win) || !window_fits(f, descriptor_window(sigma))) {
        if (lane == 0) num[k] = 0;
        return;
    }
    for (int b = 0; b < kOriBins; ++b) part[lane][b] = 0.0;
    const double dxf = (double)f.dxf, dyf = (double)f.dyf;
    const double maxdist = (double)(win * win) + 0.5;
    const double s = (double)(sigma * 1.5f);
    const int side = 2 * win + 1;
    for (int t = lane; t < side * side; t += 64) {
        const int dy = t / side - win, dx = t % side - win;
        const double ddx = (double)dx - dxf, ddy = (double)dy - dyf;
        const double dist = ddx * ddx + ddy * ddy;
        if (dist > maxdist) continue;
        double gm, go;
        grad_ori(f.img, f.w, f.h, f.ix + dx, f.iy + dy, &gm, &go);
        const double weight = exp(-(dist / (2.0 * s * s)));
        int bin = (int)((double)kOriBins * go / (2.0 * kPi));
        bin = min(max(bin, 0), kOriBins - 1);
        part[lane][bin] += gm * weight;
    }
    __syncthreads();
    if (lane < kOriBins) {
        double v = 0.0;
        for (int l = 0; l < 64; ++l) v += part[l][lane];
        hist[lane] = v;
    }
    __syncthreads();
    if (lane != 0) return;
    for (int i = 0; i < 6; ++i) {
        const double first = hist[0];
        double prev = hist[kOriBins - 1];
        for (int j = 0; j < kOriBins - 1; ++j) {
            const double cur = hist[j];
            hist[j] = (prev + cur + hist[j + 1]) / 3.0;
            prev = cur;
        }
        hist[kOriBins - 1] = (prev + hist[kOriBins - 1] + first) / 3.0;
    }
    double maxh = hist[0];
    for (int i = 1; i < kOriBins; ++i) maxh = hist[i] > maxh ? hist[i] : maxh;
    const double cut = (double)0.8f * maxh;
    int count = 0;
    for (int i = 0; i < kOriBins; ++i) {
        const double h0 = hist[(i + kOriBins - 1) % kOriBins], h1 = hist[i], h2 = hist[(i + 1) % kOriBins];
        if (h1 <= cut || h1 <= h0 || h1 <= h2) continue;
        const double x = -0.5 * (h2 - h0) / (h0 - 2.0 * h1 + h2);
        if (count < kMaxOrientations)
            orientations[(size_t)k * kMaxOrientations + count] = (float)(2.0 * kPi * (x + (double)i + 0.5) / (double)kOriBins);
        ++count;
    }
    num[k] = min(count, kMaxOrientations);   // 36 circular bins have at most 18 strict local maxima
}

// Sift::descriptor_assignment, one wave per (keypoint, orientation).  The 4 x 4 x 8 histogram exists 32 times;
// lanes l and l + 32 share copy l and add to it one after the other, so that every copy receives its samples
// in a fixed order; element e is the sum of the 32 copies in order.
constexpr int kDescCopies = 32;
__global__ __launch_bounds__(64) void descriptor_kernel(PyramidView pyr, const Keypoint *kps, const float *sigmas,
    const DescriptorJob *jobs, int n, float *out)
{
    __shared__ double part[kDescCopies][128 + 1];
    __shared__ double vec[128];
    __shared__ double norm;
    const int j = blockIdx.x;
    if (j >= n) return;
    const int lane = threadIdx.x;
    const DescriptorJob job = jobs[j];
    const Keypoint kp = kps[job.keypoint];
    const float sigma = sigmas[job.keypoint];
    const KeypointFrame f = keypoint_frame(pyr, kp);
    const int win = descriptor_window(sigma);
    float *dst = out + (size_t)j * 128;
    if (!f.valid || !window_fits(f, win)) {   // the orientation kernel lets no such keypoint through
        dst[lane] = 0.0f;
        dst[lane + 64] = 0.0f;
        return;
    }
    for (int e = lane; e < kDescCopies * 129; e += 64) (&part[0][0])[e] = 0.0;
    __syncthreads();
    const double o = (double)job.orientation;
    const double sino = sin(o), coso = cos(o);
    const double binsize = (double)(3.0f * sigma);
    const double dxf = (double)f.dxf, dyf = (double)f.dyf;
    const double binoff = 1.5;
    const int side = 2 * win + 1, total = side * side;
    double *mine = part[lane & (kDescCopies - 1)];
    for (int base = 0; base < total; base += 64) {
        const int t = base + lane;
        int idx[8];
        double val[8];
        int cnt = 0;
        if (t < total) {
            const int dy = t / side - win, dx = t % side - win;
            double mod, angle;
            grad_ori(f.img, f.w, f.h, f.ix + dx, f.iy + dy, &mod, &angle);
            double theta = angle - o;
            if (theta < 0.0) theta += 2.0 * kPi;
            const double winx = (double)dx - dxf, winy = (double)dy - dyf;
            const double binx = (coso * winx + sino * winy) / binsize + binoff;
            const double biny = (-sino * winx + coso * winy) / binsize + binoff;
            const double bint = theta * 8.0 / (2.0 * kPi) - 0.5;
            const double ex = binx - binoff, ey = biny - binoff;
            const double gw = exp(-((ex * ex + ey * ey) / 8.0));
            const double contrib = mod * gw;
            const int bx0 = (int)floor(binx), by0 = (int)floor(biny), bt0 = (int)floor(bint);
            const int bxi[2] = {bx0, bx0 + 1}, byi[2] = {by0, by0 + 1};
            int bti[2] = {bt0, bt0 + 1};
            const double wx[2] = {(double)bxi[1] - binx, 1.0 - ((double)bxi[1] - binx)};
            const double wy[2] = {(double)byi[1] - biny, 1.0 - ((double)byi[1] - biny)};
            const double wt[2] = {(double)bti[1] - bint, 1.0 - ((double)bti[1] - bint)};
            if (bti[0] < 0) bti[0] += 8;
            if (bti[1] >= 8) bti[1] -= 8;
#pragma unroll
            for (int yy = 0; yy < 2; ++yy)
#pragma unroll
                for (int xx = 0; xx < 2; ++xx)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        const bool inside = bxi[xx] >= 0 && bxi[xx] < 4 && byi[yy] >= 0 && byi[yy] < 4
                            && bti[tt] >= 0 && bti[tt] < 8;
                        idx[cnt] = inside ? bti[tt] + bxi[xx] * 8 + byi[yy] * 32 : -1;
                        val[cnt] = contrib * wx[xx] * wy[yy] * wt[tt];
                        ++cnt;
                    }
        }
        // the two halves of the wave take turns at the copies they share
        if (lane < 32)
            for (int c = 0; c < cnt; ++c)
                if (idx[c] >= 0) mine[idx[c]] += val[c];
        __syncthreads();
        if (lane >= 32)
            for (int c = 0; c < cnt; ++c)
                if (idx[c] >= 0) mine[idx[c]] += val[c];
        __syncthreads();
    }
    for (int e = lane; e < 128; e += 64) {
        double v = 0.0;
        for (int c = 0; c < kDescCopies; ++c) v += part[c][e];
        vec[e] = v;
    }
    // normalise, clamp at 0.2, normalise
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        if (lane == 0) {
            double sq = 0.0;
            for (int e = 0; e < 128; ++e) sq = sq + vec[e] * vec[e];
            norm = sqrt(sq);
        }
        __syncthreads();
        for (int e = lane; e < 128; e += 64) {
            double v = vec[e] / norm;
            if (pass == 0) v = v < (double)0.2f ? v : (double)0.2f;
            vec[e] = v;
        }
    }
    __syncthreads();
    dst[lane] = (float)vec[lane];
    dst[lane + 64] = (float)vec[lane + 64];
}

inline dim3 row_grid(int w, int h) { return dim3((unsigned)((w + kBlock - 1) / kBlock), (unsigned)h); }

}  // namespace

void launch_to_float(hipStream_t s, const uint8_t *pixels, int w, int h, int channels, float *out)
{
    const int n = w * h;
    hipLaunchKernelGGL(to_float_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pixels, n, channels, out);
}

void launch_double_size(hipStream_t s, const float *in, int w, int h, float *out)
{
    hipLaunchKernelGGL(double_size_kernel, row_grid(2 * w, 2 * h), dim3(kBlock), 0, s, in, w, h, out);
}

void launch_half_size(hipStream_t s, const float *in, int w, int h, float *out, float w1, float w2, float w3)
{
    hipLaunchKernelGGL(half_size_kernel, row_grid((w + 1) >> 1, (h + 1) >> 1), dim3(kBlock), 0, s, in, w, h, out, w1, w2, w3);
}

void launch_blur(hipStream_t s, const float *in, float *sep, float *out, const float *base, float *dog, int w, int h,
    const BlurWeights &wt)
{
    hipLaunchKernelGGL(blur_rows_kernel, row_grid(w, h), dim3(kBlock), 0, s, in, sep, w, h, wt);
    hipLaunchKernelGGL(blur_cols_kernel, dim3((w + kColTile - 1) / kColTile, (h + kColTile - 1) / kColTile), dim3(kBlock), 0, s,
        (const float *)sep, out, base, dog, w, h, wt);
}

void launch_extrema(hipStream_t s, const float *d0, const float *d1, const float *d2, int w, int h, int block_base,
    int32_t *counts, const int32_t *offsets, Keypoint *out, int capacity, float octave, float sample)
{
    const int blocks = extrema_blocks(w, h);
    if (!blocks) return;
    if (!offsets)
        hipLaunchKernelGGL(extrema_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, d0, d1, d2, w, h, block_base, counts, offsets,
            out, capacity, octave, sample);
    else
        hipLaunchKernelGGL(extrema_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, d0, d1, d2, w, h, block_base, counts, offsets,
            out, capacity, octave, sample);
}

void launch_localise(hipStream_t s, PyramidView pyr, LocaliseParams prm, const Keypoint *cand, int n, Keypoint *out,
    uint8_t *keep, int32_t *counts)
{
    hipLaunchKernelGGL(localise_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pyr, prm, cand, n, out, keep, counts);
}

void launch_orientation(hipStream_t s, PyramidView pyr, const Keypoint *kps, const float *sigma, int n, int32_t *num,
    float *orientations)
{
    hipLaunchKernelGGL(orientation_kernel, dim3(n), dim3(64), 0, s, pyr, kps, sigma, n, num, orientations);
}

void launch_descriptor(hipStream_t s, PyramidView pyr, const Keypoint *kps, const float *sigma, const DescriptorJob *jobs,
    int n, float *out)
{
    hipLaunchKernelGGL(descriptor_kernel, dim3(n), dim3(64), 0, s, pyr, kps, sigma, jobs, n, out);
}

}  // namespace sift
}  // namespace osfm
