// Kernels of the observation refinement (refine_kernels.h; DESIGN.md "Observation refinement").
//
// refine_kernel: one wave per observation.  Lane l owns the samples k = l, l + 64, ... of the (2 radius + 1)^2 window,
// in row-major order of the offsets u, for the template and for the target alike, so a lane reads back from LDS only
// what it wrote itself and the waves of a workgroup never meet: there is no barrier in the kernel.  Every exit is
// taken by the whole wave (the conditions are wave sums or wave votes).  A sample is read only after its own
// coordinates passed the inside test; the tail of the last stride runs no loop body at all.
//
// Sums: a lane adds its samples in ascending k, then the 64 partial sums are folded by the butterfly 32, 16, ..., 1.
// a + b == b + a to the bit, so every lane ends with the same value and the order is that of folding the upper half
// of the lanes onto the lower half -- which is how tests/refine_restatement.py adds.  The build has -ffp-contract=off.
#include "refine_kernels.h"

namespace osfm {
namespace refine {
namespace {

constexpr int kThreads = 64 * kWavesPerGroup;

__global__ __launch_bounds__(256) void grey_kernel(const uint8_t *__restrict__ px, int64_t n, int channels, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (channels == 1) {
        out[i] = (float)px[i];
    } else {
        const uint8_t *p = px + 3 * i;
        out[i] = (float)((int)p[0] + (int)p[1] + (int)p[2]) / 3.0f;
    }
}

// the reference observation and the alive count of a track, and the track of every observation: a thread per track
__global__ __launch_bounds__(256) void track_pass_kernel(Tracks t, Work w)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= t.num_tracks) return;
    int64_t ref = -1;
    int32_t count = 0;
    for (int64_t f = t.offsets[i]; f < t.offsets[i + 1]; ++f) {
        w.track_of[f] = (int32_t)i;
        if (!t.alive || t.alive[f]) {
            if (ref < 0) ref = f;
            ++count;
        }
    }
    w.ref_obs[i] = ref;
    w.alive_count[i] = count;
}

struct Sample { double v, gx, gy; };

// false for a NaN coordinate too
__device__ inline bool inside(double x, double y, const Image &im)
{
    return x >= 0.0 && x <= (double)(im.w - 1) && y >= 0.0 && y <= (double)(im.h - 1);
}

// The bilinear interpolant and its derivative at a point that passed inside().  A point on the last column (row) is
// interpolated in the cell to its left (above) with weight 1, so that no pixel beyond the image is read.
__device__ inline Sample bilinear(const Image &im, double x, double y)
{
    int x0 = (int)floor(x), y0 = (int)floor(y);
    x0 = min(x0, max(im.w - 2, 0));
    y0 = min(y0, max(im.h - 2, 0));
    const int x1 = min(x0 + 1, im.w - 1), y1 = min(y0 + 1, im.h - 1);
    const double fx = x - (double)x0, fy = y - (double)y0;
    const float *r0 = im.px + (size_t)y0 * (size_t)im.w, *r1 = im.px + (size_t)y1 * (size_t)im.w;
    const double i00 = (double)r0[x0], i01 = (double)r0[x1], i10 = (double)r1[x0], i11 = (double)r1[x1];
    const double top = (1.0 - fx) * i00 + fx * i01, bot = (1.0 - fx) * i10 + fx * i11;
    Sample s;
    s.v = (1.0 - fy) * top + fy * bot;
    s.gx = (1.0 - fy) * (i01 - i00) + fy * (i11 - i10);
    s.gy = (1.0 - fx) * (i10 - i00) + fx * (i11 - i01);
    return s;
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct Warp {
    double px, py, a00, a01, a10, a11;
};

__device__ inline void warp_point(const Warp &w, double sx, double sy, double *x, double *y)
{
    *x = w.px + (w.a00 * sx + w.a01 * sy);
    *y = w.py + (w.a10 * sx + w.a11 * sy);
}

// index of entry (a, b), a <= b, of the upper triangle stored row by row
__device__ constexpr int tri(int a, int b) { return a * kParams - a * (a - 1) / 2 + (b - a); }

// Cholesky of the diagonally scaled normal matrix and the step, in place: acc holds the upper triangle row by row,
// then the right hand side; entry (k, j) becomes L[j][k].  False (ill conditioned): a diagonal entry that is not
// positive, or a pivot below min_pivot.
__device__ inline bool solve_step(double *acc, double min_pivot, double *delta)
{
    double d[kParams];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < kParams; ++a) {
        if (!(acc[tri(a, a)] > 0.0)) ok = false;
        d[a] = 1.0 / sqrt(acc[tri(a, a)]);
    }
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < kParams; ++j) {
        double s = (acc[tri(j, j)] * d[j]) * d[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= acc[tri(k, j)] * acc[tri(k, j)];
        if (!(s >= min_pivot)) ok = false;
        const double ljj = sqrt(s);
        acc[tri(j, j)] = ljj;
#pragma unroll
        for (int i = j + 1; i < kParams; ++i) {
            double t = (acc[tri(j, i)] * d[i]) * d[j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= acc[tri(k, i)] * acc[tri(k, j)];
            acc[tri(j, i)] = t / ljj;
        }
    }
    if (!ok) return false;
    double y[kParams];
#pragma unroll
    for (int i = 0; i < kParams; ++i) {
        double t = acc[36 + i] * d[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= acc[tri(k, i)] * y[k];
        y[i] = t / acc[tri(i, i)];
    }
#pragma unroll
    for (int i = kParams - 1; i >= 0; --i) {
        double t = y[i];
#pragma unroll
        for (int k = i + 1; k < kParams; ++k) t -= acc[tri(i, k)] * delta[k];
        delta[i] = t / acc[tri(i, i)];
    }
#pragma unroll
    for (int i = 0; i < kParams; ++i) delta[i] = delta[i] * d[i];
    return true;
}

struct Result {
    double x, y, a[4], score;
    int32_t iterations;
};

// The refinement of one observation by one wave; tmpl: this wave's kMaxSamples doubles of LDS.  Returns the status;
// *r holds the refined values where it is OSFM_REFINE_REFINED, and score / iterations as far as the wave came.
__device__ int refine_one(const Image &ir, const Image &it, double rx, double ry, double p0x, double p0y, const double *A0,
    const osfm_refine_options &o, double *tmpl, int lane, Result *r)
{
    const int R = o.radius, side = 2 * R + 1, N = side * side;
    const double step = o.step, dN = (double)N;
    // the template and its mean
    bool out = false;
    double s1 = 0.0;
    for (int k = lane; k < N; k += 64) {
        const double sx = step * (double)(k % side - R), sy = step * (double)(k / side - R);
        const double x = rx + sx, y = ry + sy;
        if (!inside(x, y, ir)) { out = true; continue; }
        const double v = bilinear(ir, x, y).v;
        tmpl[k] = v;
        s1 += v;
    }
    if (__any(out)) return OSFM_REFINE_OUTSIDE;
    const double mean_t = wave_sum(s1) / dN;
    double s2 = 0.0;
    for (int k = lane; k < N; k += 64) {
        const double c = tmpl[k] - mean_t;
        s2 += c * c;
    }
    const double ss_t = wave_sum(s2);
    Warp w{p0x, p0y, A0[0], A0[1], A0[2], A0[3]};
    for (int k = lane; k < N; k += 64) {
        double x, y;
        warp_point(w, step * (double)(k % side - R), step * (double)(k / side - R), &x, &y);
        if (!inside(x, y, it)) out = true;
    }
    if (__any(out)) return OSFM_REFINE_OUTSIDE;
    if (sqrt(ss_t / dN) < o.min_contrast) return OSFM_REFINE_FLAT;

    // The photometric pair comes first in the elimination and the gain multiplies I - mean(T), with the bias starting
    // at mean(T): the same model as g I + b (the steps of Gauss-Newton do not depend on a linear change of the
    // parameters), in which the pivots of the six geometric parameters are what is left of them once brightness
    // and contrast are accounted for -- on a straight edge, next to nothing
    double gain = 1.0, bias = mean_t;
    bool converged = false;
    for (int iter = 0; iter < o.max_iterations; ++iter) {
        double acc[kSums];
#pragma unroll
        for (int i = 0; i < kSums; ++i) acc[i] = 0.0;
        for (int k = lane; k < N; k += 64) {
            const double sx = step * (double)(k % side - R), sy = step * (double)(k / side - R);
            double x, y;
            warp_point(w, sx, sy, &x, &y);
            if (!inside(x, y, it)) { out = true; continue; }
            const Sample s = bilinear(it, x, y);
            const double centred = s.v - mean_t;
            const double res = tmpl[k] - (gain * centred + bias);
            double j[kParams];
            j[0] = 1.0; j[1] = centred;
            j[2] = gain * s.gx; j[3] = gain * s.gy;
            j[4] = j[2] * sx; j[5] = j[2] * sy; j[6] = j[3] * sx; j[7] = j[3] * sy;
            int idx = 0;
#pragma unroll
            for (int a = 0; a < kParams; ++a)
#pragma unroll
                for (int b = a; b < kParams; ++b) acc[idx++] += j[a] * j[b];
#pragma unroll
            for (int a = 0; a < kParams; ++a) acc[36 + a] += j[a] * res;
            acc[44] += res * res;
        }
        if (__any(out)) return OSFM_REFINE_OUTSIDE;
#pragma unroll
        for (int i = 0; i < kSums; ++i) acc[i] = wave_sum(acc[i]);
        double delta[kParams];
        if (!solve_step(acc, o.min_pivot, delta)) return OSFM_REFINE_ILL_CONDITIONED;
        bias += delta[0]; gain += delta[1];
        w.px += delta[2]; w.py += delta[3];
        w.a00 += delta[4]; w.a01 += delta[5]; w.a10 += delta[6]; w.a11 += delta[7];
        r->iterations = iter + 1;
        if (sqrt(delta[2] * delta[2] + delta[3] * delta[3]) < o.eps) { converged = true; break; }
    }
    // the final patch: inside, then its correlation with the template (mean first, then the centred sums)
    double sj = 0.0;
    for (int k = lane; k < N; k += 64) {
        double x, y;
        warp_point(w, step * (double)(k % side - R), step * (double)(k / side - R), &x, &y);
        if (!inside(x, y, it)) { out = true; continue; }
        sj += bilinear(it, x, y).v;
    }
    if (__any(out)) return OSFM_REFINE_OUTSIDE;
    const double mean_j = wave_sum(sj) / dN;
    double c_tj = 0.0, c_jj = 0.0;
    for (int k = lane; k < N; k += 64) {
        double x, y;
        warp_point(w, step * (double)(k % side - R), step * (double)(k / side - R), &x, &y);
        const double cj = bilinear(it, x, y).v - mean_j, ct = tmpl[k] - mean_t;
        c_tj += ct * cj;
        c_jj += cj * cj;
    }
    c_tj = wave_sum(c_tj);
    c_jj = wave_sum(c_jj);
    const double den = sqrt(ss_t * c_jj);
    r->score = den > 0.0 ? c_tj / den : 0.0;
    if (!converged) return OSFM_REFINE_NOT_CONVERGED;
    const double dx = w.px - p0x, dy = w.py - p0y;
    if (sqrt(dx * dx + dy * dy) > o.max_shift) return OSFM_REFINE_REJECT_SHIFT;
    // singular values of M = A A0^-1: (E, H) and (F, G) are the rotation and the reflection part of M
    const double det0 = A0[0] * A0[3] - A0[1] * A0[2];
    const double i00 = A0[3] / det0, i01 = -A0[1] / det0, i10 = -A0[2] / det0, i11 = A0[0] / det0;
    const double m00 = w.a00 * i00 + w.a01 * i10, m01 = w.a00 * i01 + w.a01 * i11;
    const double m10 = w.a10 * i00 + w.a11 * i10, m11 = w.a10 * i01 + w.a11 * i11;
    const double E = 0.5 * (m00 + m11), F = 0.5 * (m00 - m11), G = 0.5 * (m10 + m01), H = 0.5 * (m10 - m01);
    const double Q = sqrt(E * E + H * H), S = sqrt(F * F + G * G);
    const double smax = Q + S, smin = fabs(Q - S);
    if (smax > o.max_deform || smin < 1.0 / o.max_deform) return OSFM_REFINE_REJECT_DEFORM;
    if (r->score < o.min_score) return OSFM_REFINE_REJECT_SCORE;
    r->x = w.px; r->y = w.py;
    r->a[0] = w.a00; r->a[1] = w.a01; r->a[2] = w.a10; r->a[3] = w.a11;
    return OSFM_REFINE_REFINED;
}

// Two waves a SIMD: the 45 sums, the step and a sample in flight need some 260 registers as the compiler schedules
// them; held to 256 it spills eight, and a third wave would cost over a hundred.
__global__ __launch_bounds__(kThreads, 2) void refine_kernel(const Image *__restrict__ images, Tracks t, Work wk, osfm_refine_options o, Out out)
{
    __shared__ double tmpl[kWavesPerGroup][kMaxSamples];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * kWavesPerGroup + wave;
    if (f >= t.num_obs) return;
    const int32_t track = wk.track_of[f];
    const int64_t ref = wk.ref_obs[track];
    const bool alive = !t.alive || t.alive[f];
    const double p0x = t.xy[2 * f], p0y = t.xy[2 * f + 1];
    double A0[4] = {1.0, 0.0, 0.0, 1.0};
    if (t.init_affine)
        for (int i = 0; i < 4; ++i) A0[i] = t.init_affine[4 * f + i];
    Result r;
    r.x = p0x; r.y = p0y; r.score = 0.0; r.iterations = 0;
    for (int i = 0; i < 4; ++i) r.a[i] = A0[i];
    int status;
    if (!alive || wk.alive_count[track] < 2) {
        status = OSFM_REFINE_UNTESTED;
    } else if (f == ref) {
        status = OSFM_REFINE_REFERENCE;
    } else {
        const Image ir = images[t.view[ref]], it = images[t.view[f]];
        status = refine_one(ir, it, t.xy[2 * ref], t.xy[2 * ref + 1], p0x, p0y, A0, o, tmpl[wave], lane, &r);
    }
    if (lane == 0) {
        out.xy[2 * f] = r.x; out.xy[2 * f + 1] = r.y;
        for (int i = 0; i < 4; ++i) out.affine[4 * f + i] = r.a[i];
        out.score[f] = r.score;
        out.status[f] = status;
        out.iterations[f] = r.iterations;
    }
}

}  // namespace

void launch_grey(hipStream_t s, const uint8_t *pixels, int w, int h, int channels, float *out)
{
    const int64_t n = (int64_t)w * h;
    if (n <= 0) return;
    hipLaunchKernelGGL(grey_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pixels, n, channels, out);
}

void launch_track_pass(hipStream_t s, const Tracks &t, const Work &w)
{
    if (t.num_tracks <= 0) return;
    hipLaunchKernelGGL(track_pass_kernel, dim3((unsigned)((t.num_tracks + 255) / 256)), dim3(256), 0, s, t, w);
}

void launch_refine(hipStream_t s, const Image *images, const Tracks &t, const Work &w, const osfm_refine_options &o, const Out &out)
{
    if (t.num_obs <= 0) return;
    hipLaunchKernelGGL(refine_kernel, dim3((unsigned)((t.num_obs + kWavesPerGroup - 1) / kWavesPerGroup)), dim3(kThreads), 0, s,
        images, t, w, o, out);
}

}  // namespace refine
}  // namespace osfm
