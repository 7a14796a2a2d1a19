// Kernels of the dense plane sweep and of the fusion (dense_kernels.h; DESIGN.md "Dense plane sweep").
//
// dense_sweep_kernel: a workgroup of 256 threads owns a 32 x 16 tile of reference pixels and its halo of `radius`.
// Per depth and source every thread warps its up to six halo texels -- position in double, in the order of
// tests/dense_restatement.py, so the inside test is the restatement's to the bit; bilinear sample in float32 -- and
// leaves (w, w^2, w r, inside) as one float4 in LDS.  The window sums are separable: a pass along the rows into a
// second plane, a pass along the columns into registers, each adding its 2 radius + 1 taps in ascending order (taps,
// not a running sum: a running float32 sum carries the rounding of everything that has left the window).  One
// ds_read_b128 per tap serves all four sums, and consecutive lanes read consecutive 16-byte slots.  The score, the
// mean over the valid sources, the best depth and its two neighbours stay in registers; nothing of the cost volume
// is written.  The warp loop and both passes run for every thread of the workgroup, so the barriers are uniform.
#include <cmath>

#include "dense_kernels.h"

namespace osfm {
namespace dense {
namespace {

std::atomic<int> g_ablation{kAblateNone};

struct Best {
    float c, minus, plus;         // c[k*], c[k* - 1], c[k* + 1]
    int k;                        // -1: no valid depth yet
    bool minus_ok, plus_ok;
};

__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// the bilinear sample of a position that passed the inside test, on the values minus 128: cell min(floor(p), w - 2),
// so the last column (row) is read with weight 1 from the cell to its left (above) and nothing beyond the image is
__device__ inline float sample(const Source &s, double px, double py)
{
    int x0 = (int)floor(px), y0 = (int)floor(py);
    x0 = min(x0, max(s.w - 2, 0));
    y0 = min(y0, max(s.h - 2, 0));
    const int x1 = min(x0 + 1, s.w - 1), y1 = min(y0 + 1, s.h - 1);
    const float fx = (float)(px - (double)x0), fy = (float)(py - (double)y0);
    const float *r0 = s.px + (size_t)y0 * (size_t)s.w, *r1 = s.px + (size_t)y1 * (size_t)s.w;
    const float i00 = r0[x0] - 128.0f, i01 = r0[x1] - 128.0f, i10 = r1[x0] - 128.0f, i11 = r1[x1] - 128.0f;
    const float top = (1.0f - fx) * i00 + fx * i01, bot = (1.0f - fx) * i10 + fx * i11;
    return (1.0f - fy) * top + fy * bot;
}

// kMode: kAblateNone is the kernel.  The others leave one part of the work out, for tools/dense_timing.py to see what
// the time is made of (osfm_dense_debug_ablation); their results mean nothing.
template <int kMode>
__global__ __launch_bounds__(kThreads) void dense_sweep_kernel(const SweepArgs a)
{
    __shared__ float4 samp[kHalo];                 // per halo texel: w, w^2, w r, inside
    __shared__ float4 rows[kHaloH * kTileW];       // the sums along the rows, per halo row and tile column
    __shared__ float reft[kHalo];                  // the reference texel minus 128 (0 outside the image)
    const int tid = threadIdx.x;
    const int R = a.radius, side = 2 * R + 1, hw = kTileW + 2 * R, hh = kTileH + 2 * R, nh = hw * hh;
    const int ox = (int)blockIdx.x * kTileW, oy = (int)blockIdx.y * kTileH;
    const float n = (float)(side * side), inv_n = 1.0f / n;

    // the halo texels of this thread: position in the halo, and whether the reference image has them
    int slot_x[kSlots], slot_y[kSlots];
    bool slot_in[kSlots];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
        const int i = tid + q * kThreads;
        const int hy = i / hw, hx = i - hy * hw;
        slot_x[q] = ox - R + hx;
        slot_y[q] = oy - R + hy;
        slot_in[q] = i < nh && slot_x[q] >= 0 && slot_x[q] < a.w && slot_y[q] >= 0 && slot_y[q] < a.h;
        if (i < nh) {
            const float r = slot_in[q] ? a.ref[(size_t)slot_y[q] * (size_t)a.w + (size_t)slot_x[q]] - 128.0f : 0.0f;
            reft[i] = r;
            samp[i] = make_float4(r, r * r, 0.0f, slot_in[q] ? 1.0f : 0.0f);
        }
    }
    // this thread's two pixels: (tx, ty) and (tx, ty + 8) of the tile
    const int tx = tid & (kTileW - 1), ty = tid >> 5;
    float sr[2], var_r[2];
    bool live[2];                 // neither BORDER nor FLAT: the pixel is scored
    uint8_t status[2];
    __syncthreads();
    for (int it = tid; it < hh * kTileW; it += kThreads) {
        const int hy = it >> 5, cx = it & (kTileW - 1);
        float4 s = samp[hy * hw + cx];
        for (int j = 1; j < side; ++j) s = add4(s, samp[hy * hw + cx + j]);
        rows[it] = s;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int py = ty + 8 * p, x = ox + tx, y = oy + py;
        float4 s = rows[py * kTileW + tx];
        for (int j = 1; j < side; ++j) s = add4(s, rows[(py + j) * kTileW + tx]);
        sr[p] = s.x;
        var_r[p] = s.y - s.x * s.x * inv_n;
        const bool border = x - R < 0 || x + R > a.w - 1 || y - R < 0 || y + R > a.h - 1;
        status[p] = border ? OSFM_DENSE_BORDER : var_r[p] < a.min_var ? OSFM_DENSE_FLAT : OSFM_DENSE_OK;
        live[p] = status[p] == OSFM_DENSE_OK;
    }

    Best best[2];
    float prev[2] = {0.0f, 0.0f};
    bool prev_ok[2] = {false, false};
#pragma unroll
    for (int p = 0; p < 2; ++p) best[p] = Best{0.0f, 0.0f, 0.0f, -1, false, false};

    const int taps = kMode == kAblateBoxSums ? 1 : side;
    for (int k = 0; k < a.num_depths; ++k) {
        const double z = a.z_min + (double)k * a.dz;
        float total[2] = {0.0f, 0.0f};
        int count[2] = {0, 0};
        for (int si = 0; si < a.num_sources; ++si) {
            const Source &s = a.src[si];
            const double cx = s.g[0] + z * s.e[0], cy = s.g[1] + z * s.e[1];
            __syncthreads();              // the passes of the source before are done with samp and rows
#pragma unroll
            for (int q = 0; q < kSlots; ++q) {
                const int i = tid + q * kThreads;
                if (i >= nh) continue;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (slot_in[q]) {
                    const double x = (double)slot_x[q], y = (double)slot_y[q];
                    double px, py;
                    if (kMode == kAblateDouble) {
                        px = (double)(((float)s.G[0][0] * (float)slot_x[q] + (float)s.G[0][1] * (float)slot_y[q]) + (float)cx);
                        py = (double)(((float)s.G[1][0] * (float)slot_x[q] + (float)s.G[1][1] * (float)slot_y[q]) + (float)cy);
                    } else {
                        px = (s.G[0][0] * x + s.G[0][1] * y) + cx;
                        py = (s.G[1][0] * x + s.G[1][1] * y) + cy;
                    }
                    if (px >= 0.0 && px <= (double)(s.w - 1) && py >= 0.0 && py <= (double)(s.h - 1)) {
                        const float w = kMode == kAblateGather ? (float)(px - floor(px)) + (float)(py - floor(py)) : sample(s, px, py);
                        v = make_float4(w, w * w, w * reft[i], 1.0f);
                    }
                }
                samp[i] = v;
            }
            __syncthreads();
            for (int it = tid; it < hh * kTileW; it += kThreads) {
                const int hy = it >> 5, c0 = it & (kTileW - 1);
                float4 t = samp[hy * hw + c0];
                for (int j = 1; j < taps; ++j) t = add4(t, samp[hy * hw + c0 + j]);
                rows[it] = t;
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (!live[p]) continue;
                const int py = ty + 8 * p;
                float4 t = rows[py * kTileW + tx];
                for (int j = 1; j < taps; ++j) t = add4(t, rows[(py + j) * kTileW + tx]);
                const float var_w = t.y - t.x * t.x * inv_n;
                if (t.w == n && var_w >= a.min_var) {
                    const float cov = t.z - t.x * sr[p] * inv_n;
                    total[p] += cov / sqrtf(var_r[p] * var_w);
                    ++count[p];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool ok = live[p] && count[p] >= a.min_sources;
            const float c = ok ? total[p] / (float)count[p] : 0.0f;
            Best &b = best[p];
            if (b.k >= 0 && b.k == k - 1) { b.plus = c; b.plus_ok = ok; }
            if (ok && (b.k < 0 || c > b.c)) {
                b.c = c; b.k = k;
                b.minus = prev[p]; b.minus_ok = prev_ok[p];
                b.plus = 0.0f; b.plus_ok = false;
            }
            prev[p] = c; prev_ok[p] = ok;
        }
    }

#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int x = ox + tx, y = oy + ty + 8 * p;
        if (x >= a.w || y >= a.h) continue;
        const Best &b = best[p];
        uint8_t st = status[p];
        if (st == OSFM_DENSE_OK) {
            if (b.k < 0) st = OSFM_DENSE_NO_SOURCES;
            else if (b.c < a.min_score) st = OSFM_DENSE_LOW_SCORE;
            else if (b.k == 0 || b.k == a.num_depths - 1 || !b.minus_ok || !b.plus_ok) st = OSFM_DENSE_RANGE_EDGE;
        }
        double depth = __builtin_nan("");
        float score = 0.0f;
        if (st == OSFM_DENSE_OK) {
            const double cm = (double)b.minus, c0 = (double)b.c, cp = (double)b.plus;
            const double off = 0.5 * (cm - cp) / (cm - 2.0 * c0 + cp);
            depth = a.z_min + ((double)b.k + off) * a.dz;
            score = b.c;
        }
        const size_t at = (size_t)y * (size_t)a.w + (size_t)x;
        a.depth[at] = depth;
        a.score[at] = score;
        a.status[at] = st;
    }
}

__device__ inline void point_of(const ViewGeo &g, int x, int y, double z, double *X)
{
    const double dx = (double)x - g.t[0], dy = (double)y - g.t[1];
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = (g.B[j][0] * dx + g.B[j][1] * dy) + z * g.d[j];
}

// A thread per pixel of view r: an OK pixel looks its point up in every other swept view, in ascending order
__global__ __launch_bounds__(256) void dense_consistency_kernel(const FuseView *__restrict__ views, int num_views, int r, int64_t pixels,
    double tol, int min_consistent, int32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const FuseView &v = views[r];
    uint8_t st = v.status[i];
    if (st == OSFM_DENSE_OK) {
        double X[3];
        point_of(v.geo, (int)(i % v.w), (int)(i / v.w), v.depth[i], X);
        int support = 0;
        bool lower = false;
        for (int si = 0; si < num_views; ++si) {
            const FuseView &s = views[si];
            if (si == r || !s.swept) continue;
            const double qx = ((s.geo.A[0][0] * X[0] + s.geo.A[0][1] * X[1]) + s.geo.A[0][2] * X[2]) + s.geo.t[0];
            const double qy = ((s.geo.A[1][0] * X[0] + s.geo.A[1][1] * X[1]) + s.geo.A[1][2] * X[2]) + s.geo.t[1];
            const double fx = floor(qx + 0.5), fy = floor(qy + 0.5);
            if (!(fx >= 0.0 && fx <= (double)(s.w - 1) && fy >= 0.0 && fy <= (double)(s.h - 1))) continue;
            const size_t at = (size_t)(int)fy * (size_t)s.w + (size_t)(int)fx;
            if (s.status[at] != OSFM_DENSE_OK) continue;
            const double zs = (s.geo.d[0] * X[0] + s.geo.d[1] * X[1]) + s.geo.d[2] * X[2];
            if (fabs(s.depth[at] - zs) <= tol * s.dz) {
                ++support;
                if (si < r) lower = true;
            }
        }
        if (support < min_consistent) st = OSFM_DENSE_INCONSISTENT;
        else if (lower) st = OSFM_DENSE_DUPLICATE;
    }
    v.final_status[i] = st;
    flags[v.offset + i] = st == OSFM_DENSE_OK ? 1 : 0;
}

__global__ __launch_bounds__(256) void dense_emit_kernel(const FuseView *__restrict__ views, int r, int64_t pixels,
    const int32_t *__restrict__ flags, const int32_t *__restrict__ scan, Cloud cloud)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const FuseView &v = views[r];
    if (!flags[v.offset + i]) return;
    const int64_t slot = scan[v.offset + i];
    const int x = (int)(i % v.w), y = (int)(i / v.w);
    double X[3];
    point_of(v.geo, x, y, v.depth[i], X);
    cloud.points[3 * slot] = X[0]; cloud.points[3 * slot + 1] = X[1]; cloud.points[3 * slot + 2] = X[2];
    cloud.view[slot] = r;
    cloud.pixel[2 * slot] = x; cloud.pixel[2 * slot + 1] = y;
}

}  // namespace

bool make_geo(const double *P, ViewGeo *g)
{
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(P[i])) return false;
    const double *a0 = P, *a1 = P + 4;
    for (int j = 0; j < 3; ++j) { g->A[0][j] = a0[j]; g->A[1][j] = a1[j]; }
    g->t[0] = P[3]; g->t[1] = P[7];
    const double c[3] = {a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]};
    const double nn = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const double m00 = (a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2];
    const double m01 = (a0[0] * a1[0] + a0[1] * a1[1]) + a0[2] * a1[2];
    const double m11 = (a1[0] * a1[0] + a1[1] * a1[1]) + a1[2] * a1[2];
    const double det = m00 * m11 - m01 * m01;
    if (!(det > 1e-12 * (m00 * m11)) || !(nn > 0.0) || !std::isfinite(det)) return false;
    for (int j = 0; j < 3; ++j) g->d[j] = c[j] / nn;
    const double i00 = m11 / det, i01 = -m01 / det, i11 = m00 / det;
    for (int j = 0; j < 3; ++j) {
        g->B[j][0] = a0[j] * i00 + a1[j] * i01;
        g->B[j][1] = a0[j] * i01 + a1[j] * i11;
    }
    return true;
}

void make_source(const ViewGeo &ref, const ViewGeo &src, Source *s)
{
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 2; ++j)
            s->G[i][j] = (src.A[i][0] * ref.B[0][j] + src.A[i][1] * ref.B[1][j]) + src.A[i][2] * ref.B[2][j];
        s->g[i] = src.t[i] - (s->G[i][0] * ref.t[0] + s->G[i][1] * ref.t[1]);
        s->e[i] = (src.A[i][0] * ref.d[0] + src.A[i][1] * ref.d[1]) + src.A[i][2] * ref.d[2];
    }
}

void launch_sweep(hipStream_t s, const SweepArgs &a)
{
    if (a.w <= 0 || a.h <= 0) return;
    const dim3 grid((unsigned)((a.w + kTileW - 1) / kTileW), (unsigned)((a.h + kTileH - 1) / kTileH));
    switch (g_ablation.load()) {
    case kAblateGather: hipLaunchKernelGGL(dense_sweep_kernel<kAblateGather>, grid, dim3(kThreads), 0, s, a); break;
    case kAblateDouble: hipLaunchKernelGGL(dense_sweep_kernel<kAblateDouble>, grid, dim3(kThreads), 0, s, a); break;
    case kAblateBoxSums: hipLaunchKernelGGL(dense_sweep_kernel<kAblateBoxSums>, grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL(dense_sweep_kernel<kAblateNone>, grid, dim3(kThreads), 0, s, a);
    }
}

int set_ablation(int mode)
{
    return g_ablation.exchange(mode >= kAblateNone && mode <= kAblateBoxSums ? mode : kAblateNone);
}

void launch_consistency(hipStream_t s, const FuseView *views, int num_views, int r, int64_t pixels, double tol, int min_consistent,
    int32_t *flags)
{
    if (pixels <= 0) return;
    hipLaunchKernelGGL(dense_consistency_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, views, num_views, r, pixels,
        tol, min_consistent, flags);
}

void launch_emit(hipStream_t s, const FuseView *views, int r, int64_t pixels, const int32_t *flags, const int32_t *scan, Cloud cloud)
{
    if (pixels <= 0) return;
    hipLaunchKernelGGL(dense_emit_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, views, r, pixels, flags, scan, cloud);
}

}  // namespace dense
}  // namespace osfm
