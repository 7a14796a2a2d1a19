// Kernels of the depth-map meshes (mesh_kernels.h).  Every rule is the one of tests/mesh_restatement.py; the sums that
// reach an output run in its order (the build contracts nothing).
#include <cmath>

#include "mesh_kernels.h"

namespace osfm {
namespace mesh {

namespace {

// ---- counting ---------------------------------------------------------------------------------------------------
// One atomic per wave, on the counter set of the workgroup's slot: atomics on one word go through the L2 one after the
// other, and 65536 waves of a 2048 x 2048 view on one word cost most of a millisecond.  The host adds the slots up.
// Every lane of the wave calls count_if (no lane has returned before).
__device__ inline unsigned long long *my_slot(unsigned long long *counters)
{
    return counters + (size_t)((blockIdx.x + blockIdx.y * gridDim.x) % kCounterSlots) * kSlotStride;
}

__device__ inline void count_if(bool p, unsigned long long *counters, int which)
{
    const unsigned long long m = __ballot(p);
    if (m != 0ull && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(&my_slot(counters)[which], (unsigned long long)__popcll(m));
}

__device__ inline void raise_error(unsigned long long *counters)
{
    atomicMax(&my_slot(counters)[kError], 1ull);
}

// ---- union-find ---------------------------------------------------------------------------------------------------
// parent[i] <= i always, and a root has parent[i] == i.  Every access goes through an atomic of the given scope: in
// the seam kernel other workgroups, on other XCDs, write the same words, and a plain load may be served from a stale
// line.  -1: the walk ran out of `budget`, or met a word that is no parent (a defect either way).
template <int Scope> __device__ inline int uf_find(int *parent, int a, int &budget)
{
    for (;;) {
        const int q = __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, Scope);
        if (q == a) return a;
        if (q < 0 || q > a || --budget < 0) return -1;
        a = q;
    }
}

// Joins the sets of a and b: the larger root is hung under the smaller one by an atomic min, which another thread's
// join of the same root may beat -- then the loser goes on with what it found there.  false: out of budget.
template <int Scope> __device__ inline bool uf_union(int *parent, int a, int b)
{
    int budget = kMaxHops;
    for (;;) {
        a = uf_find<Scope>(parent, a, budget);
        b = uf_find<Scope>(parent, b, budget);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&parent[a], b, __ATOMIC_RELAXED, Scope);
        if (old == a) return true;
        if (--budget < 0) return false;
        a = old;
    }
}

__global__ __launch_bounds__(256) void mesh_solid_kernel(View v, uint8_t *__restrict__ solid, unsigned long long *__restrict__ counters)
{
    const int64_t n = (int64_t)v.w * v.h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool s = false;
    if (i < n) {
        s = v.status[i] == OSFM_DENSE_OK;
        if (s && v.final_status) {
            const uint8_t f = v.final_status[i];
            s = f == OSFM_DENSE_OK || f == OSFM_DENSE_DUPLICATE;
        }
        solid[i] = s ? 1 : 0;
    }
    count_if(s, counters, kSolid);
}

__global__ __launch_bounds__(kLabelThreads) void mesh_label_tile_kernel(int w, int h, const uint8_t *__restrict__ solid,
    int32_t *__restrict__ parent, int32_t *__restrict__ local, int32_t *__restrict__ tile_size, int32_t *__restrict__ size,
    unsigned long long *__restrict__ counters)
{
    __shared__ int par[kLabelThreads];
    __shared__ int cnt[kLabelThreads];
    __shared__ uint8_t sol[kLabelThreads];
    const int li = (int)threadIdx.x, tx = li % kLabelTileW, ty = li / kLabelTileW;
    const int x = (int)blockIdx.x * kLabelTileW + tx, y = (int)blockIdx.y * kLabelTileH + ty;
    const bool in = x < w && y < h;
    const size_t i = in ? (size_t)y * w + x : 0;
    const bool s = in && solid[i] != 0;
    par[li] = li;
    cnt[li] = 0;
    sol[li] = s ? 1 : 0;
    __syncthreads();
    bool ok = true;
    if (s && tx > 0 && sol[li - 1]) ok = uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, li - 1) && ok;
    if (s && ty > 0 && sol[li - kLabelTileW]) ok = uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, li - kLabelTileW) && ok;
    __syncthreads();
    int budget = kMaxHops;
    int root = s ? uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, budget) : li;
    if (root < 0) { ok = false; root = li; }
    if (s) atomicAdd(&cnt[root], 1);
    __syncthreads();
    if (!ok) raise_error(counters);
    if (in) {
        const int32_t g = (int32_t)(((size_t)blockIdx.y * kLabelTileH + root / kLabelTileW) * w + (size_t)blockIdx.x * kLabelTileW + root % kLabelTileW);
        parent[i] = s ? g : -1;
        local[i] = s ? g : -1;
        tile_size[i] = s && root == li ? cnt[li] : 0;
        size[i] = 0;
    }
}

__global__ __launch_bounds__(256) void mesh_label_seam_kernel(int w, int h, const uint8_t *__restrict__ solid, int32_t *parent,
    unsigned long long *__restrict__ counters)
{
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !solid[i]) return;
    const int x = (int)(i % w), y = (int)(i / w);
    bool ok = true;
    if (x > 0 && x % kLabelTileW == 0 && solid[i - 1]) ok = uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)i, (int)i - 1) && ok;
    if (y > 0 && y % kLabelTileH == 0 && solid[i - w]) ok = uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)i, (int)i - w) && ok;
    if (!ok) raise_error(counters);
}

// the seam kernel has ended: parent[] is final and read as it is
__global__ __launch_bounds__(256) void mesh_label_root_kernel(int w, int h, const uint8_t *__restrict__ solid, int32_t *parent,
    int32_t *__restrict__ local, const int32_t *__restrict__ tile_size, int32_t *__restrict__ size, unsigned long long *__restrict__ counters)
{
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !solid[i] || local[i] != (int32_t)i) return;
    int budget = kMaxHops;
    const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)i, budget);
    if (r < 0) { raise_error(counters); return; }          // local[i] stays i: a valid index
    atomicAdd(&size[r], tile_size[i]);
    local[i] = r;
}

__global__ __launch_bounds__(256) void mesh_label_clear_kernel(int w, int h, int min_island, uint8_t *__restrict__ solid,
    const int32_t *__restrict__ local, const int32_t *__restrict__ size, unsigned long long *__restrict__ counters)
{
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool island = false, is_root = false;
    if (i < n && solid[i]) {
        const int32_t a = local[i];
        const int32_t r = local[a];                          // a tile-local root holds its root
        is_root = a == (int32_t)i && r == (int32_t)i;
        island = size[r] < min_island;
        if (island) solid[i] = 0;
    }
    count_if(island, counters, kIslandPixels);
    count_if(is_root, counters, kComponents);
}

// ---- triangles -----------------------------------------------------------------------------------------------------
__device__ inline bool cut(double za, double zb, double lim)
{
    return fabs(za - zb) > lim;
}

__global__ __launch_bounds__(256) void mesh_blocks_kernel(View v, const uint8_t *__restrict__ solid, int dd, double thr, double thr_diag,
    uint8_t *__restrict__ blocks, int32_t *__restrict__ tflags, unsigned long long *__restrict__ counters)
{
    const int64_t n = (int64_t)v.w * v.h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned keep = 0, dropped = 0;
    if (i < n) {
        const int x = (int)(i % v.w), y = (int)(i / v.w);
        if (x < v.w - 1 && y < v.h - 1) {
            const int64_t at[4] = {i, i + 1, i + v.w, i + v.w + 1};
            unsigned m = 0;
            double z[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool s = solid[at[c]] != 0;
                m |= s ? 1u << c : 0u;
                z[c] = s ? v.depth[at[c]] : 0.0;
            }
            unsigned cand = 0;
            if (m == 7u) cand = 1u;
            else if (m == 11u) cand = 2u;
            else if (m == 13u) cand = 4u;
            else if (m == 14u) cand = 8u;
            else if (m == 15u) cand = fabs(z[0] - z[3]) < fabs(z[1] - z[2]) ? 6u : 9u;
            keep = cand;
            if (dd) {
                const bool s01 = cut(z[0], z[1], thr), s02 = cut(z[0], z[2], thr), s13 = cut(z[1], z[3], thr), s23 = cut(z[2], z[3], thr);
                const bool d03 = cut(z[0], z[3], thr_diag), d12 = cut(z[1], z[2], thr_diag);
                unsigned bad = 0;
                if (s02 || d12 || s01) bad |= 1u;             // T1 = (0, 2, 1)
                if (d03 || s13 || s01) bad |= 2u;             // T2 = (0, 3, 1)
                if (s02 || s23 || d03) bad |= 4u;             // T3 = (0, 2, 3)
                if (d12 || s23 || s13) bad |= 8u;             // T4 = (1, 2, 3)
                keep = cand & ~bad;
                dropped = (unsigned)__popc(cand & bad);
            }
        }
        blocks[i] = (uint8_t)keep;
        tflags[i] = __popc(keep);
    }
    count_if(dropped >= 1u, counters, kDropped);
    count_if(dropped >= 2u, counters, kDropped);
}

// ---- the triangles around a pixel -----------------------------------------------------------------------------------
// The pixel sits at (1, 1) of a 3 x 3 neighbourhood, positions p = 3 row + column.  Block q of the four that hold it
// (NW, NE, SW, SE: ascending block index) has its first pixel at (q & 1, q >> 1) and the pixel as its corner 3 - q.
__device__ constexpr int kTri[4][3] = {{0, 2, 1}, {0, 3, 1}, {0, 2, 3}, {1, 2, 3}};

__device__ inline int pos_of(int q, int c)
{
    return ((q >> 1) + (c >> 1)) * 3 + (q & 1) + (c & 1);
}

__device__ inline unsigned block_at(const uint8_t *__restrict__ blocks, int w, int h, int bx, int by)
{
    return bx >= 0 && by >= 0 && bx < w - 1 && by < h - 1 ? (unsigned)blocks[(size_t)by * w + bx] : 0u;
}

// uses[p]: how many of the pixel's triangles name position p
__device__ inline void incident(const uint8_t *__restrict__ blocks, int w, int h, int x, int y, unsigned bytes[4], int uses[9])
{
#pragma unroll
    for (int p = 0; p < 9; ++p) uses[p] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bytes[q] = block_at(blocks, w, h, x - 1 + (q & 1), y - 1 + (q >> 1));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool mine = kTri[t][0] == 3 - q || kTri[t][1] == 3 - q || kTri[t][2] == 3 - q;
            if (!mine) bytes[q] &= ~(1u << t);
            if (mine && (bytes[q] >> t & 1u)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) uses[pos_of(q, kTri[t][k])]++;
            }
        }
    }
}

__global__ __launch_bounds__(256) void mesh_vertices_kernel(int w, int h, const uint8_t *__restrict__ blocks, int32_t *__restrict__ vflags,
    uint8_t *__restrict__ cls, uint8_t *__restrict__ links, uint8_t *__restrict__ dist, unsigned long long *__restrict__ counters)
{
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int c = -1;
    if (i < n) {
        unsigned bytes[4];
        int uses[9];
        incident(blocks, w, h, (int)(i % w), (int)(i / w), bytes, uses);
        unsigned link = 0;
        int open = 0;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            if (p == 4) continue;
            if (uses[p] > 0) link |= 1u << (p < 4 ? p : p - 1);
            if (uses[p] == 1) ++open;
        }
        // An edge that one triangle names ends a chain.  The triangles around a pixel do not overlap in the image, so
        // a closed fan leaves room for no second chain: no open edge is SIMPLE, two are one chain, more are several.
        if (uses[4] > 0) c = open == 0 ? OSFM_MESH_VERTEX_SIMPLE : open == 2 ? OSFM_MESH_VERTEX_BORDER : OSFM_MESH_VERTEX_COMPLEX;
        vflags[i] = c >= 0 ? 1 : 0;
        cls[i] = (uint8_t)(c >= 0 ? c : 0);
        links[i] = (uint8_t)link;
        dist[i] = c == OSFM_MESH_VERTEX_BORDER ? 0 : 255;
    }
    count_if(c == OSFM_MESH_VERTEX_SIMPLE, counters, kSimple);
    count_if(c == OSFM_MESH_VERTEX_BORDER, counters, kBorder);
    count_if(c == OSFM_MESH_VERTEX_COMPLEX, counters, kComplex);
}

__global__ __launch_bounds__(256) void mesh_distance_kernel(int w, int h, const uint8_t *__restrict__ links, const uint8_t *__restrict__ in,
    uint8_t *__restrict__ out)
{
    const int64_t n = (int64_t)w * h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned link = links[i];
    unsigned d = in[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int p = k < 4 ? k : k + 1;
        if (link >> k & 1u) {                                  // a link only ever points inside the image
            const unsigned o = in[i + (int64_t)(p / 3 - 1) * w + (p % 3 - 1)];
            if (o != 255u && o + 1u < d) d = o + 1u;
        }
    }
    out[i] = (uint8_t)d;
}

// the fusion's formula (dense_kernels.hip, point_of), in its order
__device__ inline void point_of(const dense::ViewGeo &g, int x, int y, double z, double X[3])
{
    const double dx = (double)x - g.t[0], dy = (double)y - g.t[1];
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = (g.B[j][0] * dx + g.B[j][1] * dy) + z * g.d[j];
}

__global__ __launch_bounds__(256) void mesh_emit_kernel(View v, const uint8_t *__restrict__ blocks, const int32_t *__restrict__ vflags,
    const int32_t *__restrict__ vscan, const int32_t *__restrict__ tscan, const uint8_t *__restrict__ cls, const uint8_t *__restrict__ dist,
    int iterations, Mesh mesh)
{
    const int64_t n = (int64_t)v.w * v.h;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % v.w), y = (int)(i / v.w);
    const unsigned own = blocks[i];                            // 0 in the last column and row
    if (own) {
        int64_t slot = tscan[i];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (own >> t & 1u) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    mesh.triangles[3 * slot + k] = vscan[i + (kTri[t][k] & 1) + (int64_t)(kTri[t][k] >> 1) * v.w];
                ++slot;
            }
    }
    if (!vflags[i]) return;
    unsigned bytes[4];
    int uses[9];
    incident(blocks, v.w, v.h, x, y, bytes, uses);
    double P[9][3];
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        P[p][0] = P[p][1] = P[p][2] = 0.0;
        if (uses[p] > 0) {                                     // named by a triangle: inside the image, and solid
            const int px = x + p % 3 - 1, py = y + p / 3 - 1;
            point_of(v.geo, px, py, v.depth[(size_t)py * v.w + px], P[p]);
        }
    }
    double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (bytes[q] >> t & 1u) {
                const int a = pos_of(q, kTri[t][0]), b = pos_of(q, kTri[t][1]), c = pos_of(q, kTri[t][2]);
                const double u0 = P[b][0] - P[a][0], u1 = P[b][1] - P[a][1], u2 = P[b][2] - P[a][2];
                const double v0 = P[c][0] - P[a][0], v1 = P[c][1] - P[a][1], v2 = P[c][2] - P[a][2];
                sum[0] += u1 * v2 - u2 * v1;
                sum[1] += u2 * v0 - u0 * v2;
                sum[2] += u0 * v1 - u1 * v0;
            }
    const double nn = sqrt((sum[0] * sum[0] + sum[1] * sum[1]) + sum[2] * sum[2]);
    const bool flat = !(nn > 0.0);
    double edges = 0.0;
    int count = 0;
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        if (p == 4) continue;
        if (uses[p] > 0) {
            const double d0 = P[p][0] - P[4][0], d1 = P[p][1] - P[4][1], d2 = P[p][2] - P[4][2];
            edges += sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            ++count;
        }
    }
    const int64_t slot = vscan[i];
    const bool stored = v.refine_status && v.refine_status[i] == OSFM_DENSE_REFINE_REFINED;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        mesh.points[3 * slot + j] = P[4][j];
        mesh.normals[3 * slot + j] = stored ? v.refine_normal[3 * i + j] : flat ? 0.0 : sum[j] / nn;
    }
    mesh.scale[slot] = edges / (double)count;
    const int d = min((int)dist[i], iterations);
    mesh.confidence[slot] = flat ? 0.0f : iterations == 0 ? 1.0f : (float)d / (float)iterations;
    mesh.pixel[2 * slot] = x; mesh.pixel[2 * slot + 1] = y;
    mesh.vclass[slot] = cls[i];
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void launch_solid(hipStream_t s, const View &v, uint8_t *solid, unsigned long long *counters)
{
    const int64_t n = (int64_t)v.w * v.h;
    if (n <= 0) return;
    hipLaunchKernelGGL(mesh_solid_kernel, dim3(blocks_of(n)), dim3(256), 0, s, v, solid, counters);
}

void launch_label(hipStream_t s, int w, int h, int min_island, uint8_t *solid, int32_t *parent, int32_t *local, int32_t *tile_size,
    int32_t *size, unsigned long long *counters)
{
    const int64_t n = (int64_t)w * h;
    if (n <= 0) return;
    const dim3 tiles((unsigned)((w + kLabelTileW - 1) / kLabelTileW), (unsigned)((h + kLabelTileH - 1) / kLabelTileH));
    hipLaunchKernelGGL(mesh_label_tile_kernel, tiles, dim3(kLabelThreads), 0, s, w, h, solid, parent, local, tile_size, size, counters);
    hipLaunchKernelGGL(mesh_label_seam_kernel, dim3(blocks_of(n)), dim3(256), 0, s, w, h, solid, parent, counters);
    hipLaunchKernelGGL(mesh_label_root_kernel, dim3(blocks_of(n)), dim3(256), 0, s, w, h, solid, parent, local, tile_size, size, counters);
    hipLaunchKernelGGL(mesh_label_clear_kernel, dim3(blocks_of(n)), dim3(256), 0, s, w, h, min_island, solid, local, size, counters);
}

void launch_blocks(hipStream_t s, const View &v, const uint8_t *solid, double thr, double thr_diag, uint8_t *blocks, int32_t *tflags,
    unsigned long long *counters)
{
    const int64_t n = (int64_t)v.w * v.h;
    if (n <= 0) return;
    hipLaunchKernelGGL(mesh_blocks_kernel, dim3(blocks_of(n)), dim3(256), 0, s, v, solid, thr > 0.0 ? 1 : 0, thr, thr_diag, blocks, tflags,
        counters);
}

void launch_vertices(hipStream_t s, int w, int h, const uint8_t *blocks, int32_t *vflags, uint8_t *cls, uint8_t *links, uint8_t *dist,
    unsigned long long *counters)
{
    const int64_t n = (int64_t)w * h;
    if (n <= 0) return;
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3(blocks_of(n)), dim3(256), 0, s, w, h, blocks, vflags, cls, links, dist, counters);
}

void launch_distance_round(hipStream_t s, int w, int h, const uint8_t *links, const uint8_t *in, uint8_t *out)
{
    const int64_t n = (int64_t)w * h;
    if (n <= 0) return;
    hipLaunchKernelGGL(mesh_distance_kernel, dim3(blocks_of(n)), dim3(256), 0, s, w, h, links, in, out);
}

void launch_emit(hipStream_t s, const View &v, const uint8_t *blocks, const int32_t *vflags, const int32_t *vscan, const int32_t *tscan,
    const uint8_t *cls, const uint8_t *dist, int iterations, Mesh mesh)
{
    const int64_t n = (int64_t)v.w * v.h;
    if (n <= 0) return;
    hipLaunchKernelGGL(mesh_emit_kernel, dim3(blocks_of(n)), dim3(256), 0, s, v, blocks, vflags, vscan, tscan, cls, dist, iterations, mesh);
}

double footprint(const dense::ViewGeo &g)
{
    const double b0[3] = {g.B[0][0], g.B[1][0], g.B[2][0]}, b1[3] = {g.B[0][1], g.B[1][1], g.B[2][1]};
    const double c[3] = {b0[1] * b1[2] - b0[2] * b1[1], b0[2] * b1[0] - b0[0] * b1[2], b0[0] * b1[1] - b0[1] * b1[0]};
    return std::sqrt(std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]));
}

}  // namespace mesh
}  // namespace osfm
