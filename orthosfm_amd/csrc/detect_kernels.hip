// The scan and the compaction of the detectors' count / scan / write scheme (see detect_kernels.h).
#include "detect_kernels.h"

namespace osfm {
namespace detect {

namespace {

// Exclusive scan of counts[n] in place by one workgroup; *total = the sum.
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void scan_kernel(int32_t *counts, int n, int32_t *total)
{
    __shared__ int buf[kScanBlock];
    int carry = 0;
    for (int base = 0; base < n; base += kScanBlock) {
        const int i = base + threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kScanBlock; off <<= 1) {
            const int t = (int)threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) counts[i] = carry + buf[threadIdx.x] - v;
        const int chunk = buf[kScanBlock - 1];
        __syncthreads();
        carry += chunk;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kBlock) void compact_kernel(const Keypoint *in, const uint8_t *keep, const int32_t *offsets, int n,
    Keypoint *out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool flag = i < n && keep[i] != 0;
    int total;
    const int rank = block_rank(flag, &total);
    if (flag) out[offsets[blockIdx.x] + rank] = in[i];   // at most n rows: `out` holds as many as `in`
}

}  // namespace

void launch_scan(hipStream_t s, int32_t *counts, int n, int32_t *total)
{
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanBlock), 0, s, counts, n, total);
}

void launch_compact(hipStream_t s, const Keypoint *in, const uint8_t *keep, const int32_t *offsets, int n, Keypoint *out)
{
    hipLaunchKernelGGL(compact_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, in, keep, offsets, n, out);
}

}  // namespace detect
}  // namespace osfm
