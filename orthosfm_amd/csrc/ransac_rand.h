// The counter-based generator of the library's RANSACs: draw `draw` of iteration `it` of stream `pair` (a view
// pair of the geometric verification, a camera group of the Tomasi-Kanade alignment) under `seed` is a pure
// function of the four, so results are reproducible and independent of launch geometry, batching and sharding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace osfm {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t ransac_rand(uint64_t seed, uint64_t pair, uint64_t it, uint64_t draw)
{
    return splitmix64(splitmix64(seed ^ (pair * 0xD1342543DE82EF95ull)) + it * 0x2545F4914F6CDD1Dull + draw);
}

}  // namespace osfm
