// The counter-based sampler that RANSAC (csrc/ransac.hip) and the tuple test of Fast Global Registration (csrc/fgr_core.h) share, as
// __host__ __device__ text: the standard splitmix64 and the draw
//   idx_j(h) = ((splitmix64(key + h * rn + j) >> 32) * n) >> 32,   key = splitmix64(seed)          (uint64 wrap-around)
// which se3et_amd/ransac.py's sample_indices restates in numpy.  It depends on (seed, h, j, n) alone.
#pragma once
#include <stdint.h>

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw j of the rn draws of trial h among n entries, n < 2^32
__host__ __device__ __forceinline__ int64_t splitmix_draw(uint64_t key, uint64_t h, uint64_t rn, uint64_t j, uint64_t n) {
  return (int64_t)(((splitmix64(key + h * rn + j) >> 32) * n) >> 32);
}
