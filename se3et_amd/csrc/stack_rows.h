// The rows of a stacked call: up to kPairMaxPairs pairs (or clouds) end to end in one array.  What every tool on stacked clouds needs and
// nothing more -- the descriptor that kernels take by value, the owner of a row, the promoting load of a float32 or float64 array, the
// host-side check of a caller's offsets -- as __host__ __device__ or inline text.  csrc/pair_grid.h builds the float64 cell grid and its
// searches on top; a file that needs no grid (csrc/voxel_downsample.hip) includes this header alone.
#pragma once
#include <stdint.h>

#define PG_HD __host__ __device__ __forceinline__

constexpr int kPairMaxPairs = 32;                                      // pairs per stacked call (SE3_PAIR_MAX_PAIRS)

// pair p's rows [start[p], start[p + 1]) of a stacked array; passed to kernels by value
struct PairRows {
  int64_t start[kPairMaxPairs + 1];
  int n;
};

// the pair (or cloud) that owns row i of a stacked array
PG_HD int pg_pair_of_row(const PairRows& rows, int64_t i) {
  int p = 0;
  while (p + 1 < rows.n && i >= rows.start[p + 1]) p++;
  return p;
}

// element i of a float32 (elem 0) or float64 (elem 1) array, as float64
PG_HD double pg_load(const void* p, int elem, int64_t i) { return elem ? ((const double*)p)[i] : (double)((const float*)p)[i]; }

// row `row` of an (n, 3) array
PG_HD void pg_load3(const void* p, int elem, int64_t row, double* out) {
  out[0] = pg_load(p, elem, 3 * row), out[1] = pg_load(p, elem, 3 * row + 1), out[2] = pg_load(p, elem, 3 * row + 2);
}

// host-side offsets -> PairRows; false unless 0 = offsets[0] <= offsets[1] <= ...  The unused tail repeats the last offset.
inline bool pg_fill_rows(PairRows* rows, const int64_t* offsets, int num_pairs) {
  rows->n = num_pairs;
  if (offsets[0] != 0) return false;
  for (int p = 0; p <= num_pairs; p++) {
    rows->start[p] = offsets[p];
    if (p > 0 && offsets[p] < offsets[p - 1]) return false;
  }
  for (int p = num_pairs + 1; p <= kPairMaxPairs; p++) rows->start[p] = offsets[num_pairs];
  return true;
}

// one cloud of n rows
inline PairRows pg_single_rows(int64_t n) {
  const int64_t offsets[2] = {0, n};
  PairRows rows;
  pg_fill_rows(&rows, offsets, 1);
  return rows;
}
