// Feature-space matching for stacked pairs: the nearest neighbour of every descriptor in the other cloud of its pair, in both directions,
// and the correspondence lists built from the two index arrays (extract_correspondences_from_feats of
// geotransformer/modules/registration/matching.py:135-170, extract_corr_indices_from_feats of utils/registration.py:179-212).  The (N, M)
// distance matrix of the reference never exists: the memory is O(N + M).
//
// Pair p owns rows [ref_offsets[p], ref_offsets[p+1]) of ref_feats and [src_offsets[p], src_offsets[p+1]) of src_feats (int64, DEVICE).
// Direction 0 searches every ref row in the src cloud of its pair, direction 1 every src row in the ref cloud.  Contract, per direction with
// query rows x and key rows y:
//   ranking   candidates are ranked by v(i, j) = (|x_i|^2 - 2 x_i.y_j) + |y_j|^2 in float32: the dot product is accumulated by
//             v_mfma_f32_16x16x4_f32 in a fixed channel order (per 16-channel step k0 + i, k0 + 4 + i, k0 + 8 + i, k0 + 12 + i for
//             i = 0..3), a norm is one fixed-order sum per row (feature_norm_kernel).  v is a function of the two rows only, never of
//             their position in a tile, a segment or a batch.
//   ties      among exactly equal v the lowest key index wins (the order (v, j) is total, so any reduction tree gives the same winner).
//   distance  the squared distance returned is recomputed for the winner as sum_k (x_k - y_k)^2, not the cancelling expression.
//   non-finite   a candidate is taken only if v < +inf, so a NaN or infinite v is never chosen; a row without such a candidate (or with
//             an empty other cloud) gets index -1 and distance +inf.
//   determinism  no atomics and no arrival order anywhere: a pair's results are bit-identical from run to run and in any batch.
//
// Three launches, no host synchronisation:
//   feature_norm_kernel        one wave per row of either cloud: |x|^2.
//   feature_nn_sweep_kernel    a workgroup owns a strip of 128 stacked query rows (a wave 32 of them) and one of S segments of the key
//                              tiles of the rows' pair; a wave computes 32 x 64 values per tile as 2 x 4 MFMA tiles from operands loaded
//                              straight from global memory (the strip's four waves read the same key rows: L1 hits), and keeps the running
//                              (v, j) of its rows in registers.  A strip that spans several pairs sweeps each of them in turn.  Both
//                              directions are slices of one grid.  Writes one (v, j) per row and segment.
//   feature_nn_select_kernel   one wave per row: the best of its S partials in segment order, then the direct squared distance.
//
// Correspondence extraction (se3_feature_corr_count_stack / _fill_stack): count, exclusive scan, fill over the pair-major sequence
// [ref rows of pair 0, src rows of pair 0, ref rows of pair 1, ...], so that pair p's entries are one contiguous range:
//   mode 0  one-way              (i, nn_src(i)) for every ref row i
//   mode 1  mutual               rows with nn_ref(nn_src(i)) == i, ascending in i
//   mode 2  bilateral, mask form the union of {(i, nn_src(i))} and {(nn_ref(j), j)}, duplicates once, in row-major (i, j) order (nonzero of
//                                the OR-ed masks).  The rank of an entry inside its row i is count{j' < j : nn_ref(j') == i}, counted by a
//                                plain scan of the pair's nn_ref (a wave reads one address at a time: a broadcast), not by atomics.
//   mode 3  bilateral, concatenated form   [arange(N), nn_ref] / [nn_src, arange(M)], duplicates kept
// A row whose index is -1 (or outside its pair) produces nothing.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SE3_WAVE;
constexpr int kStrip = 32 * kWaves;        // query rows per workgroup
constexpr int kTile = 64;                  // keys per tile
constexpr int kMaxSegments = 16;
constexpr int kTargetBlocks = 1024;        // segments are added until the grid has about this many workgroups

template <bool VEC>
__device__ __forceinline__ f32x4 fn_load4(const float* row, int k, int C) {
  if (VEC) return k < C ? *reinterpret_cast<const f32x4*>(row + k) : f32x4{0.f, 0.f, 0.f, 0.f};      // C % 4 == 0: k < C covers k + 3
  f32x4 v;
#pragma unroll
  for (int i = 0; i < 4; i++) v[i] = k + i < C ? row[k + i] : 0.f;
  return v;
}

// the pair of stacked row `row`: the first p with off[p + 1] > row (empty pairs are skipped; row < off[P])
__device__ __forceinline__ int pair_of_row(const int64_t* __restrict__ off, int P, int64_t row) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid + 1] > row) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// norms[0, nref) of the ref rows, norms[nref, nref + nsrc) of the src rows
__global__ __launch_bounds__(kThreads) void feature_norm_kernel(const float* __restrict__ ref, const float* __restrict__ src, int64_t nref,
                                                                int64_t nsrc, int C, float* __restrict__ norms) {
  const int64_t row = (int64_t)blockIdx.x * kWaves + threadIdx.x / SE3_WAVE;
  if (row >= nref + nsrc) return;
  const float* x = row < nref ? ref + row * C : src + (row - nref) * C;
  float s = 0.f;
  for (int k = se3_lane(); k < C; k += SE3_WAVE) s = __builtin_fmaf(x[k], x[k], s);
  s = se3_wave_sum(s);
  if (se3_lane() == 0) norms[row] = s;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void feature_nn_sweep_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                                    const int64_t* __restrict__ ref_off, const int64_t* __restrict__ src_off,
                                                                    int P, int64_t nref, int64_t nsrc, int C, int ref_strips, int S,
                                                                    const float* __restrict__ norms, float* __restrict__ part_v,
                                                                    int32_t* __restrict__ part_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, kq = lane >> 4;
  const bool fwd = (int)blockIdx.x < ref_strips;                       // direction 0: ref rows query the src cloud
  const float* q = fwd ? ref : src;
  const float* key = fwd ? src : ref;
  const int64_t* qoff = fwd ? ref_off : src_off;
  const int64_t* koff = fwd ? src_off : ref_off;
  const int64_t nq = fwd ? nref : nsrc, nk = fwd ? nsrc : nref, qbase = fwd ? 0 : nref;
  const float* qn = norms + qbase;
  const float* kn = norms + (fwd ? nref : 0);
  const int64_t r0 = (int64_t)((int)blockIdx.x - (fwd ? 0 : ref_strips)) * kStrip;
  const int64_t rend = r0 + kStrip < nq ? r0 + kStrip : nq;
  const int64_t w0 = r0 + 32 * wave;                                   // this wave's 32 rows
  const int g = blockIdx.y;
  const float inf = __builtin_inff();
  for (int p = pair_of_row(qoff, P, r0); p < P && qoff[p] < rend; p++) {
    const int64_t qlo = qoff[p] > r0 ? qoff[p] : r0, qhi = qoff[p + 1] < rend ? qoff[p + 1] : rend;
    if (qlo >= qhi || w0 >= qhi || w0 + 32 <= qlo) continue;           // (wave-uniform; the kernel has no barrier)
    const int64_t kb = koff[p], ke = koff[p + 1] < nk ? koff[p + 1] : nk;
    const int64_t nkp = ke > kb ? ke - kb : 0;
    const int64_t tiles = (nkp + kTile - 1) / kTile, per = (tiles + S - 1) / S;
    const int64_t t0 = g * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    const float* xr[2];
    float xn[2][4];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      xr[t] = q + clamp64(w0 + 16 * t + c, qlo, qhi - 1) * C;          // rows outside the pair's part of the strip are clamped, never written
#pragma unroll
      for (int r = 0; r < 4; r++) xn[t][r] = qn[clamp64(w0 + 16 * t + 4 * kq + r, qlo, qhi - 1)];
    }
    float bv[2][4];
    int bi[2][4];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) bv[t][r] = inf, bi[t][r] = -1;
    for (int64_t tile = t0; tile < t1; tile++) {
      const int col0 = (int)(tile * kTile);
      const float* yr[4];
      float yn[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int64_t col = col0 + 16 * t + c < nkp ? col0 + 16 * t + c : nkp - 1;
        yr[t] = key + (kb + col) * C;
        yn[t] = kn[kb + col];
      }
      f32x4 acc[2][4];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 a[2], b[4];
#pragma unroll
      for (int t = 0; t < 2; t++) a[t] = fn_load4<VEC>(xr[t], 4 * kq, C);
#pragma unroll
      for (int t = 0; t < 4; t++) b[t] = fn_load4<VEC>(yr[t], 4 * kq, C);
      for (int k0 = 0; k0 < C; k0 += 16) {
        f32x4 an[2], bn[4];
#pragma unroll
        for (int t = 0; t < 2; t++) an[t] = fn_load4<VEC>(xr[t], k0 + 16 + 4 * kq, C);   // the next step's rows behind this step's MFMAs
#pragma unroll
        for (int t = 0; t < 4; t++) bn[t] = fn_load4<VEC>(yr[t], k0 + 16 + 4 * kq, C);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int tj = 0; tj < 4; tj++) acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti][i], b[tj][i], acc[ti][tj], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 2; t++) a[t] = an[t];
#pragma unroll
        for (int t = 0; t < 4; t++) b[t] = bn[t];
      }
      // acc[ti][tj][r] = x[w0 + 16 ti + 4 kq + r] . y[col0 + 16 tj + c]; a lane meets its keys in ascending order, so `<` keeps the lowest
#pragma unroll
      for (int tj = 0; tj < 4; tj++) {
        const int col = col0 + 16 * tj + c;
        const bool live = col < nkp;
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float v = (xn[ti][r] - 2.0f * acc[ti][tj][r]) + yn[tj];
            if (live && v < bv[ti][r]) bv[ti][r] = v, bi[ti][r] = col;   // false for a NaN and for +inf
          }
      }
    }
    // the 16 lanes of a quarter hold the candidates of the same rows: the least (v, j) of them
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = bv[ti][r];
        int j = bi[ti][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float ov = __shfl_xor(v, o);
          const int oj = __shfl_xor(j, o);
          if (ov < v || (ov == v && oj < j)) v = ov, j = oj;
        }
        const int64_t row = w0 + 16 * ti + 4 * kq + r;
        if (c == 0 && row >= qlo && row < qhi) {
          part_v[(qbase + row) * S + g] = v;
          part_i[(qbase + row) * S + g] = j;
        }
      }
  }
}

__global__ __launch_bounds__(kThreads) void feature_nn_select_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                                     const int64_t* __restrict__ ref_off, const int64_t* __restrict__ src_off,
                                                                     int P, int64_t nref, int64_t nsrc, int C, int S,
                                                                     const float* __restrict__ part_v, const int32_t* __restrict__ part_i,
                                                                     int64_t* __restrict__ nn_src_idx, float* __restrict__ nn_src_dist,
                                                                     int64_t* __restrict__ nn_ref_idx, float* __restrict__ nn_ref_dist) {
  const int64_t row = (int64_t)blockIdx.x * kWaves + threadIdx.x / SE3_WAVE;
  if (row >= nref + nsrc) return;
  const bool fwd = row < nref;
  const int64_t r = fwd ? row : row - nref;
  float bv = __builtin_inff();
  int bj = -1;
  for (int g = 0; g < S; g++) {                                        // segments hold ascending key ranges: `<` keeps the lowest index
    const float v = part_v[row * S + g];
    if (v < bv) bv = v, bj = part_i[row * S + g];
  }
  float d = __builtin_inff();
  if (bj >= 0) {
    const int p = pair_of_row(fwd ? ref_off : src_off, P, r);
    const float* x = (fwd ? ref : src) + r * C;
    const float* y = (fwd ? src : ref) + ((fwd ? src_off : ref_off)[p] + bj) * C;
    float s = 0.f;
    for (int k = se3_lane(); k < C; k += SE3_WAVE) {
      const float e = x[k] - y[k];
      s = __builtin_fmaf(e, e, s);
    }
    d = se3_wave_sum(s);
  }
  if (se3_lane() == 0) {
    (fwd ? nn_src_idx : nn_ref_idx)[r] = bj;
    (fwd ? nn_src_dist : nn_ref_dist)[r] = d;
  }
}

int segments_for(int64_t nref, int64_t nsrc) {
  const int64_t strips = se3_cdiv(nref, kStrip) + se3_cdiv(nsrc, kStrip);
  const int64_t s = strips > 0 ? se3_cdiv(kTargetBlocks, strips) : 1;
  return (int)(s < 1 ? 1 : (s > kMaxSegments ? kMaxSegments : s));
}

// ---- correspondence extraction ------------------------------------------------------------------------------------------------------------
struct CorrView {
  const int64_t* nn_src;     // (nref) pair-local src index of every ref row, -1: none
  const int64_t* nn_ref;     // (nsrc) pair-local ref index of every src row
  const int64_t* ref_off;
  const int64_t* src_off;
  int P;
  int64_t nref, nsrc;
  int mode;
};

struct CorrElement {         // element e of the pair-major sequence
  int p;
  bool is_ref;
  int64_t local, n, m;       // its row in its cloud, the pair's ref and src rows
  const int64_t* ns;         // the pair's nn_src / nn_ref
  const int64_t* nr;
  int64_t vbase;             // the sequence index of the pair's first ref row
};

__device__ __forceinline__ CorrElement corr_locate(const CorrView& v, int64_t e) {
  int lo = 0, hi = v.P - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v.ref_off[mid + 1] + v.src_off[mid + 1] > e) hi = mid;
    else lo = mid + 1;
  }
  CorrElement c;
  c.p = lo;
  c.vbase = v.ref_off[lo] + v.src_off[lo];
  c.n = v.ref_off[lo + 1] - v.ref_off[lo];
  c.m = v.src_off[lo + 1] - v.src_off[lo];
  c.local = e - c.vbase;
  c.is_ref = c.local < c.n;
  if (!c.is_ref) c.local -= c.n;
  c.ns = v.nn_src + v.ref_off[lo];
  c.nr = v.nn_ref + v.src_off[lo];
  return c;
}

// src rows j' < limit of the pair whose nearest ref row is i
__device__ __forceinline__ int64_t corr_count_before(const int64_t* __restrict__ nr, int64_t i, int64_t limit) {
  int64_t n = 0;
  for (int64_t j = 0; j < limit; j++) n += nr[j] == i;
  return n;
}

__global__ __launch_bounds__(kThreads) void feature_corr_count_kernel(CorrView v, int64_t* __restrict__ counts) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= v.nref + v.nsrc) return;
  const CorrElement c = corr_locate(v, e);
  int64_t n = 0;
  if (c.is_ref) {
    const int64_t j = c.ns[c.local];
    const bool valid = j >= 0 && j < c.m;
    const bool mutual = valid && c.nr[j] == c.local;
    if (v.mode == 1) n = mutual;
    else if (v.mode == 2) n = (int64_t)valid + corr_count_before(c.nr, c.local, c.m) - (int64_t)mutual;
    else n = valid;
  } else if (v.mode == 3) {
    const int64_t i = c.nr[c.local];
    n = i >= 0 && i < c.n;
  }
  counts[e] = n;
}

__global__ __launch_bounds__(kThreads) void feature_corr_fill_kernel(CorrView v, const int64_t* __restrict__ offsets, int64_t total,
                                                                     int64_t* __restrict__ out_ref, int64_t* __restrict__ out_src) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= v.nref + v.nsrc) return;
  const CorrElement c = corr_locate(v, e);
  int64_t pos = -1, i = 0, j = 0;
  if (c.is_ref) {
    i = c.local, j = c.ns[i];
    const bool valid = j >= 0 && j < c.m;
    if (v.mode == 1 ? (valid && c.nr[j] == i) : valid) pos = offsets[e] + (v.mode == 2 ? corr_count_before(c.nr, i, j) : 0);
  } else if (v.mode == 3) {
    j = c.local, i = c.nr[j];
    if (i >= 0 && i < c.n) pos = offsets[e];
  } else if (v.mode == 2) {
    j = c.local, i = c.nr[j];
    if (i >= 0 && i < c.n && c.ns[i] != j) {                           // (the ref row wrote (i, nn_src(i)) itself)
      const int64_t jd = c.ns[i];
      const bool extra = jd >= 0 && jd < j && c.nr[jd] != i;           // the row's own entry lies before j and is not among the counted
      pos = offsets[c.vbase + i] + corr_count_before(c.nr, i, j) + (int64_t)extra;
    }
  }
  if (pos >= 0 && pos < total) out_ref[pos] = i, out_src[pos] = j;
}

int corr_args_ok(const int64_t* nn_src, const int64_t* nn_ref, const int64_t* ref_off, const int64_t* src_off, int num_pairs, int64_t nref,
                 int64_t nsrc, int mode, const char* what) {
  SE3_REQUIRE(num_pairs >= 0 && nref >= 0 && nsrc >= 0, SE3_ERR_INVALID_ARG, "%s: %d pairs, %lld ref rows, %lld src rows", what, num_pairs,
              (long long)nref, (long long)nsrc);
  SE3_REQUIRE(mode >= 0 && mode <= 3, SE3_ERR_INVALID_ARG, "%s: mode %d (0 one-way, 1 mutual, 2 bilateral mask, 3 bilateral concatenated)",
              what, mode);
  SE3_REQUIRE(ref_off && src_off && (nref == 0 || nn_src) && (nsrc == 0 || nn_ref), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_pairs > 0 || nref + nsrc == 0, SE3_ERR_INVALID_ARG, "%s: rows without pairs", what);
  return SE3_OK;
}

}  // namespace

extern "C" size_t se3_feature_nn_workspace_bytes(int64_t num_ref_rows, int64_t num_src_rows) {
  if (num_ref_rows < 0 || num_src_rows < 0) return 0;
  const size_t rows = (size_t)(num_ref_rows + num_src_rows);
  const size_t S = (size_t)segments_for(num_ref_rows, num_src_rows);
  Se3Carver c(nullptr);
  c.take<float>(rows), c.take<float>(rows * S), c.take<int32_t>(rows * S);
  return c.bytes() + 256;
}

extern "C" int se3_feature_nn_stack(const float* ref_feats, const float* src_feats, const int64_t* ref_offsets, const int64_t* src_offsets,
                                    int num_pairs, int64_t num_ref_rows, int64_t num_src_rows, int channels, void* workspace,
                                    size_t workspace_bytes, int64_t* nn_src_indices, float* nn_src_sq_distances, int64_t* nn_ref_indices,
                                    float* nn_ref_sq_distances, void* stream) {
  SE3_REQUIRE(num_pairs >= 0 && num_ref_rows >= 0 && num_src_rows >= 0, SE3_ERR_INVALID_ARG,
              "feature_nn_stack: %d pairs, %lld ref rows, %lld src rows", num_pairs, (long long)num_ref_rows, (long long)num_src_rows);
  SE3_REQUIRE(channels >= 1, SE3_ERR_INVALID_ARG, "feature_nn_stack: %d channels", channels);
  const int64_t rows = num_ref_rows + num_src_rows;
  if (rows == 0) return SE3_OK;
  SE3_REQUIRE(num_pairs > 0, SE3_ERR_INVALID_ARG, "feature_nn_stack: rows without pairs");
  SE3_REQUIRE(rows / kWaves + 2 < (1ll << 31), SE3_ERR_UNSUPPORTED, "feature_nn_stack: %lld rows", (long long)rows);
  SE3_REQUIRE(ref_offsets && src_offsets && (num_ref_rows == 0 || (ref_feats && nn_src_indices && nn_src_sq_distances)) &&
                  (num_src_rows == 0 || (src_feats && nn_ref_indices && nn_ref_sq_distances)),
              SE3_ERR_INVALID_ARG, "feature_nn_stack: null pointer");
  const size_t need = se3_feature_nn_workspace_bytes(num_ref_rows, num_src_rows);
  SE3_REQUIRE(workspace && workspace_bytes >= need, SE3_ERR_INVALID_ARG, "feature_nn_stack: workspace of %zu bytes, %zu needed",
              workspace_bytes, need);
  const int S = segments_for(num_ref_rows, num_src_rows), C = channels;
  Se3Carver c((void*)se3_align256((uintptr_t)workspace));
  float* norms = c.take<float>((size_t)rows);
  float* part_v = c.take<float>((size_t)rows * S);
  int32_t* part_i = c.take<int32_t>((size_t)rows * S);
  hipStream_t st = (hipStream_t)stream;
  const unsigned row_blocks = (unsigned)se3_cdiv(rows, kWaves);
  const int ref_strips = (int)se3_cdiv(num_ref_rows, kStrip), src_strips = (int)se3_cdiv(num_src_rows, kStrip);
  feature_norm_kernel<<<row_blocks, kThreads, 0, st>>>(ref_feats, src_feats, num_ref_rows, num_src_rows, C, norms);
  const dim3 grid((unsigned)(ref_strips + src_strips), (unsigned)S);
  const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(ref_feats) | reinterpret_cast<uintptr_t>(src_feats)) & 15) == 0;
  if (vec)
    feature_nn_sweep_kernel<true><<<grid, kThreads, 0, st>>>(ref_feats, src_feats, ref_offsets, src_offsets, num_pairs, num_ref_rows,
                                                             num_src_rows, C, ref_strips, S, norms, part_v, part_i);
  else
    feature_nn_sweep_kernel<false><<<grid, kThreads, 0, st>>>(ref_feats, src_feats, ref_offsets, src_offsets, num_pairs, num_ref_rows,
                                                              num_src_rows, C, ref_strips, S, norms, part_v, part_i);
  feature_nn_select_kernel<<<row_blocks, kThreads, 0, st>>>(ref_feats, src_feats, ref_offsets, src_offsets, num_pairs, num_ref_rows,
                                                            num_src_rows, C, S, part_v, part_i, nn_src_indices, nn_src_sq_distances,
                                                            nn_ref_indices, nn_ref_sq_distances);
  SE3_CHECK_LAUNCH("feature_nn_stack");
  return SE3_OK;
}

extern "C" int se3_feature_corr_count_stack(const int64_t* nn_src_indices, const int64_t* nn_ref_indices, const int64_t* ref_offsets,
                                            const int64_t* src_offsets, int num_pairs, int64_t num_ref_rows, int64_t num_src_rows, int mode,
                                            int64_t* entry_offsets, void* stream) {
  const int ok = corr_args_ok(nn_src_indices, nn_ref_indices, ref_offsets, src_offsets, num_pairs, num_ref_rows, num_src_rows, mode,
                              "feature_corr_count_stack");
  if (ok != SE3_OK) return ok;
  SE3_REQUIRE(entry_offsets, SE3_ERR_INVALID_ARG, "feature_corr_count_stack: null pointer");
  const int64_t rows = num_ref_rows + num_src_rows;
  hipStream_t st = (hipStream_t)stream;
  const CorrView v{nn_src_indices, nn_ref_indices, ref_offsets, src_offsets, num_pairs, num_ref_rows, num_src_rows, mode};
  if (rows > 0) feature_corr_count_kernel<<<(unsigned)se3_cdiv(rows, kThreads), kThreads, 0, st>>>(v, entry_offsets);
  se3_exclusive_scan_i64(entry_offsets, rows, st);
  SE3_CHECK_LAUNCH("feature_corr_count_stack");
  return SE3_OK;
}

extern "C" int se3_feature_corr_fill_stack(const int64_t* nn_src_indices, const int64_t* nn_ref_indices, const int64_t* ref_offsets,
                                           const int64_t* src_offsets, int num_pairs, int64_t num_ref_rows, int64_t num_src_rows, int mode,
                                           const int64_t* entry_offsets, int64_t total, int64_t* ref_corr_indices,
                                           int64_t* src_corr_indices, void* stream) {
  const int ok = corr_args_ok(nn_src_indices, nn_ref_indices, ref_offsets, src_offsets, num_pairs, num_ref_rows, num_src_rows, mode,
                              "feature_corr_fill_stack");
  if (ok != SE3_OK) return ok;
  SE3_REQUIRE(total >= 0, SE3_ERR_INVALID_ARG, "feature_corr_fill_stack: total %lld", (long long)total);
  const int64_t rows = num_ref_rows + num_src_rows;
  if (total == 0 || rows == 0) return SE3_OK;
  SE3_REQUIRE(entry_offsets && ref_corr_indices && src_corr_indices, SE3_ERR_INVALID_ARG, "feature_corr_fill_stack: null pointer");
  const CorrView v{nn_src_indices, nn_ref_indices, ref_offsets, src_offsets, num_pairs, num_ref_rows, num_src_rows, mode};
  feature_corr_fill_kernel<<<(unsigned)se3_cdiv(rows, kThreads), kThreads, 0, (hipStream_t)stream>>>(v, entry_offsets, total,
                                                                                                   ref_corr_indices, src_corr_indices);
  SE3_CHECK_LAUNCH("feature_corr_fill_stack");
  return SE3_OK;
}
