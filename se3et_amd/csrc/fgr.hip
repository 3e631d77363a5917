// Fast Global Registration of stacked pairs, resident on the device: Open3D's registration_fgr_based_on_correspondence (Zhou, Park,
// Koltun, ECCV 2016; FastGlobalRegistration.cpp, versions >= 0.13) for up to SE3_PAIR_MAX_PAIRS pairs per call, three launches, nothing read
// back.  csrc/fgr_core.h holds the text as __host__ __device__ functions, csrc/icp_core.h the ordered sum, the 6x6 solve, the composition
// and the series, csrc/splitmix.h the sampler; se3et_amd/fgr.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
//   fgr_normalize_kernel   one workgroup of 256 threads per pair: the refusals (0) and the figures of the normalisation (3).
//   fgr_tuple_kernel       one workgroup per pair: the tuple test (1) in an exact parallel form of the serial loop.  Trials run in chunks of
//                          SE3_FGR_TUPLE_CHUNK = 256 in trial order, one per thread; a block exclusive scan (block_ops.h) over the accept
//                          flags ranks the accepted ones; those with a rank below the cap are written; the workgroup leaves, uniformly, once
//                          the shared total reaches the cap.  No atomics.  (Not launched without the tuple test.)
//   fgr_optimize_kernel    one workgroup per pair: the count (2), all iteration_number steps of the loop (4) in ONE launch, M and mu in
//                          registers, then the original scale and the inverse (5).  Static LDS 27 x 256 x 8 bytes = 54 KiB, as for
//                          generalized ICP; no global state beyond the transform, mu and the status.
//
// Contract (one pair).  Source S (ns, 3) and reference R (nr, 3), float32 or float64, promoted to float64 on load.  Correspondences C are
// (K, 2) int64 rows of (src row, ref row), as ransac_pairs takes them.  All arithmetic is float64 with contraction off.  The result is T
// with ref ~ T src.
//   0. Refusals.  A non-finite coordinate in either cloud sets SE3_FGR_NONFINITE and gives a NaN transform, like ICP.  An empty cloud or
//      K = 0 sets SE3_FGR_EMPTY and gives the identity.  An index of C outside its cloud sets SE3_FGR_BAD_INDEX and gives a NaN transform.
//      They are tested in this order and the first that holds is the only one set (an empty cloud has no index to be wrong about).
//   1. Tuple test (tuple_test; Open3D's AdvancedMatching).  Trials are t = 0 .. 100 K - 1.  Trial t draws
//        a_j = ((splitmix64(splitmix64(seed) + 3 t + j) >> 32) * K) >> 32,  j = 0, 1, 2                      (uint64 wrap-around)
//      which is ransac.sample_indices(seed, K, 100 K, 3)[t]: the sampler of csrc/ransac.hip, one text in csrc/splitmix.h.  The squared edges
//      ls_e, lr_e are taken in each cloud between the points of rows C[a_0], C[a_1], C[a_2], for the edges (0, 1), (1, 2), (2, 0), each as
//      (dx dx + dy dy) + dz dz.  The trial is accepted iff for all three edges ls_e tau2 < lr_e and lr_e tau2 < ls_e, with
//      tau2 = tuple_scale tuple_scale rounded once.  The first maximum_tuple_count accepted trials in trial order each append C[a_0], C[a_1],
//      C[a_2] to the working list C'; duplicates are kept.  Without the tuple test C' = C.
//      Differences from Open3D: the random stream (Open3D's is not reproducible); and the comparison, which is on squared lengths in place
//      of li tau < lj && lj < li / tau: no root and no division, so host and device agree to the bit.  Degenerate triples reject themselves
//      through the strict inequalities.
//   2. Too few correspondences.  |C'| < 10 gives the identity and sets SE3_FGR_TOO_FEW.
//   3. Normalisation (NormalizePointCloud, over ALL rows of both clouds, not only the matched ones).  Each cloud's mean is taken in the
//      icp_sum order (lane l of 256 adds rows l, l + 256, .. serially, then a fixed tree over the lanes) and divided by the row count; the
//      clouds are centred; scale = sqrt(max over both clouds of the centred squared norm (dx dx + dy dy) + dz dz).
//      use_absolute_scale false: g = scale, mu = 1; true: g = 1, mu = scale.  The centred points are divided by g.  A scale that is not
//      > 0 gives the identity and sets SE3_FGR_SINGULAR.
//   4. GNC loop (OptimizePairwiseRegistration).  The REFERENCE cloud is the moving one.  Start from M = I; run it = 0 ..
//      iteration_number - 1.  For each row of C', with p the normalised source point and q' = M q the moved normalised reference point
//      ((M0 q0 + M1 q1) + M2 q2, then + M3): d = p - q'; the weight is w = (mu / (d.d + mu))^2; each coordinate a has a Jacobian row J with
//      J[3 + a] = -1, J[(a+1)%3] = -q'[(a+2)%3] and J[(a+2)%3] = q'[(a+1)%3].  The sums A = sum w J J^T (21 terms) and b = sum w J d_a
//      (6 terms) are taken through icp_sum<27>.  A x = -b is solved by icp_cholesky6; a failure sets SE3_FGR_SINGULAR, takes the identity
//      update, and the loop goes on.  The update is U = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5], then M <- U M with icp_compose.  After the
//      update: if decrease_mu and it % 4 == 0 and mu > maximum_correspondence_distance, then mu <- mu / division_factor.  As in Open3D,
//      maximum_correspondence_distance is compared in NORMALISED units unless use_absolute_scale.
//      Difference from Open3D: q' is recomputed from M each iteration; Open3D moves a copy incrementally, so the rounding differs.
//      Step angles.  A numpy sketch of this contract took steps of up to 1.14 rad on clean flat clouds, so ICP's 1 rad refusal is wrong
//      here.  The sine and cosine of an angle with |a| < SE3_FGR_MAX_ANGLE = 4 come from icp_sin / icp_cos of a / 4, followed by two
//      double-angle steps (s <- (2 s) c, c <- c c - s s), every operation rounded on its own, so host and device agree to the bit.  A
//      non-finite angle, or |a| >= 4, sets SE3_FGR_STEP_REFUSED; the pair then ends with the M it had.
//   5. Original scale and direction.  M maps ref to src, so A_R = M_R and A_t = -M_R mean_R + g M_t + mean_S.  The rigid inverse is
//      returned in closed form, (A_R^T, -A_R^T A_t).
//   6. Evaluation (Open3D's returned RegistrationResult).  fitness and inlier_rmse of T at maximum_correspondence_distance are taken on
//      the original clouds through the ICP entry with max_iteration = 0 (se3et_amd/fgr.py); there is no kernel for it here.
//   Results are bit-identical from run to run, for a pair alone or in any batch, and between the device and se3_debug_fgr_host.
#include <math.h>

#include <vector>

#include "common.h"
#include "fgr_core.h"          // (and through it icp_core.h, pair_grid.h, splitmix.h)

namespace {

// what the kernels get: the stacked arrays of a call
struct FgrCall {
  const void* src;
  int src_elem;
  PairRows src_rows;
  const void* ref;
  int ref_elem;
  PairRows ref_rows;
  const int64_t* corr;
  PairRows corr_rows;
  int64_t* tuples;                // (P, 3 cap, 2) or null
  int64_t* trials;                // (P, cap) or null
  double* norm;                   // (P, 8)
  double* T;
  int* status;
  int* ncorr;
  int* ntuples;
  double* mu;                     // or null
};

__host__ __device__ const void* fgr_rows_at(const void* base, int elem, int64_t row) {
  return elem ? (const void*)((const double*)base + 3 * row) : (const void*)((const float*)base + 3 * row);
}

__host__ __device__ FgrPair fgr_pair_of(const FgrCall& c, int cap, int p) {
  FgrPair v;
  const int64_t s0 = c.src_rows.start[p], r0 = c.ref_rows.start[p], c0 = c.corr_rows.start[p];
  v.src = fgr_rows_at(c.src, c.src_elem, s0), v.src_elem = c.src_elem, v.ns = c.src_rows.start[p + 1] - s0;
  v.ref = fgr_rows_at(c.ref, c.ref_elem, r0), v.ref_elem = c.ref_elem, v.nr = c.ref_rows.start[p + 1] - r0;
  v.corr = c.corr + 2 * c0, v.K = c.corr_rows.start[p + 1] - c0;
  v.tuples = c.tuples ? c.tuples + (int64_t)p * 6 * cap : nullptr;
  v.trials = c.trials ? c.trials + (int64_t)p * cap : nullptr;
  v.norm = c.norm + 8 * p, v.T = c.T + 16 * p, v.status = c.status + p, v.ncorr = c.ncorr + p, v.ntuples = c.ntuples + p;
  v.mu = c.mu ? c.mu + p : nullptr;
  return v;
}

__global__ __launch_bounds__(kFgrLanes) void fgr_normalize_kernel(FgrCall c, FgrParams prm) {
  __shared__ double sh[3 * kFgrLanes];
  const FgrPair v = fgr_pair_of(c, prm.cap, blockIdx.x);
  fgr_pair_normalize(v, prm, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

__global__ __launch_bounds__(kFgrLanes) void fgr_tuple_kernel(FgrCall c, FgrParams prm) {
  __shared__ int sh[kFgrLanes];
  const FgrPair v = fgr_pair_of(c, prm.cap, blockIdx.x);
  if (*v.status != 0) return;                              // (refused or empty: written by the launch before; uniform)
  const int64_t trials = kFgrTrialsPerCorrespondence * v.K;
  int total = 0;
  for (int64_t base = 0; base < trials && total < prm.cap; base += kFgrChunk) {
    int chunk_total = 0;
    fgr_tuple_chunk(v, prm, base, trials, total, threadIdx.x, threadIdx.x + 1,
                    [&](bool ok) { return se3_block_exclusive<int, kFgrLanes>(ok ? 1 : 0, sh, &chunk_total); });
    total += chunk_total;                                  // (read from LDS by every thread: the loop's test is uniform)
  }
  if (threadIdx.x == 0) {
    const int kept = total < prm.cap ? total : prm.cap;
    *v.ntuples = kept;
    *v.ncorr = 3 * kept;
  }
}

__global__ __launch_bounds__(kFgrLanes) void fgr_optimize_kernel(FgrCall c, FgrParams prm) {
  __shared__ double sh[kFgrSums * kFgrLanes];
  const FgrPair v = fgr_pair_of(c, prm.cap, blockIdx.x);
  fgr_pair_optimize(v, prm, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

struct FgrLayout {
  double* norm;
  int64_t* tuples;
};

size_t fgr_carve(int num_pairs, int cap, int tuple_test, char* base, FgrLayout* L) {
  Se3Carver c(base);
  FgrLayout l;
  const size_t P = (size_t)(num_pairs > 0 ? num_pairs : 1);
  l.norm = c.take<double>(8 * P);
  l.tuples = c.take<int64_t>(tuple_test ? 6 * P * (size_t)(cap > 0 ? cap : 1) : 1);
  if (L) *L = l;
  return c.bytes();
}

bool fgr_params(FgrParams* prm, double maxdist, double division_factor, int use_absolute_scale, int decrease_mu, int iteration_number,
                double tuple_scale, int cap, int tuple_test, uint64_t seed) {
  if (!(maxdist > 0.0) || !(maxdist < INFINITY) || !(division_factor >= 1.0) || !(division_factor < INFINITY)) return false;
  if (iteration_number < 0 || iteration_number > SE3_FGR_MAX_ITERATION || !(tuple_scale > 0.0) || !(tuple_scale <= 1.0)) return false;
  if (cap < 0 || cap > SE3_FGR_MAX_TUPLE_COUNT) return false;
  prm->maxdist = maxdist, prm->division_factor = division_factor, prm->tau2 = tuple_scale * tuple_scale;
  prm->use_absolute_scale = use_absolute_scale != 0, prm->decrease_mu = decrease_mu != 0, prm->iteration_number = iteration_number;
  prm->tuple_test = tuple_test != 0, prm->cap = cap, prm->key = splitmix64(seed);
  return true;
}

#define FGR_PARAMS_TEXT                                                                                                                  \
  "%s: distance %g (finite, > 0), division_factor %g (finite, >= 1), iteration_number %d (0 .. %d), tuple_scale %g (in (0, 1]), "       \
  "maximum_tuple_count %d (0 .. %d)"

}  // namespace

extern "C" size_t se3_fgr_workspace_bytes(int num_pairs, int maximum_tuple_count, int tuple_test) {
  if (num_pairs < 0 || num_pairs > kPairMaxPairs || maximum_tuple_count < 0 || maximum_tuple_count > SE3_FGR_MAX_TUPLE_COUNT) return 0;
  return fgr_carve(num_pairs, maximum_tuple_count, tuple_test, nullptr, nullptr);
}

extern "C" int se3_fgr_stack(const void* src_points, int src_elem, const int64_t* src_offsets_host, const void* ref_points, int ref_elem,
                             const int64_t* ref_offsets_host, const int64_t* correspondences, const int64_t* corr_offsets_host, int num_pairs,
                             double maximum_correspondence_distance, double division_factor, int use_absolute_scale, int decrease_mu,
                             int iteration_number, double tuple_scale, int maximum_tuple_count, int tuple_test, uint64_t seed,
                             double* out_transforms, int* out_status, int* out_num_correspondences, int* out_num_tuples, double* out_mu,
                             int64_t* out_tuples, int64_t* out_trials, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "fgr_stack";
  SE3_REQUIRE(src_points && ref_points && correspondences && src_offsets_host && ref_offsets_host && corr_offsets_host && workspace,
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_transforms && out_status && out_num_correspondences && out_num_tuples, SE3_ERR_INVALID_ARG, "%s: null result pointer", what);
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs && (src_elem == 0 || src_elem == 1) && (ref_elem == 0 || ref_elem == 1),
              SE3_ERR_INVALID_ARG, "%s: %d pairs (at most %d), src_elem %d, ref_elem %d", what, num_pairs, kPairMaxPairs, src_elem, ref_elem);
  FgrParams prm;
  SE3_REQUIRE(fgr_params(&prm, maximum_correspondence_distance, division_factor, use_absolute_scale, decrease_mu, iteration_number, tuple_scale,
                         maximum_tuple_count, tuple_test, seed),
              SE3_ERR_INVALID_ARG, FGR_PARAMS_TEXT, what, maximum_correspondence_distance, division_factor, iteration_number,
              SE3_FGR_MAX_ITERATION, tuple_scale, maximum_tuple_count, SE3_FGR_MAX_TUPLE_COUNT);
  FgrCall c;
  SE3_REQUIRE(pg_fill_rows(&c.src_rows, src_offsets_host, num_pairs) && pg_fill_rows(&c.ref_rows, ref_offsets_host, num_pairs) &&
                  pg_fill_rows(&c.corr_rows, corr_offsets_host, num_pairs),
              SE3_ERR_INVALID_ARG, "%s: offsets must start at 0 and not decrease", what);
  for (int p = 0; p < num_pairs; p++)
    SE3_REQUIRE(c.corr_rows.start[p + 1] - c.corr_rows.start[p] <= SE3_FGR_MAX_CORRESPONDENCES, SE3_ERR_UNSUPPORTED,
                "%s: pair %d has %lld correspondences (at most %d)", what, p, (long long)(c.corr_rows.start[p + 1] - c.corr_rows.start[p]),
                SE3_FGR_MAX_CORRESPONDENCES);
  FgrLayout L;
  SE3_REQUIRE(fgr_carve(num_pairs, prm.cap, prm.tuple_test, (char*)workspace, &L) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "%s: workspace of %zu bytes is too small", what, workspace_bytes);
  if (num_pairs == 0) return SE3_OK;
  c.src = src_points, c.src_elem = src_elem, c.ref = ref_points, c.ref_elem = ref_elem, c.corr = correspondences;
  c.tuples = prm.tuple_test ? (out_tuples ? out_tuples : L.tuples) : nullptr;
  c.trials = prm.tuple_test ? out_trials : nullptr;
  c.norm = L.norm, c.T = out_transforms, c.status = out_status, c.ncorr = out_num_correspondences, c.ntuples = out_num_tuples, c.mu = out_mu;
  hipStream_t st = (hipStream_t)stream;
  fgr_normalize_kernel<<<(unsigned)num_pairs, kFgrLanes, 0, st>>>(c, prm);
  if (prm.tuple_test) fgr_tuple_kernel<<<(unsigned)num_pairs, kFgrLanes, 0, st>>>(c, prm);
  fgr_optimize_kernel<<<(unsigned)num_pairs, kFgrLanes, 0, st>>>(c, prm);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ---- the same text on host memory, one pair, no GPU (tests/test_fgr_cpu.py, tools/fgr_probe.py) ------------------------------------------------
extern "C" int se3_debug_fgr_host(const void* src_points, int64_t ns, int src_elem, const void* ref_points, int64_t nr, int ref_elem,
                                  const int64_t* correspondences, int64_t num_correspondences, double maximum_correspondence_distance,
                                  double division_factor, int use_absolute_scale, int decrease_mu, int iteration_number, double tuple_scale,
                                  int maximum_tuple_count, int tuple_test, uint64_t seed, double* out_transform, int* out_status,
                                  int* out_num_correspondences, int* out_num_tuples, double* out_mu, int64_t* out_tuples, int64_t* out_trials) {
  const char* what = "debug_fgr_host";
  SE3_REQUIRE(src_points && ref_points && correspondences, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_transform && out_status && out_num_correspondences && out_num_tuples, SE3_ERR_INVALID_ARG, "%s: null result pointer", what);
  SE3_REQUIRE(ns >= 0 && nr >= 0 && num_correspondences >= 0 && (src_elem == 0 || src_elem == 1) && (ref_elem == 0 || ref_elem == 1),
              SE3_ERR_INVALID_ARG, "%s: ns %lld, nr %lld, %lld correspondences, src_elem %d, ref_elem %d", what, (long long)ns, (long long)nr,
              (long long)num_correspondences, src_elem, ref_elem);
  SE3_REQUIRE(num_correspondences <= SE3_FGR_MAX_CORRESPONDENCES, SE3_ERR_UNSUPPORTED, "%s: %lld correspondences (at most %d)", what,
              (long long)num_correspondences, SE3_FGR_MAX_CORRESPONDENCES);
  FgrParams prm;
  SE3_REQUIRE(fgr_params(&prm, maximum_correspondence_distance, division_factor, use_absolute_scale, decrease_mu, iteration_number, tuple_scale,
                         maximum_tuple_count, tuple_test, seed),
              SE3_ERR_INVALID_ARG, FGR_PARAMS_TEXT, what, maximum_correspondence_distance, division_factor, iteration_number,
              SE3_FGR_MAX_ITERATION, tuple_scale, maximum_tuple_count, SE3_FGR_MAX_TUPLE_COUNT);
  std::vector<double> sh((size_t)kFgrSums * kFgrLanes), norm(8);
  std::vector<int64_t> tuples(prm.tuple_test && !out_tuples ? (size_t)6 * (prm.cap > 0 ? prm.cap : 1) : 1);
  FgrPair v;
  v.src = src_points, v.src_elem = src_elem, v.ns = ns, v.ref = ref_points, v.ref_elem = ref_elem, v.nr = nr;
  v.corr = correspondences, v.K = num_correspondences;
  v.tuples = prm.tuple_test ? (out_tuples ? out_tuples : tuples.data()) : nullptr;
  v.trials = prm.tuple_test ? out_trials : nullptr;
  v.norm = norm.data(), v.T = out_transform, v.status = out_status, v.ncorr = out_num_correspondences, v.ntuples = out_num_tuples, v.mu = out_mu;
  auto none = [] {};
  fgr_pair_normalize(v, prm, 0, kFgrLanes, sh.data(), none);
  if (prm.tuple_test && *v.status == 0) {
    const int64_t trials = kFgrTrialsPerCorrespondence * v.K;
    int total = 0;
    for (int64_t base = 0; base < trials && total < prm.cap; base += kFgrChunk) {
      int run = 0;
      fgr_tuple_chunk(v, prm, base, trials, total, 0, kFgrLanes, [&](bool ok) {
        const int before = run;
        run += ok ? 1 : 0;
        return before;
      });
      total += run;
    }
    const int kept = total < prm.cap ? total : prm.cap;
    *v.ntuples = kept, *v.ncorr = 3 * kept;
  }
  fgr_pair_optimize(v, prm, 0, kFgrLanes, sh.data(), none);
  return SE3_OK;
}

extern "C" int se3_debug_fgr_sincos_host(const double* x, int64_t n, double* out_sin, double* out_cos) {
  SE3_REQUIRE(x && out_sin && out_cos && n >= 0, SE3_ERR_INVALID_ARG, "debug_fgr_sincos_host: null pointer or n %lld", (long long)n);
  for (int64_t i = 0; i < n; i++) {
    SE3_REQUIRE(fabs(x[i]) < kFgrMaxAngle, SE3_ERR_INVALID_ARG, "debug_fgr_sincos_host: %g is outside (-4, 4)", x[i]);
    fgr_sincos(x[i], &out_sin[i], &out_cos[i]);
  }
  return SE3_OK;
}
