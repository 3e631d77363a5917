// Scan preparation, part 1: Open3D's voxel_down_sample (geotransformer/utils/open3d.py:57-65) for stacked clouds: the stages of
// csrc/grid_subsample.hip (bounds, hash, rank, fill, select) under Open3D's voxel semantics, on the scan and bounding box of block_ops.h.
// se3et_amd/scan_prep.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off.)
//
//   voxel_bounds_kernel   one workgroup per cloud: float64 bounding box, the non-finite flag, the extent check, the origin.
//   voxel_insert_kernel   one thread per point: 63-bit key of three 21-bit indices into the cloud's open-addressing table by a 64-bit CAS,
//                         atomicMin of the first-seen input index, atomicAdd of the member count (integer atomics only).
//   voxel_rank_kernel     one workgroup per cloud: prefix sum over the "I am my voxel's first member" flags ranks the voxels by first-seen
//                         index (no sort), a second prefix sum over the counts in rank order places the member lists.
//   voxel_fill_kernel     one thread per point: appends its index to its voxel's member list (integer atomic cursor).
//   voxel_mean_kernel     one thread per voxel of at most 64 members: orders the members by input index (insertion sort: lists are
//                         short, and arrive almost ordered), sums serially, divides once, writes with plain stores.
//   voxel_large_kernel    one workgroup per cloud, for the voxels above 64 members (a voxel size far above the point spacing; none in a
//                         usual call, which costs a scan of the counts): the workgroup ranks the members of such a voxel together (each
//                         member's place is the number of smaller indices), then one thread sums in that order -- the same bits.
//
// Contract (points (n, 3) float32 or float64, optional normals (n, 3) of the same type, voxel_size > 0; everything float64, float32 inputs
// promoted on load).
//   - origin o_d = min_d - 0.5 voxel_size; voxel index i_d = floor((p_d - o_d) / voxel_size): a true division, no reciprocal multiply.
//   - a cloud is refused when an axis would need 2^21 voxels or more ((max_d - o_d) / voxel_size >= 2^21), when voxel_size is not a
//     positive finite number (on the host, before any launch), or when a point is non-finite: the last two are bits 2 and 1 of a device
//     status word that the caller reads in the same host synchronisation that fetches the output counts.
//   - output row of a voxel: the float64 mean of its members, each coordinate summed sequentially in ascending input index, then divided
//     once by the count.  Normals: the same mean of the members' normals, NOT renormalised.
//   - output order: voxels ascend in the input index of their first member (Open3D's order is its unordered_map's: unspecified).
//   - n = 0 gives an empty output.  No float atomics: a cloud's output is bit-identical alone or anywhere in a batch, and from run to run.
#include <math.h>

#include <unordered_map>
#include <vector>

#include "common.h"
#include "stack_rows.h"
#include "voxel_key.h"

namespace {

constexpr int kVoxelThreads = 256;
constexpr int kVoxelSerialMax = 64;                   // members that one thread orders; larger voxels are ordered by a workgroup
constexpr int kVoxelNonFinite = 1, kVoxelTooMany = 2;
constexpr unsigned long long kVoxelEmptyKey = ~0ull;
constexpr int64_t kVoxelMaxPoints = (1ll << 30) - 64;          // table slots (2 n + clouds) and every index stay below 2^31

// ---- the contract's arithmetic: the same text on the host and on the device -------------------------------------------------------------------
// mean of rows members[0 .. count) (ascending) of `src` (cloud-local rows from row0)
PG_HD void vd_mean(const void* src, int elem, int64_t row0, const int* members, int count, double* out) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t < count; t++)
    for (int d = 0; d < 3; d++) s[d] += pg_load(src, elem, 3 * (row0 + members[t]) + d);
  for (int d = 0; d < 3; d++) out[d] = s[d] / (double)count;
}

struct VoxelMeta {
  double org[3];
  int ok, flags;                   // flags: 0, or why the cloud is refused (the status bits)
};

// per cloud c: table slots [2 start_c + c, 2 start_c + c + cap_c), cap_c = 2 n_c + 1; per point / per voxel arrays by the stacked row
struct VoxelLayout {
  VoxelMeta* meta;                 // [P]
  unsigned long long* keys;        // [T]  T = 2 n + P
  int* first;                      // [T]  lowest input index of the slot's voxel
  int* count;                      // [T]  members of the slot's voxel
  int* cursor;                     // [n]  fill position of voxel (start_c + rank)      (count and cursor are zeroed together)
  int* vrank;                      // [T]  rank of the slot's voxel in its cloud's output
  int* slot_of;                    // [n]  table slot of every point
  int* member_start;               // [n]  first member of voxel (start_c + rank) in `members` (cloud-local)
  int* voxel_count;                // [n]  members of voxel (start_c + rank)
  int* members;                    // [n]  member lists, cloud by cloud
  int* ordered;                    // [n]  the lists of the large voxels in ascending order (same places as `members`)
};

size_t vd_carve(int64_t n_total, int num_clouds, char* base, VoxelLayout* L) {
  Se3Carver c(base);
  const size_t n = (size_t)(n_total > 0 ? n_total : 1), P = (size_t)(num_clouds > 0 ? num_clouds : 1), T = 2 * n + P;
  VoxelLayout l;
  l.meta = c.take<VoxelMeta>(P);
  l.keys = c.take<unsigned long long>(T);
  l.first = c.take<int>(T);
  l.count = c.take<int>(T + n);
  l.cursor = l.count + T;
  l.vrank = c.take<int>(T);
  l.slot_of = c.take<int>(n);
  l.member_start = c.take<int>(n);
  l.voxel_count = c.take<int>(n);
  l.members = c.take<int>(n);
  l.ordered = c.take<int>(n);
  if (L) *L = l;
  return c.bytes();
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_bounds_kernel(const void* __restrict__ pts, const void* __restrict__ nrm, int elem,
                                                                     PairRows rows, double voxel_size, VoxelLayout L, int* __restrict__ status) {
  __shared__ double sh[kVoxelThreads / 64];
  __shared__ int bad;
  const int c = blockIdx.x;
  const int64_t s0 = rows.start[c], n = rows.start[c + 1] - s0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool finite = true;
  for (int64_t i = s0 + threadIdx.x; i < s0 + n; i += kVoxelThreads)
    for (int d = 0; d < 3; d++) {
      const double v = pg_load(pts, elem, 3 * i + d);
      finite = finite && isfinite(v) && (!nrm || isfinite(pg_load(nrm, elem, 3 * i + d)));
      mn[d] = fmin(mn[d], v);
      mx[d] = fmax(mx[d], v);
    }
  if (!finite) bad = kVoxelNonFinite;                       // (every writer stores the same word)
  se3_block_bounds<double, kVoxelThreads>(mn, mx, sh);
  if (threadIdx.x == 0) {
    VoxelMeta* m = L.meta + c;
    int flags = bad;
    for (int d = 0; d < 3; d++) {
      m->org[d] = vd_origin(mn[d], voxel_size);
      if (n > 0 && !flags && !vd_axis_ok(mx[d], m->org[d], voxel_size)) flags |= kVoxelTooMany;
    }
    m->ok = flags == 0;
    m->flags = flags;
    if (flags) atomicOr(status, flags);
  }
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_insert_kernel(const void* __restrict__ pts, int elem, PairRows rows, int64_t n_total,
                                                                     double voxel_size, VoxelLayout L) {
  const int64_t i = (int64_t)blockIdx.x * kVoxelThreads + threadIdx.x;
  if (i >= n_total) return;
  const int c = pg_pair_of_row(rows, i);
  if (!L.meta[c].ok) return;
  const int64_t s0 = rows.start[c], base = 2 * s0 + c;
  const unsigned long long cap = 2ull * (unsigned long long)(rows.start[c + 1] - s0) + 1ull;
  double p[3];
  pg_load3(pts, elem, i, p);
  const unsigned long long key = vd_key(p, L.meta[c].org, voxel_size);
  unsigned long long h = ((key * 0x9E3779B97F4A7C15ull) >> 20) % cap;
  for (unsigned long long probe = 0; probe < cap; probe++) {             // (the table has more slots than the cloud has points: it ends)
    const unsigned long long seen = atomicCAS(L.keys + base + h, kVoxelEmptyKey, key);
    if (seen == kVoxelEmptyKey || seen == key) break;
    h = h + 1 == cap ? 0 : h + 1;
  }
  const int64_t slot = base + (int64_t)h;
  atomicMin(L.first + slot, (int)(i - s0));
  atomicAdd(L.count + slot, 1);
  L.slot_of[i] = (int)slot;
}

__global__ __launch_bounds__(1024) void voxel_rank_kernel(PairRows rows, VoxelLayout L, int* __restrict__ out_counts) {
  __shared__ int sh[1024];
  const int c = blockIdx.x, t = threadIdx.x;
  const int64_t s0 = rows.start[c];
  const int n = L.meta[c].ok ? (int)(rows.start[c + 1] - s0) : 0;
  const int chunk = (n + 1023) / 1024;
  const int lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  int sum = 0, voxels;
  for (int i = lo; i < hi; i++) sum += L.first[L.slot_of[s0 + i]] == i;
  int run = se3_block_exclusive(sum, sh, &voxels);
  for (int i = lo; i < hi; i++) {
    const int slot = L.slot_of[s0 + i];
    if (L.first[slot] == i) {
      L.vrank[slot] = run;
      L.voxel_count[s0 + run] = L.count[slot];
      run++;
    }
  }
  if (t == 0) out_counts[c] = L.meta[c].ok ? voxels : -L.meta[c].flags;          // a refused cloud: minus its status bits
  __syncthreads();                                                       // voxel_count[s0 .. s0 + voxels) is written
  const int vchunk = (voxels + 1023) / 1024;
  const int vlo = t * vchunk < voxels ? t * vchunk : voxels, vhi = vlo + vchunk < voxels ? vlo + vchunk : voxels;
  sum = 0;
  for (int v = vlo; v < vhi; v++) sum += L.voxel_count[s0 + v];
  int total;
  run = se3_block_exclusive(sum, sh, &total);
  for (int v = vlo; v < vhi; v++) {
    L.member_start[s0 + v] = run;
    run += L.voxel_count[s0 + v];
  }
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_fill_kernel(PairRows rows, int64_t n_total, VoxelLayout L) {
  const int64_t i = (int64_t)blockIdx.x * kVoxelThreads + threadIdx.x;
  if (i >= n_total) return;
  const int c = pg_pair_of_row(rows, i);
  if (!L.meta[c].ok) return;
  const int64_t s0 = rows.start[c];
  const int v = L.vrank[L.slot_of[i]];
  const int pos = atomicAdd(L.cursor + s0 + v, 1);
  L.members[s0 + L.member_start[s0 + v] + pos] = (int)(i - s0);
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_mean_kernel(const void* __restrict__ pts, const void* __restrict__ nrm, int elem,
                                                                   PairRows rows, int64_t n_total, VoxelLayout L,
                                                                   const int* __restrict__ out_counts, double* __restrict__ out_points,
                                                                   double* __restrict__ out_normals) {
  const int64_t i = (int64_t)blockIdx.x * kVoxelThreads + threadIdx.x;
  if (i >= n_total) return;
  const int c = pg_pair_of_row(rows, i);
  const int64_t s0 = rows.start[c];
  const int v = (int)(i - s0);
  if (!L.meta[c].ok || v >= out_counts[c]) return;
  int64_t row = v;                                                        // output rows: the clouds back to back
  for (int b = 0; b < c; b++) row += out_counts[b] > 0 ? out_counts[b] : 0;
  int* mem = L.members + s0 + L.member_start[s0 + v];
  const int count = L.voxel_count[s0 + v];
  if (count > kVoxelSerialMax) return;                                    // voxel_large_kernel's
  for (int a = 1; a < count; a++) {                                       // ascending input index (the arrival order was the atomics')
    const int x = mem[a];
    int b = a;
    for (; b > 0 && mem[b - 1] > x; b--) mem[b] = mem[b - 1];
    mem[b] = x;
  }
  double m[3];
  vd_mean(pts, elem, s0, mem, count, m);
  for (int d = 0; d < 3; d++) out_points[3 * row + d] = m[d];
  if (nrm) {
    vd_mean(nrm, elem, s0, mem, count, m);
    for (int d = 0; d < 3; d++) out_normals[3 * row + d] = m[d];
  }
}

__global__ __launch_bounds__(kVoxelThreads) void voxel_large_kernel(const void* __restrict__ pts, const void* __restrict__ nrm, int elem,
                                                                    PairRows rows, VoxelLayout L, const int* __restrict__ out_counts,
                                                                    double* __restrict__ out_points, double* __restrict__ out_normals) {
  __shared__ int large[kVoxelThreads];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (!L.meta[c].ok) return;                                              // (uniform over the workgroup, like every branch around a barrier below)
  const int64_t s0 = rows.start[c];
  const int voxels = out_counts[c];
  int64_t row0 = 0;
  for (int b = 0; b < c; b++) row0 += out_counts[b] > 0 ? out_counts[b] : 0;
  for (int base = 0; base < voxels; base += kVoxelThreads) {
    const int mine = base + tid < voxels && L.voxel_count[s0 + base + tid] > kVoxelSerialMax;
    large[tid] = mine;
    if (!__syncthreads_or(mine)) continue;                                // no large voxel among these 256
    for (int j = 0; j < kVoxelThreads; j++) {
      if (!large[j]) continue;
      const int v = base + j, count = L.voxel_count[s0 + v];
      const int* mem = L.members + s0 + L.member_start[s0 + v];
      int* ord = L.ordered + s0 + L.member_start[s0 + v];
      for (int a = tid; a < count; a += kVoxelThreads) {                  // the indices are distinct: the ranks are a permutation
        const int x = mem[a];
        int pos = 0;
        for (int t = 0; t < count; t++) pos += mem[t] < x;
        ord[pos] = x;
      }
      __syncthreads();
      double m[3];
      if (tid == 0) {
        vd_mean(pts, elem, s0, ord, count, m);
        for (int d = 0; d < 3; d++) out_points[3 * (row0 + v) + d] = m[d];
      }
      if (tid == SE3_WAVE && nrm) {
        vd_mean(nrm, elem, s0, ord, count, m);
        for (int d = 0; d < 3; d++) out_normals[3 * (row0 + v) + d] = m[d];
      }
    }
    __syncthreads();                                                      // `large` is rewritten by the next round
  }
}

bool voxel_size_ok(double v) { return isfinite(v) && v > 0.0; }

}  // namespace

extern "C" size_t se3_voxel_downsample_workspace_bytes(int64_t n_total, int num_clouds) {
  if (n_total < 0 || n_total > kVoxelMaxPoints || num_clouds < 0 || num_clouds > kPairMaxPairs) return 0;
  return vd_carve(n_total, num_clouds, nullptr, nullptr);
}

extern "C" int se3_voxel_downsample_stack(const void* points, int elem, const void* normals, const int64_t* offsets_host, int num_clouds,
                                          double voxel_size, double* out_points, double* out_normals, int* out_counts, int* status,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  SE3_REQUIRE(points && offsets_host && out_points && out_counts && status && workspace && (out_normals || !normals), SE3_ERR_INVALID_ARG,
              "voxel_downsample_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "voxel_downsample_stack: %d clouds (at most %d), elem %d", num_clouds, kPairMaxPairs, elem);
  SE3_REQUIRE(voxel_size_ok(voxel_size), SE3_ERR_INVALID_ARG, "voxel_downsample_stack: voxel size %g is not a positive finite number", voxel_size);
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "voxel_downsample_stack: offsets must start at 0 and not decrease");
  const int64_t n_total = rows.start[num_clouds];
  SE3_REQUIRE(n_total <= kVoxelMaxPoints, SE3_ERR_UNSUPPORTED, "voxel_downsample_stack: %lld points in one call", (long long)n_total);
  VoxelLayout L;
  SE3_REQUIRE(vd_carve(n_total, num_clouds, (char*)workspace, &L) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "voxel_downsample_stack: workspace of %zu bytes is too small", workspace_bytes);
  if (num_clouds == 0) return SE3_OK;                                     // (nothing is launched and nothing written)
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)(n_total > 0 ? n_total : 1), T = 2 * n + (size_t)num_clouds;
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess || hipMemsetAsync(L.keys, 0xff, sizeof(unsigned long long) * T, st) != hipSuccess ||
      hipMemsetAsync(L.first, 0x7f, sizeof(int) * T, st) != hipSuccess ||                   // 0x7f7f7f7f: above every index
      hipMemsetAsync(L.count, 0, sizeof(int) * (T + n), st) != hipSuccess) {
    se3_set_error("voxel_downsample_stack: hipMemsetAsync failed");
    return SE3_ERR_LAUNCH;
  }
  const unsigned blocks = (unsigned)se3_cdiv(n_total, kVoxelThreads);
  voxel_bounds_kernel<<<(unsigned)num_clouds, kVoxelThreads, 0, st>>>(points, normals, elem, rows, voxel_size, L, status);
  if (n_total > 0) voxel_insert_kernel<<<blocks, kVoxelThreads, 0, st>>>(points, elem, rows, n_total, voxel_size, L);
  voxel_rank_kernel<<<(unsigned)num_clouds, 1024, 0, st>>>(rows, L, out_counts);
  if (n_total > 0) {
    voxel_fill_kernel<<<blocks, kVoxelThreads, 0, st>>>(rows, n_total, L);
    voxel_mean_kernel<<<blocks, kVoxelThreads, 0, st>>>(points, normals, elem, rows, n_total, L, out_counts, out_points, out_normals);
    voxel_large_kernel<<<(unsigned)num_clouds, kVoxelThreads, 0, st>>>(points, normals, elem, rows, L, out_counts, out_points, out_normals);
  }
  SE3_CHECK_LAUNCH("voxel_downsample_stack");
  return SE3_OK;
}

// The contract on host memory for one cloud, no GPU: the same index, key, extent and mean text, a std::unordered_map for the table.
// *status: 0, or the bits of the device status word (then *out_count = 0).
extern "C" int se3_debug_voxel_downsample_host(const void* points, int64_t n, int elem, const void* normals, double voxel_size, double* out_points,
                                               double* out_normals, int64_t* out_count, int* status) {
  SE3_REQUIRE(points && out_points && out_count && status && (out_normals || !normals), SE3_ERR_INVALID_ARG,
              "debug_voxel_downsample_host: null pointer");
  SE3_REQUIRE(n >= 0 && n <= kVoxelMaxPoints && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_voxel_downsample_host: n %lld, elem %d",
              (long long)n, elem);
  SE3_REQUIRE(voxel_size_ok(voxel_size), SE3_ERR_INVALID_ARG, "debug_voxel_downsample_host: voxel size %g is not a positive finite number",
              voxel_size);
  *out_count = 0, *status = 0;
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, org[3];
  for (int64_t i = 0; i < 3 * n; i++) {
    const double v = pg_load(points, elem, i);
    if (!isfinite(v) || (normals && !isfinite(pg_load(normals, elem, i)))) *status = kVoxelNonFinite;
    mn[i % 3] = fmin(mn[i % 3], v), mx[i % 3] = fmax(mx[i % 3], v);
  }
  for (int d = 0; d < 3; d++) {
    org[d] = vd_origin(mn[d], voxel_size);
    if (n > 0 && !*status && !vd_axis_ok(mx[d], org[d], voxel_size)) *status |= kVoxelTooMany;
  }
  if (*status || n == 0) return SE3_OK;
  std::unordered_map<unsigned long long, int> rank;
  std::vector<std::vector<int>> members;
  for (int64_t i = 0; i < n; i++) {
    double p[3];
    pg_load3(points, elem, i, p);
    const auto it = rank.emplace(vd_key(p, org, voxel_size), (int)members.size());
    if (it.second) members.emplace_back();
    members[(size_t)it.first->second].push_back((int)i);
  }
  for (size_t v = 0; v < members.size(); v++) {
    vd_mean(points, elem, 0, members[v].data(), (int)members[v].size(), out_points + 3 * v);
    if (normals) vd_mean(normals, elem, 0, members[v].data(), (int)members[v].size(), out_normals + 3 * v);
  }
  *out_count = (int64_t)members.size();
  return SE3_OK;
}
