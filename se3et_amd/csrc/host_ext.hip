// Host-pointer (CPU) variants of the two ops of the reference's pybind extension `geotransformer.ext` ("plus CPU
// (host-pointer) variants ... for DataLoader workers"): the reference runs them inside forked DataLoader workers
// (geotransformer/utils/data.py:159-209, utils/torch.py:65-75), where a HIP context cannot be used.  Plain C++ on host memory, stateless,
// safe to call concurrently from several processes / threads; same arithmetic contract as the device kernels (csrc/grid_subsample.hip,
// csrc/radius_neighbors.hip) and as the reference sources:
//   grid subsampling   extensions/cpu/grid_subsampling/grid_subsampling_cpu.cpp:3-109, grid_subsampling_cpu.h:24-74
//   radius neighbours  extensions/cpu/radius_neighbors/radius_neighbors_cpu.cpp:3-91 (nanoflann radius search, sorted by distance)
// SE3_EXACT_FP: compiled with -ffp-contract=off (se3et_amd/build.py): the float expressions mirror unfused x86 arithmetic.
#define SE3_EXACT_FP 1
#include "common.h"
#include <math.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace {

// One cloud.  Output order = iteration order of a std::unordered_map<size_t, ...> filled in first-seen voxel order -- the very container
// (and libstdc++) the reference iterates, so the emission order is reproduced by construction.
int64_t grid_subsample_one(const float* pts, const float* nrm, int64_t n, float voxel, float* s_pts, float* s_nrm) {
  if (n == 0) return 0;
  float mn[3] = {pts[0], pts[1], pts[2]}, mx[3] = {pts[0], pts[1], pts[2]};
  for (int64_t i = 0; i < n; i++)
    for (int d = 0; d < 3; d++) {
      const float v = pts[3 * i + d];
      if (v < mn[d]) mn[d] = v;
      if (v > mx[d]) mx[d] = v;
    }
  const float inv = (float)(1.0 / (double)voxel);          // `minCorner * (1. / voxel_size)`: the scale is rounded to float by operator*
  float org[3];
  for (int d = 0; d < 3; d++) org[d] = floorf(mn[d] * inv) * voxel;
  const size_t nx = (size_t)(floorf((mx[0] - org[0]) / voxel) + 1), ny = (size_t)(floorf((mx[1] - org[1]) / voxel) + 1);
  struct Cell { int count; float sx, sy, sz; int64_t best; double best_d; };
  std::unordered_map<size_t, int64_t> slot_of;             // voxel id -> dense slot, keys inserted in first-seen order
  std::vector<Cell> cells;
  std::vector<int64_t> cell_of((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    // (through the signed conversion, explicitly: an index of -1 -- float rounding at the cloud's own minimum -- wraps as in the reference's
    // x86-64 build, grid_subsampling_cpu.cpp:47-49)
    const size_t ix = (size_t)(int64_t)floorf((pts[3 * i] - org[0]) / voxel), iy = (size_t)(int64_t)floorf((pts[3 * i + 1] - org[1]) / voxel),
                 iz = (size_t)(int64_t)floorf((pts[3 * i + 2] - org[2]) / voxel);
    const size_t key = ix + nx * iy + nx * ny * iz;
    auto it = slot_of.find(key);
    if (it == slot_of.end()) {
      it = slot_of.emplace(key, (int64_t)cells.size()).first;
      cells.push_back(Cell{0, 0.f, 0.f, 0.f, -1, 0.0});
    }
    Cell& c = cells[(size_t)it->second];
    c.count += 1;
    c.sx += pts[3 * i]; c.sy += pts[3 * i + 1]; c.sz += pts[3 * i + 2];            // float accumulation in input order
    cell_of[(size_t)i] = it->second;
  }
  for (int64_t i = 0; i < n; i++) {                                                  // member closest to the voxel mean, first minimum
    Cell& c = cells[(size_t)cell_of[(size_t)i]];
    const float a = (float)(1.0 / (double)c.count);
    const float dx = pts[3 * i] - c.sx * a, dy = pts[3 * i + 1] - c.sy * a, dz = pts[3 * i + 2] - c.sz * a;
    const double dist = (double)sqrtf(dx * dx + dy * dy + dz * dz);
    if (c.best < 0 || dist < c.best_d) { c.best = i; c.best_d = dist; }
  }
  int64_t o = 0;
  for (const auto& kv : slot_of) {
    const int64_t src = cells[(size_t)kv.second].best;
    for (int d = 0; d < 3; d++) {
      s_pts[3 * o + d] = pts[3 * src + d];
      if (s_nrm) s_nrm[3 * o + d] = nrm[3 * src + d];
    }
    o++;
  }
  return o;
}

}  // namespace
#include "kdtree_ref.h"
namespace {
using se3_kd::Hit;
using se3_kd::KdTree;

// All neighbours of every query of one cloud within `radius`: ascending distance, exactly tied distances in the reference's order.
template <typename Emit>
void radius_search_one(const float* q, int64_t nq, const float* s, int64_t ns, int64_t s_offset, float radius, Emit emit) {
  const float r2 = radius * radius;
  std::vector<Hit> hits;
  if (ns == 0) {
    for (int64_t i = 0; i < nq; i++) emit(i, hits);
    return;
  }
  const KdTree tree(s, ns);
  for (int64_t i = 0; i < nq; i++) {
    hits.clear();
    tree.radius(q + 3 * i, r2, hits);
    std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.d2 < b.d2; });      // (on the distance alone, as the reference)
    for (Hit& h : hits) h.idx += s_offset;
    emit(i, hits);
  }
}

}  // namespace

extern "C" int se3_grid_subsample_host(const float* points, const float* normals, int64_t n, const int64_t* lengths, int batch, float voxel_size,
                                       float* s_points, float* s_normals, int64_t* s_lengths) {
  SE3_REQUIRE(points && lengths && s_points && s_lengths, SE3_ERR_INVALID_ARG, "grid_subsample_host: null pointer");
  SE3_REQUIRE((normals == nullptr) == (s_normals == nullptr), SE3_ERR_INVALID_ARG, "grid_subsample_host: normals in and out must both be given or both NULL");
  SE3_REQUIRE(voxel_size > 0.f && batch >= 1, SE3_ERR_INVALID_ARG, "grid_subsample_host: bad voxel size / batch");
  int64_t start = 0, out = 0;
  for (int b = 0; b < batch; b++) {
    SE3_REQUIRE(lengths[b] >= 0 && start + lengths[b] <= n, SE3_ERR_INVALID_ARG, "grid_subsample_host: lengths exceed the point count");
    const int64_t m = grid_subsample_one(points + 3 * start, normals ? normals + 3 * start : nullptr, lengths[b], voxel_size,
                                         s_points + 3 * out, s_normals ? s_normals + 3 * out : nullptr);
    s_lengths[b] = m;
    out += m;
    start += lengths[b];
  }
  return SE3_OK;
}

// Two calls as for the reference's variable-width result: with out == NULL only *max_count is computed; with out (nq, limit) the rows
// are filled (ascending distance, padded with ns) and *max_count reports the largest in-radius count (may exceed limit).
extern "C" int se3_radius_neighbors_host(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths,
                                         const int64_t* s_lengths, int batch, float radius, int64_t limit, int64_t* out, int64_t* max_count) {
  SE3_REQUIRE(q_points && s_points && q_lengths && s_lengths && max_count, SE3_ERR_INVALID_ARG, "radius_neighbors_host: null pointer");
  SE3_REQUIRE(batch >= 1 && (out == nullptr || limit >= 1), SE3_ERR_INVALID_ARG, "radius_neighbors_host: bad batch / limit");
  int64_t q0 = 0, s0 = 0, mc = 0;
  for (int b = 0; b < batch; b++) {
    SE3_REQUIRE(q0 + q_lengths[b] <= nq && s0 + s_lengths[b] <= ns, SE3_ERR_INVALID_ARG, "radius_neighbors_host: lengths exceed the point counts");
    radius_search_one(q_points + 3 * q0, q_lengths[b], s_points + 3 * s0, s_lengths[b], s0, radius, [&](int64_t i, const std::vector<Hit>& hits) {
      mc = std::max<int64_t>(mc, (int64_t)hits.size());
      if (out) {
        int64_t* row = out + (q0 + i) * limit;
        for (int64_t k = 0; k < limit; k++) row[k] = k < (int64_t)hits.size() ? hits[(size_t)k].idx : ns;
      }
    });
    q0 += q_lengths[b];
    s0 += s_lengths[b];
  }
  *max_count = mc;
  return SE3_OK;
}

// ---- count-only search on host memory (neighbour-limit calibration; the device form: csrc/radius_neighbors.hip) --------------------------
// Per query only the NUMBER of support points with d2 < r^2 is wanted, so no tree and no sort: the finite support points of a cloud are
// binned into cells of edge > radius (counting sort) and a query tests the points of the 3 x 3 x 3 cells around it with the search's float
// arithmetic.  A cell walk only ever skips points further than a cell edge away, so the counts equal the exhaustive scan's.  Points with a
// non-finite coordinate are never within a radius of anything (their d2 is inf or NaN) and are left out of the cells.
#include <stdlib.h>
#include <thread>
namespace {

constexpr int kHostGridCap = 128;                  // cells per axis at most
constexpr int kHostMaxHistBins = 4096;             // as the device entry

struct CountCells {
  double org[3], inv_cell;
  int dim[3];
  std::vector<int> start;                          // (cells + 1) offsets into xyz
  std::vector<float> xyz;                          // the binned points, cell by cell

  CountCells(const float* s, int64_t ns, float radius) {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    int64_t kept = 0;
    auto finite = [&](int64_t i) { return isfinite(s[3 * i]) && isfinite(s[3 * i + 1]) && isfinite(s[3 * i + 2]); };
    for (int64_t i = 0; i < ns; i++) {
      if (!finite(i)) continue;
      for (int d = 0; d < 3; d++) {
        const double v = s[3 * i + d];
        if (kept == 0 || v < lo[d]) lo[d] = v;
        if (kept == 0 || v > hi[d]) hi[d] = v;
      }
      kept++;
    }
    double ext = 0;
    for (int d = 0; d < 3; d++) ext = std::max(ext, hi[d] - lo[d]);
    const double cell = std::max(std::max((double)fabsf(radius), ext / (kHostGridCap - 1)), 1e-20) * 1.0001;
    inv_cell = 1.0 / cell;
    int cells = 1;
    for (int d = 0; d < 3; d++) {
      org[d] = lo[d];
      dim[d] = std::min(kHostGridCap, std::max(1, (int)floor((hi[d] - lo[d]) * inv_cell) + 1));
      cells *= dim[d];
    }
    start.assign((size_t)cells + 1, 0);
    std::vector<int> cell_of((size_t)ns, -1);
    for (int64_t i = 0; i < ns; i++) {
      if (!finite(i)) continue;
      int c[3];
      for (int d = 0; d < 3; d++) c[d] = std::min(dim[d] - 1, std::max(0, (int)floor((s[3 * i + d] - org[d]) * inv_cell)));
      cell_of[(size_t)i] = c[0] + dim[0] * (c[1] + dim[1] * c[2]);
      start[(size_t)cell_of[(size_t)i] + 1]++;
    }
    for (int c = 0; c < cells; c++) start[(size_t)c + 1] += start[(size_t)c];
    std::vector<int> fill(start.begin(), start.end() - 1);
    xyz.resize((size_t)kept * 3);
    for (int64_t i = 0; i < ns; i++) {
      if (cell_of[(size_t)i] < 0) continue;
      const size_t o = (size_t)fill[(size_t)cell_of[(size_t)i]]++;
      for (int d = 0; d < 3; d++) xyz[3 * o + d] = s[3 * i + d];
    }
  }

  int count(const float* q, float r2) const {
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) return 0;
    int c[3];
    for (int d = 0; d < 3; d++) c[d] = (int)std::min((double)dim[d] + 1, std::max(-2.0, floor((q[d] - org[d]) * inv_cell)));
    const int x0 = std::max(c[0] - 1, 0), x1 = std::min(c[0] + 1, dim[0] - 1);
    if (x0 > x1) return 0;
    int n = 0;
    for (int z = std::max(c[2] - 1, 0); z <= std::min(c[2] + 1, dim[2] - 1); z++)
      for (int y = std::max(c[1] - 1, 0); y <= std::min(c[1] + 1, dim[1] - 1); y++) {
        const size_t row = (size_t)dim[0] * ((size_t)y + (size_t)dim[1] * (size_t)z);
        for (int k = start[row + (size_t)x0]; k < start[row + (size_t)x1 + 1]; k++) {
          // unfused float32 (this file is compiled with -ffp-contract=off), the association of the searches
          const float dx = q[0] - xyz[3 * (size_t)k], dy = q[1] - xyz[3 * (size_t)k + 1], dz = q[2] - xyz[3 * (size_t)k + 2];
          const float d2 = (dx * dx + dy * dy) + dz * dz;
          n += d2 < r2 ? 1 : 0;
        }
      }
    return n;
  }
};

int host_threads() {                               // SE3_HOST_THREADS (default 1: DataLoader workers are processes of their own)
  const char* e = getenv("SE3_HOST_THREADS");
  const int n = e ? atoi(e) : 1;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}

}  // namespace

extern "C" int se3_radius_count_hist_host(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths,
                                          const int64_t* s_lengths, int batch, float radius, int hist_n, const int* slot_of_cloud,
                                          int num_slots, int32_t* hist, int32_t* dropped, int32_t* max_count) {
  SE3_REQUIRE(batch >= 1 && batch <= SE3_MAX_BATCH, SE3_ERR_INVALID_ARG, "radius_count_hist_host: batch %d not in [1,%d]", batch, SE3_MAX_BATCH);
  SE3_REQUIRE(hist_n >= 1 && hist_n <= kHostMaxHistBins, SE3_ERR_UNSUPPORTED, "radius_count_hist_host: hist_n %d not in [1,%d]", hist_n,
              kHostMaxHistBins);
  SE3_REQUIRE(q_points && s_points && q_lengths && s_lengths && slot_of_cloud && hist && dropped && max_count, SE3_ERR_INVALID_ARG,
              "radius_count_hist_host: null pointer");
  SE3_REQUIRE(num_slots >= 1, SE3_ERR_INVALID_ARG, "radius_count_hist_host: num_slots %d", num_slots);
  int64_t q0 = 0, s0 = 0;
  for (int b = 0; b < batch; b++) {
    SE3_REQUIRE(slot_of_cloud[b] >= 0 && slot_of_cloud[b] < num_slots, SE3_ERR_INVALID_ARG,
                "radius_count_hist_host: slot %d of cloud %d not in [0,%d)", slot_of_cloud[b], b, num_slots);
    SE3_REQUIRE(q_lengths[b] >= 0 && s_lengths[b] >= 0, SE3_ERR_INVALID_ARG, "radius_count_hist_host: negative length");
    q0 += q_lengths[b];
    s0 += s_lengths[b];
  }
  SE3_REQUIRE(q0 == nq && s0 == ns, SE3_ERR_INVALID_ARG, "radius_count_hist_host: lengths do not sum to the sizes");
  const float r2 = radius * radius;
  const int threads = host_threads();
  q0 = s0 = 0;
  for (int b = 0; b < batch; b++) {
    const int64_t qn = q_lengths[b];
    const CountCells cells(s_points + 3 * s0, s_lengths[b], radius);
    const float* q = q_points + 3 * q0;
    // every thread a contiguous share of the queries and a histogram of its own (hist_n bins, dropped, largest count), added up in order
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(threads, qn / 256));
    std::vector<std::vector<int32_t>> local((size_t)parts, std::vector<int32_t>((size_t)hist_n + 2, 0));
    auto work = [&](int t) {
      std::vector<int32_t>& h = local[(size_t)t];
      for (int64_t i = qn * t / parts; i < qn * (t + 1) / parts; i++) {
        const int c = r2 > 0.f ? cells.count(q + 3 * i, r2) : 0;
        h[(size_t)(c < hist_n ? c : hist_n)]++;
        if (c > h[(size_t)hist_n + 1]) h[(size_t)hist_n + 1] = c;
      }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < parts; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread& t : pool) t.join();
    int32_t* row = hist + (size_t)slot_of_cloud[b] * hist_n;
    for (const std::vector<int32_t>& h : local) {
      for (int i = 0; i < hist_n; i++) row[i] += h[(size_t)i];
      dropped[slot_of_cloud[b]] += h[(size_t)hist_n];
      max_count[b] = std::max(max_count[b], h[(size_t)hist_n + 1]);
    }
    q0 += qn;
    s0 += s_lengths[b];
  }
  return SE3_OK;
}
