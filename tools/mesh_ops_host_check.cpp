// Stand-alone check of the host entries of csrc/mesh_ops.hip (se3_debug_mesh_*_host) for a sanitizer build: its own main, no Python, no GPU
// work.  It runs the named cases of tests/mesh_ops_fixture.py (rebuilt here in C++), every array allocated at its exact size on the heap
// so that AddressSanitizer sees the first byte past each of them, and checks the invariants that need no reference.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/mesh_ops_host_check.cpp se3et_amd/csrc/mesh_ops.hip se3et_amd/csrc/capi_common.hip -o /tmp/mesh_ops_host_check && /tmp/mesh_ops_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../include/se3et_hip.h"

namespace {

struct Mesh {
  std::string name;
  std::vector<double> v;       // n x 3
  std::vector<int64_t> t;      // m x 3
  int64_t n() const { return (int64_t)v.size() / 3; }
  int64_t m() const { return (int64_t)t.size() / 3; }
};

uint64_t g_seed = 12345;
double uniform() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

Mesh mesh(const char* name, int n, std::vector<int64_t> t) {
  Mesh M;
  M.name = name;
  for (int i = 0; i < 3 * n; i++) M.v.push_back(uniform());
  M.t = t;
  return M;
}

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      fprintf(stderr, "%s: %s fails (%s)\n", M.name.c_str(), #cond, se3_last_error()); \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

// exact-size heap arrays: one byte past any of them is a sanitizer report
template <class T>
T* fresh(int64_t count) { return (T*)malloc(sizeof(T) * (size_t)(count > 0 ? count : 0) + (count > 0 ? 0 : 1)); }

void run(const Mesh& M, int expect_status, int expect_clusters) {
  const int64_t n = M.n(), m = M.m();
  int64_t counts[4];
  int64_t* toff = fresh<int64_t>(n + 1);
  int64_t* noff = fresh<int64_t>(n + 1);
  int* trows = fresh<int>(3 * m);
  CHECK(se3_debug_mesh_incidence_host(M.t.data(), n, m, toff, trows, noff, 0, nullptr, counts) == 0);
  CHECK(counts[0] == expect_status && counts[1] <= 3 * m && toff[n] == counts[1] && noff[n] == counts[2]);
  int* nrows = fresh<int>(counts[2]);
  CHECK(se3_debug_mesh_incidence_host(M.t.data(), n, m, toff, trows, noff, counts[2], nrows, counts) == 0);
  for (int64_t i = 0; i < n; i++) {
    for (int64_t k = toff[i] + 1; k < toff[i + 1]; k++) CHECK(trows[k - 1] < trows[k]);
    for (int64_t k = noff[i]; k < noff[i + 1]; k++) CHECK(nrows[k] >= 0 && nrows[k] < n && nrows[k] != i && (k == noff[i] || nrows[k - 1] < nrows[k]));
  }

  int64_t* labels = fresh<int64_t>(m);
  int64_t* sizes = fresh<int64_t>(m);
  double* area = fresh<double>(m);
  CHECK(se3_debug_mesh_components_host(M.v.data(), M.t.data(), n, m, toff, trows, labels, sizes, area, counts) == 0);
  CHECK(counts[0] == expect_status && (expect_clusters < 0 || counts[1] == expect_clusters));
  const int64_t clusters = counts[1];
  int64_t members = 0;
  for (int64_t c = 0; c < counts[1]; c++) {
    members += sizes[c];
    CHECK(sizes[c] > 0 && area[c] >= 0.0);
  }
  CHECK(members == m);
  for (int64_t t = 0; t < m; t++) CHECK(labels[t] >= 0 && labels[t] < counts[1] && (t > 0 || labels[t] == 0));

  double* tn = fresh<double>(3 * m);
  double* vn = fresh<double>(3 * n);
  CHECK(se3_debug_mesh_normals_host(M.v.data(), M.t.data(), n, m, toff, trows, 1, tn, vn) == 0);
  for (int64_t i = 0; i < n; i++) CHECK(fabs(sqrt(vn[3 * i] * vn[3 * i] + vn[3 * i + 1] * vn[3 * i + 1] + vn[3 * i + 2] * vn[3 * i + 2]) - 1.0) < 1e-14);

  uint8_t* keep = fresh<uint8_t>(m);
  for (int pass = 0; pass < 3; pass++) {                                  // every second triangle, all, none
    for (int64_t t = 0; t < m; t++) keep[t] = pass == 0 ? (uint8_t)(t % 2) : (uint8_t)(pass == 1);
    int64_t* vmap = fresh<int64_t>(n);
    CHECK(se3_debug_mesh_select_host(M.v.data(), M.v.data(), nullptr, M.t.data(), keep, n, m, 0, 0, nullptr, nullptr, nullptr, nullptr, vmap, counts) == 0);
    const int64_t nv = counts[1], nt = counts[2];
    double* ov = fresh<double>(3 * nv);
    double* on = fresh<double>(3 * nv);
    int64_t* ot = fresh<int64_t>(3 * nt);
    CHECK(se3_debug_mesh_select_host(M.v.data(), M.v.data(), nullptr, M.t.data(), keep, n, m, nv, nt, ov, on, nullptr, ot, vmap, counts) == 0);
    CHECK(counts[1] == nv && counts[2] == nt && (pass != 2 || (nv == 0 && nt == 0)));
    for (int64_t k = 0; k < 3 * nt; k++) CHECK(ot[k] >= 0 && ot[k] < nv);
    free(vmap), free(ov), free(on), free(ot);
  }

  for (int pass = 0; pass < 3; pass++) {                                  // vertex clustering: cells larger than the mesh, middling, tiny
    const double voxel_size = pass == 0 ? 10.0 : (pass == 1 ? 0.37 : 1e-3);
    int64_t* vmap = fresh<int64_t>(n);
    CHECK(se3_debug_mesh_cluster_vertices_host(M.v.data(), M.v.data(), nullptr, M.t.data(), n, m, voxel_size, 0, 0, nullptr, nullptr, nullptr, nullptr, vmap,
                                               counts) == 0);
    const int64_t nv = counts[1], nt = counts[2];
    CHECK((counts[0] & ~(int64_t)SE3_MESH_OPS_BAD_TRIANGLE) == 0 && nv <= n && nt <= m && (n == 0 || nv >= 1) && (pass != 0 || (nv <= 1 && nt == 0)));
    double* ov = fresh<double>(3 * nv);
    double* on = fresh<double>(3 * nv);
    int64_t* ot = fresh<int64_t>(3 * nt);
    CHECK(se3_debug_mesh_cluster_vertices_host(M.v.data(), M.v.data(), nullptr, M.t.data(), n, m, voxel_size, nv, nt, ov, on, nullptr, ot, vmap, counts) == 0);
    CHECK(counts[1] == nv && counts[2] == nt);
    for (int64_t i = 0; i < n; i++) CHECK(vmap[i] >= 0 && vmap[i] < nv);
    for (int64_t k = 0; k < nt; k++) CHECK(ot[3 * k] >= 0 && ot[3 * k] < ot[3 * k + 1] && ot[3 * k] < ot[3 * k + 2] && ot[3 * k + 1] < nv && ot[3 * k + 2] < nv);
    for (int64_t k = 0; k < 3 * nv; k++) CHECK(isfinite(ov[k]) && ov[k] == on[k]);
    free(vmap), free(ov), free(on), free(ot);
  }

  double* out = fresh<double>(3 * n);
  for (int method = SE3_MESH_SMOOTH_SIMPLE; method <= SE3_MESH_SMOOTH_TAUBIN; method++)
    for (int iterations = 0; iterations < 4; iterations += 3) {
      CHECK(se3_debug_mesh_smooth_host(M.v.data(), n, noff, nrows, method, iterations, 0.5, -0.53, out) == 0);
      for (int64_t i = 0; i < 3 * n; i++) CHECK(isfinite(out[i]) && (iterations > 0 || out[i] == M.v[(size_t)i]));
    }
  free(toff), free(noff), free(trows), free(nrows), free(labels), free(sizes), free(area), free(tn), free(vn), free(keep), free(out);
  printf("%-22s %6lld vertices %6lld triangles: status %d, %lld clusters ok\n", M.name.c_str(), (long long)n, (long long)m, expect_status, (long long)clusters);
}

}  // namespace

int main() {
  std::vector<int64_t> tets = {0, 1, 2, 0, 3, 1, 1, 3, 2, 2, 3, 0, 3, 4, 5, 3, 6, 4, 4, 6, 5, 5, 6, 3};
  run(mesh("two_tets_one_vertex", 7, tets), 0, 2);
  run(mesh("edge_pair_same", 4, {0, 1, 2, 1, 0, 3}), 0, 1);
  run(mesh("edge_pair_opposite", 4, {0, 1, 2, 0, 1, 3}), 0, 1);
  run(mesh("three_on_edge", 5, {0, 1, 2, 0, 1, 3, 1, 0, 4}), 0, 1);
  run(mesh("duplicate_triangle", 4, {0, 1, 2, 1, 2, 3, 0, 1, 2}), 0, 1);
  run(mesh("degenerate", 4, {0, 0, 1, 0, 1, 2, 3, 3, 3}), 0, 2);
  run(mesh("interleaved", 9, {0, 1, 2, 3, 4, 5, 2, 1, 6, 5, 4, 7, 6, 1, 8}), 0, 2);
  run(mesh("no_triangles", 5, {}), 0, 0);
  run(mesh("nothing", 0, {}), 0, 0);
  run(mesh("isolated_vertex", 5, {0, 1, 2, 2, 1, 3}), 0, 1);
  run(mesh("one_neighbor", 2, {0, 0, 1}), 0, 1);
  run(mesh("bad_n", 4, {0, 1, 2, 1, 2, 4, 2, 1, 3}), SE3_MESH_OPS_BAD_TRIANGLE, 2);
  run(mesh("bad_minus_one", 4, {0, 1, 2, -1, 2, 3, 2, 1, 3}), SE3_MESH_OPS_BAD_TRIANGLE, 2);
  run(mesh("bad_far", 4, {0, 1, 2, 1, 2, (int64_t)1 << 40, INT64_MIN, 1, 3}), SE3_MESH_OPS_BAD_TRIANGLE, 3);
  std::vector<int64_t> fan;
  for (int i = 0; i < 100; i++) fan.insert(fan.end(), {0, 1 + i, 1 + (i + 1) % 100});
  run(mesh("fan_100", 101, fan), 0, 1);
  std::vector<int64_t> strip(3 * 4096);
  std::vector<int> order(4096);
  for (int i = 0; i < 4096; i++) order[i] = i;
  for (int i = 4095; i > 0; i--) {                                        // a fixed shuffle
    const int j = (int)((uniform() * 0.5 + 0.5) * (i + 1)) % (i + 1);
    const int x = order[i];
    order[i] = order[j], order[j] = x;
  }
  for (int k = 0; k < 4096; k++) {
    const int i = order[k];
    strip[3 * k] = i % 2 ? i + 1 : i, strip[3 * k + 1] = i % 2 ? i : i + 1, strip[3 * k + 2] = i + 2;
  }
  run(mesh("strip_4096", 4098, strip), 0, 1);
  std::vector<int64_t> grid;
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 8; j++) {
      const int64_t a = i * 9 + j, b = (i + 1) * 9 + j, c = (i + 1) * 9 + j + 1, d = i * 9 + j + 1;
      grid.insert(grid.end(), {a, b, c, a, c, d});
    }
  run(mesh("grid", 81, grid), 0, 1);
  printf("mesh_ops_host_check: all cases ok\n");
  return 0;
}
