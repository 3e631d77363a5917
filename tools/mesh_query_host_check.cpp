// Stand-alone check of the host entries of csrc/mesh_query.hip (se3_debug_mesh_*_host) for a sanitizer build: its own main, no Python, no
// GPU work.  It runs the named cases of tests/mesh_query_fixture.py (rebuilt here in C++) and a seeded triangle soup, every array allocated
// at its exact size on the heap so that AddressSanitizer sees the first byte past each of them, and checks what needs no reference: the
// walk over the tree answers as the brute force does, bit for bit.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/mesh_query_host_check.cpp se3et_amd/csrc/mesh_query.hip se3et_amd/csrc/capi_common.hip -o /tmp/mesh_query_host_check && /tmp/mesh_query_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <utility>
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

uint64_t g_seed = 2013;
double uniform() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

Mesh soup(const char* name, int n, std::vector<int64_t> t) {
  Mesh M;
  M.name = name;
  for (int i = 0; i < 3 * n; i++) M.v.push_back(uniform());
  M.t = std::move(t);
  return M;
}

Mesh cube() {
  Mesh M;
  M.name = "cube";
  for (double x : {0.25, 1.0})
    for (double y : {0.25, 1.0})
      for (double z : {0.25, 1.0}) M.v.insert(M.v.end(), {x, y, z});
  const int quads[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
  for (auto& q : quads) M.t.insert(M.t.end(), {q[0], q[1], q[2], q[0], q[2], q[3]});
  return M;
}

Mesh icosphere(int levels) {
  Mesh M;
  M.name = "icosphere";
  const double g = (1 + sqrt(5.0)) / 2;
  const double p[12][3] = {{-1, g, 0}, {1, g, 0}, {-1, -g, 0}, {1, -g, 0}, {0, -1, g}, {0, 1, g}, {0, -1, -g}, {0, 1, -g}, {g, 0, -1}, {g, 0, 1}, {-g, 0, -1}, {-g, 0, 1}};
  std::vector<double> v;
  for (auto& q : p) {
    const double r = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    v.insert(v.end(), {q[0] / r, q[1] / r, q[2] / r});
  }
  std::vector<int64_t> t = {0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                            3, 9,  4, 3, 4, 2, 3, 2, 6, 3, 6, 8,  3, 8,  9,  4, 9, 5, 2, 4,  11, 6, 2,  10, 8, 6,  7, 9, 8, 1};
  for (int l = 0; l < levels; l++) {
    std::map<std::pair<int64_t, int64_t>, int64_t> mid;
    auto middle = [&](int64_t a, int64_t b) {
      const auto key = std::make_pair(std::min(a, b), std::max(a, b));
      auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      double q[3], r = 0;
      for (int k = 0; k < 3; k++) q[k] = v[3 * a + k] + v[3 * b + k], r += q[k] * q[k];
      r = sqrt(r);
      v.insert(v.end(), {q[0] / r, q[1] / r, q[2] / r});
      return mid[key] = (int64_t)v.size() / 3 - 1;
    };
    std::vector<int64_t> out;
    for (size_t i = 0; i < t.size(); i += 3) {
      const int64_t a = t[i], b = t[i + 1], c = t[i + 2], ab = middle(a, b), bc = middle(b, c), ca = middle(c, a);
      out.insert(out.end(), {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca});
    }
    t = out;
  }
  const double scale[3] = {1.0, 0.7, 1.3}, move[3] = {3.1, -2.2, 0.4};
  for (size_t i = 0; i < v.size(); i++) M.v.push_back(v[i] * scale[i % 3] + move[i % 3]);
  M.t = t;
  return M;
}

Mesh chain() {
  Mesh M;
  M.name = "chain";
  const double cell = ldexp(1.0, -21), d = 1e-9;
  std::vector<std::vector<double>> centres;
  for (int i = 0; i < 8; i++) centres.push_back({(0.05 + 0.1 * (i & 1)) * cell, (0.05 + 0.1 * (i >> 1 & 1)) * cell, (0.05 + 0.1 * (i >> 2 & 1)) * cell});
  for (int axis = 0; axis < 3; axis++) {
    for (int j = 0; j <= 21; j++) {
      std::vector<double> c(3, 0.5 * cell);
      c[axis] = j < 21 ? (ldexp(1.0, j) + 0.5) * cell : 1.0;
      centres.push_back(c);
    }
  }
  const double off[3][3] = {{d, 0, 0}, {0, d, 0}, {-d, -d, 0.5 * d}};
  for (auto& c : centres)
    for (auto& o : off) {
      for (int k = 0; k < 3; k++) M.v.push_back(c[k] + o[k]);
      M.t.push_back((int64_t)M.t.size());
    }
  return M;
}

template <class T>
struct Exact {                 // an array at its exact size on the heap (a size of zero still has an address)
  T* p;
  size_t count;
  explicit Exact(size_t n, int fill = 0x5a) : p((T*)malloc(n ? n * sizeof(T) : 1)), count(n) { memset(p, fill, n * sizeof(T)); }
  Exact(const std::vector<T>& x) : Exact(x.size()) {
    if (!x.empty()) memcpy(p, x.data(), x.size() * sizeof(T));
  }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
  bool same(const Exact& o) const { return count == o.count && (count == 0 || memcmp(p, o.p, count * sizeof(T)) == 0); }
};

int g_failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                 \
      g_failures++;                 \
    }                               \
  } while (0)
#define OK(call) CHECK((call) == SE3_OK, "%s: %s: %s", M.name.c_str(), #call, se3_last_error())

void run(const Mesh& M) {
  const int64_t n = M.n(), m = M.m();
  Exact<double> v(M.v);
  Exact<int64_t> t(M.t), keys((size_t)m), counts(4);
  OK(se3_debug_mesh_bvh_host(SE3_MESH_BVH_KEYS, v.p, t.p, n, m, keys.p, nullptr, nullptr, nullptr, counts.p));
  std::vector<int64_t> order((size_t)m);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    const bool ia = keys.p[a] < 0, ib = keys.p[b] < 0;
    return ia != ib ? ib : keys.p[a] < keys.p[b];
  });
  std::vector<int64_t> sorted;
  for (int64_t o : order) sorted.push_back(keys.p[o]);
  Exact<int64_t> ord(order), skeys(sorted);
  Exact<char> nodes((size_t)(2 * (m > 0 ? m : 1)) * SE3_MESH_QUERY_NODE_BYTES);
  OK(se3_debug_mesh_bvh_host(SE3_MESH_BVH_TREE, v.p, t.p, n, m, nullptr, skeys.p, ord.p, nodes.p, counts.p));
  const int64_t root = counts.p[3];

  // rays and query points: towards and around the mesh, far away, degenerate
  double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
  for (int64_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++)
      if (isfinite(M.v[3 * i + k])) lo[k] = i ? fmin(lo[k], M.v[3 * i + k]) : M.v[3 * i + k], hi[k] = i ? fmax(hi[k], M.v[3 * i + k]) : M.v[3 * i + k];
  std::vector<double> rays, queries;
  for (int r = 0; r < 400; r++) {
    double o[3], p[3];
    const double reach = r % 7 == 0 ? 1e6 : (r % 3 == 0 ? 0.2 : 2.0);
    for (int k = 0; k < 3; k++) {
      const double c = (lo[k] + hi[k]) / 2, e = hi[k] - lo[k] + 1e-3;
      o[k] = c + reach * e * uniform();
      p[k] = m && r % 2 ? M.v[3 * ((M.t[(size_t)(3 * (r % m))] % (n ? n : 1) + n) % (n ? n : 1)) + k] : c + 0.5 * e * uniform();
    }
    const double len = r % 11 == 0 ? 1e-30 : (r % 13 == 0 ? 1e30 : 1.0);
    rays.insert(rays.end(), {o[0], o[1], o[2], (p[0] - o[0]) * len, (p[1] - o[1]) * len, (p[2] - o[2]) * len});
    queries.insert(queries.end(), {r % 5 == 0 ? p[0] : o[0], r % 5 == 0 ? p[1] : o[1], r % 5 == 0 ? p[2] : o[2]});
  }
  rays.insert(rays.end(), {0, 0, 0, 0, 0, 0, 0, 0, 0, NAN, 1, 0, INFINITY, 0, 0, 1, 0, 0});
  queries.insert(queries.end(), {NAN, 0, 0});
  const int64_t R = (int64_t)rays.size() / 6, Q = (int64_t)queries.size() / 3;
  Exact<double> ry(rays), qs(queries);
  for (int pass = 0; pass < 2; pass++) {                                   // everything, then the any-hit flags
    Exact<double> bt((size_t)R), bu((size_t)2 * R), bn((size_t)3 * R), wt((size_t)R), wu((size_t)2 * R), wn((size_t)3 * R);
    Exact<int64_t> bi((size_t)R), wi((size_t)R);
    Exact<uint8_t> bh((size_t)R), wh((size_t)R);
    if (pass == 0) {
      OK(se3_debug_mesh_cast_rays_host(v.p, t.p, n, m, ry.p, R, 0.0, INFINITY, 0, bt.p, bi.p, bu.p, bn.p, nullptr));
      OK(se3_debug_mesh_walk_rays_host(v.p, t.p, n, m, nodes.p, root, ry.p, R, 0.0, INFINITY, 0, wt.p, wi.p, wu.p, wn.p, nullptr));
      CHECK(bt.same(wt) && bi.same(wi) && bu.same(wu) && bn.same(wn), "%s: the walk and the brute force cast differently", M.name.c_str());
      int64_t hits = 0;
      for (int64_t r = 0; r < R; r++) hits += bi.p[r] >= 0;
      printf("%-16s n %6lld m %6lld live %6lld flat %3lld status %lld root %6lld  rays hit %lld of %lld\n", M.name.c_str(), (long long)n, (long long)m,
             (long long)counts.p[1], (long long)counts.p[2], (long long)counts.p[0], (long long)root, (long long)hits, (long long)R);
    } else {
      OK(se3_debug_mesh_cast_rays_host(v.p, t.p, n, m, ry.p, R, 0.0, INFINITY, 1, nullptr, nullptr, nullptr, nullptr, bh.p));
      OK(se3_debug_mesh_walk_rays_host(v.p, t.p, n, m, nodes.p, root, ry.p, R, 0.0, INFINITY, 1, nullptr, nullptr, nullptr, nullptr, wh.p));
      CHECK(bh.same(wh), "%s: the any-hit flags differ", M.name.c_str());
    }
  }
  Exact<double> bp((size_t)3 * Q), bd((size_t)Q), bu((size_t)2 * Q), bn((size_t)3 * Q), wp((size_t)3 * Q), wd((size_t)Q), wu((size_t)2 * Q), wn((size_t)3 * Q);
  Exact<int64_t> bi((size_t)Q), wi((size_t)Q);
  OK(se3_debug_mesh_closest_points_host(v.p, t.p, n, m, qs.p, Q, bp.p, bd.p, bi.p, bu.p, bn.p));
  OK(se3_debug_mesh_walk_points_host(v.p, t.p, n, m, nodes.p, root, qs.p, Q, wp.p, wd.p, wi.p, wu.p, wn.p));
  CHECK(bp.same(wp) && bd.same(wd) && bi.same(wi) && bu.same(wu) && bn.same(wn), "%s: the walk and the brute force find different closest points", M.name.c_str());

  const int H = 9, W = 11;
  const double c[3] = {(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2};
  std::vector<double> view = {1, 0, 0, c[0], 0, 1, 0, c[1], 0, 0, 1, c[2] - 2.0 * (hi[2] - lo[2] + 1e-3), 8.0, 8.0, 5.2, 4.1};
  Exact<double> vw(view), points((size_t)3 * H * W), normals((size_t)3 * H * W);
  Exact<float> depth((size_t)H * W);
  Exact<int64_t> ids((size_t)H * W);
  Exact<uint8_t> mask((size_t)H * W);
  OK(se3_debug_mesh_render_host(v.p, t.p, n, m, vw.p, 1, H, W, 1e-3, 1e3, depth.p, points.p, normals.p, ids.p, mask.p));
  for (int i = 0; i < H * W; i++) CHECK(mask.p[i] <= 1 && (mask.p[i] == 1) == (ids.p[i] >= 0) && ids.p[i] < (m > 0 ? m : 1), "%s: pixel %d", M.name.c_str(), i);
}

}  // namespace

int main() {
  std::vector<Mesh> meshes;
  meshes.push_back(soup("one", 3, {0, 1, 2}));
  meshes.push_back(soup("edge_pair", 4, {1, 3, 2, 0, 1, 2}));
  {
    Mesh fan = soup("fan_100", 101, {});
    for (int i = 0; i < 100; i++) {
      fan.v[3 * (i + 1)] = cos(i * 0.0628318530718), fan.v[3 * (i + 1) + 1] = sin(i * 0.0628318530718), fan.v[3 * (i + 1) + 2] = 0.1 * cos((double)i);
      fan.t.insert(fan.t.end(), {0, 1 + i, 1 + (i + 1) % 100});
    }
    meshes.push_back(fan);
  }
  meshes.push_back(cube());
  meshes.push_back(icosphere(2));
  meshes.push_back(chain());
  {
    Mesh same = soup("coincident_200", 3, {});
    for (int i = 0; i < 200; i++) same.t.insert(same.t.end(), {0, 1, 2});
    meshes.push_back(same);
  }
  meshes.push_back(soup("bad_triangle", 6, {0, 1, 2, 1, 2, 6, 3, 4, 5, 2, -1, 3}));
  {
    Mesh bad = soup("nan_vertex", 6, {0, 1, 2, 3, 4, 5, 2, 3, 5});
    bad.v[3 * 4 + 1] = NAN;
    meshes.push_back(bad);
  }
  {
    Mesh flat = soup("zero_area", 5, {0, 1, 2, 0, 1, 4, 3, 3, 1, 1, 2, 3});
    for (int k = 0; k < 3; k++) flat.v[3 * 4 + k] = flat.v[k] + 2 * (flat.v[3 + k] - flat.v[k]);
    meshes.push_back(flat);
  }
  meshes.push_back(soup("no_triangles", 6, {}));
  meshes.push_back(soup("nothing", 0, {}));
  {
    Mesh big = soup("soup_500", 300, {});
    for (int i = 0; i < 1500; i++) big.t.push_back((int64_t)((uniform() + 1.0) * 150.0) % 300);
    meshes.push_back(big);
  }
  for (const Mesh& M : meshes) run(M);
  printf(g_failures ? "%d check(s) FAILED\n" : "every check passed\n", g_failures);
  return g_failures ? 1 : 0;
}
