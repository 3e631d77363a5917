// The host side of the pair grid under AddressSanitizer and UBSan, as a stand-alone program (tools/pair_grid_host_sanitize.sh builds and
// runs it; no GPU is used and nothing is launched): se3_debug_pair_nearest_neighbor_host, se3_debug_knn_host and
// se3_debug_keypoint_nms_host -- PairHostGrid, pg_single_rows, pg_build_host and the walks of csrc/pair_grid.h -- on a cloud of one
// point, one of 65 and an empty one, each searched in itself, in float32 and float64.  Exit status 0: every call returned SE3_OK, a
// point's nearest neighbour is the point itself, and the sanitizers found nothing.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../include/se3et_hip.h"

template <class Real>
static int run(int64_t n) {
  const int elem = sizeof(Real) == 8;
  std::vector<Real> pts((size_t)(3 * n + 3));          // (never an empty buffer: the entries refuse a null pointer)
  uint64_t state = 88172645463325252ull + (uint64_t)n;
  for (auto& v : pts) {
    state ^= state << 13, state ^= state >> 7, state ^= state << 17;
    v = (Real)((double)(state >> 11) / 9007199254740992.0);
  }
  const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const int k = 33;
  std::vector<double> dist((size_t)n + 1), d2((size_t)(n * k) + 1);
  std::vector<int64_t> idx((size_t)n + 1), knn((size_t)(n * k) + 1), order((size_t)n + 1), kept((size_t)n + 1);
  int bad = 0;
  const auto must = [&](int rc, const char* what) {
    if (rc != SE3_OK) printf("n = %lld, elem %d: %s: %s\n", (long long)n, elem, what, se3_last_error()), bad++;
  };
  must(se3_debug_pair_nearest_neighbor_host(pts.data(), n, pts.data(), n, elem, eye, dist.data(), idx.data()), "nearest neighbour");
  must(se3_debug_knn_host(pts.data(), n, pts.data(), n, elem, k, knn.data(), d2.data()), "k nearest");
  for (int64_t i = 0; i < n; i++) order[(size_t)i] = n - 1 - i;
  int64_t count = -1;
  int status = -1;
  must(se3_debug_keypoint_nms_host(pts.data(), n, elem, order.data(), 0.25, 0, kept.data(), &count, &status), "keypoint NMS");
  for (int64_t i = 0; i < n; i++)
    if (idx[(size_t)i] != i || dist[(size_t)i] != 0.0 || knn[(size_t)(i * k)] != i)
      printf("n = %lld, elem %d: row %lld is not its own neighbour\n", (long long)n, elem, (long long)i), bad++;
  if (status != 0 || count < (n > 0) || count > n)
    printf("n = %lld, elem %d: NMS kept %lld, status %d\n", (long long)n, elem, (long long)count, status), bad++;
  printf("n = %2lld  elem %d  NMS kept %lld\n", (long long)n, elem, (long long)count);
  return bad;
}

int main() {
  int bad = 0;
  for (int64_t n : {1, 65, 0}) bad += run<float>(n) + run<double>(n);
  printf(bad ? "pair_grid_host_sanitize: %d failures\n" : "pair_grid_host_sanitize: ok\n", bad);
  return bad != 0;
}
