// Multiway registration of csrc/pose_graph.hip as __host__ __device__ text: the information matrix of one pair (pgo_information), the
// arc tangent of the edge residual (pgo_atan2), and one pose graph's whole optimisation (pgo_graph_optimize: refusals, pass 1, pruning,
// pass 2, the reference node).  The kernels run it with one workgroup of kPgoLanes threads per pair / graph (each thread one lane,
// `barrier` = __syncthreads); the se3_debug_*_host entries run the same text serially over all lanes with a no-op barrier.  Nothing is
// kept in a lane's registers across a barrier except values that every lane computes alike: all other state lives in the workspace or in
// `sh`.  The ordered sum, the composition, the update matrix and the maximum are those of icp_core.h and fgr_core.h.  The contract is the
// header comment of pose_graph.hip.
#pragma once
#include "fgr_core.h"

#define PGO_HD __host__ __device__ inline

constexpr int kPgoLanes = kIcpLanes;                  // the lanes of icp_sum: 256
constexpr int kPgoMaxDim = 6 * SE3_PGO_MAX_NODES;     // 384 unknowns at the node limit
constexpr int kPgoShSums = 2 * kPgoLanes;             // sh: two sum columns, the Cholesky panel (one row of L), the solve's vector
constexpr int kPgoShDoubles = kPgoShSums + 2 * kPgoMaxDim;
constexpr double kPgoMaxAngle = SE3_PGO_MAX_ANGLE;

struct PgoOptions {
  int max_iteration, max_iteration_lm;
  double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual, upper_scale_factor, lower_scale_factor;
  double max_correspondence_distance, edge_prune_threshold, preference_loop_closure;
};

// ---- the arc tangent ---------------------------------------------------------------------------------------------------------------------
// atan(u) for |u| <= tan(pi / 8): u + (u z) q(z), z = u u, q the Taylor coefficients (-1)^k / (2 k + 1), k = 1 .. 20, by Horner's rule,
// every operation rounded on its own.  The first term left out is z^21 / 43 <= 0.1716^21 / 43 < 2e-18 of u.
PG_HD double pgo_atan_series(double u) {
#pragma clang fp contract(off)
  const double z = u * u;
  double q = 1.0 / 41.0;
  for (int k = 19; k >= 1; k--) {
    const double c = 1.0 / (double)(2 * k + 1);
    const double qz = q * z;
    q = (k & 1) ? qz - c : qz + c;
  }
  const double uz = u * z;
  const double tail = uz * q;
  return u + tail;
}

// atan2(y, x) for finite arguments, in (-pi, pi].  t = min(|x|, |y|) / max(|x|, |y|) in [0, 1] (the swap); t > tan(pi / 8) is reduced once
// more, atan t = pi / 4 + atan((t - 1) / (t + 1)); then the series; then the swaps are undone: pi / 2 - r where |y| > |x|, pi - r where
// x < 0, the sign of y last.  The three constants are added as a high and a low part.  Exact cases: x = y = 0 (any signs) gives a zero;
// y = +-0 gives +-0 for x > 0 and +-pi for x < 0; x = +-0 gives +-pi / 2.  A non-finite argument gives a NaN or some angle: the callers
// have refused it before.
PG_HD double pgo_atan2(double y, double x) {
#pragma clang fp contract(off)
  const double kTanPi8 = 0.41421356237309503;
  const double kPi4Hi = 0.78539816339744828, kPi4Lo = 3.061616997868383e-17;
  const double kPi2Hi = 1.5707963267948966, kPi2Lo = 6.123233995736766e-17;
  const double kPiHi = 3.1415926535897931, kPiLo = 1.2246467991473532e-16;
  const double ax = fabs(x), ay = fabs(y);
  const bool swap = ay > ax;
  const double mn = swap ? ax : ay, mx = swap ? ay : ax;
  double r = 0.0;
  if (mx > 0.0) {
    const double t = mn / mx;
    if (t > kTanPi8) {
      const double num = t - 1.0, den = t + 1.0;
      const double a = pgo_atan_series(num / den);
      const double lo = a + kPi4Lo;
      r = kPi4Hi + lo;
    } else {
      r = pgo_atan_series(t);
    }
  }
  if (swap) {
    const double d = kPi2Hi - r;
    r = d + kPi2Lo;
  }
  if (x < 0.0) {
    const double d = kPiHi - r;
    r = d + kPiLo;
  }
  return copysign(r, y);
}

// ---- rigid 4x4 algebra ---------------------------------------------------------------------------------------------------------------------
// the inverse of a rigid 4x4 in closed form: (R^T, -R^T t), the translation as -((a + b) + c)
PG_HD void pgo_inverse(const double* X, double* out) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) out[4 * i + j] = X[4 * j + i];
    const double a = X[i] * X[3], b = X[4 + i] * X[7], c = X[8 + i] * X[11];
    const double s = (a + b) + c;
    out[4 * i + 3] = -s;
  }
  out[12] = 0.0, out[13] = 0.0, out[14] = 0.0, out[15] = 1.0;
}

// vec6 of a rigid 4x4: the Euler angles of R = Rz(gamma) Ry(beta) Rx(alpha), then the translation
PG_HD void pgo_vec6(const double* M, double* e) {
#pragma clang fp contract(off)
  const double a = M[0] * M[0], b = M[4] * M[4];
  const double sy = pg_sqrt(a + b);
  if (!(sy < 1e-6)) {
    e[0] = pgo_atan2(M[9], M[10]), e[1] = pgo_atan2(-M[8], sy), e[2] = pgo_atan2(M[4], M[0]);
  } else {
    e[0] = pgo_atan2(-M[6], M[5]), e[1] = pgo_atan2(-M[8], sy), e[2] = 0.0;
  }
  e[3] = M[3], e[4] = M[7], e[5] = M[11];
}

// A = T^-1 Xt^-1 of an edge
PG_HD void pgo_edge_left(const double* T, const double* Xt, double* A) {
  double Ti[16], Xi[16];
  pgo_inverse(T, Ti), pgo_inverse(Xt, Xi);
  icp_compose(Ti, Xi, A);
}

// the residual e = vec6(T^-1 Xt^-1 Xs) of an edge and its e^T L e = sum_a e_a (sum_b L_ab e_b)
PG_HD double pgo_edge_residual(const double* Xs, const double* Xt, const double* T, const double* info, double* e) {
#pragma clang fp contract(off)
  double A[16], M[16];
  pgo_edge_left(T, Xt, A);
  icp_compose(A, Xs, M);
  pgo_vec6(M, e);
  double q = 0.0;
  for (int a = 0; a < 6; a++) {
    double s = 0.0;
    for (int b = 0; b < 6; b++) {
      const double m = info[6 * a + b] * e[b];
      s = s + m;
    }
    const double m = e[a] * s;
    q = q + m;
  }
  return q;
}

// W = l (Js^T (L Js)) (6x6, row-major) and g = l (Js^T (L e)) of an edge; column i of Js is lin6(A (D_i Xs)).  Jt = -Js, so the edge adds W
// to both diagonal blocks, -W to the two others, g to the source's part of b and -g to the target's: a negation is exact.
PG_HD void pgo_edge_system(const double* Xs, const double* Xt, const double* T, const double* info, const double* e, double l, double* W,
                           double* g) {
#pragma clang fp contract(off)
  double A[16], J[6][6];
  pgo_edge_left(T, Xt, A);
  for (int i = 0; i < 6; i++) {
    double B[3][4];                                          // the first three rows of D_i Xs (its last row is zero)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) B[r][c] = 0.0;
    if (i < 3) {
      const int r1 = (i + 1) % 3, r2 = (i + 2) % 3;          // D_i has [r1][r2] = -1 and [r2][r1] = 1
      for (int c = 0; c < 4; c++) B[r1][c] = -Xs[4 * r2 + c], B[r2][c] = Xs[4 * r1 + c];
    } else {
      B[i - 3][3] = 1.0;                                     // row 3 of Xs is 0 0 0 1
    }
    double M[3][4];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) {
        const double x = A[4 * r] * B[0][c], y = A[4 * r + 1] * B[1][c], z = A[4 * r + 2] * B[2][c];
        M[r][c] = (x + y) + z;
      }
    J[0][i] = (M[2][1] - M[1][2]) / 2.0, J[1][i] = (M[0][2] - M[2][0]) / 2.0, J[2][i] = (M[1][0] - M[0][1]) / 2.0;
    J[3][i] = M[0][3], J[4][i] = M[1][3], J[5][i] = M[2][3];
  }
  double LJ[6][6], Le[6];
  for (int a = 0; a < 6; a++) {
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int b = 0; b < 6; b++) {
        const double m = info[6 * a + b] * J[b][j];
        s = s + m;
      }
      LJ[a][j] = s;
    }
    double s = 0.0;
    for (int b = 0; b < 6; b++) {
      const double m = info[6 * a + b] * e[b];
      s = s + m;
    }
    Le[a] = s;
  }
  for (int i = 0; i < 6; i++) {
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int a = 0; a < 6; a++) {
        const double m = J[a][i] * LJ[a][j];
        s = s + m;
      }
      W[6 * i + j] = l * s;
    }
    double s = 0.0;
    for (int a = 0; a < 6; a++) {
      const double m = J[a][i] * Le[a];
      s = s + m;
    }
    g[i] = l * s;
  }
}

// ---- one graph ---------------------------------------------------------------------------------------------------------------------------
// every pointer already points at the graph's first entry
struct PgoGraph {
  int N, E, reference_node;
  const double* X0;          // (N, 4, 4)
  const int64_t* edges;      // (E, 2): (source node, target node)
  const double* T;           // (E, 4, 4)
  const double* info;        // (E, 6, 6)
  const uint8_t* uncertain;  // (E)
  double* X;                 // (N, 4, 4): the result
  double* conf1;             // (E)
  double* conf2;             // (E)
  uint8_t* kept;             // (E)
  int* status;
  int* out_info;             // 6
  double* residuals;         // 2
  // scratch, laid out by pgo_scratch
  double *H, *L, *b, *delta, *y, *Xa, *Xb, *ea, *eb, *qa, *qb, *l, *W, *g;
  int *list, *adj_off, *adj;
  double* trace;             // host alone: (trace_rows, 4) or null
  int64_t trace_rows;
  int* trace_count;          // 2
};

// the scratch of a graph of N nodes and E edges from `base` (256-byte aligned); returns the bytes it takes (base may be null)
PGO_HD size_t pgo_scratch(int N, int E, char* base, PgoGraph* v) {
  const size_t n6 = 6 * (size_t)N, e = (size_t)(E > 0 ? E : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  double* H = (double*)take(8 * n6 * n6);
  double* L = (double*)take(8 * n6 * n6);
  double* vec = (double*)take(8 * 3 * n6);
  double* X = (double*)take(8 * 32 * (size_t)N);
  double* ed = (double*)take(8 * (12 + 3 + 36 + 6) * e);
  int* ints = (int*)take(4 * (e + (size_t)N + 2 + 4 * e));
  if (v) {
    v->H = H, v->L = L, v->b = vec, v->delta = vec + n6, v->y = vec + 2 * n6, v->Xa = X, v->Xb = X + 16 * (size_t)N;
    v->ea = ed, v->eb = ed + 6 * e, v->qa = ed + 12 * e, v->qb = ed + 13 * e, v->l = ed + 14 * e, v->W = ed + 15 * e, v->g = ed + 51 * e;
    v->list = ints, v->adj_off = ints + e, v->adj = ints + e + N + 2;
  }
  return off;
}

// the state of a pass that moves between its two buffers (uniform over the lanes)
struct PgoState {
  double *X, *Xn, *e, *en, *q, *qn;
};

// e and e^T L e of the pass's edges (list[0 .. En)) under the poses X
template <class Barrier>
PGO_HD void pgo_residuals(const PgoGraph& v, int En, const double* X, double* e, double* q, int lane_begin, int lane_end, Barrier&& barrier) {
  for (int l = lane_begin; l < lane_end; l++)
    for (int k = l; k < En; k += kPgoLanes) {
      const int64_t o = v.list[k];
      q[k] = pgo_edge_residual(X + 16 * v.edges[2 * o], X + 16 * v.edges[2 * o + 1], v.T + 16 * o, v.info + 36 * o, e + 6 * k);
    }
  barrier();
}

// the line process: l = 1 for a certain edge, (mu / (mu + e^T L e))^2 for an uncertain one
template <class Barrier>
PGO_HD void pgo_line_process(const PgoGraph& v, int En, const double* q, double mu, int lane_begin, int lane_end, Barrier&& barrier) {
#pragma clang fp contract(off)
  for (int l = lane_begin; l < lane_end; l++)
    for (int k = l; k < En; k += kPgoLanes) {
      double w = 1.0;
      if (v.uncertain[v.list[k]]) {
        const double den = mu + q[k];
        const double t = mu / den;
        w = t * t;
      }
      v.l[k] = w;
    }
  barrier();
}

// F = sum over the pass's edges of l e^T L e + (uncertain ? mu (sqrt(l) - 1)^2 : 0), in the order of icp_sum
template <class Barrier>
PGO_HD double pgo_total(const PgoGraph& v, int En, const double* q, double mu, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
  double F[1];
  icp_sum<1>(En, lane_begin, lane_end,
             [&](int64_t k, double* acc) {
#pragma clang fp contract(off)
               const double w = v.l[k];
               double term = w * q[k];
               if (v.uncertain[v.list[k]]) {
                 const double r = pg_sqrt(w) - 1.0;
                 const double rr = r * r;
                 const double m = mu * rr;
                 term = term + m;
               }
               acc[0] += term;
             },
             sh, barrier, F);
  return F[0];
}

// H (the lower triangle, column-major: entry (r, c), r >= c, at H[c n6 + r]) and b from the pass's edges under X: every entry is the sum
// of its edges' terms in ascending edge index from zero.  Each edge's W and g are formed once, one edge per lane; then one entry per lane
// walks the edges of its row's node (adj: ascending) and adds what belongs to it.
template <class Barrier>
PGO_HD void pgo_system(const PgoGraph& v, int En, const double* X, const double* e, int lane_begin, int lane_end, Barrier&& barrier) {
#pragma clang fp contract(off)
  const int N = v.N, n6 = 6 * N;
  for (int l = lane_begin; l < lane_end; l++)
    for (int k = l; k < En; k += kPgoLanes) {
      const int64_t o = v.list[k];
      pgo_edge_system(X + 16 * v.edges[2 * o], X + 16 * v.edges[2 * o + 1], v.T + 16 * o, v.info + 36 * o, e + 6 * k, v.l[k], v.W + 36 * k,
                      v.g + 6 * k);
    }
  barrier();
  for (int l = lane_begin; l < lane_end; l++) {
    for (int idx = l; idx < N * N * 36; idx += kPgoLanes) {
      const int blk = idx / 36, ij = idx % 36, p = blk / N, c = blk % N, i = ij / 6, j = ij % 6;
      if (c > p || (c == p && j > i)) continue;
      double s = 0.0;
      for (int a = v.adj_off[p]; a < v.adj_off[p + 1]; a++) {
        const int k = v.adj[2 * a], other = v.adj[2 * a + 1] >> 1;
        if (c == p) s = s + v.W[36 * k + 6 * i + j];
        else if (other == c) s = s - v.W[36 * k + 6 * i + j];
      }
      v.H[(size_t)(6 * c + j) * n6 + 6 * p + i] = s;
    }
    for (int r = l; r < n6; r += kPgoLanes) {
      const int p = r / 6, i = r % 6;
      double s = 0.0;
      for (int a = v.adj_off[p]; a < v.adj_off[p + 1]; a++) {
        const int k = v.adj[2 * a];
        if (v.adj[2 * a + 1] & 1) s = s - v.g[6 * k + i];      // the node is the edge's target
        else s = s + v.g[6 * k + i];
      }
      v.b[r] = s;
    }
  }
  barrier();
}

// delta <- the solution of (H + lambda I) delta = -b by a Cholesky factorisation, L_ij = (a_ij - sum_{k<j} L_ik L_jk) / L_jj with the
// k-sum in ascending k, every product and subtraction rounded on its own (column by column: lane i forms row i's entry; row j of L is
// the panel in sh).  The forward solve subtracts in ascending k, the backward solve in descending k: the order in which the unknowns
// become known.  False, the same on every lane, when a pivot is not > 0 or not finite.
template <class Barrier>
PGO_HD bool pgo_solve(const PgoGraph& v, double lambda, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  const int n6 = 6 * v.N;
  double* L = v.L;
  double* panel = sh + kPgoShSums;
  double* vec = panel + kPgoMaxDim;
  for (int l = lane_begin; l < lane_end; l++) {
    for (int idx = l; idx < n6 * n6; idx += kPgoLanes) {
      const int c = idx / n6, r = idx % n6;
      if (r >= c) L[idx] = r == c ? v.H[idx] + lambda : v.H[idx];
    }
    for (int i = l; i < n6; i += kPgoLanes) vec[i] = -v.b[i];
  }
  barrier();
  for (int j = 0; j < n6; j++) {
    for (int l = lane_begin; l < lane_end; l++)
      for (int k = l; k < j; k += kPgoLanes) panel[k] = L[(size_t)k * n6 + j];
    barrier();
    for (int l = lane_begin; l < lane_end; l++)
      for (int i = j + l; i < n6; i += kPgoLanes) {
        double s = L[(size_t)j * n6 + i];
        for (int k = 0; k < j; k++) {
          const double m = L[(size_t)k * n6 + i] * panel[k];
          s = s - m;
        }
        L[(size_t)j * n6 + i] = s;
      }
    barrier();
    const double d = L[(size_t)j * n6 + j];
    barrier();                                                           // (every lane has read the pivot that the next loop overwrites)
    if (!(d > 0.0) || !(d < INFINITY)) return false;
    const double ljj = pg_sqrt(d);
    for (int l = lane_begin; l < lane_end; l++)
      for (int i = j + l; i < n6; i += kPgoLanes) L[(size_t)j * n6 + i] = i == j ? ljj : L[(size_t)j * n6 + i] / ljj;
    barrier();
  }
  for (int k = 0; k < n6; k++) {
    const double yk = vec[k] / L[(size_t)k * n6 + k];
    for (int l = lane_begin; l < lane_end; l++)
      for (int i = k + l; i < n6; i += kPgoLanes) {
        if (i == k) {
          v.y[k] = yk;
        } else {
          const double m = L[(size_t)k * n6 + i] * yk;
          vec[i] = vec[i] - m;
        }
      }
    barrier();
  }
  for (int l = lane_begin; l < lane_end; l++)
    for (int i = l; i < n6; i += kPgoLanes) vec[i] = v.y[i];
  barrier();
  for (int k = n6 - 1; k >= 0; k--) {
    const double xk = vec[k] / L[(size_t)k * n6 + k];
    barrier();                                                           // (read before lane k % 256 may go on; vec[k] is not written again)
    for (int l = lane_begin; l < lane_end; l++)
      for (int i = l; i <= k; i += kPgoLanes) {
        if (i == k) {
          v.delta[k] = xk;
        } else {
          const double m = L[(size_t)i * n6 + k] * xk;
          vec[i] = vec[i] - m;
        }
      }
    barrier();
  }
  return true;
}

// One pass over the edges list[0 .. En) from the poses in st.X; on return st.X holds the pass's poses and v.l its line process.
// Uniform over the lanes.
template <class Barrier>
PGO_HD void pgo_pass(const PgoGraph& v, const PgoOptions& o, int En, int pass, PgoState& st, int* status, int* stop_reason, int* iterations,
                     int* trials_out, double* residual, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  const int N = v.N, n6 = 6 * N;
  // the edges of every node, ascending: adj holds (edge, 2 other + (the node is the target))
  if (lane_begin == 0) {
    // (adj_off has N + 2 words: the counts go two places up, so that after the prefix sums word n + 1 is node n's cursor, and after
    // the fill node n + 1's start)
    for (int n = 0; n <= N + 1; n++) v.adj_off[n] = 0;
    for (int k = 0; k < En; k++) v.adj_off[v.edges[2 * v.list[k]] + 2]++, v.adj_off[v.edges[2 * v.list[k] + 1] + 2]++;
    for (int n = 2; n <= N + 1; n++) v.adj_off[n] += v.adj_off[n - 1];
    for (int k = 0; k < En; k++) {
      const int s = (int)v.edges[2 * v.list[k]], t = (int)v.edges[2 * v.list[k] + 1];
      int a = v.adj_off[s + 1]++;
      v.adj[2 * a] = k, v.adj[2 * a + 1] = 2 * t;
      a = v.adj_off[t + 1]++;
      v.adj[2 * a] = k, v.adj[2 * a + 1] = 2 * s + 1;
    }
  }
  barrier();
  double s1[1];
  icp_sum<1>(En, lane_begin, lane_end, [&](int64_t k, double* acc) { acc[0] += v.info[36 * (int64_t)v.list[k] + 35]; }, sh, barrier, s1);
  const double r2 = o.max_correspondence_distance * o.max_correspondence_distance;
  const double pr = o.preference_loop_closure * r2;
  const double mu = En > 0 ? pr * (s1[0] / (double)En) : 0.0;
  pgo_residuals(v, En, st.X, st.e, st.q, lane_begin, lane_end, barrier);
  pgo_line_process(v, En, st.q, mu, lane_begin, lane_end, barrier);
  double F = pgo_total(v, En, st.q, mu, lane_begin, lane_end, sh, barrier);
  pgo_system(v, En, st.X, st.e, lane_begin, lane_end, barrier);
  const double maxdiag = fgr_max(n6, lane_begin, lane_end, [&](int64_t i) { return fabs(v.H[(size_t)i * n6 + i]); }, sh, barrier);
  double lambda = 1e-5 * maxdiag, nu = 2.0;
  double maxb = fgr_max(n6, lane_begin, lane_end, [&](int64_t i) { return fabs(v.b[i]); }, sh, barrier);
  int reason = SE3_PGO_STOP_NONE, it = 0, trials = 0;
  bool stop = false;
  auto fire = [&](int why) {
    if (!stop) reason = why;
    stop = true;
  };
  if (maxb < o.min_right_term) fire(SE3_PGO_STOP_RIGHT_TERM);
  int64_t trace_at = pass == 0 ? 0 : (v.trace_count ? v.trace_count[0] : 0), trace_n = 0;
  for (; !stop; it++) {
    int lm = 0;
    double rho = 0.0;
    do {
      bool left = false, accepted = false;                               // left: a test that leaves the trial loop before its count
      const double used = lambda;
      double Fn = NAN;
      rho = 0.0;
      trials++;
      if (!pgo_solve(v, lambda, lane_begin, lane_end, sh, barrier)) {
        *status |= SE3_PGO_SINGULAR;
        fire(SE3_PGO_STOP_REFUSED);
        left = true;
      } else {
        double nn[2];
        icp_sum<2>(n6, lane_begin, lane_end,
                   [&](int64_t i, double* acc) {
#pragma clang fp contract(off)
                     double x[6];
                     pgo_vec6(st.X + 16 * (i / 6), x);
                     const double dd = v.delta[i] * v.delta[i], xx = x[i % 6] * x[i % 6];
                     acc[0] += dd, acc[1] += xx;
                   },
                   sh, barrier, nn);
        const double nd = pg_sqrt(nn[0]), nx = pg_sqrt(nn[1]);
        const double bound = o.min_relative_increment * (nx + o.min_relative_increment);
        if (nd < bound) fire(SE3_PGO_STOP_RELATIVE_INCREMENT);
        if (!stop) {
          double bad[1];
          icp_sum<1>(n6, lane_begin, lane_end, [&](int64_t i, double* acc) { acc[0] += (i % 6 < 3 && !(fabs(v.delta[i]) < kPgoMaxAngle)) ? 1.0 : 0.0; },
                     sh, barrier, bad);
          if (bad[0] > 0.0) {
            *status |= SE3_PGO_STEP_REFUSED;
            fire(SE3_PGO_STOP_REFUSED);
            left = true;
          } else {
            for (int l = lane_begin; l < lane_end; l++)
              for (int n = l; n < N; n += kPgoLanes) {
                const double* x = v.delta + 6 * n;
                double sx, cx, sy, cy, sz, cz, U[16];
                fgr_sincos(x[0], &sx, &cx), fgr_sincos(x[1], &sy, &cy), fgr_sincos(x[2], &sz, &cz);
                icp_sincos_to_matrix(sx, cx, sy, cy, sz, cz, x, U);
                icp_compose(U, st.X + 16 * n, st.Xn + 16 * n);
              }
            barrier();
            pgo_residuals(v, En, st.Xn, st.en, st.qn, lane_begin, lane_end, barrier);
            Fn = pgo_total(v, En, st.qn, mu, lane_begin, lane_end, sh, barrier);
            double den[1];
            icp_sum<1>(n6, lane_begin, lane_end,
                       [&](int64_t i, double* acc) {
#pragma clang fp contract(off)
                         const double ld = lambda * v.delta[i];
                         const double m = v.delta[i] * (ld - v.b[i]);
                         acc[0] += m;
                       },
                       sh, barrier, den);
            rho = (F - Fn) / (den[0] + 1e-3);
            if (rho > 0.0) {
              if (F - Fn < o.min_relative_residual_increment * F) {
                fire(SE3_PGO_STOP_RELATIVE_RESIDUAL);
                left = true;
              } else {
                const double c = 2.0 * rho - 1.0;
                const double c3 = 1.0 - c * c * c;
                const double inner = c3 < o.upper_scale_factor ? c3 : o.upper_scale_factor;
                lambda = lambda * (o.lower_scale_factor > inner ? o.lower_scale_factor : inner);
                nu = 2.0;
                accepted = true;
                F = Fn;
                double* t;
                t = st.X, st.X = st.Xn, st.Xn = t;
                t = st.e, st.e = st.en, st.en = t;
                t = st.q, st.q = st.qn, st.qn = t;
                pgo_line_process(v, En, st.q, mu, lane_begin, lane_end, barrier);
                pgo_system(v, En, st.X, st.e, lane_begin, lane_end, barrier);
                maxb = fgr_max(n6, lane_begin, lane_end, [&](int64_t i) { return fabs(v.b[i]); }, sh, barrier);
                if (maxb < o.min_right_term) {
                  fire(SE3_PGO_STOP_RIGHT_TERM);
                  left = true;
                }
              }
            } else {
              lambda = lambda * nu;
              nu = 2.0 * nu;
            }
          }
        }
      }
      if (v.trace && lane_begin == 0 && trace_at + trace_n < v.trace_rows) {
        double* row = v.trace + 4 * (trace_at + trace_n);
        row[0] = used, row[1] = rho, row[2] = accepted ? 1.0 : 0.0, row[3] = Fn;
        trace_n++;
      }
      if (left) break;
      lm++;
      if (lm >= o.max_iteration_lm) fire(SE3_PGO_STOP_MAX_ITERATION_LM);
    } while (!(rho > 0.0 || stop));
    if (F < o.min_residual) fire(SE3_PGO_STOP_RESIDUAL);
    if (it + 1 >= o.max_iteration) fire(SE3_PGO_STOP_MAX_ITERATION);
  }
  if (v.trace_count && lane_begin == 0) v.trace_count[pass] = (int)trace_n;
  *stop_reason = reason, *iterations = it, *trials_out = trials, *residual = F;
}

// The whole optimisation of a graph: the refusals, pass 1 on all edges, the pruning, pass 2 on the kept edges, the reference node.
template <class Barrier>
PGO_HD void pgo_graph_optimize(const PgoGraph& v, const PgoOptions& o, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  const int N = v.N, E = v.E;
  double bad[2];
  icp_sum<2>((int64_t)16 * N + 53 * (int64_t)E, lane_begin, lane_end,
             [&](int64_t i, double* acc) {
               if (i < 16 * (int64_t)N) {
                 acc[0] += isfinite(v.X0[i]) ? 0.0 : 1.0;
                 return;
               }
               i -= 16 * (int64_t)N;
               if (i < 16 * (int64_t)E) {
                 acc[0] += isfinite(v.T[i]) ? 0.0 : 1.0;
               } else if (i < 52 * (int64_t)E) {
                 acc[0] += isfinite(v.info[i - 16 * (int64_t)E]) ? 0.0 : 1.0;
               } else {
                 const int64_t k = i - 52 * (int64_t)E, s = v.edges[2 * k], t = v.edges[2 * k + 1];
                 acc[1] += (s < 0 || s >= N || t < 0 || t >= N || s == t) ? 1.0 : 0.0;
               }
             },
             sh, barrier, bad);
  const bool options_ok = isfinite(o.min_relative_increment) && isfinite(o.min_relative_residual_increment) && isfinite(o.min_right_term) &&
                          isfinite(o.min_residual) && isfinite(o.upper_scale_factor) && isfinite(o.lower_scale_factor) &&
                          isfinite(o.max_correspondence_distance) && isfinite(o.edge_prune_threshold) && isfinite(o.preference_loop_closure);
  int status = 0;
  if (bad[0] > 0.0 || !options_ok) status = SE3_PGO_NONFINITE;
  else if (N == 0) status = SE3_PGO_EMPTY;
  else if (bad[1] > 0.0) status = SE3_PGO_BAD_INDEX;
  if (status != 0) {
    for (int l = lane_begin; l < lane_end; l++) {
      for (int i = l; i < 16 * N; i += kPgoLanes) v.X[i] = NAN;
      for (int k = l; k < E; k += kPgoLanes) v.conf1[k] = 0.0, v.conf2[k] = 0.0, v.kept[k] = 0;
    }
    if (lane_begin == 0) {
      *v.status = status;
      for (int k = 0; k < 6; k++) v.out_info[k] = 0;
      v.out_info[0] = v.out_info[3] = SE3_PGO_STOP_REFUSED;
      v.residuals[0] = v.residuals[1] = 0.0;
      if (v.trace_count) v.trace_count[0] = v.trace_count[1] = 0;
    }
    return;
  }
  PgoState st = {v.Xa, v.Xb, v.ea, v.eb, v.qa, v.qb};
  for (int l = lane_begin; l < lane_end; l++) {
    for (int i = l; i < 16 * N; i += kPgoLanes) st.X[i] = v.X0[i];
    for (int k = l; k < E; k += kPgoLanes) v.list[k] = k;
  }
  barrier();
  int info[6];
  double res[2];
  pgo_pass(v, o, E, 0, st, &status, &info[0], &info[1], &info[2], &res[0], lane_begin, lane_end, sh, barrier);
  for (int l = lane_begin; l < lane_end; l++) {
    for (int k = l; k < E; k += kPgoLanes) {
      v.conf1[k] = v.l[k], v.conf2[k] = 0.0;
      v.kept[k] = (!v.uncertain[k] || v.l[k] > o.edge_prune_threshold) ? 1 : 0;
    }
  }
  barrier();
  int En = 0;
  for (int k = 0; k < E; k++) En += v.kept[k];                           // (every lane counts: uniform)
  barrier();
  if (lane_begin == 0)
    for (int k = 0, n = 0; k < E; k++)
      if (v.kept[k]) v.list[n++] = k;
  barrier();
  pgo_pass(v, o, En, 1, st, &status, &info[3], &info[4], &info[5], &res[1], lane_begin, lane_end, sh, barrier);
  for (int l = lane_begin; l < lane_end; l++)
    for (int k = l; k < En; k += kPgoLanes) v.conf2[v.list[k]] = v.l[k];
  // the reference node: every pose is left-multiplied by X_ref(input) X_ref(output)^-1; the node itself gets its input pose, exactly
  double C[16];
  if (v.reference_node >= 0) {
    double inv[16];
    pgo_inverse(st.X + 16 * v.reference_node, inv);
    icp_compose(v.X0 + 16 * v.reference_node, inv, C);
  }
  for (int l = lane_begin; l < lane_end; l++)
    for (int n = l; n < N; n += kPgoLanes) {
      double out[16];
      if (v.reference_node < 0) {
        for (int k = 0; k < 16; k++) out[k] = st.X[16 * n + k];
      } else if (n == v.reference_node) {
        for (int k = 0; k < 16; k++) out[k] = v.X0[16 * n + k];
      } else {
        icp_compose(C, st.X + 16 * n, out);
      }
      for (int k = 0; k < 16; k++) v.X[16 * n + k] = out[k];
    }
  if (lane_begin == 0) {
    *v.status = status;
    for (int k = 0; k < 6; k++) v.out_info[k] = info[k];
    v.residuals[0] = res[0], v.residuals[1] = res[1];
  }
}

// ---- the information matrix of a pair --------------------------------------------------------------------------------------------------------
// Lambda = sum G^T G over the source rows with nn_d2 < r2, G of the REFERENCE point q = ref[nn_idx]; the 21 distinct entries in the order
// of icp_sum (sh holds 21 columns).  A non-finite coordinate or transform: a NaN matrix and NONFINITE; an empty cloud: zero and EMPTY.
template <class Barrier>
PGO_HD void pgo_information(const void* src, int elem, int64_t n, const double* ref, int64_t nref, const double* T, const int* nn_idx,
                            const double* nn_d2, double r2, double* out, double* out_count, int* out_status, int lane_begin, int lane_end,
                            double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  double bad_s[1], bad_r[1];
  icp_sum<1>(n, lane_begin, lane_end, [&](int64_t i, double* acc) { acc[0] += icp_finite3(src, elem, i) ? 0.0 : 1.0; }, sh, barrier, bad_s);
  icp_sum<1>(nref, lane_begin, lane_end, [&](int64_t i, double* acc) { acc[0] += icp_finite3(ref, 1, i) ? 0.0 : 1.0; }, sh, barrier, bad_r);
  bool refused = bad_s[0] + bad_r[0] > 0.0;
  for (int k = 0; k < 16; k++) refused = refused || !isfinite(T[k]);
  double s[21];
  int status = 0;
  if (refused) {
    status = SE3_PGO_NONFINITE;
    for (int k = 0; k < 21; k++) s[k] = NAN;
  } else if (n == 0 || nref == 0) {
    status = SE3_PGO_EMPTY;
    for (int k = 0; k < 21; k++) s[k] = 0.0;
  } else {
    icp_sum<21>(n, lane_begin, lane_end,
                [&](int64_t i, double* acc) {
#pragma clang fp contract(off)
                  if (!(nn_d2[i] < r2)) return;
                  const double* q = ref + 3 * (int64_t)nn_idx[i];
                  const double G[3][6] = {{0.0, q[2], -q[1], 1.0, 0.0, 0.0}, {-q[2], 0.0, q[0], 0.0, 1.0, 0.0}, {q[1], -q[0], 0.0, 0.0, 0.0, 1.0}};
                  for (int a = 0, e = 0; a < 6; a++)
                    for (int b = a; b < 6; b++, e++) {
                      const double x = G[0][a] * G[0][b], y = G[1][a] * G[1][b], z = G[2][a] * G[2][b];
                      const double t = (x + y) + z;
                      acc[e] += t;
                    }
                },
                sh, barrier, s);
  }
  if (lane_begin == 0) {
    for (int a = 0, e = 0; a < 6; a++)
      for (int b = a; b < 6; b++, e++) out[6 * a + b] = out[6 * b + a] = s[e];
    *out_count = refused ? NAN : s[20];
    *out_status = status;
  }
}
