// The integer work of DBSCAN on the grid of csrc/pair_grid.h (csrc/dbscan.hip carries the contract): the core test, the lock-free union
// of neighbouring core rows, a row's label.  __host__ __device__ text that the kernels and se3_debug_dbscan_host both run; the caller
// hands in how a parent word is read (load), lowered (lower: an atomic minimum) and exchanged (cas), so the host runs the same loops on
// plain memory.
//
// The forest.  parent[x] <= x always; x is a root iff parent[x] == x.  Only two writes exist: cas(a, a, b) with b < a on a ROOT a (a hook:
// the larger root goes under the smaller), and lower(x, g) with g < parent[x] an ancestor of x on a NON-root x (path halving).  A row that
// stopped being a root never becomes one again, every word only ever decreases, and a word always names a member of its own set.  So the
// root of a set is its lowest row, whatever the order of the writes, and the final partition is that of the undirected graph alone.
//
// Termination.  db_find: every step moves to parent[x] < x, so it ends within x steps whatever other threads write meanwhile.  db_union:
// a pass ends when the two roots are equal or its cas succeeds; the cas fails only when another thread's cas on the same word succeeded
// in between (lower never touches a root), and at most n - 1 hooks can succeed in a cloud of n rows, so the failed passes of all threads
// together are bounded by (n - 1) times the number of threads: lock-free, no thread waits for another's write, there is no lock.
#pragma once
#include <stdint.h>

#include "pair_grid.h"

// the root of x's set at some moment of the walk, halving the path on the way
template <class Load, class Lower>
PG_HD int db_find(int x, Load&& load, Lower&& lower) {
  for (;;) {
    const int p = load(x);
    if (p == x) return x;
    const int g = load(p);
    if (g < p) lower(x, g);
    x = p;
  }
}

// one set of a's and b's
template <class Load, class Lower, class Cas>
PG_HD void db_union(int a, int b, Load&& load, Lower&& lower, Cas&& cas) {
  for (;;) {
    a = db_find(a, load, lower);
    b = db_find(b, load, lower);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    if (cas(a, b) == a) return;                              // parent[a]: a -> b, if a is still a root
  }
}

// i is a core row iff its ball (d^2 < eps eps strict, itself and duplicates included) holds at least min_points rows
PG_HD bool db_is_core(const PairGridView& g, int p, const double* q, double eps, int64_t min_points) {
  return pg_ball_count(g, p, q, eps, eps * eps) >= min_points;
}

// core row i of cloud p: one set with every core neighbour of a lower index (the relation is symmetric: d^2 is formed from squares)
template <class Core, class Load, class Lower, class Cas>
PG_HD void db_link_row(const PairGridView& g, int p, const double* q, double eps, int i, Core&& core, Load&& load, Lower&& lower, Cas&& cas) {
  pg_ball_walk(g, p, q, eps, eps * eps, [&](int j) {
    if (j < i && core(j)) db_union(i, j, load, lower, cas);
  });
}

// the label of row i once every core row knows its root and every root its rank: a core row's own cluster, else the lowest cluster among
// its core neighbours, else -1
template <class Core, class Cluster>
PG_HD int db_label_row(const PairGridView& g, int p, const double* q, double eps, int i, Core&& core, Cluster&& cluster) {
  if (core(i)) return cluster(i);
  int best = -1;
  pg_ball_walk(g, p, q, eps, eps * eps, [&](int j) {
    if (!core(j)) return;
    const int c = cluster(j);
    if (best < 0 || c < best) best = c;
  });
  return best;
}
