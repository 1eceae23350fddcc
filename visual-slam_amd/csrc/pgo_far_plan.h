// pgo_far_plan.h -- the host half of the pose graph's band-plus-low-rank route (pgo.hip "FAR EDGES", DESIGN.md
// section 25): which edges leave the band, how wide the band of the rest is, the right-hand-side blocks and the arena.
// Plain C++, no HIP, no vsl_ctx: tests/cpp/pgo_far_plan_test.cpp drives it under g++.
//
// The damped, scaled normal equations are split as A = M + W W^T: M keeps every edge whose endpoints are at most d*
// apart in free index (and the LM diagonal), W has six columns per FAR edge.  Distances:
//   d_e = |f_a - f_b|   both endpoints free
//   d_e = 0             one endpoint fixed (the edge touches one diagonal block only: always near)
//   d_e = -1            both endpoints fixed (the edge takes no part)
// CANDIDATES are the distinct d_e >= 0; for a candidate d*: far = {e : d_e > d*}, k = |far|, bw = 6 d* + 5, m = 6 k.
// ADMISSIBLE: 1 <= k <= PGF_MAX_FAR, the band rule of pgo_storage (bw + 33) * 2 < n, and every connected component of
// the near graph over the free nodes holds a node with an edge to a fixed node (union-find) -- else M is singular as soon
// as the damping is small (two sessions joined only by loop edges).
// CHOICE: the admissible candidate with the least pgf_model_flops, ties to the smaller d*.  The model's constants are
// operation counts, not measurements.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "chol_plan.h"

#define PGF_COLS 16      // right-hand sides of a workgroup: one matrix-instruction tile (COV_COLS, vsl_cov_x_at)
#define PGF_MAX_FAR 128  // most far edges of a split: C is at most 768 x 768

enum PgfStatus {
  PGF_OK = 0,
  PGF_NO_SPLIT = 1,      // max_near_distance < 0: no candidate is admissible
  PGF_BAND_TOO_WIDE = 2, // forced d*: the band is not narrower than the matrix
  PGF_TOO_MANY_FAR = 3   // forced d*: more than PGF_MAX_FAR far edges
};

// factor + forward and back substitution of m + 1 columns + the sparse rows of C + C's factor
inline double pgf_model_flops(int n, int bw, int m) {
  const double dn = n, db = bw, dm = m;
  return dn * db * db + 4.0 * dn * db * (dm + 1.0) + 24.0 * dm * dm + dm * dm * dm / 3.0;
}

inline bool pgf_band_rule(int n, int bw) { return (size_t)(bw + 33) * 2 < (size_t)n; }

inline size_t pgf_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct PgfPlan {
  int status = PGF_OK;
  int nf = 0, n = 0;
  int d_star = 0, bw = 0, k = 0, m = 0;
  int ncols = 0, nblk = 0;         // m + 1 right-hand sides (column 0: b) in nblk blocks of PGF_COLS
  std::vector<int> free_idx;       // node -> free index, -1: fixed
  std::vector<int> dist;           // d_e per edge (-1: both endpoints fixed)
  std::vector<uint8_t> far;        // per edge
  std::vector<int> far_edges;      // the far edges, in edge order: far edge e' owns columns 1 + 6 e' .. 6 + 6 e'
  std::vector<int> row_first;      // [nblk] first non-zero row of the block's right-hand sides (n: an empty block)
  // the caller's share of the arena, bytes from its start: [inputs, one copy up | work]
  size_t off_far = 0, off_far_edges = 0, off_row_first = 0, in_bytes = 0;
  size_t off_Linv = 0, off_X = 0, off_C = 0, off_z = 0, off_diag = 0, off_dfar = 0, off_flag = 0, total = 0;
};

inline void pgf_distances(int n_nodes, const uint8_t* node_fixed, const int32_t* ea, const int32_t* eb, int n_edges, PgfPlan& P) {
  P.free_idx.assign(n_nodes, -1);
  P.nf = 0;
  for (int i = 0; i < n_nodes; i++)
    if (!node_fixed[i]) P.free_idx[i] = P.nf++;
  P.n = 6 * P.nf;
  P.dist.resize(n_edges);
  for (int e = 0; e < n_edges; e++) {
    const int fa = P.free_idx[ea[e]], fb = P.free_idx[eb[e]];
    P.dist[e] = (fa < 0 && fb < 0) ? -1 : (fa < 0 || fb < 0) ? 0 : std::abs(fa - fb);
  }
}

// every component of the near graph (free nodes, edges with both endpoints free and d_e <= d_star) is anchored
inline bool pgf_anchored(const PgfPlan& P, const int32_t* ea, const int32_t* eb, int n_edges, int d_star) {
  std::vector<int> parent(P.nf);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  for (int e = 0; e < n_edges; e++) {
    const int fa = P.free_idx[ea[e]], fb = P.free_idx[eb[e]];
    if (fa < 0 || fb < 0 || P.dist[e] > d_star) continue;
    const int ra = find(fa), rb = find(fb);
    if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
  }
  std::vector<uint8_t> anchored(P.nf, 0);
  for (int e = 0; e < n_edges; e++) {
    const int fa = P.free_idx[ea[e]], fb = P.free_idx[eb[e]];
    if ((fa < 0) == (fb < 0)) continue;
    anchored[find(fa < 0 ? fb : fa)] = 1;
  }
  for (int f = 0; f < P.nf; f++)
    if (!anchored[find(f)]) return false;
  return true;
}

inline int pgf_count_far(const PgfPlan& P, int d_star) {
  int k = 0;
  for (int d : P.dist) k += d > d_star;
  return k;
}

inline bool pgf_admissible(const PgfPlan& P, const int32_t* ea, const int32_t* eb, int n_edges, int d_star) {
  const int k = pgf_count_far(P, d_star);
  return k >= 1 && k <= PGF_MAX_FAR && pgf_band_rule(P.n, 6 * d_star + 5) && pgf_anchored(P, ea, eb, n_edges, d_star);
}

// the admissible candidate of least model cost, ties to the smaller d*; -1: none
inline int pgf_choose(const PgfPlan& P, const int32_t* ea, const int32_t* eb, int n_edges) {
  std::vector<int> cand;
  for (int d : P.dist)
    if (d >= 0) cand.push_back(d);
  std::sort(cand.begin(), cand.end());
  cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
  int best = -1;
  double best_cost = 0.0;
  for (int d : cand) {  // ascending: a strict comparison keeps the smaller d* on a tie
    if (!pgf_admissible(P, ea, eb, n_edges, d)) continue;
    const double c = pgf_model_flops(P.n, 6 * d + 5, 6 * pgf_count_far(P, d));
    if (best < 0 || c < best_cost) {
      best = d;
      best_cost = c;
    }
  }
  return best;
}

// max_near_distance < 0: the plan's choice (PGF_NO_SPLIT when no candidate is admissible); >= 0: d* as given, k = 0
// allowed (a plain band solve), not checked for anchoring (a singular M fails its pivot test on the device).
inline PgfPlan pgf_plan(int n_nodes, const uint8_t* node_fixed, const int32_t* ea, const int32_t* eb, int n_edges, int max_near_distance) {
  PgfPlan P;
  pgf_distances(n_nodes, node_fixed, ea, eb, n_edges, P);
  if (max_near_distance < 0) {
    P.d_star = pgf_choose(P, ea, eb, n_edges);
    if (P.d_star < 0) {
      P.d_star = 0;
      P.status = PGF_NO_SPLIT;
      return P;
    }
  } else {
    P.d_star = max_near_distance;
    if (max_near_distance >= P.nf || !chol_band_declared(P.n, 6 * max_near_distance + 5)) {  // (also: no free node)
      P.status = PGF_BAND_TOO_WIDE;
      return P;
    }
    if (pgf_count_far(P, P.d_star) > PGF_MAX_FAR) {
      P.status = PGF_TOO_MANY_FAR;
      return P;
    }
  }
  P.bw = 6 * P.d_star + 5;
  P.far.assign(n_edges, 0);
  for (int e = 0; e < n_edges; e++)
    if (P.dist[e] > P.d_star) {
      P.far[e] = 1;
      P.far_edges.push_back(e);
    }
  P.k = (int)P.far_edges.size();
  P.m = 6 * P.k;
  P.ncols = P.m + 1;
  P.nblk = (P.ncols + PGF_COLS - 1) / PGF_COLS;
  // column 0 is b: dense from row 0.  A far edge's columns are non-zero at its two endpoints' rows only.
  P.row_first.assign(P.nblk, P.n);
  if (P.nblk > 0) P.row_first[0] = 0;
  for (int q = 0; q < P.k; q++) {
    const int e = P.far_edges[q], lo = 6 * std::min(P.free_idx[ea[e]], P.free_idx[eb[e]]);
    for (int blk = (1 + 6 * q) / PGF_COLS; blk <= (6 + 6 * q) / PGF_COLS; blk++) P.row_first[blk] = std::min(P.row_first[blk], lo);
  }
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += pgf_align(bytes);
    return o;
  };
  const size_t n = (size_t)P.n, m = (size_t)P.m;
  P.off_far = take((size_t)n_edges);
  P.off_far_edges = take(sizeof(int) * (size_t)P.k);
  P.off_row_first = take(sizeof(int) * (size_t)P.nblk);
  P.in_bytes = at;
  P.off_Linv = take(sizeof(double) * (size_t)((P.n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB);
  P.off_X = take(sizeof(double) * (size_t)P.nblk * n * PGF_COLS);
  P.off_C = take(sizeof(double) * m * m);
  P.off_z = take(sizeof(double) * m);
  P.off_diag = take(sizeof(double) * n);  // diag M before the factorisation (the hook's pivot test)
  P.off_dfar = take(sizeof(double) * n);  // diag W W^T (the LM diagonal is taken from the full diag H)
  P.off_flag = take(sizeof(int) * 2);
  P.total = at;
  return P;
}
