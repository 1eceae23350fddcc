// pgo_cov_plan.h -- the host half of the pose graph's covariance calls (pgo_cov.hip: vsl_pgo_covariance,
// vsl_pgo_joint_covariance, vsl_pgo_edge_consistency): everything derived from the graph and the query before the first
// byte goes to the device.  Plain C++, no HIP, no vsl_ctx: tests/cpp/pgo_cov_plan_test.cpp drives it under g++.
//   pgc_check_pairs   the argument rules of a pair list
//   pgc_classify      from a device numbering: the class of every pair, the unique column nodes, the unit-column blocks
//   pgc_plan          a PAIR query: device numbering (the fold on the ring route), the class of every pair, the unique
//                     column nodes and each pair's columns among them, the unit-column blocks, the share of the arena
//   pgc_node_plan     a NODE-LIST query (the marginal call): the same numbering, the unique queried nodes in ascending
//                     device order and each query's place among them, their unit columns on the dense route (none on
//                     the band routes: a diagonal block lies inside the band of the inverse), the same share of the arena
// THE ORDER THE DEVICE SEES.  Routes 0 and 1 keep the nodes' own order: device free index = free index.  Route 2
// relabels the free nodes by the fold of chol_plan.h (free index f -> chol_fold_pos(nf, f)) and puts the fixed nodes
// behind them in their old order: what pgo_cov.hip's pgo_fold_problem hands to the device.
// CLASSES on the band routes (bw = the half bandwidth of the band the device builds):
//   PGC_ONE_FIXED  one node is fixed: its rows and columns are zero, the other node's diagonal block is read from Z
//   PGC_READ       6 |f_a - f_b| + 5 <= bw: the whole cross block lies in the band of the inverse, read from Z
//   PGC_SOLVE      every other pair: the six unit columns of ONE node are solved against the band factor -- the node
//                  with the LARGER device free index (a rule of the unordered pair): its forward substitution starts at
//                  its own row, the later of the two, and the back substitution stops at the other node's row
// On the dense route every queried free node gets its six columns (the diagonal blocks come from them as well) and a
// cross block is the average of the two mirror entries.  A pair's or a node's columns depend on it alone, so a result
// never depends on what else is queried; a column node shared by several queries is solved once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "chol_plan.h"

#define PGC_COLS 16  // unit columns of a workgroup: one matrix-instruction tile (COV_COLS of ba_cov_plan.h)

enum PgcPairError { PGC_PAIR_OK = 0, PGC_PAIR_RANGE = 1, PGC_PAIR_SAME = 2, PGC_PAIR_BOTH_FIXED = 3 };
enum PgcKind { PGC_ONE_FIXED = 0, PGC_READ = 1, PGC_SOLVE = 2 };

// first offending pair in *bad (untouched when all are fine)
inline int pgc_check_pairs(int n_nodes, const uint8_t* node_fixed, const int32_t* a, const int32_t* b, int n_pairs, int* bad) {
  for (int q = 0; q < n_pairs; q++) {
    int e = PGC_PAIR_OK;
    if (a[q] < 0 || a[q] >= n_nodes || b[q] < 0 || b[q] >= n_nodes)
      e = PGC_PAIR_RANGE;
    else if (a[q] == b[q])
      e = PGC_PAIR_SAME;
    else if (node_fixed[a[q]] && node_fixed[b[q]])
      e = PGC_PAIR_BOTH_FIXED;
    if (e) {
      if (bad) *bad = q;
      return e;
    }
  }
  return PGC_PAIR_OK;
}

// one pair as the device kernels read it (eight ints)
struct PgcPairDev {
  int32_t fa, fb;  // device free index, -1: fixed
  int32_t ca, cb;  // first of the node's six right-hand sides in X, -1: none
  int32_t na, nb;  // node ids of the device problem (its poses)
  int32_t kind, pad;
};

inline size_t pgc_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct PgcPlan {
  int nf = 0, n = 0, bw = 0, n_pairs = 0, nblk = 0;
  bool dense = false, folded = false;
  int n_fixed = 0, n_read = 0, n_solve = 0;
  std::vector<int> dev_free;   // node -> device free index, -1: fixed
  std::vector<int> dev_node;   // node -> node id of the device problem
  std::vector<int> col_nodes;  // unique column nodes, ascending device free index: right-hand sides 6 s .. 6 s + 5 for slot s
  std::vector<PgcPairDev> pairs;
  std::vector<int> col_unk;    // [PGC_COLS * nblk] unknown of each unit column, -1: an empty column
  std::vector<int> row_lo;     // [nblk] lowest row of X that a pair reads from the block (band routes)
  // the node-list query (pgc_node_plan; empty in a pair plan)
  std::vector<int> q_free;     // the unique queried nodes, ascending device free index: diagonal block s belongs to q_free[s]
  std::vector<int> q_slot;     // [queries] the block of each query
  // the caller's share of the arena: [inputs, one copy up | work | outputs, one copy back]; with_cand: the edge call
  size_t off_pairs = 0, off_q_free = 0, off_col_unk = 0, off_row_lo = 0, off_meas = 0, off_meas_cov = 0, in_bytes = 0;
  size_t off_Hdiag = 0, off_Linv = 0, off_X = 0;
  size_t out_off = 0, off_blocks = 0, off_cov = 0, off_resid = 0, off_resid_cov = 0, off_chi2 = 0, out_bytes = 0, total = 0;  // outputs relative to out_off
};

// the unit-column blocks of P.col_nodes (unique, ascending): six columns per node, PGC_COLS per workgroup
inline void pgc_columns(PgcPlan& P) {
  const int m = 6 * (int)P.col_nodes.size();
  P.nblk = (m + PGC_COLS - 1) / PGC_COLS;
  P.col_unk.assign((size_t)P.nblk * PGC_COLS, -1);
  for (int j = 0; j < m; j++) P.col_unk[j] = 6 * P.col_nodes[j / 6] + j % 6;
  P.row_lo.assign(P.nblk, P.n);
}

// The part of the plan that follows from a device numbering: P.nf, P.n, P.dev_free, P.dev_node are set by the caller
// (pgc_plan below for the pose graph; ba_pair_plan.h for the reduced camera system of a bundle adjustment, whose band
// order is the reverse Cuthill-McKee order of its host plan).  Fills the pairs, their classes, the unique column nodes,
// the unit-column blocks and row_lo.
inline void pgc_classify(PgcPlan& P, bool dense, int bw, bool no_band_read, const int32_t* a, const int32_t* b, int n_pairs) {
  P.dense = dense;
  P.bw = dense ? 0 : bw;
  P.n_pairs = n_pairs;
  P.pairs.resize(n_pairs);
  for (int q = 0; q < n_pairs; q++) {
    PgcPairDev& d = P.pairs[q];
    d.fa = P.dev_free[a[q]];
    d.fb = P.dev_free[b[q]];
    d.na = P.dev_node[a[q]];
    d.nb = P.dev_node[b[q]];
    d.ca = d.cb = -1;
    d.pad = 0;
    if (d.fa < 0 || d.fb < 0)
      d.kind = PGC_ONE_FIXED;
    else if (!dense && !no_band_read && 6 * std::abs(d.fa - d.fb) + 5 <= bw)
      d.kind = PGC_READ;
    else
      d.kind = PGC_SOLVE;
    P.n_fixed += d.kind == PGC_ONE_FIXED;
    P.n_read += d.kind == PGC_READ;
    P.n_solve += d.kind == PGC_SOLVE;
    if (dense) {
      if (d.fa >= 0) P.col_nodes.push_back(d.fa);
      if (d.fb >= 0) P.col_nodes.push_back(d.fb);
    } else if (d.kind == PGC_SOLVE) {
      P.col_nodes.push_back(std::max(d.fa, d.fb));
    }
  }
  std::sort(P.col_nodes.begin(), P.col_nodes.end());
  P.col_nodes.erase(std::unique(P.col_nodes.begin(), P.col_nodes.end()), P.col_nodes.end());
  pgc_columns(P);
  auto slot_of = [&](int f) { return (int)(std::lower_bound(P.col_nodes.begin(), P.col_nodes.end(), f) - P.col_nodes.begin()); };
  for (int q = 0; q < n_pairs; q++) {
    PgcPairDev& d = P.pairs[q];
    if (dense) {
      if (d.fa >= 0) d.ca = 6 * slot_of(d.fa);
      if (d.fb >= 0) d.cb = 6 * slot_of(d.fb);
    } else if (d.kind == PGC_SOLVE) {
      const int c = 6 * slot_of(std::max(d.fa, d.fb)), lo = 6 * std::min(d.fa, d.fb);
      (d.fa > d.fb ? d.ca : d.cb) = c;
      for (int blk = c / PGC_COLS; blk <= (c + 5) / PGC_COLS; blk++) P.row_lo[blk] = std::min(P.row_lo[blk], lo);
    }
  }
}

// the device numbering of a pose graph (see the file header): P.nf, P.n, P.dev_free, P.dev_node
inline void pgc_number(PgcPlan& P, int n_nodes, const uint8_t* node_fixed, bool folded) {
  P.folded = folded;
  for (int i = 0; i < n_nodes; i++) P.nf += node_fixed[i] ? 0 : 1;
  P.n = 6 * P.nf;
  P.dev_free.assign(n_nodes, -1);
  P.dev_node.resize(n_nodes);
  for (int i = 0, f = 0, next_fixed = P.nf; i < n_nodes; i++) {
    if (node_fixed[i]) {
      P.dev_node[i] = folded ? next_fixed++ : i;
    } else {
      P.dev_free[i] = folded ? chol_fold_pos(P.nf, f) : f;
      P.dev_node[i] = folded ? P.dev_free[i] : i;
      f++;
    }
  }
}

// the share of the arena of a classified plan (either query: the other one's slots are empty)
inline void pgc_layout(PgcPlan& P, bool with_cand) {
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += pgc_align(bytes);
    return o;
  };
  const size_t np = (size_t)P.n_pairs, nc = with_cand ? np : 0, nq = P.q_free.size();
  P.off_pairs = take(sizeof(PgcPairDev) * np);
  P.off_q_free = take(sizeof(int) * nq);
  P.off_col_unk = take(sizeof(int) * P.col_unk.size());
  P.off_row_lo = take(sizeof(int) * P.row_lo.size());
  P.off_meas = take(sizeof(double) * 6 * nc);
  P.off_meas_cov = take(sizeof(double) * 36 * nc);
  P.in_bytes = at;
  P.off_Hdiag = take(sizeof(double) * (size_t)P.n);
  P.off_Linv = take(P.dense ? sizeof(double) * (size_t)((P.n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB : 0);
  P.off_X = take(sizeof(double) * (size_t)P.nblk * P.n * PGC_COLS);
  P.out_off = at;
  P.off_blocks = take(sizeof(double) * 36 * nq) - P.out_off;
  P.off_cov = take(sizeof(double) * 144 * np) - P.out_off;
  P.off_resid = take(sizeof(double) * 6 * nc) - P.out_off;
  P.off_resid_cov = take(sizeof(double) * 36 * nc) - P.out_off;
  P.off_chi2 = take(sizeof(double) * nc) - P.out_off;
  P.out_bytes = at - P.out_off;
  P.total = at;
}

// node_fixed: [n_nodes]; folded: the ring route; dense / bw: the storage decision for the problem the device builds
// (pgo_storage); no_band_read: the diagnostic that sends in-band pairs through the solve.  The pairs have passed
// pgc_check_pairs.
inline PgcPlan pgc_plan(int n_nodes, const uint8_t* node_fixed, bool folded, bool dense, int bw, bool no_band_read,
                        const int32_t* a, const int32_t* b, int n_pairs, bool with_cand) {
  PgcPlan P;
  pgc_number(P, n_nodes, node_fixed, folded);
  pgc_classify(P, dense, bw, no_band_read, a, b, n_pairs);
  pgc_layout(P, with_cand);
  return P;
}

// The node-list query: nodes[0 .. n_q) are in range and free (duplicates and any order allowed).  The dense route
// solves the six unit columns of every unique queried node, ascending -- the columns pgc_classify gives a dense pair
// query that names the same nodes, so both calls solve the same workgroups; the band routes solve none.
inline PgcPlan pgc_node_plan(int n_nodes, const uint8_t* node_fixed, bool folded, bool dense, int bw, const int32_t* nodes, int n_q) {
  PgcPlan P;
  pgc_number(P, n_nodes, node_fixed, folded);
  P.dense = dense;
  P.bw = dense ? 0 : bw;
  for (int q = 0; q < n_q; q++) P.q_free.push_back(P.dev_free[nodes[q]]);
  std::sort(P.q_free.begin(), P.q_free.end());
  P.q_free.erase(std::unique(P.q_free.begin(), P.q_free.end()), P.q_free.end());
  P.q_slot.resize(n_q);
  for (int q = 0; q < n_q; q++)
    P.q_slot[q] = (int)(std::lower_bound(P.q_free.begin(), P.q_free.end(), P.dev_free[nodes[q]]) - P.q_free.begin());
  if (dense) P.col_nodes = P.q_free;
  pgc_columns(P);
  pgc_layout(P, false);
  return P;
}
