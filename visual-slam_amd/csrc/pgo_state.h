// pgo_state.h -- host-side state of a pose-graph call and the host functions that pgo.hip, the home of the solver's
// kernels, shares with the covariance calls (pgo_cov.hip).  The build has no relocatable device code: a kernel is launched
// from the file that defines it, so pgo_cov.hip reaches the linearisation through these.
#pragma once
#include <vector>

#include "vsl_common.h"
#include "dev_arena.h"
#include "pgo_far_plan.h"

// THE storage decision of a graph: dense (ld = 0), or, when the graph is narrow in the nodes' own order (keyframes in
// time order: odometry + covisibility edges, and the loop edge that closes the ring), lower band storage -- linear or
// CYCLIC (the band closes on itself; chol.hip's ring solver) -- with ld = bw + 32 slots left of the diagonal.
struct PgoStorage {
  int ld = 0, bw = 0, cyclic = 0;
  size_t h_elems = 0;
  int route() const { return ld > 0 ? (cyclic ? 2 : 1) : 0; }  // the `storage` the entry points report
};

struct PgoState {
  int N = 0, E = 0, n = 0;
  int ld = 0, bw = 0, cyclic = 0;  // the PgoStorage handed to pgo_setup (the far-edge route: the band of the near edges)
  size_t h_elems = 0;
  size_t extra_bytes = 0;    // the caller's share of the arena (the covariance calls: pgo_cov_plan.h)
  char* extra = nullptr;
  // ONE device allocation per solve (dev_arena.h): 23 hipMalloc / hipFree pairs were ~1 ms of a 3 ms solve
  DevArena arena;
  double *poses = nullptr, *cand = nullptr, *meas = nullptr, *r = nullptr, *Ja = nullptr, *Jb = nullptr, *cost = nullptr;
  double *colsq = nullptr, *scale = nullptr, *H = nullptr, *g = nullptr, *A = nullptr, *b = nullptr, *gabs = nullptr;
  double *part = nullptr, *part2 = nullptr, *scalars = nullptr;
  int *free_idx = nullptr, *edge_a = nullptr, *edge_b = nullptr, *inc_off = nullptr, *inc = nullptr, *flag = nullptr;
  // per-edge information matrices (the _w entry points; null: identity weights, the unweighted kernels).  U: what
  // pgo_edge_whiten_kernel leaves, 21 doubles per edge, null when unweighted; wbad: its lowest failing edge
  const double* edge_info = nullptr;  // host, [E][36]
  const char* who = "vsl_pose_graph_optimize";  // the entry point, for the messages of pgo_setup
  double* U = nullptr;
  int* wbad = nullptr;
  // FAR EDGES.  far_mode: 0 the route is not asked for (every call but the two below), 1 vsl_pose_graph_optimize* with
  // the switch on (taken when today's decision is dense with n > 128 and the plan finds a split), 2 vsl_pgo_far_solve
  // (every size; far_max_near as handed in).  far_on: this solve takes it -- the storage is then the linear band of the
  // near edges, and the plan's share of the arena sits in `extra`.
  int far_mode = 0, far_max_near = -1;
  bool far_on = false;
  PgfPlan far;
  uint8_t* far_flags = nullptr;
  int *far_list = nullptr, *far_row_first = nullptr, *far_ok = nullptr;
  double *far_Linv = nullptr, *far_X = nullptr, *far_C = nullptr, *far_z = nullptr, *far_diag = nullptr, *far_dfar = nullptr;
};

int pgo_validate(vsl_ctx* ctx, const vsl_pgo_problem* p);
// node -> free index (-1: fixed), the free nodes counted in node order
std::vector<int> pgo_free_index(const vsl_pgo_problem* p, int* nf_out);
// The decision (host only) from 6 nf unknowns and the edges' distances in free indices.  force_dense: the parity hooks;
// linear_only: a folded ring -- the relabelled graph is a linear band, never a ring again.  A call decides once per
// problem it builds and hands the result to pgo_setup.
PgoStorage pgo_storage(vsl_ctx* ctx, const vsl_pgo_problem* p, const std::vector<int>& free_idx, int nf, bool force_dense,
                       bool linear_only);
// the arena (st.extra_bytes of it the caller's), the uploads, the incidence lists, the whitened weights
int pgo_setup(vsl_ctx* ctx, const vsl_pgo_problem* p, const std::vector<int>& free_idx, int nf, const PgoStorage& sto, PgoState& st);
// residuals + Jacobians at st.poses and the scaled normal equations; first: with the Jacobi scale taken from this
// linearisation.  *cost_out = total cost (synchronises)
int pgo_linearize(vsl_ctx* ctx, PgoState& st, const vsl_ba_options* opt, bool first, double* cost_out);
// unit scale (the solver's Jacobi scale is not part of H), one linearisation at the poses as they are: the H of
// vsl_pgo_linearize, of the covariance calls and of vsl_pgo_far_solve
int pgo_linearize_unit(vsl_ctx* ctx, PgoState& st, const vsl_ba_options* opt, double* cost_out);
