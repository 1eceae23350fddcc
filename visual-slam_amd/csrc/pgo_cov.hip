// pgo_cov.hip -- covariances of a pose graph: blocks of H^-1, H = J^T J of one linearisation at the poses handed in (unit
// scale, no damping: what vsl_pgo_linearize returns).
//   vsl_pgo_covariance[_w]         the 6 x 6 diagonal blocks of a list of nodes
//   vsl_pgo_joint_covariance[_w]   the 12 x 12 joint blocks of pairs of nodes
//   vsl_pgo_edge_consistency[_w]   on top of those, the covariance and the chi-square of a candidate edge's residual
// (include/vslam_hip.h has the definitions).  ONE run serves all three.  The host plan -- the fold, the class of each
// pair, the column nodes, the share of the arena -- is pgo_cov_plan.h; the set-up and the linearisation are the solver's
// (pgo_state.h); the chain from diag H to the blocks of the inverse is the layer shared with bundle adjustment
// (ba_cov.hip, vsl_cov_*_dev in vsl_common.h).  Three routes, chosen by pgo_storage as for the solve:
//   0 dense        vsl_chol_factor_dev, then the unit columns of every distinct queried free node -- O(n^2) per column;
//                  diagonal and cross blocks are read from them
//   1 linear band  vsl_chol_selinv_band_dev (chol.hip "SELECTED INVERSION"): the whole band of H^-1 in O(n bw^2).  The
//                  diagonal blocks lie inside it (bw >= 5), and so do the cross blocks of PGC_READ pairs; for the
//                  PGC_SOLVE pairs the band unit-column solve with the inverted diagonal blocks the inversion left
//   2 ring         the FREE nodes are relabelled by the fold of chol_plan.h on the host -- free index f becomes
//                  chol_fold_pos(nf, f), the edges follow, the edge ORDER stays -- so that the ring is a linear band of at
//                  most twice the node distance; pgo_build_kernel builds that band as for any graph, then route 1.  A
//                  block of the inverse does not move under a relabelling of the nodes.
// then vsl_cov_diag_blocks_dev (the node list), vsl_cov_pair_blocks_dev (the pairs) and pgo_edge_consistency_kernel (one
// wavefront per candidate, the edge call only).
// "Not positive definite" is the rule of ba_cov.hip on every route: a pivot L_ii^2 <= 2^-36 H_ii, diag H taken before
// the factorisation.  A block depends on H alone, never on what else is queried; the band routes read the lower
// triangle of a block and mirror it, the dense route averages the two mirror entries: exactly symmetric either way.
// A joint block's diagonal blocks are the marginal call's bytes: the same kernels behind the same run.
#include <algorithm>
#include <vector>

#include "vsl_common.h"
#include "pgo_cov_plan.h"
#include "pgo_device.h"
#include "pgo_state.h"

namespace {

// One wavefront per candidate.  Lane 0 evaluates r and both Jacobian blocks with the dual numbers of
// pgo_linearize_kernel (seed_pose, edge_residual; no corrector); the lanes share T = Sigma J^T (12 x 6) and M = J T
// (6 x 6), every sum in ascending index order; Sigma_r = (M + M^T) / 2; lane 0 factors Sigma_r + Sigma_m and solves.
__global__ __launch_bounds__(64) void pgo_edge_consistency_kernel(int n_cand, const double* __restrict__ poses,
                                                                  const PgcPairDev* __restrict__ pairs, const double* __restrict__ meas,
                                                                  const double* __restrict__ meas_cov, const double* __restrict__ joint,
                                                                  const int* __restrict__ ok, double* __restrict__ resid,
                                                                  double* __restrict__ resid_cov, double* __restrict__ chi2) {
  __shared__ double Jm[6][12], Tm[12][6], Mm[6][6], rs[6];
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= n_cand || !*ok) return;
  const PgcPairDev p = pairs[q];
  if (lane == 0) {
    D12 qc[4], tc[3], qn[4], tn[3], rd[6];
    seed_pose(poses + 7 * (size_t)p.na, 0, qc, tc);
    seed_pose(poses + 7 * (size_t)p.nb, 6, qn, tn);
    edge_residual(qc, tc, qn, tn, meas + 6 * (size_t)q, rd);
    for (int i = 0; i < 6; i++) {
      rs[i] = rd[i].v;
      resid[6 * (size_t)q + i] = rd[i].v;
      // a fixed node does not move: its term is dropped
      for (int c = 0; c < 6; c++) {
        Jm[i][c] = p.fa >= 0 ? rd[i].d[c] : 0.0;
        Jm[i][6 + c] = p.fb >= 0 ? rd[i].d[6 + c] : 0.0;
      }
    }
  }
  __syncthreads();
  const double* S = joint + 144 * (size_t)q;
  for (int t = lane; t < 72; t += 64) {
    const int a = t / 6, i = t % 6;
    double s = 0.0;
    for (int b = 0; b < 12; b++) s += S[12 * a + b] * Jm[i][b];
    Tm[a][i] = s;
  }
  __syncthreads();
  if (lane < 36) {
    const int i = lane / 6, j = lane % 6;
    double s = 0.0;
    for (int a = 0; a < 12; a++) s += Jm[i][a] * Tm[a][j];
    Mm[i][j] = s;
  }
  __syncthreads();
  if (lane < 36) {
    const int i = lane / 6, j = lane % 6;
    resid_cov[36 * (size_t)q + lane] = 0.5 * (Mm[i][j] + Mm[j][i]);
  }
  if (lane == 0) {
    double A[6][6], y[6];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        A[i][j] = 0.5 * (Mm[i][j] + Mm[j][i]);
        if (meas_cov) A[i][j] += 0.5 * (meas_cov[36 * (size_t)q + 6 * i + j] + meas_cov[36 * (size_t)q + 6 * j + i]);
      }
    bool pd = true;
    double c2 = 0.0;
    for (int j = 0; j < 6 && pd; j++) {
      double d = A[j][j];
      for (int k = 0; k < j; k++) d -= A[j][k] * A[j][k];
      if (!(d > 0.0) || !isfinite(d)) {
        pd = false;
        break;
      }
      const double l = sqrt(d);
      A[j][j] = l;
      for (int i = j + 1; i < 6; i++) {
        double s = A[i][j];
        for (int k = 0; k < j; k++) s -= A[i][k] * A[j][k];
        A[i][j] = s / l;
      }
      double s = rs[j];
      for (int k = 0; k < j; k++) s -= A[j][k] * y[k];
      y[j] = s / l;
      c2 += y[j] * y[j];
    }
    chi2[q] = pd ? c2 : __builtin_nan("");
  }
}

// the graph with its free nodes relabelled by the fold: new id chol_fold_pos(nf, f) for free index f, the fixed nodes
// behind them in their old order
struct PgoFolded {
  std::vector<double> poses;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> ea, eb;
  vsl_pgo_problem prob;
};
void pgo_fold_problem(const vsl_pgo_problem* p, const std::vector<int>& free_idx, int nf, PgoFolded& F) {
  const int N = p->n_nodes, E = p->n_edges;
  std::vector<int> new_of(N);
  int next_fixed = nf;
  for (int i = 0; i < N; i++) new_of[i] = free_idx[i] >= 0 ? chol_fold_pos(nf, free_idx[i]) : next_fixed++;
  F.poses.resize(7 * (size_t)N);
  F.fixed.resize(N);
  for (int i = 0; i < N; i++) {
    memcpy(&F.poses[7 * (size_t)new_of[i]], p->poses + 7 * (size_t)i, 7 * sizeof(double));
    F.fixed[new_of[i]] = p->node_fixed[i];
  }
  F.ea.resize(E);
  F.eb.resize(E);
  for (int e = 0; e < E; e++) {
    F.ea[e] = new_of[p->edge_a[e]];
    F.eb[e] = new_of[p->edge_b[e]];
  }
  F.prob = *p;
  F.prob.poses = F.poses.data();
  F.prob.node_fixed = F.fixed.data();
  F.prob.edge_a = F.ea.data();
  F.prob.edge_b = F.eb.data();
}

// One call: a node list (by_node: the marginal call) or a pair list (the joint call; with_cand: the edge call)
struct PgoCovCall {
  const char* name;
  const double* edge_info;  // the _w calls: information matrices of the graph's own edges (the fold keeps the edge order)
  bool by_node;
  const int32_t* nodes;
  int n_q;
  double* blocks;  // [n_q][36]
  const int32_t *a = nullptr, *b = nullptr;
  int n_pairs = 0;
  bool with_cand = false;
  const double *cand_meas = nullptr, *meas_cov = nullptr;                          // the edge call (meas_cov nullable)
  double *cov = nullptr, *resid = nullptr, *resid_cov = nullptr, *chi2 = nullptr;  // outputs (cov: the joint call; chi2 nullable)
  int count() const { return by_node ? n_q : n_pairs; }
};

// the argument rules of each call
int pgo_cov_check(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const PgoCovCall& c) {
  if (c.by_node) {
    if (!opt || c.n_q < 0 || (c.n_q > 0 && (!c.nodes || !c.blocks)))
      return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null argument or negative count", c.name);
    for (int q = 0; q < c.n_q; q++) {
      if (c.nodes[q] < 0 || c.nodes[q] >= prob->n_nodes) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: node %d out of range", c.name, c.nodes[q]);
      if (prob->node_fixed[c.nodes[q]]) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: node %d is fixed", c.name, c.nodes[q]);
    }
    return VSL_OK;
  }
  if (!opt || c.n_pairs < 0 ||
      (c.n_pairs > 0 && (!c.a || !c.b || (c.with_cand ? (!c.cand_meas || !c.resid || !c.resid_cov) : !c.cov))))
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null argument or negative count", c.name);
  int bad = 0;
  switch (pgc_check_pairs(prob->n_nodes, prob->node_fixed, c.a, c.b, c.n_pairs, &bad)) {
    case PGC_PAIR_RANGE: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d (%d, %d): node out of range", c.name, bad, c.a[bad], c.b[bad]);
    case PGC_PAIR_SAME: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d names node %d twice", c.name, bad, c.a[bad]);
    case PGC_PAIR_BOTH_FIXED: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d (%d, %d): both nodes are fixed", c.name, bad, c.a[bad], c.b[bad]);
    default: break;
  }
  return VSL_OK;
}

// Everything behind the validation.  run: the problem the device builds (the folded graph on the ring route), with its
// free index and storage decision; orig: the caller's graph, whose node ids the plan numbers (the fold is the plan's
// own).  host_in / host_out are read / written by copies on the stream.
int pgo_cov_run(vsl_ctx* ctx, const vsl_pgo_problem* run, const std::vector<int>& run_free, int nf, const PgoStorage& sto,
                const vsl_ba_options* opt, bool folded, const PgoCovCall& c, const vsl_pgo_problem* orig, std::vector<char>& host_in,
                std::vector<char>& host_out) {
  const bool dense = sto.ld == 0;
  const PgcPlan P = c.by_node ? pgc_node_plan(orig->n_nodes, orig->node_fixed, folded, dense, sto.bw, c.nodes, c.n_q)
                              : pgc_plan(orig->n_nodes, orig->node_fixed, folded, dense, sto.bw, ctx->pgo_cov_no_band_read, c.a, c.b,
                                         c.n_pairs, c.with_cand);
  PgoState st;
  st.edge_info = c.edge_info;
  st.who = c.name;
  st.extra_bytes = P.total;
  int rc;
  if ((rc = pgo_setup(ctx, run, run_free, nf, sto, st))) return rc;
  if (st.n != P.n) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: the set-up and the plan disagree", c.name);
  hipStream_t s = ctx->stream;
  const int n = st.n, np = P.n_pairs, nQ = (int)P.q_free.size();
  char* dev = st.extra;
  host_in.assign(P.in_bytes, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(host_in.data() + off, src, bytes);
  };
  put(P.off_pairs, P.pairs.data(), sizeof(PgcPairDev) * P.pairs.size());
  put(P.off_q_free, P.q_free.data(), sizeof(int) * P.q_free.size());
  put(P.off_col_unk, P.col_unk.data(), sizeof(int) * P.col_unk.size());
  put(P.off_row_lo, P.row_lo.data(), sizeof(int) * P.row_lo.size());
  if (c.with_cand) {
    put(P.off_meas, c.cand_meas, sizeof(double) * 6 * (size_t)np);
    if (c.meas_cov) put(P.off_meas_cov, c.meas_cov, sizeof(double) * 36 * (size_t)np);
  }
  VSL_HIP(ctx, hipMemcpyAsync(dev, host_in.data(), P.in_bytes, hipMemcpyHostToDevice, s));
  const PgcPairDev* pairs = (const PgcPairDev*)(dev + P.off_pairs);
  double* X = (double*)(dev + P.off_X);
  double* joint = (double*)(dev + P.out_off + P.off_cov);
  double cost = 0;
  if ((rc = pgo_linearize_unit(ctx, st, opt, &cost))) return rc;
  // st.A: the second band array of the solve, here the band of the inverse
  const VslCovInverse inv{n, st.ld, st.bw, st.H, dense ? nullptr : st.A, dense ? (double*)(dev + P.off_Linv) : nullptr,
                          (double*)(dev + P.off_Hdiag), (const int*)(dev + P.off_col_unk), (const int*)(dev + P.off_row_lo), P.nblk, X,
                          st.flag};
  if ((rc = vsl_cov_inverse_dev(ctx, inv))) return rc;
  if ((rc = vsl_cov_diag_blocks_dev(ctx, n, nQ, (const int*)(dev + P.off_q_free), st.ld, st.A, X, st.flag,
                                    (double*)(dev + P.out_off + P.off_blocks))))
    return rc;
  if ((rc = vsl_cov_pair_blocks_dev(ctx, n, np, pairs, dense ? 0 : 1, st.A, st.ld, X, st.flag, joint))) return rc;
  if (c.with_cand)
    hipLaunchKernelGGL(pgo_edge_consistency_kernel, dim3(np), dim3(64), 0, s, np, st.poses, pairs, (const double*)(dev + P.off_meas),
                       c.meas_cov ? (const double*)(dev + P.off_meas_cov) : (const double*)nullptr, joint, st.flag,
                       (double*)(dev + P.out_off + P.off_resid), (double*)(dev + P.out_off + P.off_resid_cov),
                       (double*)(dev + P.out_off + P.off_chi2));
  VSL_CHECK_LAUNCH(ctx);
  int ok = 0;
  host_out.assign(P.out_bytes, 0);
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data(), dev + P.out_off, P.out_bytes, hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipMemcpyAsync(&ok, st.flag, sizeof(int), hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipStreamSynchronize(s));
  if (!ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: the normal equations are not positive definite (no fixed node, or a free node without an edge)", c.name);
  for (int q = 0; q < c.n_q; q++)
    memcpy(c.blocks + 36 * (size_t)q, host_out.data() + P.off_blocks + sizeof(double) * 36 * (size_t)P.q_slot[q], 36 * sizeof(double));
  if (c.cov) memcpy(c.cov, host_out.data() + P.off_cov, sizeof(double) * 144 * (size_t)np);
  if (c.with_cand) {
    memcpy(c.resid, host_out.data() + P.off_resid, sizeof(double) * 6 * (size_t)np);
    memcpy(c.resid_cov, host_out.data() + P.off_resid_cov, sizeof(double) * 36 * (size_t)np);
    if (c.chi2) memcpy(c.chi2, host_out.data() + P.off_chi2, sizeof(double) * (size_t)np);
  }
  return VSL_OK;
}

// every entry point: the problem's and the call's rules, the route of the caller's graph (the solve's own decision, on
// the host), the fold on the ring route, the run, the drain on an error
int pgo_cov_call(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const PgoCovCall& c, int* storage) {
  int rc = pgo_validate(ctx, prob);
  if (rc) return rc;
  if ((rc = pgo_cov_check(ctx, prob, opt, c))) return rc;
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(prob, &nf);
  const PgoStorage sto = pgo_storage(ctx, prob, free_idx, nf, false, false);
  const int route = sto.route();
  if (storage) *storage = route;
  if (c.count() == 0) return VSL_OK;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<char> host_in, host_out;
  bool dense = sto.ld == 0;
  if (route == 2) {
    // the relabelled graph is a problem of its own: a linear band, never a ring again (or dense, where that band is wide)
    PgoFolded F;
    pgo_fold_problem(prob, free_idx, nf, F);
    int nf_run = 0;
    const std::vector<int> run_free = pgo_free_index(&F.prob, &nf_run);
    const PgoStorage run_sto = pgo_storage(ctx, &F.prob, run_free, nf_run, false, true);
    dense = run_sto.ld == 0;
    rc = pgo_cov_run(ctx, &F.prob, run_free, nf_run, run_sto, opt, true, c, prob, host_in, host_out);
  } else {
    rc = pgo_cov_run(ctx, prob, free_idx, nf, sto, opt, false, c, prob, host_in, host_out);
  }
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);  // queued copies read host buffers that end here
    return rc;
  }
  if (storage) *storage = dense ? 0 : route;
  return VSL_OK;
}

}  // namespace

extern "C" int vsl_pgo_covariance(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const int32_t* nodes, int n_q,
                                  double* cov, int* storage) {
  return pgo_cov_call(ctx, prob, opt, PgoCovCall{"vsl_pgo_covariance", nullptr, true, nodes, n_q, cov}, storage);
}
// H of the weighted problem
extern "C" int vsl_pgo_covariance_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                    const int32_t* nodes, int n_q, double* cov, int* storage) {
  return pgo_cov_call(ctx, prob, opt, PgoCovCall{"vsl_pgo_covariance_w", edge_info, true, nodes, n_q, cov}, storage);
}

extern "C" int vsl_pgo_joint_covariance(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const int32_t* pair_a,
                                        const int32_t* pair_b, int n_pairs, double* cov, int* storage) {
  const PgoCovCall c{"vsl_pgo_joint_covariance", nullptr, false, nullptr, 0, nullptr, pair_a, pair_b, n_pairs, false, nullptr, nullptr, cov};
  return pgo_cov_call(ctx, prob, opt, c, storage);
}
extern "C" int vsl_pgo_joint_covariance_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                          const int32_t* pair_a, const int32_t* pair_b, int n_pairs, double* cov, int* storage) {
  const PgoCovCall c{"vsl_pgo_joint_covariance_w", edge_info, false, nullptr, 0, nullptr, pair_a, pair_b, n_pairs, false, nullptr, nullptr, cov};
  return pgo_cov_call(ctx, prob, opt, c, storage);
}

extern "C" int vsl_pgo_edge_consistency(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const int32_t* cand_a,
                                        const int32_t* cand_b, const double* cand_meas, const double* meas_cov, int n_cand,
                                        double* resid, double* resid_cov, double* chi2, int* storage) {
  const PgoCovCall c{"vsl_pgo_edge_consistency", nullptr, false, nullptr, 0, nullptr, cand_a, cand_b, n_cand, true, cand_meas, meas_cov,
                     nullptr, resid, resid_cov, chi2};
  return pgo_cov_call(ctx, prob, opt, c, storage);
}
// edge_info shapes H and so Sigma; the candidate's residual stays unwhitened, meas_cov keeps its meaning
extern "C" int vsl_pgo_edge_consistency_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                          const int32_t* cand_a, const int32_t* cand_b, const double* cand_meas, const double* meas_cov,
                                          int n_cand, double* resid, double* resid_cov, double* chi2, int* storage) {
  const PgoCovCall c{"vsl_pgo_edge_consistency_w", edge_info, false, nullptr, 0, nullptr, cand_a, cand_b, n_cand, true, cand_meas, meas_cov,
                     nullptr, resid, resid_cov, chi2};
  return pgo_cov_call(ctx, prob, opt, c, storage);
}
