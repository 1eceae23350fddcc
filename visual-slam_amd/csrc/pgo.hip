// pgo.hip -- pose graph optimisation: the numerical core of
// visnav::pose_graph_optimization (include/visnav/loop_closure_utils.h:446-587).  Residual blocks
//     r = log(T_w_c^-1 * T_w_n) - upsilon_omega                  (PoseGraphRelativePoseCostFunctor, reprojection.h:107-126)
// on SE3 blocks with the tangent parameterisation T * exp(delta) (local_parameterization_se3.hpp:43-63),
// HuberLoss, Levenberg-Marquardt with the [upstream] Ceres policy restated for bundle adjustment in ba.hip.
//
// One thread per edge evaluates the residual and both 6x6 Jacobian blocks with forward-mode dual numbers
// (pgo_device.h: 12 partials, what ceres::AutoDiffCostFunction<., 6, 7, 7> followed by the SE3 plus-Jacobian computes), the
// normal equations are accumulated by row owners -- one thread owns one ROW of H and walks the node's incident edges in
// edge order (lists built once per solve on the host): no atomics, results do not depend on timing -- into the storage
// pgo_storage picks for the graph: a linear or cyclic band when the graph is narrow in the keyframes' own order (chol.hip's
// band and ring solvers), dense otherwise (the blocked Cholesky), and, opt-in, a band for the near edges plus a low-rank
// update for a few far ones where one long edge would otherwise make the whole matrix dense ("FAR EDGES" below,
// pgo_far_plan.h).  This runs once per loop closure.
// This file: the solver's kernels, the set-up, the LM loop, the linearise hooks and the far-edge route.  The covariance
// calls are pgo_cov.hip; they reach the set-up and the linearisation through pgo_state.h.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "vsl_common.h"
#include "lm_policy.h"
#include "dev_arena.h"
#include "pgo_far_plan.h"
#include "pgo_device.h"
#include "pgo_state.h"

namespace {

// Per-edge information matrices (the _w entry points): Omega_e = L L^T, U = L^T kept as its 21 upper-triangle entries
// row by row (row i: columns i .. 5).  One thread per edge: the two mirror entries of Omega averaged (the rule of
// meas_cov), 6 x 6 Cholesky, "not positive definite" by the rule of ba_cov.hip (a pivot L_ii^2 <= 2^-36 Omega_ii, or not
// finite); the lowest failing edge index is left in *bad (preset above every index; integer atomicMin: independent of timing).
__global__ __launch_bounds__(64) void pgo_edge_whiten_kernel(int n_edges, const double* __restrict__ info, double* __restrict__ U,
                                                             int* __restrict__ bad) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n_edges) return;
  const double* W = info + 36 * (size_t)e;
  double L[6][6];
  bool pd = true;
  for (int j = 0; j < 6; j++) {
    const double wjj = W[7 * j];
    double d = wjj;
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
    if (!isfinite(d) || !(d > 0x1p-36 * wjj)) {
      pd = false;
      break;
    }
    const double l = sqrt(d);
    L[j][j] = l;
    for (int i = j + 1; i < 6; i++) {
      double s = 0.5 * (W[6 * i + j] + W[6 * j + i]);
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  if (!pd) {
    atomicMin(bad, e);
    return;
  }
  double* Ue = U + 21 * (size_t)e;
  for (int i = 0, at = 0; i < 6; i++)
    for (int j = i; j < 6; j++) Ue[at++] = L[j][i];  // (an infinite entry has failed the pivot of its row above)
}

// r <- U r in place, rows ascending (row i reads entries i .. 5: none of them written yet), each row of U loaded when
// its turn comes; the sum of a row runs over ascending column index.  T = D12 (value and 12 partials) or double.
__device__ __forceinline__ double scl(double u, double a) { return u * a; }
__device__ __forceinline__ D12 scl(double u, const D12& a) {
  D12 r;
  r.v = u * a.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = u * a.d[i];
  return r;
}
template <class T>
__device__ __forceinline__ void whiten_rows(const double* __restrict__ Ue, T* r) {
#pragma unroll
  for (int i = 0, at = 0; i < 6; i++) {
    T acc = scl(Ue[at++], r[i]);
#pragma unroll
    for (int j = i + 1; j < 6; j++) acc = acc + scl(Ue[at++], r[j]);
    r[i] = acc;
  }
}

// r (6), Ja / Jb (6x6 row-major) per edge, robustified (ceres Corrector with rho'' <= 0: sqrt(rho') on both),
// cost[e] = rho(|r|^2) / 2.  WEIGHTED: r and its partials are whitened by the edge's U (pgo_edge_whiten_kernel) before
// the squared norm is taken -- Huber, the corrector and every consumer of r / Ja / Jb then see U r, U J.
template <bool JAC, bool WEIGHTED>
__global__ __launch_bounds__(64) void pgo_linearize_kernel(int n_edges, const double* __restrict__ poses, const int* __restrict__ edge_a,
                                                           const int* __restrict__ edge_b, const double* __restrict__ meas,
                                                           const double* __restrict__ U, int use_huber, double huber,
                                                           double* __restrict__ r_out, double* __restrict__ Ja,
                                                           double* __restrict__ Jb, double* __restrict__ cost) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n_edges) return;
  const double* pa = poses + 7 * (size_t)edge_a[e];
  const double* pb = poses + 7 * (size_t)edge_b[e];
  double r[6], s = 0;
  if (JAC) {
    D12 qc[4], tc[3], qn[4], tn[3], rd[6];
    seed_pose(pa, 0, qc, tc);
    seed_pose(pb, 6, qn, tn);
    edge_residual(qc, tc, qn, tn, meas + 6 * (size_t)e, rd);
    if (WEIGHTED) whiten_rows(U + 21 * (size_t)e, rd);
    for (int i = 0; i < 6; i++) {
      r[i] = rd[i].v;
      s += r[i] * r[i];
    }
    double k = 1.0;
    if (use_huber && s > huber * huber) k = sqrt(huber / sqrt(s));
    for (int i = 0; i < 6; i++)
      for (int c = 0; c < 6; c++) {
        Ja[36 * (size_t)e + 6 * i + c] = k * rd[i].d[c];
        Jb[36 * (size_t)e + 6 * i + c] = k * rd[i].d[6 + c];
      }
    for (int i = 0; i < 6; i++) r_out[6 * (size_t)e + i] = k * r[i];
  } else {
    edge_residual(pa, pa + 4, pb, pb + 4, meas + 6 * (size_t)e, r);
    if (WEIGHTED) whiten_rows(U + 21 * (size_t)e, r);
    for (int i = 0; i < 6; i++) s += r[i] * r[i];
  }
  double rho0 = s;
  if (use_huber && s > huber * huber) rho0 = 2.0 * huber * sqrt(s) - huber * huber;
  cost[e] = 0.5 * rho0;
}

// squared column norms of the (robustified) Jacobian, for the Jacobi scaling
// incidence lists: node i's entries inc[inc_off[i] .. inc_off[i + 1]) = 2 * edge + side (0: the node is edge_a, 1: edge_b),
// ascending.  One thread per (free node, column): squared column norm of the Jacobian, summed in list order.
__global__ void pgo_colsq_kernel(int n_nodes, const int* __restrict__ inc_off, const int* __restrict__ inc,
                                 const int* __restrict__ free_idx, const double* __restrict__ Ja, const double* __restrict__ Jb,
                                 double* __restrict__ colsq) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_nodes * 6) return;
  const int node = t / 6, c = t - node * 6;
  const int nx = free_idx[node];
  if (nx < 0) return;
  double s = 0;
  for (int k = inc_off[node]; k < inc_off[node + 1]; k++) {
    const int e = inc[k] >> 1, x = inc[k] & 1;
    const double* J = (x ? Jb : Ja) + 36 * (size_t)e;
    double q = 0;
    for (int i = 0; i < 6; i++) q += J[6 * i + c] * J[6 * i + c];
    s += q;
  }
  colsq[6 * nx + c] = s;
}

__global__ void pgo_scale_kernel(int n, const double* __restrict__ colsq, double* __restrict__ scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) scale[i] = 1.0 / (1.0 + sqrt(colsq[i]));
}

// H (n x n, scaled) += J^T J, g += J^T r: one thread per (edge, block x, column c)
// One thread per (free node, row c of its 6 x 6 block row): row 6 nx + c of the scaled normal equations and entry
// 6 nx + c of the gradient, accumulated over the node's incident edges in list order.  The thread is the only writer
// of its row (H and g are zeroed before the launch).
// Band forms (round 4): ld > 0 -- row i of H keeps its columns [i - (ld), i] at H[i * (ld + 1) + (j - i + ld)] (the
// LAPACK-style lower band storage of chol.hip, ld = bandwidth + 32); the thread writes the entries at or left of the
// diagonal (the mirror entries belong to the other endpoint's thread), and in the CYCLIC form (`cyclic`) the entries of
// the wrap-around corner (j - i >= n - bw: nodes that are neighbours around the loop) as (i, j - n) in the leading slots
// of its row.  ld = 0: dense, every entry.
// far (nullable; "FAR EDGES" below): an edge with far[e] set stays out of H -- g still sums it -- and its share of H_ii
// goes to dfar[i] instead.
__global__ void pgo_build_kernel(int n_nodes, int n, const int* __restrict__ inc_off, const int* __restrict__ inc,
                                 const int* __restrict__ edge_a, const int* __restrict__ edge_b,
                                 const int* __restrict__ free_idx, const double* __restrict__ r, const double* __restrict__ Ja,
                                 const double* __restrict__ Jb, const double* __restrict__ scale, double* __restrict__ H,
                                 double* __restrict__ g, int ld, int bw, int cyclic, const uint8_t* __restrict__ far = nullptr,
                                 double* __restrict__ dfar = nullptr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_nodes * 6) return;
  const int node = t / 6, c = t - node * 6;
  const int nx = free_idx[node];
  if (nx < 0) return;
  const double sx = scale[6 * nx + c];
  const int i = 6 * nx + c;
  double* __restrict__ Hrow = ld > 0 ? H + (size_t)i * (ld + 1) + (ld - i) : H + (size_t)i * n;  // Hrow[j] = entry (i, j)
  double gacc = 0, dacc = 0;  // dacc: the FAR edges' share of H_ii (far != null: they stay out of H, section "FAR EDGES")
  for (int k = inc_off[node]; k < inc_off[node + 1]; k++) {
    const int e = inc[k] >> 1, x = inc[k] & 1;
    const double* Jx = (x ? Jb : Ja) + 36 * (size_t)e;
    const double* re = r + 6 * (size_t)e;
    double col[6], gv = 0;
    for (int q = 0; q < 6; q++) {
      col[q] = Jx[6 * q + c];
      gv += col[q] * re[q];
    }
    gacc += sx * gv;
    if (far && far[e]) {
      double q2 = 0;
      for (int q = 0; q < 6; q++) q2 += col[q] * col[q];
      dacc += sx * sx * q2;
      continue;
    }
    for (int y = 0; y < 2; y++) {
      const int ny = free_idx[y ? edge_b[e] : edge_a[e]];
      if (ny < 0) continue;
      const double* Jy = (y ? Jb : Ja) + 36 * (size_t)e;
      for (int c2 = 0; c2 < 6; c2++) {
        int j = 6 * ny + c2;
        if (ld > 0) {
          if (j > i) {
            if (!(cyclic && j - i >= n - bw)) continue;  // the mirror entry is the other thread's
            j -= n;                                        // wrap-around corner: column "below zero"
          } else if (i - j > bw) {
            continue;  // (cyclic: the far side of a wrap pair -- stored by the row of the smaller index)
          }
        }
        double hv = 0;
        for (int q = 0; q < 6; q++) hv += col[q] * Jy[6 * q + c2];
        Hrow[j] += sx * scale[6 * ny + c2] * hv;
      }
    }
  }
  g[6 * nx + c] = gacc;
  if (dfar) dfar[i] = dacc;
}

// band forms: A = H (all s_elems slots) with the LM damping on the diagonal, b = -g, gabs
__global__ void pgo_damp_band_kernel(int n, size_t elems, int ld, const double* __restrict__ H, const double* __restrict__ g,
                                     const double* __restrict__ scale, double inv_radius, double* __restrict__ A,
                                     double* __restrict__ b, double* __restrict__ gabs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= elems) return;
  double v = H[t];
  const size_t row = t / (size_t)(ld + 1);
  if (row < (size_t)n && t - row * (ld + 1) == (size_t)ld) {  // the diagonal slot of row `row`
    v += fmin(fmax(v, 1e-6), 1e32) * inv_radius;
    b[row] = -g[row];
    gabs[row] = fabs(g[row] / scale[row]);
  }
  A[t] = v;
}

// ---- FAR EDGES (the host plan is pgo_far_plan.h).  The damped, scaled system the dense route
// would factorise is A = M + W W^T: M = the linear band of the NEAR edges plus the LM diagonal (pgo_build_kernel with the
// far flags, then the kernel below), W (n x m, m = 6 k) six columns per far edge e, column r of its block = the scaled
// row r of [Ja Jb] at the rows of its two endpoints.  With Y = M^-1 [b W] (band factor, vsl_band_rhs_solve_dev):
//   C = I + W^T Y_W,  C z = W^T y,  x = y - Y_W z
// Right-hand sides X: blocks of n x 16 (vsl_cov_x_at); column 0 is b, columns 1 + 6 e' .. 6 + 6 e' far edge e'.

// the band route's damping with the diagonal of the FULL H: H_ii = M_ii + (W W^T)_ii, as the dense route sees it
__global__ void pgo_damp_far_kernel(int n, size_t elems, int ld, const double* __restrict__ H, const double* __restrict__ dfar,
                                    const double* __restrict__ g, const double* __restrict__ scale, double inv_radius,
                                    double* __restrict__ A, double* __restrict__ b, double* __restrict__ gabs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= elems) return;
  double v = H[t];
  const size_t row = t / (size_t)(ld + 1);
  if (row < (size_t)n && t - row * (ld + 1) == (size_t)ld) {
    v += fmin(fmax(v + dfar[row], 1e-6), 1e32) * inv_radius;
    b[row] = -g[row];
    gabs[row] = fabs(g[row] / scale[row]);
  }
  A[t] = v;
}

// X (cleared by the caller) <- [b | W]: one thread per entry of b, then one per non-zero entry of W (72 per far edge)
__global__ void pgo_far_columns_kernel(int n, int k, const int* __restrict__ far_edges, const int* __restrict__ edge_a,
                                       const int* __restrict__ edge_b, const int* __restrict__ free_idx,
                                       const double* __restrict__ Ja, const double* __restrict__ Jb,
                                       const double* __restrict__ scale, const double* __restrict__ b, double* __restrict__ X) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    X[vsl_cov_x_at(n, t, 0)] = b[t];
    return;
  }
  const int u = t - n;
  if (u >= 72 * k) return;
  const int q = u / 72, side = (u % 72) / 36, r = (u % 36) / 6, c = u % 6, e = far_edges[q];
  const int row = 6 * free_idx[side ? edge_b[e] : edge_a[e]] + c;  // (a far edge has two free endpoints)
  X[vsl_cov_x_at(n, row, 1 + 6 * q + r)] = scale[row] * (side ? Jb : Ja)[36 * (size_t)e + 6 * r + c];
}

// entry `at` (0 .. 11: endpoint a's six rows, then b's) of column j = 6 q + r of W: its row and value
__device__ __forceinline__ double pgo_far_w(int at, int e, int r, const int* __restrict__ edge_a, const int* __restrict__ edge_b,
                                            const int* __restrict__ free_idx, const double* __restrict__ Ja,
                                            const double* __restrict__ Jb, const double* __restrict__ scale, int* row) {
  const int side = at / 6, c = at - 6 * side;
  *row = 6 * free_idx[side ? edge_b[e] : edge_a[e]] + c;
  return scale[*row] * (side ? Jb : Ja)[36 * (size_t)e + 6 * r + c];
}

// C = I + W^T Y_W (m x m row-major, the lower triangle computed and mirrored: exactly symmetric) and rhs = W^T y.  One
// thread per (i, j), j = 0 .. m (j = m: the right-hand side); the sum runs over the 12 non-zero rows of W's column i in
// fixed order.
__global__ void pgo_far_capacitance_kernel(int n, int m, const int* __restrict__ far_edges, const int* __restrict__ edge_a,
                                           const int* __restrict__ edge_b, const int* __restrict__ free_idx,
                                           const double* __restrict__ Ja, const double* __restrict__ Jb,
                                           const double* __restrict__ scale, const double* __restrict__ X, double* __restrict__ Cm,
                                           double* __restrict__ rhs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)m * (m + 1)) return;
  const int i = (int)(t / (m + 1)), j = (int)(t - (size_t)i * (m + 1));
  if (j < m && j > i) return;  // the mirror of (j, i)
  const int e = far_edges[i / 6], r = i % 6, col = j == m ? 0 : 1 + j;
  double s = 0;
  for (int at = 0; at < 12; at++) {
    int row;
    const double w = pgo_far_w(at, e, r, edge_a, edge_b, free_idx, Ja, Jb, scale, &row);
    s += w * X[vsl_cov_x_at(n, row, col)];
  }
  if (j == m) {
    rhs[i] = s;
  } else {
    if (i == j) s += 1.0;
    Cm[(size_t)i * m + j] = s;
    Cm[(size_t)j * m + i] = s;
  }
}

// x = y - Y_W z, one thread per row, the m products summed in ascending column order.  A failed pivot of C (*ok_c)
// clears *flag, which a failed pivot of M has cleared already: the step is an unsuccessful one.
__global__ void pgo_far_apply_kernel(int n, int m, const double* __restrict__ X, const double* __restrict__ z,
                                     const int* __restrict__ ok_c, double* __restrict__ x, int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0 && !*ok_c) *flag = 0;
  double s = 0;
  for (int j = 0; j < m; j++) s += X[vsl_cov_x_at(n, i, 1 + j)] * z[j];
  x[i] = X[vsl_cov_x_at(n, i, 0)] - s;
}

// band forms: the model cost change without H: d^T H d = sum over the edges of |Ja S_a d_a + Jb S_b d_b|^2.
// part[e] = |J_e S d|^2 / 2 per edge; the gradient part -d_i g_i per unknown goes to part2 (flag cleared on a non-finite d_i)
__global__ void pgo_model_edges_kernel(int n_edges, const int* __restrict__ edge_a, const int* __restrict__ edge_b,
                                       const int* __restrict__ free_idx, const double* __restrict__ Ja,
                                       const double* __restrict__ Jb, const double* __restrict__ scale,
                                       const double* __restrict__ d, double* __restrict__ part) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const int fa = free_idx[edge_a[e]], fb = free_idx[edge_b[e]];
  double v[6] = {0, 0, 0, 0, 0, 0};
  // (H is the SCALED system S J^T J S and d its solution: the kernels' Ja / Jb are unscaled, build applies S -- so here)
  for (int side = 0; side < 2; side++) {
    const int f = side ? fb : fa;
    if (f < 0) continue;
    const double* J = (side ? Jb : Ja) + 36 * (size_t)e;
    for (int q = 0; q < 6; q++)
      for (int c = 0; c < 6; c++) v[q] += J[6 * q + c] * (scale[6 * f + c] * d[6 * f + c]);
  }
  double s = 0;
  for (int q = 0; q < 6; q++) s += v[q] * v[q];
  part[e] = 0.5 * s;
}
__global__ void pgo_model_grad_kernel(int n, const double* __restrict__ g, const double* __restrict__ d, double* __restrict__ part,
                                      int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  part[i] = -d[i] * g[i];
  if (!isfinite(d[i])) *flag = 0;
}

// A = H + diag(clamp(H_ii)) / radius, b = -g; gabs[i] = |g_i / scale_i|
__global__ void pgo_damp_kernel(int n, const double* __restrict__ H, const double* __restrict__ g, const double* __restrict__ scale,
                                double inv_radius, double* __restrict__ A, double* __restrict__ b, double* __restrict__ gabs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * n) return;
  const int i = (int)(t / n), j = (int)(t - (size_t)i * n);
  double v = H[t];
  if (i == j) {
    v += fmin(fmax(v, 1e-6), 1e32) * inv_radius;
    b[i] = -g[i];
    gabs[i] = fabs(g[i] / scale[i]);
  }
  A[t] = v;
}

// part[i] = -d_i (g_i + (H d)_i / 2); flag cleared if d_i is not finite
__global__ void pgo_model_kernel(int n, const double* __restrict__ H, const double* __restrict__ g, const double* __restrict__ d,
                                 double* __restrict__ part, int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double hd = 0;
  for (int j = 0; j < n; j++) hd += H[(size_t)i * n + j] * d[j];
  part[i] = -d[i] * (g[i] + 0.5 * hd);
  if (!isfinite(d[i])) *flag = 0;
}

// candidate poses T * exp(scale .* d) for the free nodes; part_step[i] / part_x[i] = squared norms per node
__global__ void pgo_update_kernel(int n_nodes, const int* __restrict__ free_idx, const double* __restrict__ poses,
                                  const double* __restrict__ d, const double* __restrict__ scale, double* __restrict__ cand,
                                  double* __restrict__ part_step, double* __restrict__ part_x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const double* p7 = poses + 7 * (size_t)i;
  double* o7 = cand + 7 * (size_t)i;
  const int f = free_idx[i];
  if (f < 0) {
    for (int c = 0; c < 7; c++) o7[c] = p7[c];
    part_step[i] = 0;
    part_x[i] = 0;
    return;
  }
  double dl[6], s2 = 0, x2 = 0;
  for (int c = 0; c < 6; c++) {
    dl[c] = scale[6 * f + c] * d[6 * f + c];
    s2 += dl[c] * dl[c];
  }
  for (int c = 0; c < 7; c++) x2 += p7[c] * p7[c];
  part_step[i] = s2;
  part_x[i] = x2;
  // Sophus SE3 exp (local_parameterization_se3.hpp:43-50: T * exp(delta))
  const double* ups = dl;
  const double* om = dl + 3;
  const double th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2], th = sqrt(th2);
  double imag, real, A, B;
  if (th < 1e-10) {
    imag = 0.5 - th2 / 48.0 + th2 * th2 / 3840.0;
    real = 1.0 - th2 / 8.0 + th2 * th2 / 384.0;
    A = 0.5;
    B = 1.0 / 6.0;
  } else {
    imag = sin(0.5 * th) / th;
    real = cos(0.5 * th);
    A = (1.0 - cos(th)) / th2;
    B = (th - sin(th)) / (th2 * th);
  }
  const double dq[4] = {imag * om[0], imag * om[1], imag * om[2], real};
  const double a[3] = {om[1] * ups[2] - om[2] * ups[1], om[2] * ups[0] - om[0] * ups[2], om[0] * ups[1] - om[1] * ups[0]};
  const double b[3] = {om[1] * a[2] - om[2] * a[1], om[2] * a[0] - om[0] * a[2], om[0] * a[1] - om[1] * a[0]};
  double dt[3], rt[3], q[4];
  for (int c = 0; c < 3; c++) dt[c] = ups[c] + A * a[c] + B * b[c];
  qrot(p7, dt, rt);
  qmul(p7, dq, q);
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; c++) o7[c] = q[c] / nq;
  for (int c = 0; c < 3; c++) o7[4 + c] = p7[4 + c] + rt[c];
}

__global__ __launch_bounds__(256) void pgo_reduce_kernel(const double* __restrict__ v, int n, double* __restrict__ out, int is_max) {
  __shared__ double sh[256];
  double a = 0;
  for (int i = threadIdx.x; i < n; i += 256) a = is_max ? fmax(a, v[i]) : a + v[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = is_max ? fmax(sh[threadIdx.x], sh[threadIdx.x + o]) : sh[threadIdx.x] + sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sh[0];
}

}  // namespace

int pgo_validate(vsl_ctx* ctx, const vsl_pgo_problem* p) {
  if (!ctx) return VSL_ERR_INVALID;
  if (!p || p->n_nodes < 0 || p->n_edges < 0 || (p->n_nodes > 0 && (!p->poses || !p->node_fixed)) ||
      (p->n_edges > 0 && (!p->edge_a || !p->edge_b || !p->edge_meas)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "pose graph: null arrays or negative sizes");
  for (int e = 0; e < p->n_edges; e++)
    if (p->edge_a[e] < 0 || p->edge_a[e] >= p->n_nodes || p->edge_b[e] < 0 || p->edge_b[e] >= p->n_nodes || p->edge_a[e] == p->edge_b[e])
      return vsl_fail(ctx, VSL_ERR_INVALID, "pose graph: edge %d connects %d and %d (%d nodes)", e, p->edge_a[e], p->edge_b[e], p->n_nodes);
  return VSL_OK;
}

namespace {
// the switch of the far-edge route: diagnostic "pgo_far_edges" or the environment variable VSL_PGO_FAR_EDGES
bool pgo_far_switch(const vsl_ctx* ctx) {
  static const bool env_on = getenv("VSL_PGO_FAR_EDGES") != nullptr;
  return ctx->pgo_far_edges || env_on;
}
}  // namespace

// THE storage decision of a graph (pgo_state.h)
PgoStorage pgo_storage(vsl_ctx* ctx, const vsl_pgo_problem* p, const std::vector<int>& free_idx, int nf, bool force_dense,
                       bool linear_only) {
  const int n = 6 * nf;
  int lin = 0, cyc = 0;
  for (int e = 0; e < p->n_edges; e++) {
    const int fa = free_idx[p->edge_a[e]], fb = free_idx[p->edge_b[e]];
    if (fa < 0 || fb < 0) continue;
    const int d = std::abs(fa - fb);
    lin = std::max(lin, d);
    cyc = std::max(cyc, std::min(d, nf - d));
  }
  const int bw_lin = 6 * lin + 5, bw_cyc = 6 * cyc + 5;
  int Bc = 0, nc = 0;
  static const bool env_dense = getenv("VSL_PGO_DENSE") != nullptr;
  PgoStorage sto;
  sto.h_elems = (size_t)n * n;
  if (!force_dense && !env_dense && !ctx->ba_force_dense && n > 128) {
    if (!linear_only && 2 * bw_cyc < bw_lin && chol_ring_available(n, bw_cyc, CholSwitches{ctx->chol_no_fused, ctx->chol_no_bcr, ctx->chol_one_ended}, &Bc, &nc)) {
      sto.cyclic = 1;
      sto.bw = bw_cyc;
    } else if ((size_t)(bw_lin + 33) * 2 < (size_t)n) {
      sto.bw = bw_lin;
    }
    if (sto.bw > 0) {
      sto.ld = sto.bw + 32;
      sto.h_elems = (size_t)n * (sto.ld + 1) + 64;
    }
  }
  return sto;
}

std::vector<int> pgo_free_index(const vsl_pgo_problem* p, int* nf_out) {
  std::vector<int> free_idx(p->n_nodes, -1);
  int nf = 0;
  for (int i = 0; i < p->n_nodes; i++)
    if (!p->node_fixed[i]) free_idx[i] = nf++;
  *nf_out = nf;
  return free_idx;
}

int pgo_setup(vsl_ctx* ctx, const vsl_pgo_problem* p, const std::vector<int>& free_idx, int nf, const PgoStorage& sto, PgoState& st) {
  st.N = p->n_nodes;
  st.E = p->n_edges;
  st.n = 6 * nf;
  st.ld = sto.ld;
  st.bw = sto.bw;
  st.cyclic = sto.cyclic;
  st.h_elems = sto.h_elems;
  if (st.far_mode == 1) {
    // dense by pgo_storage's own rule (not by a diagnostic that asks for dense; the solver never forces it), and a split exists
    static const bool env_dense = getenv("VSL_PGO_DENSE") != nullptr;
    if (st.ld == 0 && st.n > 128 && !env_dense && !ctx->ba_force_dense) {
      st.far = pgf_plan(p->n_nodes, p->node_fixed, p->edge_a, p->edge_b, p->n_edges, -1);
      st.far_on = st.far.status == PGF_OK;
    }
  } else if (st.far_mode == 2) {
    st.far = pgf_plan(p->n_nodes, p->node_fixed, p->edge_a, p->edge_b, p->n_edges, st.far_max_near);
    if (st.far.status == PGF_NO_SPLIT)
      return vsl_fail(ctx, VSL_ERR_INVALID, "%s: no admissible split (every candidate has no far edge, more than %d of them, a band that is not narrow, or a near component without a fixed neighbour)", st.who, PGF_MAX_FAR);
    if (st.far.status == PGF_BAND_TOO_WIDE)
      return vsl_fail(ctx, VSL_ERR_INVALID, "%s: max_near_distance %d: the band is not narrower than the matrix (%d unknowns)", st.who, st.far_max_near, st.n);
    if (st.far.status == PGF_TOO_MANY_FAR)
      return vsl_fail(ctx, VSL_ERR_INVALID, "%s: max_near_distance %d leaves more than %d far edges", st.who, st.far_max_near, PGF_MAX_FAR);
    st.far_on = true;
  }
  if (st.far_on) {
    st.cyclic = 0;
    st.bw = st.far.bw;
    st.ld = st.bw + 32;
    st.h_elems = (size_t)st.n * (st.ld + 1) + 64;
    st.extra_bytes = st.far.total;
  }
  const size_t N = st.N, E = st.E, n = st.n;
  ArenaPlan plan(26);
  plan.add(st.poses, 7 * N);
  plan.add(st.cand, 7 * N);
  plan.add(st.free_idx, N);
  plan.add(st.edge_a, E);
  plan.add(st.edge_b, E);
  plan.add(st.inc_off, N + 1);
  plan.add(st.inc, 2 * E);
  plan.add(st.meas, 6 * E);
  plan.add(st.r, 6 * E);
  plan.add(st.Ja, 36 * E);
  plan.add(st.Jb, 36 * E);
  plan.add(st.cost, E);
  plan.add(st.colsq, n);
  plan.add(st.scale, n);
  plan.add(st.H, st.h_elems);
  plan.add(st.g, n);
  plan.add(st.A, st.h_elems);
  plan.add(st.b, n);
  plan.add(st.gabs, n);
  plan.add(st.part, std::max(std::max(n, N), E));
  plan.add(st.part2, std::max(std::max(n, N), E));
  plan.add(st.scalars, 8);
  plan.add(st.flag, 2);
  plan.add(st.extra, st.extra_bytes);
  const bool weighted = st.edge_info && E > 0;
  plan.add(st.U, weighted ? 21 * E : 0);
  plan.add(st.wbad, weighted ? 1 : 0);
  if (st.arena.acquire(ctx, ArenaPolicy::OWNED, plan) != hipSuccess)
    return vsl_fail(ctx, VSL_ERR_NOMEM, "%s: device allocation of %zu bytes failed", st.who, plan.total());
  hipStream_t s = ctx->stream;
  if (N) VSL_HIP(ctx, hipMemcpyAsync(st.poses, p->poses, 56 * N, hipMemcpyHostToDevice, s));
  if (N) VSL_HIP(ctx, hipMemcpyAsync(st.free_idx, free_idx.data(), 4 * N, hipMemcpyHostToDevice, s));
  // incidence lists in edge order (a counting sort over the nodes keeps the edge indices ascending inside a list)
  std::vector<int> inc_off(N + 1, 0), inc(2 * E);
  for (size_t e = 0; e < E; e++) {
    inc_off[p->edge_a[e] + 1]++;
    inc_off[p->edge_b[e] + 1]++;
  }
  for (size_t i = 0; i < N; i++) inc_off[i + 1] += inc_off[i];
  {
    std::vector<int> cur(inc_off.begin(), inc_off.end() - 1);
    for (size_t e = 0; e < E; e++) {
      inc[cur[p->edge_a[e]]++] = 2 * (int)e;
      inc[cur[p->edge_b[e]]++] = 2 * (int)e + 1;
    }
  }
  VSL_HIP(ctx, hipMemcpyAsync(st.inc_off, inc_off.data(), 4 * (N + 1), hipMemcpyHostToDevice, s));
  if (E) VSL_HIP(ctx, hipMemcpyAsync(st.inc, inc.data(), 8 * E, hipMemcpyHostToDevice, s));
  if (E) {
    VSL_HIP(ctx, hipMemcpyAsync(st.edge_a, p->edge_a, 4 * E, hipMemcpyHostToDevice, s));
    VSL_HIP(ctx, hipMemcpyAsync(st.edge_b, p->edge_b, 4 * E, hipMemcpyHostToDevice, s));
    VSL_HIP(ctx, hipMemcpyAsync(st.meas, p->edge_meas, 48 * E, hipMemcpyHostToDevice, s));
  }
  static const int none = INT_MAX;  // (static: the asynchronous upload reads it after this function may have returned)
  int bad = none;
  if (weighted) {
    // Omega is staged in Ja (36 E doubles, written by the first linearisation only after this); U once per call
    VSL_HIP(ctx, hipMemcpyAsync(st.Ja, st.edge_info, 288 * E, hipMemcpyHostToDevice, s));
    VSL_HIP(ctx, hipMemcpyAsync(st.wbad, &none, 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pgo_edge_whiten_kernel, dim3((st.E + 63) / 64), dim3(64), 0, s, st.E, st.Ja, st.U, st.wbad);
    VSL_CHECK_LAUNCH(ctx);
    VSL_HIP(ctx, hipMemcpyAsync(&bad, st.wbad, 4, hipMemcpyDeviceToHost, s));
  } else {
    st.U = nullptr;  // (an empty arena slot still has an address)
  }
  if (st.far_on) {
    const PgfPlan& F = st.far;
    st.far_flags = (uint8_t*)(st.extra + F.off_far);
    st.far_list = (int*)(st.extra + F.off_far_edges);
    st.far_row_first = (int*)(st.extra + F.off_row_first);
    st.far_Linv = (double*)(st.extra + F.off_Linv);
    st.far_X = (double*)(st.extra + F.off_X);
    st.far_C = (double*)(st.extra + F.off_C);
    st.far_z = (double*)(st.extra + F.off_z);
    st.far_diag = (double*)(st.extra + F.off_diag);
    st.far_dfar = (double*)(st.extra + F.off_dfar);
    st.far_ok = (int*)(st.extra + F.off_flag);
    if (E) VSL_HIP(ctx, hipMemcpyAsync(st.far_flags, F.far.data(), E, hipMemcpyHostToDevice, s));
    if (F.k) VSL_HIP(ctx, hipMemcpyAsync(st.far_list, F.far_edges.data(), sizeof(int) * (size_t)F.k, hipMemcpyHostToDevice, s));
    VSL_HIP(ctx, hipMemcpyAsync(st.far_row_first, F.row_first.data(), sizeof(int) * (size_t)F.nblk, hipMemcpyHostToDevice, s));
  }
  VSL_HIP(ctx, hipStreamSynchronize(s));  // free_idx and the incidence lists are locals
  if (bad != none)
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: edge_info of edge %d is not positive definite (a pivot L_ii^2 <= 2^-36 Omega_ii, or not finite)", st.who, bad);
  return VSL_OK;
}

int pgo_linearize(vsl_ctx* ctx, PgoState& st, const vsl_ba_options* opt, bool first, double* cost_out) {
  hipStream_t s = ctx->stream;
  const int E = st.E, n = st.n;
  if (E > 0) {
    if (st.U)
      hipLaunchKernelGGL((pgo_linearize_kernel<true, true>), dim3((E + 63) / 64), dim3(64), 0, s, E, st.poses, st.edge_a, st.edge_b,
                         st.meas, st.U, opt->use_huber, opt->huber_parameter, st.r, st.Ja, st.Jb, st.cost);
    else
      hipLaunchKernelGGL((pgo_linearize_kernel<true, false>), dim3((E + 63) / 64), dim3(64), 0, s, E, st.poses, st.edge_a, st.edge_b,
                         st.meas, (const double*)nullptr, opt->use_huber, opt->huber_parameter, st.r, st.Ja, st.Jb, st.cost);
  }
  if (first && n > 0) {
    VSL_HIP(ctx, hipMemsetAsync(st.colsq, 0, 8 * (size_t)n, s));
    if (st.N > 0)
      hipLaunchKernelGGL(pgo_colsq_kernel, dim3((st.N * 6 + 255) / 256), dim3(256), 0, s, st.N, st.inc_off, st.inc, st.free_idx,
                         st.Ja, st.Jb, st.colsq);
    hipLaunchKernelGGL(pgo_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.colsq, st.scale);
  }
  if (n > 0) {
    VSL_HIP(ctx, hipMemsetAsync(st.H, 0, 8 * st.h_elems, s));
    VSL_HIP(ctx, hipMemsetAsync(st.g, 0, 8 * (size_t)n, s));
    if (st.N > 0)
      hipLaunchKernelGGL(pgo_build_kernel, dim3((st.N * 6 + 255) / 256), dim3(256), 0, s, st.N, n, st.inc_off, st.inc, st.edge_a,
                         st.edge_b, st.free_idx, st.r, st.Ja, st.Jb, st.scale, st.H, st.g, st.ld, st.bw, st.cyclic,
                         st.far_on ? (const uint8_t*)st.far_flags : (const uint8_t*)nullptr, st.far_on ? st.far_dfar : (double*)nullptr);
  }
  hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.cost, E, st.scalars, 0);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpyAsync(cost_out, st.scalars, 8, hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipStreamSynchronize(s));
  return VSL_OK;
}

int pgo_linearize_unit(vsl_ctx* ctx, PgoState& st, const vsl_ba_options* opt, double* cost_out) {
  if (st.n > 0) {
    // fill scale with ones by pretending every column norm is zero
    VSL_HIP(ctx, hipMemsetAsync(st.colsq, 0, 8 * (size_t)st.n, ctx->stream));
    hipLaunchKernelGGL(pgo_scale_kernel, dim3((st.n + 255) / 256), dim3(256), 0, ctx->stream, st.n, st.colsq, st.scale);
  }
  return pgo_linearize(ctx, st, opt, false, cost_out);
}

namespace {
// FAR EDGES: x = (M + W W^T)^-1 b, enqueued.  M: a band array (st.H or st.A, destroyed: M <- L), b and x: n doubles
// (may be the same).  pivot_test: diag M (st.far_diag, taken by the caller before this) against the factor by the
// 2^-36 rule of the covariance calls -- the undamped hook, where a singular M may pass the factorisation's own test on
// rounding noise.  st.flag is left 1 / 0 as a band solve leaves it.
int pgo_far_solve_enqueue(vsl_ctx* ctx, PgoState& st, double* M, const double* b, double* x, bool pivot_test) {
  hipStream_t s = ctx->stream;
  const int n = st.n, m = st.far.m, k = st.far.k, nblk = st.far.nblk;
  int rc;
  if ((rc = vsl_chol_factor_band_dev(ctx, M + st.ld, n, st.ld, st.bw, st.flag, st.far_Linv))) return rc;
  if (pivot_test && (rc = vsl_cov_band_pivot_dev(ctx, n, M, st.ld, st.far_diag, st.flag))) return rc;
  VSL_HIP(ctx, hipMemsetAsync(st.far_X, 0, sizeof(double) * (size_t)nblk * n * PGF_COLS, s));
  hipLaunchKernelGGL(pgo_far_columns_kernel, dim3((n + 72 * k + 255) / 256), dim3(256), 0, s, n, k, st.far_list, st.edge_a, st.edge_b,
                     st.free_idx, st.Ja, st.Jb, st.scale, b, st.far_X);
  if ((rc = vsl_band_rhs_solve_dev(ctx, n, M, st.ld, st.bw, st.far_Linv, st.far_row_first, nblk, st.far_X, st.flag))) return rc;
  static const int one = 1;  // (static: the asynchronous upload reads it after this function may have returned)
  VSL_HIP(ctx, hipMemcpyAsync(st.far_ok, &one, sizeof(int), hipMemcpyHostToDevice, s));
  if (m > 0) {
    hipLaunchKernelGGL(pgo_far_capacitance_kernel, dim3((unsigned)(((size_t)m * (m + 1) + 255) / 256)), dim3(256), 0, s, n, m,
                       st.far_list, st.edge_a, st.edge_b, st.free_idx, st.Ja, st.Jb, st.scale, st.far_X, st.far_C, st.far_z);
    if ((rc = vsl_chol_solve_dev(ctx, st.far_C, st.far_z, m, st.far_ok))) return rc;
  }
  hipLaunchKernelGGL(pgo_far_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, m, st.far_X, st.far_z, st.far_ok, x, st.flag);
  VSL_CHECK_LAUNCH(ctx);
  ctx->last_pgo_far_solves++;
  return VSL_OK;
}

// The band forms as a dense symmetric matrix (host): slot s of row i, s = 0 .. bw left of the diagonal, is entry
// (i, i - s); a column below zero is the wrap-around corner of the cyclic form, entry (i, i - s + n); every entry is
// mirrored.  Returns how many non-zero values lie where pgo_build_kernel writes nothing: the 32 padding slots left of
// each row's band, the trailing 64, and -- linear form -- the in-band slots of columns below zero.
int pgo_expand_band(const PgoState& st, const double* Hs, double* H) {
  const int n = st.n, ld = st.ld;
  int stray = 0;
  std::fill(H, H + (size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) {
    const double* row = Hs + (size_t)i * (ld + 1);
    for (int s = ld; s > st.bw; s--) stray += row[ld - s] != 0.0;
    for (int s = 0; s <= st.bw; s++) {
      int j = i - s;
      if (j < 0) {
        if (!st.cyclic) {
          stray += row[ld - s] != 0.0;
          continue;
        }
        j += n;
      }
      H[(size_t)i * n + j] = H[(size_t)j * n + i] = row[ld - s];
    }
  }
  for (size_t t = (size_t)n * (ld + 1); t < st.h_elems; t++) stray += Hs[t] != 0.0;
  return stray;
}

// the two test hooks: the normal equations at the given poses in the storage pgo_setup chose, returned dense
int pgo_linearize_hook(vsl_ctx* ctx, const char* who, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt, bool force_dense,
                       bool jacobi_scale, double* H, double* g, double* cost, int* n_free, int* storage, int* half_bandwidth,
                       int* stray_nonzeros) {
  int rc = pgo_validate(ctx, prob);
  if (rc) return rc;
  if (!opt) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: options are null", who);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  PgoState st;
  st.edge_info = edge_info;
  st.who = who;
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(prob, &nf);
  if ((rc = pgo_setup(ctx, prob, free_idx, nf, pgo_storage(ctx, prob, free_idx, nf, force_dense, false), st))) return rc;
  double c = 0;
  if ((rc = jacobi_scale ? pgo_linearize(ctx, st, opt, true, &c) : pgo_linearize_unit(ctx, st, opt, &c))) return rc;
  int stray = 0;
  if (H && st.n) {
    if (st.ld > 0) {
      std::vector<double> Hs(st.h_elems);
      VSL_HIP(ctx, hipMemcpy(Hs.data(), st.H, 8 * st.h_elems, hipMemcpyDeviceToHost));
      stray = pgo_expand_band(st, Hs.data(), H);
    } else {
      VSL_HIP(ctx, hipMemcpy(H, st.H, 8 * (size_t)st.n * st.n, hipMemcpyDeviceToHost));
    }
  }
  if (g && st.n) VSL_HIP(ctx, hipMemcpy(g, st.g, 8 * (size_t)st.n, hipMemcpyDeviceToHost));
  if (cost) *cost = c;
  if (n_free) *n_free = st.n / 6;
  if (storage) *storage = st.ld > 0 ? (st.cyclic ? 2 : 1) : 0;
  if (half_bandwidth) *half_bandwidth = st.ld > 0 ? st.bw : 0;
  if (stray_nonzeros) *stray_nonzeros = stray;
  return VSL_OK;
}

int pgo_optimize(vsl_ctx* ctx, const char* who, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                 vsl_ba_summary* summary) {
  int rc = pgo_validate(ctx, prob);
  if (rc) return rc;
  if (!opt) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: options are null", who);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  PgoState st;
  st.edge_info = edge_info;
  st.who = who;
  st.far_mode = pgo_far_switch(ctx) ? 1 : 0;
  ctx->last_pgo_far_taken = ctx->last_pgo_far_k = ctx->last_pgo_far_bw = ctx->last_pgo_far_cols = 0;
  ctx->last_pgo_far_solves = 0;
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(prob, &nf);
  if ((rc = pgo_setup(ctx, prob, free_idx, nf, pgo_storage(ctx, prob, free_idx, nf, false, false), st))) return rc;
  if (st.far_on) {
    ctx->last_pgo_far_taken = 1;
    ctx->last_pgo_far_k = st.far.k;
    ctx->last_pgo_far_bw = st.far.bw;
    ctx->last_pgo_far_cols = st.far.ncols;
  }
  hipStream_t s = ctx->stream;
  const int n = st.n, N = st.N, E = st.E;
  vsl_ba_summary sum;
  memset(&sum, 0, sizeof(sum));
  double cost = 0;
  if ((rc = pgo_linearize(ctx, st, opt, true, &cost))) return rc;
  sum.initial_cost = cost;
  LmState lm;
  double gmax = 1e300;
  int it = 0, term;
  bool need_gmax = true;
  while (true) {
    if (it >= opt->max_num_iterations) { sum.termination = 0; break; }
    if ((term = lm_gate(lm, need_gmax ? INFINITY : gmax)) >= 0) { sum.termination = term; break; }
    if (n == 0) { sum.termination = 2; break; }
    // damped system + gradient norm
    if (st.far_on)
      hipLaunchKernelGGL(pgo_damp_far_kernel, dim3((unsigned)((st.h_elems + 255) / 256)), dim3(256), 0, s, n, st.h_elems, st.ld,
                         st.H, st.far_dfar, st.g, st.scale, 1.0 / lm.radius, st.A, st.b, st.gabs);
    else if (st.ld > 0)
      hipLaunchKernelGGL(pgo_damp_band_kernel, dim3((unsigned)((st.h_elems + 255) / 256)), dim3(256), 0, s, n, st.h_elems, st.ld,
                         st.H, st.g, st.scale, 1.0 / lm.radius, st.A, st.b, st.gabs);
    else
      hipLaunchKernelGGL(pgo_damp_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, s, n, st.H, st.g, st.scale,
                         1.0 / lm.radius, st.A, st.b, st.gabs);
    const bool gmax_pending = need_gmax;
    if (need_gmax) {
      // max |gradient| of this linearisation: reduced here, READ with the step's scalars below (round 4: one host round
      // trip per iteration instead of three -- a gradient below tolerance is found one step late and that step is dropped)
      hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.gabs, n, st.scalars + 1, 1);
      need_gmax = false;
    }
    it++;
    if (st.far_on)
      rc = pgo_far_solve_enqueue(ctx, st, st.A, st.b, st.b, false);
    else if (st.ld > 0)
      rc = vsl_chol_solve_band_dev(ctx, st.A + st.ld, st.b, n, st.ld, st.bw, st.flag, st.cyclic);
    else
      rc = vsl_chol_solve_dev(ctx, st.A, st.b, n, st.flag);
    if (rc) return rc;
    // (the factorisation leaves flag = 1 on success, 0 on a bad pivot; the kernels below only ever CLEAR it -- on a
    // non-finite step --, so one read at the end tells both; after a failed factorisation they run on numbers nobody uses)
    double sc[6] = {0, 0, 0, 0, 0, 0};  // |g| max | model (gradient part in band form) | step^2 | x^2 | candidate cost | band form: sum |J S d|^2 / 2
    int finite = 1;
    {
      if (st.ld > 0) {
        // model change = sum_i -d_i g_i - sum_e |J_e S d|^2 / 2 (no product with H: the band keeps one triangle only)
        hipLaunchKernelGGL(pgo_model_edges_kernel, dim3((E + 255) / 256 > 0 ? (E + 255) / 256 : 1), dim3(256), 0, s, E, st.edge_a,
                           st.edge_b, st.free_idx, st.Ja, st.Jb, st.scale, st.b, st.part2);
        hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.part2, E, st.scalars + 6, 0);
        hipLaunchKernelGGL(pgo_model_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.g, st.b, st.part, st.flag);
      } else {
        hipLaunchKernelGGL(pgo_model_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.H, st.g, st.b, st.part, st.flag);
      }
      hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.part, n, st.scalars + 2, 0);
      hipLaunchKernelGGL(pgo_update_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, st.free_idx, st.poses, st.b, st.scale,
                         st.cand, st.part, st.part2);
      hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.part, N, st.scalars + 3, 0);
      hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.part2, N, st.scalars + 4, 0);
      if (E > 0) {
        if (st.U)
          hipLaunchKernelGGL((pgo_linearize_kernel<false, true>), dim3((E + 63) / 64), dim3(64), 0, s, E, st.cand, st.edge_a,
                             st.edge_b, st.meas, st.U, opt->use_huber, opt->huber_parameter, (double*)nullptr, (double*)nullptr,
                             (double*)nullptr, st.cost);
        else
          hipLaunchKernelGGL((pgo_linearize_kernel<false, false>), dim3((E + 63) / 64), dim3(64), 0, s, E, st.cand, st.edge_a,
                             st.edge_b, st.meas, (const double*)nullptr, opt->use_huber, opt->huber_parameter, (double*)nullptr,
                             (double*)nullptr, (double*)nullptr, st.cost);
      }
      hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, s, st.cost, E, st.scalars + 5, 0);
      VSL_CHECK_LAUNCH(ctx);
      VSL_HIP(ctx, hipMemcpyAsync(sc, st.scalars + 1, 48, hipMemcpyDeviceToHost, s));
      VSL_HIP(ctx, hipMemcpyAsync(&finite, st.flag, 4, hipMemcpyDeviceToHost, s));
      VSL_HIP(ctx, hipStreamSynchronize(s));
    }
    if (gmax_pending) {
      gmax = sc[0];
      if (gmax <= LM_GRADIENT_TOLERANCE) {  // lm_gate's first test, one step late
        it--;
        sum.termination = 2;
        break;
      }
    }
    if (st.ld > 0) sc[1] -= sc[5];
    const double model = sc[1], step_norm = sqrt(sc[2]), x_norm = sqrt(sc[3]), cand_cost = sc[4];
    const double radius_used = lm.radius;
    LmInfo info;
    const int verdict = lm_judge(lm, finite != 0 && model > 0.0, cost, cand_cost, model, step_norm, x_norm, &info);
    if (verdict >= 0) { sum.termination = verdict; break; }
    if (verdict == LM_INVALID) continue;
    if (opt->verbosity >= 2) fprintf(stderr, "pgo %3d cost %.6e change %.3e |g| %.3e step %.3e rho %.3e radius %.3e\n", it, cand_cost, info.cost_change, gmax, step_norm, info.rel, radius_used);
    if (verdict == LM_ACCEPTED) {
      std::swap(st.poses, st.cand);
      if ((rc = pgo_linearize(ctx, st, opt, false, &cost))) return rc;  // (the accepted point's cost comes from here)
      need_gmax = true;
      sum.successful_steps++;
    }
  }
  sum.iterations = it;
  sum.final_cost = cost;
  if (N) VSL_HIP(ctx, hipMemcpy(prob->poses, st.poses, 56 * (size_t)N, hipMemcpyDeviceToHost));
  if (opt->verbosity >= 1)
    fprintf(stderr, "vsl PGO: iterations %d, initial cost %.6e, final cost %.6e, termination %d\n", sum.iterations, sum.initial_cost,
            sum.final_cost, sum.termination);
  if (summary) *summary = sum;
  return VSL_OK;
}
}  // namespace

// H (n x n row-major, n = 6 x free nodes in node order), g and cost of the robustified problem at the given
// poses, unscaled -- the test hook next to orc_pgo_linearize.
extern "C" int vsl_pgo_linearize(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, double* H, double* g,
                                 double* cost, int* n_free) {
  return pgo_linearize_hook(ctx, "vsl_pgo_linearize", prob, nullptr, opt, true, false, H, g, cost, n_free, nullptr, nullptr, nullptr);
}
// ... of the weighted problem (edge_info: [n_edges][36], Omega_e row-major; NULL: the call above)
extern "C" int vsl_pgo_linearize_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                   double* H, double* g, double* cost, int* n_free) {
  return pgo_linearize_hook(ctx, "vsl_pgo_linearize_w", prob, edge_info, opt, true, false, H, g, cost, n_free, nullptr, nullptr, nullptr);
}

// The same in the storage vsl_pose_graph_optimize takes for this graph (dense, band or cyclic band: H is expanded on the
// host), with the Jacobi scale of the solver's first linearisation when jacobi_scale is set.
extern "C" int vsl_pgo_linearize_stored(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, int jacobi_scale,
                                        double* H, double* g, double* cost, int* n_free, int* storage, int* half_bandwidth,
                                        int* stray_nonzeros) {
  return pgo_linearize_hook(ctx, "vsl_pgo_linearize_stored", prob, nullptr, opt, false, jacobi_scale != 0, H, g, cost, n_free,
                            storage, half_bandwidth, stray_nonzeros);
}
extern "C" int vsl_pgo_linearize_stored_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                          int jacobi_scale, double* H, double* g, double* cost, int* n_free, int* storage,
                                          int* half_bandwidth, int* stray_nonzeros) {
  return pgo_linearize_hook(ctx, "vsl_pgo_linearize_stored_w", prob, edge_info, opt, false, jacobi_scale != 0, H, g, cost, n_free,
                            storage, half_bandwidth, stray_nonzeros);
}

// The parity hook of the far-edge route (include/vslam_hip.h): H x = b for the H, g of vsl_pgo_linearize_w through the
// band factor of the near edges and the low-rank update of the far ones, at every size.
extern "C" int vsl_pgo_far_solve(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                 const double* b, int max_near_distance, double* x, int* far_edges, int* half_bandwidth) {
  int rc = pgo_validate(ctx, prob);
  if (rc) return rc;
  if (!opt || !x) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_pgo_far_solve: options or x are null");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  PgoState st;
  st.edge_info = edge_info;
  st.who = "vsl_pgo_far_solve";
  st.far_mode = 2;
  st.far_max_near = max_near_distance < 0 ? -1 : max_near_distance;
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(prob, &nf);
  if ((rc = pgo_setup(ctx, prob, free_idx, nf, pgo_storage(ctx, prob, free_idx, nf, false, false), st))) return rc;
  hipStream_t s = ctx->stream;
  const int n = st.n;
  if (far_edges) *far_edges = st.far.k;
  if (half_bandwidth) *half_bandwidth = st.far.bw;
  double cost = 0;
  if ((rc = pgo_linearize_unit(ctx, st, opt, &cost))) return rc;
  if (b)
    VSL_HIP(ctx, hipMemcpyAsync(st.b, b, 8 * (size_t)n, hipMemcpyHostToDevice, s));
  else
    VSL_HIP(ctx, hipMemcpyAsync(st.b, st.g, 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
  if ((rc = vsl_cov_diag_dev(ctx, n, st.H, st.ld, st.far_diag))) return rc;
  rc = pgo_far_solve_enqueue(ctx, st, st.H, st.b, st.b, true);
  int ok = 0;
  if (rc == VSL_OK) {
    hipError_t e = hipMemcpyAsync(x, st.b, 8 * (size_t)n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&ok, st.flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = vsl_fail(ctx, VSL_ERR_HIP, "vsl_pgo_far_solve: copy back -> %s", hipGetErrorString(e));
  }
  VSL_HIP(ctx, hipStreamSynchronize(s));  // (also on an error: queued copies read b)
  if (rc) return rc;
  if (!ok) {
    std::fill(x, x + n, 0.0);
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_pgo_far_solve: the band of the near edges or the capacitance matrix is not positive definite (no fixed node, or a near component without one)");
  }
  return VSL_OK;
}

extern "C" int vsl_pose_graph_optimize(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, vsl_ba_summary* summary) {
  return pgo_optimize(ctx, "vsl_pose_graph_optimize", prob, nullptr, opt, summary);
}
// the cost is sum rho(r^T Omega_e r) / 2: Huber on the whitened squared norm (edge_info NULL: the call above)
extern "C" int vsl_pose_graph_optimize_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                         vsl_ba_summary* summary) {
  return pgo_optimize(ctx, "vsl_pose_graph_optimize_w", prob, edge_info, opt, summary);
}
