// pgo.hip -- pose graph optimisation: the numerical core of
// visnav::pose_graph_optimization (include/visnav/loop_closure_utils.h:446-587).  Residual blocks
//     r = log(T_w_c^-1 * T_w_n) - upsilon_omega                  (PoseGraphRelativePoseCostFunctor, reprojection.h:107-126)
// on SE3 blocks with the tangent parameterisation T * exp(delta) (local_parameterization_se3.hpp:43-63),
// HuberLoss, Levenberg-Marquardt with the [upstream] Ceres policy restated for bundle adjustment in ba.hip.
//
// One thread per edge evaluates the residual and both 6x6 Jacobian blocks with forward-mode dual numbers
// (12 partials: what ceres::AutoDiffCostFunction<., 6, 7, 7> followed by the SE3 plus-Jacobian computes), the
// normal equations are accumulated by row owners -- one thread owns one ROW of H and walks the node's incident edges in
// edge order (lists built once per solve on the host): no atomics, results do not depend on timing -- into the storage
// pgo_storage picks for the graph: a linear or cyclic band when the graph is narrow in the keyframes' own order (chol.hip's
// band and ring solvers), dense otherwise (the blocked Cholesky), and, opt-in, a band for the near edges plus a low-rank
// update for a few far ones where one long edge would otherwise make the whole matrix dense ("FAR EDGES" below,
// pgo_far_plan.h).  This runs once per loop closure.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "vsl_common.h"
#include "lm_policy.h"
#include "dev_arena.h"
#include "pgo_cov_plan.h"
#include "pgo_far_plan.h"
#include "relpose_math.h"

namespace {

struct D12 {
  double v;
  double d[12];
};
__device__ __forceinline__ D12 mk(double x) {
  D12 r;
  r.v = x;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = 0.0;
  return r;
}
__device__ __forceinline__ D12 operator+(const D12& a, const D12& b) {
  D12 r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] + b.d[i];
  return r;
}
__device__ __forceinline__ D12 operator-(const D12& a, const D12& b) {
  D12 r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] - b.d[i];
  return r;
}
__device__ __forceinline__ D12 operator-(const D12& a) {
  D12 r;
  r.v = -a.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = -a.d[i];
  return r;
}
__device__ __forceinline__ D12 operator*(const D12& a, const D12& b) {
  D12 r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
__device__ __forceinline__ D12 operator/(const D12& a, const D12& b) {
  D12 r;
  const double inv = 1.0 / b.v;
  r.v = a.v * inv;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
__device__ __forceinline__ D12 dsqrt(const D12& a) {
  D12 r;
  r.v = sqrt(a.v);
  const double k = 0.5 / r.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] * k;
  return r;
}
__device__ __forceinline__ D12 datan2(const D12& y, const D12& x) {
  D12 r;
  r.v = atan2(y.v, x.v);
  const double den = 1.0 / (x.v * x.v + y.v * y.v);
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = (x.v * y.d[i] - y.v * x.d[i]) * den;
  return r;
}
__device__ __forceinline__ D12 dsin(const D12& a) {
  D12 r;
  r.v = sin(a.v);
  const double c = cos(a.v);
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = c * a.d[i];
  return r;
}
__device__ __forceinline__ D12 dcos(const D12& a) {
  D12 r;
  r.v = cos(a.v);
  const double s = -sin(a.v);
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = s * a.d[i];
  return r;
}
__device__ __forceinline__ double dsqrt(double a) { return sqrt(a); }
__device__ __forceinline__ double datan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ double dsin(double a) { return sin(a); }
__device__ __forceinline__ double dcos(double a) { return cos(a); }
__device__ __forceinline__ double val(double a) { return a; }
__device__ __forceinline__ double val(const D12& a) { return a.v; }
__device__ __forceinline__ double lift(double, double x) { return x; }
__device__ __forceinline__ D12 lift(const D12&, double x) { return mk(x); }

template <class T>
__device__ void qmul(const T* a, const T* b, T* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
template <class T>
__device__ void qrot(const T* q, const T* p, T* o) {
  T uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
  const T c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) o[i] = p[i] + q[3] * uv[i] + c[i];
}

// Sophus::SE3::log of (q, t): out = (upsilon, omega)   (so3.hpp logAndTheta, se3.hpp log)
template <class T>
__device__ void se3_log(const T* q, const T* t, T* out) {
  const T sq_n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
  const T w = q[3];
  T two_atan, c;
  if (val(sq_n) < 1e-20) {
    two_atan = lift(w, 2.0) / w - lift(w, 2.0 / 3.0) * sq_n / (w * w * w);
    c = lift(w, 1.0 / 12.0);
  } else {
    const T n = dsqrt(sq_n);
    const T half = val(w) < 0 ? datan2(-n, -w) : datan2(n, w);
    two_atan = lift(w, 2.0) * half / n;
    const T theta = two_atan * n;
    if (fabs(val(theta)) < 1e-6) {
      c = lift(w, 1.0 / 12.0);
    } else {
      const T ht = lift(w, 0.5) * theta;
      c = (lift(w, 1.0) - theta * dcos(ht) / (lift(w, 2.0) * dsin(ht))) / (theta * theta);
    }
  }
  const T om[3] = {two_atan * q[0], two_atan * q[1], two_atan * q[2]};
  const T a[3] = {om[1] * t[2] - om[2] * t[1], om[2] * t[0] - om[0] * t[2], om[0] * t[1] - om[1] * t[0]};
  const T b[3] = {om[1] * a[2] - om[2] * a[1], om[2] * a[0] - om[0] * a[2], om[0] * a[1] - om[1] * a[0]};
  for (int i = 0; i < 3; i++) {
    out[i] = t[i] - lift(w, 0.5) * a[i] + c * b[i];
    out[3 + i] = om[i];
  }
}

template <class T>
__device__ void edge_residual(const T* qc, const T* tc, const T* qn, const T* tn, const double* meas, T* r) {
  const T qci[4] = {-qc[0], -qc[1], -qc[2], qc[3]};
  T q[4], dt[3], t[3];
  qmul(qci, qn, q);
  for (int i = 0; i < 3; i++) dt[i] = tn[i] - tc[i];
  qrot(qci, dt, t);
  T lg[6];
  se3_log(q, t, lg);
  for (int i = 0; i < 6; i++) r[i] = lg[i] - lift(q[3], meas[i]);
}

// T exp(delta) to first order in dual arithmetic: q' = q (x) (omega / 2, 1), t' = t + R upsilon
__device__ void seed_pose(const double* p7, int first, D12* q, D12* t) {
  for (int i = 0; i < 4; i++) q[i] = mk(p7[i]);
  for (int i = 0; i < 3; i++) t[i] = mk(p7[4 + i]);
  for (int k = 0; k < 3; k++) {
    double e[3] = {0, 0, 0}, re[3];
    e[k] = 1.0;
    qrot(p7, e, re);
    for (int i = 0; i < 3; i++) t[i].d[first + k] = re[i];
    const double w[4] = {0.5 * e[0], 0.5 * e[1], 0.5 * e[2], 0.0};
    double qq[4];
    qmul(p7, w, qq);
    for (int i = 0; i < 4; i++) q[i].d[first + 3 + k] = qq[i];
  }
}

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

static int pgo_validate(vsl_ctx* ctx, const vsl_pgo_problem* p) {
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
struct PgoState {
  int N = 0, E = 0, n = 0;
  // storage of the normal equations: dense (ld = 0) or, when the graph is narrow in the nodes' own order (keyframes in
  // time order: odometry + covisibility edges, and the loop edge that closes the ring), lower band storage -- linear or
  // CYCLIC (the band closes on itself; chol.hip's ring solver) -- with ld = bw + 32 slots left of the diagonal
  int ld = 0, bw = 0, cyclic = 0;
  size_t h_elems = 0;
  bool force_dense = false;
  bool linear_only = false;  // vsl_pgo_covariance on a folded ring: the relabelled graph is a linear band, never a ring again
  size_t extra_bytes = 0;    // the caller's share of the arena (vsl_pgo_covariance: factor scratch, columns, blocks)
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

// the switch of the far-edge route: diagnostic "pgo_far_edges" or the environment variable VSL_PGO_FAR_EDGES
bool pgo_far_switch(const vsl_ctx* ctx) {
  static const bool env_on = getenv("VSL_PGO_FAR_EDGES") != nullptr;
  return ctx->pgo_far_edges || env_on;
}

// THE storage decision of a graph (host only): dense, linear band or cyclic band -- st.ld / bw / cyclic / h_elems from
// st.n = 6 nf unknowns and the edges' distances in free indices.  pgo_setup and vsl_pgo_covariance ask it.
void pgo_storage(vsl_ctx* ctx, const vsl_pgo_problem* p, const std::vector<int>& free_idx, int nf, PgoState& st) {
  st.N = p->n_nodes;
  st.E = p->n_edges;
  st.n = 6 * nf;
  st.cyclic = 0;
  st.bw = 0;
  {
    int lin = 0, cyc = 0;
    for (int e = 0; e < st.E; e++) {
      const int fa = free_idx[p->edge_a[e]], fb = free_idx[p->edge_b[e]];
      if (fa < 0 || fb < 0) continue;
      const int d = std::abs(fa - fb);
      lin = std::max(lin, d);
      cyc = std::max(cyc, std::min(d, nf - d));
    }
    const int bw_lin = 6 * lin + 5, bw_cyc = 6 * cyc + 5;
    int Bc = 0, nc = 0;
    static const bool env_dense = getenv("VSL_PGO_DENSE") != nullptr;
    st.ld = 0;
    st.h_elems = (size_t)st.n * st.n;
    if (!st.force_dense && !env_dense && !ctx->ba_force_dense && st.n > 128) {
      if (!st.linear_only && 2 * bw_cyc < bw_lin && chol_ring_available(st.n, bw_cyc, CholSwitches{ctx->chol_no_fused, ctx->chol_no_bcr, ctx->chol_one_ended}, &Bc, &nc)) {
        st.cyclic = 1;
        st.bw = bw_cyc;
      } else if ((size_t)(bw_lin + 33) * 2 < (size_t)st.n) {
        st.cyclic = 0;
        st.bw = bw_lin;
      } else {
        st.bw = 0;
      }
      if (st.bw > 0) {
        st.ld = st.bw + 32;
        st.h_elems = (size_t)st.n * (st.ld + 1) + 64;
      }
    }
  }
}

std::vector<int> pgo_free_index(const vsl_pgo_problem* p, int* nf_out) {
  std::vector<int> free_idx(p->n_nodes, -1);
  int nf = 0;
  for (int i = 0; i < p->n_nodes; i++)
    if (!p->node_fixed[i]) free_idx[i] = nf++;
  *nf_out = nf;
  return free_idx;
}

int pgo_setup(vsl_ctx* ctx, const vsl_pgo_problem* p, PgoState& st) {
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(p, &nf);
  pgo_storage(ctx, p, free_idx, nf, st);
  if (st.far_mode == 1) {
    // dense by pgo_storage's own rule (not by a diagnostic that asks for dense), and a split exists
    static const bool env_dense = getenv("VSL_PGO_DENSE") != nullptr;
    if (st.ld == 0 && st.n > 128 && !st.force_dense && !env_dense && !ctx->ba_force_dense) {
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

// residuals + Jacobians at st.poses, optional (re)build of the scaled normal equations; *cost_out = total cost
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
  st.force_dense = force_dense;
  st.edge_info = edge_info;
  st.who = who;
  if ((rc = pgo_setup(ctx, prob, st))) return rc;
  // unit scaling: fill scale with ones by pretending every column norm is zero
  if (!jacobi_scale && st.n > 0) {
    VSL_HIP(ctx, hipMemsetAsync(st.colsq, 0, 8 * (size_t)st.n, ctx->stream));
    hipLaunchKernelGGL(pgo_scale_kernel, dim3((st.n + 255) / 256), dim3(256), 0, ctx->stream, st.n, st.colsq, st.scale);
  }
  double c = 0;
  if ((rc = pgo_linearize(ctx, st, opt, jacobi_scale, &c))) return rc;
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

namespace {
__global__ void pgo_cov_diag_kernel(int n, const double* __restrict__ H, int ld, double* __restrict__ d);  // (the covariance section)
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
  if ((rc = pgo_setup(ctx, prob, st))) return rc;
  hipStream_t s = ctx->stream;
  const int n = st.n;
  if (far_edges) *far_edges = st.far.k;
  if (half_bandwidth) *half_bandwidth = st.far.bw;
  // unit scale, one linearisation at the poses as they are (vsl_pgo_covariance's)
  VSL_HIP(ctx, hipMemsetAsync(st.colsq, 0, 8 * (size_t)n, s));
  hipLaunchKernelGGL(pgo_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.colsq, st.scale);
  double cost = 0;
  if ((rc = pgo_linearize(ctx, st, opt, false, &cost))) return rc;
  if (b)
    VSL_HIP(ctx, hipMemcpyAsync(st.b, b, 8 * (size_t)n, hipMemcpyHostToDevice, s));
  else
    VSL_HIP(ctx, hipMemcpyAsync(st.b, st.g, 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(pgo_cov_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.H, st.ld, st.far_diag);
  VSL_CHECK_LAUNCH(ctx);
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

namespace {
int pgo_optimize(vsl_ctx* ctx, const char* who, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                 vsl_ba_summary* summary);
}
extern "C" int vsl_pose_graph_optimize(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, vsl_ba_summary* summary) {
  return pgo_optimize(ctx, "vsl_pose_graph_optimize", prob, nullptr, opt, summary);
}
// the cost is sum rho(r^T Omega_e r) / 2: Huber on the whitened squared norm (edge_info NULL: the call above)
extern "C" int vsl_pose_graph_optimize_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                         vsl_ba_summary* summary) {
  return pgo_optimize(ctx, "vsl_pose_graph_optimize_w", prob, edge_info, opt, summary);
}
namespace {
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
  if ((rc = pgo_setup(ctx, prob, st))) return rc;
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

// ---------------------------------------------------------------------------------------------------------------
// vsl_pgo_covariance: the 6 x 6 diagonal blocks of H^-1, H = J^T J of one linearisation at the poses handed in (unit
// scale, no damping: what vsl_pgo_linearize returns).  Three routes, chosen by pgo_storage as for the solve:
//   0 dense        vsl_chol_factor_dev, then one solve per queried unit column (ba_cov.hip's kernel) -- O(n^2) per column
//   1 linear band  vsl_chol_selinv_band_dev (chol.hip "SELECTED INVERSION"): the whole band of H^-1 in O(n bw^2); the
//                  diagonal blocks lie inside it (bw >= 5)
//   2 ring         the FREE nodes are relabelled by the fold of chol_plan.h on the host -- free index f becomes
//                  chol_fold_pos(nf, f), the edges follow, the edge ORDER stays -- so that the ring is a linear band of at
//                  most twice the node distance; pgo_build_kernel builds that band as for any graph, then route 1.  A
//                  diagonal block of the inverse does not move under a relabelling of the nodes.
// "Not positive definite" is the rule of ba_cov.hip on every route: a pivot L_ii^2 <= 2^-36 H_ii, diag H taken before
// the factorisation.  A block depends on H alone, never on what else is queried; the band routes read the lower
// triangle of a block and mirror it, the dense route averages the two mirror entries: exactly symmetric either way.
namespace {

// H: the storage as pgo_build_kernel filled it (ld = 0: dense n x n; else rows of ld + 1 slots, the diagonal last)
__global__ void pgo_cov_diag_kernel(int n, const double* __restrict__ H, int ld, double* __restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = ld > 0 ? H[(size_t)i * (ld + 1) + ld] : H[(size_t)i * n + i];
}

// (band routes: the pivot test and the blocks are ba_cov.hip's, vsl_cov_band_pivot_dev / vsl_cov_band_blocks_dev)

// dense route: the diagonal block of X (right-hand sides 6 q .. 6 q + 5 belong to q_free[q]), symmetrised
__global__ void pgo_cov_blocks_dense_kernel(int n, int nQ, const int* __restrict__ q_free, const double* __restrict__ X,
                                            const int* __restrict__ ok, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * nQ || !*ok) return;
  const int q = t / 36, a = (t % 36) / 6, b = t % 6, c = q_free[q];
  out[t] = 0.5 * (X[vsl_cov_x_at(n, 6 * c + a, 6 * q + b)] + X[vsl_cov_x_at(n, 6 * c + b, 6 * q + a)]);
}

inline size_t pgc_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

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

// q_free: the unique queried nodes as free indices of `prob` (the folded graph on route 2), ascending.  q_free, col_unk
// and blocks are read / written by copies on the stream: the caller keeps them until it has synchronised.
int pgo_cov_run(vsl_ctx* ctx, const char* who, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt, bool linear_only,
                const std::vector<int>& q_free, std::vector<int>& col_unk, std::vector<double>& blocks, int* route) {
  const int nQ = (int)q_free.size();
  int nf = 0;
  for (int i = 0; i < prob->n_nodes; i++) nf += !prob->node_fixed[i];
  const int n = 6 * nf, m = 6 * nQ, nblk = (m + 15) / 16;
  PgoState st;
  st.linear_only = linear_only;
  st.edge_info = edge_info;
  st.who = who;
  {
    // the decision is needed before the arena is sized: the dense route keeps its columns there
    PgoState probe;
    probe.linear_only = linear_only;
    int nf2 = 0;
    pgo_storage(ctx, prob, pgo_free_index(prob, &nf2), nf, probe);
    const bool dense = probe.ld == 0;
    size_t at = 0;
    at += pgc_pad(sizeof(double) * (size_t)n);                                                                   // diag H
    at += pgc_pad(sizeof(int) * (size_t)nQ);                                                                     // q_free
    at += pgc_pad(sizeof(double) * 36 * (size_t)nQ);                                                             // blocks
    if (dense) {
      at += pgc_pad(sizeof(double) * (size_t)((n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB);  // Linv
      at += pgc_pad(sizeof(int) * (size_t)nblk * 16);                                                            // unit columns
      at += pgc_pad(sizeof(double) * (size_t)nblk * n * 16);                                                     // X
    }
    st.extra_bytes = at;
  }
  int rc;
  if ((rc = pgo_setup(ctx, prob, st))) return rc;
  hipStream_t s = ctx->stream;
  const bool dense = st.ld == 0;
  *route = dense ? 0 : 1;
  char* x = st.extra;
  double* Hdiag = (double*)x;
  x += pgc_pad(sizeof(double) * (size_t)n);
  int* q_dev = (int*)x;
  x += pgc_pad(sizeof(int) * (size_t)nQ);
  double* out = (double*)x;
  x += pgc_pad(sizeof(double) * 36 * (size_t)nQ);
  // unit scale (the solver's Jacobi scale is not part of H), one linearisation at the poses as they are
  VSL_HIP(ctx, hipMemsetAsync(st.colsq, 0, 8 * (size_t)n, s));
  hipLaunchKernelGGL(pgo_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.colsq, st.scale);
  double cost = 0;
  if ((rc = pgo_linearize(ctx, st, opt, false, &cost))) return rc;
  VSL_HIP(ctx, hipMemcpyAsync(q_dev, q_free.data(), sizeof(int) * (size_t)nQ, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(pgo_cov_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.H, st.ld, Hdiag);
  VSL_CHECK_LAUNCH(ctx);
  if (dense) {
    double* Linv = (double*)x;
    x += pgc_pad(sizeof(double) * (size_t)((n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB);
    int* col_dev = (int*)x;
    x += pgc_pad(sizeof(int) * (size_t)nblk * 16);
    double* X = (double*)x;
    col_unk.assign((size_t)nblk * 16, -1);
    for (int j = 0; j < m; j++) col_unk[j] = 6 * q_free[j / 6] + j % 6;
    VSL_HIP(ctx, hipMemcpyAsync(col_dev, col_unk.data(), sizeof(int) * col_unk.size(), hipMemcpyHostToDevice, s));
    if ((rc = vsl_chol_factor_dev(ctx, st.H, n, st.flag, Linv))) return rc;
    if ((rc = vsl_cov_unit_columns_dev(ctx, n, st.H, Linv, Hdiag, col_dev, nblk, X, st.flag))) return rc;
    hipLaunchKernelGGL(pgo_cov_blocks_dense_kernel, dim3((36 * nQ + 255) / 256), dim3(256), 0, s, n, nQ, q_dev, X, st.flag, out);
  } else {
    // st.A: the second band array of the solve, here the band of the inverse
    if ((rc = vsl_chol_selinv_band_dev(ctx, st.H + st.ld, st.A + st.ld, n, st.ld, st.bw, st.flag))) return rc;
    if ((rc = vsl_cov_band_pivot_dev(ctx, n, st.H, st.ld, Hdiag, st.flag))) return rc;
    if ((rc = vsl_cov_band_blocks_dev(ctx, nQ, q_dev, st.A, st.ld, st.flag, out))) return rc;
  }
  VSL_CHECK_LAUNCH(ctx);
  int ok = 0;
  blocks.assign(36 * (size_t)nQ, 0.0);
  VSL_HIP(ctx, hipMemcpyAsync(blocks.data(), out, sizeof(double) * blocks.size(), hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipMemcpyAsync(&ok, st.flag, sizeof(int), hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipStreamSynchronize(s));
  if (!ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: the normal equations are not positive definite (no fixed node, or a free node without an edge)", who);
  return VSL_OK;
}
}  // namespace

namespace {
int pgo_covariance(vsl_ctx* ctx, const char* who, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                   const int32_t* nodes, int n_q, double* cov, int* storage);
}
extern "C" int vsl_pgo_covariance(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const int32_t* nodes, int n_q,
                                  double* cov, int* storage) {
  return pgo_covariance(ctx, "vsl_pgo_covariance", prob, nullptr, opt, nodes, n_q, cov, storage);
}
// H of the weighted problem (the fold keeps the edge order: edge_info follows the edges as it is)
extern "C" int vsl_pgo_covariance_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                    const int32_t* nodes, int n_q, double* cov, int* storage) {
  return pgo_covariance(ctx, "vsl_pgo_covariance_w", prob, edge_info, opt, nodes, n_q, cov, storage);
}
namespace {
int pgo_covariance(vsl_ctx* ctx, const char* who, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                   const int32_t* nodes, int n_q, double* cov, int* storage) {
  int rc = pgo_validate(ctx, prob);
  if (rc) return rc;
  if (!opt || n_q < 0 || (n_q > 0 && (!nodes || !cov)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null argument or negative count", who);
  for (int q = 0; q < n_q; q++) {
    if (nodes[q] < 0 || nodes[q] >= prob->n_nodes) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: node %d out of range", who, nodes[q]);
    if (prob->node_fixed[nodes[q]]) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: node %d is fixed", who, nodes[q]);
  }
  // the route of this graph: the solve's own decision, on the host
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(prob, &nf);
  int route;
  {
    PgoState probe;
    pgo_storage(ctx, prob, free_idx, nf, probe);
    route = probe.ld > 0 ? (probe.cyclic ? 2 : 1) : 0;
  }
  if (storage) *storage = route;
  if (n_q == 0) return VSL_OK;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  // the unique queried nodes, ascending in the free index the device will see
  std::vector<int> key(n_q), q_free, slot(n_q);
  for (int q = 0; q < n_q; q++) key[q] = route == 2 ? chol_fold_pos(nf, free_idx[nodes[q]]) : free_idx[nodes[q]];
  q_free = key;
  std::sort(q_free.begin(), q_free.end());
  q_free.erase(std::unique(q_free.begin(), q_free.end()), q_free.end());
  for (int q = 0; q < n_q; q++) slot[q] = (int)(std::lower_bound(q_free.begin(), q_free.end(), key[q]) - q_free.begin());
  std::vector<double> blocks;
  std::vector<int> col_unk;
  int ran = 0;
  if (route == 2) {
    PgoFolded F;
    pgo_fold_problem(prob, free_idx, nf, F);
    rc = pgo_cov_run(ctx, who, &F.prob, edge_info, opt, true, q_free, col_unk, blocks, &ran);
    if (rc == VSL_OK && ran == 1) ran = 2;
  } else {
    rc = pgo_cov_run(ctx, who, prob, edge_info, opt, false, q_free, col_unk, blocks, &ran);
  }
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);  // queued copies read host buffers that end here
    return rc;
  }
  if (storage) *storage = ran;
  for (int q = 0; q < n_q; q++) memcpy(cov + 36 * (size_t)q, blocks.data() + 36 * (size_t)slot[q], 36 * sizeof(double));
  return VSL_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// vsl_pgo_joint_covariance / vsl_pgo_edge_consistency: the 12 x 12 joint covariance of pairs of nodes and, on top of it,
// the covariance and the chi-square of a candidate edge's residual (include/vslam_hip.h has the definitions).  The
// host plan -- validation, the fold, the class of each pair, the column nodes, the arena -- is pgo_cov_plan.h.  The
// chain is vsl_pgo_covariance's up to the inverse, then
//   route 0     unit columns of every distinct queried free node (ba_cov.hip's dense solve)
//   routes 1, 2 selected inversion and pivot test; for the PGC_SOLVE pairs the band unit-column solve
//               (vsl_cov_band_unit_columns_dev) with the inverted diagonal blocks the inversion left in its scratch
//   pgo_joint_blocks_kernel       one thread per entry of a 12 x 12 block
//   pgo_edge_consistency_kernel   one wavefront per candidate (the edge call only)
// vsl_pgo_covariance and the solver are not touched by any of it.
namespace {

// One entry per thread.  Diagonal blocks: the rule of vsl_pgo_covariance on the same route, bit for bit (band: entry
// (max, min) of Z; dense: the two mirror entries of the node's own columns averaged).  Cross block, entry (row r of node
// x, column c of node y): with columns for both nodes the average of X_y[6 x + r][c] and X_x[6 y + c][r]; with columns
// for one of them that single entry; with none entry (max, min) of Z.  Every rule gives (x, r; y, c) and (y, c; x, r)
// the same number: the block is symmetric and a swapped pair is the swapped, transposed block.
__global__ void pgo_joint_blocks_kernel(int n, int n_pairs, const PgcPairDev* __restrict__ pairs, int band, const double* __restrict__ Z,
                                        int ld, const double* __restrict__ X, const int* __restrict__ ok, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 144 * n_pairs || !*ok) return;
  const PgcPairDev p = pairs[t / 144];
  const int I = (t % 144) / 12, J = t % 12;
  const int fx = I < 6 ? p.fa : p.fb, fy = J < 6 ? p.fa : p.fb;
  const int cx = I < 6 ? p.ca : p.cb, cy = J < 6 ? p.ca : p.cb;
  const int r = I % 6, c = J % 6;
  double v = 0.0;
  if (fx >= 0 && fy >= 0) {
    const int i = 6 * fx + r, j = 6 * fy + c;
    const bool cols = !(band && fx == fy) && (cx >= 0 || cy >= 0);
    if (!cols)
      v = Z[(size_t)max(i, j) * (ld + 1) + ld - (max(i, j) - min(i, j))];
    else if (cx >= 0 && cy >= 0)
      v = 0.5 * (X[vsl_cov_x_at(n, i, cy + c)] + X[vsl_cov_x_at(n, j, cx + r)]);
    else if (cy >= 0)
      v = X[vsl_cov_x_at(n, i, cy + c)];
    else
      v = X[vsl_cov_x_at(n, j, cx + r)];
  }
  out[t] = v;
}

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

// The producer side of the _w entry points (vsl_ba_relative_pose_covariance, ba_cov.hip): one wavefront per pair
// (a, b) of a bundle-adjustment problem, whose 12 x 12 joint block of S^-1 is in `joint`.  Lane 0 evaluates the
// functor at a zero measurement with the dual numbers above -- meas = log(T_a^-1 T_b), and the Jacobians of the
// residual, which do not depend on the measurement; a fixed camera's half of J is zero.  The lanes share T = Sigma J^T
// and M = J T as in pgo_edge_consistency_kernel (every sum in ascending index order), cov = (M + M^T) / 2.  Lane 0
// factors cov = L L^T (a pivot L_ii^2 <= 2^-36 cov_ii, or one that is not finite, fails) and inverts L by forward
// substitution; info_ij = sum_{k >= max(i, j)} Linv_ki Linv_kj, k ascending, one lane per entry: (i, j) and (j, i) sum
// the same products in the same order.  The result is then put through the pivot test of pgo_edge_whiten_kernel, so a
// finite info is one that the _w calls accept.  A failing pair gets 36 NaN and singular[q] = 1.  No atomics.
__global__ __launch_bounds__(64) void ba_relpose_kernel(int n_pairs, const double* __restrict__ poses,
                                                        const PgcPairDev* __restrict__ pairs, const double* __restrict__ joint,
                                                        const int* __restrict__ ok, double* __restrict__ meas,
                                                        double* __restrict__ cov, double* __restrict__ info,
                                                        int* __restrict__ singular) {
  __shared__ double Jm[6][12], Tm[12][6], Mm[6][6], Am[6][6], Li[6][6];
  __shared__ int bad;
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= n_pairs || !*ok) return;
  const PgcPairDev p = pairs[q];
  if (lane == 0) {
    D12 qc[4], tc[3], qn[4], tn[3], rd[6];
    const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    seed_pose(poses + 7 * (size_t)p.na, 0, qc, tc);
    seed_pose(poses + 7 * (size_t)p.nb, 6, qn, tn);
    edge_residual(qc, tc, qn, tn, zero, rd);
    for (int i = 0; i < 6; i++) {
      meas[6 * (size_t)q + i] = rd[i].v;
      for (int c = 0; c < 6; c++) {
        Jm[i][c] = p.fa >= 0 ? rd[i].d[c] : 0.0;
        Jm[i][6 + c] = p.fb >= 0 ? rd[i].d[6 + c] : 0.0;
      }
    }
    bad = 0;
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
    const double s = 0.5 * (Mm[i][j] + Mm[j][i]);
    cov[36 * (size_t)q + lane] = s;
    Am[i][j] = s;
  }
  __syncthreads();
  // the 6 x 6 steps are relpose_math.h's (tests/cpp/relpose_math_test.cpp drives their failure branches on the host)
  if (lane == 0 && !rpm_factor_invert(Am, Li)) bad = 1;  // Am <- L, Li <- L^-1
  __syncthreads();
  if (!bad && lane < 36) Mm[lane / 6][lane % 6] = rpm_info_entry(Li, lane / 6, lane % 6);  // Omega
  __syncthreads();
  if (!bad && lane == 0 && !rpm_accepts(Mm, Am)) bad = 1;
  __syncthreads();
  if (lane < 36) info[36 * (size_t)q + lane] = bad ? __builtin_nan("") : Mm[lane / 6][lane % 6];
  if (lane == 0) singular[q] = bad;
}

struct PgoJointCall {
  const char* name;
  const int32_t *a, *b;
  int n_pairs;
  bool with_cand;
  const double *cand_meas, *meas_cov;                // the edge call (meas_cov nullable)
  double *cov, *resid, *resid_cov, *chi2;            // outputs (cov: the joint call; chi2 nullable)
  const double* edge_info = nullptr;                 // the _w calls: information matrices of the graph's own edges
};

// everything behind the validation; host_in / host_out are read / written by copies on the stream
int pgo_joint_run(vsl_ctx* ctx, const vsl_pgo_problem* run, const vsl_ba_options* opt, bool folded, const PgoJointCall& c,
                  const vsl_pgo_problem* orig, std::vector<char>& host_in, std::vector<char>& host_out, bool* dense_out) {
  int nf = 0;
  const std::vector<int> run_free = pgo_free_index(run, &nf);
  PgoState st;
  st.linear_only = folded;
  st.edge_info = c.edge_info;
  st.who = c.name;
  {
    PgoState probe;
    probe.linear_only = folded;
    pgo_storage(ctx, run, run_free, nf, probe);
    st.bw = probe.bw;
    st.ld = probe.ld;
  }
  const bool dense = st.ld == 0;
  *dense_out = dense;
  // (the plan numbers the nodes from the caller's graph: the fold is its own)
  const PgcPlan P = pgc_plan(orig->n_nodes, orig->node_fixed, folded, dense, st.bw, ctx->pgo_cov_no_band_read, c.a, c.b, c.n_pairs,
                             c.with_cand);
  st.extra_bytes = P.total;
  int rc;
  if ((rc = pgo_setup(ctx, run, st))) return rc;
  if ((st.ld == 0) != dense || st.n != P.n) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: the set-up and the plan disagree", c.name);
  hipStream_t s = ctx->stream;
  const int n = st.n, np = c.n_pairs;
  char* dev = st.extra;
  host_in.assign(P.in_bytes, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(host_in.data() + off, src, bytes);
  };
  put(P.off_pairs, P.pairs.data(), sizeof(PgcPairDev) * P.pairs.size());
  put(P.off_col_unk, P.col_unk.data(), sizeof(int) * P.col_unk.size());
  put(P.off_row_lo, P.row_lo.data(), sizeof(int) * P.row_lo.size());
  if (c.with_cand) {
    put(P.off_meas, c.cand_meas, sizeof(double) * 6 * (size_t)np);
    if (c.meas_cov) put(P.off_meas_cov, c.meas_cov, sizeof(double) * 36 * (size_t)np);
  }
  VSL_HIP(ctx, hipMemcpyAsync(dev, host_in.data(), P.in_bytes, hipMemcpyHostToDevice, s));
  const PgcPairDev* pairs = (const PgcPairDev*)(dev + P.off_pairs);
  const int* col_dev = (const int*)(dev + P.off_col_unk);
  double* Hdiag = (double*)(dev + P.off_Hdiag);
  double* X = (double*)(dev + P.off_X);
  double* out = (double*)(dev + P.out_off + P.off_cov);
  // unit scale, one linearisation at the poses as they are: vsl_pgo_covariance's H
  VSL_HIP(ctx, hipMemsetAsync(st.colsq, 0, 8 * (size_t)n, s));
  hipLaunchKernelGGL(pgo_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.colsq, st.scale);
  double cost = 0;
  if ((rc = pgo_linearize(ctx, st, opt, false, &cost))) return rc;
  hipLaunchKernelGGL(pgo_cov_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, st.H, st.ld, Hdiag);
  VSL_CHECK_LAUNCH(ctx);
  if (dense) {
    double* Linv = (double*)(dev + P.off_Linv);
    if ((rc = vsl_chol_factor_dev(ctx, st.H, n, st.flag, Linv))) return rc;
    if ((rc = vsl_cov_unit_columns_dev(ctx, n, st.H, Linv, Hdiag, col_dev, P.nblk, X, st.flag))) return rc;
  } else {
    if ((rc = vsl_chol_selinv_band_dev(ctx, st.H + st.ld, st.A + st.ld, n, st.ld, st.bw, st.flag))) return rc;
    if ((rc = vsl_cov_band_pivot_dev(ctx, n, st.H, st.ld, Hdiag, st.flag))) return rc;
    if ((rc = vsl_cov_band_unit_columns_dev(ctx, n, st.H, st.ld, st.bw, vsl_chol_selinv_linv_dev(ctx, n, st.bw), col_dev,
                                            (const int*)(dev + P.off_row_lo), P.nblk, X, st.flag)))
      return rc;
  }
  hipLaunchKernelGGL(pgo_joint_blocks_kernel, dim3((144 * np + 255) / 256), dim3(256), 0, s, n, np, pairs, dense ? 0 : 1, st.A, st.ld, X,
                     st.flag, out);
  if (c.with_cand)
    hipLaunchKernelGGL(pgo_edge_consistency_kernel, dim3(np), dim3(64), 0, s, np, st.poses, pairs, (const double*)(dev + P.off_meas),
                       c.meas_cov ? (const double*)(dev + P.off_meas_cov) : (const double*)nullptr, out, st.flag,
                       (double*)(dev + P.out_off + P.off_resid), (double*)(dev + P.out_off + P.off_resid_cov),
                       (double*)(dev + P.out_off + P.off_chi2));
  VSL_CHECK_LAUNCH(ctx);
  int ok = 0;
  host_out.assign(P.out_bytes, 0);
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data(), dev + P.out_off, P.out_bytes, hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipMemcpyAsync(&ok, st.flag, sizeof(int), hipMemcpyDeviceToHost, s));
  VSL_HIP(ctx, hipStreamSynchronize(s));
  if (!ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: the normal equations are not positive definite (no fixed node, or a free node without an edge)", c.name);
  if (c.cov) memcpy(c.cov, host_out.data() + P.off_cov, sizeof(double) * 144 * (size_t)np);
  if (c.with_cand) {
    memcpy(c.resid, host_out.data() + P.off_resid, sizeof(double) * 6 * (size_t)np);
    memcpy(c.resid_cov, host_out.data() + P.off_resid_cov, sizeof(double) * 36 * (size_t)np);
    if (c.chi2) memcpy(c.chi2, host_out.data() + P.off_chi2, sizeof(double) * (size_t)np);
  }
  return VSL_OK;
}

int pgo_joint_call(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const PgoJointCall& c, int* storage) {
  int rc = pgo_validate(ctx, prob);
  if (rc) return rc;
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
  int nf = 0;
  const std::vector<int> free_idx = pgo_free_index(prob, &nf);
  int route;
  {
    PgoState probe;
    pgo_storage(ctx, prob, free_idx, nf, probe);
    route = probe.ld > 0 ? (probe.cyclic ? 2 : 1) : 0;
  }
  if (storage) *storage = route;
  if (c.n_pairs == 0) return VSL_OK;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<char> host_in, host_out;
  PgoFolded F;
  const vsl_pgo_problem* run = prob;
  if (route == 2) {
    pgo_fold_problem(prob, free_idx, nf, F);
    run = &F.prob;
  }
  bool dense = false;
  rc = pgo_joint_run(ctx, run, opt, route == 2, c, prob, host_in, host_out, &dense);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);  // queued copies read host buffers that end here
    return rc;
  }
  if (storage) *storage = dense ? 0 : route;
  return VSL_OK;
}
}  // namespace

int vsl_pgo_relpose_dev(vsl_ctx* ctx, int n_pairs, const double* poses, const PgcPairDev* pairs, const double* joint,
                        const int* ok_dev, double* meas, double* cov, double* info, int* singular) {
  if (n_pairs <= 0) return VSL_OK;
  hipLaunchKernelGGL(ba_relpose_kernel, dim3(n_pairs), dim3(64), 0, ctx->stream, n_pairs, poses, pairs, joint, ok_dev, meas, cov,
                     info, singular);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

extern "C" int vsl_pgo_joint_covariance(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const int32_t* pair_a,
                                        const int32_t* pair_b, int n_pairs, double* cov, int* storage) {
  if (!ctx) return VSL_ERR_INVALID;
  const PgoJointCall c{"vsl_pgo_joint_covariance", pair_a, pair_b, n_pairs, false, nullptr, nullptr, cov, nullptr, nullptr, nullptr};
  return pgo_joint_call(ctx, prob, opt, c, storage);
}
extern "C" int vsl_pgo_joint_covariance_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                          const int32_t* pair_a, const int32_t* pair_b, int n_pairs, double* cov, int* storage) {
  if (!ctx) return VSL_ERR_INVALID;
  PgoJointCall c{"vsl_pgo_joint_covariance_w", pair_a, pair_b, n_pairs, false, nullptr, nullptr, cov, nullptr, nullptr, nullptr};
  c.edge_info = edge_info;
  return pgo_joint_call(ctx, prob, opt, c, storage);
}

extern "C" int vsl_pgo_edge_consistency(vsl_ctx* ctx, const vsl_pgo_problem* prob, const vsl_ba_options* opt, const int32_t* cand_a,
                                        const int32_t* cand_b, const double* cand_meas, const double* meas_cov, int n_cand,
                                        double* resid, double* resid_cov, double* chi2, int* storage) {
  if (!ctx) return VSL_ERR_INVALID;
  const PgoJointCall c{"vsl_pgo_edge_consistency", cand_a, cand_b, n_cand, true, cand_meas, meas_cov, nullptr, resid, resid_cov, chi2};
  return pgo_joint_call(ctx, prob, opt, c, storage);
}
// edge_info shapes H and so Sigma; the candidate's residual stays unwhitened, meas_cov keeps its meaning
extern "C" int vsl_pgo_edge_consistency_w(vsl_ctx* ctx, const vsl_pgo_problem* prob, const double* edge_info, const vsl_ba_options* opt,
                                          const int32_t* cand_a, const int32_t* cand_b, const double* cand_meas, const double* meas_cov,
                                          int n_cand, double* resid, double* resid_cov, double* chi2, int* storage) {
  if (!ctx) return VSL_ERR_INVALID;
  PgoJointCall c{"vsl_pgo_edge_consistency_w", cand_a, cand_b, n_cand, true, cand_meas, meas_cov, nullptr, resid, resid_cov, chi2};
  c.edge_info = edge_info;
  return pgo_joint_call(ctx, prob, opt, c, storage);
}
