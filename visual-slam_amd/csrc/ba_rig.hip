// ba_rig.hip -- rig-constrained bundle adjustment: ONE SE(3) block per stereo frame (the body), the calibrated
// extrinsics T_b_c held fixed, T_w_c = T_w_b * T_b_c[cam_intr].  vsl_bundle_adjust_rig, and the two parity hooks
// vsl_ba_rig_linearize / vsl_ba_rig_system (include/vslam_hip.h "rig-constrained bundle adjustment").
// The covariances of the rig posterior (vsl_ba_rig_covariance, vsl_ba_rig_relative_pose_covariance) are
// the section "COVARIANCES" at the end of this file.
//
// Residual, camera models, Huber corrector and cost are those of vsl_bundle_adjust (ba_device.h); what changes is the
// pose block an observation differentiates against.  With T_c_b = T_b_c^-1 = (R, t),
//   T_w_b exp(d) T_b_c = T_w_c exp(Ad(T_c_b) d),   Ad = [[R, [t]x R], [0, R]]  in the (upsilon, omega) order,
// so F_b = F_c Ad = [F_u R, (F_u [t]x + F_w) R], formed in registers per observation (rig_body_jacobian).  Everything
// downstream of the stored blocks works on BODY columns: Jacobi scaling, LM damping, the Schur complement, the step.
//
// The chain (all reductions in a fixed order: two solves give the same bits; no floating-point atomics anywhere):
//   rig_cams_kernel        camera poses from the bodies
//   rig_linearize_kernel   r, F_b, E per observation (robustified, scaled when scales are given), cost partials
//   rig_lm_cols_kernel     per landmark: squared column norms of E, E^T r
//   rig_body_block_kernel  per free body and segment: partial H = sum F_b^T F_b, g = sum F_b^T r over a slice of the body's
//                          observations; rig_body_block_finish_kernel adds the segments in order
//   rig_lm_groups_kernel   per landmark: P (+ damping), P^-1, b; per (landmark, free body) GROUP W = sum F_b^T E over
//                          the group's observations -- a landmark seen by both cameras of a body is one group of two --
//                          and Y = W P^-1
//   rig_schur_block_kernel workgroups per 6 x 6 block (a, b), a >= b, of the reduced system and segment: walks a slice of
//                          the groups of body a (ascending landmark), finds body b's group of the same landmark by
//                          bisection, sums Y_a W_b^T per thread, reduces in a fixed tree; rig_schur_finish_kernel adds the
//                          segments in order and writes the block and its mirror image (S is exactly symmetric).
//                          A landmark with any number of observations is the same code: the per-landmark kernels
//                          loop, the gather sees one group per body.
//   dense SPD solve        ba_chol_small_kernel up to 128 unknowns, the dense panel factorisation of chol.hip beyond
//   rig_backsub_kernel, rig_model_kernel, rig_update_kernel: landmark step, model cost change, T_w_b * exp(step)
// The LM loop is host-decided with ONE synchronisation per iteration (the candidate is linearised speculatively into a
// second set of blocks, as in vsl_bundle_adjust's host loop) under the policy of lm_policy.h.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "vsl_common.h"
#include "lm_policy.h"
#include "dev_arena.h"
#include "ba_device.h"
#include "ba_rig_plan.h"
#include "ba_rig_cov_plan.h"
#include "pgo_cov_plan.h"

namespace {

struct RigDims {
  int C, B, L, O, G, nfree, n;
  int model0, model1;
  int use_huber;
  double huber;
};

// F (2 x 6, camera tangent) -> F Ad(T_c_b), T_c_b = (R row-major 9, t 3)
__device__ __forceinline__ void rig_body_jacobian(const double* __restrict__ Rt, double* F) {
  const double* R = Rt;
  const double tx = Rt[9], ty = Rt[10], tz = Rt[11];
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const double u0 = F[6 * a], u1 = F[6 * a + 1], u2 = F[6 * a + 2];
    // u^T [t]x + w^T, [t]x = [0 -tz ty; tz 0 -tx; -ty tx 0]
    const double w0 = (u1 * tz - u2 * ty) + F[6 * a + 3];
    const double w1 = (u2 * tx - u0 * tz) + F[6 * a + 4];
    const double w2 = (u0 * ty - u1 * tx) + F[6 * a + 5];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      F[6 * a + j] = u0 * R[j] + u1 * R[3 + j] + u2 * R[6 + j];
      F[6 * a + 3 + j] = w0 * R[j] + w1 * R[3 + j] + w2 * R[6 + j];
    }
  }
}

// sums of N per-thread values over a 256-thread workgroup in a fixed order (lanes by shuffle, then the four waves in
// order): every thread gets the sums back in acc.  sh: 4 * N doubles
template <int N>
__device__ __forceinline__ void rig_block_sum(double* acc, double* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave * N + k] = v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) acc[k] = ((sh[k] + sh[N + k]) + sh[2 * N + k]) + sh[3 * N + k];
  __syncthreads();
}

// T_w_c = T_w_b * T_b_c
__global__ void rig_cams_kernel(int C, const double* __restrict__ bodies, const double* __restrict__ tbc,
                                const int* __restrict__ cam_body, const int* __restrict__ cam_intr, double* __restrict__ cams) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double* T = bodies + 7 * (size_t)cam_body[c];
  const double* e = tbc + 7 * cam_intr[c];
  double R[9];
  quat_R(T, R);
  double* o = cams + 7 * (size_t)c;
  const double qx = T[0], qy = T[1], qz = T[2], qw = T[3];
  o[0] = qw * e[0] + qx * e[3] + qy * e[2] - qz * e[1];
  o[1] = qw * e[1] - qx * e[2] + qy * e[3] + qz * e[0];
  o[2] = qw * e[2] + qx * e[1] - qy * e[0] + qz * e[3];
  o[3] = qw * e[3] - qx * e[0] - qy * e[1] - qz * e[2];
  for (int i = 0; i < 3; i++) o[4 + i] = T[4 + i] + (R[3 * i] * e[4] + R[3 * i + 1] * e[5] + R[3 * i + 2] * e[6]);
}

__global__ __launch_bounds__(256) void rig_linearize_kernel(RigDims D, const double* __restrict__ cams,
                                                            const double* __restrict__ points, const double* __restrict__ intr,
                                                            const double* __restrict__ tcb, const int* __restrict__ cam_intr,
                                                            const int* __restrict__ cam_slot, const int* __restrict__ obs_cam,
                                                            const int* __restrict__ obs_lm, const double* __restrict__ obs_uv,
                                                            const double* __restrict__ scale_c, const double* __restrict__ scale_l,
                                                            double* __restrict__ r_out, double* __restrict__ F_out,
                                                            double* __restrict__ E_out, double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double c = 0;
  if (i < D.O) {
    const int cam = obs_cam[i], lm = obs_lm[i], k = cam_intr[cam];
    double r[2], F[12], E[6];
    residual_blocks(k ? D.model1 : D.model0, intr + 8 * k, cams + 7 * (size_t)cam, points + 3 * (size_t)lm, obs_uv + 2 * (size_t)i, r, F,
                    E, true);
    rig_body_jacobian(tcb + 12 * k, F);
    const double s = r[0] * r[0] + r[1] * r[1];
    double rho0 = s, rho1 = 1.0;
    if (D.use_huber) huber(s, D.huber, rho0, rho1);
    c = 0.5 * rho0;
    const double sr = sqrt(rho1);
    r_out[2 * (size_t)i] = r[0] * sr;
    r_out[2 * (size_t)i + 1] = r[1] * sr;
    const int slot = cam_slot[cam];
    for (int j = 0; j < 6; j++) {
      const double sc = (scale_c && slot >= 0) ? scale_c[6 * (size_t)slot + j] : 1.0;
      F_out[12 * (size_t)i + j] = F[j] * sr * sc;
      F_out[12 * (size_t)i + 6 + j] = F[6 + j] * sr * sc;
    }
    for (int j = 0; j < 3; j++) {
      const double sc = scale_l ? scale_l[3 * (size_t)lm + j] : 1.0;
      E_out[6 * (size_t)i + j] = E[j] * sr * sc;
      E_out[6 * (size_t)i + 3 + j] = E[3 + j] * sr * sc;
    }
  }
  const double t = block_sum_256(c, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// scalars[slot] = sum / max of partials[0..n) in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void rig_reduce_kernel(const double* __restrict__ partials, int n, double* __restrict__ scalars,
                                                         int slot, int is_max) {
  __shared__ double sh[256];
  double v = 0;
  for (int i = threadIdx.x; i < n; i += 256) v = is_max ? fmax(v, partials[i]) : v + partials[i];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = is_max ? fmax(sh[threadIdx.x], sh[threadIdx.x + o]) : sh[threadIdx.x] + sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) scalars[slot] = sh[0];
}

__global__ __launch_bounds__(256) void rig_lm_cols_kernel(RigDims D, const int* __restrict__ lm_start, const double* __restrict__ r,
                                                          const double* __restrict__ E, double* __restrict__ n2l,
                                                          double* __restrict__ grad_l) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= D.L) return;
  double n2[3] = {0, 0, 0}, g[3] = {0, 0, 0};
  for (int i = lm_start[l]; i < lm_start[l + 1]; i++) {
    const double* e = E + 6 * (size_t)i;
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    for (int j = 0; j < 3; j++) {
      n2[j] += e[j] * e[j] + e[3 + j] * e[3 + j];
      g[j] += e[j] * r0 + e[3 + j] * r1;
    }
  }
  for (int j = 0; j < 3; j++) {
    n2l[3 * (size_t)l + j] = n2[j];
    grad_l[3 * (size_t)l + j] = g[j];
  }
}

// grid (free bodies, segments): a workgroup sums every `segments`-th 256-observation slice of its body -- the 21 upper
// entries of H = sum F^T F and the 6 of g = sum F^T r -- into part[(body, segment)][27].  (One workgroup per body walked
// 22 k observations of the benchmark's window in 88 dependent trips: 120 us with six workgroups on the chip.)
__global__ __launch_bounds__(256) void rig_body_block_kernel(const int* __restrict__ bo_start, const int* __restrict__ bo_obs,
                                                             const double* __restrict__ r, const double* __restrict__ F,
                                                             double* __restrict__ part) {
  __shared__ double sh[4 * 27];
  const int s = blockIdx.x, seg = blockIdx.y, nseg = gridDim.y;
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = 0;
  for (int q = bo_start[s] + seg * 256 + threadIdx.x; q < bo_start[s + 1]; q += 256 * nseg) {
    const int i = bo_obs[q];
    const double* f = F + 12 * (size_t)i;
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = a; b < 6; b++) acc[k++] += f[a] * f[b] + f[6 + a] * f[6 + b];
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] += f[a] * r0 + f[6 + a] * r1;
  }
  rig_block_sum<27>(acc, sh);
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)s * nseg + seg) * 27;
#pragma unroll
    for (int k = 0; k < 27; k++) o[k] = acc[k];
  }
}

// the segments of a body in order: H (mirrored, exactly symmetric) and g
__global__ void rig_body_block_finish_kernel(int nfree, int nseg, const double* __restrict__ part, double* __restrict__ H,
                                             double* __restrict__ g) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nfree * 27) return;
  const int s = t / 27, k = t - s * 27;
  double v = 0;
  for (int q = 0; q < nseg; q++) v += part[((size_t)s * nseg + q) * 27 + k];
  if (k >= 21) {
    g[6 * (size_t)s + (k - 21)] = v;
  } else {
    int a = 0, rem = k;  // k-th entry of the upper triangle, row-major
    while (rem >= 6 - a) {
      rem -= 6 - a;
      a++;
    }
    const int b = a + rem;
    H[36 * (size_t)s + 6 * a + b] = v;
    H[36 * (size_t)s + 6 * b + a] = v;
  }
}

// Jacobi scaling (computed once, from the unscaled blocks): 1 / (1 + sqrt(column norm^2)), bodies from diag H
__global__ void rig_make_scale_kernel(int nfree, int L, const double* __restrict__ H, const double* __restrict__ n2l,
                                      double* __restrict__ scale_c, double* __restrict__ scale_l) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * nfree) scale_c[i] = 1.0 / (1.0 + sqrt(H[36 * (size_t)(i / 6) + 7 * (i % 6)]));
  if (i < 3 * L) scale_l[i] = 1.0 / (1.0 + sqrt(n2l[i]));
}

// LM diagonals clamp(column norm^2, 1e-6, 1e32) of the scaled blocks and the workgroup's max |gradient| of the
// UNSCALED problem
__global__ __launch_bounds__(256) void rig_diag_kernel(int nfree, int L, const double* __restrict__ H, const double* __restrict__ n2l,
                                                       const double* __restrict__ g_b, const double* __restrict__ grad_l,
                                                       const double* __restrict__ scale_c, const double* __restrict__ scale_l,
                                                       double* __restrict__ diag_c, double* __restrict__ diag_l,
                                                       double* __restrict__ gabs) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double m = 0;
  if (i < 6 * nfree) {
    diag_c[i] = fmin(fmax(H[36 * (size_t)(i / 6) + 7 * (i % 6)], 1e-6), 1e32);
    m = fabs(g_b[i] / scale_c[i]);
  }
  if (i < 3 * L) {
    diag_l[i] = fmin(fmax(n2l[i], 1e-6), 1e32);
    m = fmax(m, fabs(grad_l[i] / scale_l[i]));
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) gabs[blockIdx.x] = sh[0];
}

// per landmark: P = sum E^T E (+ diag_l * inv_radius), P^-1, b = sum E^T r; per group of the landmark W = sum F^T E
// (6 x 3 row-major) over the group's observations and Y = W P^-1.  A landmark whose P cannot be inverted gets
// P^-1 = 0: it contributes nothing to S and does not move.
__global__ __launch_bounds__(256) void rig_lm_groups_kernel(RigDims D, const int* __restrict__ lm_start, const int* __restrict__ lm_grp,
                                                            const int* __restrict__ grp_begin, const int* __restrict__ grp_end,
                                                            const double* __restrict__ r, const double* __restrict__ F,
                                                            const double* __restrict__ E, const double* __restrict__ diag_l,
                                                            double inv_radius, double* __restrict__ W, double* __restrict__ Y,
                                                            double* __restrict__ Pinv, double* __restrict__ bl) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= D.L) return;
  double P[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  for (int i = lm_start[l]; i < lm_start[l + 1]; i++) {
    const double* e = E + 6 * (size_t)i;
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    for (int j = 0; j < 3; j++) {
      for (int k = j; k < 3; k++) P[3 * j + k] += e[j] * e[k] + e[3 + j] * e[3 + k];
      b[j] += e[j] * r0 + e[3 + j] * r1;
    }
  }
  if (diag_l)
    for (int j = 0; j < 3; j++) P[4 * j] += diag_l[3 * (size_t)l + j] * inv_radius;
  P[3] = P[1]; P[6] = P[2]; P[7] = P[5];
  double Pi[9];
  if (!inv3(P, Pi))
    for (int j = 0; j < 9; j++) Pi[j] = 0.0;
  for (int j = 0; j < 9; j++) Pinv[9 * (size_t)l + j] = Pi[j];
  for (int j = 0; j < 3; j++) bl[3 * (size_t)l + j] = b[j];
  for (int g = lm_grp[l]; g < lm_grp[l + 1]; g++) {
    double w[18];
    for (int j = 0; j < 18; j++) w[j] = 0;
    for (int i = grp_begin[g]; i < grp_end[g]; i++) {
      const double* f = F + 12 * (size_t)i;
      const double* e = E + 6 * (size_t)i;
      for (int a = 0; a < 6; a++)
        for (int j = 0; j < 3; j++) w[3 * a + j] += f[a] * e[j] + f[6 + a] * e[3 + j];
    }
    for (int a = 0; a < 6; a++)
      for (int j = 0; j < 3; j++) {
        W[18 * (size_t)g + 3 * a + j] = w[3 * a + j];
        Y[18 * (size_t)g + 3 * a + j] = w[3 * a] * Pi[j] + w[3 * a + 1] * Pi[3 + j] + w[3 * a + 2] * Pi[6 + j];
      }
  }
}

// grid (nfree, nfree, segments): the workgroups of block (a = x, b = y), a >= b (the others leave at once), each sum
// every `segments`-th 256-group slice of body a's groups: Y_a W_b^T over the landmarks both bodies see (36 sums) and, on
// the diagonal, Y_a b_l (6 more), into spart[(pair a (a + 1) / 2 + b, segment)][42].
__global__ __launch_bounds__(256) void rig_schur_block_kernel(const int* __restrict__ bg_start, const int* __restrict__ bg_grp,
                                                              const int* __restrict__ bg_lm, const double* __restrict__ W,
                                                              const double* __restrict__ Y, const double* __restrict__ bl,
                                                              double* __restrict__ spart) {
  __shared__ double sh[4 * 42];
  const int a = blockIdx.x, b = blockIdx.y, seg = blockIdx.z, nseg = gridDim.z;
  if (b > a) return;
  double acc[42];
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = 0;
  const int b0 = bg_start[b], b1 = bg_start[b + 1];
  for (int k = bg_start[a] + seg * 256 + threadIdx.x; k < bg_start[a + 1]; k += 256 * nseg) {
    const int lm = bg_lm[k];
    int p = k;
    if (a != b) {
      int lo = b0, hi = b1;  // first position in [b0, b1) whose landmark is >= lm
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (bg_lm[mid] < lm) lo = mid + 1;
        else hi = mid;
      }
      if (lo >= b1 || bg_lm[lo] != lm) continue;
      p = lo;
    }
    const double* y = Y + 18 * (size_t)bg_grp[k];
    const double* w = W + 18 * (size_t)bg_grp[p];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) acc[6 * i + j] += y[3 * i] * w[3 * j] + y[3 * i + 1] * w[3 * j + 1] + y[3 * i + 2] * w[3 * j + 2];
    if (a == b) {
      const double* bb = bl + 3 * (size_t)lm;
#pragma unroll
      for (int i = 0; i < 6; i++) acc[36 + i] += y[3 * i] * bb[0] + y[3 * i + 1] * bb[1] + y[3 * i + 2] * bb[2];
    }
  }
  rig_block_sum<42>(acc, sh);
  if (threadIdx.x == 0) {
    double* o = spart + (((size_t)a * (a + 1) / 2 + b) * nseg + seg) * 42;
#pragma unroll
    for (int k = 0; k < 42; k++) o[k] = acc[k];
  }
}

// grid (nfree, nfree), 64 threads: the segments of block (a, b), a >= b, in order, then
//   S_ab = [a == b] (H_a + diag_c * inv_radius) - sum,  mirrored into S_ba (S is exactly symmetric);
//   a == b also: rhs_a = g_a - sum.
// Workgroup (0, 0) arms the two flags of the step (flag[0] all finite, flag[1] factorisation succeeded).
__global__ __launch_bounds__(64) void rig_schur_finish_kernel(int n, int nseg, const double* __restrict__ spart,
                                                              const double* __restrict__ H, const double* __restrict__ g_b,
                                                              const double* __restrict__ diag_c, double inv_radius,
                                                              double* __restrict__ S, double* __restrict__ rhs,
                                                              int* __restrict__ flag) {
  const int a = blockIdx.x, b = blockIdx.y;
  if (b > a) return;
  if (a == 0 && threadIdx.x < 2) flag[threadIdx.x] = 1;
  const int e = threadIdx.x;
  if (e >= 42) return;
  const double* p = spart + ((size_t)a * (a + 1) / 2 + b) * nseg * 42;
  double sum = 0;
  for (int q = 0; q < nseg; q++) sum += p[(size_t)q * 42 + e];
  if (e < 36) {
    const int i = e / 6, j = e - 6 * i;
    const size_t at = (size_t)(6 * a + i) * n + 6 * b + j, mirror = (size_t)(6 * b + j) * n + 6 * a + i;
    if (a != b) {
      S[at] = -sum;
      S[mirror] = -sum;
    } else if (i >= j) {
      double h = H[36 * (size_t)a + e];
      if (i == j && diag_c) h += diag_c[6 * (size_t)a + i] * inv_radius;
      const double v = h - sum;
      S[at] = v;
      S[mirror] = v;
    }
  } else if (a == b) {
    rhs[6 * (size_t)a + (e - 36)] = g_b[6 * (size_t)a + (e - 36)] - sum;
  }
}

// delta_l = -P^-1 (b_l + sum over the landmark's groups of W^T delta_body); flag[0] cleared on a non-finite step
__global__ __launch_bounds__(256) void rig_backsub_kernel(RigDims D, const int* __restrict__ lm_grp, const int* __restrict__ grp_slot,
                                                          const double* __restrict__ W, const double* __restrict__ Pinv,
                                                          const double* __restrict__ bl, const double* __restrict__ dc,
                                                          double* __restrict__ dl, int* __restrict__ finite_flag) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  for (int j = l; j < D.n; j += gridDim.x * 256)
    if (!isfinite(dc[j])) *finite_flag = 0;
  if (l >= D.L) return;
  double t[3] = {bl[3 * (size_t)l], bl[3 * (size_t)l + 1], bl[3 * (size_t)l + 2]};
  for (int g = lm_grp[l]; g < lm_grp[l + 1]; g++) {
    const double* w = W + 18 * (size_t)g;
    const double* d = dc + 6 * (size_t)grp_slot[g];
    for (int j = 0; j < 3; j++)
      for (int a = 0; a < 6; a++) t[j] += w[3 * a + j] * d[a];
  }
  const double* Pi = Pinv + 9 * (size_t)l;
  for (int j = 0; j < 3; j++) {
    const double v = -(Pi[3 * j] * t[0] + Pi[3 * j + 1] * t[1] + Pi[3 * j + 2] * t[2]);
    dl[3 * (size_t)l + j] = v;
    if (!isfinite(v)) *finite_flag = 0;
  }
}

// model cost change partials: -(J d)^T (r + J d / 2)
__global__ __launch_bounds__(256) void rig_model_kernel(RigDims D, const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                                        const int* __restrict__ cam_slot, const double* __restrict__ r,
                                                        const double* __restrict__ F, const double* __restrict__ E,
                                                        const double* __restrict__ dc, const double* __restrict__ dl,
                                                        double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v = 0;
  if (i < D.O) {
    const int slot = cam_slot[obs_cam[i]], lm = obs_lm[i];
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    double m0 = 0, m1 = 0;
    if (slot >= 0)
      for (int j = 0; j < 6; j++) {
        m0 += f[j] * dc[6 * (size_t)slot + j];
        m1 += f[6 + j] * dc[6 * (size_t)slot + j];
      }
    for (int j = 0; j < 3; j++) {
      m0 += e[j] * dl[3 * (size_t)lm + j];
      m1 += e[3 + j] * dl[3 * (size_t)lm + j];
    }
    v = -(m0 * (r[2 * (size_t)i] + m0 / 2.0) + m1 * (r[2 * (size_t)i + 1] + m1 / 2.0));
  }
  const double t = block_sum_256(v, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// candidate bodies T_w_b * exp(step .* scale) and points p + step .* scale; partials [0, nb): squared step norm,
// [nb, 2 nb): squared norm of the current free bodies and points
__global__ __launch_bounds__(256) void rig_update_kernel(RigDims D, const int* __restrict__ body_slot, const double* __restrict__ bodies,
                                                         const double* __restrict__ points, const double* __restrict__ dc,
                                                         const double* __restrict__ dl, const double* __restrict__ scale_c,
                                                         const double* __restrict__ scale_l, double* __restrict__ cand_bodies,
                                                         double* __restrict__ cand_points, double* __restrict__ partials, int nb) {
  __shared__ double sh[256];
  const int t = blockIdx.x * 256 + threadIdx.x;
  double step2 = 0, x2 = 0;
  if (t < D.B) {
    const int slot = body_slot[t];
    const double* T = bodies + 7 * (size_t)t;
    double* o = cand_bodies + 7 * (size_t)t;
    if (slot < 0) {
      for (int j = 0; j < 7; j++) o[j] = T[j];
    } else {
      double d[6];
      for (int j = 0; j < 6; j++) {
        d[j] = dc[6 * (size_t)slot + j] * scale_c[6 * (size_t)slot + j];
        step2 += d[j] * d[j];
      }
      for (int j = 0; j < 7; j++) x2 += T[j] * T[j];
      se3_plus(T, d, o);
    }
  }
  if (t < D.L) {
    for (int j = 0; j < 3; j++) {
      const double dd = dl[3 * (size_t)t + j] * scale_l[3 * (size_t)t + j];
      step2 += dd * dd;
      const double xv = points[3 * (size_t)t + j];
      x2 += xv * xv;
      cand_points[3 * (size_t)t + j] = xv + dd;
    }
  }
  const double a = block_sum_256(step2, sh);
  __syncthreads();
  const double b = block_sum_256(x2, sh);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = a;
    partials[nb + blockIdx.x] = b;
  }
}

// scalars[slot] and scalars[slot + 1] = sums of partials[0..n) and partials[n..2n): a workgroup each
__global__ __launch_bounds__(256) void rig_reduce2_kernel(const double* __restrict__ partials, int n, double* __restrict__ scalars,
                                                          int slot) {
  __shared__ double sh[256];
  const double* p = partials + (size_t)blockIdx.x * n;
  double v = 0;
  for (int i = threadIdx.x; i < n; i += 256) v += p[i];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) scalars[slot + blockIdx.x] = sh[0];
}

// ------------------------------------------------------------------------------------------------ host state
// what a linearisation point owns: the LM loop keeps two and swaps them when a step is accepted
struct RigSet {
  double *bodies = nullptr, *cams = nullptr, *points = nullptr;
  double *r = nullptr, *F = nullptr, *E = nullptr, *n2l = nullptr, *grad_l = nullptr, *H = nullptr, *g_b = nullptr;
  double *diag_c = nullptr, *diag_l = nullptr;
};

struct RigState {
  RigDims D;
  RigPlan plan;
  DevArena arena;
  int nb_obs = 1, nb_upd = 1, nb_diag = 1;
  int body_seg = 1, schur_seg = 1;  // workgroups per free body in rig_body_block_kernel / per block in rig_schur_block_kernel
  RigSet cur, cand;
  double *intr = nullptr, *tbc = nullptr, *tcb = nullptr, *obs_uv = nullptr;
  double *scale_c = nullptr, *scale_l = nullptr, *W = nullptr, *Y = nullptr, *Pinv = nullptr, *bl = nullptr;
  double *S = nullptr, *rhs = nullptr, *dc = nullptr, *dl = nullptr, *partials = nullptr, *scalars = nullptr;
  double *body_part = nullptr, *schur_part = nullptr;
  int* flag = nullptr;  // 128 bytes behind scalars: one copy brings both back
  int *cam_intr = nullptr, *cam_body = nullptr, *cam_slot = nullptr, *body_slot = nullptr, *obs_cam = nullptr, *obs_lm = nullptr;
  int *lm_start = nullptr, *lm_grp = nullptr, *grp_slot = nullptr, *grp_begin = nullptr, *grp_end = nullptr;
  int *bg_start = nullptr, *bg_grp = nullptr, *bg_lm = nullptr, *bo_start = nullptr, *bo_obs = nullptr;
  char* extra = nullptr;  // the covariance calls' share of the arena (behind everything else: no other offset moves)
};

int rig_validate(vsl_ctx* ctx, const char* who, const vsl_ba_problem* p, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                 RigPlan& plan) {
  if (!ctx) return VSL_ERR_INVALID;
  if (!p || !rig || !opt || !p->poses || !p->cam_intr || !p->intr || !p->points || !p->obs_cam || !p->obs_lm || !p->obs_uv ||
      !rig->body_poses || !rig->body_fixed || !rig->cam_body || !rig->T_b_c)
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null pointer", who);
  for (int k = 0; k < 2; k++)
    if (p->cam_model[k] < 0 || p->cam_model[k] > 3) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: unknown camera model %d", who, p->cam_model[k]);
  RigPlanIn in;
  in.n_cams = p->n_cams; in.n_lms = p->n_lms; in.n_obs = p->n_obs;
  in.cam_intr = p->cam_intr; in.obs_cam = p->obs_cam; in.obs_lm = p->obs_lm;
  in.n_bodies = rig->n_bodies; in.body_fixed = rig->body_fixed; in.cam_body = rig->cam_body; in.T_b_c = rig->T_b_c;
  const int st = rig_plan_build(in, plan);
  if (st != RIG_PLAN_OK) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: %s (index %d)", who, rig_plan_message(st), plan.first_bad);
  return VSL_OK;
}

// plan -> ONE arena (the context's), uploads; synchronises
int rig_setup(vsl_ctx* ctx, const vsl_ba_problem* p, const vsl_ba_rig* rig, const vsl_ba_options* opt, RigState& st,
              size_t extra_bytes = 0) {
  const RigPlan& hp = st.plan;
  RigDims& D = st.D;
  D.C = p->n_cams; D.B = rig->n_bodies; D.L = p->n_lms; D.O = p->n_obs; D.G = hp.n_groups();
  D.nfree = hp.n_free; D.n = 6 * hp.n_free;
  D.model0 = p->cam_model[0]; D.model1 = p->cam_model[1];
  D.use_huber = opt->use_huber; D.huber = opt->huber_parameter;
  const size_t C = D.C, B = D.B, L = D.L, O = D.O, G = D.G, n = D.n, nf = D.nfree;
  st.nb_obs = (int)((O + 255) / 256);
  st.nb_upd = (int)((std::max(B, L) + 255) / 256);
  st.nb_diag = (int)((std::max(n, 3 * L) + 255) / 256);
  // a workgroup of the two gathers takes about two 256-entry trips of the longest body list (at most 64 segments)
  int max_obs = 0, max_grp = 0;
  for (int b = 0; b < hp.n_free; b++) {
    max_obs = std::max(max_obs, hp.bo_start[b + 1] - hp.bo_start[b]);
    max_grp = std::max(max_grp, hp.bg_start[b + 1] - hp.bg_start[b]);
  }
  st.body_seg = std::min(64, std::max(1, (max_obs + 511) / 512));
  st.schur_seg = std::min(64, std::max(1, (max_grp + 511) / 512));
  ArenaPlan plan(80);
  for (RigSet* s : {&st.cur, &st.cand}) {
    plan.add(s->bodies, 7 * B); plan.add(s->cams, 7 * C); plan.add(s->points, 3 * L);
    plan.add(s->r, 2 * O); plan.add(s->F, 12 * O); plan.add(s->E, 6 * O);
    plan.add(s->n2l, 3 * L); plan.add(s->grad_l, 3 * L); plan.add(s->H, 36 * nf); plan.add(s->g_b, n);
    plan.add(s->diag_c, n); plan.add(s->diag_l, 3 * L);
  }
  plan.add(st.intr, 16); plan.add(st.tbc, 14); plan.add(st.tcb, 24); plan.add(st.obs_uv, 2 * O);
  plan.add(st.scale_c, n); plan.add(st.scale_l, 3 * L);
  plan.add(st.W, 18 * G); plan.add(st.Y, 18 * G); plan.add(st.Pinv, 9 * L); plan.add(st.bl, 3 * L);
  plan.add(st.S, n * n); plan.add(st.rhs, n); plan.add(st.dc, n); plan.add(st.dl, 3 * L);
  plan.add(st.partials, (size_t)std::max(std::max(st.nb_obs, 2 * st.nb_upd), st.nb_diag));
  plan.add(st.scalars, 32);  // 16 doubles, then the flags
  plan.add(st.body_part, nf * st.body_seg * 27); plan.add(st.schur_part, nf * (nf + 1) / 2 * st.schur_seg * 42);
  plan.add(st.cam_intr, C); plan.add(st.cam_body, C); plan.add(st.cam_slot, C); plan.add(st.body_slot, B);
  plan.add(st.obs_cam, O); plan.add(st.obs_lm, O);
  plan.add(st.lm_start, L + 1); plan.add(st.lm_grp, L + 1);
  plan.add(st.grp_slot, G); plan.add(st.grp_begin, G); plan.add(st.grp_end, G);
  plan.add(st.bg_start, nf + 1); plan.add(st.bg_grp, G); plan.add(st.bg_lm, G);
  plan.add(st.bo_start, nf + 1); plan.add(st.bo_obs, hp.bo_obs.size());
  if (extra_bytes) plan.add(st.extra, extra_bytes);
  hipError_t e = st.arena.acquire(ctx, ArenaPolicy::BORROWED, plan);
  if (e != hipSuccess) return vsl_fail(ctx, e == hipErrorOutOfMemory ? VSL_ERR_NOMEM : VSL_ERR_HIP, "rig bundle adjustment: %zu bytes of device memory: %s", plan.total(), hipGetErrorString(e));
  st.flag = (int*)(st.scalars + 16);

  std::vector<double> uv(2 * O);
  for (size_t q = 0; q < O; q++) {
    uv[2 * q] = p->obs_uv[2 * (size_t)hp.perm[q]];
    uv[2 * q + 1] = p->obs_uv[2 * (size_t)hp.perm[q] + 1];
  }
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  };
  VSL_HIP(ctx, hipMemsetAsync(st.scalars, 0, 256, ctx->stream));
  VSL_HIP(ctx, up(st.cur.bodies, rig->body_poses, 56 * B));
  VSL_HIP(ctx, up(st.cur.points, p->points, 24 * L));
  VSL_HIP(ctx, up(st.intr, p->intr, 128));
  VSL_HIP(ctx, up(st.tbc, hp.T_b_c, sizeof(hp.T_b_c)));
  VSL_HIP(ctx, up(st.tcb, hp.T_c_b, sizeof(hp.T_c_b)));
  VSL_HIP(ctx, up(st.obs_uv, uv.data(), 16 * O));
  VSL_HIP(ctx, up(st.cam_intr, p->cam_intr, 4 * C));
  VSL_HIP(ctx, up(st.cam_body, rig->cam_body, 4 * C));
  VSL_HIP(ctx, up(st.cam_slot, hp.cam_slot.data(), 4 * C));
  VSL_HIP(ctx, up(st.body_slot, hp.body_slot.data(), 4 * B));
  VSL_HIP(ctx, up(st.obs_cam, hp.obs_cam.data(), 4 * O));
  VSL_HIP(ctx, up(st.obs_lm, hp.obs_lm.data(), 4 * O));
  VSL_HIP(ctx, up(st.lm_start, hp.lm_start.data(), 4 * (L + 1)));
  VSL_HIP(ctx, up(st.lm_grp, hp.lm_grp.data(), 4 * (L + 1)));
  VSL_HIP(ctx, up(st.grp_slot, hp.grp_slot.data(), 4 * G));
  VSL_HIP(ctx, up(st.grp_begin, hp.grp_begin.data(), 4 * G));
  VSL_HIP(ctx, up(st.grp_end, hp.grp_end.data(), 4 * G));
  VSL_HIP(ctx, up(st.bg_start, hp.bg_start.data(), 4 * (nf + 1)));
  VSL_HIP(ctx, up(st.bg_grp, hp.bg_grp.data(), 4 * G));
  VSL_HIP(ctx, up(st.bg_lm, hp.bg_lm.data(), 4 * G));
  VSL_HIP(ctx, up(st.bo_start, hp.bo_start.data(), 4 * (nf + 1)));
  VSL_HIP(ctx, up(st.bo_obs, hp.bo_obs.data(), 4 * hp.bo_obs.size()));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the uploads read host vectors that die here
  return VSL_OK;
}

int rig_cams(vsl_ctx* ctx, RigState& st, RigSet& s) {
  hipLaunchKernelGGL(rig_cams_kernel, dim3((st.D.C + 255) / 256), dim3(256), 0, ctx->stream, st.D.C, s.bodies, st.tbc, st.cam_body,
                     st.cam_intr, s.cams);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

// cameras, blocks and cost (-> scalars[cost_slot]) of a set at its bodies / points
int rig_linearize(vsl_ctx* ctx, RigState& st, RigSet& s, bool scaled, int cost_slot) {
  VslStage stage(ctx, VSL_STAGE_BA_LIN);
  int rc = rig_cams(ctx, st, s);
  if (rc) return rc;
  hipLaunchKernelGGL(rig_linearize_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, st.D, s.cams, s.points, st.intr, st.tcb,
                     st.cam_intr, st.cam_slot, st.obs_cam, st.obs_lm, st.obs_uv, scaled ? st.scale_c : nullptr,
                     scaled ? st.scale_l : nullptr, s.r, s.F, s.E, st.partials);
  hipLaunchKernelGGL(rig_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, st.partials, st.nb_obs, st.scalars, cost_slot, 0);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int rig_columns(vsl_ctx* ctx, RigState& st, RigSet& s) {
  VslStage stage(ctx, VSL_STAGE_BA_LIN);
  hipLaunchKernelGGL(rig_lm_cols_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.lm_start, s.r, s.E, s.n2l,
                     s.grad_l);
  hipLaunchKernelGGL(rig_body_block_kernel, dim3(st.D.nfree, st.body_seg), dim3(256), 0, ctx->stream, st.bo_start, st.bo_obs, s.r, s.F,
                     st.body_part);
  hipLaunchKernelGGL(rig_body_block_finish_kernel, dim3((st.D.nfree * 27 + 255) / 256), dim3(256), 0, ctx->stream, st.D.nfree,
                     st.body_seg, st.body_part, s.H, s.g_b);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int rig_diag_gmax(vsl_ctx* ctx, RigState& st, RigSet& s, int slot) {
  hipLaunchKernelGGL(rig_diag_kernel, dim3(st.nb_diag), dim3(256), 0, ctx->stream, st.D.nfree, st.D.L, s.H, s.n2l, s.g_b, s.grad_l,
                     st.scale_c, st.scale_l, s.diag_c, s.diag_l, st.partials);
  hipLaunchKernelGGL(rig_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, st.partials, st.nb_diag, st.scalars, slot, 1);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

// the reduced body system of the current set; damped by inv_radius when `damp`
int rig_schur(vsl_ctx* ctx, RigState& st, bool damp, double inv_radius) {
  VslStage stage(ctx, VSL_STAGE_BA_SCHUR);
  const RigSet& s = st.cur;
  hipLaunchKernelGGL(rig_lm_groups_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.lm_start, st.lm_grp,
                     st.grp_begin, st.grp_end, s.r, s.F, s.E, damp ? s.diag_l : nullptr, inv_radius, st.W, st.Y, st.Pinv, st.bl);
  hipLaunchKernelGGL(rig_schur_block_kernel, dim3(st.D.nfree, st.D.nfree, st.schur_seg), dim3(256), 0, ctx->stream, st.bg_start,
                     st.bg_grp, st.bg_lm, st.W, st.Y, st.bl, st.schur_part);
  hipLaunchKernelGGL(rig_schur_finish_kernel, dim3(st.D.nfree, st.D.nfree), dim3(64), 0, ctx->stream, st.D.n, st.schur_seg,
                     st.schur_part, s.H, s.g_b, damp ? s.diag_c : nullptr, inv_radius, st.S, st.rhs, st.flag);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

// dc = -(S^-1 rhs) by the library's dense SPD solvers; flag[1] = factorisation succeeded
int rig_solve(vsl_ctx* ctx, RigState& st) {
  VslStage stage(ctx, VSL_STAGE_BA_SOLVE);
  const int n = st.D.n;
  if (n <= 128) return vsl_ba_chol_small_launch(ctx, n, st.S, st.rhs, st.dc, st.flag + 1);
  return vsl_chol_solve_band_dev(ctx, st.S, st.rhs, n, n, n, st.flag + 1, 0, st.dc);
}

// from dc: landmark step, finite check, scalars[2] = model cost change, candidate bodies / points, [3] / [4] = squared
// step / x norms
int rig_step(vsl_ctx* ctx, RigState& st) {
  VslStage stage(ctx, VSL_STAGE_BA_SOLVE);
  const RigSet& s = st.cur;
  hipLaunchKernelGGL(rig_backsub_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.lm_grp, st.grp_slot, st.W,
                     st.Pinv, st.bl, st.dc, st.dl, st.flag);
  hipLaunchKernelGGL(rig_model_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, st.D, st.obs_cam, st.obs_lm, st.cam_slot, s.r, s.F,
                     s.E, st.dc, st.dl, st.partials);
  hipLaunchKernelGGL(rig_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, st.partials, st.nb_obs, st.scalars, 2, 0);
  hipLaunchKernelGGL(rig_update_kernel, dim3(st.nb_upd), dim3(256), 0, ctx->stream, st.D, st.body_slot, s.bodies, s.points, st.dc,
                     st.dl, st.scale_c, st.scale_l, st.cand.bodies, st.cand.points, st.partials, st.nb_upd);
  hipLaunchKernelGGL(rig_reduce2_kernel, dim3(2), dim3(256), 0, ctx->stream, st.partials, st.nb_upd, st.scalars, 3);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

// iteration 0 of the solve: blocks at the start, Jacobi scaling from the unscaled columns, the scaled blocks, their
// columns, LM diagonals; scalars[0] = cost, [1] = max |gradient|
int rig_first_linearization(vsl_ctx* ctx, RigState& st) {
  int rc;
  if ((rc = rig_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  hipLaunchKernelGGL(rig_make_scale_kernel, dim3(st.nb_diag), dim3(256), 0, ctx->stream, st.D.nfree, st.D.L, st.cur.H, st.cur.n2l,
                     st.scale_c, st.scale_l);
  VSL_CHECK_LAUNCH(ctx);
  if ((rc = rig_linearize(ctx, st, st.cur, true, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  return rig_diag_gmax(ctx, st, st.cur, 1);
}

}  // namespace

extern "C" int vsl_ba_rig_linearize(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                                    double* S, double* g, double* cost, int* n_free_bodies) {
  RigState st;
  int rc = rig_validate(ctx, "vsl_ba_rig_linearize", prob, rig, opt, st.plan);
  if (rc) return rc;
  if (!S || !g || !cost || !n_free_bodies) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_linearize: null output");
  if (st.plan.n_fixed == 0)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_linearize: no fixed body: the gauge is free and the reduced system singular");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rig_setup(ctx, prob, rig, opt, st))) return rc;
  if ((rc = rig_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  if ((rc = rig_schur(ctx, st, false, 0.0))) return rc;
  const size_t n = st.D.n;
  std::vector<double> hS(n * n), hg(n);
  double c = 0;
  VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * n * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hg.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(S, hS.data(), 8 * n * n);
  memcpy(g, hg.data(), 8 * n);
  *cost = c;
  *n_free_bodies = st.D.nfree;
  return VSL_OK;
}

extern "C" int vsl_ba_rig_system(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                                 double inv_radius, double* S, double* rhs, double* scale_b, double* db, double* cost, int* chol_ok) {
  RigState st;
  int rc = rig_validate(ctx, "vsl_ba_rig_system", prob, rig, opt, st.plan);
  if (rc) return rc;
  if (!(inv_radius >= 0.0) || !std::isfinite(inv_radius)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_system: inv_radius %g", inv_radius);
  if (st.plan.n_fixed == 0)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_system: no fixed body: the gauge is free and the reduced system singular");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rig_setup(ctx, prob, rig, opt, st))) return rc;
  if ((rc = rig_first_linearization(ctx, st))) return rc;
  if ((rc = rig_schur(ctx, st, true, inv_radius))) return rc;
  const size_t n = st.D.n;
  std::vector<double> hS(n * n), hv(3 * n);
  double c = 0;
  int flags[2] = {0, 0};
  // (the large-system factorisation works in place: S and rhs are read before it runs)
  VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * n * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hv.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hv.data() + n, st.scale_c, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = rig_solve(ctx, st))) return rc;
  VSL_HIP(ctx, hipMemcpyAsync(hv.data() + 2 * n, st.dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(flags, st.flag, 8, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (S) memcpy(S, hS.data(), 8 * n * n);
  if (rhs) memcpy(rhs, hv.data(), 8 * n);
  if (scale_b) memcpy(scale_b, hv.data() + n, 8 * n);
  if (db) memcpy(db, hv.data() + 2 * n, 8 * n);
  if (cost) *cost = c;
  if (chol_ok) *chol_ok = flags[1] != 0;
  if (!flags[1] && !chol_ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_system: the reduced system is not positive definite");
  return VSL_OK;
}

// [upstream] ceres::Solve, TRUST_REGION / LEVENBERG_MARQUARDT / Schur on the problem whose parameter blocks are the body
// poses and the landmarks: the loop of vsl_bundle_adjust's host path (ba.hip) on the rig's kernels.
extern "C" int vsl_bundle_adjust_rig(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                                     vsl_ba_summary* summary) {
  const double t_start = now_ms();
  RigState st;
  int rc = rig_validate(ctx, "vsl_bundle_adjust_rig", prob, rig, opt, st.plan);
  if (rc) return rc;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rig_setup(ctx, prob, rig, opt, st))) return rc;
  const RigDims& D = st.D;
  vsl_ba_summary sum;
  memset(&sum, 0, sizeof(sum));
  const bool prof_was = ctx->profiling;
  double base_ms[3];
  for (int k = 0; k < 3; k++) base_ms[k] = ctx->stage_ms[VSL_STAGE_BA_LIN + k];

  if ((rc = rig_first_linearization(ctx, st))) return rc;
  double* hsc = nullptr;
  {
    void* hp = nullptr;
    if ((rc = vsl_ctx_hpinned(ctx, 256, &hp))) return rc;
    hsc = (double*)hp;
  }
  const int* hflag = (const int*)(hsc + 16);
  VSL_HIP(ctx, hipMemcpyAsync(hsc, st.scalars, 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double cost = hsc[0], gmax = hsc[1];
  sum.initial_cost = cost;

  LmState lm;
  int iteration = 0, term;
  if (opt->verbosity >= 2) lm_print_header(cost);
  // One host round trip per iteration: Schur, solve, step, candidate AND the candidate's linearisation (into the other
  // set: its cost is the candidate's cost, and an accepted step has its next linearisation already) are enqueued, one
  // copy brings the flags and scalars back, the host applies lm_policy.h.
  while (true) {
    if (iteration >= opt->max_num_iterations) { sum.termination = 0; break; }
    if ((term = lm_gate(lm, gmax)) >= 0) { sum.termination = term; break; }
    iteration++;
    if ((rc = rig_schur(ctx, st, true, 1.0 / lm.radius))) return rc;
    if ((rc = rig_solve(ctx, st))) return rc;
    if ((rc = rig_step(ctx, st))) return rc;
    if ((rc = rig_linearize(ctx, st, st.cand, true, 5))) return rc;
    if ((rc = rig_columns(ctx, st, st.cand))) return rc;
    if ((rc = rig_diag_gmax(ctx, st, st.cand, 6))) return rc;
    VSL_HIP(ctx, hipMemcpyAsync(hsc, st.scalars, 16 * sizeof(double) + 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double model_change = hsc[2], step_norm = sqrt(hsc[3]), x_norm = sqrt(hsc[4]), cand_cost = hsc[5];
    const bool ok = hflag[0] != 0 && hflag[1] != 0 && model_change > 0.0;
    const double radius_used = lm.radius;
    LmInfo info;
    const int verdict = lm_judge(lm, ok, cost, cand_cost, model_change, step_norm, x_norm, &info);
    if (verdict == LM_ACCEPTED) std::swap(st.cur, st.cand);
    if (verdict >= 0) { sum.termination = verdict; break; }
    if (verdict == LM_INVALID) {
      if (opt->verbosity >= 2) lm_print_invalid(iteration, lm.radius);
      continue;
    }
    if (opt->verbosity >= 2) lm_print_row(iteration, cand_cost, info.cost_change, gmax, step_norm, info.rel, radius_used);
    if (verdict == LM_ACCEPTED) {
      cost = cand_cost;
      gmax = hsc[6];
      sum.successful_steps++;
    }
  }
  sum.iterations = iteration;
  sum.final_cost = cost;
  // the cameras of the final bodies (the current set's were derived when it was linearised)
  VSL_HIP(ctx, hipMemcpyAsync(rig->body_poses, st.cur.bodies, sizeof(double) * 7 * (size_t)D.B, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(prob->poses, st.cur.cams, sizeof(double) * 7 * (size_t)D.C, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(prob->points, st.cur.points, sizeof(double) * 3 * (size_t)D.L, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double ms;
  int64_t cnt;
  vsl_ctx_stage_ms(ctx, VSL_STAGE_BA_LIN, &ms, &cnt);
  sum.linearize_ms = ctx->stage_ms[VSL_STAGE_BA_LIN] - base_ms[0];
  sum.schur_ms = ctx->stage_ms[VSL_STAGE_BA_SCHUR] - base_ms[1];
  sum.solve_ms = ctx->stage_ms[VSL_STAGE_BA_SOLVE] - base_ms[2];
  vsl_ctx_set_profiling(ctx, prof_was ? 1 : 0);
  sum.total_ms = now_ms() - t_start;
  if (opt->verbosity >= 1)
    fprintf(stderr, "vsl rig BA: %d free bodies, iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n", D.nfree,
            sum.iterations, sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
  if (summary) *summary = sum;
  return VSL_OK;
}

// ================================================================================================== COVARIANCES
// vsl_ba_rig_covariance / vsl_ba_rig_relative_pose_covariance (include/vslam_hip.h "covariances in rig form", DESIGN.md
// 28): the posterior of the RIG problem, H = J^T J over [free bodies | landmarks], Sigma = H^-1, at the bodies / points
// handed in.  Nothing is optimised.  The chain, all on the context's stream inside one arena loan:
//   rig_cams -> rig_linearize -> rig_columns -> rig_schur      the solve's own kernels, unscaled and undamped: the S of
//                                                              vsl_ba_rig_linearize, bit for bit
//   vsl_cov_inverse_dev (ba_cov.hip "THE SHARED LAYER")        diag S, vsl_chol_factor_dev, ba_cov_solve_kernel: the six
//                                                              unit columns of every body of Q (ba_rig_cov_plan.h)
//   rig_cov_pose_kernel       body block = the diagonal block of X, mirror entries averaged; camera block =
//                             Ad(T_c_b) Sigma_bb Ad(T_c_b)^T in registers, averaged with its transpose
//   rig_cov_landmark_kernel   one wavefront per queried landmark: P_l and the per-GROUP W from the stored F_b, E,
//                             P_l^-1 + P_l^-1 (sum_a sum_a' W_a^T [S^-1]_aa' W_a') P_l^-1
//   vsl_cov_pair_blocks_dev, vsl_ba_relpose_dev (ba_cov.hip)   joint blocks of body pairs and the pose graph's functor
//                                                              on the BODY poses
// No floating-point atomics; every sum in a fixed order: a subset query returns the bits of a full query (a column of X
// does not depend on its neighbours, ba_cov.hip), two calls return the same bits, and a pair's diagonal blocks are the
// marginal call's bits (the same average of the same two entries of the same columns).
#define RIG_COV_LM_TOL 5.6843418860808015e-14  // 2^-44: the pivot rule of ba_cov.hip for P_l

namespace {

// v (upsilon, omega) -> Ad(T_c_b) v, Ad = [[R, [t]x R], [0, R]], T_c_b = (R row-major 9, t 3): the column form of
// rig_body_jacobian
__device__ __forceinline__ void rig_adjoint_apply(const double* __restrict__ Rt, const double* v, double* o) {
  const double* R = Rt;
  const double tx = Rt[9], ty = Rt[10], tz = Rt[11];
  double ru[3], rw[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    ru[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
    rw[i] = R[3 * i] * v[3] + R[3 * i + 1] * v[4] + R[3 * i + 2] * v[5];
  }
  o[0] = ru[0] + (ty * rw[2] - tz * rw[1]);
  o[1] = ru[1] + (tz * rw[0] - tx * rw[2]);
  o[2] = ru[2] + (tx * rw[1] - ty * rw[0]);
  o[3] = rw[0];
  o[4] = rw[1];
  o[5] = rw[2];
}

// One thread per pose query (item): body block A = the diagonal block of X at the body's own columns, the two mirror
// entries averaged (the rule, and so the bits, of ba_cov_pose_kernel and of a pair block's diagonal); item_ext >= 0: the
// camera block Ad A Ad^T, B = Ad A column by column, M = B Ad^T row by row, (M + M^T) / 2.  With an identity extrinsic
// (R = I, t = 0 exactly) every product is the entry itself plus zeros: the camera block equals the body block.
__global__ __launch_bounds__(64) void rig_cov_pose_kernel(int n, int n_items, const int* __restrict__ item_q,
                                                          const int* __restrict__ item_ext, const int* __restrict__ q_free,
                                                          const double* __restrict__ X, const double* __restrict__ tcb,
                                                          const int* __restrict__ ok, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items || !*ok) return;
  const int q = item_q[t], f = q_free[q], ext = item_ext[t];
  double A[36];
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++)
      A[6 * a + b] = 0.5 * (X[vsl_cov_x_at(n, 6 * f + a, 6 * q + b)] + X[vsl_cov_x_at(n, 6 * f + b, 6 * q + a)]);
  double* o = out + 36 * (size_t)t;
  if (ext < 0) {
#pragma unroll
    for (int e = 0; e < 36; e++) o[e] = A[e];
    return;
  }
  const double* Rt = tcb + 12 * ext;
  double B[36], M[36];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double v[6], w[6];
#pragma unroll
    for (int r = 0; r < 6; r++) v[r] = A[6 * r + c];
    rig_adjoint_apply(Rt, v, w);
#pragma unroll
    for (int r = 0; r < 6; r++) B[6 * r + c] = w[r];
  }
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double w[6];
    rig_adjoint_apply(Rt, B + 6 * r, w);  // row r of B Ad^T = Ad (row r of B)^T
#pragma unroll
    for (int c = 0; c < 6; c++) M[6 * r + c] = w[c];
  }
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) o[6 * a + b] = 0.5 * (M[6 * a + b] + M[6 * b + a]);
}

// One wavefront per unique queried landmark u (landmark l = u_lm[u]).  Its groups are lm_grp[l] .. lm_grp[l + 1] of the
// rig plan, ascending free-body slot, each with its adjacent observations [grp_begin, grp_end): a landmark seen by both
// cameras of a body contributes ONE W.  F, E: the stored blocks of the unscaled rig linearisation (Huber corrector
// applied).  P_l: every lane sums all observations of the landmark in ascending order (fixed bodies first), the order
// and the bits of rig_lm_groups_kernel; W of group i by lane i mod 64, its observations ascending.  Dynamic LDS only:
// M [16 doubles] | W [18 K] | T [9 K], K = groups of the landmark (at most RCP_GMAX).
__global__ __launch_bounds__(64) void rig_cov_landmark_kernel(int n, const int* __restrict__ u_lm, const int* __restrict__ lm_start,
                                                              const int* __restrict__ lm_grp, const int* __restrict__ grp_slot,
                                                              const int* __restrict__ grp_begin, const int* __restrict__ grp_end,
                                                              const double* __restrict__ F, const double* __restrict__ E,
                                                              const int* __restrict__ qpos, const double* __restrict__ X,
                                                              const int* __restrict__ ok, double* __restrict__ out,
                                                              int* __restrict__ degenerate) {
  extern __shared__ __attribute__((aligned(16))) double rig_cov_sh[];
  if (!*ok) return;
  const int u = blockIdx.x, lane = threadIdx.x, l = u_lm[u];
  const int g0 = lm_grp[l], K = lm_grp[l + 1] - g0;
  double* M = rig_cov_sh;
  double* W = rig_cov_sh + 16;
  double* T = W + 18 * (size_t)K;
  double P[6] = {0, 0, 0, 0, 0, 0};  // xx xy xz yy yz zz
  for (int i = lm_start[l]; i < lm_start[l + 1]; i++) {
    const double* e = E + 6 * (size_t)i;
    P[0] += e[0] * e[0] + e[3] * e[3];
    P[1] += e[0] * e[1] + e[3] * e[4];
    P[2] += e[0] * e[2] + e[3] * e[5];
    P[3] += e[1] * e[1] + e[4] * e[4];
    P[4] += e[1] * e[2] + e[4] * e[5];
    P[5] += e[2] * e[2] + e[5] * e[5];
  }
  for (int i = lane; i < K; i += 64) {
    double w[18];
#pragma unroll
    for (int j = 0; j < 18; j++) w[j] = 0.0;
    for (int k = grp_begin[g0 + i]; k < grp_end[g0 + i]; k++) {
      const double* f = F + 12 * (size_t)k;
      const double* e = E + 6 * (size_t)k;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int j = 0; j < 3; j++) w[3 * a + j] += f[a] * e[j] + f[6 + a] * e[3 + j];
    }
#pragma unroll
    for (int j = 0; j < 18; j++) W[18 * i + j] = w[j];
  }
  // P = L D L^T: positive definite to working precision iff every pivot is a fair share of its diagonal entry
  const double d0 = P[0];
  const double l1 = P[1] / d0, l2 = P[2] / d0;
  const double d1 = P[3] - l1 * P[1];
  const double m = P[4] - l1 * P[2];
  const double d2 = P[5] - l2 * P[2] - (m / d1) * m;
  const double P9[9] = {P[0], P[1], P[2], P[1], P[3], P[4], P[2], P[4], P[5]};
  double Pi[9];
  const bool pd = d0 > 0.0 && d1 > RIG_COV_LM_TOL * P[3] && d2 > RIG_COV_LM_TOL * P[5] && isfinite(d0 + d1 + d2) && inv3(P9, Pi);
  if (!pd) {  // (wave-uniform: every lane holds the same P)
    if (lane < 9) out[9 * (size_t)u + lane] = __builtin_nan("");
    if (lane == 0) degenerate[u] = 1;
    return;
  }
  if (lane == 0) degenerate[u] = 0;
  __syncthreads();
  // T_i = W_i^T sum_j [S^-1]_{s(i) s(j)} W_j, j ascending
  for (int i = lane; i < K; i += 64) {
    const int row = 6 * grp_slot[g0 + i];
    double Z[18];
#pragma unroll
    for (int e = 0; e < 18; e++) Z[e] = 0.0;
    for (int j = 0; j < K; j++) {
      const int col = 6 * qpos[grp_slot[g0 + j]];
      const double* Wj = W + 18 * j;
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int b = 0; b < 6; b++) {
          const double s = X[vsl_cov_x_at(n, row + r, col + b)];
#pragma unroll
          for (int y = 0; y < 3; y++) Z[3 * r + y] += s * Wj[3 * b + y];
        }
    }
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
      for (int y = 0; y < 3; y++) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) s += W[18 * i + 3 * r + x] * Z[3 * r + y];
        T[9 * i + 3 * x + y] = s;
      }
  }
  __syncthreads();
  if (lane < 9) {
    double s = 0.0;
    for (int i = 0; i < K; i++) s += T[9 * i + lane];  // ascending slot
    M[lane] = s;
  }
  __syncthreads();
  if (lane < 9) {
    const int x = lane / 3, y = lane % 3;
    // Q = P^-1 M P^-1, entries (x, y) and (y, x); the result is symmetrised like the pose blocks
    double qxy = 0.0, qyx = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        qxy += Pi[3 * x + r] * M[3 * r + c] * Pi[3 * c + y];
        qyx += Pi[3 * y + r] * M[3 * r + c] * Pi[3 * c + x];
      }
    out[9 * (size_t)u + lane] = Pi[3 * x + y] + 0.5 * (qxy + qyx);
  }
}

// the S of vsl_ba_rig_linearize in st.S, the stored blocks in st.cur
int rig_cov_system(vsl_ctx* ctx, RigState& st) {
  int rc;
  if ((rc = rig_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  return rig_schur(ctx, st, false, 0.0);
}

const char* const RIG_NOT_PD = "%s: the reduced body system is not positive definite";

// everything of the marginal call behind the validation; host_in / host_out outlive the stream work (the caller
// synchronises on an error)
int rig_cov_run(vsl_ctx* ctx, const char* who, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                RigState& st, const RigCovPlan& P, std::vector<char>& host_in, std::vector<char>& host_out) {
  int rc;
  if ((rc = rig_setup(ctx, prob, rig, opt, st, P.total))) return rc;
  char* dev = st.extra;
  const int n = st.D.n;
  host_in.assign(P.in_bytes, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(host_in.data() + off, src, bytes);
  };
  const int one = 1;
  put(P.off_ok, &one, sizeof(int));
  put(P.off_col_unk, P.col_unk.data(), sizeof(int) * P.col_unk.size());
  put(P.off_q_free, P.q_free.data(), sizeof(int) * P.q_free.size());
  put(P.off_qpos, P.qpos.data(), sizeof(int) * P.qpos.size());
  put(P.off_item_q, P.item_q.data(), sizeof(int) * P.item_q.size());
  put(P.off_item_ext, P.item_ext.data(), sizeof(int) * P.item_ext.size());
  put(P.off_u_lm, P.u_lm.data(), sizeof(int) * P.u_lm.size());
  VSL_HIP(ctx, hipMemcpyAsync(dev, host_in.data(), P.in_bytes, hipMemcpyHostToDevice, ctx->stream));
  int* ok = (int*)(dev + P.off_ok);
  double* X = (double*)(dev + P.off_X);
  if ((rc = rig_cov_system(ctx, st))) return rc;
  if (P.nQ > 0) {
    VslStage s(ctx, VSL_STAGE_BA_SOLVE);
    const VslCovInverse inv{n, 0, 0, st.S, nullptr, (double*)(dev + P.off_Linv), (double*)(dev + P.off_Sdiag),
                            (const int*)(dev + P.off_col_unk), nullptr, P.nblk, X, ok};
    if ((rc = vsl_cov_inverse_dev(ctx, inv))) return rc;
    if (P.n_items > 0) {
      hipLaunchKernelGGL(rig_cov_pose_kernel, dim3((P.n_items + 63) / 64), dim3(64), 0, ctx->stream, n, P.n_items,
                         (const int*)(dev + P.off_item_q), (const int*)(dev + P.off_item_ext), (const int*)(dev + P.off_q_free), X,
                         st.tcb, ok, (double*)(dev + P.out_off + P.off_pose));
      VSL_CHECK_LAUNCH(ctx);
    }
  }
  if (P.nu > 0) {
    const size_t lds = sizeof(double) * (16 + 27 * (size_t)std::max(P.gmax, 1));
    hipLaunchKernelGGL(rig_cov_landmark_kernel, dim3(P.nu), dim3(64), lds, ctx->stream, n, (const int*)(dev + P.off_u_lm),
                       st.lm_start, st.lm_grp, st.grp_slot, st.grp_begin, st.grp_end, st.cur.F, st.cur.E,
                       (const int*)(dev + P.off_qpos), X, ok, (double*)(dev + P.out_off + P.off_point),
                       (int*)(dev + P.out_off + P.off_deg));
    VSL_CHECK_LAUNCH(ctx);
  }
  host_out.assign(P.out_bytes + sizeof(int), 0);
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data(), dev + P.out_off, P.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data() + P.out_bytes, ok, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int ok_host;
  memcpy(&ok_host, host_out.data() + P.out_bytes, sizeof(int));
  if (!ok_host) return vsl_fail(ctx, VSL_ERR_NUMERIC, RIG_NOT_PD, who);
  return VSL_OK;
}

int rig_rel_run(vsl_ctx* ctx, const char* who, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                RigState& st, const BaPairPlan& P, int np, std::vector<char>& host_in, std::vector<char>& host_out) {
  int rc;
  if ((rc = rig_setup(ctx, prob, rig, opt, st, P.total))) return rc;
  const PgcPlan& G = P.G;
  char* dev = st.extra;
  const int n = st.D.n;
  if (G.n != n) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: the set-up and the plan disagree", who);
  host_in.assign(P.in_bytes, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(host_in.data() + off, src, bytes);
  };
  const int one = 1;
  put(P.off_ok, &one, sizeof(int));
  put(P.off_pairs, G.pairs.data(), sizeof(PgcPairDev) * G.pairs.size());
  put(P.off_col_unk, G.col_unk.data(), sizeof(int) * G.col_unk.size());
  put(P.off_row_lo, G.row_lo.data(), sizeof(int) * G.row_lo.size());
  VSL_HIP(ctx, hipMemcpyAsync(dev, host_in.data(), P.in_bytes, hipMemcpyHostToDevice, ctx->stream));
  int* ok = (int*)(dev + P.off_ok);
  const PgcPairDev* pairs = (const PgcPairDev*)(dev + P.off_pairs);
  double* X = (double*)(dev + P.off_X);
  double* joint = (double*)(dev + P.out_off + P.off_joint);
  if ((rc = rig_cov_system(ctx, st))) return rc;
  {
    VslStage s(ctx, VSL_STAGE_BA_SOLVE);
    const VslCovInverse inv{n, 0, 0, st.S, nullptr, (double*)(dev + P.off_Linv), (double*)(dev + P.off_Sdiag),
                            (const int*)(dev + P.off_col_unk), nullptr, G.nblk, X, ok};
    if ((rc = vsl_cov_inverse_dev(ctx, inv))) return rc;
    if ((rc = vsl_cov_pair_blocks_dev(ctx, n, np, pairs, 0, nullptr, 0, X, ok, joint))) return rc;
    // the pose graph's functor on the BODY poses (PgcPairDev::na / nb are body ids)
    if ((rc = vsl_ba_relpose_dev(ctx, np, st.cur.bodies, pairs, joint, ok, (double*)(dev + P.out_off + P.off_meas),
                                 (double*)(dev + P.out_off + P.off_cov), (double*)(dev + P.out_off + P.off_info),
                                 (int*)(dev + P.out_off + P.off_sing))))
      return rc;
  }
  host_out.assign(P.out_bytes + sizeof(int), 0);
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data(), dev + P.out_off, P.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data() + P.out_bytes, ok, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int ok_host;
  memcpy(&ok_host, host_out.data() + P.out_bytes, sizeof(int));
  if (!ok_host) return vsl_fail(ctx, VSL_ERR_NUMERIC, RIG_NOT_PD, who);
  return VSL_OK;
}

}  // namespace

extern "C" int vsl_ba_rig_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                                     const int32_t* bodies, int n_body_q, double* cov_body, const int32_t* cams, int n_cam_q,
                                     double* cov_cam, const int32_t* lms, int n_lm_q, double* cov_point, int* n_degenerate) {
  const char* who = "vsl_ba_rig_covariance";
  std::vector<char> host_in, host_out;  // read / written by copies on the stream: they outlive the synchronisation below
  RigCovPlan P;
  int rc;
  {
    RigState st;  // holds the loan of the context's arena
    if ((rc = rig_validate(ctx, who, prob, rig, opt, st.plan))) return rc;
    if ((n_body_q > 0 && !cov_body) || (n_cam_q > 0 && !cov_cam) || (n_lm_q > 0 && !cov_point))
      return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null output", who);
    try {
      const int e = rcp_plan(st.plan, rig->n_bodies, prob->n_cams, prob->n_lms, prob->cam_intr, bodies, n_body_q, cams, n_cam_q, lms,
                             n_lm_q, P);
      if (e != RCP_OK) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: %s (%d)", who, rcp_message(e), P.first_bad);
    } catch (const std::bad_alloc&) {
      return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    if (st.plan.n_fixed == 0)
      return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: no fixed body: the gauge is free and the reduced system singular", who);
    if (n_body_q == 0 && n_cam_q == 0 && n_lm_q == 0) {  // nothing is launched
      if (n_degenerate) *n_degenerate = 0;
      return VSL_OK;
    }
    VSL_HIP(ctx, hipSetDevice(ctx->device));
    try {
      rc = rig_cov_run(ctx, who, prob, rig, opt, st, P, host_in, host_out);
    } catch (const std::bad_alloc&) {
      rc = vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    // an error return may leave kernels and copies queued that use the arena and the host buffers: drain the stream
    // before the loan ends (a later solve on this context gets the same block)
    if (rc) (void)hipStreamSynchronize(ctx->stream);
  }
  if (rc) return rc;
  const double* pose = (const double*)(host_out.data() + P.off_pose);
  const double* point = (const double*)(host_out.data() + P.off_point);
  const int* deg = (const int*)(host_out.data() + P.off_deg);
  if (n_body_q > 0) memcpy(cov_body, pose, 36 * sizeof(double) * (size_t)n_body_q);
  if (n_cam_q > 0) memcpy(cov_cam, pose + 36 * (size_t)n_body_q, 36 * sizeof(double) * (size_t)n_cam_q);
  int nd = 0;
  for (int q = 0; q < n_lm_q; q++) {
    memcpy(cov_point + 9 * (size_t)q, point + 9 * (size_t)P.lm_q2u[q], 9 * sizeof(double));
    nd += deg[P.lm_q2u[q]] ? 1 : 0;
  }
  if (n_degenerate) *n_degenerate = nd;
  return VSL_OK;
}

extern "C" int vsl_ba_rig_relative_pose_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig,
                                                   const vsl_ba_options* opt, const int32_t* body_a, const int32_t* body_b,
                                                   int n_pairs, double* joint, double* meas, double* cov, double* info,
                                                   int* n_singular) {
  const char* who = "vsl_ba_rig_relative_pose_covariance";
  std::vector<char> host_in, host_out;
  BaPairPlan P;
  int rc;
  {
    RigState st;  // holds the loan of the context's arena
    if ((rc = rig_validate(ctx, who, prob, rig, opt, st.plan))) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!body_a || !body_b))) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null argument or negative count", who);
    try {
      int bad = 0;
      switch (rcp_pair_plan(st.plan, rig->n_bodies, rig->body_fixed, body_a, body_b, n_pairs, P, &bad)) {
        case PGC_PAIR_RANGE: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d (%d, %d): body out of range", who, bad, body_a[bad], body_b[bad]);
        case PGC_PAIR_SAME: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d names body %d twice", who, bad, body_a[bad]);
        case PGC_PAIR_BOTH_FIXED: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d (%d, %d): both bodies are fixed", who, bad, body_a[bad], body_b[bad]);
        default: break;
      }
    } catch (const std::bad_alloc&) {
      return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    if (st.plan.n_fixed == 0)
      return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: no fixed body: the gauge is free and the reduced system singular", who);
    if (n_pairs == 0 || (!joint && !meas && !cov && !info)) {  // nothing is launched
      if (n_singular) *n_singular = 0;
      return VSL_OK;
    }
    VSL_HIP(ctx, hipSetDevice(ctx->device));
    try {
      rc = rig_rel_run(ctx, who, prob, rig, opt, st, P, n_pairs, host_in, host_out);
    } catch (const std::bad_alloc&) {
      rc = vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // as above: drain before the loan ends
  }
  if (rc) return rc;
  const size_t np = (size_t)n_pairs;
  if (joint) memcpy(joint, host_out.data() + P.off_joint, sizeof(double) * 144 * np);
  if (meas) memcpy(meas, host_out.data() + P.off_meas, sizeof(double) * 6 * np);
  if (cov) memcpy(cov, host_out.data() + P.off_cov, sizeof(double) * 36 * np);
  if (info) memcpy(info, host_out.data() + P.off_info, sizeof(double) * 36 * np);
  const int* sing = (const int*)(host_out.data() + P.off_sing);
  int ns = 0;
  for (size_t q = 0; q < np; q++) ns += sing[q] ? 1 : 0;
  if (n_singular) *n_singular = ns;
  return VSL_OK;
}
