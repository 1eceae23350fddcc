// ba_rig.hip -- rig-constrained bundle adjustment: ONE SE(3) block per stereo frame (the body), the calibrated
// extrinsics T_b_c held fixed, T_w_c = T_w_b * T_b_c[cam_intr].  vsl_bundle_adjust_rig, and the two parity hooks
// vsl_ba_rig_linearize / vsl_ba_rig_system (include/vslam_hip.h "rig-constrained bundle adjustment").
// vsl_global_bundle_adjust_rig / vsl_ba_rig_map_system run the same chain for whole maps: the reduced body
// system gathered over co-visible body pairs only (rig_schur_pairs_kernel) into dense / band / cyclic-band storage.
// The covariances of the rig posterior (vsl_ba_rig_covariance, vsl_ba_rig_relative_pose_covariance) are
// the section "COVARIANCES" of this file; the extrinsics as unknowns (vsl_bundle_adjust_rig_ext) the section
// "EXTRINSICS" behind them, and the covariances of THAT posterior (vsl_ba_rig_ext_covariance) the section
// "EXTRINSICS: COVARIANCES" at its end.
//
// Residual, camera models, Huber corrector and cost are those of vsl_bundle_adjust (ba_device.h); what changes is the
// pose block an observation differentiates against.  With T_c_b = T_b_c^-1 = (R, t),
//   T_w_b exp(d) T_b_c = T_w_c exp(Ad(T_c_b) d),   Ad = [[R, [t]x R], [0, R]]  in the (upsilon, omega) order,
// so F_b = F_c Ad = [F_u R, (F_u [t]x + F_w) R], formed in registers per observation (rig_body_jacobian, ba_device.h).
// Everything downstream of the stored blocks works on BODY columns: Jacobi scaling, LM damping, the Schur complement, the
// step.  So everything that does not depend on how a landmark's observations group into bodies runs on the kernels of
// ba.hip, through the plain-pointer launchers of ba_state.h (a kernel is launched from the file that defines it), with
// the body slot of a camera (cam_slot) where the free solver has its free-camera index.
//
// The chain (all reductions in a fixed order: two solves give the same bits; no floating-point atomics anywhere).
// OWN = a kernel of this file, ba = a kernel of ba.hip:
//   OWN rig_cams_kernel         camera poses from the bodies
//   ba  ba_linearize_kernel<RIG> r, F_b, E per observation (robustified, scaled when scales are given), cost partials
//   ba  ba_reduce_kernel        sums / maxima of partials into the scalars
//   ba  ba_lm_cols_kernel       per landmark: squared column norms of E, E^T r
//   OWN rig_body_block_kernel   per free body and segment: partial H = sum F_b^T F_b, g = sum F_b^T r over a slice of the
//                               body's observations.  NOT ba_cam_block_kernel: this one sums the lanes of a wave by
//                               shuffle and then the four waves in order, that one goes through a 256-wide LDS tree -- two
//                               summation orders, two sets of bits, and both solvers' results are pinned
//   ba  ba_cam_block_finish_kernel  adds the segments of a block in order
//   ba  ba_make_scale_kernel, ba_diag_kernel   Jacobi scaling (once), LM diagonals and max |gradient|
//   OWN rig_lm_groups_kernel    per landmark: P (+ damping), P^-1, b; per (landmark, free body) GROUP W = sum F_b^T E over
//                               the group's observations -- a landmark seen by both cameras of a body is one group of two
//                               -- and Y = W P^-1
//   OWN rig_schur_block_kernel  workgroups per 6 x 6 block (a, b), a >= b, of the reduced system and segment: walks a slice
//                               of the groups of body a (ascending landmark), finds body b's group of the same landmark by
//                               bisection, sums Y_a W_b^T per thread, reduces in a fixed tree; rig_schur_finish_kernel adds
//                               the segments in order and writes the block and its mirror image (S is exactly symmetric).
//                               A landmark with any number of observations is the same code: the per-landmark kernels
//                               loop, the gather sees one group per body.
//   ba  dense SPD solve         ba_chol_small_kernel up to 128 unknowns, the dense panel factorisation of chol.hip beyond
//   OWN rig_backsub_kernel      landmark step from the groups' W, finite check
//   ba  ba_model_kernel, ba_update_kernel, ba_reduce2_kernel   model cost change, T_w_b * exp(step) (the pose blocks are
//                               the bodies), squared step / x norms
// The LM loop is lm_speculative_loop (lm_policy.h), the one vsl_bundle_adjust's host path runs: host-decided with ONE
// synchronisation per iteration, the candidate linearised speculatively into a second set of blocks.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "vsl_common.h"
#include "lm_policy.h"
#include "dev_arena.h"
#include "ba_device.h"
#include "ba_state.h"
#include "ba_rig_plan.h"
#include "ba_rig_cov_plan.h"
#include "pgo_cov_plan.h"

namespace {

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

// per landmark: P = sum E^T E (+ diag_l * inv_radius), P^-1, b = sum E^T r; per group of the landmark W = sum F^T E
// (6 x 3 row-major) over the group's observations and Y = W P^-1.  A landmark whose P cannot be inverted gets
// P^-1 = 0: it contributes nothing to S and does not move.
__global__ __launch_bounds__(256) void rig_lm_groups_kernel(BaDims D, const int* __restrict__ lm_start, const int* __restrict__ lm_grp,
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

// ---- the map route (vsl_global_bundle_adjust_rig): the gather over the CO-VISIBLE pairs only
// grid (items): item = (listed pair, segment) of RigMapPlan; the workgroup sums every nseg-th 256-group slice of body
// hi's groups, exactly as rig_schur_block_kernel does for its block (hi, lo): Y_hi W_lo^T over the landmarks both bodies
// see and, on the diagonal, Y_hi b_l, into spart[item][42].  A pair that shares no landmark is not in the list: no
// workgroup walks it.
__global__ __launch_bounds__(256) void rig_schur_pairs_kernel(const int* __restrict__ item_pair, const int* __restrict__ pair_first,
                                                              const int* __restrict__ pair_hi, const int* __restrict__ pair_lo,
                                                              const int* __restrict__ bg_start, const int* __restrict__ bg_grp,
                                                              const int* __restrict__ bg_lm, const double* __restrict__ W,
                                                              const double* __restrict__ Y, const double* __restrict__ bl,
                                                              double* __restrict__ spart) {
  __shared__ double sh[4 * 42];
  const int item = blockIdx.x, pr = item_pair[item];
  const int seg = item - pair_first[pr], nseg = pair_first[pr + 1] - pair_first[pr];
  const int a = pair_hi[pr], b = pair_lo[pr];
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
    double* o = spart + (size_t)item * 42;
#pragma unroll
    for (int k = 0; k < 42; k++) o[k] = acc[k];
  }
}

// grid (listed pairs), 64 threads: the segments of pair (hi, lo) in order, then the block into the storage of the layout
// (rig_map_entry_at, ba_rig_plan.h): dense with its mirror image; the band forms keep the lower triangle, the cyclic one
// its wrap-around blocks transposed at negative columns.  The storage was cleared before (rig_schur): what no listed
// pair owns is zero.  hi == lo also: rhs = g - sum.  Pair 0 arms the two flags of the step.
__global__ __launch_bounds__(64) void rig_schur_band_finish_kernel(int form, int ldS, int offS, int nfree, int half_cyc,
                                                                   const int* __restrict__ pair_first, const int* __restrict__ pair_hi,
                                                                   const int* __restrict__ pair_lo, const double* __restrict__ spart,
                                                                   const double* __restrict__ H, const double* __restrict__ g_b,
                                                                   const double* __restrict__ diag_c, double inv_radius,
                                                                   double* __restrict__ S, double* __restrict__ rhs,
                                                                   int* __restrict__ flag) {
  const int pr = blockIdx.x, a = pair_hi[pr], b = pair_lo[pr];
  if (pr == 0 && threadIdx.x < 2) flag[threadIdx.x] = 1;
  const int e = threadIdx.x;
  if (e >= 42) return;
  const int first = pair_first[pr], nseg = pair_first[pr + 1] - first;
  const double* p = spart + (size_t)first * 42;
  double sum = 0;
  for (int q = 0; q < nseg; q++) sum += p[(size_t)q * 42 + e];
  if (e < 36) {
    const int i = e / 6, j = e - 6 * i;
    if (a != b) {
      S[rig_map_entry_at(form, ldS, offS, nfree, half_cyc, a, b, i, j)] = -sum;
      if (form == 0) S[(size_t)(6 * b + j) * ldS + 6 * a + i] = -sum;
    } else if (i >= j) {
      double h = H[36 * (size_t)a + e];
      if (i == j && diag_c) h += diag_c[6 * (size_t)a + i] * inv_radius;
      const double v = h - sum;
      S[rig_map_entry_at(form, ldS, offS, nfree, half_cyc, a, a, i, j)] = v;
      if (form == 0) S[(size_t)(6 * a + j) * ldS + 6 * a + i] = v;
    }
  } else if (a == b) {
    rhs[6 * (size_t)a + (e - 36)] = g_b[6 * (size_t)a + (e - 36)] - sum;
  }
}

// delta_l = -P^-1 (b_l + sum over the landmark's groups of W^T delta_body); flag[0] cleared on a non-finite step
__global__ __launch_bounds__(256) void rig_backsub_kernel(BaDims D, const int* __restrict__ lm_grp, const int* __restrict__ grp_slot,
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

// ------------------------------------------------------------------------------------------------ host state
// what a linearisation point owns: the LM loop keeps two and swaps them when a step is accepted
struct RigSet {
  double *bodies = nullptr, *cams = nullptr, *points = nullptr;
  double *r = nullptr, *F = nullptr, *E = nullptr, *n2l = nullptr, *grad_l = nullptr, *H = nullptr, *g_b = nullptr;
  double *diag_c = nullptr, *diag_l = nullptr;
};

struct RigState {
  BaDims D;  // of the shared kernels: C cameras, nfree free BODIES, n = 6 nfree
  int B = 0, G = 0;  // bodies, (landmark, free body) groups
  RigPlan plan;
  DevArena arena;
  int nb_obs = 1;
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
  // the map route (vsl_global_bundle_adjust_rig): S in the layout's storage, the gather over the listed pairs
  bool map = false;
  RigMapPlan mp;
  int *item_pair = nullptr, *pair_first = nullptr, *pair_hi = nullptr, *pair_lo = nullptr;
  double* S_eff() { return S + (map ? mp.layout.offS : 0); }
};

// the layout switches of the map route: those of the general path's host loop (ba.hip ba_layout_switches), no rule of its own
BaLayoutSwitches rig_map_switches(vsl_ctx* ctx) {
  static const bool env_no_cyclic = getenv("VSL_BA_NO_CYCLIC") != nullptr;
  BaLayoutSwitches sw;
  sw.allow_band = true;
  sw.force_dense = ctx->ba_force_dense;
  sw.no_cyclic = ctx->ba_no_cyclic || env_no_cyclic;
  sw.schur_atomics = ctx->ba_schur_atomics;
  sw.chol_no_bcr = ctx->chol_no_bcr;
  sw.chol_no_fused = ctx->chol_no_fused;
  return sw;
}

// mp: the map route -- the plan comes from rig_map_plan_build (slots in band order where the layout renumbers)
int rig_validate(vsl_ctx* ctx, const char* who, const vsl_ba_problem* p, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                 RigPlan& plan, RigMapPlan* mp = nullptr) {
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
  int st;
  if (mp) {
    try {
      st = rig_map_plan_build(in, rig_map_switches(ctx), plan, *mp);
    } catch (const std::bad_alloc&) {
      return vsl_fail(ctx, VSL_ERR_NOMEM, "%s: out of host memory", who);
    }
  } else {
    st = rig_plan_build(in, plan);
  }
  if (st != RIG_PLAN_OK) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: %s (index %d)", who, rig_plan_message(st), plan.first_bad);
  return VSL_OK;
}

// plan -> ONE arena (the context's), uploads; synchronises
int rig_setup(vsl_ctx* ctx, const vsl_ba_problem* p, const vsl_ba_rig* rig, const vsl_ba_options* opt, RigState& st,
              size_t extra_bytes = 0) {
  const RigPlan& hp = st.plan;
  BaDims& D = st.D;
  D.C = p->n_cams; D.L = p->n_lms; D.O = p->n_obs;
  D.nfree = hp.n_free; D.n = 6 * hp.n_free;
  D.model0 = p->cam_model[0]; D.model1 = p->cam_model[1];
  D.use_huber = opt->use_huber; D.huber = opt->huber_parameter;
  st.B = rig->n_bodies; st.G = hp.n_groups();
  const size_t C = D.C, B = st.B, L = D.L, O = D.O, G = st.G, n = D.n, nf = D.nfree;
  st.nb_obs = (int)((O + 255) / 256);
  // partials of the shared launchers (ba_state.h): observations, 2 x pose blocks / landmarks, LM diagonal entries
  const size_t nb_upd = (std::max(B, L) + 255) / 256, nb_diag = (std::max(n, 3 * L) + 255) / 256;
  // a workgroup of the two gathers takes about two 256-entry trips of the longest body list (at most 64 segments)
  int max_obs = 0, max_grp = 0;
  for (int b = 0; b < hp.n_free; b++) {
    max_obs = std::max(max_obs, hp.bo_start[b + 1] - hp.bo_start[b]);
    max_grp = std::max(max_grp, hp.bg_start[b + 1] - hp.bg_start[b]);
  }
  st.body_seg = std::min(64, std::max(1, (max_obs + 511) / 512));
  st.schur_seg = std::min(64, std::max(1, (max_grp + 511) / 512));  // (the map route takes its segments per pair from the plan)
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
  plan.add(st.S, st.map ? st.mp.layout.s_elems : n * n); plan.add(st.rhs, n); plan.add(st.dc, n); plan.add(st.dl, 3 * L);
  plan.add(st.partials, std::max(std::max((size_t)st.nb_obs, 2 * nb_upd), nb_diag));
  plan.add(st.scalars, 32);  // 16 doubles, then the flags
  plan.add(st.body_part, nf * st.body_seg * 27); plan.add(st.schur_part, st.map ? (size_t)st.mp.n_items() * 42 : nf * (nf + 1) / 2 * st.schur_seg * 42);
  plan.add(st.cam_intr, C); plan.add(st.cam_body, C); plan.add(st.cam_slot, C); plan.add(st.body_slot, B);
  plan.add(st.obs_cam, O); plan.add(st.obs_lm, O);
  plan.add(st.lm_start, L + 1); plan.add(st.lm_grp, L + 1);
  plan.add(st.grp_slot, G); plan.add(st.grp_begin, G); plan.add(st.grp_end, G);
  plan.add(st.bg_start, nf + 1); plan.add(st.bg_grp, G); plan.add(st.bg_lm, G);
  plan.add(st.bo_start, nf + 1); plan.add(st.bo_obs, hp.bo_obs.size());
  if (extra_bytes) plan.add(st.extra, extra_bytes);
  if (st.map) {
    plan.add(st.item_pair, st.mp.item_pair.size()); plan.add(st.pair_first, st.mp.pair_first.size());
    plan.add(st.pair_hi, st.mp.pair_hi.size()); plan.add(st.pair_lo, st.mp.pair_lo.size());
  }
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
  if (st.map) {
    VSL_HIP(ctx, up(st.item_pair, st.mp.item_pair.data(), 4 * st.mp.item_pair.size()));
    VSL_HIP(ctx, up(st.pair_first, st.mp.pair_first.data(), 4 * st.mp.pair_first.size()));
    VSL_HIP(ctx, up(st.pair_hi, st.mp.pair_hi.data(), 4 * st.mp.pair_hi.size()));
    VSL_HIP(ctx, up(st.pair_lo, st.mp.pair_lo.data(), 4 * st.mp.pair_lo.size()));
  }
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
  if ((rc = vsl_ba_linearize_launch(ctx, st.D, s.cams, s.points, st.intr, st.tcb, st.cam_intr, st.cam_slot, st.obs_cam, st.obs_lm,
                                    st.obs_uv, scaled ? st.scale_c : nullptr, scaled ? st.scale_l : nullptr, s.r, s.F, s.E,
                                    st.partials)))
    return rc;
  return vsl_ba_reduce_launch(ctx, st.partials, st.nb_obs, st.scalars, cost_slot, false);
}

int rig_columns(vsl_ctx* ctx, RigState& st, RigSet& s) {
  VslStage stage(ctx, VSL_STAGE_BA_LIN);
  int rc = vsl_ba_lm_cols_launch(ctx, st.D.L, st.lm_start, s.r, s.E, s.n2l, s.grad_l);
  if (rc) return rc;
  hipLaunchKernelGGL(rig_body_block_kernel, dim3(st.D.nfree, st.body_seg), dim3(256), 0, ctx->stream, st.bo_start, st.bo_obs, s.r, s.F,
                     st.body_part);
  return vsl_ba_block_finish_launch(ctx, st.D.nfree, st.body_seg, st.body_part, s.H, s.g_b);
}

int rig_diag_gmax(vsl_ctx* ctx, RigState& st, RigSet& s, int slot) {
  return vsl_ba_diag_gmax_launch(ctx, st.D.nfree, st.D.L, s.H, s.n2l, s.g_b, s.grad_l, st.scale_c, st.scale_l, s.diag_c, s.diag_l,
                                 st.partials, st.scalars, slot);
}

// the reduced body system of the current set; damped by inv_radius when `damp`
int rig_schur(vsl_ctx* ctx, RigState& st, bool damp, double inv_radius) {
  VslStage stage(ctx, VSL_STAGE_BA_SCHUR);
  const RigSet& s = st.cur;
  hipLaunchKernelGGL(rig_lm_groups_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.lm_start, st.lm_grp,
                     st.grp_begin, st.grp_end, s.r, s.F, s.E, damp ? s.diag_l : nullptr, inv_radius, st.W, st.Y, st.Pinv, st.bl);
  if (st.map) {
    // The solver destroys S in place and the finish kernel writes the blocks of the listed pairs only: the WHOLE storage
    // is cleared per build (in-band blocks of pairs that share no landmark, the padding rows, the slack), as ba_schur does
    const BaLayout& y = st.mp.layout;
    VSL_HIP(ctx, hipMemsetAsync(st.S, 0, sizeof(double) * y.s_elems, ctx->stream));
    hipLaunchKernelGGL(rig_schur_pairs_kernel, dim3(st.mp.n_items()), dim3(256), 0, ctx->stream, st.item_pair, st.pair_first, st.pair_hi,
                       st.pair_lo, st.bg_start, st.bg_grp, st.bg_lm, st.W, st.Y, st.bl, st.schur_part);
    hipLaunchKernelGGL(rig_schur_band_finish_kernel, dim3(st.mp.n_pairs()), dim3(64), 0, ctx->stream, st.mp.form, y.ldS, y.offS,
                       st.D.nfree, st.mp.half_cyc, st.pair_first, st.pair_hi, st.pair_lo, st.schur_part, s.H, s.g_b,
                       damp ? s.diag_c : nullptr, inv_radius, st.S, st.rhs, st.flag);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }
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
  if (st.map) {  // dense, band or ring by the layout (dense: ldS = bw = n, no offset -- the call below)
    const BaLayout& y = st.mp.layout;
    return vsl_chol_solve_band_dev(ctx, st.S_eff(), st.rhs, n, y.ldS, y.bw, st.flag + 1, y.cyclic ? 1 : 0, st.dc);
  }
  return vsl_chol_solve_band_dev(ctx, st.S, st.rhs, n, n, n, st.flag + 1, 0, st.dc);
}

// from dc: landmark step, finite check, scalars[2] = model cost change, candidate bodies / points, [3] / [4] = squared
// step / x norms
int rig_step(vsl_ctx* ctx, RigState& st) {
  VslStage stage(ctx, VSL_STAGE_BA_SOLVE);
  const RigSet& s = st.cur;
  hipLaunchKernelGGL(rig_backsub_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.lm_grp, st.grp_slot, st.W,
                     st.Pinv, st.bl, st.dc, st.dl, st.flag);
  int rc = vsl_ba_model_launch(ctx, st.D.O, st.obs_cam, st.obs_lm, st.cam_slot, s.r, s.F, s.E, st.dc, st.dl, st.partials);
  if (rc) return rc;
  if ((rc = vsl_ba_reduce_launch(ctx, st.partials, st.nb_obs, st.scalars, 2, false))) return rc;
  // (the pose blocks of the update are the bodies)
  return vsl_ba_update_launch(ctx, st.B, st.D.L, st.body_slot, s.bodies, s.points, st.dc, st.dl, st.scale_c, st.scale_l,
                              st.cand.bodies, st.cand.points, st.partials, st.scalars, 3);
}

// iteration 0 of the solve: blocks at the start, Jacobi scaling from the unscaled columns, the scaled blocks, their
// columns, LM diagonals; scalars[0] = cost, [1] = max |gradient|
int rig_first_linearization(vsl_ctx* ctx, RigState& st) {
  int rc;
  if ((rc = rig_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  if ((rc = vsl_ba_make_scale_launch(ctx, st.D.nfree, st.D.L, st.cur.H, st.cur.n2l, st.scale_c, st.scale_l))) return rc;
  if ((rc = rig_linearize(ctx, st, st.cur, true, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  return rig_diag_gmax(ctx, st, st.cur, 1);
}

// the S of vsl_ba_rig_linearize (unscaled, undamped) in st.S, the stored blocks in st.cur
int rig_unscaled_system(vsl_ctx* ctx, RigState& st) {
  int rc;
  if ((rc = rig_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rig_columns(ctx, st, st.cur))) return rc;
  return rig_schur(ctx, st, false, 0.0);
}

// An error behind the set-up may leave kernels and copies queued that use the borrowed arena (and the caller's host
// buffers): the stream is drained before the loan ends -- a later solve on this context gets the same block.  Returns rc.
int rig_drain(vsl_ctx* ctx, int rc) {
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
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
  const size_t n = st.D.n;
  std::vector<double> hS(n * n), hg(n);  // (the targets of queued copies: they outlive the drain below)
  double c = 0;
  auto run = [&]() -> int {
    int e;
    if ((e = rig_unscaled_system(ctx, st))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * n * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hg.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSL_OK;
  };
  if ((rc = run())) return rig_drain(ctx, rc);
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
  const size_t n = st.D.n;
  std::vector<double> hS(n * n), hv(3 * n);  // (the targets of queued copies: they outlive the drain below)
  double c = 0;
  int flags[2] = {0, 0};
  auto run = [&]() -> int {
    int e;
    if ((e = rig_first_linearization(ctx, st))) return e;
    if ((e = rig_schur(ctx, st, true, inv_radius))) return e;
    // (the large-system factorisation works in place: S and rhs are read before it runs)
    VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * n * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + n, st.scale_c, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((e = rig_solve(ctx, st))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + 2 * n, st.dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(flags, st.flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSL_OK;
  };
  if ((rc = run())) return rig_drain(ctx, rc);
  if (S) memcpy(S, hS.data(), 8 * n * n);
  if (rhs) memcpy(rhs, hv.data(), 8 * n);
  if (scale_b) memcpy(scale_b, hv.data() + n, 8 * n);
  if (db) memcpy(db, hv.data() + 2 * n, 8 * n);
  if (cost) *cost = c;
  if (chol_ok) *chol_ok = flags[1] != 0;
  if (!flags[1] && !chol_ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_system: the reduced system is not positive definite");
  return VSL_OK;
}

namespace {

// vsl_bundle_adjust_rig behind the set-up
int rig_solve_run(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt, RigState& st,
                  double t_start, vsl_ba_summary* summary) {
  int rc;
  const BaDims& D = st.D;
  vsl_ba_summary sum;
  memset(&sum, 0, sizeof(sum));
  const BaSolveTimes times(ctx, t_start);

  if ((rc = rig_first_linearization(ctx, st))) return rc;
  double sc[16];  // [0] cost, [1] max |gradient| at the start
  int unused_flags[2];
  if ((rc = ba_fetch_step(ctx, st.scalars, sc, unused_flags))) return rc;
  sum.initial_cost = sc[0];

  // lm_speculative_loop: Schur, solve, step, candidate AND the candidate's linearisation (into the other set: its cost is
  // the candidate's cost, and an accepted step has its next linearisation already) are enqueued, one copy brings the
  // flags and scalars back, the host applies lm_policy.h.
  auto enqueue = [&](double radius) -> int {
    int e;
    if ((e = rig_schur(ctx, st, true, 1.0 / radius))) return e;
    if ((e = rig_solve(ctx, st))) return e;
    if ((e = rig_step(ctx, st))) return e;
    if ((e = rig_linearize(ctx, st, st.cand, true, 5))) return e;
    if ((e = rig_columns(ctx, st, st.cand))) return e;
    return rig_diag_gmax(ctx, st, st.cand, 6);
  };
  auto fetch = [&](double* s16, int* flags) -> int { return ba_fetch_step(ctx, st.scalars, s16, flags); };
  auto settle = [&](bool accepted) {
    if (accepted) std::swap(st.cur, st.cand);
  };
  LmLoopResult lm;
  if ((rc = lm_speculative_loop(opt->max_num_iterations, opt->verbosity, sc[0], sc[1], enqueue, fetch, settle, &lm))) return rc;
  sum.iterations = lm.iterations;
  sum.successful_steps = lm.successful_steps;
  sum.termination = lm.termination;
  sum.final_cost = lm.final_cost;
  // the cameras of the final bodies (the current set's were derived when it was linearised)
  VSL_HIP(ctx, hipMemcpyAsync(rig->body_poses, st.cur.bodies, sizeof(double) * 7 * (size_t)st.B, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(prob->poses, st.cur.cams, sizeof(double) * 7 * (size_t)D.C, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(prob->points, st.cur.points, sizeof(double) * 3 * (size_t)D.L, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  char label[64];
  snprintf(label, sizeof(label), "vsl rig %sBA: %d free bodies,", st.map ? "map " : "", D.nfree);
  ba_finish_summary(ctx, times, opt->verbosity, label, sum, summary);
  return VSL_OK;
}

}  // namespace

// [upstream] ceres::Solve, TRUST_REGION / LEVENBERG_MARQUARDT / Schur on the problem whose parameter blocks are the body
// poses and the landmarks: the loop of vsl_bundle_adjust's host path (lm_speculative_loop) on the rig's chain.
extern "C" int vsl_bundle_adjust_rig(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                                     vsl_ba_summary* summary) {
  const double t_start = now_ms();
  RigState st;  // holds the loan of the context's arena
  int rc = rig_validate(ctx, "vsl_bundle_adjust_rig", prob, rig, opt, st.plan);
  if (rc) return rc;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rig_setup(ctx, prob, rig, opt, st))) return rc;
  rc = rig_solve_run(ctx, prob, rig, opt, st, t_start, summary);
  return rc ? rig_drain(ctx, rc) : VSL_OK;
}

// ---- the map route: the same chain and the same LM loop; the reduced body system is gathered over the
// co-visible body pairs only (rig_schur_pairs_kernel), stored as ba_reduced_layout says (dense / band in reverse
// Cuthill-McKee order of the bodies / cyclic band in the bodies' own order) and solved by vsl_chol_solve_band_dev.
namespace {

// validation and plan of the map route; the read-out of vsl_ctx_last_ba_layout
int rig_map_begin(vsl_ctx* ctx, const char* who, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                  RigState& st) {
  st.map = true;
  const int rc = rig_validate(ctx, who, prob, rig, opt, st.plan, &st.mp);
  if (rc) return rc;
  ctx->last_ba_s_elems = (int64_t)st.mp.layout.s_elems;
  ctx->last_ba_banded = st.mp.form;
  ctx->last_ba_bw = st.mp.layout.bw;
  return VSL_OK;
}

}  // namespace

extern "C" int vsl_global_bundle_adjust_rig(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig,
                                            const vsl_ba_options* opt, vsl_ba_summary* summary) {
  const double t_start = now_ms();
  RigState st;  // holds the loan of the context's arena
  int rc = rig_map_begin(ctx, "vsl_global_bundle_adjust_rig", prob, rig, opt, st);
  if (rc) return rc;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rig_setup(ctx, prob, rig, opt, st))) return rc;
  rc = rig_solve_run(ctx, prob, rig, opt, st, t_start, summary);
  return rc ? rig_drain(ctx, rc) : VSL_OK;
}

extern "C" int vsl_ba_rig_map_system(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                                     double inv_radius, double* S, double* rhs, double* scale_b, double* db, double* cost,
                                     int* chol_ok) {
  RigState st;
  int rc = rig_map_begin(ctx, "vsl_ba_rig_map_system", prob, rig, opt, st);
  if (rc) return rc;
  if (!(inv_radius >= 0.0) || !std::isfinite(inv_radius)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_map_system: inv_radius %g", inv_radius);
  if (st.plan.n_fixed == 0)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_map_system: no fixed body: the gauge is free and the reduced system singular");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rig_setup(ctx, prob, rig, opt, st))) return rc;
  const size_t n = st.D.n, se = st.mp.layout.s_elems;
  std::vector<double> hS(se), hv(3 * n);  // (the targets of queued copies: they outlive the drain below)
  double c = 0;
  int flags[2] = {0, 0};
  auto run = [&]() -> int {
    int e;
    if ((e = rig_first_linearization(ctx, st))) return e;
    if ((e = rig_schur(ctx, st, true, inv_radius))) return e;
    // (the factorisation works in place: the storage and rhs are read before it runs)
    VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * se, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + n, st.scale_c, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((e = rig_solve(ctx, st))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + 2 * n, st.dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(flags, st.flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSL_OK;
  };
  if ((rc = run())) return rig_drain(ctx, rc);
  // the band expanded on the host, slots back to ascending body id
  if (S) rig_map_expand(st.mp, st.D.nfree, hS.data(), S);
  if (rhs) rig_map_unpermute(st.mp, st.D.nfree, hv.data(), rhs);
  if (scale_b) rig_map_unpermute(st.mp, st.D.nfree, hv.data() + n, scale_b);
  if (db) rig_map_unpermute(st.mp, st.D.nfree, hv.data() + 2 * n, db);
  if (cost) *cost = c;
  if (chol_ok) *chol_ok = flags[1] != 0;
  if (!flags[1] && !chol_ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_map_system: the reduced system is not positive definite");
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
  if ((rc = rig_unscaled_system(ctx, st))) return rc;
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
  if ((rc = rig_unscaled_system(ctx, st))) return rc;
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

// ================================================================================================== EXTRINSICS
// vsl_bundle_adjust_rig_ext / vsl_ba_rig_ext_linearize / vsl_ba_rig_ext_system (include/vslam_hip.h "rig bundle
// adjustment with the extrinsics as unknowns"): the rig solve with T_b_c[k] <- T_b_c[k] exp(eps_k) of the
// free blocks estimated beside the bodies.  T_w_c = T_w_b T_b_c[k] exp(eps_k), so the block of an observation against
// eps_k is the CAMERA Jacobian F_x = F_c, before the adjoint that makes it F_b.  A free block is one more pose slot
// behind the free bodies (RigExtPlan, ba_rig_plan.h): the solver's pose-block array is [bodies | block 0 | block 1], the
// cameras and Ad(T_b_c^-1) are derived from it per linearisation, and the kernels of ba.hip that work on slots (scaling,
// diagonals, update, norms) and the gathers of this file that work on per-slot lists (rig_body_block_kernel,
// rig_schur_block_kernel, rig_backsub_kernel) run unchanged on n_slots = free bodies + free blocks.  New here:
//   rigx_linearize_kernel      r, F_b, F_x, E per observation (robustified, scaled), cost partials
//   rigx_border_kernel         per (slot, free block, segment): a body slot sums H_be = sum F_b^T F_x over its observations
//                              in that block (36); the block's own slot sums H_ee (21) and g_e (6); the other free block's
//                              slot sums nothing (H_ee' = 0: no observation is in both) and its zeros are written
//   rigx_border_finish_kernel  segments in order -> Hbe per (slot, block), H and g of the extrinsic slots
//   rigx_lm_groups_kernel      rig_lm_groups_kernel on index lists: an extrinsic group's observations are not adjacent
//   rigx_schur_finish_kernel   rig_schur_finish_kernel plus S_eb = H_eb - sum Y_e W_b^T on the border blocks
//   rigx_model_kernel          model cost change with both pose slots of an observation
// No free body: the body launches (grids over free bodies) are skipped, nothing else changes.  Every sum in a fixed
// order, no atomics.  ext_free = {0, 0} never gets here: the three calls hand over to the rig calls.
namespace {

__global__ __launch_bounds__(256) void rigx_linearize_kernel(BaDims D, int B, const double* __restrict__ pose_blocks,
                                                             const double* __restrict__ cams, const double* __restrict__ points,
                                                             const double* __restrict__ intr, const int* __restrict__ cam_intr,
                                                             const int* __restrict__ cam_slot, const int* __restrict__ cam_eslot,
                                                             const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                                             const double* __restrict__ obs_uv, const double* __restrict__ scale_c,
                                                             const double* __restrict__ scale_l, double* __restrict__ r_out,
                                                             double* __restrict__ F_out, double* __restrict__ Fx_out,
                                                             double* __restrict__ E_out, double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double c = 0;
  if (i < D.O) {
    const int cam = obs_cam[i], lm = obs_lm[i], k = cam_intr[cam];
    double r[2], F[12], Fx[12], E[6];
    residual_blocks(k ? D.model1 : D.model0, intr + 8 * k, cams + 7 * (size_t)cam, points + 3 * (size_t)lm, obs_uv + 2 * (size_t)i, r,
                    F, E, true);
#pragma unroll
    for (int j = 0; j < 12; j++) Fx[j] = F[j];
    // T_c_b = (R^T, -R^T t) of the extrinsic at this linearisation point
    const double* e = pose_blocks + 7 * (size_t)(B + k);
    double Re[9], Rt[12];
    quat_R(e, Re);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) Rt[3 * a + b] = Re[3 * b + a];
#pragma unroll
    for (int a = 0; a < 3; a++) Rt[9 + a] = -(Rt[3 * a] * e[4] + Rt[3 * a + 1] * e[5] + Rt[3 * a + 2] * e[6]);
    rig_body_jacobian(Rt, F);
    const double s = r[0] * r[0] + r[1] * r[1];
    double rho0 = s, rho1 = 1.0;
    if (D.use_huber) huber(s, D.huber, rho0, rho1);
    c = 0.5 * rho0;
    const double sr = sqrt(rho1);
    r_out[2 * (size_t)i] = r[0] * sr;
    r_out[2 * (size_t)i + 1] = r[1] * sr;
    const int fb = cam_slot[cam], fe = cam_eslot[cam];
    for (int j = 0; j < 6; j++) {
      const double sb = (scale_c && fb >= 0) ? scale_c[6 * fb + j] : 1.0;
      F_out[12 * (size_t)i + j] = F[j] * sr * sb;
      F_out[12 * (size_t)i + 6 + j] = F[6 + j] * sr * sb;
      const double se = (scale_c && fe >= 0) ? scale_c[6 * fe + j] : 1.0;
      Fx_out[12 * (size_t)i + j] = Fx[j] * sr * se;
      Fx_out[12 * (size_t)i + 6 + j] = Fx[6 + j] * sr * se;
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

// grid (slots, free blocks, segments): a workgroup sums every `segments`-th 256-observation slice of its slot's
// observation list into part[((slot, block), segment)][36].  Slot of a body: H_be = sum F_b^T F_x (6 x 6 row-major) over
// the observations whose camera is of that block.  The block's own slot: [0, 21) the upper triangle of sum F_x^T F_x,
// [21, 27) sum F_x^T r, the rest zero.  The slot of the other free block: 36 zeros.
__global__ __launch_bounds__(256) void rigx_border_kernel(int nfb, const int* __restrict__ so_start, const int* __restrict__ so_obs,
                                                          const int* __restrict__ obs_cam, const int* __restrict__ cam_eslot,
                                                          const double* __restrict__ r, const double* __restrict__ F,
                                                          const double* __restrict__ Fx, double* __restrict__ part) {
  __shared__ double sh[4 * 36];
  const int s = blockIdx.x, kx = blockIdx.y, ne = gridDim.y, seg = blockIdx.z, nseg = gridDim.z;
  const int es = nfb + kx;
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; k++) acc[k] = 0;
  if (s < nfb) {
    for (int q = so_start[s] + seg * 256 + threadIdx.x; q < so_start[s + 1]; q += 256 * nseg) {
      const int i = so_obs[q];
      if (cam_eslot[obs_cam[i]] != es) continue;
      const double* f = F + 12 * (size_t)i;
      const double* x = Fx + 12 * (size_t)i;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) acc[6 * a + b] += f[a] * x[b] + f[6 + a] * x[6 + b];
    }
  } else if (s == es) {
    for (int q = so_start[s] + seg * 256 + threadIdx.x; q < so_start[s + 1]; q += 256 * nseg) {
      const int i = so_obs[q];
      const double* x = Fx + 12 * (size_t)i;
      const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) acc[k++] += x[a] * x[b] + x[6 + a] * x[6 + b];
#pragma unroll
      for (int a = 0; a < 6; a++) acc[21 + a] += x[a] * r0 + x[6 + a] * r1;
    }
  }
  rig_block_sum<36>(acc, sh);
  if (threadIdx.x == 0) {
    double* o = part + (((size_t)s * ne + kx) * nseg + seg) * 36;
#pragma unroll
    for (int k = 0; k < 36; k++) o[k] = acc[k];
  }
}

// grid (slots, free blocks), 64 threads: the segments in order.  Hbe[(slot, block)][36] for every slot but the block's
// own (H_be of a body, the zeros of H_ee'); the block's own slot gets H (6 x 6, mirrored) and g
__global__ __launch_bounds__(64) void rigx_border_finish_kernel(int nfb, int nseg, const double* __restrict__ part,
                                                                double* __restrict__ Hbe, double* __restrict__ H,
                                                                double* __restrict__ g) {
  const int s = blockIdx.x, kx = blockIdx.y, ne = gridDim.y, e = threadIdx.x;
  if (e >= 36) return;
  const double* p = part + ((size_t)s * ne + kx) * nseg * 36;
  double v = 0;
  for (int q = 0; q < nseg; q++) v += p[(size_t)q * 36 + e];
  if (s != nfb + kx) {
    Hbe[((size_t)s * ne + kx) * 36 + e] = v;
  } else if (e >= 21) {
    if (e < 27) g[6 * (size_t)s + (e - 21)] = v;
  } else {
    int a = 0, rem = e;  // e-th entry of the upper triangle, row-major
    while (rem >= 6 - a) {
      rem -= 6 - a;
      a++;
    }
    const int b = a + rem;
    H[36 * (size_t)s + 6 * a + b] = v;
    H[36 * (size_t)s + 6 * b + a] = v;
  }
}

// rig_lm_groups_kernel with every group's observations named through an index list (grp_first / grp_obs); a group of a
// slot >= nfb is an extrinsic group and reads F_x
__global__ __launch_bounds__(256) void rigx_lm_groups_kernel(BaDims D, int nfb, const int* __restrict__ lm_start,
                                                             const int* __restrict__ lm_grp, const int* __restrict__ grp_slot,
                                                             const int* __restrict__ grp_first, const int* __restrict__ grp_obs,
                                                             const double* __restrict__ r, const double* __restrict__ F,
                                                             const double* __restrict__ Fx, const double* __restrict__ E,
                                                             const double* __restrict__ diag_l, double inv_radius,
                                                             double* __restrict__ W, double* __restrict__ Y,
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
    const double* Fs = grp_slot[g] < nfb ? F : Fx;
    double w[18];
    for (int j = 0; j < 18; j++) w[j] = 0;
    for (int q = grp_first[g]; q < grp_first[g + 1]; q++) {
      const int i = grp_obs[q];
      const double* f = Fs + 12 * (size_t)i;
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

// grid (slots, slots), 64 threads: rig_schur_finish_kernel with the border.  Block (a, b), a > b, of an extrinsic slot a
// (body slot or the other block b): S_ab = H_eb - sum, H_eb = Hbe[(b, a - nfb)]^T; two body slots: -sum; the diagonal as
// there.  Mirrored: S is exactly symmetric.  Workgroup (0, 0) arms the two flags of the step.
__global__ __launch_bounds__(64) void rigx_schur_finish_kernel(int n, int nfb, int ne, int nseg, const double* __restrict__ spart,
                                                               const double* __restrict__ H, const double* __restrict__ g_b,
                                                               const double* __restrict__ Hbe, const double* __restrict__ diag_c,
                                                               double inv_radius, double* __restrict__ S, double* __restrict__ rhs,
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
      const double v = a >= nfb ? Hbe[((size_t)b * ne + (a - nfb)) * 36 + 6 * j + i] - sum : -sum;
      S[at] = v;
      S[mirror] = v;
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

// model cost change partials -(J d)^T (r + J d / 2) with J d = F_b d_body + F_x d_ext + E d_l
__global__ __launch_bounds__(256) void rigx_model_kernel(int O, const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                                         const int* __restrict__ cam_slot, const int* __restrict__ cam_eslot,
                                                         const double* __restrict__ r, const double* __restrict__ F,
                                                         const double* __restrict__ Fx, const double* __restrict__ E,
                                                         const double* __restrict__ dc, const double* __restrict__ dl,
                                                         double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v = 0;
  if (i < O) {
    const int cam = obs_cam[i], fb = cam_slot[cam], fe = cam_eslot[cam], lm = obs_lm[i];
    const double* f = F + 12 * (size_t)i;
    const double* x = Fx + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    double m0 = 0, m1 = 0;
    if (fb >= 0)
      for (int j = 0; j < 6; j++) {
        m0 += f[j] * dc[6 * fb + j];
        m1 += f[6 + j] * dc[6 * fb + j];
      }
    if (fe >= 0)
      for (int j = 0; j < 6; j++) {
        m0 += x[j] * dc[6 * fe + j];
        m1 += x[6 + j] * dc[6 * fe + j];
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

// ---- host state of the extrinsics solve
struct RigxSet {
  double *blocks = nullptr, *cams = nullptr, *points = nullptr;  // blocks: [bodies | extrinsic 0 | extrinsic 1], 7 each
  double *r = nullptr, *F = nullptr, *Fx = nullptr, *E = nullptr, *n2l = nullptr, *grad_l = nullptr, *H = nullptr, *g = nullptr;
  double *diag_c = nullptr, *diag_l = nullptr;
  double* Hbe = nullptr;  // [(slot, free block)][36]: H_be of the body slots, the zeros of H_ee'
};

struct RigxState {
  BaDims D;  // of the shared kernels: nfree = SLOTS (free bodies + free blocks), n = 6 nfree
  int B = 0, G = 0, nfb = 0, ne = 0;
  RigPlan plan;
  RigExtPlan xp;
  DevArena arena;
  int nb_obs = 1, obs_seg = 1, grp_seg = 1;
  RigxSet cur, cand;
  double *intr = nullptr, *obs_uv = nullptr, *scale_c = nullptr, *scale_l = nullptr, *W = nullptr, *Y = nullptr, *Pinv = nullptr;
  double *bl = nullptr, *S = nullptr, *rhs = nullptr, *dc = nullptr, *dl = nullptr, *partials = nullptr;
  double *scalars = nullptr, *body_part = nullptr, *border_part = nullptr, *schur_part = nullptr;
  int* flag = nullptr;
  int *cam_intr = nullptr, *cam_body = nullptr, *cam_slot = nullptr, *cam_eslot = nullptr, *pose_free = nullptr;
  int *obs_cam = nullptr, *obs_lm = nullptr, *lm_start = nullptr, *lm_grp = nullptr, *grp_slot = nullptr, *grp_first = nullptr;
  int *grp_obs = nullptr, *sg_start = nullptr, *sg_grp = nullptr, *sg_lm = nullptr, *so_start = nullptr, *so_obs = nullptr;
  char* extra = nullptr;  // the covariance call's share of the arena (behind everything else: no other offset moves)
};

int rigx_validate(vsl_ctx* ctx, const char* who, const vsl_ba_problem* p, const vsl_ba_rig* rig, const uint8_t* ext_free,
                  const double* T_b_c, const vsl_ba_options* opt, RigxState& st) {
  if (!p || !rig || !opt || !ext_free || !T_b_c || !p->poses || !p->cam_intr || !p->intr || !p->points || !p->obs_cam || !p->obs_lm ||
      !p->obs_uv || !rig->body_poses || !rig->body_fixed || !rig->cam_body)
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null pointer", who);
  for (int k = 0; k < 2; k++)
    if (p->cam_model[k] < 0 || p->cam_model[k] > 3) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: unknown camera model %d", who, p->cam_model[k]);
  RigPlanIn in;
  in.n_cams = p->n_cams; in.n_lms = p->n_lms; in.n_obs = p->n_obs;
  in.cam_intr = p->cam_intr; in.obs_cam = p->obs_cam; in.obs_lm = p->obs_lm;
  in.n_bodies = rig->n_bodies; in.body_fixed = rig->body_fixed; in.cam_body = rig->cam_body; in.T_b_c = T_b_c;
  int rc;
  try {
    rc = rig_ext_plan_build(in, ext_free, st.plan, st.xp);
  } catch (const std::bad_alloc&) {
    return vsl_fail(ctx, VSL_ERR_NOMEM, "%s: out of host memory", who);
  }
  if (rc != RIG_PLAN_OK) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: %s (index %d)", who, rig_plan_message(rc), st.plan.first_bad);
  return VSL_OK;
}

// plans -> ONE arena (the context's), uploads; synchronises
int rigx_setup(vsl_ctx* ctx, const vsl_ba_problem* p, const vsl_ba_rig* rig, const vsl_ba_options* opt, RigxState& st,
               size_t extra_bytes = 0) {
  const RigPlan& hp = st.plan;
  const RigExtPlan& xp = st.xp;
  BaDims& D = st.D;
  D.C = p->n_cams; D.L = p->n_lms; D.O = p->n_obs;
  D.nfree = xp.n_slots; D.n = 6 * xp.n_slots;
  D.model0 = p->cam_model[0]; D.model1 = p->cam_model[1];
  D.use_huber = opt->use_huber; D.huber = opt->huber_parameter;
  st.B = rig->n_bodies; st.G = xp.n_groups(); st.nfb = hp.n_free; st.ne = xp.n_ext;
  const size_t C = D.C, B = st.B, L = D.L, O = D.O, G = st.G, n = D.n, ns = D.nfree, ne = st.ne, nfb = st.nfb;
  st.nb_obs = (int)((O + 255) / 256);
  const size_t nb_upd = (std::max(B + 2, L) + 255) / 256, nb_diag = (std::max(n, 3 * L) + 255) / 256;
  // segments as the rig solve takes them (rig_segments), from the longest slot list: the extrinsic slots' are the long ones
  int max_obs = 0, max_grp = 0;
  for (int s = 0; s < xp.n_slots; s++) {
    max_obs = std::max(max_obs, xp.so_start[s + 1] - xp.so_start[s]);
    max_grp = std::max(max_grp, xp.sg_start[s + 1] - xp.sg_start[s]);
  }
  st.obs_seg = rig_segments(max_obs);
  st.grp_seg = rig_segments(max_grp);
  ArenaPlan plan(80);
  for (RigxSet* s : {&st.cur, &st.cand}) {
    plan.add(s->blocks, 7 * (B + 2)); plan.add(s->cams, 7 * C); plan.add(s->points, 3 * L);
    plan.add(s->r, 2 * O); plan.add(s->F, 12 * O); plan.add(s->Fx, 12 * O); plan.add(s->E, 6 * O);
    plan.add(s->n2l, 3 * L); plan.add(s->grad_l, 3 * L); plan.add(s->H, 36 * ns); plan.add(s->g, n);
    plan.add(s->diag_c, n); plan.add(s->diag_l, 3 * L); plan.add(s->Hbe, 36 * ns * ne);
  }
  plan.add(st.intr, 16); plan.add(st.obs_uv, 2 * O);
  plan.add(st.scale_c, n); plan.add(st.scale_l, 3 * L);
  plan.add(st.W, 18 * G); plan.add(st.Y, 18 * G); plan.add(st.Pinv, 9 * L); plan.add(st.bl, 3 * L);
  plan.add(st.S, n * n); plan.add(st.rhs, n); plan.add(st.dc, n); plan.add(st.dl, 3 * L);
  plan.add(st.partials, std::max(std::max((size_t)st.nb_obs, 2 * nb_upd), nb_diag));
  plan.add(st.scalars, 32);  // 16 doubles, then the flags
  plan.add(st.body_part, std::max<size_t>(1, nfb) * st.obs_seg * 27);
  plan.add(st.border_part, ns * ne * st.obs_seg * 36);
  plan.add(st.schur_part, ns * (ns + 1) / 2 * st.grp_seg * 42);
  plan.add(st.cam_intr, C); plan.add(st.cam_body, C); plan.add(st.cam_slot, C); plan.add(st.cam_eslot, C);
  plan.add(st.pose_free, B + 2); plan.add(st.obs_cam, O); plan.add(st.obs_lm, O);
  plan.add(st.lm_start, L + 1); plan.add(st.lm_grp, L + 1);
  plan.add(st.grp_slot, G); plan.add(st.grp_first, G + 1); plan.add(st.grp_obs, xp.grp_obs.size());
  plan.add(st.sg_start, ns + 1); plan.add(st.sg_grp, G); plan.add(st.sg_lm, G);
  plan.add(st.so_start, ns + 1); plan.add(st.so_obs, xp.so_obs.size());
  if (extra_bytes) plan.add(st.extra, extra_bytes);
  hipError_t e = st.arena.acquire(ctx, ArenaPolicy::BORROWED, plan);
  if (e != hipSuccess) return vsl_fail(ctx, e == hipErrorOutOfMemory ? VSL_ERR_NOMEM : VSL_ERR_HIP, "rig bundle adjustment (extrinsics): %zu bytes of device memory: %s", plan.total(), hipGetErrorString(e));
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
  VSL_HIP(ctx, up(st.cur.blocks, rig->body_poses, 56 * B));
  VSL_HIP(ctx, up(st.cur.blocks + 7 * B, hp.T_b_c, sizeof(hp.T_b_c)));  // normalised by the plan
  VSL_HIP(ctx, up(st.cur.points, p->points, 24 * L));
  VSL_HIP(ctx, up(st.intr, p->intr, 128));
  VSL_HIP(ctx, up(st.obs_uv, uv.data(), 16 * O));
  VSL_HIP(ctx, up(st.cam_intr, p->cam_intr, 4 * C));
  VSL_HIP(ctx, up(st.cam_body, rig->cam_body, 4 * C));
  VSL_HIP(ctx, up(st.cam_slot, hp.cam_slot.data(), 4 * C));
  VSL_HIP(ctx, up(st.cam_eslot, xp.cam_eslot.data(), 4 * C));
  VSL_HIP(ctx, up(st.pose_free, xp.pose_free.data(), 4 * (B + 2)));
  VSL_HIP(ctx, up(st.obs_cam, hp.obs_cam.data(), 4 * O));
  VSL_HIP(ctx, up(st.obs_lm, hp.obs_lm.data(), 4 * O));
  VSL_HIP(ctx, up(st.lm_start, hp.lm_start.data(), 4 * (L + 1)));
  VSL_HIP(ctx, up(st.lm_grp, xp.lm_grp.data(), 4 * (L + 1)));
  VSL_HIP(ctx, up(st.grp_slot, xp.grp_slot.data(), 4 * G));
  VSL_HIP(ctx, up(st.grp_first, xp.grp_first.data(), 4 * (G + 1)));
  VSL_HIP(ctx, up(st.grp_obs, xp.grp_obs.data(), 4 * xp.grp_obs.size()));
  VSL_HIP(ctx, up(st.sg_start, xp.sg_start.data(), 4 * (ns + 1)));
  VSL_HIP(ctx, up(st.sg_grp, xp.sg_grp.data(), 4 * G));
  VSL_HIP(ctx, up(st.sg_lm, xp.sg_lm.data(), 4 * G));
  VSL_HIP(ctx, up(st.so_start, xp.so_start.data(), 4 * (ns + 1)));
  VSL_HIP(ctx, up(st.so_obs, xp.so_obs.data(), 4 * xp.so_obs.size()));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the uploads read host vectors that die here
  return VSL_OK;
}

// cameras (rig_cams_kernel reads the extrinsics from the tail of the pose blocks), blocks and cost (-> scalars[cost_slot])
int rigx_linearize(vsl_ctx* ctx, RigxState& st, RigxSet& s, bool scaled, int cost_slot) {
  VslStage stage(ctx, VSL_STAGE_BA_LIN);
  hipLaunchKernelGGL(rig_cams_kernel, dim3((st.D.C + 255) / 256), dim3(256), 0, ctx->stream, st.D.C, s.blocks, s.blocks + 7 * (size_t)st.B,
                     st.cam_body, st.cam_intr, s.cams);
  hipLaunchKernelGGL(rigx_linearize_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, st.D, st.B, s.blocks, s.cams, s.points, st.intr,
                     st.cam_intr, st.cam_slot, st.cam_eslot, st.obs_cam, st.obs_lm, st.obs_uv, scaled ? st.scale_c : nullptr,
                     scaled ? st.scale_l : nullptr, s.r, s.F, s.Fx, s.E, st.partials);
  VSL_CHECK_LAUNCH(ctx);
  return vsl_ba_reduce_launch(ctx, st.partials, st.nb_obs, st.scalars, cost_slot, false);
}

// landmark columns; H, g of the body slots (skipped without a free body) and of the extrinsic slots; the border blocks
int rigx_columns(vsl_ctx* ctx, RigxState& st, RigxSet& s) {
  VslStage stage(ctx, VSL_STAGE_BA_LIN);
  int rc = vsl_ba_lm_cols_launch(ctx, st.D.L, st.lm_start, s.r, s.E, s.n2l, s.grad_l);
  if (rc) return rc;
  if (st.nfb > 0) {
    hipLaunchKernelGGL(rig_body_block_kernel, dim3(st.nfb, st.obs_seg), dim3(256), 0, ctx->stream, st.so_start, st.so_obs, s.r, s.F,
                       st.body_part);
    if ((rc = vsl_ba_block_finish_launch(ctx, st.nfb, st.obs_seg, st.body_part, s.H, s.g))) return rc;
  }
  hipLaunchKernelGGL(rigx_border_kernel, dim3(st.D.nfree, st.ne, st.obs_seg), dim3(256), 0, ctx->stream, st.nfb, st.so_start, st.so_obs,
                     st.obs_cam, st.cam_eslot, s.r, s.F, s.Fx, st.border_part);
  hipLaunchKernelGGL(rigx_border_finish_kernel, dim3(st.D.nfree, st.ne), dim3(64), 0, ctx->stream, st.nfb, st.obs_seg, st.border_part,
                     s.Hbe, s.H, s.g);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int rigx_diag_gmax(vsl_ctx* ctx, RigxState& st, RigxSet& s, int slot) {
  return vsl_ba_diag_gmax_launch(ctx, st.D.nfree, st.D.L, s.H, s.n2l, s.g, s.grad_l, st.scale_c, st.scale_l, s.diag_c, s.diag_l,
                                 st.partials, st.scalars, slot);
}

// the reduced system over [free bodies | free blocks] of the current set; damped by inv_radius when `damp`
int rigx_schur(vsl_ctx* ctx, RigxState& st, bool damp, double inv_radius) {
  VslStage stage(ctx, VSL_STAGE_BA_SCHUR);
  const RigxSet& s = st.cur;
  const int ns = st.D.nfree;
  hipLaunchKernelGGL(rigx_lm_groups_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.nfb, st.lm_start, st.lm_grp,
                     st.grp_slot, st.grp_first, st.grp_obs, s.r, s.F, s.Fx, s.E, damp ? s.diag_l : nullptr, inv_radius, st.W, st.Y,
                     st.Pinv, st.bl);
  hipLaunchKernelGGL(rig_schur_block_kernel, dim3(ns, ns, st.grp_seg), dim3(256), 0, ctx->stream, st.sg_start, st.sg_grp, st.sg_lm, st.W,
                     st.Y, st.bl, st.schur_part);
  hipLaunchKernelGGL(rigx_schur_finish_kernel, dim3(ns, ns), dim3(64), 0, ctx->stream, st.D.n, st.nfb, st.ne, st.grp_seg, st.schur_part,
                     s.H, s.g, s.Hbe, damp ? s.diag_c : nullptr, inv_radius, st.S, st.rhs, st.flag);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int rigx_solve(vsl_ctx* ctx, RigxState& st) {
  VslStage stage(ctx, VSL_STAGE_BA_SOLVE);
  const int n = st.D.n;
  if (n <= 128) return vsl_ba_chol_small_launch(ctx, n, st.S, st.rhs, st.dc, st.flag + 1);
  return vsl_chol_solve_band_dev(ctx, st.S, st.rhs, n, n, n, st.flag + 1, 0, st.dc);
}

int rigx_step(vsl_ctx* ctx, RigxState& st) {
  VslStage stage(ctx, VSL_STAGE_BA_SOLVE);
  const RigxSet& s = st.cur;
  hipLaunchKernelGGL(rig_backsub_kernel, dim3((st.D.L + 255) / 256), dim3(256), 0, ctx->stream, st.D, st.lm_grp, st.grp_slot, st.W,
                     st.Pinv, st.bl, st.dc, st.dl, st.flag);
  hipLaunchKernelGGL(rigx_model_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, st.D.O, st.obs_cam, st.obs_lm, st.cam_slot,
                     st.cam_eslot, s.r, s.F, s.Fx, s.E, st.dc, st.dl, st.partials);
  VSL_CHECK_LAUNCH(ctx);
  int rc = vsl_ba_reduce_launch(ctx, st.partials, st.nb_obs, st.scalars, 2, false);
  if (rc) return rc;
  // (the pose blocks of the update are the bodies and the two extrinsics)
  return vsl_ba_update_launch(ctx, st.B + 2, st.D.L, st.pose_free, s.blocks, s.points, st.dc, st.dl, st.scale_c, st.scale_l,
                              st.cand.blocks, st.cand.points, st.partials, st.scalars, 3);
}

int rigx_first_linearization(vsl_ctx* ctx, RigxState& st) {
  int rc;
  if ((rc = rigx_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rigx_columns(ctx, st, st.cur))) return rc;
  if ((rc = vsl_ba_make_scale_launch(ctx, st.D.nfree, st.D.L, st.cur.H, st.cur.n2l, st.scale_c, st.scale_l))) return rc;
  if ((rc = rigx_linearize(ctx, st, st.cur, true, 0))) return rc;
  if ((rc = rigx_columns(ctx, st, st.cur))) return rc;
  return rigx_diag_gmax(ctx, st, st.cur, 1);
}

// T_b_c normalised as the plan does it: what a call without a free block hands back
void rigx_normalised(const double* T_b_c, double* out) {
  for (int k = 0; k < 2; k++) {
    const double* T = T_b_c + 7 * k;
    double nn = 0;
    for (int j = 0; j < 4; j++) nn += T[j] * T[j];
    nn = std::sqrt(nn);
    for (int j = 0; j < 4; j++) out[7 * k + j] = T[j] / nn;
    for (int j = 4; j < 7; j++) out[7 * k + j] = T[j];
  }
}

}  // namespace

extern "C" int vsl_ba_rig_ext_linearize(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const uint8_t* ext_free,
                                        const double* T_b_c, const vsl_ba_options* opt, double* S, double* g, double* cost,
                                        int* n_free_bodies, int* n_free_ext) {
  if (!ctx) return VSL_ERR_INVALID;
  if (!rig || !ext_free || !T_b_c) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_ext_linearize: null pointer");
  if (!S || !g || !cost || !n_free_bodies || !n_free_ext) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_ext_linearize: null output");
  if (!ext_free[0] && !ext_free[1]) {  // the rig call itself
    vsl_ba_rig held = *rig;
    held.T_b_c = T_b_c;
    int nfb = 0;
    const int rc = vsl_ba_rig_linearize(ctx, prob, &held, opt, S, g, cost, &nfb);
    if (rc) return rc;
    *n_free_bodies = nfb;
    *n_free_ext = 0;
    return VSL_OK;
  }
  RigxState st;
  int rc = rigx_validate(ctx, "vsl_ba_rig_ext_linearize", prob, rig, ext_free, T_b_c, opt, st);
  if (rc) return rc;
  if (st.plan.n_fixed == 0)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_ext_linearize: no fixed body: the gauge is free and the reduced system singular");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rigx_setup(ctx, prob, rig, opt, st))) return rc;
  const size_t n = st.D.n;
  std::vector<double> hS(n * n), hg(n);  // (the targets of queued copies: they outlive the drain below)
  double c = 0;
  auto run = [&]() -> int {
    int e;
    if ((e = rigx_linearize(ctx, st, st.cur, false, 0))) return e;
    if ((e = rigx_columns(ctx, st, st.cur))) return e;
    if ((e = rigx_schur(ctx, st, false, 0.0))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * n * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hg.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSL_OK;
  };
  if ((rc = run())) return rig_drain(ctx, rc);
  memcpy(S, hS.data(), 8 * n * n);
  memcpy(g, hg.data(), 8 * n);
  *cost = c;
  *n_free_bodies = st.nfb;
  *n_free_ext = st.ne;
  return VSL_OK;
}

extern "C" int vsl_ba_rig_ext_system(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const uint8_t* ext_free,
                                     const double* T_b_c, const vsl_ba_options* opt, double inv_radius, double* S, double* rhs,
                                     double* scale, double* d, double* cost, int* chol_ok) {
  if (!ctx) return VSL_ERR_INVALID;
  if (!rig || !ext_free || !T_b_c) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_ext_system: null pointer");
  if (!ext_free[0] && !ext_free[1]) {  // the rig call itself
    vsl_ba_rig held = *rig;
    held.T_b_c = T_b_c;
    return vsl_ba_rig_system(ctx, prob, &held, opt, inv_radius, S, rhs, scale, d, cost, chol_ok);
  }
  RigxState st;
  int rc = rigx_validate(ctx, "vsl_ba_rig_ext_system", prob, rig, ext_free, T_b_c, opt, st);
  if (rc) return rc;
  if (!(inv_radius >= 0.0) || !std::isfinite(inv_radius)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_rig_ext_system: inv_radius %g", inv_radius);
  if (st.plan.n_fixed == 0)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_ext_system: no fixed body: the gauge is free and the reduced system singular");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rigx_setup(ctx, prob, rig, opt, st))) return rc;
  const size_t n = st.D.n;
  std::vector<double> hS(n * n), hv(3 * n);  // (the targets of queued copies: they outlive the drain below)
  double c = 0;
  int flags[2] = {0, 0};
  auto run = [&]() -> int {
    int e;
    if ((e = rigx_first_linearization(ctx, st))) return e;
    if ((e = rigx_schur(ctx, st, true, inv_radius))) return e;
    // (the large-system factorisation works in place: S and rhs are read before it runs)
    VSL_HIP(ctx, hipMemcpyAsync(hS.data(), st.S, 8 * n * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data(), st.rhs, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + n, st.scale_c, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((e = rigx_solve(ctx, st))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + 2 * n, st.dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(flags, st.flag, 8, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSL_OK;
  };
  if ((rc = run())) return rig_drain(ctx, rc);
  if (S) memcpy(S, hS.data(), 8 * n * n);
  if (rhs) memcpy(rhs, hv.data(), 8 * n);
  if (scale) memcpy(scale, hv.data() + n, 8 * n);
  if (d) memcpy(d, hv.data() + 2 * n, 8 * n);
  if (cost) *cost = c;
  if (chol_ok) *chol_ok = flags[1] != 0;
  if (!flags[1] && !chol_ok) return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_rig_ext_system: the reduced system is not positive definite");
  return VSL_OK;
}

extern "C" int vsl_bundle_adjust_rig_ext(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const uint8_t* ext_free,
                                         double* T_b_c_io, const vsl_ba_options* opt, vsl_ba_summary* summary) {
  const double t_start = now_ms();
  if (!ctx) return VSL_ERR_INVALID;
  if (!rig || !ext_free || !T_b_c_io) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_bundle_adjust_rig_ext: null pointer");
  if (!ext_free[0] && !ext_free[1]) {  // the rig call itself; the extrinsics come back normalised and otherwise untouched
    vsl_ba_rig held = *rig;
    held.T_b_c = T_b_c_io;
    const int rc = vsl_bundle_adjust_rig(ctx, prob, &held, opt, summary);
    if (rc) return rc;
    double nrm[14];
    rigx_normalised(T_b_c_io, nrm);
    memcpy(T_b_c_io, nrm, sizeof(nrm));
    return VSL_OK;
  }
  RigxState st;  // holds the loan of the context's arena
  int rc = rigx_validate(ctx, "vsl_bundle_adjust_rig_ext", prob, rig, ext_free, T_b_c_io, opt, st);
  if (rc) return rc;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = rigx_setup(ctx, prob, rig, opt, st))) return rc;
  double ext[14];  // (the target of a queued copy: it outlives the drain below)
  auto run = [&]() -> int {
    int e;
    const BaDims& D = st.D;
    vsl_ba_summary sum;
    memset(&sum, 0, sizeof(sum));
    const BaSolveTimes times(ctx, t_start);
    if ((e = rigx_first_linearization(ctx, st))) return e;
    double sc[16];  // [0] cost, [1] max |gradient| at the start
    int unused_flags[2];
    if ((e = ba_fetch_step(ctx, st.scalars, sc, unused_flags))) return e;
    sum.initial_cost = sc[0];
    // the loop of vsl_bundle_adjust_rig on the chain above
    auto enqueue = [&](double radius) -> int {
      int q;
      if ((q = rigx_schur(ctx, st, true, 1.0 / radius))) return q;
      if ((q = rigx_solve(ctx, st))) return q;
      if ((q = rigx_step(ctx, st))) return q;
      if ((q = rigx_linearize(ctx, st, st.cand, true, 5))) return q;
      if ((q = rigx_columns(ctx, st, st.cand))) return q;
      return rigx_diag_gmax(ctx, st, st.cand, 6);
    };
    auto fetch = [&](double* s16, int* flags) -> int { return ba_fetch_step(ctx, st.scalars, s16, flags); };
    auto settle = [&](bool accepted) {
      if (accepted) std::swap(st.cur, st.cand);
    };
    LmLoopResult lm;
    if ((e = lm_speculative_loop(opt->max_num_iterations, opt->verbosity, sc[0], sc[1], enqueue, fetch, settle, &lm))) return e;
    sum.iterations = lm.iterations;
    sum.successful_steps = lm.successful_steps;
    sum.termination = lm.termination;
    sum.final_cost = lm.final_cost;
    VSL_HIP(ctx, hipMemcpyAsync(rig->body_poses, st.cur.blocks, sizeof(double) * 7 * (size_t)st.B, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(ext, st.cur.blocks + 7 * (size_t)st.B, sizeof(ext), hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(prob->poses, st.cur.cams, sizeof(double) * 7 * (size_t)D.C, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(prob->points, st.cur.points, sizeof(double) * 3 * (size_t)D.L, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(T_b_c_io, ext, sizeof(ext));
    char label[80];
    snprintf(label, sizeof(label), "vsl rig BA (extrinsics): %d free bodies, %d free blocks,", st.nfb, st.ne);
    ba_finish_summary(ctx, times, opt->verbosity, label, sum, summary);
    return VSL_OK;
  };
  rc = run();
  return rc ? rig_drain(ctx, rc) : VSL_OK;
}

// ================================================================================ EXTRINSICS: COVARIANCES
// vsl_ba_rig_ext_covariance (include/vslam_hip.h "covariances with the extrinsics as unknowns"): the
// posterior of the problem vsl_bundle_adjust_rig_ext adjusts, H = J^T J over [free bodies | free blocks | landmarks],
// Sigma = H^-1, at the bodies / extrinsics / points handed in.  Nothing is optimised.  One arena loan, one
// synchronisation:
//   rigx_linearize -> rigx_columns -> rigx_schur     the solve's own kernels, unscaled and undamped: the S of
//                                                    vsl_ba_rig_ext_linearize, bit for bit; F_b, F_x, E stay resident
//   vsl_cov_inverse_dev                              the six unit columns of every slot of Q (rxcp_plan); its 2^-36 pivot
//                                                    rule is the gauge detector the solve lacks
//   rigx_cov_gauge_kernel                            the same rule on S_uu [S^-1]_uu of every solved column: independent of
//                                                    the elimination order
//   vsl_cov_pair_blocks_dev                          the (body slot, block slot) and (block 0, block 1) joint blocks
//   rigx_cov_pose_kernel      one thread per pose item: body / extrinsic / cross blocks, the camera sandwich with
//                             A = [Ad(T_b_c^-1) | I]
//   rigx_cov_landmark_kernel  one wavefront per queried landmark over ALL its groups, extrinsic groups included
// No floating-point atomics; every sum in a fixed order.  ext_free = {0, 0} never gets here: the call hands over to
// vsl_ba_rig_covariance.
namespace {

// One thread per pose item (RigExtCovItem, ba_rig_cov_plan.h).  A diagonal block is read from the slot's own columns, the
// two mirror entries averaged -- the rule of rig_cov_pose_kernel and of a joint block's diagonal (ba_pair_blocks_kernel):
// the same bits.  RXC_CAM_FREE_HELD is rig_cov_pose_kernel's sequence.  RXC_CAM_FREE_FREE: with the joint block
// [[Sbb, Sbe], [Seb, See]] of the pair, M = Ad Sbb Ad^T + Ad Sbe + (Ad Sbe)^T + See, summed in that order per entry,
// then (M + M^T) / 2.
__global__ __launch_bounds__(64) void rigx_cov_pose_kernel(int n, int n_items, const RigExtCovItem* __restrict__ items,
                                                           const int* __restrict__ q_slot, const double* __restrict__ X,
                                                           const double* __restrict__ joint, const double* __restrict__ tcb,
                                                           const int* __restrict__ ok, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items || !*ok) return;
  const RigExtCovItem it = items[t];
  double* o = out + 36 * (size_t)t;
  if (it.kind == RXC_CROSS) {
    const double* J = joint + 144 * (size_t)it.pair;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b++) o[6 * a + b] = J[12 * a + 6 + b];
    return;
  }
  const int q = it.q, f = q_slot[q];
  double A[36];
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++)
      A[6 * a + b] = 0.5 * (X[vsl_cov_x_at(n, 6 * f + a, 6 * q + b)] + X[vsl_cov_x_at(n, 6 * f + b, 6 * q + a)]);
  if (it.kind == RXC_BODY || it.kind == RXC_CAM_FIXED_FREE || it.kind == RXC_EXT) {
#pragma unroll
    for (int e = 0; e < 36; e++) o[e] = A[e];
    return;
  }
  const double* Rt = tcb + 12 * it.blk;
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
  if (it.kind == RXC_CAM_FREE_FREE) {
    const double* J = joint + 144 * (size_t)it.pair;
    double Cx[36];  // Ad Sbe, column by column
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double v[6], w[6];
#pragma unroll
      for (int r = 0; r < 6; r++) v[r] = J[12 * r + 6 + c];
      rig_adjoint_apply(Rt, v, w);
#pragma unroll
      for (int r = 0; r < 6; r++) Cx[6 * r + c] = w[r];
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b++) B[6 * a + b] = ((M[6 * a + b] + Cx[6 * a + b]) + Cx[6 * b + a]) + J[12 * (6 + a) + 6 + b];
#pragma unroll
    for (int e = 0; e < 36; e++) M[e] = B[e];
  }
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) o[6 * a + b] = 0.5 * (M[6 * a + b] + M[6 * b + a]);
}

// The 2^-36 pivot rule made independent of the elimination order.  1 / (S_uu [S^-1]_uu) is the pivot ratio unknown u would
// have if it were eliminated LAST; the factorisation tests each unknown at its own place in [bodies | blocks] only, and in
// float64 the pivot of a gauge direction whose component in the last unknowns is small is rounding noise near the
// threshold (7e-11 against 1.5e-11 on the one-fixed-body window, 3e-15 in long double).  One thread per
// solved column: S_uu [S^-1]_uu >= 2^36, or an entry that is not positive and finite, clears *ok (every failing thread
// stores the same 0).  Sdiag: diag S before the factorisation.
__global__ void rigx_cov_gauge_kernel(int n, int n_cols, const int* __restrict__ q_slot, const double* __restrict__ Sdiag,
                                      const double* __restrict__ X, int* __restrict__ ok) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_cols || !*ok) return;
  const int u = 6 * q_slot[j / 6] + j % 6;
  const double v = Sdiag[u] * X[vsl_cov_x_at(n, u, j)];
  if (!(v > 0.0) || !(v < 68719476736.0)) *ok = 0;  // 2^36
}

// rig_cov_landmark_kernel on the groups of RigExtPlan: one wavefront per unique queried landmark u (l = u_lm[u]), its
// groups lm_grp[l] .. lm_grp[l + 1] in ascending slot (bodies, then blocks), each naming its observations through
// grp_obs[grp_first[g] .. grp_first[g + 1]) (ascending); a group of a slot >= nfb is an extrinsic group and reads F_x.
// P_l and W in the sum orders of rigx_lm_groups_kernel.  Dynamic LDS only: M [16 doubles] | W [18 K] | T [9 K], K = groups
// of the landmark (at most RCP_GMAX).
__global__ __launch_bounds__(64) void rigx_cov_landmark_kernel(int n, int nfb, const int* __restrict__ u_lm,
                                                               const int* __restrict__ lm_start, const int* __restrict__ lm_grp,
                                                               const int* __restrict__ grp_slot, const int* __restrict__ grp_first,
                                                               const int* __restrict__ grp_obs, const double* __restrict__ F,
                                                               const double* __restrict__ Fx, const double* __restrict__ E,
                                                               const int* __restrict__ qpos, const double* __restrict__ X,
                                                               const int* __restrict__ ok, double* __restrict__ out,
                                                               int* __restrict__ degenerate) {
  extern __shared__ __attribute__((aligned(16))) double rigx_cov_sh[];
  if (!*ok) return;
  const int u = blockIdx.x, lane = threadIdx.x, l = u_lm[u];
  const int g0 = lm_grp[l], K = lm_grp[l + 1] - g0;
  double* M = rigx_cov_sh;
  double* W = rigx_cov_sh + 16;
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
    const double* Fs = grp_slot[g0 + i] < nfb ? F : Fx;
    double w[18];
#pragma unroll
    for (int j = 0; j < 18; j++) w[j] = 0.0;
    for (int k = grp_first[g0 + i]; k < grp_first[g0 + i + 1]; k++) {
      const int ob = grp_obs[k];
      const double* f = Fs + 12 * (size_t)ob;
      const double* e = E + 6 * (size_t)ob;
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

// everything behind the validation; host_in / host_out outlive the stream work (the caller synchronises on an error)
int rigx_cov_run(vsl_ctx* ctx, const char* who, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const vsl_ba_options* opt,
                 RigxState& st, const RigExtCovPlan& P, std::vector<char>& host_in, std::vector<char>& host_out) {
  int rc;
  if ((rc = rigx_setup(ctx, prob, rig, opt, st, P.total))) return rc;
  char* dev = st.extra;
  const int n = st.D.n;
  host_in.assign(P.in_bytes, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(host_in.data() + off, src, bytes);
  };
  const int one = 1;
  put(P.off_ok, &one, sizeof(int));
  put(P.off_col_unk, P.col_unk.data(), sizeof(int) * P.col_unk.size());
  put(P.off_q_slot, P.q_slot.data(), sizeof(int) * P.q_slot.size());
  put(P.off_qpos, P.qpos.data(), sizeof(int) * P.qpos.size());
  put(P.off_items, P.items.data(), sizeof(RigExtCovItem) * P.items.size());
  put(P.off_pairs, P.pairs.data(), sizeof(PgcPairDev) * P.pairs.size());
  put(P.off_u_lm, P.u_lm.data(), sizeof(int) * P.u_lm.size());
  put(P.off_tcb, st.plan.T_c_b, sizeof(st.plan.T_c_b));
  VSL_HIP(ctx, hipMemcpyAsync(dev, host_in.data(), P.in_bytes, hipMemcpyHostToDevice, ctx->stream));
  int* ok = (int*)(dev + P.off_ok);
  double* X = (double*)(dev + P.off_X);
  double* joint = (double*)(dev + P.out_off + P.off_joint);
  // the S of vsl_ba_rig_ext_linearize: the same three calls
  if ((rc = rigx_linearize(ctx, st, st.cur, false, 0))) return rc;
  if ((rc = rigx_columns(ctx, st, st.cur))) return rc;
  if ((rc = rigx_schur(ctx, st, false, 0.0))) return rc;
  if (P.nQ > 0) {
    VslStage s(ctx, VSL_STAGE_BA_SOLVE);
    const VslCovInverse inv{n, 0, 0, st.S, nullptr, (double*)(dev + P.off_Linv), (double*)(dev + P.off_Sdiag),
                            (const int*)(dev + P.off_col_unk), nullptr, P.nblk, X, ok};
    if ((rc = vsl_cov_inverse_dev(ctx, inv))) return rc;
    hipLaunchKernelGGL(rigx_cov_gauge_kernel, dim3((6 * P.nQ + 255) / 256), dim3(256), 0, ctx->stream, n, 6 * P.nQ,
                       (const int*)(dev + P.off_q_slot), (const double*)(dev + P.off_Sdiag), X, ok);
    VSL_CHECK_LAUNCH(ctx);
    if ((rc = vsl_cov_pair_blocks_dev(ctx, n, P.n_pairs, (const PgcPairDev*)(dev + P.off_pairs), 0, nullptr, 0, X, ok, joint))) return rc;
    if (P.n_items > 0) {
      hipLaunchKernelGGL(rigx_cov_pose_kernel, dim3((P.n_items + 63) / 64), dim3(64), 0, ctx->stream, n, P.n_items,
                         (const RigExtCovItem*)(dev + P.off_items), (const int*)(dev + P.off_q_slot), X, joint,
                         (const double*)(dev + P.off_tcb), ok, (double*)(dev + P.out_off + P.off_pose));
      VSL_CHECK_LAUNCH(ctx);
    }
  }
  if (P.nu > 0) {
    const size_t lds = sizeof(double) * (16 + 27 * (size_t)std::max(P.gmax, 1));
    hipLaunchKernelGGL(rigx_cov_landmark_kernel, dim3(P.nu), dim3(64), lds, ctx->stream, n, st.nfb, (const int*)(dev + P.off_u_lm),
                       st.lm_start, st.lm_grp, st.grp_slot, st.grp_first, st.grp_obs, st.cur.F, st.cur.Fx, st.cur.E,
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
  if (!ok_host)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: the reduced system over bodies and extrinsics is not positive definite to working precision (a gauge direction is free?)", who);
  return VSL_OK;
}

}  // namespace

extern "C" int vsl_ba_rig_ext_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_rig* rig, const uint8_t* ext_free,
                                         const double* T_b_c, const vsl_ba_options* opt, const int32_t* bodies, int n_body_q,
                                         double* cov_body, const int32_t* cams, int n_cam_q, double* cov_cam, const int32_t* lms,
                                         int n_lm_q, double* cov_point, double* cov_ext, double* cov_body_ext, int* n_degenerate) {
  const char* who = "vsl_ba_rig_ext_covariance";
  if (!ctx) return VSL_ERR_INVALID;
  if (!rig || !ext_free || !T_b_c) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null pointer", who);
  if (!ext_free[0] && !ext_free[1]) {  // the rig call itself; cov_ext / cov_body_ext have no entry (m = 0): not written
    vsl_ba_rig held = *rig;
    held.T_b_c = T_b_c;
    return vsl_ba_rig_covariance(ctx, prob, &held, opt, bodies, n_body_q, cov_body, cams, n_cam_q, cov_cam, lms, n_lm_q, cov_point,
                                 n_degenerate);
  }
  std::vector<char> host_in, host_out;  // read / written by copies on the stream: they outlive the synchronisation below
  RigExtCovPlan P;
  int rc;
  {
    RigxState st;  // holds the loan of the context's arena
    if ((rc = rigx_validate(ctx, who, prob, rig, ext_free, T_b_c, opt, st))) return rc;
    if ((n_body_q > 0 && !cov_body) || (n_cam_q > 0 && !cov_cam) || (n_lm_q > 0 && !cov_point))
      return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null output", who);
    try {
      const int e = rxcp_plan(st.plan, st.xp, rig->n_bodies, prob->n_cams, prob->n_lms, prob->cam_intr, bodies, n_body_q, cams,
                              n_cam_q, lms, n_lm_q, cov_ext != nullptr, cov_body_ext != nullptr, P);
      if (e != RCP_OK) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: %s (%d)", who, rxcp_message(e), P.first_bad);
    } catch (const std::bad_alloc&) {
      return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    if (st.plan.n_fixed == 0)
      return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: no fixed body: the gauge is free and the reduced system singular", who);
    if (n_body_q == 0 && n_cam_q == 0 && n_lm_q == 0 && !cov_ext && !cov_body_ext) {  // nothing is launched
      if (n_degenerate) *n_degenerate = 0;
      return VSL_OK;
    }
    VSL_HIP(ctx, hipSetDevice(ctx->device));
    try {
      rc = rigx_cov_run(ctx, who, prob, rig, opt, st, P, host_in, host_out);
    } catch (const std::bad_alloc&) {
      rc = vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    // an error return may leave kernels and copies queued that use the arena and the host buffers: drain the stream
    // before the loan ends
    if (rc) (void)hipStreamSynchronize(ctx->stream);
  }
  if (rc) return rc;
  const double* pose = (const double*)(host_out.data() + P.off_pose);
  const double* jnt = (const double*)(host_out.data() + P.off_joint);
  const double* point = (const double*)(host_out.data() + P.off_point);
  const int* deg = (const int*)(host_out.data() + P.off_deg);
  if (n_body_q > 0) memcpy(cov_body, pose, 36 * sizeof(double) * (size_t)n_body_q);
  if (n_cam_q > 0) memcpy(cov_cam, pose + 36 * (size_t)n_body_q, 36 * sizeof(double) * (size_t)n_cam_q);
  const size_t behind = (size_t)n_body_q + (size_t)n_cam_q;
  if (cov_ext) {
    if (P.n_ext == 1) memcpy(cov_ext, pose + 36 * behind, 36 * sizeof(double));
    else memcpy(cov_ext, jnt + 144 * (size_t)P.ext_pair, 144 * sizeof(double));
  }
  if (cov_body_ext && P.n_cross > 0) memcpy(cov_body_ext, pose + 36 * (behind + P.n_ext_items), 36 * sizeof(double) * (size_t)P.n_cross);
  int nd = 0;
  for (int q = 0; q < n_lm_q; q++) {
    memcpy(cov_point + 9 * (size_t)q, point + 9 * (size_t)P.lm_q2u[q], 9 * sizeof(double));
    nd += deg[P.lm_q2u[q]] ? 1 : 0;
  }
  if (n_degenerate) *n_degenerate = nd;
  return VSL_OK;
}
