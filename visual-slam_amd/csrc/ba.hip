// ba.hip -- K6 (reprojection residual + Jacobian blocks) and K7 (Schur-complement reduction) plus the
// Levenberg-Marquardt loop that drives them.
//
// Replaces visnav::bundle_adjustment (include/visnav/map_utils.h:337-421) and
// visnav::global_bundle_adjustment (include/visnav/loop_closure_utils.h:672-748), i.e. what
// ceres::Solve does with BundleAdjustmentReprojectionCostFunctor (include/visnav/reprojection.h:81-105),
// the four camera models (include/visnav/camera_models.h), LocalParameterizationSE3
// (include/visnav/local_parameterization_se3.hpp:43-63), HuberLoss and SPARSE_SCHUR.
//
// Differences in HOW (the WHAT is the same optimisation problem and the same LM policy, restated in
// oracle/orc_ba.cpp from [upstream] Ceres 2.0/2.1):
//   * derivatives are closed-form 2x6 / 2x3 blocks in the tangent space of T*exp(delta), not dual
//     numbers through the quaternion followed by the 7x6 plus-Jacobian;
//   * observations are stored sorted by landmark; every reduction runs in a fixed order (per-landmark
//     loops, per-camera tree reductions, thread-owned Schur entries), so a solve is bit-reproducible
//     from run to run -- no floating-point atomics on the small-system path;
//   * Schur complement, small systems (6*free cameras <= 128, the local-BA window): each of the
//     (6C)^2 entries of S is OWNED by one thread of a 1024-thread workgroup, which keeps it in a
//     register while the workgroup streams its share of the landmarks through LDS (per landmark:
//     W = F^T E and Y = W P^-1 per observation, plus a camera->observation slot table).  Per-workgroup
//     partial matrices are summed in a fixed order afterwards.
//   * large systems (global BA): one wavefront per landmark, fp64 hardware atomics into the dense S,
//     blocked dense Cholesky (chol.hip).
//
// The host-side state (BaState) and the launchers declared in ba_state.h are shared with ba_session.hip, the session
// solver behind vsl_global_bundle_adjust (large maps, multi-GPU): its recompute-form kernels are ba_large.h, its
// stored-blocks form runs the kernels of this file.  The rig-constrained solver (ba_rig.hip) runs on them too: every
// kernel that does not depend on how observations group into pose blocks (linearisation -- a template instantiation
// applies the rig's adjoint --, reductions, landmark columns, block finish, Jacobi scaling, LM diagonals, model change,
// update) has ONE launch site here, a plain-pointer launcher (vsl_ba_*_launch, ba_state.h) that both chains call.  The
// speculative host loop itself is lm_speculative_loop (lm_policy.h), shared with vsl_bundle_adjust_rig.
//
// Algorithmic bytes per LM iteration: n_obs*(16 + 8) + n_lms*24 + n_cams*56 + 128 in;
// (6C)^2*8 + 6C*8 + n_lms*96 out.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <new>

#include "vsl_common.h"
#include "lm_policy.h"
#include "dev_arena.h"
#include "ba_host_plan.h"
#include "ba_device.h"
#include "ba_state.h"

namespace {

// ---------------------------------------------------------------------------------------- kernels
// K6.  One thread per observation (observations sorted by landmark).  Writes the robustified (and, when
// scale_c/scale_l are given, Jacobi-scaled) blocks and a per-workgroup cost partial.  RIG (ba_rig.hip): `poses` are the
// camera poses derived from the bodies, cam_free maps a camera to its BODY's slot, and F becomes the block against the
// body pose, F Ad(T_c_b) with tcb[12 k] the inverse extrinsic of intrinsics block k; RIG = false never reads tcb.
template <bool RIG>
__global__ __launch_bounds__(256) void ba_linearize_kernel(BaDims D, const double* __restrict__ poses,
                                                           const double* __restrict__ points,
                                                           const double* __restrict__ intr,
                                                           const int* __restrict__ cam_intr,
                                                           const int* __restrict__ cam_free,
                                                           const int* __restrict__ obs_cam,
                                                           const int* __restrict__ obs_lm,
                                                           const double* __restrict__ obs_uv,
                                                           const double* __restrict__ scale_c,
                                                           const double* __restrict__ scale_l, double* __restrict__ r_out,
                                                           double* __restrict__ F_out, double* __restrict__ E_out,
                                                           double* __restrict__ partials, int robust,
                                                           const double* __restrict__ tcb) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double c = 0;
  if (i < D.O) {
    const int cam = obs_cam[i], lm = obs_lm[i], k = cam_intr[cam];
    double r[2], F[12], E[6];
    residual_blocks(k ? D.model1 : D.model0, intr + 8 * k, poses + 7 * cam, points + 3 * lm, obs_uv + 2 * i, r, F, E,
                    true);
    if (RIG) rig_body_jacobian(tcb + 12 * k, F);
    const double s = r[0] * r[0] + r[1] * r[1];
    double rho0 = s, rho1 = 1.0;
    if (D.use_huber) huber(s, D.huber, rho0, rho1);
    c = 0.5 * rho0;
    const double sr = robust ? sqrt(rho1) : 1.0;
    r_out[2 * (size_t)i] = r[0] * sr;
    r_out[2 * (size_t)i + 1] = r[1] * sr;
    const int fc = cam_free[cam];
    for (int j = 0; j < 6; j++) {
      const double sc = (scale_c && fc >= 0) ? scale_c[6 * fc + j] : 1.0;
      F_out[12 * (size_t)i + j] = F[j] * sr * sc;
      F_out[12 * (size_t)i + 6 + j] = F[6 + j] * sr * sc;
    }
    for (int j = 0; j < 3; j++) {
      const double sc = scale_l ? scale_l[3 * lm + j] : 1.0;
      E_out[6 * (size_t)i + j] = E[j] * sr * sc;
      E_out[6 * (size_t)i + 3 + j] = E[3 + j] * sr * sc;
    }
  }
  const double t = block_sum_256(c, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// cost only, at candidate parameters
__global__ __launch_bounds__(256) void ba_cost_kernel(BaDims D, const double* __restrict__ poses,
                                                      const double* __restrict__ points, const double* __restrict__ intr,
                                                      const int* __restrict__ cam_intr, const int* __restrict__ obs_cam,
                                                      const int* __restrict__ obs_lm, const double* __restrict__ obs_uv,
                                                      int o_first, int o_count, double* __restrict__ partials) {
  __shared__ double sh[256];
  const int t = blockIdx.x * 256 + threadIdx.x;
  double c = 0;
  if (t < o_count) {
    const int i = o_first + t;
    const int cam = obs_cam[i], lm = obs_lm[i], k = cam_intr[cam];
    double r[2];
    residual_blocks(k ? D.model1 : D.model0, intr + 8 * k, poses + 7 * cam, points + 3 * lm, obs_uv + 2 * i, r, nullptr,
                    nullptr, false);
    const double s = r[0] * r[0] + r[1] * r[1];
    double rho0 = s, rho1 = 1.0;
    if (D.use_huber) huber(s, D.huber, rho0, rho1);
    c = 0.5 * rho0;
  }
  const double v = block_sum_256(c, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

// scalars[slot] = sum / max of partials[0..n) in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void ba_reduce_kernel(const double* __restrict__ partials, int n,
                                                        double* __restrict__ scalars, int slot, int is_max) {
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

// per-landmark column statistics: squared column norms of E and E^T r
__global__ __launch_bounds__(256) void ba_lm_cols_kernel(BaDims D, const int* __restrict__ lm_start,
                                                         const double* __restrict__ r, const double* __restrict__ E,
                                                         double* __restrict__ n2l, double* __restrict__ grad_l) {
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

// per-camera normal-equation block: H = sum F^T F (6x6) and g = sum F^T r over the camera's observations (camera
// CSR).  grid = (free cameras, segments): a workgroup sums every `segments`-th 256-observation slice of its camera
// (the local-BA window has ~11k observations per camera and only 12 free cameras: one workgroup per camera left
// the chip idle for 128 us behind a serial chain of dependent loads), all 27 accumulators go through ONE LDS tree
// (8 barriers, not 27 x 9), partials are summed per camera in segment order afterwards -- fixed order throughout.
__global__ __launch_bounds__(256) void ba_cam_block_kernel(const int* __restrict__ free_cams,
                                                           const int* __restrict__ cam_start,
                                                           const int* __restrict__ cam_obs, const double* __restrict__ r,
                                                           const double* __restrict__ F, double* __restrict__ part) {
  __shared__ double sh[27][256];
  const int fc = blockIdx.x, seg = blockIdx.y, nseg = gridDim.y;
  const int cam = free_cams[fc];
  double acc[27];
  for (int k = 0; k < 27; k++) acc[k] = 0;
  for (int q = cam_start[cam] + seg * 256 + threadIdx.x; q < cam_start[cam + 1]; q += 256 * nseg) {
    const int i = cam_obs[q];
    const double* f = F + 12 * (size_t)i;
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    int k = 0;
    for (int a = 0; a < 6; a++)
      for (int b = a; b < 6; b++) acc[k++] += f[a] * f[b] + f[6 + a] * f[6 + b];
    for (int a = 0; a < 6; a++) acc[21 + a] += f[a] * r0 + f[6 + a] * r1;
  }
#pragma unroll
  for (int k = 0; k < 27; k++) sh[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 27; k++) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 27) part[((size_t)fc * nseg + seg) * 27 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void ba_cam_block_finish_kernel(int nfree, int nseg, const double* __restrict__ part, double* __restrict__ H,
                                           double* __restrict__ g) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nfree * 27) return;
  const int fc = t / 27, k = t - fc * 27;
  double v = 0;
  for (int sgm = 0; sgm < nseg; sgm++) v += part[((size_t)fc * nseg + sgm) * 27 + k];
  if (k >= 21) {
    g[6 * (size_t)fc + (k - 21)] = v;
  } else {
    int a = 0, rem = k;  // k-th entry of the upper triangle, row-major
    while (rem >= 6 - a) {
      rem -= 6 - a;
      a++;
    }
    const int bcol = a + rem;
    H[36 * (size_t)fc + 6 * a + bcol] = v;
    H[36 * (size_t)fc + 6 * bcol + a] = v;
  }
}

// Jacobi scaling (computed once): scale = 1 / (1 + sqrt(column norm^2)); for cameras from diag(H)
__global__ void ba_make_scale_kernel(int nfree, int L, const double* __restrict__ H, const double* __restrict__ n2l,
                                     double* __restrict__ scale_c, double* __restrict__ scale_l) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * nfree) scale_c[i] = 1.0 / (1.0 + sqrt(H[36 * (size_t)(i / 6) + 7 * (i % 6)]));
  if (i < 3 * L) scale_l[i] = 1.0 / (1.0 + sqrt(n2l[i]));
}

__global__ void ba_apply_scale_kernel(int O, const int* __restrict__ cam_free, const int* __restrict__ obs_cam,
                                      const int* __restrict__ obs_lm, const double* __restrict__ scale_c,
                                      const double* __restrict__ scale_l, double* __restrict__ F, double* __restrict__ E) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= O) return;
  const int fc = cam_free[obs_cam[i]], lm = obs_lm[i];
  if (fc >= 0)
    for (int j = 0; j < 6; j++) {
      F[12 * (size_t)i + j] *= scale_c[6 * fc + j];
      F[12 * (size_t)i + 6 + j] *= scale_c[6 * fc + j];
    }
  for (int j = 0; j < 3; j++) {
    E[6 * (size_t)i + j] *= scale_l[3 * lm + j];
    E[6 * (size_t)i + 3 + j] *= scale_l[3 * lm + j];
  }
}

// gradient max-norm of the UNSCALED problem: |g_scaled / scale|, and LM diagonals
//   diag = clamp(col norm^2, 1e-6, 1e32) (kept when reuse != 0), D2 = diag / radius
__global__ __launch_bounds__(256) void ba_diag_kernel(int nfree, int L, const double* __restrict__ H, const double* __restrict__ n2l,
                                                      const double* __restrict__ g_c, const double* __restrict__ grad_l,
                                                      const double* __restrict__ scale_c, const double* __restrict__ scale_l,
                                                      double* __restrict__ diag_c, double* __restrict__ diag_l,
                                                      double* __restrict__ gabs) {
  // gabs[blockIdx.x] = the workgroup's maximum (one 45k-entry max by a single workgroup afterwards cost ~40 us)
  __shared__ double sh[256];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nc = 6 * nfree, nl = 3 * L;
  double m = 0;
  if (i < nc) {
    diag_c[i] = fmin(fmax(H[36 * (size_t)(i / 6) + 7 * (i % 6)], 1e-6), 1e32);
    m = fabs(g_c[i] / scale_c[i]);
  }
  if (i < nl) {
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

// K7, small systems.  See the file header.  LB landmarks are staged per barrier pair.
#define SCH_THREADS 1024
#ifndef SCH_LB
#define SCH_LB 16
#endif
#ifndef SCH_GMAX
#define SCH_GMAX 256
#endif
#define SCH_KMAX 24   // observations of one landmark that hit FREE cameras (<= free cameras <= 21)
#define SCH_EPT 16    // owned entries per thread: n <= 128
#define SCH_CMAX 22   // free cameras

// BLOCK3 = false: every thread owns up to SCH_EPT single entries of the full n x n matrix (the first formulation;
//   6 LDS doubles per 3 multiply-adds, LDS-bandwidth-bound; kept as the cross-check of the other one).
// BLOCK3 = true (default): a thread owns ONE 3 x 3 sub-block (bi, bj), bi >= bj, of the LOWER block triangle --
//   n = 6 * cameras is a multiple of 3, nb = n / 3 <= 42, nb (nb + 1) / 2 <= 903 <= SCH_THREADS sub-blocks, so threads
//   beyond that count own nothing (own = false guards every use) -- 18 LDS doubles per 27 fused multiply-adds; the
//   finish kernel mirrors the strictly-upper sub-blocks (S is symmetric).  A first attempt at this variant in round 1
//   faulted on the GPU and was reverted uncommitted (its source is lost); this one was written against the extents
//   listed in DESIGN.md section 5 (the round-1 Schur fault) and is tested at n = 72, 108 and 126.
template <bool BLOCK3>
__global__ __launch_bounds__(SCH_THREADS) void ba_schur_small_kernel(
    BaDims D, const int* __restrict__ lm_start, const int* __restrict__ obs_cam, const int* __restrict__ cam_free,
    const double* __restrict__ r, const double* __restrict__ F, const double* __restrict__ E,
    const double* __restrict__ diag_l, double inv_radius, int l_first, int l_count, int lm_per_wg,
    double* __restrict__ S_part, double* __restrict__ rhs_part, double* __restrict__ Pinv_out,
    double* __restrict__ bl_out) {
  __shared__ double W[SCH_LB][SCH_KMAX][18];
  __shared__ double Y[SCH_LB][SCH_KMAX][18];
  __shared__ double Pi_s[SCH_LB][9];
  __shared__ double b_s[SCH_LB][3];
  __shared__ int slot[SCH_LB][SCH_CMAX];
  __shared__ int kcnt[SCH_LB];
  __shared__ int obs_of[SCH_LB][SCH_KMAX];  // observation index of the k-th free-camera observation
  __shared__ int ok_s[SCH_LB];
  __shared__ int cam_of[SCH_LB][SCH_KMAX];  // free camera of the k-th free-camera observation
  __shared__ int dup_to[SCH_LB][SCH_KMAX];  // the slot its block is summed into: the first slot of the same camera
  __shared__ int dupf[SCH_LB];              // the landmark has a camera with more than one observation
  const int n = D.n, tid = threadIdx.x;
  const int wl0 = l_first + blockIdx.x * lm_per_wg;
  const int wl1 = min(l_first + l_count, wl0 + lm_per_wg);
  double acc[BLOCK3 ? 9 : SCH_EPT];
  int ei[BLOCK3 ? 1 : SCH_EPT];  // packed (c1, x, c2, y) of the owned entries
  // BLOCK3: sub-block (bi, bj) of thread tid = bi (bi + 1) / 2 + bj, bj <= bi < nb
  int bi = 0, bj = 0;
  bool own = false;
  if (BLOCK3) {
    const int nb = n / 3;
    bi = (int)((sqrt(8.0 * tid + 1.0) - 1.0) * 0.5);
    while (bi * (bi + 1) / 2 > tid) bi--;
    while ((bi + 1) * (bi + 2) / 2 <= tid) bi++;
    bj = tid - bi * (bi + 1) / 2;
    own = bi < nb;  // bj <= bi by construction
#pragma unroll
    for (int e = 0; e < 9; e++) acc[e] = 0;
  } else {
#pragma unroll
    for (int e = 0; e < SCH_EPT; e++) {
      acc[e] = 0;
      const int idx = tid + e * SCH_THREADS;
      if (idx < n * n) {
        const int i = idx / n, j = idx - i * n;
        ei[e] = (i / 6) | ((i % 6) << 8) | ((j / 6) << 16) | ((j % 6) << 24);
      } else {
        ei[e] = -1;
      }
    }
  }
  double racc = 0;  // thread tid < n owns rhs[tid]
  for (int s0 = wl0; s0 < wl1; s0 += SCH_LB) {
    const int nl = min(SCH_LB, wl1 - s0);
    // phase A: per landmark P, b, P^-1 and the slot table -- one WAVE per staged landmark: lanes take
    // the observations, 64 at a time (fixed cameras are not limited, so a landmark can have more), xor-shuffle
    // tree sums (fixed order), the free-camera rank of an observation from ballot prefixes
    {
      const int wv = tid >> 6, ln = tid & 63;
      if (wv < nl) {
        const int l = s0 + wv;
        const int o0 = lm_start[l], o1 = lm_start[l + 1];
        const int i = o0 + ln;
        const bool have = i < o1;
        double P6[6] = {0, 0, 0, 0, 0, 0}, bb[3] = {0, 0, 0};  // P upper: 00 01 02 11 12 22
        int fc = -1;
        if (have) {
          const double* e = E + 6 * (size_t)i;
          const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
          P6[0] = e[0] * e[0] + e[3] * e[3];
          P6[1] = e[0] * e[1] + e[3] * e[4];
          P6[2] = e[0] * e[2] + e[3] * e[5];
          P6[3] = e[1] * e[1] + e[4] * e[4];
          P6[4] = e[1] * e[2] + e[4] * e[5];
          P6[5] = e[2] * e[2] + e[5] * e[5];
          for (int x = 0; x < 3; x++) bb[x] = e[x] * r0 + e[3 + x] * r1;
          fc = cam_free[obs_cam[i]];
        }
        // observations beyond the first 64 (many fixed cameras, or cameras that see the landmark more than once)
        // are folded in serially
        for (int j = o0 + 64 + ln; j < o1; j += 64) {
          const double* e = E + 6 * (size_t)j;
          const double r0 = r[2 * (size_t)j], r1 = r[2 * (size_t)j + 1];
          P6[0] += e[0] * e[0] + e[3] * e[3];
          P6[1] += e[0] * e[1] + e[3] * e[4];
          P6[2] += e[0] * e[2] + e[3] * e[5];
          P6[3] += e[1] * e[1] + e[4] * e[4];
          P6[4] += e[1] * e[2] + e[4] * e[5];
          P6[5] += e[2] * e[2] + e[5] * e[5];
          for (int x = 0; x < 3; x++) bb[x] += e[x] * r0 + e[3 + x] * r1;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
          for (int q = 0; q < 6; q++) P6[q] += __shfl_xor(P6[q], o);
#pragma unroll
          for (int q = 0; q < 3; q++) bb[q] += __shfl_xor(bb[q], o);
        }
        double P[9] = {P6[0], P6[1], P6[2], P6[1], P6[3], P6[4], P6[2], P6[4], P6[5]};
        if (diag_l) {
          P[0] += diag_l[3 * (size_t)l] * inv_radius;
          P[4] += diag_l[3 * (size_t)l + 1] * inv_radius;
          P[8] += diag_l[3 * (size_t)l + 2] * inv_radius;
        }
        if (ln < SCH_CMAX) slot[wv][ln] = -1;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // 64 observations at a time: a window with many FIXED cameras has landmarks with more than 64 observations, and
        // a free camera among the later ones used to lose its W block (its E^T E was in P all the same)
        int seen_free = 0;
        for (int base = o0; base < o1; base += 64) {  // wave-uniform
          const int j = base + ln;
          const bool hv = j < o1;
          const int fcj = base == o0 ? fc : (hv ? cam_free[obs_cam[j]] : -1);
          const unsigned long long fm = __ballot(hv && fcj >= 0);
          const int rank = seen_free + __popcll(fm & ((1ull << ln) - 1ull));
          if (hv && fcj >= 0 && rank < SCH_KMAX) {
            cam_of[wv][rank] = fcj;
            obs_of[wv][rank] = j;
          }
          seen_free += __popcll(fm);
        }
        // (seen_free <= SCH_KMAX, repeats included: ba_host_plan counts the free-camera observations of every
        // landmark and sends a problem with more to the large-system kernels -- the min is a logic guard)
        const int k = min(seen_free, SCH_KMAX);
        // camera -> slot.  A free camera that observes the landmark more than once owns the slot of its FIRST
        // observation; the W / Y blocks of the later ones are added to that slot after phase B (two lanes used to write
        // one slot entry here, and whichever lost the race lost its block)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        bool later = false;
        if (ln < k) {
          const int c = cam_of[wv][ln];
          int first = ln;
          for (int q = ln - 1; q >= 0; q--)
            if (cam_of[wv][q] == c) first = q;
          dup_to[wv][ln] = first;
          later = first != ln;
          if (!later) slot[wv][c] = ln;
        }
        const bool any_later = __ballot(later) != 0ull;
        double Pi[9];
        const bool ok = o1 > o0 && inv3(P, Pi);
        if (ln == 0) {
          ok_s[wv] = ok;
          kcnt[wv] = ok ? k : 0;
          dupf[wv] = ok && any_later;
          for (int q = 0; q < 9; q++) Pi_s[wv][q] = ok ? Pi[q] : 0.0;
          for (int q = 0; q < 3; q++) b_s[wv][q] = ok ? bb[q] : 0.0;
          if (Pinv_out)
            for (int q = 0; q < 9; q++) Pinv_out[9 * (size_t)l + q] = ok ? Pi[q] : 0.0;
          if (bl_out)
            for (int q = 0; q < 3; q++) bl_out[3 * (size_t)l + q] = ok ? bb[q] : 0.0;
        }
      }
    }
    __syncthreads();
    // phase B: W = F^T E (6x3) and Y = W P^-1 for every free-camera observation of the staged landmarks
    for (int item = tid; item < nl * SCH_KMAX * 6; item += SCH_THREADS) {
      const int li = item / (SCH_KMAX * 6), rem = item - li * (SCH_KMAX * 6);
      const int q = rem / 6, x = rem - q * 6;
      if (q >= kcnt[li]) continue;
      const int i = obs_of[li][q];
      const double* f = F + 12 * (size_t)i;
      const double* e = E + 6 * (size_t)i;
      double w[3];
      for (int y = 0; y < 3; y++) w[y] = f[x] * e[y] + f[6 + x] * e[3 + y];
      const double* Pi = Pi_s[li];
      for (int y = 0; y < 3; y++) {
        W[li][q][3 * x + y] = w[y];
        Y[li][q][3 * x + y] = w[0] * Pi[y] + w[1] * Pi[3 + y] + w[2] * Pi[6 + y];
      }
    }
    __syncthreads();
    bool merge = false;  // workgroup-uniform
    for (int li = 0; li < nl; li++) merge = merge || dupf[li] != 0;
    if (merge) {  // a thread per entry of a FIRST slot adds the later slots of the same camera, in slot order
      for (int item = tid; item < nl * SCH_KMAX * 18; item += SCH_THREADS) {
        const int li = item / (SCH_KMAX * 18), rem = item - li * (SCH_KMAX * 18);
        const int f = rem / 18, t = rem - f * 18;
        if (!dupf[li] || f >= kcnt[li] || dup_to[li][f] != f) continue;
        double w = W[li][f][t], y = Y[li][f][t];
        for (int q = f + 1; q < kcnt[li]; q++)
          if (dup_to[li][q] == f) {
            w += W[li][q][t];
            y += Y[li][q][t];
          }
        W[li][f][t] = w;
        Y[li][f][t] = y;
      }
      __syncthreads();
    }
    // phase C: owned entries
    for (int li = 0; li < nl; li++) {
      if (!ok_s[li]) continue;
      if (BLOCK3) {
        if (own) {
          // cameras bi / 2 and bj / 2 (< nfree <= SCH_CMAX); rows 3 (bi % 2) .. +2 of Y = 9 contiguous doubles
          const int q1 = slot[li][bi >> 1], q2 = slot[li][bj >> 1];
          if (q1 >= 0 && q2 >= 0) {
            const double* y1 = &Y[li][q1][9 * (bi & 1)];
            const double* w2 = &W[li][q2][9 * (bj & 1)];
            double yv[9], wv[9];
#pragma unroll
            for (int t = 0; t < 9; t++) {
              yv[t] = y1[t];
              wv[t] = w2[t];
            }
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
              for (int b = 0; b < 3; b++)
                acc[3 * a + b] = fma(-yv[3 * a + 2], wv[3 * b + 2], fma(-yv[3 * a + 1], wv[3 * b + 1], fma(-yv[3 * a], wv[3 * b], acc[3 * a + b])));
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < SCH_EPT; e++) {
          const int pk = ei[e];
          if (pk < 0) continue;
          const int q1 = slot[li][pk & 0xFF], q2 = slot[li][(pk >> 16) & 0xFF];
          if (q1 < 0 || q2 < 0) continue;
          const double* y1 = &Y[li][q1][3 * ((pk >> 8) & 0xFF)];
          const double* w2 = &W[li][q2][3 * ((pk >> 24) & 0xFF)];
          acc[e] -= y1[0] * w2[0] + y1[1] * w2[1] + y1[2] * w2[2];
        }
      }
      if (tid < n) {
        const int q1 = slot[li][tid / 6];
        if (q1 >= 0) {
          const double* y1 = &Y[li][q1][3 * (tid % 6)];
          racc -= y1[0] * b_s[li][0] + y1[1] * b_s[li][1] + y1[2] * b_s[li][2];
        }
      }
    }
    __syncthreads();
  }
  if (BLOCK3) {
    if (own) {  // rows 3 bi .. 3 bi + 2 < n, columns 3 bj .. 3 bj + 2 < n
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) S_part[(size_t)blockIdx.x * n * n + (size_t)(3 * bi + a) * n + (3 * bj + b)] = acc[3 * a + b];
    }
  } else {
#pragma unroll
    for (int e = 0; e < SCH_EPT; e++) {
      const int idx = tid + e * SCH_THREADS;
      if (idx < n * n) S_part[(size_t)blockIdx.x * n * n + idx] = acc[e];
    }
  }
  if (tid < n) rhs_part[(size_t)blockIdx.x * n + tid] = racc;
}

// S = sum_g S_part[g] + blockdiag(H) + diag(D2_c);  rhs = sum_g rhs_part[g] + g_c.  A workgroup owns 16 consecutive
// entries; 16 threads per entry each sum a sixteenth of the partials, the sixteen sub-sums are added in order (fixed
// order, 16-deep dependent load chains instead of G-deep ones: 114 -> ~12 us for 256 partials of a 72 x 72 system).
__global__ __launch_bounds__(256) void ba_schur_finish_kernel(int n, int G, const double* __restrict__ S_part,
                                                              const double* __restrict__ rhs_part, const double* __restrict__ H,
                                                              const double* __restrict__ g_c, const double* __restrict__ diag_c,
                                                              double inv_radius, double* __restrict__ S, double* __restrict__ rhs,
                                                              int lower_blocks) {
  __shared__ double sh[16][17];
  const int e = threadIdx.x & 15, c = threadIdx.x >> 4;
  const int total = n * n + n;  // the n*n entries of S, then the n entries of rhs
  const int idx = blockIdx.x * 16 + e;
  const int per = (G + 15) / 16;
  double v = 0;
  if (idx < total) {
    const bool is_rhs = idx >= n * n;
    int sidx = idx;
    if (!is_rhs && lower_blocks) {  // the partials hold the lower triangle of 3 x 3 sub-blocks: mirror the rest
      const int i = idx / n, j = idx - i * n;
      if (i / 3 < j / 3) sidx = j * n + i;
    }
    const double* src = is_rhs ? rhs_part + (idx - n * n) : S_part + sidx;
    const size_t stride = is_rhs ? (size_t)n : (size_t)n * n;
    for (int g = c * per; g < min(G, (c + 1) * per); g++) v += src[(size_t)g * stride];
  }
  sh[c][e] = v;
  __syncthreads();
  if (c == 0 && idx < total) {
    double t = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) t += sh[k][e];
    if (idx < n * n) {
      const int i = idx / n, j = idx - i * n;
      if (i / 6 == j / 6) t += H[36 * (size_t)(i / 6) + 6 * (i % 6) + (j % 6)];
      if (i == j && diag_c) t += diag_c[i] * inv_radius;
      S[idx] = t;
    } else {
      rhs[idx - n * n] = t + g_c[idx - n * n];
    }
  }
}

// K7, large systems: one wavefront per landmark, fp64 hardware atomics into the dense S.
__global__ __launch_bounds__(256) void ba_schur_atomic_kernel(BaDims D, const int* __restrict__ lm_start,
                                                              const int* __restrict__ obs_cam,
                                                              const int* __restrict__ cam_free, const double* __restrict__ r,
                                                              const double* __restrict__ F, const double* __restrict__ E,
                                                              const double* __restrict__ diag_l, double inv_radius,
                                                              int l_first, int l_count, double* __restrict__ S,
                                                              double* __restrict__ rhs, double* __restrict__ Pinv_out,
                                                              double* __restrict__ bl_out, int lower_only, int ldS) {
  // S is addressed as S[row * ldS + col]: ldS = n for the dense matrix; band storage (chol.hip "BAND FORM") passes
  // storage + bws and ldS = bws together with lower_only = 2: only entries with col <= row exist there
  constexpr int KM = 64;
  __shared__ double Ws[4][KM][18];
  __shared__ double Ys[4][KM][18];
  __shared__ int cs[4][KM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l = l_first + blockIdx.x * 4 + wave;
  if (l >= l_first + l_count) return;
  const int a = lm_start[l], b = lm_start[l + 1];
  if (a == b) return;
  // P and b: lanes stride the observations, xor-shuffle tree reduction (fixed order)
  double P[6] = {0, 0, 0, 0, 0, 0}, bb[3] = {0, 0, 0};  // P upper: 00 01 02 11 12 22
  for (int i = a + lane; i < b; i += 64) {
    const double* e = E + 6 * (size_t)i;
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    P[0] += e[0] * e[0] + e[3] * e[3];
    P[1] += e[0] * e[1] + e[3] * e[4];
    P[2] += e[0] * e[2] + e[3] * e[5];
    P[3] += e[1] * e[1] + e[4] * e[4];
    P[4] += e[1] * e[2] + e[4] * e[5];
    P[5] += e[2] * e[2] + e[5] * e[5];
    for (int x = 0; x < 3; x++) bb[x] += e[x] * r0 + e[3 + x] * r1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int q = 0; q < 6; q++) P[q] += __shfl_xor(P[q], o);
    for (int q = 0; q < 3; q++) bb[q] += __shfl_xor(bb[q], o);
  }
  double Pf[9] = {P[0], P[1], P[2], P[1], P[3], P[4], P[2], P[4], P[5]};
  if (diag_l) {
    Pf[0] += diag_l[3 * (size_t)l] * inv_radius;
    Pf[4] += diag_l[3 * (size_t)l + 1] * inv_radius;
    Pf[8] += diag_l[3 * (size_t)l + 2] * inv_radius;
  }
  double Pi[9];
  const bool ok = inv3(Pf, Pi);
  if (lane == 0) {
    if (Pinv_out)
      for (int q = 0; q < 9; q++) Pinv_out[9 * (size_t)l + q] = ok ? Pi[q] : 0.0;
    if (bl_out)
      for (int q = 0; q < 3; q++) bl_out[3 * (size_t)l + q] = ok ? bb[q] : 0.0;
  }
  if (!ok) return;
  // observations in chunks of KM free-camera hits (a landmark seen by more than KM free cameras is
  // processed chunk x chunk)
  for (int qa = a; qa < b; qa += KM) {
    const int na = min(KM, b - qa);
    for (int qb = a; qb < b; qb += KM) {
      const int nb = min(KM, b - qb);
      // stage Y of chunk a and W of chunk b
      for (int item = lane; item < na * 6; item += 64) {
        const int q = item / 6, x = item - q * 6, i = qa + q;
        const double* f = F + 12 * (size_t)i;
        const double* e = E + 6 * (size_t)i;
        double w[3];
        for (int y = 0; y < 3; y++) w[y] = f[x] * e[y] + f[6 + x] * e[3 + y];
        for (int y = 0; y < 3; y++) Ys[wave][q][3 * x + y] = w[0] * Pi[y] + w[1] * Pi[3 + y] + w[2] * Pi[6 + y];
        if (x == 0) cs[wave][q] = cam_free[obs_cam[i]];
      }
      for (int item = lane; item < nb * 6; item += 64) {
        const int q = item / 6, x = item - q * 6, i = qb + q;
        const double* f = F + 12 * (size_t)i;
        const double* e = E + 6 * (size_t)i;
        for (int y = 0; y < 3; y++) Ws[wave][q][3 * x + y] = f[x] * e[y] + f[6 + x] * e[3 + y];
      }
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();
      for (int item = lane; item < na * nb * 36; item += 64) {
        const int q1 = item / (nb * 36), rem = item - q1 * (nb * 36);
        const int q2 = rem / 36, xy = rem - q2 * 36, x = xy / 6, y = xy - x * 6;
        const int c1 = cs[wave][q1], c2 = cam_free[obs_cam[qb + q2]];
        // lower_only: the Cholesky solve reads only the lower triangle -- blocks above the block diagonal
        // are not accumulated (half the atomics); the diagonal blocks stay complete
        if (c1 < 0 || c2 < 0 || (lower_only && c1 < c2) || (lower_only == 2 && c1 == c2 && x < y)) continue;
        const double* y1 = &Ys[wave][q1][3 * x];
        const double* w2 = &Ws[wave][q2][3 * y];
        unsafeAtomicAdd(&S[(size_t)(6 * c1 + x) * ldS + 6 * c2 + y], -(y1[0] * w2[0] + y1[1] * w2[1] + y1[2] * w2[2]));
      }
      if (qb == a) {
        for (int item = lane; item < na * 6; item += 64) {
          const int q = item / 6, x = item - q * 6;
          const int c1 = cs[wave][q];
          if (c1 < 0) continue;
          const double* y1 = &Ys[wave][q][3 * x];
          unsafeAtomicAdd(&rhs[6 * c1 + x], -(y1[0] * bb[0] + y1[1] * bb[1] + y1[2] * bb[2]));
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- K7, large systems, gather form (the default).  The block structure of the reduced camera system is fixed over
// the LM iterations of a solve: block (c1, c2), c1 >= c2, receives one term -Y_i W_j^T per landmark seen by both
// cameras (i, j = that landmark's observations by c1 and c2).  The (i, j) pairs are listed per block ONCE per solve (count / scan / fill, below); every
// iteration a per-landmark kernel writes W_i = F_i^T E_i and Y_i = W_i P^-1 for every observation, and a per-block
// kernel sums its list -- every entry of S is written once, by one lane, no atomics (157 M fp64 atomics per iteration at
// 1000 cameras / 881k observations took 2.5 ms).
// Slot of block (c1, c2): band form c1 * (hb + 1) + (c1 - c2) with hb = the half bandwidth in cameras; otherwise the
// packed lower triangle c1 (c1 + 1) / 2 + c2.
__device__ __forceinline__ int ba_pair_slot(int c1, int c2, int hbp1) {
  return hbp1 > 0 ? c1 * hbp1 + (c1 - c2) : c1 * (c1 + 1) / 2 + c2;
}

// FILL = false: cnt[slot] += 1 per pair; FILL = true: pairs[start[slot] + cursor[slot]++] = (i, j)
template <bool FILL>
__global__ void ba_pair_list_kernel(int l_first, int l_count, const int* __restrict__ lm_start, const int* __restrict__ obs_cam,
                                    const int* __restrict__ cam_free, const int* __restrict__ cam_pos, int hbp1, int nfree_cyclic,
                                    int* __restrict__ cnt, const int* __restrict__ start, int* __restrict__ pairs) {
  const int l = l_first + blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= l_first + l_count) return;
  const int a = lm_start[l], b = lm_start[l + 1];
  for (int i = a; i < b; i++) {
    const int ci = cam_free[obs_cam[i]];
    if (ci < 0) continue;
    for (int j = a; j < b; j++) {
      const int cj = cam_free[obs_cam[j]];
      if (cj < 0 || cj > ci) continue;  // (two observations of one landmark by the SAME camera: both orders land in the diagonal block)
      int slot, pi = i, pj = j;
      if (nfree_cyclic > 0 && ci - cj >= hbp1) {
        // cyclic band: the two cameras are neighbours AROUND the loop -- the block is (cj, ci - nfree), stored in row cj
        // (the smaller index) at distance cj + nfree - ci, and the roles of the two observations swap with it
        slot = cj * hbp1 + (cj + nfree_cyclic - ci);
        pi = j;
        pj = i;
      } else {
        slot = ba_pair_slot(ci, cj, hbp1);
      }
      const int k = atomicAdd(&cnt[slot], 1);
      if (FILL) {
        const size_t pos = (size_t)start[slot] + k;
        pairs[2 * pos] = cam_pos[pi];  // where the block of the observation lives (camera-major order)
        pairs[2 * pos + 1] = cam_pos[pj];
      }
    }
  }
}

// exclusive prefix sum of cnt[0 .. n) into start[0 .. n], one workgroup
__global__ __launch_bounds__(1024) void ba_pair_scan_kernel(int n, const int* __restrict__ cnt, int* __restrict__ start) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int idx = base + tid;
    const int v = idx < n ? cnt[idx] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int off = carry_s;
    for (int w = 0; w < wave; w++) off += wsum[w];
    if (idx < n) start[idx] = off + x - v;
    __syncthreads();
    if (tid == 1023) carry_s = off + x;
    __syncthreads();
  }
  if (tid == 0) start[n] = carry_s;
}

// the fill order of a slot's list depends on the scheduling of the atomics above; sorting every list by its
// (i, j) keys once makes the summation order of the gather -- and with it the whole large-system solve -- reproducible
// run to run.  One wavefront per slot, rank sort in LDS (lists hold a few hundred pairs; beyond PAIR_SORT_MAX a list
// stays in fill order).
#define PAIR_SORT_MAX 2048
__global__ __launch_bounds__(64) void ba_pair_sort_kernel(const int* __restrict__ start, int* __restrict__ pairs) {
  __shared__ unsigned long long key[PAIR_SORT_MAX];
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int p0 = start[slot], n = start[slot + 1] - p0;
  if (n < 2 || n > PAIR_SORT_MAX) return;
  for (int t = lane; t < n; t += 64) {
    const int2 ij = *(const int2*)(pairs + 2 * (size_t)(p0 + t));
    key[t] = ((unsigned long long)(unsigned)ij.x << 32) | (unsigned)ij.y;
  }
  __syncthreads();
  for (int t = lane; t < n; t += 64) {
    const unsigned long long mine = key[t];
    int rank = 0;
    for (int u = 0; u < n; u++) rank += key[u] < mine;  // keys are distinct: (i, j) occurs once
    int2 ij;
    ij.x = (int)(mine >> 32);
    ij.y = (int)(mine & 0xffffffffu);
    *(int2*)(pairs + 2 * (size_t)(p0 + rank)) = ij;
  }
}

// rhs of the reduced system, gather form: rhs[6 fc + x] = -sum over the observations of free camera fc (contiguous in
// camera-major order) whose landmark lies in [l_first, l_first + l_count) of Y_i[x] . b_l -- one wavefront per camera,
// lanes stride the observations, xor-tree (fixed order).  ba_add_cam_blocks_kernel adds g_c afterwards.
__global__ __launch_bounds__(64) void ba_schur_rhs_kernel(int nfree, const int* __restrict__ free_cams,
                                                          const int* __restrict__ cam_start, const int* __restrict__ cam_obs,
                                                          const int* __restrict__ obs_lm, const double* __restrict__ Yg,
                                                          const double* __restrict__ bl, int l_first, int l_count,
                                                          double* __restrict__ rhs) {
  const int fc = blockIdx.x, lane = threadIdx.x;
  const int c = free_cams[fc];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int k = cam_start[c] + lane; k < cam_start[c + 1]; k += 64) {
    const int l = obs_lm[cam_obs[k]];
    if (l < l_first || l >= l_first + l_count) continue;
    const double* y = Yg + 18 * (size_t)k;
    const double b0 = bl[3 * (size_t)l], b1 = bl[3 * (size_t)l + 1], b2 = bl[3 * (size_t)l + 2];
#pragma unroll
    for (int x = 0; x < 6; x++) acc[x] += y[3 * x] * b0 + y[3 * x + 1] * b1 + y[3 * x + 2] * b2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int x = 0; x < 6; x++) acc[x] += __shfl_xor(acc[x], o);
  if (lane < 6) rhs[6 * fc + lane] = -acc[lane];
}

// per landmark (one wavefront): P, b, P^-1 (kept for the back-substitution), and for every observation W and Y = W P^-1
// (Y = 0 for a landmark whose P is singular: it contributes nothing)
__global__ __launch_bounds__(256) void ba_schur_prep_kernel(BaDims D, const int* __restrict__ lm_start,
                                                            const int* __restrict__ obs_cam, const int* __restrict__ cam_free,
                                                            const int* __restrict__ cam_pos, const double* __restrict__ r,
                                                            const double* __restrict__ F, const double* __restrict__ E,
                                                            const double* __restrict__ diag_l, double inv_radius,
                                                            int l_first, int l_count, double* __restrict__ Wg,
                                                            double* __restrict__ Yg,
                                                            double* __restrict__ rhs, double* __restrict__ Pinv_out,
                                                            double* __restrict__ bl_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l = l_first + blockIdx.x * 4 + wave;
  if (l >= l_first + l_count) return;
  const int a = lm_start[l], b = lm_start[l + 1];
  if (a == b) return;
  double P[6] = {0, 0, 0, 0, 0, 0}, bb[3] = {0, 0, 0};  // P upper: 00 01 02 11 12 22
  for (int i = a + lane; i < b; i += 64) {
    const double* e = E + 6 * (size_t)i;
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    P[0] += e[0] * e[0] + e[3] * e[3];
    P[1] += e[0] * e[1] + e[3] * e[4];
    P[2] += e[0] * e[2] + e[3] * e[5];
    P[3] += e[1] * e[1] + e[4] * e[4];
    P[4] += e[1] * e[2] + e[4] * e[5];
    P[5] += e[2] * e[2] + e[5] * e[5];
    for (int x = 0; x < 3; x++) bb[x] += e[x] * r0 + e[3 + x] * r1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int q = 0; q < 6; q++) P[q] += __shfl_xor(P[q], o);
    for (int q = 0; q < 3; q++) bb[q] += __shfl_xor(bb[q], o);
  }
  double Pf[9] = {P[0], P[1], P[2], P[1], P[3], P[4], P[2], P[4], P[5]};
  if (diag_l) {
    Pf[0] += diag_l[3 * (size_t)l] * inv_radius;
    Pf[4] += diag_l[3 * (size_t)l + 1] * inv_radius;
    Pf[8] += diag_l[3 * (size_t)l + 2] * inv_radius;
  }
  double Pi[9];
  const bool ok = inv3(Pf, Pi);
  if (lane == 0) {
    if (Pinv_out)
      for (int q = 0; q < 9; q++) Pinv_out[9 * (size_t)l + q] = ok ? Pi[q] : 0.0;
    if (bl_out)
      for (int q = 0; q < 3; q++) bl_out[3 * (size_t)l + q] = ok ? bb[q] : 0.0;
  }
  for (int item = lane; item < (b - a) * 6; item += 64) {
    const int q = item / 6, x = item - q * 6, i = a + q;
    const int c = cam_free[obs_cam[i]];
    if (c < 0) continue;
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    double w[3], y[3];
    for (int z = 0; z < 3; z++) w[z] = f[x] * e[z] + f[6 + x] * e[3 + z];
    for (int z = 0; z < 3; z++) y[z] = ok ? w[0] * Pi[z] + w[1] * Pi[3 + z] + w[2] * Pi[6 + z] : 0.0;
    const size_t at = 18 * (size_t)cam_pos[i] + 3 * x;
    for (int z = 0; z < 3; z++) {
      Wg[at + z] = w[z];
      Yg[at + z] = y[z];
    }
  }
}

// per block slot (one wavefront): S_block = -sum over the slot's pairs of Y_i W_j^T, written once.  A lane takes every
// 64th pair of the list -- both 144-byte blocks with 16-byte loads, all 36 products -- so 64 pairs' loads are in flight
// at once (one pair per iteration with the 36 entries over the lanes was bound by the latency of the dependent loads
// pair -> W / Y: 0.85 ms per iteration at 4.4 M pairs); the 36 x 64 partial sums are folded through LDS in lane order.
// (Sessions in the recompute form pass ONE array for both operands: the block Z = F^T E chol(P^-1) of ba_large.h, with
// Y_i W_j^T = Z_i Z_j^T.)
// The blocks of a round's 64 pairs are FETCHED COOPERATIVELY (round 4): the 128 blocks are 1152 pieces of 16 bytes,
// piece m = 64 t + lane belongs to block m / 9, so nine consecutive lanes read one contiguous 144-byte block and an
// instruction touches ~10 cache lines; they land in LDS at double2[m] (linear, conflict-free) and every lane reads its
// own two blocks from there.  With a lane loading its own blocks every 16-byte load instruction touched 64 different
// lines, and the L1's one-line-per-cycle tag rate -- 18 instructions x 64 lines per round -- bounded the kernel.
// Band form keeps only x >= y of a diagonal block (lower_mode 2); lower_mode 1 = dense lower triangle (diagonal blocks
// complete), 0 = full matrix (the mirror block is written as well).
__global__ __launch_bounds__(64) void ba_schur_gather_kernel(int n_slots, int hbp1, const int* __restrict__ start,
                                                             const int* __restrict__ pairs, const double* __restrict__ Wg,
                                                             const double* __restrict__ Yg, double* __restrict__ S, int ldS,
                                                             int lower_mode) {
  __shared__ double red[36][65];  // (halved with a shuffle step first -- 12 instead of 8 wavefronts per compute unit -- the kernel was 9% SLOWER: more rows in flight than the L2 holds)
  int slot = blockIdx.x;
  if (hbp1 > 0) {
    // Band form, XCD-aware order (round 4): workgroup b runs on XCD b % 8 (round-robin dispatch), and every XCD gets a
    // CONTIGUOUS range of camera rows, walked in order.  The hbp1 slots of a row read the same Y blocks (the row camera's
    // observations) and the rows c .. c + hbp1 - 1 the same W blocks (camera c's): with slot = blockIdx.x those readers
    // sat on all eight XCDs, each L2 (4 MB) fetched every block for itself and the kernel ran at the fabric's ~5 TB/s
    // (1.3 GB per launch for 254 MB of distinct blocks).
    const int nrows = n_slots / hbp1, rpx = (nrows + 7) >> 3;
    const int k = (int)(blockIdx.x >> 3), row = (int)(blockIdx.x & 7) * rpx + k / hbp1;
    if (row >= nrows) return;
    slot = row * hbp1 + k % hbp1;
  }
  const int p0 = start[slot], p1 = start[slot + 1];
  if (p0 == p1) return;
  const int lane = threadIdx.x;
  double acc[36];
#pragma unroll
  for (int e = 0; e < 36; e++) acc[e] = 0.0;
  double2* stage = (double2*)&red[0][0];  // 1152 pieces of a round; the same LDS folds the partial sums afterwards
  static_assert(sizeof(red) >= 1152 * sizeof(double2), "the staging area must fit");
  for (int base = p0; base < p1; base += 64) {
    const int p = base + lane;
    const bool have = p < p1;
    int2 ij = make_int2(0, 0);  // (idle lanes fetch block 0: valid memory, never accumulated)
    if (have) ij = *(const int2*)(pairs + 2 * (size_t)p);
    double2 piece[18];
#pragma unroll
    for (int t = 0; t < 18; t++) {
      const int m = 64 * t + lane, b = m / 9, part = m - 9 * b;
      const int iy = __shfl(ij.x, b & 63), iw = __shfl(ij.y, b & 63);
      const double* src = b < 64 ? Yg + 18 * (size_t)iy : Wg + 18 * (size_t)iw;
      piece[t] = *(const double2*)(src + 2 * part);
    }
#pragma unroll
    for (int t = 0; t < 18; t++) stage[64 * t + lane] = piece[t];
    __syncthreads();
    if (have) {
      double yv[18], wv[18];
#pragma unroll
      for (int q = 0; q < 9; q++) {
        const double2 a2 = stage[9 * lane + q], b2 = stage[9 * (64 + lane) + q];
        yv[2 * q] = a2.x;
        yv[2 * q + 1] = a2.y;
        wv[2 * q] = b2.x;
        wv[2 * q + 1] = b2.y;
      }
#pragma unroll
      for (int x = 0; x < 6; x++)
#pragma unroll
        for (int y = 0; y < 6; y++)
          acc[6 * x + y] += yv[3 * x] * wv[3 * y] + yv[3 * x + 1] * wv[3 * y + 1] + yv[3 * x + 2] * wv[3 * y + 2];
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 36; e++) red[e][lane] = acc[e];
  __syncthreads();
  if (lane >= 36) return;
  const int x = lane / 6, y = lane - 6 * x;
  double tot = 0.0;
  const int nl = min(64, p1 - p0);
  for (int l = 0; l < nl; l++) tot += red[lane][l];
  const double v = -tot;
  int c1, c2;
  if (hbp1 > 0) {
    c1 = slot / hbp1;
    c2 = c1 - (slot - c1 * hbp1);
  } else {
    c1 = (int)((sqrt(8.0 * (double)slot + 1.0) - 1.0) * 0.5);
    while (c1 * (c1 + 1) / 2 > slot) c1--;
    while ((c1 + 1) * (c1 + 2) / 2 <= slot) c1++;
    c2 = slot - c1 * (c1 + 1) / 2;
  }
  if (!(lower_mode == 2 && c1 == c2 && x < y)) S[(size_t)(6 * c1 + x) * ldS + 6 * c2 + y] = v;
  if (lower_mode == 0 && c1 != c2) S[(size_t)(6 * c2 + y) * ldS + 6 * c1 + x] = v;
}

// S += blockdiag(H) + diag(D2); rhs += g_c   (large-system path, S pre-zeroed before the atomics)
__global__ void ba_add_cam_blocks_kernel(int nfree, const double* __restrict__ H, const double* __restrict__ g_c,
                                         const double* __restrict__ diag_c, double inv_radius, double* __restrict__ S,
                                         double* __restrict__ rhs, int ldS, int lower_elems) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = 6 * nfree;
  if (t < nfree * 36) {
    const int fc = t / 36, x = (t % 36) / 6, y = t % 6;
    double v = H[t];
    if (x == y && diag_c) v += diag_c[6 * fc + x] * inv_radius;
    if (!(lower_elems && y > x)) S[(size_t)(6 * fc + x) * ldS + 6 * fc + y] += v;
  }
  if (t < n) rhs[t] += g_c[t];
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {  // `lane` wave-uniform (a constant after unrolling)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// dense Cholesky solve in LDS, one workgroup; n <= 128.  dc = -(S^-1 rhs); flag = 0 on failure.
//
// Blocked right-looking factorisation, 8-column panels, THREE workgroup barriers per panel (the first version ran one
// pivot -> sqrt -> divide -> barrier round and a serial per-row trailing update per COLUMN: 124 us for 72 x 72):
//   panel:    a thread owns a row of the panel (8 values in registers).  Each wavefront factors the 8 x 8 diagonal
//             block redundantly in its lanes 0..7 (row per lane, column broadcasts by v_readlane: no LDS, no barrier),
//             then every row is solved against that factor with readlane broadcasts of its entries;
//   trailing: 4 x 4 register tiles of the lower triangle, 8-deep products from the panel rows in LDS.
// Rows are padded to an odd stride (column walks spread over the banks).  The substitutions run in one wavefront, two
// rows per lane, multiplying by the stored reciprocal pivots.
#define CH_NB 8
__global__ __launch_bounds__(256) void ba_chol_small_kernel(int n, const double* __restrict__ S, const double* __restrict__ rhs,
                                                            double* __restrict__ dc, int* __restrict__ ok_flag,
                                                            int* __restrict__ arm_flag = nullptr) {
  __shared__ double A[128 * 129 + 256];  // static: dynamic LDS above 64 KiB is refused by the runtime
  __shared__ int fail_s;
  const int ld = n | 1;
  double* bvec = A + 128 * 129;
  double* invd = bvec + 128;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < n * n; i += 256) {
    const int r = i / n, c = i - r * n;
    A[r * ld + c] = S[i];
  }
  for (int i = tid; i < n; i += 256) bvec[i] = rhs[i];
  if (tid == 0) fail_s = 0;
  __syncthreads();
#ifdef CHS_TIMING
  long long tp[6] = {0, 0, 0, 0, 0, 0}, tt = __builtin_amdgcn_s_memtime();
#define CHS_STAMP(q) { const long long t2 = __builtin_amdgcn_s_memtime(); tp[q] += t2 - tt; tt = t2; }
#else
#define CHS_STAMP(q)
#endif
  CHS_STAMP(0)
  for (int j0 = 0; j0 < n; j0 += CH_NB) {
    const int w = min(CH_NB, n - j0);  // a ragged last panel is completed with identity columns
    const int row = j0 + tid;
    const bool valid = tid < 128 && row < n;
    double a[CH_NB], dr[CH_NB];
    if (tid < 128) {
#pragma unroll
      for (int c = 0; c < CH_NB; c++) {
        a[c] = (valid && c < w) ? A[row * ld + j0 + c] : 0.0;
        dr[c] = (lane < w && c < w) ? A[(j0 + lane) * ld + j0 + c] : (lane == c ? 1.0 : 0.0);
      }
    }
    __syncthreads();  // the second wavefront has read the diagonal block before the first one overwrites it with L
    CHS_STAMP(1)
    if (tid < 128) {
      double inv[CH_NB], x[CH_NB];
      bool good = true;
#pragma unroll
      for (int c = 0; c < CH_NB; c++) {
        const double d = readlane_f64(dr[c], c);
        if (!(d > 0.0) || !isfinite(d)) good = false;  // wave-uniform
        // 1 / sqrt(d) by the hardware estimate and two Newton steps, sqrt(d) = d / sqrt(d): the IEEE sqrt and divide
        // expansions are ~100 dependent fp64 instructions each, and the pivots are a serial chain (measured in the band
        // solver of chol.hip: ~1500 cycles per pivot, i.e. most of this kernel's 60 us at n = 72)
        double iv = __builtin_amdgcn_rsq(d);
        iv = iv * (1.5 - 0.5 * d * iv * iv);
        iv = iv * (1.5 - 0.5 * d * iv * iv);
        inv[c] = iv;
        dr[c] = (lane == c) ? d * iv : dr[c] * iv;     // lanes > c: l(lane, c)
#pragma unroll
        for (int k = c + 1; k < CH_NB; k++) dr[k] -= dr[c] * readlane_f64(dr[c], k);  // meaningful for lanes >= k
      }
      // x L_d^T = a: the row of L in this panel (for a diagonal-block row this reproduces that row of L_d)
#pragma unroll
      for (int c = 0; c < CH_NB; c++) {
        double t = a[c];
#pragma unroll
        for (int k = 0; k < c; k++) t -= x[k] * readlane_f64(dr[k], c);
        x[c] = t * inv[c];
      }
      if (valid) {
#pragma unroll
        for (int c = 0; c < CH_NB; c++)
          if (c < w && tid >= c) A[row * ld + j0 + c] = x[c];
      }
      if (tid == 0) {
#pragma unroll
        for (int c = 0; c < CH_NB; c++)
          if (c < w) invd[j0 + c] = inv[c];
        if (!good) fail_s = 1;
      }
    }
    __syncthreads();
    CHS_STAMP(2)
    if (fail_s) break;  // workgroup-uniform
    const int r0 = j0 + CH_NB, rem = n - r0;
    if (rem > 0) {
      const int T = (rem + 3) >> 2, ntiles = T * (T + 1) / 2;
      for (int tile = tid; tile < ntiles; tile += 256) {
        int ti = (int)((__fsqrt_rn(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);  // fp32 estimate, corrected below (an fp64 sqrt costs more than the tile)
        while (ti * (ti + 1) / 2 > tile) ti--;
        while ((ti + 1) * (ti + 2) / 2 <= tile) ti++;
        const int tj = tile - ti * (ti + 1) / 2;
        const int ib = r0 + 4 * ti, kb = r0 + 4 * tj;
        double Li[4][CH_NB], Lk[4][CH_NB];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int ir = min(ib + q, n - 1), kr = min(kb + q, n - 1);
#pragma unroll
          for (int c = 0; c < CH_NB; c++) {
            Li[q][c] = A[ir * ld + j0 + c];
            Lk[q][c] = A[kr * ld + j0 + c];
          }
        }
#pragma unroll
        for (int qa = 0; qa < 4; qa++)
#pragma unroll
          for (int qb = 0; qb < 4; qb++) {
            const int i = ib + qa, k = kb + qb;
            if (i < n && k <= i) {
              double acc = A[i * ld + k];
#pragma unroll
              for (int c = 0; c < CH_NB; c++) acc = fma(-Li[qa][c], Lk[qb][c], acc);
              A[i * ld + k] = acc;
            }
          }
      }
    }
    __syncthreads();
    CHS_STAMP(3)
  }
  const bool good = fail_s == 0;
  if (good && tid < 64) {
    // substitutions by one wavefront, two rows per lane, no workgroup barriers: L y = b, then L^T x = y.  Panel by
    // panel: the eight factor entries a lane needs for a panel are read from LDS BEFORE the panel's eight serial steps
    // (with the read inside every step the chain was 144 x (LDS latency + broadcast): 52k of the kernel's 125k cycles)
    const int r0 = lane, r1 = lane + 64;
    double b0 = r0 < n ? bvec[r0] : 0.0, b1 = r1 < n ? bvec[r1] : 0.0;
    // the reciprocal pivots ride in registers too (lane l: pivots l and l + 64) and are broadcast like the solution
    // entries: an LDS read of invd[j] inside a step put the LDS latency back into the chain
    const double inv0 = r0 < n ? invd[r0] : 0.0, inv1 = r1 < n ? invd[r1] : 0.0;
    for (int j0 = 0; j0 < n; j0 += CH_NB) {
      double a0[CH_NB], a1[CH_NB];
#pragma unroll
      for (int c = 0; c < CH_NB; c++) {
        const int j = min(j0 + c, n - 1);
        a0[c] = (r0 > j && r0 < n) ? A[r0 * ld + j] : 0.0;
        a1[c] = (r1 > j && r1 < n) ? A[r1 * ld + j] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < CH_NB; c++) {
        const int j = j0 + c;
        if (j < n) {  // wave-uniform
          // j is wave-uniform: scalar broadcasts, not LDS permutes
          const double yj = readlane_f64(j < 64 ? b0 : b1, j & 63) * readlane_f64(j < 64 ? inv0 : inv1, j & 63);
          if (lane == (j & 63)) {
            if (j < 64) b0 = yj; else b1 = yj;
          }
          b0 -= a0[c] * yj;  // a0 / a1 are zero for rows at or above j
          b1 -= a1[c] * yj;
        }
      }
    }
    for (int j0 = ((n - 1) / CH_NB) * CH_NB; j0 >= 0; j0 -= CH_NB) {
      double a0[CH_NB], a1[CH_NB];
#pragma unroll
      for (int c = 0; c < CH_NB; c++) {
        const int j = min(j0 + c, n - 1);
        a0[c] = (r0 < j && j0 + c < n) ? A[j * ld + r0] : 0.0;
        a1[c] = (r1 < j && j0 + c < n) ? A[j * ld + r1] : 0.0;
      }
#pragma unroll
      for (int c = CH_NB - 1; c >= 0; c--) {
        const int j = j0 + c;
        if (j < n) {
          const double xj = readlane_f64(j < 64 ? b0 : b1, j & 63) * readlane_f64(j < 64 ? inv0 : inv1, j & 63);
          if (lane == (j & 63)) {
            if (j < 64) b0 = xj; else b1 = xj;
          }
          b0 -= a0[c] * xj;  // zero for rows at or below j
          b1 -= a1[c] * xj;
        }
      }
    }
    if (r0 < n) dc[r0] = -b0;
    if (r1 < n) dc[r1] = -b1;
  }
  CHS_STAMP(4)
#ifdef CHS_TIMING
  if (tid == 0) printf("chol_small n %d cycles: load %lld panel-load+barrier %lld factor+solve+store %lld trailing %lld substitutions %lld\n", n, tp[0], tp[1], tp[2], tp[3], tp[4]);
#endif
  if (tid == 0) {
    *ok_flag = good ? 1 : 0;
    if (arm_flag) *arm_flag = 1;  // the 'all finite' flag of the step: armed here, cleared by the back-substitution kernel
  }
}

// delta_l = -P^-1 (b_l + sum_q W_q^T delta_c)
__global__ __launch_bounds__(256) void ba_backsub_kernel(BaDims D, const int* __restrict__ lm_start,
                                                         const int* __restrict__ obs_cam, const int* __restrict__ cam_free,
                                                         const double* __restrict__ F, const double* __restrict__ E,
                                                         const double* __restrict__ Pinv, const double* __restrict__ bl,
                                                         const double* __restrict__ dc, double* __restrict__ dl,
                                                         int* __restrict__ finite_flag = nullptr) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (finite_flag)  // the camera step is checked here as well (it saves the launch of ba_all_finite2_kernel)
    for (int j = l; j < D.n; j += gridDim.x * 256)
      if (!isfinite(dc[j])) *finite_flag = 0;
  if (l >= D.L) return;
  double t[3] = {bl[3 * (size_t)l], bl[3 * (size_t)l + 1], bl[3 * (size_t)l + 2]};
  for (int i = lm_start[l]; i < lm_start[l + 1]; i++) {
    const int fc = cam_free[obs_cam[i]];
    if (fc < 0) continue;
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    double fd0 = 0, fd1 = 0;
    for (int j = 0; j < 6; j++) {
      fd0 += f[j] * dc[6 * fc + j];
      fd1 += f[6 + j] * dc[6 * fc + j];
    }
    for (int j = 0; j < 3; j++) t[j] += e[j] * fd0 + e[3 + j] * fd1;
  }
  const double* Pi = Pinv + 9 * (size_t)l;
  for (int j = 0; j < 3; j++) {
    const double v = -(Pi[3 * j] * t[0] + Pi[3 * j + 1] * t[1] + Pi[3 * j + 2] * t[2]);
    dl[3 * (size_t)l + j] = v;
    if (finite_flag && !isfinite(v)) *finite_flag = 0;
  }
}

// model cost change partials: -(J d)^T (r + J d / 2)
__global__ __launch_bounds__(256) void ba_model_kernel(BaDims D, const int* __restrict__ obs_cam,
                                                       const int* __restrict__ obs_lm, const int* __restrict__ cam_free,
                                                       const double* __restrict__ r, const double* __restrict__ F,
                                                       const double* __restrict__ E, const double* __restrict__ dc,
                                                       const double* __restrict__ dl, double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v = 0;
  if (i < D.O) {
    const int fc = cam_free[obs_cam[i]], lm = obs_lm[i];
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    double m0 = 0, m1 = 0;
    if (fc >= 0)
      for (int j = 0; j < 6; j++) {
        m0 += f[j] * dc[6 * fc + j];
        m1 += f[6 + j] * dc[6 * fc + j];
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

// candidate = Plus(x, step .* scale): T * exp(delta) for poses (local_parameterization_se3.hpp:43-50),
// x + delta for points.  Per-workgroup partials: [0..nb) squared step norm, [nb..2nb) squared x norm
// (of the CURRENT x, non-constant blocks only).
__global__ __launch_bounds__(256) void ba_update_kernel(BaDims D, const int* __restrict__ cam_free,
                                                        const double* __restrict__ poses, const double* __restrict__ points,
                                                        const double* __restrict__ dc, const double* __restrict__ dl,
                                                        const double* __restrict__ scale_c, const double* __restrict__ scale_l,
                                                        double* __restrict__ cand_poses, double* __restrict__ cand_points,
                                                        double* __restrict__ partials, int nb) {
  __shared__ double sh[256];
  const int t = blockIdx.x * 256 + threadIdx.x;
  double step2 = 0, x2 = 0;
  if (t < D.C) {
    const int fc = cam_free[t];
    const double* T = poses + 7 * (size_t)t;
    double* o = cand_poses + 7 * (size_t)t;
    if (fc < 0) {
      for (int j = 0; j < 7; j++) o[j] = T[j];
    } else {
      double d[6];
      for (int j = 0; j < 6; j++) {
        d[j] = dc[6 * fc + j] * scale_c[6 * fc + j];
        step2 += d[j] * d[j];
      }
      for (int j = 0; j < 7; j++) x2 += T[j] * T[j];
      se3_plus(T, d, o);  // [upstream] Sophus SE3::exp (ba_device.h)
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

__global__ void ba_set_flags_kernel(int* __restrict__ flag) {
  if (threadIdx.x < 2) flag[threadIdx.x] = 1;
}

// both step vectors in one launch
__global__ void ba_all_finite2_kernel(int na, const double* __restrict__ a, int nb, const double* __restrict__ b,
                                      int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if ((i < na && !isfinite(a[i])) || (i < nb && !isfinite(b[i]))) *flag = 0;
}

// scalars[slot] and scalars[slot + 1] = sums of partials[0..n) and partials[n..2n): one launch, a workgroup each
__global__ __launch_bounds__(256) void ba_reduce2_kernel(const double* __restrict__ partials, int n, double* __restrict__ scalars,
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

// raw per-observation residual / Jacobian blocks in the caller's observation order (parity hook)
__global__ void ba_raw_blocks_kernel(BaDims D, const double* __restrict__ poses, const double* __restrict__ points,
                                     const double* __restrict__ intr, const int* __restrict__ cam_intr,
                                     const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                     const double* __restrict__ obs_uv, double* __restrict__ r, double* __restrict__ F,
                                     double* __restrict__ E) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.O) return;
  const int cam = obs_cam[i], lm = obs_lm[i], k = cam_intr[cam];
  double rr[2], FF[12], EE[6];
  residual_blocks(k ? D.model1 : D.model0, intr + 8 * k, poses + 7 * cam, points + 3 * lm, obs_uv + 2 * i, rr, FF, EE, true);
  r[2 * (size_t)i] = rr[0];
  r[2 * (size_t)i + 1] = rr[1];
  for (int j = 0; j < 12; j++) F[12 * (size_t)i + j] = FF[j];
  for (int j = 0; j < 6; j++) E[6 * (size_t)i + j] = EE[j];
}

}  // namespace

// ------------------------------------------------------- host-side state: ba_state.h; set-up and launchers
int ba_validate(vsl_ctx* ctx, const vsl_ba_problem* p) {
  if (!ctx) return VSL_ERR_INVALID;
  if (!p || p->n_cams <= 0 || p->n_lms <= 0 || p->n_obs <= 0 || !p->poses || !p->cam_fixed || !p->cam_intr || !p->intr ||
      !p->points || !p->obs_cam || !p->obs_lm || !p->obs_uv)
    return vsl_fail(ctx, VSL_ERR_INVALID, "bundle adjustment: null pointer or empty problem");
  for (int k = 0; k < 2; k++)
    if (p->cam_model[k] < 0 || p->cam_model[k] > 3) return vsl_fail(ctx, VSL_ERR_INVALID, "unknown camera model %d", p->cam_model[k]);
  for (int i = 0; i < p->n_obs; i++)
    if (p->obs_cam[i] < 0 || p->obs_cam[i] >= p->n_cams || p->obs_lm[i] < 0 || p->obs_lm[i] >= p->n_lms)
      return vsl_fail(ctx, VSL_ERR_INVALID, "observation %d references camera %d / landmark %d out of range", i, p->obs_cam[i], p->obs_lm[i]);
  for (int c = 0; c < p->n_cams; c++)
    if (p->cam_intr[c] < 0 || p->cam_intr[c] > 1) return vsl_fail(ctx, VSL_ERR_INVALID, "cam_intr[%d] = %d not in {0,1}", c, p->cam_intr[c]);
  return VSL_OK;
}

// the layout switches of a caller: its use and the context's diagnostics
static BaLayoutSwitches ba_layout_switches(vsl_ctx* ctx, const BaCaller& caller) {
  static const bool env_no_cyclic = getenv("VSL_BA_NO_CYCLIC") != nullptr;
  BaLayoutSwitches sw;
  sw.allow_band = (caller.use == BaUse::HOST_LOOP || caller.use == BaUse::SESSION || caller.use == BaUse::GLOBAL_COVARIANCE) &&
                  !caller.matrix_free;  // (no S: no band order to look for, the cameras keep their own numbering)
  sw.force_dense = ctx->ba_force_dense;
  sw.no_cyclic = ctx->ba_no_cyclic || env_no_cyclic || caller.use == BaUse::GLOBAL_COVARIANCE;
  sw.schur_atomics = ctx->ba_schur_atomics;
  sw.chol_no_bcr = ctx->chol_no_bcr;
  sw.chol_no_fused = ctx->chol_no_fused;
  return sw;
}

int ba_layout_of(vsl_ctx* ctx, const vsl_ba_problem* p, const BaCaller& caller, bool* banded) {
  try {
    const BaHostPlan hp = ba_host_plan(p, caller.graph_prob, ba_layout_switches(ctx, caller),
                                       BaPlanLimits{SCH_CMAX, SCH_KMAX, caller.run_max_obs, caller.run_max_lms}, [](const char*) {});
    *banded = hp.layout.banded;
  } catch (const std::bad_alloc&) {
    return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
  }
  return VSL_OK;
}

int ba_setup(vsl_ctx* ctx, const vsl_ba_problem* p, const vsl_ba_options* o, BaState& st, const BaCaller& caller) {
  BaTrace tr;
  const ArenaPolicy arena_policy =
      caller.use == BaUse::HOST_LOOP || caller.use == BaUse::COVARIANCE || caller.use == BaUse::GLOBAL_COVARIANCE ? ArenaPolicy::BORROWED
                                                                                                                   : ArenaPolicy::OWNED;
  ctx->last_pcg_solves = ctx->last_pcg_iterations = 0;  // (read-out of the matrix-free route: vsl_ctx_last_ba_pcg)
  ctx->last_pcg_iterations_last = 0;
  ctx->last_pcg_rel_residual = 0.0;
  BaDims& D = st.D;
  D.C = p->n_cams;
  D.L = p->n_lms;
  D.O = p->n_obs;
  D.model0 = p->cam_model[0];
  D.model1 = p->cam_model[1];
  D.use_huber = o ? o->use_huber : 1;
  D.huber = o ? o->huber_parameter : 1.0;
  // everything the host derives from the problem (ba_host_plan.h); the rest of this function is what needs the device
  const BaLayoutSwitches sw = ba_layout_switches(ctx, caller);
  BaHostPlan hp;
  size_t extra_bytes = caller.extra_bytes;
  try {
    // (runs_at_any_size: no system counts as small, so the landmark runs of the recompute form are always cut)
    hp = ba_host_plan(p, caller.graph_prob, sw,
                      BaPlanLimits{caller.runs_at_any_size ? 0 : SCH_CMAX, SCH_KMAX, caller.run_max_obs, caller.run_max_lms},
                      [&](const char* what) { tr.lap(what); });
    if (caller.plan_extra) {
      const int rc = caller.plan_extra(caller.plan_extra_self, hp, &extra_bytes);
      if (rc) return rc;
    }
  } catch (const std::bad_alloc&) {
    return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
  }
  D.nfree = hp.nfree;
  D.n = 6 * D.nfree;
  st.banded = hp.layout.banded;
  st.cyclic = hp.layout.cyclic;
  st.bw = hp.layout.bw;
  st.ldS = hp.layout.ldS;
  st.offS = hp.layout.offS;
  st.s_elems = hp.layout.s_elems;
  st.perm = std::move(hp.perm);
  st.small = hp.small;
  // the form of the iteration, BEFORE the arena is planned: only a session runs the recompute form (ba_large.h); "ba_no_fused" /
  // VSL_BA_NO_FUSED keep it on the operator-by-operator chain over stored r / F / E blocks (A/B runs, tests)
  static const bool env_no_fused = getenv("VSL_BA_NO_FUSED") != nullptr;
  st.recompute = caller.use == BaUse::SESSION && ba_recompute_form(hp, ctx->ba_no_fused || env_no_fused, ctx->ba_schur_atomics);
  st.matrix_free = caller.matrix_free;
  if (st.matrix_free) {
    // the matrix-free route works on the Z blocks of the recompute form and on nothing else: no quiet other route
    if (!st.recompute)
      return vsl_fail(ctx, VSL_ERR_INVALID,
                      "bundle adjustment, iterative Schur: needs the recompute form (a free camera, no landmark with more than %d "
                      "observations, no \"ba_no_fused\" / \"ba_schur_atomics\")", caller.run_max_obs);
    st.banded = st.cyclic = false;  // S does not exist: no layout
    st.bw = 0;
    st.ldS = st.offS = 0;
    st.s_elems = 0;
  }
  // (diagnostic read-out for benchmarks: vsl_ctx_last_ba_layout; 3 = matrix-free)
  ctx->last_ba_s_elems = (int64_t)st.s_elems;
  ctx->last_ba_banded = st.matrix_free ? 3 : (st.cyclic ? 2 : (st.banded ? 1 : 0));
  ctx->last_ba_bw = st.bw;
  BaStored& sb = st.sb;
  BaRecompute& rc = st.rc;
  rc.n_wg = st.recompute ? hp.n_wg : 0;
  st.nb_obs = (D.O + 255) / 256;
  st.nb_upd = (std::max(D.C, D.L) + 255) / 256;
  st.G = std::min(SCH_GMAX, (D.L + SCH_LB - 1) / SCH_LB);
  st.lm_per_wg = ((D.L + st.G - 1) / st.G + SCH_LB - 1) / SCH_LB * SCH_LB;
  st.G = (D.L + st.lm_per_wg - 1) / st.lm_per_wg;

  const size_t n = (size_t)D.n, L = (size_t)D.L, O = (size_t)D.O, C = (size_t)D.C;
  // enough workgroups per camera that a camera's observations are ~2 slices of 256 per workgroup (1 when cameras are many)
  st.cb_seg = D.nfree > 0 ? std::max(1, std::min(32, (int)(D.O / std::max(1, D.nfree) / 512))) : 1;
  rc.bl_seg = st.cb_seg;  // (one workgroup per 256 observations of a camera measured 121 us against 80: more gathers in flight than the L2 holds)
  const size_t nfree = (size_t)D.nfree, pair_elems = std::max<size_t>(hp.n_pairs < ((size_t)1 << 31) ? hp.n_pairs : 1, 1);
  ArenaPlan plan(66);
  plan.add(st.poses, 7 * C); plan.add(st.points, 3 * L); plan.add(st.intr, 16); plan.add(st.cam_intr, C); plan.add(st.cam_free, C);
  plan.add(st.free_cams, hp.free_cams.size()); plan.add(st.obs_cam, O); plan.add(st.obs_lm, O); plan.add(st.obs_uv, 2 * O);
  plan.add(st.lm_start, L + 1); plan.add(st.cam_start, C + 1); plan.add(st.cam_obs, O);
  plan.add(st.cand_poses, 7 * C); plan.add(st.cand_points, 3 * L);
  if (!st.recompute) { plan.add(sb.r, 2 * O); plan.add(sb.F, 12 * O); plan.add(sb.E, 6 * O); }
  plan.add(st.scale_c, n); plan.add(st.scale_l, 3 * L); plan.add(st.n2l, 3 * L);
  if (!st.recompute) plan.add(sb.grad_l, 3 * L);
  plan.add(st.cam_part, 33 * std::max<size_t>(1, nfree) * std::max(st.cb_seg, rc.bl_seg)); plan.add(st.H, 36 * nfree); plan.add(st.g_c, n);
  if (!st.recompute) { plan.add(sb.diag_c, n); plan.add(sb.diag_l, 3 * L); plan.add(sb.gabs, n + 3 * L); }
  plan.add(st.S, st.s_elems); plan.add(st.rhs, n);
  plan.add(st.Pinv, 9 * L); plan.add(st.bl, 3 * L); plan.add(st.dc, n);
  if (!st.recompute) {
    plan.add(sb.dl, 3 * L);
    plan.add(sb.partials, (size_t)(2 * std::max(st.nb_obs, st.nb_upd) + 16));
  }
  plan.add(st.scalars, 16 + 2 /* = 4 ints */);  // 16 scalars, then flag: 4 ints in the 16 bytes of 2 doubles
  if (st.small) {
    plan.add(sb.S_part, n * n * st.G);
    plan.add(sb.rhs_part, n * st.G);
  } else {
    st.hbp1 = st.banded ? (st.bw - 5) / 6 + 1 : 0;
    st.n_slots = st.banded ? D.nfree * st.hbp1 : D.nfree * (D.nfree + 1) / 2;
    st.n_pairs_cap = hp.n_pairs;
    st.pair_l0 = st.pair_lc = -1;
    if (!st.matrix_free) {  // (the matrix-free route gathers nothing: no pair lists)
      plan.add(st.pair_cnt, (size_t)st.n_slots + 1);
      plan.add(st.pair_start, (size_t)st.n_slots + 1);
      plan.add(st.pairs, 2 * pair_elems);
    }
    plan.add(st.cam_pos, O);
    if (!st.recompute) plan.add(sb.Wg, 18 * O);
    plan.add(st.Yg, 18 * O);
  }
  if (st.recompute) {
    plan.add(rc.wg_lm, (size_t)rc.n_wg + 1);
    plan.add(rc.lpart, 4 * (size_t)rc.n_wg);
    plan.add(rc.pbs, 3 * L);
    plan.add(rc.cam_lm, O);
    plan.add(rc.cam_uv, 2 * O);
  }
  if (st.matrix_free) {
    plan.add(rc.pcg_x, n); plan.add(rc.pcg_r, n); plan.add(rc.pcg_z, n); plan.add(rc.pcg_p, n); plan.add(rc.pcg_q, n);
    plan.add(rc.pcg_t, 3 * L);
    plan.add(rc.pcg_part, 6 * nfree * (size_t)rc.bl_seg);
    plan.add(rc.pcg_minv, 36 * nfree);
    plan.add(rc.pcg_rec, 1);
  }
  if (caller.use == BaUse::HOST_LOOP) {
    plan.add(sb.r2, 2 * O); plan.add(sb.F2, 12 * O); plan.add(sb.E2, 6 * O); plan.add(sb.n2l2, 3 * L); plan.add(sb.grad_l2, 3 * L);
    plan.add(sb.H2, 36 * nfree); plan.add(sb.g_c2, n); plan.add(sb.diag_c2, n); plan.add(sb.diag_l2, 3 * L);
  }
  if (caller.use == BaUse::SESSION) plan.add(st.diagc_keep, std::max<size_t>(n, 1));
  if (extra_bytes) plan.add(st.extra, extra_bytes);
  VSL_HIP(ctx, st.arena.acquire(ctx, arena_policy, plan));
  st.flag = (int*)(st.scalars + 16);
  tr.lap("arena", plan.total());
  auto up = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  };
  VSL_HIP(ctx, up(st.poses, p->poses, 8 * 7 * C));
  VSL_HIP(ctx, up(st.points, p->points, 8 * 3 * L));
  VSL_HIP(ctx, up(st.intr, p->intr, 8 * 16));
  VSL_HIP(ctx, up(st.cam_intr, p->cam_intr, 4 * C));
  VSL_HIP(ctx, up(st.cam_free, hp.cam_free.data(), 4 * C));
  VSL_HIP(ctx, up(st.free_cams, hp.free_cams.data(), 4 * hp.free_cams.size()));
  VSL_HIP(ctx, up(st.obs_cam, hp.obs_cam, 4 * O));
  VSL_HIP(ctx, up(st.obs_lm, hp.obs_lm, 4 * O));
  VSL_HIP(ctx, up(st.obs_uv, hp.obs_uv, 16 * O));
  VSL_HIP(ctx, up(st.lm_start, hp.lm_start.data(), 4 * (L + 1)));
  VSL_HIP(ctx, up(st.cam_start, hp.cam_start.data(), 4 * (C + 1)));
  VSL_HIP(ctx, up(st.cam_obs, hp.cam_obs.data(), 4 * O));
  if (!st.small) VSL_HIP(ctx, up(st.cam_pos, hp.cam_pos.data(), 4 * O));
  if (st.recompute) VSL_HIP(ctx, up(rc.wg_lm, hp.wg_lm.data(), 4 * hp.wg_lm.size()));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the uploads above read host vectors that die here
  tr.lap("uploads");
  return VSL_OK;
}

// ---- the plain-pointer launchers of ba_state.h: the ONE launch site of each of these kernels.  The BaCommon launchers
// below, the host loop and the intrinsics solver go through them, and so does the rig chain of ba_rig.hip.
int vsl_ba_linearize_launch(vsl_ctx* ctx, const BaDims& D, const double* poses, const double* points, const double* intr,
                            const double* tcb, const int* cam_intr, const int* cam_free, const int* obs_cam, const int* obs_lm,
                            const double* obs_uv, const double* scale_c, const double* scale_l, double* r, double* F, double* E,
                            double* partials) {
  const dim3 grid((D.O + 255) / 256);
  if (tcb)
    hipLaunchKernelGGL(ba_linearize_kernel<true>, grid, dim3(256), 0, ctx->stream, D, poses, points, intr, cam_intr, cam_free, obs_cam,
                       obs_lm, obs_uv, scale_c, scale_l, r, F, E, partials, 1, tcb);
  else
    hipLaunchKernelGGL(ba_linearize_kernel<false>, grid, dim3(256), 0, ctx->stream, D, poses, points, intr, cam_intr, cam_free, obs_cam,
                       obs_lm, obs_uv, scale_c, scale_l, r, F, E, partials, 1, (const double*)nullptr);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_reduce_launch(vsl_ctx* ctx, const double* partials, int n, double* scalars, int slot, bool is_max) {
  hipLaunchKernelGGL(ba_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, partials, n, scalars, slot, is_max ? 1 : 0);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_reduce2_launch(vsl_ctx* ctx, const double* partials, int n, double* scalars, int slot) {
  hipLaunchKernelGGL(ba_reduce2_kernel, dim3(2), dim3(256), 0, ctx->stream, partials, n, scalars, slot);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_lm_cols_launch(vsl_ctx* ctx, int L, const int* lm_start, const double* r, const double* E, double* n2l, double* grad_l) {
  BaDims D{};
  D.L = L;  // all the kernel reads
  hipLaunchKernelGGL(ba_lm_cols_kernel, dim3((L + 255) / 256), dim3(256), 0, ctx->stream, D, lm_start, r, E, n2l, grad_l);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_block_finish_launch(vsl_ctx* ctx, int nfree, int nseg, const double* part, double* H, double* g) {
  hipLaunchKernelGGL(ba_cam_block_finish_kernel, dim3((nfree * 27 + 255) / 256), dim3(256), 0, ctx->stream, nfree, nseg, part, H, g);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_make_scale_launch(vsl_ctx* ctx, int nfree, int L, const double* H, const double* n2l, double* scale_c, double* scale_l) {
  hipLaunchKernelGGL(ba_make_scale_kernel, dim3((std::max(6 * nfree, 3 * L) + 255) / 256), dim3(256), 0, ctx->stream, nfree, L, H, n2l,
                     scale_c, scale_l);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_diag_gmax_launch(vsl_ctx* ctx, int nfree, int L, const double* H, const double* n2l, const double* g_c, const double* grad_l,
                            const double* scale_c, const double* scale_l, double* diag_c, double* diag_l, double* gabs,
                            double* scalars, int slot) {
  const int nb = (std::max(6 * nfree, 3 * L) + 255) / 256;
  hipLaunchKernelGGL(ba_diag_kernel, dim3(nb), dim3(256), 0, ctx->stream, nfree, L, H, n2l, g_c, grad_l, scale_c, scale_l, diag_c,
                     diag_l, gabs);
  return vsl_ba_reduce_launch(ctx, gabs, nb, scalars, slot, true);
}

int vsl_ba_model_launch(vsl_ctx* ctx, int O, const int* obs_cam, const int* obs_lm, const int* cam_free, const double* r,
                        const double* F, const double* E, const double* dc, const double* dl, double* partials) {
  BaDims D{};
  D.O = O;  // all the kernel reads
  hipLaunchKernelGGL(ba_model_kernel, dim3((O + 255) / 256), dim3(256), 0, ctx->stream, D, obs_cam, obs_lm, cam_free, r, F, E, dc, dl,
                     partials);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_update_launch(vsl_ctx* ctx, int n_poses, int L, const int* pose_free, const double* poses, const double* points,
                         const double* dc, const double* dl, const double* scale_c, const double* scale_l, double* cand_poses,
                         double* cand_points, double* partials, double* scalars, int slot) {
  BaDims D{};
  D.C = n_poses;  // the kernel reads the two counts
  D.L = L;
  const int nb = (std::max(n_poses, L) + 255) / 256;
  hipLaunchKernelGGL(ba_update_kernel, dim3(nb), dim3(256), 0, ctx->stream, D, pose_free, poses, points, dc, dl, scale_c, scale_l,
                     cand_poses, cand_points, partials, nb);
  return vsl_ba_reduce2_launch(ctx, partials, nb, scalars, slot);
}

int ba_linearize(vsl_ctx* ctx, BaCommon& st, BaStored& sb, bool scaled, int cost_slot) {
  VslStage s(ctx, VSL_STAGE_BA_LIN);
  int rc = vsl_ba_linearize_launch(ctx, st.D, st.poses, st.points, st.intr, nullptr, st.cam_intr, st.cam_free, st.obs_cam, st.obs_lm,
                                   st.obs_uv, scaled ? st.scale_c : nullptr, scaled ? st.scale_l : nullptr, sb.r, sb.F, sb.E,
                                   sb.partials);
  if (rc) return rc;
  return vsl_ba_reduce_launch(ctx, sb.partials, st.nb_obs, st.scalars, cost_slot, false);
}

int ba_columns(vsl_ctx* ctx, BaCommon& st, BaStored& sb) {
  const BaDims& D = st.D;
  VslStage s(ctx, VSL_STAGE_BA_LIN);
  int rc = vsl_ba_lm_cols_launch(ctx, D.L, st.lm_start, sb.r, sb.E, st.n2l, sb.grad_l);
  if (rc || D.nfree == 0) return rc;
  hipLaunchKernelGGL(ba_cam_block_kernel, dim3(D.nfree, st.cb_seg), dim3(256), 0, ctx->stream, st.free_cams, st.cam_start, st.cam_obs,
                     sb.r, sb.F, st.cam_part);
  return vsl_ba_block_finish_launch(ctx, D.nfree, st.cb_seg, st.cam_part, st.H, st.g_c);
}

// workgroups of ba_schur_gather_kernel: one per slot; in band form eight equal row ranges (see the kernel)
static unsigned gather_grid(const BaCommon& st) {
  if (st.hbp1 <= 0) return (unsigned)st.n_slots;
  const int nrows = st.n_slots / st.hbp1;
  return 8u * (unsigned)((nrows + 7) / 8) * (unsigned)st.hbp1;
}

int ba_pair_lists(vsl_ctx* ctx, BaCommon& st, int l0, int lc) {
  if (st.pair_l0 == l0 && st.pair_lc == lc) return VSL_OK;
  VSL_HIP(ctx, hipMemsetAsync(st.pair_cnt, 0, sizeof(int) * ((size_t)st.n_slots + 1), ctx->stream));
  hipLaunchKernelGGL(ba_pair_list_kernel<false>, dim3((lc + 255) / 256), dim3(256), 0, ctx->stream, l0, lc, st.lm_start, st.obs_cam,
                     st.cam_free, st.cam_pos, st.hbp1, st.cyclic ? st.D.nfree : 0, st.pair_cnt, (const int*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(ba_pair_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, st.n_slots, st.pair_cnt, st.pair_start);
  VSL_HIP(ctx, hipMemsetAsync(st.pair_cnt, 0, sizeof(int) * ((size_t)st.n_slots + 1), ctx->stream));
  hipLaunchKernelGGL(ba_pair_list_kernel<true>, dim3((lc + 255) / 256), dim3(256), 0, ctx->stream, l0, lc, st.lm_start, st.obs_cam,
                     st.cam_free, st.cam_pos, st.hbp1, st.cyclic ? st.D.nfree : 0, st.pair_cnt, st.pair_start, st.pairs);
  hipLaunchKernelGGL(ba_pair_sort_kernel, dim3(st.n_slots), dim3(64), 0, ctx->stream, st.pair_start, st.pairs);
  VSL_CHECK_LAUNCH(ctx);
  st.pair_l0 = l0;
  st.pair_lc = lc;
  return VSL_OK;
}

int ba_schur(vsl_ctx* ctx, BaCommon& st, BaStored& sb, bool damp, double radius, int l0, int lc, bool keep_backsub, bool lower_only) {
  const BaDims& D = st.D;
  const int n = D.n;
  // no free camera: there is no S, but the back-substitution still needs P^-1 and b of every landmark (n = 0 is a
  // small system: ba_schur_small_kernel writes both and owns no entry of S)
  if (n == 0 && !keep_backsub) return VSL_OK;
  VslStage s(ctx, VSL_STAGE_BA_SCHUR);
  const double inv_radius = damp ? 1.0 / radius : 0.0;
  const double* dgl = damp ? sb.diag_l : nullptr;
  const double* dgc = damp ? sb.diag_c : nullptr;
  double* Pinv = keep_backsub ? st.Pinv : nullptr;
  double* bl = keep_backsub ? st.bl : nullptr;
  if (st.small) {
    const int lpw = ((lc + st.G - 1) / st.G + SCH_LB - 1) / SCH_LB * SCH_LB;
    const int G = lpw > 0 ? (lc + lpw - 1) / lpw : 0;
    const bool block3 = !ctx->ba_schur_entries;
    if (G > 0) {
      if (block3)
        hipLaunchKernelGGL(ba_schur_small_kernel<true>, dim3(G), dim3(SCH_THREADS), 0, ctx->stream, D, st.lm_start, st.obs_cam,
                           st.cam_free, sb.r, sb.F, sb.E, dgl, inv_radius, l0, lc, lpw, sb.S_part, sb.rhs_part, Pinv, bl);
      else
        hipLaunchKernelGGL(ba_schur_small_kernel<false>, dim3(G), dim3(SCH_THREADS), 0, ctx->stream, D, st.lm_start, st.obs_cam,
                           st.cam_free, sb.r, sb.F, sb.E, dgl, inv_radius, l0, lc, lpw, sb.S_part, sb.rhs_part, Pinv, bl);
    }
    if (n > 0)
      hipLaunchKernelGGL(ba_schur_finish_kernel, dim3((n * n + n + 15) / 16), dim3(256), 0, ctx->stream, n, G, sb.S_part, sb.rhs_part,
                         st.H, st.g_c, dgc, inv_radius, st.S, st.rhs, block3 ? 1 : 0);
  } else {
    VSL_HIP(ctx, hipMemsetAsync(st.S, 0, sizeof(double) * st.s_elems, ctx->stream));
    VSL_HIP(ctx, hipMemsetAsync(st.rhs, 0, sizeof(double) * n, ctx->stream));
    const int lower_mode = st.banded ? 2 : ((lower_only && n > 128) ? 1 : 0);  // n <= 128 is solved by ba_chol_small_kernel (full matrix)
    // (pair lists index with 32-bit positions: a problem with 2^31 pairs or more keeps the atomic form)
    if (lc > 0 && (ctx->ba_schur_atomics || st.n_pairs_cap >= ((size_t)1 << 31)))
      hipLaunchKernelGGL(ba_schur_atomic_kernel, dim3((lc + 3) / 4), dim3(256), 0, ctx->stream, D, st.lm_start, st.obs_cam,
                         st.cam_free, sb.r, sb.F, sb.E, dgl, inv_radius, l0, lc, st.S_eff(), st.rhs, Pinv, bl, lower_mode, st.ldS);
    else if (lc > 0) {
      int rc = ba_pair_lists(ctx, st, l0, lc);
      if (rc) return rc;
      hipLaunchKernelGGL(ba_schur_prep_kernel, dim3((lc + 3) / 4), dim3(256), 0, ctx->stream, D, st.lm_start, st.obs_cam,
                         st.cam_free, st.cam_pos, sb.r, sb.F, sb.E, dgl, inv_radius, l0, lc, sb.Wg, st.Yg, st.rhs, Pinv, st.bl);
      if (D.nfree > 0)
        hipLaunchKernelGGL(ba_schur_rhs_kernel, dim3(D.nfree), dim3(64), 0, ctx->stream, D.nfree, st.free_cams, st.cam_start,
                           st.cam_obs, st.obs_lm, st.Yg, st.bl, l0, lc, st.rhs);
      hipLaunchKernelGGL(ba_schur_gather_kernel, dim3(gather_grid(st)), dim3(64), 0, ctx->stream, st.n_slots, st.hbp1,
                         st.pair_start, st.pairs, sb.Wg, st.Yg, st.S_eff(), st.ldS, lower_mode);
    }
    hipLaunchKernelGGL(ba_add_cam_blocks_kernel, dim3((D.nfree * 36 + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, st.H, st.g_c,
                       dgc, inv_radius, st.S_eff(), st.rhs, st.ldS, st.banded ? 1 : 0);
  }
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int ba_solve_enqueue(vsl_ctx* ctx, BaCommon& st, bool flags_set) {
  const int n = st.D.n;
  VslStage s(ctx, VSL_STAGE_BA_SOLVE);
  if ((n == 0 || n > 128) && !flags_set) hipLaunchKernelGGL(ba_set_flags_kernel, dim3(1), dim3(64), 0, ctx->stream, st.flag);
  if (n == 0) return VSL_OK;
  if (n <= 128) {
    hipLaunchKernelGGL(ba_chol_small_kernel, dim3(1), dim3(256), 0, ctx->stream, n, st.S, st.rhs, st.dc, st.flag + 1, st.flag);
  } else {
    // dc = -(S^-1 rhs): the solver writes the negated solution as well
    int rc = vsl_chol_solve_band_dev(ctx, st.S_eff(), st.rhs, n, st.ldS, st.bw, st.flag + 1, st.cyclic ? 1 : 0, st.dc);
    if (rc) return rc;
  }
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

// The step chain of the stored-blocks form, written once: the host loop of vsl_bundle_adjust and the session's
// StoredForm (through ba_candidate) both run it.  Everything is enqueued; a failed factorisation leaves a stale or
// non-finite dc, which these kernels only do arithmetic with (no index depends on step data) and which the caller
// discards on flag[1] = 0.
int ba_step_from_dc(vsl_ctx* ctx, BaCommon& st, BaStored& sb) {
  const BaDims& D = st.D;
  hipLaunchKernelGGL(ba_backsub_kernel, dim3((D.L + 255) / 256), dim3(256), 0, ctx->stream, D, st.lm_start, st.obs_cam,
                     st.cam_free, sb.F, sb.E, st.Pinv, st.bl, st.dc, sb.dl, st.flag);
  int rc = vsl_ba_model_launch(ctx, D.O, st.obs_cam, st.obs_lm, st.cam_free, sb.r, sb.F, sb.E, st.dc, sb.dl, sb.partials);
  if (rc) return rc;
  if ((rc = vsl_ba_reduce_launch(ctx, sb.partials, st.nb_obs, st.scalars, 2, false))) return rc;
  return vsl_ba_update_launch(ctx, D.C, D.L, st.cam_free, st.poses, st.points, st.dc, sb.dl, st.scale_c, st.scale_l, st.cand_poses,
                              st.cand_points, sb.partials, st.scalars, 3);
}

int read_scalars(vsl_ctx* ctx, BaCommon& st, double* out, int n) {
  VSL_HIP(ctx, hipMemcpyAsync(out, st.scalars, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VSL_OK;
}

namespace {
// camera-only parts of the step / x norms (identical on every rank).  A kernel of the session's stored-blocks step that
// lives here, beside the chain it runs in: compiled in ba_session.hip its LDS reads come out differently
__global__ __launch_bounds__(256) void sess_cam_norms_kernel(BaDims D, const int* __restrict__ cam_free,
                                                             const double* __restrict__ poses, const double* __restrict__ dc,
                                                             const double* __restrict__ scale_c, double* __restrict__ scalars) {
  __shared__ double sh[256];
  double step2 = 0, x2 = 0;
  for (int c = threadIdx.x; c < D.C; c += 256) {
    const int fc = cam_free[c];
    if (fc < 0) continue;
    for (int j = 0; j < 6; j++) {
      const double d = dc[6 * fc + j] * scale_c[6 * fc + j];
      step2 += d * d;
    }
    for (int j = 0; j < 7; j++) x2 += poses[7 * (size_t)c + j] * poses[7 * (size_t)c + j];
  }
  const double a = block_sum_256(step2, sh);
  __syncthreads();
  const double b = block_sum_256(x2, sh);
  if (threadIdx.x == 0) {
    scalars[6] = a;
    scalars[7] = b;
  }
}
}  // namespace

// ---- what only the session's stored-blocks form launches (ba_session.hip): no stage of their own, as the session runs them
int ba_apply_scale(vsl_ctx* ctx, BaCommon& st, BaStored& sb) {
  hipLaunchKernelGGL(ba_apply_scale_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, st.D.O, st.cam_free, st.obs_cam, st.obs_lm,
                     st.scale_c, st.scale_l, sb.F, sb.E);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int ba_schur_gather(vsl_ctx* ctx, BaCommon& st, const double* W, const double* Y, int lower_mode) {
  hipLaunchKernelGGL(ba_schur_gather_kernel, dim3(gather_grid(st)), dim3(64), 0, ctx->stream, st.n_slots, st.hbp1,
                     st.pair_start, st.pairs, W, Y, st.S_eff(), st.ldS, lower_mode);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int ba_max_of(vsl_ctx* ctx, const double* v, int n, double* dst) { return vsl_ba_reduce_launch(ctx, v, n, dst, 0, true); }

int ba_candidate(vsl_ctx* ctx, BaCommon& st, BaStored& sb) {
  const BaDims& D = st.D;
  int rc = ba_step_from_dc(ctx, st, sb);
  if (rc) return rc;
  hipLaunchKernelGGL(sess_cam_norms_kernel, dim3(1), dim3(256), 0, ctx->stream, D, st.cam_free, st.poses, st.dc, st.scale_c,
                     st.scalars);
  hipLaunchKernelGGL(ba_cost_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, D, st.cand_poses, st.cand_points, st.intr,
                     st.cam_intr, st.obs_cam, st.obs_lm, st.obs_uv, 0, D.O, sb.partials);
  return vsl_ba_reduce_launch(ctx, sb.partials, st.nb_obs, st.scalars, 5, false);
}

int vsl_ba_chol_small_launch(vsl_ctx* ctx, int n, const double* S, const double* rhs, double* dc, int* ok_flag) {
  hipLaunchKernelGGL(ba_chol_small_kernel, dim3(1), dim3(256), 0, ctx->stream, n, S, rhs, dc, ok_flag, (int*)nullptr);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

extern "C" int vsl_ba_residuals_jacobians(vsl_ctx* ctx, const vsl_ba_problem* prob, double* r, double* J_pose,
                                          double* J_point) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!r || !J_pose || !J_point) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_residuals_jacobians: null output");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  BaState st;
  if ((rc = ba_setup(ctx, prob, nullptr, st, BaCaller{BaUse::PARITY_HOOK}))) return rc;
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  hipLaunchKernelGGL(ba_raw_blocks_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, D, st.poses, st.points, st.intr, st.cam_intr,
                     st.obs_cam, st.obs_lm, st.obs_uv, sb.r, sb.F, sb.E);
  VSL_CHECK_LAUNCH(ctx);
  std::vector<double> hr(2 * (size_t)D.O), hF(12 * (size_t)D.O), hE(6 * (size_t)D.O);
  VSL_HIP(ctx, hipMemcpyAsync(hr.data(), sb.r, 8 * hr.size(), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hF.data(), sb.F, 8 * hF.size(), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hE.data(), sb.E, 8 * hE.size(), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int q = 0; q < D.O; q++) {  // back to the caller's observation order
    const size_t i = st.perm.empty() ? (size_t)q : (size_t)st.perm[q];
    memcpy(r + 2 * i, &hr[2 * (size_t)q], 16);
    memcpy(J_pose + 12 * i, &hF[12 * (size_t)q], 96);
    memcpy(J_point + 6 * i, &hE[6 * (size_t)q], 48);
  }
  return VSL_OK;
}

extern "C" int vsl_ba_linearize(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, int lm_first,
                                int lm_count, double* S, double* g, double* cost, int* n_free) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!opt || !S || !g || !cost || !n_free) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_linearize: null argument");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  BaState st;
  if ((rc = ba_setup(ctx, prob, opt, st, BaCaller{BaUse::SINGLE_LINEARIZE}))) return rc;
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  int l0 = 0, lc = D.L;
  if (lm_count >= 0) {
    if (lm_first < 0 || lm_first > D.L) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_linearize: lm_first out of range");
    l0 = lm_first;
    lc = std::min(lm_count, D.L - lm_first);
  }
  if ((rc = ba_linearize(ctx, st, sb, false))) return rc;
  if (lm_count >= 0) {
    // restrict to the observations of the landmark range: zero the others' blocks so that the camera
    // sums and the cost only see the range (observations are sorted by landmark => one contiguous run)
    std::vector<int> lm_start(D.L + 1);
    VSL_HIP(ctx, hipMemcpyAsync(lm_start.data(), st.lm_start, sizeof(int) * lm_start.size(), hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t o0 = (size_t)lm_start[l0], o1 = (size_t)lm_start[l0 + lc];
    if (o0 > 0) {
      VSL_HIP(ctx, hipMemsetAsync(sb.r, 0, 16 * o0, ctx->stream));
      VSL_HIP(ctx, hipMemsetAsync(sb.F, 0, 96 * o0, ctx->stream));
      VSL_HIP(ctx, hipMemsetAsync(sb.E, 0, 48 * o0, ctx->stream));
    }
    if (o1 < (size_t)D.O) {
      VSL_HIP(ctx, hipMemsetAsync(sb.r + 2 * o1, 0, 16 * ((size_t)D.O - o1), ctx->stream));
      VSL_HIP(ctx, hipMemsetAsync(sb.F + 12 * o1, 0, 96 * ((size_t)D.O - o1), ctx->stream));
      VSL_HIP(ctx, hipMemsetAsync(sb.E + 6 * o1, 0, 48 * ((size_t)D.O - o1), ctx->stream));
    }
    const int oc = (int)(o1 - o0);
    const int nb = (oc + 255) / 256;
    if (nb > 0)
      hipLaunchKernelGGL(ba_cost_kernel, dim3(nb), dim3(256), 0, ctx->stream, D, st.poses, st.points, st.intr, st.cam_intr,
                         st.obs_cam, st.obs_lm, st.obs_uv, (int)o0, oc, sb.partials);
    if ((rc = vsl_ba_reduce_launch(ctx, sb.partials, nb, st.scalars, 0, false))) return rc;
  }
  if ((rc = ba_columns(ctx, st, sb))) return rc;
  if ((rc = ba_schur(ctx, st, sb, false, 1.0, l0, lc, false, false))) return rc;
  double sc[1];
  if ((rc = read_scalars(ctx, st, sc, 1))) return rc;
  *cost = sc[0];
  *n_free = D.nfree;
  if (D.n > 0) {
    VSL_HIP(ctx, hipMemcpy(S, st.S, sizeof(double) * (size_t)D.n * D.n, hipMemcpyDeviceToHost));
    VSL_HIP(ctx, hipMemcpy(g, st.rhs, sizeof(double) * D.n, hipMemcpyDeviceToHost));
  }
  return VSL_OK;
}

// ---- what the two speculative host loops (vsl_bundle_adjust below, vsl_bundle_adjust_rig in ba_rig.hip) share besides
// lm_speculative_loop: the one copy per iteration and the summary's tail
int ba_fetch_step(vsl_ctx* ctx, const double* scalars, double* sc16, int* flags2) {
  void* hp = nullptr;
  int rc = vsl_ctx_hpinned(ctx, 256, &hp);
  if (rc) return rc;
  VSL_HIP(ctx, hipMemcpyAsync(hp, scalars, 16 * sizeof(double) + 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(sc16, hp, 16 * sizeof(double));
  memcpy(flags2, (const char*)hp + 16 * sizeof(double), 2 * sizeof(int));
  return VSL_OK;
}

// per-stage device times (summary.linearize_ms / schur_ms / solve_ms) only when the context has profiling switched
// on (vsl_ctx_set_profiling): the HIP events around every stage cost ~60 us per LM iteration of a local window
// (0.36 -> 0.30 ms per iteration), so a plain call goes without them
BaSolveTimes::BaSolveTimes(vsl_ctx* ctx, double t_start_ms) : t_start(t_start_ms), prof_was(ctx->profiling) {
  for (int k = 0; k < 3; k++) base_ms[k] = ctx->stage_ms[VSL_STAGE_BA_LIN + k];
}

void ba_finish_summary(vsl_ctx* ctx, const BaSolveTimes& t, int verbosity, const char* label, vsl_ba_summary& sum,
                       vsl_ba_summary* out) {
  double ms;
  int64_t cnt;
  vsl_ctx_stage_ms(ctx, VSL_STAGE_BA_LIN, &ms, &cnt);
  sum.linearize_ms = ctx->stage_ms[VSL_STAGE_BA_LIN] - t.base_ms[0];
  sum.schur_ms = ctx->stage_ms[VSL_STAGE_BA_SCHUR] - t.base_ms[1];
  sum.solve_ms = ctx->stage_ms[VSL_STAGE_BA_SOLVE] - t.base_ms[2];
  vsl_ctx_set_profiling(ctx, t.prof_was ? 1 : 0);
  sum.total_ms = now_ms() - t.t_start;
  if (verbosity >= 1)
    fprintf(stderr, "%s iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n", label, sum.iterations,
            sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
  if (out) *out = sum;
}

// vsl_bundle_adjust behind the set-up: the speculative host loop (lm_policy.h) on the stored-blocks chain
static int ba_host_loop_solve(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, BaState& st, bool no_fused,
                              double t_start, vsl_ba_summary* summary) {
  int rc;
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  const int nc = D.n;
  // A window without a free camera (the application's first keyframe).  [upstream] Ceres moves the landmarks alone, and
  // so do this loop under "ba_no_fused" and the session.  The DEFAULT path never has: ba_schur used to return before P^-1
  // and b existed, every step came out invalid and the landmarks stayed (termination 4).  The application's trajectories
  // rest on that, so the default path keeps it -- now with zeroed blocks instead of unwritten ones -- until it is changed
  // on purpose.
  const bool hold_landmarks = nc == 0 && !no_fused;
  if (hold_landmarks) {
    VSL_HIP(ctx, hipMemsetAsync(st.Pinv, 0, sizeof(double) * 9 * (size_t)D.L, ctx->stream));
    VSL_HIP(ctx, hipMemsetAsync(st.bl, 0, sizeof(double) * 3 * (size_t)D.L, ctx->stream));
  }
  vsl_ba_summary sum;
  memset(&sum, 0, sizeof(sum));
  const BaSolveTimes times(ctx, t_start);

  // iteration 0: evaluate, Jacobi scaling from the unscaled Jacobian, then scale it
  if ((rc = ba_linearize(ctx, st, sb, false))) return rc;
  if ((rc = ba_columns(ctx, st, sb))) return rc;
  if ((rc = vsl_ba_make_scale_launch(ctx, D.nfree, D.L, st.H, st.n2l, st.scale_c, st.scale_l))) return rc;
  if ((rc = ba_apply_scale(ctx, st, sb))) return rc;
  if ((rc = ba_columns(ctx, st, sb))) return rc;

  auto diag_and_gmax = [&](int slot) -> int {
    return vsl_ba_diag_gmax_launch(ctx, D.nfree, D.L, st.H, st.n2l, st.g_c, sb.grad_l, st.scale_c, st.scale_l, sb.diag_c, sb.diag_l,
                                   sb.gabs, st.scalars, slot);
  };
  if ((rc = diag_and_gmax(1))) return rc;
  double sc[2];
  if ((rc = read_scalars(ctx, st, sc, 2))) return rc;
  sum.initial_cost = sc[0];

  // One host round trip per LM iteration (lm_speculative_loop, lm_policy.h): the whole iteration is enqueued without
  // waiting -- Schur, Cholesky, back-substitution, model / step norms, candidate parameters AND the linearisation at the
  // candidate (into the second set of blocks: its cost is the candidate's cost, and if the step is accepted it is the
  // next iteration's linearisation already) -- then ONE copy brings back [Cholesky ok, finite] + 7 scalars and the host
  // applies the [upstream] Ceres step policy.  A rejected or invalid step swaps the sets back; its speculative work
  // (~60 us of device time) is the price.  (The first version synchronised three times per iteration: after the
  // Cholesky, after the candidate cost, after the re-linearisation.)
  auto enqueue = [&](double radius) -> int {
    int e;
    if ((e = ba_schur(ctx, st, sb, true, radius, 0, D.L, !hold_landmarks, true))) return e;
    if ((e = ba_solve_enqueue(ctx, st))) return e;  // flag[1] = Cholesky ok
    {
      VslStage s(ctx, VSL_STAGE_BA_SOLVE);
      if ((e = ba_step_from_dc(ctx, st, sb))) return e;
    }
    // speculative: the candidate becomes the current point, its linearisation goes to the other set;
    // scalars[5] = cost there, scalars[6] = max |gradient| there (slots 0/1 keep the current point's values)
    st.swap_sets();
    if ((e = ba_linearize(ctx, st, sb, true, 5))) return e;
    if ((e = ba_columns(ctx, st, sb))) return e;
    return diag_and_gmax(6);
  };
  auto fetch = [&](double* s16, int* flags) -> int { return ba_fetch_step(ctx, st.scalars, s16, flags); };
  // (accepted: the sets stay swapped, the speculative linearisation is the current one)
  auto settle = [&](bool accepted) {
    if (!accepted) st.swap_sets();
  };
  LmLoopResult lm;
  if ((rc = lm_speculative_loop(opt->max_num_iterations, opt->verbosity, sc[0], sc[1], enqueue, fetch, settle, &lm))) return rc;
  sum.iterations = lm.iterations;
  sum.successful_steps = lm.successful_steps;
  sum.termination = lm.termination;
  sum.final_cost = lm.final_cost;
  VSL_HIP(ctx, hipMemcpyAsync(prob->poses, st.poses, sizeof(double) * 7 * (size_t)D.C, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(prob->points, st.points, sizeof(double) * 3 * (size_t)D.L, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ba_finish_summary(ctx, times, opt->verbosity, "vsl BA:", sum, summary);
  return VSL_OK;
}

// [upstream] ceres::Solve, TRUST_REGION / LEVENBERG_MARQUARDT / Schur, defaults (see oracle/orc_ba.cpp
// for the option values this loop restates).
extern "C" int vsl_bundle_adjust(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt,
                                 vsl_ba_summary* summary) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!opt) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_bundle_adjust: options are null");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  static const bool env_no_fused = getenv("VSL_BA_NO_FUSED") != nullptr;  // same switch for applications without a diagnostics hook
  const bool no_fused = ctx->ba_no_fused || env_no_fused;
  if (!no_fused) {  // local windows: the fused iteration (ba_fused.hip); everything else continues below
    int handled = 0;
    rc = vsl_ba_fused_solve(ctx, prob, opt, summary, &handled);
    if (rc || handled) return rc;
    // Large maps (more free cameras than the fused window takes: the reduced system goes through the pair-list gather
    // and the band solver): the session solver at world size 1 -- the recompute-form iteration of ba_large.h, the cyclic
    // band form, one host round trip per iteration -- the same LM policy on the same numbers
    // (tests/test_ba_dist_gpu.py::test_session_world1_matches_single_call_and_oracle).  ba_host_loop_solve remains for
    // mid-size windows the fused kernels decline (more than 64 cameras, a landmark seen more than 64 times), for
    // "ba_no_fused" and as the cross-check of both.
    int nfree = 0;
    for (int c = 0; c < prob->n_cams; c++) nfree += prob->cam_fixed[c] ? 0 : 1;
    if (6 * nfree > 128) return vsl_global_bundle_adjust(ctx, prob, opt, nullptr, nullptr, 0, 1, summary);
  }
  const double t_start = now_ms();
  BaState st;  // holds the loan of the context's arena
  if ((rc = ba_setup(ctx, prob, opt, st, BaCaller{BaUse::HOST_LOOP}))) return rc;
  rc = ba_host_loop_solve(ctx, prob, opt, st, no_fused, t_start, summary);
  // an error return may leave kernels and copies queued on the arena: drain the stream before the loan ends (the next
  // solve on this context gets the same block)
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// =================================================================================================
// bundle_adjustment with BundleAdjustmentOptions::optimize_intrinsics = true (include/visnav/map_utils.h:324, :397-403:
// the two 8-parameter intrinsics blocks are NOT set constant).  The reference never enables it (a hidden GUI variable,
// src/slam.cpp:304, :1545), so this path is written for correctness, not for the last microsecond: its own plain
// Levenberg-Marquardt loop (several host round trips per iteration) over the same restated Ceres policy, the reduced
// system [poses (6 per free camera) | intrinsics (2 x 8)] assembled densely with fp64 atomics -- the camera-camera part
// by the large-system kernel above, the intrinsics border by the kernels below -- and solved by the dense Cholesky.
// The unused trailing parameters of a model have zero Jacobian columns, exactly like Ceres' size-8 block: the LM
// diagonal floor (1e-6 / radius) keeps the system definite and they keep their values.
namespace {

// d(u, v) / d intrinsics at the camera-frame point (x, y, z): Gu[8], Gv[8] (camera_models.h project() of the four models)
__device__ __forceinline__ void project_intr_jac(int model, const double* __restrict__ ip, double x, double y, double z,
                                                 double* Gu, double* Gv) {
  const double fx = ip[0], fy = ip[1];
  for (int j = 0; j < 8; j++) Gu[j] = Gv[j] = 0.0;
  Gu[2] = 1.0;
  Gv[3] = 1.0;
  if (model == VSL_CAM_PINHOLE) {
    Gu[0] = x / z;
    Gv[1] = y / z;
  } else if (model == VSL_CAM_EUCM) {
    const double alpha = ip[4], beta = ip[5];
    const double rho2 = x * x + y * y;
    const double d = sqrt(beta * rho2 + z * z);
    const double den = alpha * d + (1.0 - alpha) * z;
    const double id = 1.0 / den, id2 = id * id;
    Gu[0] = x * id;
    Gv[1] = y * id;
    const double dden_da = d - z, dden_db = alpha * rho2 / (2.0 * d);
    Gu[4] = -fx * x * dden_da * id2; Gv[4] = -fy * y * dden_da * id2;
    Gu[5] = -fx * x * dden_db * id2; Gv[5] = -fy * y * dden_db * id2;
  } else if (model == VSL_CAM_KB4) {
    const double k1 = ip[4], k2 = ip[5], k3 = ip[6], k4 = ip[7];
    const double r = sqrt(x * x + y * y);
    if (r == 0.0) return;  // u = cx, v = cy
    const double th = atan2(r, z);
    const double t2 = th * th, t3 = t2 * th, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const double d = th + k1 * t3 + k2 * t5 + k3 * t7 + k4 * t9;
    const double xr = x / r, yr = y / r;
    Gu[0] = d * xr;
    Gv[1] = d * yr;
    Gu[4] = fx * xr * t3; Gv[4] = fy * yr * t3;
    Gu[5] = fx * xr * t5; Gv[5] = fy * yr * t5;
    Gu[6] = fx * xr * t7; Gv[6] = fy * yr * t7;
    Gu[7] = fx * xr * t9; Gv[7] = fy * yr * t9;
  } else {  // double sphere
    const double xi = ip[4], alpha = ip[5];
    const double d1 = sqrt(x * x + y * y + z * z);
    const double k = xi * d1 + z;
    const double d2 = sqrt(x * x + y * y + k * k);
    const double den = alpha * d2 + (1.0 - alpha) * k;
    const double id = 1.0 / den, id2 = id * id;
    Gu[0] = x * id;
    Gv[1] = y * id;
    const double dden_dxi = alpha * (k * d1 / d2) + (1.0 - alpha) * d1, dden_da = d2 - k;
    Gu[4] = -fx * x * dden_dxi * id2; Gv[4] = -fy * y * dden_dxi * id2;
    Gu[5] = -fx * x * dden_da * id2;  Gv[5] = -fy * y * dden_da * id2;
  }
}

// one thread per observation: robustified residual and the three Jacobian blocks F (2x6, pose tangent), G (2x8,
// intrinsics), E (2x3, landmark), Jacobi-scaled when `scale` (n camera columns followed by 16 intrinsics columns) is given
__global__ __launch_bounds__(256) void bai_linearize_kernel(BaDims D, const double* __restrict__ poses,
                                                            const double* __restrict__ points, const double* __restrict__ intr,
                                                            const int* __restrict__ cam_intr, const int* __restrict__ cam_free,
                                                            const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                                            const double* __restrict__ obs_uv, const double* __restrict__ scale,
                                                            const double* __restrict__ scale_l, double* __restrict__ r_out,
                                                            double* __restrict__ F_out, double* __restrict__ E_out,
                                                            double* __restrict__ G_out, double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double c = 0;
  if (i < D.O) {
    const int cam = obs_cam[i], lm = obs_lm[i], k = cam_intr[cam], model = k ? D.model1 : D.model0;
    const double* pose = poses + 7 * (size_t)cam;
    const double* pw = points + 3 * (size_t)lm;
    double r[2], F[12], E[6], Gu[8], Gv[8];
    residual_blocks(model, intr + 8 * k, pose, pw, obs_uv + 2 * (size_t)i, r, F, E, true);
    {
      double R[9];
      quat_R(pose, R);
      const double d[3] = {pw[0] - pose[4], pw[1] - pose[5], pw[2] - pose[6]};
      project_intr_jac(model, intr + 8 * k, R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2],
                       R[2] * d[0] + R[5] * d[1] + R[8] * d[2], Gu, Gv);
    }
    const double s = r[0] * r[0] + r[1] * r[1];
    double rho0 = s, rho1 = 1.0;
    if (D.use_huber) huber(s, D.huber, rho0, rho1);
    c = 0.5 * rho0;
    const double sr = sqrt(rho1);
    r_out[2 * (size_t)i] = r[0] * sr;
    r_out[2 * (size_t)i + 1] = r[1] * sr;
    const int fc = cam_free[cam];
    for (int j = 0; j < 6; j++) {
      const double sc = (scale && fc >= 0) ? scale[6 * fc + j] : 1.0;
      F_out[12 * (size_t)i + j] = F[j] * sr * sc;
      F_out[12 * (size_t)i + 6 + j] = F[6 + j] * sr * sc;
    }
    for (int j = 0; j < 8; j++) {  // residual = p_2d - projection
      const double sc = scale ? scale[D.n + 8 * k + j] : 1.0;
      G_out[16 * (size_t)i + j] = -Gu[j] * sr * sc;
      G_out[16 * (size_t)i + 8 + j] = -Gv[j] * sr * sc;
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

// squared column norms and gradient J^T r of all columns: cameras + intrinsics in n2 / grad (n + 16), landmarks in
// n2l / gradl (3 L).  Outputs pre-zeroed.  The 32 intrinsics sums go through LDS first.
__global__ __launch_bounds__(256) void bai_stats_kernel(BaDims D, const int* __restrict__ cam_free, const int* __restrict__ cam_intr,
                                                        const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                                        const double* __restrict__ r, const double* __restrict__ F,
                                                        const double* __restrict__ E, const double* __restrict__ G,
                                                        double* __restrict__ n2, double* __restrict__ grad,
                                                        double* __restrict__ n2l, double* __restrict__ gradl) {
  __shared__ double acc[32];
  if (threadIdx.x < 32) acc[threadIdx.x] = 0.0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.O) {
    const int cam = obs_cam[i], fc = cam_free[cam], k = cam_intr[cam], lm = obs_lm[i];
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    const double* g = G + 16 * (size_t)i;
    if (fc >= 0)
      for (int j = 0; j < 6; j++) {
        unsafeAtomicAdd(&n2[6 * fc + j], f[j] * f[j] + f[6 + j] * f[6 + j]);
        unsafeAtomicAdd(&grad[6 * fc + j], f[j] * r0 + f[6 + j] * r1);
      }
    for (int j = 0; j < 8; j++) {
      unsafeAtomicAdd(&acc[8 * k + j], g[j] * g[j] + g[8 + j] * g[8 + j]);
      unsafeAtomicAdd(&acc[16 + 8 * k + j], g[j] * r0 + g[8 + j] * r1);
    }
    for (int j = 0; j < 3; j++) {
      unsafeAtomicAdd(&n2l[3 * (size_t)lm + j], e[j] * e[j] + e[3 + j] * e[3 + j]);
      unsafeAtomicAdd(&gradl[3 * (size_t)lm + j], e[j] * r0 + e[3 + j] * r1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 16) unsafeAtomicAdd(&n2[D.n + threadIdx.x], acc[threadIdx.x]);
  else if (threadIdx.x < 32) unsafeAtomicAdd(&grad[D.n + threadIdx.x - 16], acc[threadIdx.x]);
}

__global__ void bai_make_scale_kernel(int nt, int L3, const double* __restrict__ n2, const double* __restrict__ n2l,
                                      double* __restrict__ scale, double* __restrict__ scale_l) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nt) scale[i] = 1.0 / (1.0 + sqrt(n2[i]));
  if (i < L3) scale_l[i] = 1.0 / (1.0 + sqrt(n2l[i]));
}

__global__ void bai_apply_scale_kernel(BaDims D, const int* __restrict__ cam_free, const int* __restrict__ cam_intr,
                                       const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                       const double* __restrict__ scale, const double* __restrict__ scale_l,
                                       double* __restrict__ F, double* __restrict__ E, double* __restrict__ G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.O) return;
  const int cam = obs_cam[i], fc = cam_free[cam], k = cam_intr[cam], lm = obs_lm[i];
  if (fc >= 0)
    for (int j = 0; j < 6; j++) {
      F[12 * (size_t)i + j] *= scale[6 * fc + j];
      F[12 * (size_t)i + 6 + j] *= scale[6 * fc + j];
    }
  for (int j = 0; j < 8; j++) {
    G[16 * (size_t)i + j] *= scale[D.n + 8 * k + j];
    G[16 * (size_t)i + 8 + j] *= scale[D.n + 8 * k + j];
  }
  for (int j = 0; j < 3; j++) {
    E[6 * (size_t)i + j] *= scale_l[3 * (size_t)lm + j];
    E[6 * (size_t)i + 3 + j] *= scale_l[3 * (size_t)lm + j];
  }
}

// LM diagonal clamp(||column||^2) of all columns and max |gradient| (one workgroup; scalars[slot] = the maximum)
__global__ __launch_bounds__(256) void bai_diag_gmax_kernel(int nt, int L3, const double* __restrict__ n2, const double* __restrict__ n2l,
                                                            const double* __restrict__ grad, const double* __restrict__ gradl,
                                                            int write_diag, double* __restrict__ diag, double* __restrict__ diag_l,
                                                            double* __restrict__ scalars, int slot) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int i = threadIdx.x; i < nt; i += 256) {
    if (write_diag) diag[i] = fmin(fmax(n2[i], 1e-6), 1e32);
    m = fmax(m, fabs(grad[i]));
  }
  for (int i = threadIdx.x; i < L3; i += 256) {
    if (write_diag) diag_l[i] = fmin(fmax(n2l[i], 1e-6), 1e32);
    m = fmax(m, fabs(gradl[i]));
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) scalars[slot] = sh[0];
}

// J^T J of the camera side before the Schur correction, and J^T r: pose-pose diagonal blocks, pose-intrinsics blocks
// (both triangles of the full matrix), intrinsics-intrinsics blocks (through LDS), into S (nt x nt) and rhs (nt)
__global__ __launch_bounds__(256) void bai_hess_kernel(BaDims D, int nt, const int* __restrict__ cam_free,
                                                       const int* __restrict__ cam_intr, const int* __restrict__ obs_cam,
                                                       const double* __restrict__ r, const double* __restrict__ F,
                                                       const double* __restrict__ G, double* __restrict__ S,
                                                       double* __restrict__ rhs) {
  __shared__ double hii[2][64];
  __shared__ double gi[16];
  if (threadIdx.x < 128) hii[threadIdx.x >> 6][threadIdx.x & 63] = 0.0;
  if (threadIdx.x < 16) gi[threadIdx.x] = 0.0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.O) {
    const int cam = obs_cam[i], fc = cam_free[cam], k = cam_intr[cam];
    const double r0 = r[2 * (size_t)i], r1 = r[2 * (size_t)i + 1];
    const double* f = F + 12 * (size_t)i;
    const double* g = G + 16 * (size_t)i;
    const int ci = D.n + 8 * k;
    if (fc >= 0) {
      for (int x = 0; x < 6; x++) {
        unsafeAtomicAdd(&rhs[6 * fc + x], f[x] * r0 + f[6 + x] * r1);
        for (int y = 0; y < 6; y++)
          unsafeAtomicAdd(&S[(size_t)(6 * fc + x) * nt + 6 * fc + y], f[x] * f[y] + f[6 + x] * f[6 + y]);
        for (int j = 0; j < 8; j++) {
          const double v = f[x] * g[j] + f[6 + x] * g[8 + j];
          if (v != 0.0) {
            unsafeAtomicAdd(&S[(size_t)(6 * fc + x) * nt + ci + j], v);
            unsafeAtomicAdd(&S[(size_t)(ci + j) * nt + 6 * fc + x], v);
          }
        }
      }
    }
    for (int a = 0; a < 8; a++) {
      unsafeAtomicAdd(&gi[8 * k + a], g[a] * r0 + g[8 + a] * r1);
      for (int b = 0; b < 8; b++) {
        const double v = g[a] * g[b] + g[8 + a] * g[8 + b];
        if (v != 0.0) unsafeAtomicAdd(&hii[k][8 * a + b], v);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int k = threadIdx.x >> 6, e = threadIdx.x & 63, a = e >> 3, b = e & 7;
    const double v = hii[k][e];
    if (v != 0.0) unsafeAtomicAdd(&S[(size_t)(D.n + 8 * k + a) * nt + D.n + 8 * k + b], v);
  } else if (threadIdx.x < 144) {
    unsafeAtomicAdd(&rhs[D.n + threadIdx.x - 128], gi[threadIdx.x - 128]);
  }
}

// Schur correction of the intrinsics border, one wavefront per landmark (P^-1 and b of the landmark come from the
// camera-camera kernel): W_i = sum_o G_o^T E_o (16 x 3), T = P^-1 W_i^T (3 x 16, kept for the back-substitution);
//   S_ii -= W_i T,  rhs_i -= T^T b,  S_ci(camera of o) -= (F_o^T E_o) T  (and its mirror)
__global__ __launch_bounds__(256) void bai_border_kernel(BaDims D, int nt, const int* __restrict__ lm_start,
                                                         const int* __restrict__ obs_cam, const int* __restrict__ cam_free,
                                                         const int* __restrict__ cam_intr, const double* __restrict__ F,
                                                         const double* __restrict__ E, const double* __restrict__ G,
                                                         const double* __restrict__ Pinv, const double* __restrict__ bl,
                                                         double* __restrict__ T_out, double* __restrict__ S,
                                                         double* __restrict__ rhs) {
  __shared__ double Wi[4][16][3];
  __shared__ double Ts[4][3][16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + wave;
  if (l >= D.L) return;
  const int a = lm_start[l], b = lm_start[l + 1];
  const double* Pi = Pinv + 9 * (size_t)l;
  if (lane < 48) {
    const int col = lane / 3, y = lane - 3 * col, k = col >> 3, j = col & 7;
    double s = 0.0;
    for (int i = a; i < b; i++) {
      if (cam_intr[obs_cam[i]] != k) continue;
      const double* g = G + 16 * (size_t)i;
      const double* e = E + 6 * (size_t)i;
      s += g[j] * e[y] + g[8 + j] * e[3 + y];
    }
    Wi[wave][col][y] = s;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  if (lane < 48) {
    const int y = lane >> 4, col = lane & 15;
    const double t = Pi[3 * y] * Wi[wave][col][0] + Pi[3 * y + 1] * Wi[wave][col][1] + Pi[3 * y + 2] * Wi[wave][col][2];
    Ts[wave][y][col] = t;
    T_out[48 * (size_t)l + 16 * y + col] = t;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < 256; e += 64) {
    const int c1 = e >> 4, c2 = e & 15;
    const double v = Wi[wave][c1][0] * Ts[wave][0][c2] + Wi[wave][c1][1] * Ts[wave][1][c2] + Wi[wave][c1][2] * Ts[wave][2][c2];
    if (v != 0.0) unsafeAtomicAdd(&S[(size_t)(D.n + c1) * nt + D.n + c2], -v);
  }
  if (lane < 16) {
    const double v = Ts[wave][0][lane] * bl[3 * (size_t)l] + Ts[wave][1][lane] * bl[3 * (size_t)l + 1] + Ts[wave][2][lane] * bl[3 * (size_t)l + 2];
    if (v != 0.0) unsafeAtomicAdd(&rhs[D.n + lane], -v);
  }
  for (int item = lane; item < (b - a) * 96; item += 64) {
    const int q = item / 96, rem = item - 96 * q, x = rem >> 4, c = rem & 15, i = a + q;
    const int fc = cam_free[obs_cam[i]];
    if (fc < 0) continue;
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    double v = 0.0;
    for (int z = 0; z < 3; z++) v += (f[x] * e[z] + f[6 + x] * e[3 + z]) * Ts[wave][z][c];
    if (v != 0.0) {
      unsafeAtomicAdd(&S[(size_t)(6 * fc + x) * nt + D.n + c], -v);
      unsafeAtomicAdd(&S[(size_t)(D.n + c) * nt + 6 * fc + x], -v);
    }
  }
}

__global__ void bai_damp_kernel(int nt, const double* __restrict__ diag, double inv_radius, double* __restrict__ S) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nt) S[(size_t)i * nt + i] += diag[i] * inv_radius;
}

// delta_l = -P^-1 (b_l + sum_o E_o^T (F_o dc + G_o di)); d = [dc (n) | di (16)]
__global__ __launch_bounds__(256) void bai_backsub_kernel(BaDims D, const int* __restrict__ lm_start, const int* __restrict__ obs_cam,
                                                          const int* __restrict__ cam_free, const int* __restrict__ cam_intr,
                                                          const double* __restrict__ F, const double* __restrict__ E,
                                                          const double* __restrict__ G, const double* __restrict__ Pinv,
                                                          const double* __restrict__ bl, const double* __restrict__ d,
                                                          double* __restrict__ dl) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= D.L) return;
  double t[3] = {bl[3 * (size_t)l], bl[3 * (size_t)l + 1], bl[3 * (size_t)l + 2]};
  for (int i = lm_start[l]; i < lm_start[l + 1]; i++) {
    const int cam = obs_cam[i], fc = cam_free[cam], k = cam_intr[cam];
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    const double* g = G + 16 * (size_t)i;
    double m0 = 0, m1 = 0;
    if (fc >= 0)
      for (int j = 0; j < 6; j++) {
        m0 += f[j] * d[6 * fc + j];
        m1 += f[6 + j] * d[6 * fc + j];
      }
    for (int j = 0; j < 8; j++) {
      m0 += g[j] * d[D.n + 8 * k + j];
      m1 += g[8 + j] * d[D.n + 8 * k + j];
    }
    for (int j = 0; j < 3; j++) t[j] += e[j] * m0 + e[3 + j] * m1;
  }
  const double* Pi = Pinv + 9 * (size_t)l;
  for (int j = 0; j < 3; j++) dl[3 * (size_t)l + j] = -(Pi[3 * j] * t[0] + Pi[3 * j + 1] * t[1] + Pi[3 * j + 2] * t[2]);
}

__global__ __launch_bounds__(256) void bai_model_kernel(BaDims D, const int* __restrict__ obs_cam, const int* __restrict__ obs_lm,
                                                        const int* __restrict__ cam_free, const int* __restrict__ cam_intr,
                                                        const double* __restrict__ r, const double* __restrict__ F,
                                                        const double* __restrict__ E, const double* __restrict__ G,
                                                        const double* __restrict__ d, const double* __restrict__ dl,
                                                        double* __restrict__ partials) {
  __shared__ double sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v = 0;
  if (i < D.O) {
    const int cam = obs_cam[i], fc = cam_free[cam], k = cam_intr[cam], lm = obs_lm[i];
    const double* f = F + 12 * (size_t)i;
    const double* e = E + 6 * (size_t)i;
    const double* g = G + 16 * (size_t)i;
    double m0 = 0, m1 = 0;
    if (fc >= 0)
      for (int j = 0; j < 6; j++) {
        m0 += f[j] * d[6 * fc + j];
        m1 += f[6 + j] * d[6 * fc + j];
      }
    for (int j = 0; j < 8; j++) {
      m0 += g[j] * d[D.n + 8 * k + j];
      m1 += g[8 + j] * d[D.n + 8 * k + j];
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

// candidate intrinsics = intrinsics + step .* scale; scalars[slot] = squared step norm, scalars[slot + 1] = squared norm
// of the current intrinsics (both blocks are non-constant parameter blocks)
__global__ void bai_intr_update_kernel(int n, const double* __restrict__ intr, const double* __restrict__ d,
                                       const double* __restrict__ scale, double* __restrict__ cand_intr,
                                       double* __restrict__ scalars, int slot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s2 = 0, x2 = 0;
  for (int j = 0; j < 16; j++) {
    const double dd = d[n + j] * scale[n + j];
    s2 += dd * dd;
    x2 += intr[j] * intr[j];
    cand_intr[j] = intr[j] + dd;
  }
  scalars[slot] = s2;
  scalars[slot + 1] = x2;
}

// ---- host side of the intrinsics solver: its buffers beside BaState, and the three routines that the LM loop
// (vsl_bundle_adjust_intrinsics) and the parity hook (vsl_ba_intrinsics_system) share, so that the hook cannot drift
// from the solve
struct BaiBuffers {
  double *G, *scale, *n2, *grad, *diag, *Sf, *rhsf, *df, *cand_intr, *Tl;
  DevArena arena;
};

int bai_acquire(vsl_ctx* ctx, const BaState& st, BaiBuffers& B) {
  const BaDims& D = st.D;
  const int nt = D.n + 16;
  ArenaPlan plan(10);
  plan.add(B.G, 16 * (size_t)D.O);
  plan.add(B.scale, (size_t)nt);
  plan.add(B.n2, (size_t)nt);
  plan.add(B.grad, (size_t)nt);
  plan.add(B.diag, (size_t)nt);
  plan.add(B.Sf, (size_t)nt * nt);
  plan.add(B.rhsf, (size_t)nt);
  plan.add(B.df, (size_t)nt);
  plan.add(B.cand_intr, 16);
  plan.add(B.Tl, 48 * (size_t)D.L);
  VSL_HIP(ctx, B.arena.acquire(ctx, ArenaPolicy::OWNED, plan));
  return VSL_OK;
}

// at the CURRENT point; scalars[0] = cost.  D is passed so that the hook can ask for the blocks without the robustifier.
int bai_linearize(vsl_ctx* ctx, BaState& st, BaiBuffers& B, const BaDims& D, bool scaled) {
  BaStored& sb = st.sb;
  hipLaunchKernelGGL(bai_linearize_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, D, st.poses, st.points, st.intr, st.cam_intr,
                     st.cam_free, st.obs_cam, st.obs_lm, st.obs_uv, scaled ? B.scale : (const double*)nullptr,
                     scaled ? st.scale_l : (const double*)nullptr, sb.r, sb.F, sb.E, B.G, sb.partials);
  return vsl_ba_reduce_launch(ctx, sb.partials, st.nb_obs, st.scalars, 0, false);
}

// column norms / gradient of the current blocks; scalars[1] = max |gradient|
int bai_stats(vsl_ctx* ctx, BaState& st, BaiBuffers& B, bool write_diag) {
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  const int nt = D.n + 16, L3 = 3 * D.L;
  hipStream_t q = ctx->stream;
  VSL_HIP(ctx, hipMemsetAsync(B.n2, 0, 8 * (size_t)nt, q));
  VSL_HIP(ctx, hipMemsetAsync(B.grad, 0, 8 * (size_t)nt, q));
  VSL_HIP(ctx, hipMemsetAsync(st.n2l, 0, 8 * (size_t)L3, q));
  VSL_HIP(ctx, hipMemsetAsync(sb.grad_l, 0, 8 * (size_t)L3, q));
  hipLaunchKernelGGL(bai_stats_kernel, dim3(st.nb_obs), dim3(256), 0, q, D, st.cam_free, st.cam_intr, st.obs_cam, st.obs_lm, sb.r, sb.F,
                     sb.E, B.G, B.n2, B.grad, st.n2l, sb.grad_l);
  hipLaunchKernelGGL(bai_diag_gmax_kernel, dim3(1), dim3(256), 0, q, nt, L3, B.n2, st.n2l, B.grad, sb.grad_l, write_diag ? 1 : 0,
                     B.diag, sb.diag_l, st.scalars, 1);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

// initial linearisation, Jacobi scaling from the unscaled column norms (once), statistics of the scaled blocks (they
// write the LM diagonal); scalars[0] = cost, scalars[1] = max |gradient|
int bai_first_linearization(vsl_ctx* ctx, BaState& st, BaiBuffers& B) {
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  const int nt = D.n + 16, L3 = 3 * D.L;
  int rc;
  if ((rc = bai_linearize(ctx, st, B, D, false))) return rc;
  if ((rc = bai_stats(ctx, st, B, false))) return rc;
  hipLaunchKernelGGL(bai_make_scale_kernel, dim3((std::max(nt, L3) + 255) / 256), dim3(256), 0, ctx->stream, nt, L3, B.n2, st.n2l,
                     B.scale, st.scale_l);
  hipLaunchKernelGGL(bai_apply_scale_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, D, st.cam_free, st.cam_intr, st.obs_cam,
                     st.obs_lm, B.scale, st.scale_l, sb.F, sb.E, B.G);
  return bai_stats(ctx, st, B, true);
}

// one system, built and solved: the reduced system [poses | intrinsics] of the stored blocks at 1 / radius = inv_radius
// (J^T J of the camera side, damping, the Schur corrections camera-camera and border), its factorisation (flag[1] = 0 when
// a pivot fails), B.df = -(Sf^-1 rhsf) and the back-substituted sb.dl.  host_S / host_rhs (nullable; the hook's) receive
// the system as it is handed to the factorisation, by copies queued BEFORE it (the large solver works in place).
int bai_build_and_solve(vsl_ctx* ctx, BaState& st, BaiBuffers& B, double inv_radius, double* host_S, double* host_rhs) {
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  const int nt = D.n + 16;
  hipStream_t q = ctx->stream;
  int rc;
  VSL_HIP(ctx, hipMemsetAsync(B.Sf, 0, 8 * (size_t)nt * nt, q));
  VSL_HIP(ctx, hipMemsetAsync(B.rhsf, 0, 8 * (size_t)nt, q));
  hipLaunchKernelGGL(bai_hess_kernel, dim3(st.nb_obs), dim3(256), 0, q, D, nt, st.cam_free, st.cam_intr, st.obs_cam, sb.r, sb.F, B.G,
                     B.Sf, B.rhsf);
  hipLaunchKernelGGL(bai_damp_kernel, dim3((nt + 255) / 256), dim3(256), 0, q, nt, B.diag, inv_radius, B.Sf);
  hipLaunchKernelGGL(ba_schur_atomic_kernel, dim3((D.L + 3) / 4), dim3(256), 0, q, D, st.lm_start, st.obs_cam, st.cam_free, sb.r,
                     sb.F, sb.E, sb.diag_l, inv_radius, 0, D.L, B.Sf, B.rhsf, st.Pinv, st.bl, 0, nt);
  hipLaunchKernelGGL(bai_border_kernel, dim3((D.L + 3) / 4), dim3(256), 0, q, D, nt, st.lm_start, st.obs_cam, st.cam_free,
                     st.cam_intr, sb.F, sb.E, B.G, st.Pinv, st.bl, B.Tl, B.Sf, B.rhsf);
  hipLaunchKernelGGL(ba_set_flags_kernel, dim3(1), dim3(64), 0, q, st.flag);
  if (host_S) VSL_HIP(ctx, hipMemcpyAsync(host_S, B.Sf, 8 * (size_t)nt * nt, hipMemcpyDeviceToHost, q));
  if (host_rhs) VSL_HIP(ctx, hipMemcpyAsync(host_rhs, B.rhsf, 8 * (size_t)nt, hipMemcpyDeviceToHost, q));
  if (nt <= 128) {
    hipLaunchKernelGGL(ba_chol_small_kernel, dim3(1), dim3(256), 0, q, nt, B.Sf, B.rhsf, B.df, st.flag + 1);
  } else {
    if ((rc = vsl_chol_solve_band_dev(ctx, B.Sf, B.rhsf, nt, nt, nt, st.flag + 1, 0, B.df))) return rc;  // df = -(Sf^-1 rhsf)
  }
  hipLaunchKernelGGL(bai_backsub_kernel, dim3((D.L + 255) / 256), dim3(256), 0, q, D, st.lm_start, st.obs_cam, st.cam_free,
                     st.cam_intr, sb.F, sb.E, B.G, st.Pinv, st.bl, B.df, sb.dl);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

}  // namespace

extern "C" int vsl_bundle_adjust_intrinsics(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, double* intr_io,
                                            vsl_ba_summary* summary) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!opt || !intr_io) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_bundle_adjust_intrinsics: null argument");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  const double t_start = now_ms();
  vsl_ba_problem p2 = *prob;
  p2.intr = intr_io;
  BaState st;
  if ((rc = ba_setup(ctx, &p2, opt, st, BaCaller{BaUse::SINGLE_LINEARIZE}))) return rc;
  BaStored& sb = st.sb;
  const BaDims& D = st.D;
  const int n = D.n, nt = n + 16, L3 = 3 * D.L;
  BaiBuffers B;
  if ((rc = bai_acquire(ctx, st, B))) return rc;
  double *const G = B.G, *const scale = B.scale, *const df = B.df, *const cand_intr = B.cand_intr;
  vsl_ba_summary sum;
  memset(&sum, 0, sizeof(sum));
  hipStream_t q = ctx->stream;
  const int nbo = st.nb_obs;
  double* scal = st.scalars;

  double h[16];
  if ((rc = bai_first_linearization(ctx, st, B))) return rc;
  if ((rc = read_scalars(ctx, st, h, 2))) return rc;
  double cost = h[0], gmax = h[1];
  sum.initial_cost = cost;
  LmState lm;  // (the first linearisation wrote the LM diagonal of the current Jacobian)
  int iteration = 0, term;
  sum.termination = 0;
  if (opt->verbosity >= 2) lm_print_header(cost);
  while (true) {
    if (iteration >= opt->max_num_iterations) { sum.termination = 0; break; }
    if ((term = lm_gate(lm, gmax)) >= 0) { sum.termination = term; break; }
    iteration++;
    const double inv_radius = 1.0 / lm.radius;
    if ((rc = bai_build_and_solve(ctx, st, B, inv_radius, nullptr, nullptr))) return rc;
    hipLaunchKernelGGL(ba_all_finite2_kernel, dim3((std::max(nt, L3) + 255) / 256), dim3(256), 0, q, nt, df, L3, sb.dl, st.flag);
    hipLaunchKernelGGL(bai_model_kernel, dim3(nbo), dim3(256), 0, q, D, st.obs_cam, st.obs_lm, st.cam_free, st.cam_intr, sb.r, sb.F,
                       sb.E, G, df, sb.dl, sb.partials);
    if ((rc = vsl_ba_reduce_launch(ctx, sb.partials, nbo, scal, 2, false))) return rc;
    // candidate point and its cost
    if ((rc = vsl_ba_update_launch(ctx, D.C, D.L, st.cam_free, st.poses, st.points, df, sb.dl, scale, st.scale_l, st.cand_poses,
                                   st.cand_points, sb.partials, scal, 3)))
      return rc;
    hipLaunchKernelGGL(bai_intr_update_kernel, dim3(1), dim3(64), 0, q, n, st.intr, df, scale, cand_intr, scal, 6);
    hipLaunchKernelGGL(ba_cost_kernel, dim3(nbo), dim3(256), 0, q, D, st.cand_poses, st.cand_points, cand_intr, st.cam_intr,
                       st.obs_cam, st.obs_lm, st.obs_uv, 0, D.O, sb.partials);
    if ((rc = vsl_ba_reduce_launch(ctx, sb.partials, nbo, scal, 5, false))) return rc;
    int hflag[2];
    VSL_HIP(ctx, hipMemcpyAsync(h, scal, sizeof(double) * 8, hipMemcpyDeviceToHost, q));
    VSL_HIP(ctx, hipMemcpyAsync(hflag, st.flag, sizeof(int) * 2, hipMemcpyDeviceToHost, q));
    VSL_HIP(ctx, hipStreamSynchronize(q));
    const double model_change = h[2], step_norm = sqrt(h[3] + h[6]), x_norm = sqrt(h[4] + h[7]), cand_cost = h[5];
    const bool ok = hflag[0] != 0 && hflag[1] != 0 && model_change > 0.0;
    const double radius_used = lm.radius;
    LmInfo info;
    const int verdict = lm_judge(lm, ok, cost, cand_cost, model_change, step_norm, x_norm, &info);
    if (verdict >= 0) { sum.termination = verdict; break; }
    if (verdict == LM_INVALID) {
      if (opt->verbosity >= 2) lm_print_invalid(iteration, lm.radius);
      continue;  // the LM diagonal is reused (the Jacobian is unchanged)
    }
    if (opt->verbosity >= 2) lm_print_row(iteration, cand_cost, info.cost_change, gmax, step_norm, info.rel, radius_used);
    if (verdict == LM_ACCEPTED) {
      std::swap(st.poses, st.cand_poses);
      std::swap(st.points, st.cand_points);
      VSL_HIP(ctx, hipMemcpyAsync(st.intr, cand_intr, 8 * 16, hipMemcpyDeviceToDevice, q));
      cost = cand_cost;
      if ((rc = bai_linearize(ctx, st, B, D, true))) return rc;
      if ((rc = bai_stats(ctx, st, B, true))) return rc;   // new LM diagonal
      if ((rc = read_scalars(ctx, st, h, 2))) return rc;
      gmax = h[1];
      sum.successful_steps++;
    }
  }
  sum.iterations = iteration;
  sum.final_cost = cost;
  VSL_HIP(ctx, hipMemcpyAsync(prob->poses, st.poses, sizeof(double) * 7 * (size_t)D.C, hipMemcpyDeviceToHost, q));
  VSL_HIP(ctx, hipMemcpyAsync(prob->points, st.points, sizeof(double) * 3 * (size_t)D.L, hipMemcpyDeviceToHost, q));
  VSL_HIP(ctx, hipMemcpyAsync(intr_io, st.intr, sizeof(double) * 16, hipMemcpyDeviceToHost, q));
  VSL_HIP(ctx, hipStreamSynchronize(q));
  sum.total_ms = now_ms() - t_start;
  if (opt->verbosity >= 1)
    fprintf(stderr, "vsl BA (intrinsics): iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n", sum.iterations,
            sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
  if (summary) *summary = sum;
  return VSL_OK;
}

extern "C" int vsl_ba_intrinsics_system(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, const double* intr16,
                                        double inv_radius, double* G, double* scale, double* S, double* rhs, double* cost,
                                        double* d, double* dl, int* chol_ok) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!opt || !intr16) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_intrinsics_system: null argument");
  if (!(inv_radius >= 0.0) || !std::isfinite(inv_radius))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_intrinsics_system: 1 / radius = %g is not a finite non-negative number", inv_radius);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  vsl_ba_problem p2 = *prob;
  p2.intr = intr16;
  BaState st;
  if ((rc = ba_setup(ctx, &p2, opt, st, BaCaller{BaUse::SINGLE_LINEARIZE}))) return rc;
  const BaDims& D = st.D;
  const size_t nt = (size_t)D.n + 16, O = (size_t)D.O, L3 = 3 * (size_t)D.L;
  BaiBuffers B;
  if ((rc = bai_acquire(ctx, st, B))) return rc;
  hipStream_t q = ctx->stream;
  std::vector<double> hG(G ? 16 * O : 0), hS(nt * nt), hv(3 * nt), hdl(L3);  // (targets of queued copies: they outlive the drain)
  double c = 0;
  int flags[2] = {0, 0};
  auto run = [&]() -> int {
    int e;
    if (G) {  // the blocks as vsl_ba_residuals_jacobians reports F and E: without the robustifier, unscaled
      BaDims raw = D;
      raw.use_huber = 0;
      if ((e = bai_linearize(ctx, st, B, raw, false))) return e;
      VSL_HIP(ctx, hipMemcpyAsync(hG.data(), B.G, 8 * 16 * O, hipMemcpyDeviceToHost, q));
    }
    if ((e = bai_first_linearization(ctx, st, B))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(&c, st.scalars, 8, hipMemcpyDeviceToHost, q));
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + nt, B.scale, 8 * nt, hipMemcpyDeviceToHost, q));
    if ((e = bai_build_and_solve(ctx, st, B, inv_radius, hS.data(), hv.data()))) return e;
    VSL_HIP(ctx, hipMemcpyAsync(hv.data() + 2 * nt, B.df, 8 * nt, hipMemcpyDeviceToHost, q));
    VSL_HIP(ctx, hipMemcpyAsync(hdl.data(), st.sb.dl, 8 * L3, hipMemcpyDeviceToHost, q));
    VSL_HIP(ctx, hipMemcpyAsync(flags, st.flag, 8, hipMemcpyDeviceToHost, q));
    VSL_HIP(ctx, hipStreamSynchronize(q));
    return VSL_OK;
  };
  if ((rc = run())) {
    (void)hipStreamSynchronize(q);  // kernels and copies may still be queued on the buffers that die here
    return rc;
  }
  if (G) memcpy(G, hG.data(), 8 * 16 * O);
  if (scale) memcpy(scale, hv.data() + nt, 8 * nt);
  if (S) memcpy(S, hS.data(), 8 * nt * nt);
  if (rhs) memcpy(rhs, hv.data(), 8 * nt);
  if (cost) *cost = c;
  if (d) memcpy(d, hv.data() + 2 * nt, 8 * nt);
  if (dl) memcpy(dl, hdl.data(), 8 * L3);
  if (chol_ok) *chol_ok = flags[1] != 0;
  if (!flags[1] && !chol_ok)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_intrinsics_system: the reduced system is not positive definite");
  return VSL_OK;
}
