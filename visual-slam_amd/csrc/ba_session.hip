// ba_session.hip -- the session solver of the global bundle adjustment: vsl_global_bundle_adjust, the one entry point
// of the multi-GPU path and of the single-GPU solve of a large map.
//
// One process per GPU.  Every rank holds all camera poses and OWNS a contiguous landmark range with its observations
// (the session is built on that sub-problem).  Per LM iteration the ranks exchange
//   packB = [ S_part (s_elems) | rhs_part (n) | diag(H_part) (n) | g_c part (n) | cost_part | 0 ]  SUM all-reduce
//   packC = [ bad, model_part, step2, x2, cand_cost_part, step2_cams, x2_cams, 0 ]                 SUM all-reduce
// (plus one MAX all-reduce of the landmark gradient norm after an accepted step, and one SUM of
// [diag(H_part) | cost_part] for the Jacobi scaling at iteration 0).  Every rank then factorises the same reduced
// camera system redundantly -- an all-reduce leaves bit-identical buffers on all ranks, so the accept / reject decisions
// agree without a broadcast.  Landmark damping and back-substitution are local.
//
// S inside packB: s_elems doubles -- n * n when dense; in band form (cameras renumbered into a narrow band by reverse
// Cuthill-McKee on the covisibility graph of the FULL problem, identically on every rank) or in CYCLIC band form
// (cameras as they came, the band closes around the loop -- the wrap blocks sit in the leading slots of the first rows)
// n * (bandwidth + 33) + 64 (BaCommon in ba_state.h, chol.hip "BAND FORM"): ~6 MB in the cyclic band form, ~12 MB in
// the linear one, instead of 287 MB at 1000 cameras.  Without a collective (world 1, no callback) S stays where it is:
// only the tail of packB is used.
//
// Collectives go through ONE caller-supplied function -- ncclAllReduce on the context's stream for RCCL
// (include/visnav_amd/bundle_adjustment.h), a host hop for the gloo tests (visual-slam_amd/ba_dist.py) -- so the loop
// does not depend on a communication library.  Policy = the [upstream] Ceres policy of vsl_bundle_adjust (lm_policy.h).
//
// Two forms of the iteration, chosen once by ba_setup (ba_host_plan.h ba_recompute_form), each written out below in one
// place: RecomputeForm (ba_large.h: nothing is stored per observation, one host round trip per iteration) and
// StoredForm (the operator-by-operator chain over r / F / E blocks through the launchers of ba.hip: small systems,
// "ba_no_fused", a landmark seen more often than a workgroup has threads).
#include <algorithm>
#include <cmath>
#include <new>

#include "vsl_common.h"
#include "lm_policy.h"
#include "dev_arena.h"
#include "ba_host_plan.h"
#include "ba_device.h"
#include "ba_state.h"
#include "ba_large.h"
#include "ba_pcg.h"

namespace {
// ---------------------------------------------------------------------------------------- kernels
__global__ void sess_pack_hdiag_kernel(int nfree, const double* __restrict__ H, const double* __restrict__ scalars,
                                       double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = 6 * nfree;
  if (i < n) out[i] = H[36 * (size_t)(i / 6) + 7 * (i % 6)];
  if (i == 0) out[n] = scalars[0];
}

__global__ void sess_scale_kernel(int nfree, int L, const double* __restrict__ hdiag_full, const double* __restrict__ n2l,
                                  double* __restrict__ scale_c, double* __restrict__ scale_l) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * nfree) scale_c[i] = 1.0 / (1.0 + sqrt(hdiag_full[i]));
  if (i < 3 * L) scale_l[i] = 1.0 / (1.0 + sqrt(n2l[i]));
}

// landmark LM diagonal (own landmarks) and |gradient| of the unscaled problem for the landmark columns
__global__ void sess_diag_l_kernel(int L, const double* __restrict__ n2l, const double* __restrict__ grad_l,
                                   const double* __restrict__ scale_l, double* __restrict__ diag_l, double* __restrict__ gabs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * L) {
    diag_l[i] = fmin(fmax(n2l[i], 1e-6), 1e32);
    gabs[i] = fabs(grad_l[i] / scale_l[i]);
  }
}

// packB tail after the n*n block: [rhs_part | diag(H_part) | g_c part (raw sum F^T r) | cost_part | 0]
__global__ void sess_pack_b_kernel(int nfree, const double* __restrict__ rhs, const double* __restrict__ H,
                                   const double* __restrict__ g_c, const double* __restrict__ scalars,
                                   double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = 6 * nfree;
  if (i < n) {
    out[i] = rhs[i];
    out[n + i] = H[36 * (size_t)(i / 6) + 7 * (i % 6)];
    out[2 * n + i] = g_c[i];
  }
  if (i == 0) {
    out[3 * n] = scalars[0];
    out[3 * n + 1] = 0.0;
  }
}

// ba_add_cam_blocks_kernel (no camera damping) and sess_pack_b_kernel in one launch: S += blockdiag(H), rhs += g_c, and
// the tail of packB from the sums
__global__ void sess_add_pack_kernel(int nfree, const double* __restrict__ H, const double* __restrict__ g_c,
                                     const double* __restrict__ scalars, double* __restrict__ S, double* __restrict__ rhs, int ldS,
                                     int lower_elems, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = 6 * nfree;
  if (t < nfree * 36) {
    const int fc = t / 36, x = (t % 36) / 6, y = t % 6;
    if (S && !(lower_elems && y > x)) S[(size_t)(6 * fc + x) * ldS + 6 * fc + y] += H[t];  // (S null: matrix-free, ba_pcg.h)
  }
  if (t < n) {
    const double r = rhs[t] + g_c[t];
    rhs[t] = r;
    out[t] = r;
    out[n + t] = H[36 * (size_t)(t / 6) + 7 * (t % 6)];
    out[2 * n + t] = g_c[t];
  }
  if (t == 0) {
    out[3 * n] = scalars[0];
    out[3 * n + 1] = 0.0;
  }
}

// S = S_full + diag(diag_c / radius); diag_c = clamp(diag H_full) when refresh, else kept.  S_full (the first
// `elems` doubles of packB, dense or band layout) has been copied into S already; this adds the damping to the
// diagonal (entry (i, i) at S_eff[i * ldS + i]) and unpacks rhs.
__global__ void sess_damp_kernel(int n, size_t elems, const double* __restrict__ packB, double inv_radius, int refresh,
                                 double* __restrict__ diag_keep, double* __restrict__ S_eff, int ldS, double* __restrict__ rhs,
                                 int* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (flags && i < 2) flags[i] = 1;  // (step finite / factorisation succeeded: what ba_set_flags_kernel would set)
  if (i < n) {
    double d = diag_keep[i];
    if (refresh) {
      d = fmin(fmax(packB[elems + n + i], 1e-6), 1e32);
      diag_keep[i] = d;
    }
    if (S_eff) S_eff[(size_t)i * ldS + i] += d * inv_radius;  // (null: matrix-free, the PCG adds the damping in its product)
    rhs[i] = packB[elems + i];
  }
}

__global__ void sess_pack_c_kernel(const double* __restrict__ scalars, const int* __restrict__ flag, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    // number of ranks whose step is unusable (flag[0] = step finite, flag[1] = factorisation succeeded)
    out[0] = (flag[0] && flag[1]) ? 0.0 : 1.0;
    out[1] = scalars[2];           // model cost change, own observations
    out[2] = scalars[3];           // squared step norm (own landmarks + cameras, see ba_dist.py)
    out[3] = scalars[4];           // squared x norm   (own landmarks + cameras)
    out[4] = scalars[5];           // candidate cost, own observations
    out[5] = scalars[6];           // squared step norm of the cameras alone (replicated on every rank)
    out[6] = scalars[7];           // squared x norm of the cameras alone
    out[7] = 0.0;
  }
}

__global__ __launch_bounds__(1024) void sess_gmax_c_kernel(int n, const double* __restrict__ g_c, const double* __restrict__ scale_c,
                                                           const double* __restrict__ cost_in, const double* __restrict__ gl,
                                                           double* __restrict__ out) {
  // out[0] = cost (copied), out[1] = max(max_i |g_c[i] / scale_c[i]|, gl[0])
  __shared__ double sh[1024];
  double m = 0;
  for (int i = threadIdx.x; i < n; i += 1024) m = fmax(m, fabs(g_c[i] / scale_c[i]));
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = cost_in[0];
    out[1] = fmax(sh[0], gl[0]);
  }
}

// ------------------------------------------------------------------------------- the two forms
// Both have: init (unscaled evaluation; bufA = [diag(H_part) | cost_part]), scale (Jacobi scaling from the all-reduced
// bufA), reduce (this rank's packB at the current point; gl[0] = max |gradient| over the owned landmark columns of the
// unscaled problem), step (from the all-reduced packB: damp the cameras, solve, back-substitute the owned landmarks,
// build the candidate, packC; refresh = 1 after an accepted step or at the first iteration, 0 when the Jacobian is
// unchanged and LM reuses its diagonal) and accept (the candidate becomes the current point).
// in_place: the solve has no collective, S stays where it is (no copy into packB and back).

struct RecomputeForm {
  vsl_ctx* ctx;
  BaCommon& st;
  BaRecompute& rc;
  const bool in_place;

  BlArgs args() const {
    BlArgs a;
    a.D = st.D;
    a.poses = st.poses;
    a.points = st.points;
    a.intr = st.intr;
    a.cam_intr = st.cam_intr;
    a.cam_free = st.cam_free;
    a.obs_cam = st.obs_cam;
    a.obs_lm = st.obs_lm;
    a.obs_uv = st.obs_uv;
    a.lm_start = st.lm_start;
    a.wg_lm = rc.wg_lm;
    a.scale_c = st.scale_c;
    a.scale_l = st.scale_l;
    return a;
  }

  // ---- the matrix-free route (ba_pcg.h): the operator on this linearisation's H and Z blocks, and one solve
  BpcgOp pcg_op(const double* diag, double inv_radius) const {
    BpcgOp a;
    a.nfree = st.D.nfree;
    a.nseg = rc.bl_seg;
    a.free_cams = st.free_cams;
    a.cam_free = st.cam_free;
    a.cam_start = st.cam_start;
    a.cam_lm = rc.cam_lm;
    a.obs_cam = st.obs_cam;
    a.cam_pos = st.cam_pos;
    a.lm_start = st.lm_start;
    a.wg_lm = rc.wg_lm;
    a.Z = st.Yg;
    a.H = st.H;
    a.diag = diag;
    a.inv_radius = inv_radius;
    return a;
  }

  // y = S v for device vectors (v: n doubles; t and the segment partials are scratch); enqueued
  int pcg_product(const BpcgOp& a, const BpcgRec* rec, const double* v) {
    hipLaunchKernelGGL(bpcg_lm_kernel, dim3(rc.n_wg), dim3(BL_THREADS), 0, ctx->stream, a, rec, v, rc.pcg_t);
    hipLaunchKernelGGL(bpcg_cam_kernel, dim3(a.nfree, a.nseg), dim3(256), 0, ctx->stream, a, rec, (const double*)rc.pcg_t, rc.pcg_part);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // solves S x = b (device, n doubles) into rc.pcg_x: preconditioner, then batches of `poll` enqueued iterations with
  // one read of the record after each; *h = the record at the end.  Counts the solve in the context's read-out.
  int pcg_solve(const BpcgOp& a, const double* b, double tol, int max_it, BpcgRec* h) {
    VslStage s(ctx, VSL_STAGE_BA_SOLVE);
    const int poll = ba_pcg_poll_of(ctx->ba_pcg_poll);
    VSL_HIP(ctx, hipMemsetAsync(rc.pcg_rec, 0, sizeof(BpcgRec), ctx->stream));
    hipLaunchKernelGGL(bpcg_precond_kernel, dim3(a.nfree), dim3(256), 0, ctx->stream, a, rc.pcg_minv, rc.pcg_rec);
    hipLaunchKernelGGL(bpcg_init_kernel, dim3(1), dim3(BPCG_T), 0, ctx->stream, a.nfree, b, (const double*)rc.pcg_minv, tol, max_it,
                       rc.pcg_x, rc.pcg_r, rc.pcg_z, rc.pcg_p, rc.pcg_rec);
    VSL_CHECK_LAUNCH(ctx);
    const long long max_batches = ba_pcg_max_batches(max_it, poll);
    for (long long batch = 0;; batch++) {
      VSL_HIP(ctx, hipMemcpyAsync(h, rc.pcg_rec, sizeof(BpcgRec), hipMemcpyDeviceToHost, ctx->stream));
      VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (h->done || batch >= max_batches) break;
      for (int k = 0; k < poll; k++) {
        int e = pcg_product(a, rc.pcg_rec, rc.pcg_p);
        if (e) return e;
        hipLaunchKernelGGL(bpcg_step_kernel, dim3(1), dim3(BPCG_T), 0, ctx->stream, a, (const double*)rc.pcg_part,
                           (const double*)rc.pcg_minv, rc.pcg_x, rc.pcg_r, rc.pcg_z, rc.pcg_p, rc.pcg_q, rc.pcg_rec);
        VSL_CHECK_LAUNCH(ctx);
      }
    }
    if (!h->done) return vsl_fail(ctx, VSL_ERR_HIP, "iterative Schur: the solve's record never reported an end");
    ctx->last_pcg_solves++;
    ctx->last_pcg_iterations += h->iterations;
    ctx->last_pcg_iterations_last = h->iterations;
    ctx->last_pcg_rel_residual = ba_pcg_rel_residual(*h);
    return VSL_OK;
  }

  // once per session: camera-major copies of (landmark, pixel) for bal_cam_kernel
  int prepare() {
    hipLaunchKernelGGL(bal_cam_major_kernel, dim3(st.nb_obs), dim3(256), 0, ctx->stream, st.D.O, st.cam_obs, st.obs_lm, st.obs_uv,
                       rc.cam_lm, rc.cam_uv);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // the Jacobi-scaling pass: unscaled column norms (st.n2l, diag of st.H) and the cost
  int init(double* bufA) {
    const BaDims& D = st.D;
    {
      VslStage s(ctx, VSL_STAGE_BA_LIN);
      const BlArgs a = args();
      hipLaunchKernelGGL(bal_prep_kernel<true>, dim3(rc.n_wg), dim3(BL_THREADS), 0, ctx->stream, a, (const int*)nullptr, 0.0,
                         (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, st.n2l, rc.lpart);
      hipLaunchKernelGGL(bal_cam_kernel<true>, dim3(D.nfree, rc.bl_seg), dim3(256), 0, ctx->stream, a, st.free_cams, st.cam_start,
                         rc.cam_lm, rc.cam_uv, (const double*)nullptr, st.cam_part);
      hipLaunchKernelGGL(bal_cam_finish_kernel, dim3((D.nfree * 33 + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, rc.bl_seg, 0,
                         st.cam_part, st.H, st.g_c, st.rhs, rc.n_wg, rc.lpart, st.scalars, (double*)nullptr);
      VSL_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(sess_pack_hdiag_kernel, dim3((D.n + 256) / 256), dim3(256), 0, ctx->stream, D.nfree, st.H, st.scalars, bufA);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // (nothing is stored per observation: there is nothing to rescale)
  int scale(const double* hdiag_full) {
    const BaDims& D = st.D;
    hipLaunchKernelGGL(sess_scale_kernel, dim3((std::max(D.n, 3 * D.L) + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, D.L,
                       hdiag_full, st.n2l, st.scale_c, st.scale_l);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // S (landmark damping only, no camera damping), rhs, H, g_c, P^-1, b at the current point; scalars[0] = cost
  int reduce(double radius, double* packB, double* gl) {
    const BaDims& D = st.D;
    {
      VslStage s(ctx, VSL_STAGE_BA_SCHUR);
      const BlArgs a = args();
      int e;
      if (!st.matrix_free) {
        VSL_HIP(ctx, hipMemsetAsync(st.S, 0, sizeof(double) * st.s_elems, ctx->stream));
        if ((e = ba_pair_lists(ctx, st, 0, D.L))) return e;
      }
      hipLaunchKernelGGL(bal_prep_kernel<false>, dim3(rc.n_wg), dim3(BL_THREADS), 0, ctx->stream, a, st.cam_pos, 1.0 / radius, st.Yg,
                         st.Pinv, st.bl, rc.pbs, (double*)nullptr, rc.lpart);
      hipLaunchKernelGGL(bal_cam_kernel<false>, dim3(D.nfree, rc.bl_seg), dim3(256), 0, ctx->stream, a, st.free_cams, st.cam_start,
                         rc.cam_lm, rc.cam_uv, rc.pbs, st.cam_part);
      hipLaunchKernelGGL(bal_cam_finish_kernel, dim3((D.nfree * 33 + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, rc.bl_seg, 1,
                         st.cam_part, st.H, st.g_c, st.rhs, rc.n_wg, rc.lpart, st.scalars, gl);
      VSL_CHECK_LAUNCH(ctx);
      // Y_i W_j^T = Z_i Z_j^T; n <= 128 is solved by ba_chol_small_kernel (full matrix)
      if (!st.matrix_free && (e = ba_schur_gather(ctx, st, st.Yg, st.Yg, st.banded ? 2 : (D.n > 128 ? 1 : 0)))) return e;
    }
    // the camera blocks are added together with the packing
    hipLaunchKernelGGL(sess_add_pack_kernel, dim3((D.nfree * 36 + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, st.H, st.g_c,
                       st.scalars, st.matrix_free ? (double*)nullptr : st.S_eff(), st.rhs, st.ldS, st.banded ? 1 : 0,
                       packB + st.s_elems);
    VSL_CHECK_LAUNCH(ctx);
    if (!in_place && !st.matrix_free) VSL_HIP(ctx, hipMemcpyAsync(packB, st.S, sizeof(double) * st.s_elems, hipMemcpyDeviceToDevice, ctx->stream));
    return VSL_OK;
  }

  // everything is enqueued, nothing is read back here: a failed factorisation leaves flag[1] = 0 and numbers nobody
  // uses (the loop's one read of packC per iteration sees the step as unusable)
  // the camera damping of a step: S += diag(diag_c / radius) (a stored S only), rhs unpacked from the all-reduced packB
  int damp(const double* packB, double radius, int refresh) {
    const BaDims& D = st.D;
    if (!in_place && !st.matrix_free)
      VSL_HIP(ctx, hipMemcpyAsync(st.S, packB, sizeof(double) * st.s_elems, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(sess_damp_kernel, dim3((D.n + 255) / 256), dim3(256), 0, ctx->stream, D.n, st.s_elems, packB, 1.0 / radius,
                       refresh, st.diagc_keep, st.matrix_free ? (double*)nullptr : st.S_eff(), st.ldS, st.rhs, st.flag);  // (sets both flags)
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // the operator of the damped, Jacobi-scaled system a step solves (after damp()), and the PCG on it
  BpcgOp pcg_damped_op(double radius) const { return pcg_op(st.diagc_keep, 1.0 / radius); }
  int pcg_damped(double radius, const double* b, double tol, int max_it, BpcgRec* h) {
    return pcg_solve(pcg_damped_op(radius), b, tol, max_it, h);
  }

  int step(const double* packB, double radius, int refresh, double* packC) {
    const BaDims& D = st.D;
    int e;
    if ((e = damp(packB, radius, refresh))) return e;
    if (st.matrix_free) {
      // dc = -(S^-1 rhs) by the PCG on the same damped, Jacobi-scaled system (same H, Z, rhs, diagonal); a failed pivot or
      // a breakdown clears flag[1] like a failed factorisation.  The host reads the solve's record once per batch.
      BpcgRec h;
      if ((e = pcg_damped(radius, st.rhs, ba_pcg_tol_of_exp(ctx->ba_pcg_tol_exp), ba_pcg_cap(D.n), &h))) return e;
      hipLaunchKernelGGL(bpcg_finish_kernel, dim3((D.n + 255) / 256), dim3(256), 0, ctx->stream, D.n, rc.pcg_x, rc.pcg_rec, -1.0, st.dc,
                         st.flag + 1);
      VSL_CHECK_LAUNCH(ctx);
    } else if ((e = ba_solve_enqueue(ctx, st, true))) {
      return e;
    }
    // candidate (cand_poses, cand_points) from dc, scalars[2..7] as the stored-blocks chain leaves them, packC
    VslStage s(ctx, VSL_STAGE_BA_STEP);
    const BlArgs a = args();
    hipLaunchKernelGGL(bal_pose_kernel, dim3(1), dim3(1024), 0, ctx->stream, D, st.cam_free, st.poses, st.dc, st.scale_c,
                       st.cand_poses, st.scalars, st.flag);
    hipLaunchKernelGGL(bal_step_kernel, dim3(rc.n_wg), dim3(BL_THREADS), 0, ctx->stream, a, st.Pinv, st.bl, st.dc, st.cand_poses,
                       st.cand_points, rc.lpart, st.flag);
    hipLaunchKernelGGL(bal_step_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, rc.n_wg, rc.lpart, st.scalars, st.flag, packC);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // (the next reduce evaluates the observations at the new point itself)
  int accept() {
    std::swap(st.poses, st.cand_poses);
    std::swap(st.points, st.cand_points);
    return VSL_OK;
  }
};

struct StoredForm {
  vsl_ctx* ctx;
  BaCommon& st;
  BaStored& sb;
  const bool in_place;

  int prepare() { return VSL_OK; }

  int init(double* bufA) {
    const BaDims& D = st.D;
    int e;
    if ((e = ba_linearize(ctx, st, sb, false))) return e;
    if ((e = ba_columns(ctx, st, sb))) return e;
    hipLaunchKernelGGL(sess_pack_hdiag_kernel, dim3((D.n + 256) / 256), dim3(256), 0, ctx->stream, D.nfree, st.H, st.scalars, bufA);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // scales the stored Jacobian blocks and refreshes the column statistics
  int scale(const double* hdiag_full) {
    const BaDims& D = st.D;
    hipLaunchKernelGGL(sess_scale_kernel, dim3((std::max(D.n, 3 * D.L) + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, D.L,
                       hdiag_full, st.n2l, st.scale_c, st.scale_l);
    VSL_CHECK_LAUNCH(ctx);
    int e = ba_apply_scale(ctx, st, sb);
    if (e) return e;
    return ba_columns(ctx, st, sb);
  }

  // Schur complement of the owned landmarks with THEIR damping (diag_l / radius) plus this rank's camera blocks, no
  // camera damping: ba_schur with damping and a zero camera diagonal
  int reduce(double radius, double* packB, double* gl) {
    const BaDims& D = st.D;
    const int n = D.n;
    int e;
    hipLaunchKernelGGL(sess_diag_l_kernel, dim3((3 * D.L + 255) / 256), dim3(256), 0, ctx->stream, D.L, st.n2l, sb.grad_l,
                       st.scale_l, sb.diag_l, sb.gabs);
    VSL_CHECK_LAUNCH(ctx);
    if ((e = ba_max_of(ctx, sb.gabs, 3 * D.L, gl))) return e;
    VSL_HIP(ctx, hipMemsetAsync(sb.diag_c, 0, sizeof(double) * (size_t)(n > 0 ? n : 1), ctx->stream));
    if ((e = ba_schur(ctx, st, sb, true, radius, 0, D.L, true, true))) return e;
    if (n > 0 && !in_place) VSL_HIP(ctx, hipMemcpyAsync(packB, st.S, sizeof(double) * st.s_elems, hipMemcpyDeviceToDevice, ctx->stream));
    // (also without a free camera: the cost behind the tail is what the loop reads)
    hipLaunchKernelGGL(sess_pack_b_kernel, dim3((n + 256) / 256), dim3(256), 0, ctx->stream, D.nfree, st.rhs, st.H, st.g_c,
                       st.scalars, packB + st.s_elems);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // enqueued like RecomputeForm::step: a failed factorisation leaves flag[1] = 0 and a candidate nobody uses
  int step(const double* packB, double radius, int refresh, double* packC) {
    const int n = st.D.n;
    int e;
    if (n > 0) {
      if (!in_place) VSL_HIP(ctx, hipMemcpyAsync(st.S, packB, sizeof(double) * st.s_elems, hipMemcpyDeviceToDevice, ctx->stream));
      hipLaunchKernelGGL(sess_damp_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, st.s_elems, packB, 1.0 / radius,
                         refresh, st.diagc_keep, st.S_eff(), st.ldS, st.rhs, st.flag);  // (sets both flags)
      VSL_CHECK_LAUNCH(ctx);
    }
    if ((e = ba_solve_enqueue(ctx, st, n > 0))) return e;  // (no free camera: it sets the flags itself)
    if ((e = ba_candidate(ctx, st, sb))) return e;
    hipLaunchKernelGGL(sess_pack_c_kernel, dim3(1), dim3(64), 0, ctx->stream, st.scalars, st.flag, packC);
    VSL_CHECK_LAUNCH(ctx);
    return VSL_OK;
  }

  // (the next iteration reads this point's cost from the new linearisation)
  int accept() {
    std::swap(st.poses, st.cand_poses);
    std::swap(st.points, st.cand_points);
    int e = ba_linearize(ctx, st, sb, true);
    if (e) return e;
    return ba_columns(ctx, st, sb);
  }
};

// ------------------------------------------------------------------------------- the session
// A rank's share of the problem on the device.  vsl_global_bundle_adjust creates it, solves it and drops it.
struct Session {
  vsl_ctx* ctx = nullptr;
  BaState st;
  int lm_first = 0, n_lms_total = 0;
  ~Session() {
    if (ctx) (void)hipStreamSynchronize(ctx->stream);  // before the arena is freed
  }
};

// sub-problem of the owned landmarks [lm_first, lm_first + lm_count) (all cameras), set-up
int sess_create(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, int lm_first, int lm_count, bool matrix_free,
                Session& s) {
  BaTrace tr;
  BaSubObs own;
  vsl_ba_problem sub = *prob;
  if (!(lm_first == 0 && lm_count == prob->n_lms)) {  // (one rank: the problem itself, no copy)
    try {
      sub = ba_sub_problem(prob, lm_first, lm_count, own);
    } catch (const std::bad_alloc&) {
      return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    if (sub.n_obs == 0) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_global_bundle_adjust: this rank's landmark range has no observations");
  }
  tr.lap("session: sub-problem");
  s.ctx = ctx;
  s.lm_first = lm_first;
  s.n_lms_total = prob->n_lms;
  // band order from the FULL problem: identical on every rank
  BaCaller caller{BaUse::SESSION, prob, BL_THREADS, BL_LMW};
  caller.matrix_free = matrix_free;
  return ba_setup(ctx, &sub, opt, s.st, caller);
}

// the switch of the matrix-free route: diagnostic "ba_iterative_schur" or the environment variable VSL_BA_ITERATIVE
bool iterative_schur_on(const vsl_ctx* ctx) {
  static const bool env_on = getenv("VSL_BA_ITERATIVE") != nullptr;
  return ctx->ba_iterative_schur || env_on;
}

// ---- the matrix-free hooks (vsl_ba_schur_apply, vsl_ba_schur_pcg): S of vsl_ba_linearize, never formed
// set-up and ONE linearisation without Jacobi scaling and without damping: H, Z blocks, and g in st.dc
int mf_linearize(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, BaState& st) {
  BaCaller caller{BaUse::SESSION, nullptr, BL_THREADS, BL_LMW};
  caller.matrix_free = true;
  caller.runs_at_any_size = true;
  int e = ba_setup(ctx, prob, opt, st, caller);
  if (e) return e;
  const BaDims& D = st.D;
  BaRecompute& rc = st.rc;
  RecomputeForm f{ctx, st, rc, true};
  hipLaunchKernelGGL(bpcg_fill_kernel, dim3((D.n + 255) / 256), dim3(256), 0, ctx->stream, (size_t)D.n, 1.0, st.scale_c);
  hipLaunchKernelGGL(bpcg_fill_kernel, dim3((3 * D.L + 255) / 256), dim3(256), 0, ctx->stream, 3 * (size_t)D.L, 1.0, st.scale_l);
  VSL_CHECK_LAUNCH(ctx);
  if ((e = f.prepare())) return e;
  const BlArgs a = f.args();
  // (scale = 1 and 1 / radius = 0: the blocks of the unscaled, undamped problem, Huber corrector applied)
  hipLaunchKernelGGL(bal_prep_kernel<false>, dim3(rc.n_wg), dim3(BL_THREADS), 0, ctx->stream, a, st.cam_pos, 0.0, st.Yg, st.Pinv, st.bl,
                     rc.pbs, (double*)nullptr, rc.lpart);
  hipLaunchKernelGGL(bal_cam_kernel<false>, dim3(D.nfree, rc.bl_seg), dim3(256), 0, ctx->stream, a, st.free_cams, st.cam_start, rc.cam_lm,
                     rc.cam_uv, rc.pbs, st.cam_part);
  hipLaunchKernelGGL(bal_cam_finish_kernel, dim3((D.nfree * 33 + 255) / 256), dim3(256), 0, ctx->stream, D.nfree, rc.bl_seg, 1,
                     st.cam_part, st.H, st.g_c, st.rhs, rc.n_wg, rc.lpart, st.scalars, st.scalars + 8);
  hipLaunchKernelGGL(bpcg_add_kernel, dim3((D.n + 255) / 256), dim3(256), 0, ctx->stream, D.n, st.rhs, st.g_c, st.dc);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int mf_check(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, const char* who, int* nfree) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!opt) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: options are null", who);
  *nfree = 0;
  for (int c = 0; c < prob->n_cams; c++) *nfree += prob->cam_fixed[c] ? 0 : 1;
  if (*nfree == 0) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: no free camera, there is no reduced camera system", who);
  return VSL_OK;
}

// The Levenberg-Marquardt loop.  poses_out [7 * n_cams] and points_all_out [3 * n_lms of the FULL problem] (host)
// receive the result on every rank.  Per iteration: SUM of packB, MAX of one scalar after an accepted step, SUM of the
// 8 doubles of packC.
template <class Form>
int sess_solve(Session& s, Form f, vsl_allreduce_fn allreduce, void* user, int world, const vsl_ba_options* opt, double* poses_out,
               double* points_all_out, vsl_ba_summary* summary) {
  vsl_ctx* ctx = s.ctx;
  BaCommon& st = s.st;
  const int n = st.D.n, max_iters = opt->max_num_iterations, verbosity = opt->verbosity;
  const size_t elems = st.s_elems, nB = elems + 3 * (size_t)n + 2;
  int rc;
  if ((rc = f.prepare())) return rc;
  const double t_start = now_ms();
  const size_t n_gather = 3 * (size_t)s.n_lms_total;  // every rank's landmarks
  double *bufA, *packB, *packC, *gl, *gather;
  ArenaPlan plan(5);
  plan.add(bufA, (size_t)n + 1);
  plan.add(packB, nB);
  plan.add(packC, 10);
  plan.add(gl, 1);
  plan.add(gather, n_gather);
  DevArena arena;
  if (arena.acquire(ctx, ArenaPolicy::OWNED, plan) != hipSuccess)
    return vsl_fail(ctx, VSL_ERR_NOMEM, "vsl_global_bundle_adjust: device allocation failed");
  auto AR = [&](double* buf, size_t count, int op) -> int {
    if (!allreduce) return VSL_OK;  // a caller that passes a callback at world 1 gets its (trivial) collectives: tests
    const int rc = allreduce(user, buf, (int64_t)count, op, (void*)ctx->stream);
    return rc ? vsl_fail(ctx, VSL_ERR_HIP, "all-reduce callback failed (%d)", rc) : VSL_OK;
  };
  auto D2H = [&](void* dst, const void* src, size_t bytes) -> int {
    VSL_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VSL_OK;
  };
  vsl_ba_summary sum;
  memset(&sum, 0, sizeof(sum));
  VSL_HIP(ctx, hipMemsetAsync(gl, 0, 8, ctx->stream));
  // iteration 0: cost, Jacobi scaling from the global column norms
  if ((rc = f.init(bufA))) return rc;
  if ((rc = AR(bufA, (size_t)n + 1, 0))) return rc;
  if ((rc = f.scale(bufA))) return rc;
  double h2[2];
  if ((rc = D2H(h2, bufA + n, 8))) return rc;
  sum.initial_cost = h2[0];
  LmState lm;
  double cost = sum.initial_cost, gmax = INFINITY;
  int it = 0, term, refresh = 1;
  bool have_h2 = false;
  double* const hostpack = packC + 8;  // [cost | max |gradient|] behind the 8 doubles of packC: one copy brings both
  sum.termination = 0;
  if (verbosity >= 2) lm_print_header(cost);
  while (true) {
    if ((rc = f.reduce(lm.radius, packB, gl))) return rc;
    if ((rc = AR(packB, nB, 0))) return rc;
    if (refresh) {
      if ((rc = AR(gl, 1, 1))) return rc;
      hipLaunchKernelGGL(sess_gmax_c_kernel, dim3(1), dim3(1024), 0, ctx->stream, n, packB + elems + 2 * (size_t)n, st.scale_c,
                         packB + elems + 3 * (size_t)n, gl, hostpack);
      VSL_CHECK_LAUNCH(ctx);
      have_h2 = false;  // (cost, |gradient|) of this linearisation: read together with the step's verdict below --
                        // ONE host round trip per iteration; a gradient below tolerance is found one step late, and
                        // that step is dropped
    }
    if (it >= max_iters) {
      if (!have_h2) {
        if ((rc = D2H(h2, hostpack, 16))) return rc;
        cost = h2[0];
        gmax = h2[1];
      }
      sum.termination = 0;
      break;
    }
    if ((term = lm_gate(lm, have_h2 ? gmax : INFINITY)) >= 0) { sum.termination = term; break; }
    it++;
    if ((rc = f.step(packB, lm.radius, refresh, packC))) return rc;
    if ((rc = AR(packC, 8, 0))) return rc;
    double c[10];
    if ((rc = D2H(c, packC, 80))) return rc;
    if (!have_h2) {
      cost = c[8];
      gmax = c[9];
      have_h2 = true;
      if (gmax <= LM_GRADIENT_TOLERANCE) {  // lm_gate's first test, one step late
        it--;
        sum.termination = 2;
        break;
      }
    }
    const double cams_step2 = c[5] / world, cams_x2 = c[6] / world;
    const double step_norm = sqrt(std::max(c[2] - (world - 1) * cams_step2, 0.0));
    const double x_norm = sqrt(std::max(c[3] - (world - 1) * cams_x2, 0.0));
    const double radius_used = lm.radius;
    LmInfo info;
    const int verdict = lm_judge(lm, c[0] == 0.0 && c[1] > 0.0, cost, c[4], c[1], step_norm, x_norm, &info);
    if (verdict >= 0) { sum.termination = verdict; break; }
    refresh = verdict == LM_ACCEPTED;
    if (verdict == LM_INVALID) continue;
    if (verbosity >= 2) lm_print_row(it, c[4], info.cost_change, gmax, step_norm, info.rel, radius_used);
    if (verdict == LM_ACCEPTED) {
      if ((rc = f.accept())) return rc;
      sum.successful_steps++;
    }
  }
  sum.iterations = it;
  sum.final_cost = cost;
  VSL_HIP(ctx, hipMemcpyAsync(poses_out, st.poses, sizeof(double) * 7 * (size_t)st.D.C, hipMemcpyDeviceToHost, ctx->stream));
  // the points: a zero buffer with the own range filled in, summed over the ranks
  VSL_HIP(ctx, hipMemsetAsync(gather, 0, 8 * n_gather, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(gather + 3 * (size_t)s.lm_first, st.points, sizeof(double) * 3 * (size_t)st.D.L, hipMemcpyDeviceToDevice,
                              ctx->stream));
  if ((rc = AR(gather, n_gather, 0))) return rc;
  VSL_HIP(ctx, hipMemcpyAsync(points_all_out, gather, 8 * n_gather, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  sum.total_ms = now_ms() - t_start;
  if (verbosity >= 1)
    fprintf(stderr, "vsl global BA (%d rank%s, %s system, bandwidth %d of %d): iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n",
            world, world > 1 ? "s" : "", st.cyclic ? "cyclic band" : (st.banded ? "band" : "dense"), st.bw, n, sum.iterations, sum.initial_cost, sum.final_cost,
            sum.termination, sum.total_ms);
  if (summary) *summary = sum;
  return VSL_OK;
}
}  // namespace

// global_bundle_adjustment (include/visnav/loop_closure_utils.h:672-748) over `world` ranks: landmarks are split into
// contiguous ranges balanced by observation count, rank `rank` owns one; poses / points of `prob` are updated in place
// on every rank.  world = 1 (allreduce may be null) is the single-GPU session path.
extern "C" int vsl_global_bundle_adjust(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, vsl_allreduce_fn allreduce,
                                        void* user, int rank, int world, vsl_ba_summary* summary) {
  int rc = ba_validate(ctx, prob);
  if (rc) return rc;
  if (!opt || world < 1 || rank < 0 || rank >= world || (world > 1 && !allreduce))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_global_bundle_adjust: bad arguments");
  // the matrix-free route has no distributed form (H would have to be summed and the products exchanged per PCG
  // iteration): refused on every rank alike, before any collective
  const bool iterative = iterative_schur_on(ctx);
  if (iterative && world > 1)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_global_bundle_adjust: iterative Schur (\"ba_iterative_schur\" / VSL_BA_ITERATIVE) runs on one rank only");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  // systems of at most 128 unknowns keep their one-workgroup dense solve: the switch is for large maps
  int nfree_all = 0;
  for (int c = 0; c < prob->n_cams; c++) nfree_all += prob->cam_fixed[c] ? 0 : 1;
  const bool matrix_free = iterative && 6 * nfree_all > 128;
  // contiguous landmark ranges balanced by observation count (the same rule as visual-slam_amd/dist.py landmark_ranges)
  std::vector<int64_t> csum(prob->n_lms + 1, 0);
  for (int i = 0; i < prob->n_obs; i++) csum[prob->obs_lm[i] + 1]++;
  for (int l = 0; l < prob->n_lms; l++) csum[l + 1] += csum[l];
  std::vector<int> cuts(world + 1, 0);
  for (int r = 1; r < world; r++) {
    const double target = (double)csum[prob->n_lms] * r / world;
    cuts[r] = (int)(std::lower_bound(csum.begin(), csum.end(), target, [](int64_t v, double t) { return (double)v < t; }) - csum.begin());
    cuts[r] = std::min(std::max(cuts[r], cuts[r - 1]), prob->n_lms);
  }
  cuts[world] = prob->n_lms;
  // Every rank computes ALL ranges, so decisions about them are identical everywhere (a rank that returned alone
  // would leave the others waiting in the first all-reduce).  A range emptied by the balancing rule (few, heavy
  // landmarks) is widened to one landmark; fewer landmarks than ranks is an error on every rank alike.
  if (prob->n_lms < world)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_global_bundle_adjust: %d landmarks cannot be split over %d ranks (every rank fails alike)",
                    prob->n_lms, world);
  for (int r = 1; r < world; r++) cuts[r] = std::min(std::max(cuts[r], cuts[r - 1] + 1), prob->n_lms - (world - r));
  const int first = cuts[rank], count = cuts[rank + 1] - cuts[rank];
  Session s;
  rc = sess_create(ctx, prob, opt, first, count, matrix_free, s);
  if (world > 1 && allreduce) {
    // rank-local failures (allocation, a bad range) are agreed on BEFORE the first data collective: MAX of a flag
    double* flag = ctx->status_word;  // allocated with the context: never null, so the collective is always entered
    int frc = 0;
    const double mine = rc ? 1.0 : 0.0;
    double any = mine;
    if (hipMemcpyAsync(flag, &mine, 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) frc = VSL_ERR_HIP;
    // (a rank that cannot stage the flag still enters the collective with whatever the word holds: it is about to
    // fail anyway and must not leave the others hanging)
    const int arc = allreduce(user, flag, 1, 1, (void*)ctx->stream);
    if (!arc && !frc && hipMemcpyAsync(&any, flag, 8, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess)
      (void)hipStreamSynchronize(ctx->stream);
    if (rc || frc || arc || any != 0.0) {
      if (rc) return rc;  // this rank's own message is already in place
      return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_global_bundle_adjust: set-up failed on %s (all ranks leave together)",
                      (frc || arc) ? "this rank's status exchange" : "another rank");
    }
  } else if (rc) {
    return rc;
  }
  const bool in_place = !allreduce;  // no collective: a constant of this solve
  BaState& st = s.st;
  if (st.recompute)
    return sess_solve(s, RecomputeForm{ctx, st, st.rc, in_place}, allreduce, user, world, opt, prob->poses, prob->points, summary);
  return sess_solve(s, StoredForm{ctx, st, st.sb, in_place}, allreduce, user, world, opt, prob->poses, prob->points, summary);
}

// y = S x with S exactly as vsl_ba_linearize documents it, never formed (include/vslam_hip.h)
extern "C" int vsl_ba_schur_apply(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, const double* x, double* y,
                                  int n_free) {
  int nfree = 0;
  int rc = mf_check(ctx, prob, opt, "vsl_ba_schur_apply", &nfree);
  if (rc) return rc;
  if (!x || !y || n_free != nfree)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_schur_apply: null vector, or n_free = %d where the problem has %d free cameras", n_free, nfree);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  BaState st;
  if ((rc = mf_linearize(ctx, prob, opt, st))) return rc;
  RecomputeForm f{ctx, st, st.rc, true};
  const int n = st.D.n;
  VSL_HIP(ctx, hipMemcpyAsync(st.rc.pcg_p, x, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  const BpcgOp a = f.pcg_op(nullptr, 0.0);
  if ((rc = f.pcg_product(a, nullptr, st.rc.pcg_p))) return rc;
  hipLaunchKernelGGL(bpcg_apply_finish_kernel, dim3((nfree + 255) / 256), dim3(256), 0, ctx->stream, a, (const double*)st.rc.pcg_p,
                     (const double*)st.rc.pcg_part, st.rc.pcg_q);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpyAsync(y, st.rc.pcg_q, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VSL_OK;
}

// S x = b by block-Jacobi PCG, same S (include/vslam_hip.h)
extern "C" int vsl_ba_schur_pcg(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, const double* b, double tol,
                                int max_iterations, double* x, int* iterations, double* rel_residual) {
  int nfree = 0;
  int rc = mf_check(ctx, prob, opt, "vsl_ba_schur_pcg", &nfree);
  if (rc) return rc;
  if (!x || !(tol >= 0.0) || max_iterations < 0)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_schur_pcg: null x, a negative or non-finite tolerance, or a negative iteration count");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  BaState st;
  if ((rc = mf_linearize(ctx, prob, opt, st))) return rc;
  RecomputeForm f{ctx, st, st.rc, true};
  const int n = st.D.n;
  if (b) VSL_HIP(ctx, hipMemcpyAsync(st.dc, b, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));  // (else g, where mf_linearize left it)
  BpcgRec h;
  if ((rc = f.pcg_solve(f.pcg_op(nullptr, 0.0), st.dc, tol, max_iterations, &h))) return rc;
  hipLaunchKernelGGL(bpcg_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, (const double*)st.rc.pcg_x,
                     (const BpcgRec*)st.rc.pcg_rec, 1.0, st.rc.pcg_q, (int*)nullptr);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpyAsync(x, st.rc.pcg_q, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (iterations) *iterations = h.iterations;
  if (rel_residual) *rel_residual = ba_pcg_rel_residual(h);
  if (h.status == BPCG_NUMERIC)
    return vsl_fail(ctx, VSL_ERR_NUMERIC, "vsl_ba_schur_pcg: %s after %d iterations (S is not positive definite to working precision); x = 0",
                    h.pivot_fail ? "a preconditioner block has a non-positive pivot" : "breakdown (p.Sp <= 0 or a non-finite value)", h.iterations);
  return VSL_OK;
}

// Diagnostic hook (include/vslam_hip.h): the damped, Jacobi-scaled system of the LM loop's FIRST step at the point handed
// in, through the loop's own functions -- RecomputeForm::init, scale, reduce, damp, pcg_damped -- and what the solve
// leaves behind.  Nothing here is a copy of the loop: a change to those functions changes what this reports.
extern "C" int vsl_ba_pcg_system(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, double inv_radius,
                                 const double* b, const double* v, double tol, int max_iterations, double* scale_c, double* rhs,
                                 double* cost, double* Minv, double* x, double* y, vsl_ba_pcg_record* record) {
  int nfree = 0;
  int rc = mf_check(ctx, prob, opt, "vsl_ba_pcg_system", &nfree);
  if (rc) return rc;
  if (!(inv_radius >= 0.0) || !std::isfinite(inv_radius) || !(tol >= 0.0) || max_iterations < 0 || (v && !y))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_ba_pcg_system: 1 / radius = %g, tol = %g or max_iterations = %d out of range, or v without y",
                    inv_radius, tol, max_iterations);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  BaState st;
  BaCaller caller{BaUse::SESSION, nullptr, BL_THREADS, BL_LMW};
  caller.matrix_free = true;
  caller.runs_at_any_size = true;
  if ((rc = ba_setup(ctx, prob, opt, st, caller))) return rc;
  const int n = st.D.n;
  const size_t nB = st.s_elems + 3 * (size_t)n + 2;
  double *bufA, *packB, *gl;
  ArenaPlan plan(3);
  plan.add(bufA, (size_t)n + 1);
  plan.add(packB, nB);
  plan.add(gl, 1);
  DevArena arena;
  if (arena.acquire(ctx, ArenaPolicy::OWNED, plan) != hipSuccess) return vsl_fail(ctx, VSL_ERR_NOMEM, "vsl_ba_pcg_system: device allocation failed");
  struct Sync {  // (the arenas are freed when this function returns: nothing may still be running on them)
    vsl_ctx* c;
    ~Sync() { (void)hipStreamSynchronize(c->stream); }
  } sync{ctx};
  RecomputeForm f{ctx, st, st.rc, true};
  const double radius = 1.0 / inv_radius;  // (inf at inv_radius = 0: every 1 / radius below is 0, no damping term)
  VSL_HIP(ctx, hipMemsetAsync(gl, 0, 8, ctx->stream));
  if ((rc = f.prepare())) return rc;
  if ((rc = f.init(bufA))) return rc;
  if ((rc = f.scale(bufA))) return rc;
  if ((rc = f.reduce(radius, packB, gl))) return rc;
  if ((rc = f.damp(packB, radius, 1))) return rc;
  const double* rhs_dev = st.rhs;
  if (b) {
    VSL_HIP(ctx, hipMemcpyAsync(st.dc, b, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    rhs_dev = st.dc;
  }
  BpcgRec h;
  if ((rc = f.pcg_damped(radius, rhs_dev, tol, max_iterations, &h))) return rc;
  // x as the solve left it (sign + 1: the loop's step is its negative), zeros after a numeric failure
  hipLaunchKernelGGL(bpcg_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, (const double*)st.rc.pcg_x,
                     (const BpcgRec*)st.rc.pcg_rec, 1.0, st.rc.pcg_q, (int*)nullptr);
  VSL_CHECK_LAUNCH(ctx);
  auto down = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  };
  VSL_HIP(ctx, down(x, st.rc.pcg_q, sizeof(double) * n));
  VSL_HIP(ctx, down(scale_c, st.scale_c, sizeof(double) * n));
  VSL_HIP(ctx, down(rhs, st.rhs, sizeof(double) * n));
  VSL_HIP(ctx, down(cost, packB + st.s_elems + 3 * (size_t)n, sizeof(double)));
  VSL_HIP(ctx, down(Minv, st.rc.pcg_minv, sizeof(double) * 36 * (size_t)nfree));
  if (v) {
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (x has left pcg_q)
    VSL_HIP(ctx, hipMemcpyAsync(st.rc.pcg_p, v, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    const BpcgOp a = f.pcg_damped_op(radius);
    if ((rc = f.pcg_product(a, nullptr, st.rc.pcg_p))) return rc;
    hipLaunchKernelGGL(bpcg_apply_finish_kernel, dim3((nfree + 255) / 256), dim3(256), 0, ctx->stream, a, (const double*)st.rc.pcg_p,
                       (const double*)st.rc.pcg_part, st.rc.pcg_q);
    VSL_CHECK_LAUNCH(ctx);
    VSL_HIP(ctx, down(y, st.rc.pcg_q, sizeof(double) * n));
  }
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (record) {
    record->status = h.status;
    record->iterations = h.iterations;
    record->pivot_fail = h.pivot_fail;
    record->segments = st.rc.bl_seg;
    record->landmark_runs = st.rc.n_wg;
    record->n_free = nfree;
    record->rr = h.rr;
    record->bb = h.bb;
    record->alpha = h.alpha;
    record->beta = h.beta;
  }
  return VSL_OK;
}
