// ba_pcg.h -- matrix-free preconditioned conjugate gradients on the reduced camera system (iterative Schur).
//
// The recompute form (ba_large.h) already leaves, per linearisation, the blocks Z = F^T E chol(P^-1) of the free
// observations in camera-major order (bal_prep_kernel) and the 6 x 6 blocks H_c (bal_cam_kernel).  With those
//   S v = (H + D) v - sum_l ( sum_{i in l} Z_i ( sum_{j in l} Z_j^T v_c(j) ) )        D: the camera LM diagonal, or none
// so S is never formed, gathered or factorised.  Per iteration three launches:
//   bpcg_lm_kernel    workgroup = a landmark run of bal_prep_kernel, thread = observation: t_l = sum Z_j^T p_c(j) in
//                     observation order;
//   bpcg_cam_kernel   workgroup = (free camera, segment) of bal_cam_kernel: partial of sum Z_i t_l(i);
//   bpcg_step_kernel  ONE workgroup: q = (H + D) p - segments in order, p.q, alpha, x += alpha p, r -= alpha q,
//                     z = M^-1 r, rho' = r.z, ||r||^2, beta, p = z + beta p, the stopping rule.
// alpha, beta, rho, the iteration count and the verdict live in a BpcgRec on the device.  Every kernel returns at once
// when rec->done is set: the host enqueues iterations in batches and reads the record once per batch, the iterations
// enqueued behind the one that finished change nothing -- the solution's bits do not depend on the batch size.
// Every sum runs in a fixed order (observation order, xor tree inside a wavefront, wavefront / segment / camera-stride
// order afterwards) and there are no floating-point atomics: two solves return the same bits.
// The preconditioner is block Jacobi with the TRUE diagonal block of S,
//   M_c = H_c + D_c - sum_l (sum_{i in c, l} Z_i)(sum_{i in c, l} Z_i)^T      (i: the observations of landmark l by camera c;
//                                                                              one per landmark unless c sees l more than once),
// inverted by a 6 x 6 Cholesky per camera.  A pivot that is not positive sets rec->pivot_fail and leaves M_c^-1 = 0:
// the solve ends as a numeric failure with x = 0, nothing non-finite is produced.
#pragma once
#include "ba_large.h"
#include "ba_pcg_plan.h"

namespace {

#define BPCG_T 1024  // threads of the one-workgroup kernels (16 wavefronts)

struct BpcgOp {
  int nfree, nseg;
  const int *free_cams, *cam_free, *cam_start, *cam_lm, *obs_cam, *cam_pos, *lm_start, *wg_lm;
  const double* Z;     // 18 doubles per observation, camera-major (only free cameras' blocks are written)
  const double* H;     // 36 doubles per free camera
  const double* diag;  // LM diagonal of the cameras (6 per free camera) or null
  double inv_radius;
};

__device__ __forceinline__ void bpcg_load_z(const double* Z, size_t k, double* z) {
  const double2* zp = (const double2*)(Z + 18 * k);
#pragma unroll
  for (int x = 0; x < 9; x++) {
    const double2 v = zp[x];
    z[2 * x] = v.x;
    z[2 * x + 1] = v.y;
  }
}

// sum over the workgroup of BPCG_T threads: xor tree, then the 16 wavefronts in order; every thread gets the value
__device__ __forceinline__ double bpcg_block_sum(double v, double* sh /* [17] */) {
  v = bl_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < BPCG_T / 64; w++) s += sh[w];
    sh[16] = s;
  }
  __syncthreads();
  const double r = sh[16];
  __syncthreads();
  return r;
}

// t[3 l + j] = sum over the free observations of landmark l of (Z^T v_c)[j], observation order
__global__ __launch_bounds__(BL_THREADS) void bpcg_lm_kernel(BpcgOp a, const BpcgRec* __restrict__ rec,
                                                             const double* __restrict__ v, double* __restrict__ t) {
  if (rec && rec->done) return;
  __shared__ double stage_s[BL_THREADS * 3];
  __shared__ int lmo_s[BL_LMW + 1];
  const int tid = threadIdx.x, bid = blockIdx.x;
  const int lm0 = a.wg_lm[bid], n_lm = a.wg_lm[bid + 1] - lm0;
  const int obs0 = a.lm_start[lm0], n_obs = a.lm_start[lm0 + n_lm] - obs0;
  if (tid <= n_lm) lmo_s[tid] = a.lm_start[lm0 + tid] - obs0;
  double w[3] = {0.0, 0.0, 0.0};
  if (tid < n_obs) {
    const size_t q = (size_t)obs0 + tid;
    const int fc = a.cam_free[a.obs_cam[q]];
    if (fc >= 0) {  // (a fixed camera's observation has no Z block)
      double z[18];
      bpcg_load_z(a.Z, (size_t)a.cam_pos[q], z);
#pragma unroll
      for (int x = 0; x < 6; x++) {
        const double pv = v[6 * (size_t)fc + x];
#pragma unroll
        for (int j = 0; j < 3; j++) w[j] += z[3 * x + j] * pv;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; j++) stage_s[3 * tid + j] = w[j];
  __syncthreads();
  if (tid < n_lm) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = lmo_s[tid]; i < lmo_s[tid + 1]; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) s[j] += stage_s[3 * i + j];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) t[3 * (size_t)(lm0 + tid) + j] = s[j];
  }
}

// part[(fc * nseg + seg) * 6 + x] = the segment's share of sum_{i in c} Z_i t_l(i)
__global__ __launch_bounds__(256) void bpcg_cam_kernel(BpcgOp a, const BpcgRec* __restrict__ rec, const double* __restrict__ t,
                                                       double* __restrict__ part) {
  if (rec && rec->done) return;
  __shared__ double sh[4][6];
  const int fc = blockIdx.x, seg = blockIdx.y, nseg = gridDim.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cam = a.free_cams[fc];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = a.cam_start[cam] + seg * 256 + threadIdx.x; k < a.cam_start[cam + 1]; k += 256 * nseg) {
    const int lm = a.cam_lm[k];
    const double t0 = t[3 * (size_t)lm], t1 = t[3 * (size_t)lm + 1], t2 = t[3 * (size_t)lm + 2];
    double z[18];
    bpcg_load_z(a.Z, (size_t)k, z);
#pragma unroll
    for (int x = 0; x < 6; x++) acc[x] += z[3 * x] * t0 + z[3 * x + 1] * t1 + z[3 * x + 2] * t2;
  }
#pragma unroll
  for (int x = 0; x < 6; x++) {
    const double s = bl_wave_sum(acc[x]);
    if (lane == 0) sh[wave][x] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6)
    part[((size_t)fc * nseg + seg) * 6 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// q_c = (H_c + D_c) v_c - (segments in order) for one camera
__device__ __forceinline__ void bpcg_q_of(const BpcgOp& a, int fc, const double* __restrict__ v, const double* __restrict__ part,
                                          double* pc, double* qv) {
#pragma unroll
  for (int x = 0; x < 6; x++) pc[x] = v[6 * (size_t)fc + x];
#pragma unroll
  for (int x = 0; x < 6; x++) {
    double h = 0.0, s = 0.0;
#pragma unroll
    for (int y = 0; y < 6; y++) h += a.H[36 * (size_t)fc + 6 * x + y] * pc[y];
    if (a.diag) h += a.diag[6 * (size_t)fc + x] * a.inv_radius * pc[x];
    for (int sg = 0; sg < a.nseg; sg++) s += part[((size_t)fc * a.nseg + sg) * 6 + x];
    qv[x] = h - s;
  }
}

// y = S v from the segment partials (the product alone: vsl_ba_schur_apply)
__global__ __launch_bounds__(256) void bpcg_apply_finish_kernel(BpcgOp a, const double* __restrict__ v, const double* __restrict__ part,
                                                                double* __restrict__ y) {
  const int fc = blockIdx.x * blockDim.x + threadIdx.x;
  if (fc >= a.nfree) return;
  double pc[6], qv[6];
  bpcg_q_of(a, fc, v, part, pc, qv);
#pragma unroll
  for (int x = 0; x < 6; x++) y[6 * (size_t)fc + x] = qv[x];
}

// M_c^-1 (36 doubles, symmetric) of M_c = H_c + D_c - sum_l (sum_{i in c, l} Z_i)(sum_{i in c, l} Z_i)^T: the squares
// Z_i Z_i^T of every observation, plus the cross terms of a landmark the camera observes more than once; one workgroup
// per free camera
__global__ __launch_bounds__(256) void bpcg_precond_kernel(BpcgOp a, double* __restrict__ Minv, BpcgRec* __restrict__ rec) {
  __shared__ double sh[4][21];
  const int fc = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cam = a.free_cams[fc];
  double acc[21];
#pragma unroll
  for (int e = 0; e < 21; e++) acc[e] = 0.0;
  for (int k = a.cam_start[cam] + threadIdx.x; k < a.cam_start[cam + 1]; k += 256) {
    double z[18];
    bpcg_load_z(a.Z, (size_t)k, z);
    int e = 0;
#pragma unroll
    for (int x = 0; x < 6; x++)
#pragma unroll
      for (int y = x; y < 6; y++) acc[e++] += z[3 * x] * z[3 * y] + z[3 * x + 1] * z[3 * y + 1] + z[3 * x + 2] * z[3 * y + 2];
    // a landmark this camera observes more than once: the block of S holds (sum_i Z_i)(sum_i Z_i)^T, so the cross terms
    // with the earlier observations of the same landmark are added (they are adjacent: the camera's list is in
    // landmark order).  No trip for a camera that sees every landmark once.
    const int lm = a.cam_lm[k];
    for (int j = k - 1; j >= a.cam_start[cam] && a.cam_lm[j] == lm; j--) {
      double w[18];
      bpcg_load_z(a.Z, (size_t)j, w);
      e = 0;
#pragma unroll
      for (int x = 0; x < 6; x++)
#pragma unroll
        for (int y = x; y < 6; y++)
          acc[e++] += (z[3 * x] * w[3 * y] + z[3 * x + 1] * w[3 * y + 1] + z[3 * x + 2] * w[3 * y + 2]) +
                      (w[3 * x] * z[3 * y] + w[3 * x + 1] * z[3 * y + 1] + w[3 * x + 2] * z[3 * y + 2]);
    }
  }
#pragma unroll
  for (int e = 0; e < 21; e++) {
    const double s = bl_wave_sum(acc[e]);
    if (lane == 0) sh[wave][e] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double M[6][6], Lm[6][6], Li[6][6];
  {
    int e = 0;
    for (int x = 0; x < 6; x++)
      for (int y = x; y < 6; y++) {
        const double zz = ((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e];
        double h = a.H[36 * (size_t)fc + 6 * x + y];
        if (x == y && a.diag) h += a.diag[6 * (size_t)fc + x] * a.inv_radius;
        M[x][y] = M[y][x] = h - zz;
        e++;
      }
  }
  bool ok = true;
  for (int j = 0; j < 6; j++) {
    double d = M[j][j];
    for (int k = 0; k < j; k++) d -= Lm[j][k] * Lm[j][k];
    if (!(d > 0.0) || !isfinite(d)) {
      ok = false;
      break;
    }
    const double l = sqrt(d);
    Lm[j][j] = l;
    for (int i = j + 1; i < 6; i++) {
      double s = M[i][j];
      for (int k = 0; k < j; k++) s -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = s / l;
    }
  }
  if (ok) {
    // Li = L^-1 (lower), M^-1 = Li^T Li
    for (int c = 0; c < 6; c++)
      for (int i = 0; i < 6; i++) {
        if (i < c) {
          Li[i][c] = 0.0;
          continue;
        }
        double s = i == c ? 1.0 : 0.0;
        for (int k = c; k < i; k++) s -= Lm[i][k] * Li[k][c];
        Li[i][c] = s / Lm[i][i];
      }
    for (int x = 0; x < 6; x++)
      for (int y = x; y < 6; y++) {
        double s = 0.0;
        for (int k = y; k < 6; k++) s += Li[k][x] * Li[k][y];
        ok = ok && isfinite(s);
        M[x][y] = M[y][x] = s;
      }
  }
  if (!ok) rec->pivot_fail = 1;
  for (int x = 0; x < 6; x++)
    for (int y = 0; y < 6; y++) Minv[36 * (size_t)fc + 6 * x + y] = ok ? M[x][y] : 0.0;
}

__device__ __forceinline__ void bpcg_minv(const double* __restrict__ Minv, int fc, const double* r, double* z) {
#pragma unroll
  for (int x = 0; x < 6; x++) {
    double s = 0.0;
#pragma unroll
    for (int y = 0; y < 6; y++) s += Minv[36 * (size_t)fc + 6 * x + y] * r[y];
    z[x] = s;
  }
}

// x = 0, r = b, z = M^-1 r, p = z, rho = r.z, ||b||^2; the record's verdict before the first iteration.  One workgroup.
// (rec->pivot_fail was cleared before bpcg_precond_kernel ran.)
__global__ __launch_bounds__(BPCG_T) void bpcg_init_kernel(int nfree, const double* __restrict__ b, const double* __restrict__ Minv,
                                                           double tol, int max_it, double* __restrict__ x, double* __restrict__ r,
                                                           double* __restrict__ z, double* __restrict__ p, BpcgRec* __restrict__ rec) {
  __shared__ double sh[17];
  double rho = 0.0, bb = 0.0;
  for (int fc = threadIdx.x; fc < nfree; fc += BPCG_T) {
    double rv[6], zv[6];
#pragma unroll
    for (int k = 0; k < 6; k++) rv[k] = b[6 * (size_t)fc + k];
    bpcg_minv(Minv, fc, rv, zv);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const size_t i = 6 * (size_t)fc + k;
      x[i] = 0.0;
      r[i] = rv[k];
      z[i] = zv[k];
      p[i] = zv[k];
      rho += rv[k] * zv[k];
      bb += rv[k] * rv[k];
    }
  }
  rho = bpcg_block_sum(rho, sh);
  bb = bpcg_block_sum(bb, sh);
  if (threadIdx.x != 0) return;
  const double tol2 = tol * tol;
  rec->rho = rho;
  rec->alpha = rec->beta = rec->pq = rec->pad0 = 0.0;
  rec->bb = bb;
  rec->rr = bb;
  rec->tol2 = tol2;
  rec->iterations = 0;
  rec->max_it = max_it;
  int status = BPCG_RUNNING;
  if (rec->pivot_fail || !isfinite(rho) || !isfinite(bb)) status = BPCG_NUMERIC;
  else if (bb <= tol2 * bb) status = BPCG_CONVERGED;  // (b = 0: x = 0 is the solution)
  else if (max_it <= 0) status = BPCG_CAP;
  else if (!(rho > 0.0)) status = BPCG_NUMERIC;
  rec->status = status;
  rec->done = status != BPCG_RUNNING;
}

// the rest of an iteration after the two passes of the product.  One workgroup.
__global__ __launch_bounds__(BPCG_T) void bpcg_step_kernel(BpcgOp a, const double* __restrict__ part, const double* __restrict__ Minv,
                                                           double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                           double* __restrict__ p, double* __restrict__ q, BpcgRec* __restrict__ rec) {
  if (rec->done) return;
  __shared__ double sh[17];
  const double rho = rec->rho;
  double pq = 0.0;
  for (int fc = threadIdx.x; fc < a.nfree; fc += BPCG_T) {
    double pc[6], qv[6];
    bpcg_q_of(a, fc, p, part, pc, qv);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      q[6 * (size_t)fc + k] = qv[k];
      pq += pc[k] * qv[k];
    }
  }
  pq = bpcg_block_sum(pq, sh);
  if (!(pq > 0.0) || !isfinite(pq)) {  // breakdown: S is not positive definite along p (uniform: every thread holds the same pq)
    if (threadIdx.x == 0) {
      rec->pq = pq;
      rec->status = BPCG_NUMERIC;
      rec->done = 1;
    }
    return;
  }
  const double alpha = rho / pq;
  double rz = 0.0, rr = 0.0;
  for (int fc = threadIdx.x; fc < a.nfree; fc += BPCG_T) {
    double rv[6], zv[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const size_t i = 6 * (size_t)fc + k;
      x[i] = x[i] + alpha * p[i];
      rv[k] = r[i] - alpha * q[i];
      r[i] = rv[k];
    }
    bpcg_minv(Minv, fc, rv, zv);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      z[6 * (size_t)fc + k] = zv[k];
      rz += rv[k] * zv[k];
      rr += rv[k] * rv[k];
    }
  }
  rz = bpcg_block_sum(rz, sh);
  rr = bpcg_block_sum(rr, sh);
  const double beta = rz / rho;
  for (int fc = threadIdx.x; fc < a.nfree; fc += BPCG_T) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const size_t i = 6 * (size_t)fc + k;
      p[i] = z[i] + beta * p[i];
    }
  }
  if (threadIdx.x != 0) return;
  const int it = rec->iterations + 1;
  rec->iterations = it;
  rec->rho = rz;
  rec->alpha = alpha;
  rec->beta = beta;
  rec->pq = pq;
  rec->rr = rr;
  int status = BPCG_RUNNING;
  if (!isfinite(rz) || !isfinite(rr)) status = BPCG_NUMERIC;
  else if (rr <= rec->tol2 * rec->bb) status = BPCG_CONVERGED;
  else if (it >= rec->max_it) status = BPCG_CAP;  // the last iterate is the step: its error in the S-norm is the smallest so far
  else if (!(rz > 0.0)) status = BPCG_NUMERIC;
  rec->status = status;
  rec->done = status != BPCG_RUNNING;
}

// out = sign * x, or zeros after a numeric failure (x may hold anything then); flag (nullable) = solve usable
__global__ void bpcg_finish_kernel(int n, const double* __restrict__ x, const BpcgRec* __restrict__ rec, double sign,
                                   double* __restrict__ out, int* __restrict__ ok_flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = rec->status != BPCG_NUMERIC;
  if (i < n) out[i] = ok ? sign * x[i] : 0.0;
  if (i == 0 && ok_flag) ok_flag[0] = ok ? 1 : 0;
}

__global__ void bpcg_fill_kernel(size_t n, double v, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// g = rhs + g_c (the reduced right-hand side as vsl_ba_linearize returns it)
__global__ void bpcg_add_kernel(int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

}  // namespace
