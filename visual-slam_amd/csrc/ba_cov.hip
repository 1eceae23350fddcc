// ba_cov.hip -- marginal covariances of poses and landmarks of a bundle-adjustment problem (vsl_ba_covariance,
// vsl_global_ba_covariance): what ceres::Covariance offers beside ceres::Solve (include/visnav/map_utils.h:405-411 calls
// only the latter).
//
// Nothing is optimised: the problem is linearised once at the poses and points handed in, exactly as vsl_ba_linearize
// documents it (Huber corrector on residual and Jacobian blocks, no Jacobi scaling, no damping).  With H = J^T J over
// the free cameras (6-vector tangent (upsilon, omega) of T exp(delta), free-camera index order) and all landmarks, the
// covariance is H^-1 (unit: 1 px^2 of observation noise).  By the block inverse of H, with S the reduced camera system,
// P_l = sum E^T E of landmark l and W_c = F_c^T E_c of its observation in free camera c:
//   pose block      Sigma_cc = [S^-1]_cc
//   landmark block  Sigma_ll = P_l^-1 + P_l^-1 (sum_c sum_c' W_c^T [S^-1]_cc' W_c') P_l^-1
//
// The chain, all on the context's stream:
//   ba_linearize -> ba_columns -> ba_schur (ba.hip: the kernels behind vsl_ba_linearize)          S, dense
//   ba_cov_diag_kernel                                                                             diag S, kept for the pivot test
//   vsl_chol_factor_dev (chol.hip: the dense panel factorisation)                                  S <- L, inverted diagonal blocks
//   ba_cov_solve_kernel      L L^T X = E_Q, Q = queried cameras + free cameras observing a queried landmark, six unit
//                            columns per camera, COV_COLS columns per workgroup
//   ba_cov_pose_kernel       the diagonal 6 x 6 blocks of X, symmetrised
//   ba_cov_landmark_kernel   one wavefront per queried landmark: E, F and the corrector re-evaluated at the state
//                            (ba_device.h / ba_large.h), P_l, W_c, the double sum in ascending (c, c') order
// Everything runs in a fixed order and without atomics: a column of X has the same bits whichever columns share its
// workgroup (an output of v_mfma_f64_16x16x4_f64 depends on its own row of A and column of B only), so a subset query
// returns the bits of the same rows of a full query, and two calls return the same bits.
//
// TWO ROUTES.  vsl_ba_covariance is the dense one, whatever the size: S is formed and factorised in dense storage (the
// dense path of vsl_spd_solve), so its cost grows with (6 x free cameras)^2 x columns -- the call for a local window.
// vsl_global_ba_covariance takes ba_reduced_layout's decision for the problem (linear band allowed, cyclic never):
// dense -> the chain above, bit for bit; linear band -> the free cameras in reverse Cuthill-McKee order (ba_setup, as
// for vsl_bundle_adjust), ba_schur into LAPACK-style band storage, and
//   vsl_chol_selinv_band_dev (chol.hip "SELECTED INVERSION")   S <- L, Z <- the band of S^-1, O(n bw^2)
//   cov_band_pivot_kernel                                       the pivot test below on the factor in the band
//   cov_band_pose_kernel                                        diagonal blocks of Z, lower triangle mirrored
//   ba_cov_landmark_band_kernel                                 the landmark scheme above, [S^-1]_cc' read from Z: cameras
//                            that observe one landmark are adjacent in the covisibility graph, so the block is in the band
// Z does not depend on the query, and a landmark's sum runs over its own observations in ascending band position: the
// subset and run-to-run guarantees hold on this route as well.  A queried landmark may have at most COV_KMAX
// observations (its W blocks are kept in LDS) on either route.
//
// THE SHARED LAYER.  "diag of the matrix, then its inverse one of two ways, then blocks of the inverse" is one chain for
// the reduced camera system here and for the pose graph's H (pgo_cov.hip), written once at the end of this file:
//   vsl_cov_diag_dev          ba_cov_diag_kernel, dense or band storage
//   vsl_cov_inverse_dev       that, then dense: vsl_chol_factor_dev + unit columns; band: vsl_chol_selinv_band_dev, the
//                             pivot test, and unit columns against the band factor where the plan has any
//   vsl_cov_diag_blocks_dev   the 6 x 6 diagonal blocks (dense: from X, mirror entries averaged; band: from Z, mirrored)
//   vsl_cov_pair_blocks_dev   ba_pair_blocks_kernel: the 12 x 12 joint blocks of pairs
// Every covariance call of either side goes through them, so a joint call's diagonal blocks are the marginal call's
// bytes by construction: the same kernels on the same columns (a node-list query and a pair query that name the same
// nodes get the same ascending unique columns from pgo_cov_plan.h, hence the same workgroups; and were the grouping to
// differ, a column's bits do not depend on its neighbours, see above).  vsl_spd_inverse_band (chol.hip) uses the dense
// unit-column solve alone (vsl_cov_unit_columns_dev).
//
// "Not positive definite" is decided to working precision: a pivot L_ii^2 <= 2^-36 S_ii fails the factorisation
// (VSL_ERR_NUMERIC); the ratio is invariant under a rescaling of the unknowns.  A free gauge (no fixed camera) leaves
// pivots of rounding-noise size, which a bare "> 0" test lets through about half of the time.  The same rule with
// 2^-44 on the three pivots of P_l marks a landmark degenerate (a single observation has rank 2).
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "vsl_common.h"
#include "dev_arena.h"
#include "ba_host_plan.h"
#include "ba_cov_plan.h"
#include "ba_pair_plan.h"
#include "ba_device.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // ba_large.h: only bl_eval and bl_wave_sum are used here, not its kernels
#include "ba_large.h"
#pragma clang diagnostic pop
#include "ba_state.h"
#include "pgo_device.h"
#include "relpose_math.h"

// (COV_NB, COV_COLS: ba_cov_plan.h)
#define COV_THREADS 256
#define COV_CHUNK 64        // rows (forward) / columns (backward) of L staged in LDS per step: one 16-row tile per wavefront
#define COV_LP 34           // LDS row pitches (doubles): 2 r + k and 16 k + c fall on distinct banks within a half wavefront
#define COV_LQ 80
#define COV_KMAX 256        // observations of a queried landmark (27 doubles of LDS each)
#define COV_PIVOT_TOL 1.4551915228366852e-11  // 2^-36
#define COV_LM_TOL 5.6843418860808015e-14     // 2^-44

static_assert(COV_NB == 32 && COV_CHUNK == 16 * (COV_THREADS / 64), "tile arithmetic of ba_cov_solve_kernel");

namespace {

typedef double cov_v4d __attribute__((ext_vector_type(4)));

// (entry (row i, right-hand side col) of X: vsl_cov_x_at of vsl_common.h -- workgroup blocks of n x COV_COLS, row-major)
static_assert(COV_COLS == 16, "vsl_cov_x_at (vsl_common.h) spells the block width out");

// S: the storage as ba_schur / pgo_build_kernel filled it (ld = 0: dense n x n; else band rows of ld + 1 slots, the
// diagonal last)
__global__ void ba_cov_diag_kernel(int n, const double* __restrict__ S, int ld, double* __restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = ld > 0 ? S[(size_t)i * (ld + 1) + ld] : S[(size_t)i * n + i];
}

// band routes: the pivot test of the file header on the factor left in the band storage
// (every failing thread stores the same 0)
__global__ void cov_band_pivot_kernel(int n, const double* __restrict__ L, int ld, const double* __restrict__ d, int* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double l = L[(size_t)i * (ld + 1) + ld], p = l * l;
  if (!(p > COV_PIVOT_TOL * d[i]) || !isfinite(p)) *ok = 0;
}

// band routes: block q = rows / columns 6 q_free[q] .. + 5 of the band array Z (storage base) of the inverse.  Only
// the lower triangle is stored: it is mirrored, so the block is exactly symmetric.
__global__ void cov_band_pose_kernel(int nQ, const int* __restrict__ q_free, const double* __restrict__ Z, int ld,
                                     const int* __restrict__ ok, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * nQ || !*ok) return;
  const int q = t / 36, a = (t % 36) / 6, b = t % 6;
  const int i = 6 * q_free[q] + max(a, b), j = 6 * q_free[q] + min(a, b);
  out[t] = Z[(size_t)i * (ld + 1) + ld - (i - j)];
}

// Joint blocks of pairs of cameras (vsl_ba_relative_pose_covariance) or nodes (vsl_pgo_joint_covariance,
// vsl_pgo_edge_consistency): one thread per entry of a 12 x 12 block of the inverse.  Diagonal blocks: the rule of the
// pose kernels of the same route, bit for bit (band: entry (max, min) of Z as cov_band_pose_kernel; dense: the two
// mirror entries of the camera's own columns averaged as ba_cov_pose_kernel).  Cross block, entry (row r of camera x,
// column c of camera y): with columns for both cameras the average of X_y[6 x + r][c] and X_x[6 y + c][r]; with columns
// for one of them that single entry; with none entry (max, min) of Z.  Every rule gives (x, r; y, c) and (y, c; x, r)
// the same number: the block is symmetric and a swapped pair is the swapped, transposed block.  A fixed camera (f < 0):
// exactly 0.0.  Z: the storage base.
__global__ void ba_pair_blocks_kernel(int n, int n_pairs, const PgcPairDev* __restrict__ pairs, int band, const double* __restrict__ Z,
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

// L L^T X = E for the COV_COLS unit columns col_unk[COV_COLS * blockIdx.x ..] (-1: an empty column) of this workgroup,
// in its n x COV_COLS block of X.  L: the dense factor (n x n row-major, lower triangle), Linv: its inverted COV_NB x
// COV_NB diagonal blocks (zero above the diagonal, identity-padded in the last one), Sdiag: diag S before the
// factorisation (nullable: no pivot test here).  Right-looking in both directions, one panel of COV_NB unknowns per step:
//   forward   Y_k = Linv_kk B_k, then B_i -= L[i, k] Y_k for the rows below, COV_CHUNK rows of the panel in LDS at a time
//   backward  X_k = Linv_kk^T Y_k, then Y_c -= L[k, c]^T X_k for the columns before, COV_CHUNK columns at a time
// every product a chain of eight v_mfma_f64_16x16x4_f64 over the 32 unknowns of the panel, one 16 x 16 tile per wavefront.
// An entry of X is touched by one lane per step, panels in ascending (descending) order: a fixed summation order per
// column.  *ok = 0 (by workgroup 0) and nothing written when a pivot fails the test in the file header.
__global__ __launch_bounds__(COV_THREADS) void ba_cov_solve_kernel(int n, const double* __restrict__ L,
                                                                   const double* __restrict__ Linv,
                                                                   const double* __restrict__ Sdiag,
                                                                   const int* __restrict__ col_unk, double* __restrict__ X,
                                                                   int* __restrict__ ok) {
  __shared__ double Li[COV_NB][COV_LP];
  __shared__ double Bk[COV_NB][COV_COLS];
  __shared__ double stage[COV_NB * COV_LQ];  // forward: [COV_CHUNK][COV_LP], backward: [COV_NB][COV_LQ]
  static_assert(COV_CHUNK * COV_LP <= COV_NB * COV_LQ, "the forward view fits");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  int bad = *ok ? 0 : 1;
  if (Sdiag)  // (null: the caller keeps to the factorisation's own pivot test)
    for (int i = tid; i < n; i += COV_THREADS) {
      const double l = L[(size_t)i * n + i], p = l * l;
      if (!(p > COV_PIVOT_TOL * Sdiag[i]) || !isfinite(p)) bad = 1;
    }
  if (__syncthreads_or(bad)) {
    if (blockIdx.x == 0 && tid == 0) *ok = 0;
    return;
  }
  double* __restrict__ Xw = X + (size_t)blockIdx.x * n * COV_COLS;
  for (int t = tid; t < n * COV_COLS; t += COV_THREADS)
    Xw[t] = col_unk[COV_COLS * blockIdx.x + (t % COV_COLS)] == t / COV_COLS ? 1.0 : 0.0;
  __syncthreads();
  const int np = (n + COV_NB - 1) / COV_NB;
  // ---- forward: L Y = E
  for (int p = 0; p < np; p++) {
    const int k = p * COV_NB, nb = min(COV_NB, n - k);
    for (int t = tid; t < COV_NB * COV_NB; t += COV_THREADS) Li[t / COV_NB][t % COV_NB] = Linv[(size_t)p * COV_NB * COV_NB + t];
    for (int t = tid; t < COV_NB * COV_COLS; t += COV_THREADS) {
      const int r = t / COV_COLS;
      Bk[r][t % COV_COLS] = r < nb ? Xw[(size_t)(k + r) * COV_COLS + (t % COV_COLS)] : 0.0;
    }
    __syncthreads();
    cov_v4d acc = {0.0, 0.0, 0.0, 0.0};
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int s = 0; s < COV_NB / 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[16 * wave + l16][4 * s + kq], Bk[4 * s + kq][l16], acc, 0, 0, 0);
    }
    __syncthreads();  // B_k has been read: Y_k takes its place
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * wave + kq + 4 * q;
        Bk[r][l16] = acc[q];
        if (r < nb) Xw[(size_t)(k + r) * COV_COLS + l16] = acc[q];
      }
    }
    __syncthreads();
    for (int i0 = k + COV_NB; i0 < n; i0 += COV_CHUNK) {
      for (int t = tid; t < COV_CHUNK * COV_NB; t += COV_THREADS) {
        const int r = t / COV_NB, c = t % COV_NB;
        stage[r * COV_LP + c] = i0 + r < n ? L[(size_t)(i0 + r) * n + k + c] : 0.0;
      }
      __syncthreads();
      const int r0 = i0 + 16 * wave;
      if (r0 < n) {
        cov_v4d a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < COV_NB / 4; s++)
          a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(stage[(16 * wave + l16) * COV_LP + 4 * s + kq], Bk[4 * s + kq][l16], a2, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int r = r0 + kq + 4 * q;
          if (r < n) Xw[(size_t)r * COV_COLS + l16] -= a2[q];
        }
      }
      __syncthreads();
    }
  }
  // ---- backward: L^T X = Y
  for (int p = np - 1; p >= 0; p--) {
    const int k = p * COV_NB, nb = min(COV_NB, n - k);
    for (int t = tid; t < COV_NB * COV_NB; t += COV_THREADS) Li[t / COV_NB][t % COV_NB] = Linv[(size_t)p * COV_NB * COV_NB + t];
    for (int t = tid; t < COV_NB * COV_COLS; t += COV_THREADS) {
      const int r = t / COV_COLS;
      Bk[r][t % COV_COLS] = r < nb ? Xw[(size_t)(k + r) * COV_COLS + (t % COV_COLS)] : 0.0;
    }
    __syncthreads();
    cov_v4d acc = {0.0, 0.0, 0.0, 0.0};
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int s = 0; s < COV_NB / 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[4 * s + kq][16 * wave + l16], Bk[4 * s + kq][l16], acc, 0, 0, 0);
    }
    __syncthreads();
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * wave + kq + 4 * q;
        Bk[r][l16] = acc[q];
        if (r < nb) Xw[(size_t)(k + r) * COV_COLS + l16] = acc[q];
      }
    }
    __syncthreads();
    for (int c0 = 0; c0 < k; c0 += COV_CHUNK) {
      for (int t = tid; t < COV_NB * COV_CHUNK; t += COV_THREADS) {
        const int r = t / COV_CHUNK, c = t % COV_CHUNK;
        stage[r * COV_LQ + c] = (r < nb && c0 + c < k) ? L[(size_t)(k + r) * n + c0 + c] : 0.0;
      }
      __syncthreads();
      const int cc0 = c0 + 16 * wave;
      if (cc0 < k) {
        cov_v4d a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < COV_NB / 4; s++)
          a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(stage[(4 * s + kq) * COV_LQ + 16 * wave + l16], Bk[4 * s + kq][l16], a2, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int r = cc0 + kq + 4 * q;
          if (r < k) Xw[(size_t)r * COV_COLS + l16] -= a2[q];
        }
      }
      __syncthreads();
    }
  }
}

// The same solve against a BAND factor (vsl_cov_band_unit_columns_dev): true entries of the inverse OUTSIDE the band
// that the selected inversion delivers.  L: the origin of the band array (storage + ld, entry (i, j) at i * ld + j,
// 0 <= i - j <= bw) that vsl_chol_selinv_band_dev left, Linv: its inverted diagonal blocks.  A panel step reaches the bw
// rows below (forward) / the bw columns before (backward) the panel only, in chunks of COV_CHUNK through the same LDS
// stage: O(n bw) per column where the dense kernel is O(n^2).
//   forward   starts at the panel of the block's first unit row: everything above is exactly zero
//   backward  stops at the panel of row_lo[block], the lowest row a caller reads (nullable: row 0); rows above that
//             panel are NOT written
// SHAPE.  The n x COV_COLS result stays in global memory and the rows a step touches (bw + 32 of them: 14 KB at bw = 77)
// are updated there, in the L2: the rows of one step are disjoint 16-row tiles of different wavefronts, a tile is read
// and written once per step, so a sliding window in LDS would save one L2 round trip per tile and step and add the
// copy in and out of the window at every panel.  Not measured against each other; this is the dense kernel's proven
// structure with the band's bounds.
// As there: one lane per entry and step, panels in ascending (descending) order, no atomics -- a column has the same
// bits whichever columns share its workgroup and wherever the forward pass starts (a zero row contributes +0.0).
// UNIT = false (vsl_band_rhs_solve_dev: the pose graph's far-edge route, pgo.hip): GENERAL right-hand sides.  The caller
// has filled X with B; col_unk is not read; row_lo[block] is the block's first non-zero row (n: the block is zero and
// stays so), where the forward pass starts; the backward pass runs to row 0.  Everything else is the same code.
template <bool UNIT>
__global__ __launch_bounds__(COV_THREADS) void cov_band_solve_kernel(int n, const double* __restrict__ L, int ld, int bw,
                                                                     const double* __restrict__ Linv,
                                                                     const int* __restrict__ col_unk,
                                                                     const int* __restrict__ row_lo, double* __restrict__ X,
                                                                     const int* __restrict__ ok) {
  __shared__ double Li[COV_NB][COV_LP];
  __shared__ double Bk[COV_NB][COV_COLS];
  __shared__ double stage[COV_NB * COV_LQ];  // forward: [COV_CHUNK][COV_LP], backward: [COV_NB][COV_LQ]
  if (!*ok) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  int first = n;
  if (UNIT) {
    for (int c = 0; c < COV_COLS; c++) {
      const int u = col_unk[COV_COLS * blockIdx.x + c];
      if (u >= 0 && u < first) first = u;
    }
  } else {
    first = max(0, row_lo[blockIdx.x]);
  }
  if (first >= n) return;  // (uniform: a block without a column)
  const int lo = (UNIT && row_lo) ? max(0, min(row_lo[blockIdx.x], first)) : 0;
  const int p_first = first / COV_NB, p_lo = lo / COV_NB, np = (n + COV_NB - 1) / COV_NB;
  double* __restrict__ Xw = X + (size_t)blockIdx.x * n * COV_COLS;
  if (UNIT) {
    for (int t = tid + p_lo * COV_NB * COV_COLS; t < n * COV_COLS; t += COV_THREADS)
      Xw[t] = col_unk[COV_COLS * blockIdx.x + (t % COV_COLS)] == t / COV_COLS ? 1.0 : 0.0;
    __syncthreads();
  }
  // ---- forward: L Y = E
  for (int p = p_first; p < np; p++) {
    const int k = p * COV_NB, nb = min(COV_NB, n - k), iend = min(n, k + COV_NB + bw);
    for (int t = tid; t < COV_NB * COV_NB; t += COV_THREADS) Li[t / COV_NB][t % COV_NB] = Linv[(size_t)p * COV_NB * COV_NB + t];
    for (int t = tid; t < COV_NB * COV_COLS; t += COV_THREADS) {
      const int r = t / COV_COLS;
      Bk[r][t % COV_COLS] = r < nb ? Xw[(size_t)(k + r) * COV_COLS + (t % COV_COLS)] : 0.0;
    }
    __syncthreads();
    cov_v4d acc = {0.0, 0.0, 0.0, 0.0};
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int s = 0; s < COV_NB / 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[16 * wave + l16][4 * s + kq], Bk[4 * s + kq][l16], acc, 0, 0, 0);
    }
    __syncthreads();  // B_k has been read: Y_k takes its place
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * wave + kq + 4 * q;
        Bk[r][l16] = acc[q];
        if (r < nb) Xw[(size_t)(k + r) * COV_COLS + l16] = acc[q];
      }
    }
    __syncthreads();
    for (int i0 = k + COV_NB; i0 < iend; i0 += COV_CHUNK) {
      for (int t = tid; t < COV_CHUNK * COV_NB; t += COV_THREADS) {
        const int r = t / COV_NB, c = t % COV_NB, i = i0 + r, j = k + c;
        stage[r * COV_LP + c] = (i < n && i - j <= bw) ? L[(size_t)i * ld + j] : 0.0;
      }
      __syncthreads();
      const int r0 = i0 + 16 * wave;
      if (r0 < iend) {
        cov_v4d a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < COV_NB / 4; s++)
          a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(stage[(16 * wave + l16) * COV_LP + 4 * s + kq], Bk[4 * s + kq][l16], a2, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int r = r0 + kq + 4 * q;
          if (r < iend) Xw[(size_t)r * COV_COLS + l16] -= a2[q];
        }
      }
      __syncthreads();
    }
  }
  // ---- backward: L^T X = Y
  for (int p = np - 1; p >= p_lo; p--) {
    const int k = p * COV_NB, nb = min(COV_NB, n - k), cbeg = max(p_lo * COV_NB, k - bw);
    for (int t = tid; t < COV_NB * COV_NB; t += COV_THREADS) Li[t / COV_NB][t % COV_NB] = Linv[(size_t)p * COV_NB * COV_NB + t];
    for (int t = tid; t < COV_NB * COV_COLS; t += COV_THREADS) {
      const int r = t / COV_COLS;
      Bk[r][t % COV_COLS] = r < nb ? Xw[(size_t)(k + r) * COV_COLS + (t % COV_COLS)] : 0.0;
    }
    __syncthreads();
    cov_v4d acc = {0.0, 0.0, 0.0, 0.0};
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int s = 0; s < COV_NB / 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[4 * s + kq][16 * wave + l16], Bk[4 * s + kq][l16], acc, 0, 0, 0);
    }
    __syncthreads();
    if (wave < COV_NB / 16) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * wave + kq + 4 * q;
        Bk[r][l16] = acc[q];
        if (r < nb) Xw[(size_t)(k + r) * COV_COLS + l16] = acc[q];
      }
    }
    __syncthreads();
    for (int c0 = cbeg; c0 < k; c0 += COV_CHUNK) {
      for (int t = tid; t < COV_NB * COV_CHUNK; t += COV_THREADS) {
        const int r = t / COV_CHUNK, c = t % COV_CHUNK, i = k + r, j = c0 + c;
        stage[r * COV_LQ + c] = (r < nb && j < k && i - j <= bw) ? L[(size_t)i * ld + j] : 0.0;
      }
      __syncthreads();
      const int cc0 = c0 + 16 * wave;
      if (cc0 < k) {
        cov_v4d a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < COV_NB / 4; s++)
          a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(stage[(4 * s + kq) * COV_LQ + 16 * wave + l16], Bk[4 * s + kq][l16], a2, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int r = cc0 + kq + 4 * q;
          if (r < k) Xw[(size_t)r * COV_COLS + l16] -= a2[q];
        }
      }
      __syncthreads();
    }
  }
}

// pose block of the camera at position q of Q (free index q_free[q], right-hand sides 6 q .. 6 q + 5): the diagonal
// block of X, symmetrised (X = S^-1 is symmetric up to rounding; (a + b) / 2 is the same number both ways round)
__global__ void ba_cov_pose_kernel(int n, int nQ, const int* __restrict__ q_free, const double* __restrict__ X,
                                   const int* __restrict__ ok, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * nQ || !*ok) return;
  const int q = t / 36, a = (t % 36) / 6, b = t % 6, c = q_free[q];
  out[t] = 0.5 * (X[vsl_cov_x_at(n, 6 * c + a, 6 * q + b)] + X[vsl_cov_x_at(n, 6 * c + b, 6 * q + a)]);
}

// Where the landmark kernel reads [S^-1]_{6 ci + r, 6 cj + b} (ci, cj: free indices of two cameras that observe the
// same landmark).  block(ci, cj) is evaluated once per camera pair, at(h, r, b) once per entry.
// Dense route: the unit columns X of the cameras of Q (right-hand sides 6 qpos[cj] .. + 5).
struct CovDenseInverse {
  int n;
  const int* __restrict__ qpos;
  const double* __restrict__ X;
  struct Block { int row, col; };
  __device__ __forceinline__ Block block(int ci, int cj) const { return Block{6 * ci, 6 * qpos[cj]}; }
  __device__ __forceinline__ double at(const Block& h, int r, int b) const { return X[vsl_cov_x_at(n, h.row + r, h.col + b)]; }
};
// Band route: the band array Z of the inverse (Z = its ORIGIN, storage + ld; cov_band_at of ba_cov_plan.h).  Two free
// cameras that observe one landmark are adjacent in the covisibility graph, so |ci - cj| <= half and every entry of
// the block lies inside the band bw = 6 half + 5.  Only the lower triangle is stored: block (ci, cj) with ci < cj is the
// transpose of block (cj, ci), and the diagonal block is mirrored -- either way entry (max, min).  Z is read in the
// wavefront's own layout straight from the L2 (a few reads per entry: staging it in LDS would buy nothing).
struct CovBandInverse {
  int ld;
  const double* __restrict__ Z;
  struct Block { int row, col; };
  __device__ __forceinline__ Block block(int ci, int cj) const { return Block{6 * ci, 6 * cj}; }
  __device__ __forceinline__ double at(const Block& h, int r, int b) const {
    const int i = h.row + r, j = h.col + b;
    return Z[(size_t)max(i, j) * ld + min(i, j)];
  }
};

// One wavefront per queried landmark u (its observations: u_start[u] .. u_start[u + 1] of o_cam / o_uv, ascending free
// index, fixed cameras first).  sh: 27 doubles per observation (W = F^T E, then T = W^T Z).
template <class Inverse>
__global__ __launch_bounds__(64) void ba_cov_landmark_kernel(BlArgs a, const int* __restrict__ u_lm, const int* __restrict__ u_start,
                                                             const int* __restrict__ o_cam, const double* __restrict__ o_uv,
                                                             Inverse inv, const int* __restrict__ ok, double* __restrict__ out,
                                                             int* __restrict__ degenerate) {
  extern __shared__ double sh[];
  __shared__ double M[9];
  if (!*ok) return;
  const int u = blockIdx.x, lane = threadIdx.x;
  const int o0 = u_start[u], K = u_start[u + 1] - o0;
  double* W = sh;
  double* T = sh + 18 * (size_t)K;
  const double* pw = a.points + 3 * (size_t)u_lm[u];
  double P[6] = {0, 0, 0, 0, 0, 0};  // xx xy xz yy yz zz
  for (int i = lane; i < K; i += 64) {
    BlObs o;
    bl_eval<false, true>(a, o_cam[o0 + i], pw, nullptr, o_uv + 2 * (size_t)(o0 + i), o);
    const double* E = o.E;
    P[0] += E[0] * E[0] + E[3] * E[3];
    P[1] += E[0] * E[1] + E[3] * E[4];
    P[2] += E[0] * E[2] + E[3] * E[5];
    P[3] += E[1] * E[1] + E[4] * E[4];
    P[4] += E[1] * E[2] + E[4] * E[5];
    P[5] += E[2] * E[2] + E[5] * E[5];
#pragma unroll
    for (int x = 0; x < 6; x++)
#pragma unroll
      for (int y = 0; y < 3; y++) W[18 * i + 3 * x + y] = o.fc >= 0 ? o.F[x] * E[y] + o.F[6 + x] * E[3 + y] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 6; j++) P[j] = bl_wave_sum(P[j]);
  // P = L D L^T: positive definite to working precision iff every pivot is a fair share of its diagonal entry
  const double d0 = P[0];
  const double l1 = P[1] / d0, l2 = P[2] / d0;
  const double d1 = P[3] - l1 * P[1];
  const double m = P[4] - l1 * P[2];
  const double d2 = P[5] - l2 * P[2] - (m / d1) * m;
  const double P9[9] = {P[0], P[1], P[2], P[1], P[3], P[4], P[2], P[4], P[5]};
  double Pi[9];
  const bool pd = d0 > 0.0 && d1 > COV_LM_TOL * P[3] && d2 > COV_LM_TOL * P[5] && isfinite(d0 + d1 + d2) && inv3(P9, Pi);
  if (!pd) {  // (wave-uniform: every lane holds the same P)
    if (lane < 9) out[9 * (size_t)u + lane] = __builtin_nan("");
    if (lane == 0) degenerate[u] = 1;
    return;
  }
  if (lane == 0) degenerate[u] = 0;
  __syncthreads();
  // T_i = W_i^T sum_j [S^-1]_{c(i) c(j)} W_j, j ascending
  for (int i = lane; i < K; i += 64) {
    const int ci = a.cam_free[o_cam[o0 + i]];
    double Z[18];
#pragma unroll
    for (int e = 0; e < 18; e++) Z[e] = 0.0;
    if (ci >= 0) {
      for (int j = 0; j < K; j++) {
        const int cj = a.cam_free[o_cam[o0 + j]];
        if (cj < 0) continue;
        const typename Inverse::Block h = inv.block(ci, cj);
        const double* Wj = W + 18 * j;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
          for (int b = 0; b < 6; b++) {
            const double s = inv.at(h, r, b);
#pragma unroll
            for (int y = 0; y < 3; y++) Z[3 * r + y] += s * Wj[3 * b + y];
          }
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
    for (int i = 0; i < K; i++) s += T[9 * i + lane];  // ascending c
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

// The producer side of the pose graph's _w entry points (vsl_ba_relative_pose_covariance): one wavefront per pair
// (a, b) of a bundle-adjustment problem, whose 12 x 12 joint block of S^-1 is in `joint`.  Lane 0 evaluates the pose
// graph's functor at a zero measurement with its own dual numbers (pgo_device.h) -- meas = log(T_a^-1 T_b), and the
// Jacobians of the residual, which do not depend on the measurement; a fixed camera's half of J is zero.  The lanes share
// T = Sigma J^T and M = J T as in pgo_edge_consistency_kernel (pgo_cov.hip; every sum in ascending index order), cov =
// (M + M^T) / 2.  Lane 0
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

// ------------------------------------------------------------------------------------------------ host side
// (the host plan -- CovPlan, CovBuffers -- is ba_cov_plan.h)

// One call of either entry point.  vsl_ba_covariance plans before the set-up (its S is dense, its free cameras are
// numbered by ascending id); vsl_global_ba_covariance plans inside it (plan_extra below), once the layout of S and the
// band order are known.
struct CovCall {
  vsl_ctx* ctx;
  const char* name;
  const vsl_ba_problem* prob;
  const int32_t* cams;
  int n_cam_q;
  const int32_t* lms;
  int n_lm_q;
  bool global;
  bool band = false;  // the route taken: S and the band of its inverse in linear band storage
  CovPlan P;
  CovBuffers B;
};

int cov_check_kmax(const CovCall& c) {
  if (c.P.kmax > COV_KMAX)
    return vsl_fail(c.ctx, VSL_ERR_INVALID, "%s: a queried landmark has %d observations (at most %d)", c.name, c.P.kmax, COV_KMAX);
  return VSL_OK;
}

void cov_size_buffers(CovCall& c, int bw) {
  const int n = 6 * c.P.nfree;
  c.B = c.band ? cov_band_buffers(c.P, n, bw) : cov_buffers(c.P, n, (6 * c.P.nQ + COV_COLS - 1) / COV_COLS);
}

// BaCaller::plan_extra of vsl_global_ba_covariance
int cov_plan_extra(void* self, const BaHostPlan& hp, size_t* extra_bytes) {
  CovCall& c = *static_cast<CovCall*>(self);
  c.band = hp.layout.banded;
  // dense: hp.cam_free is the ascending numbering, the plan is vsl_ba_covariance's.  Band: hp.cam_free is the band order.
  c.P = cov_plan(c.prob, hp.cam_free, hp.nfree, !c.band, c.cams, c.n_cam_q, c.lms, c.n_lm_q);
  const int rc = cov_check_kmax(c);
  if (rc) return rc;
  cov_size_buffers(c, hp.layout.bw);
  *extra_bytes = c.B.total;
  return VSL_OK;
}

// everything behind the validation; host_in / host_out outlive the stream work (the caller synchronises on an error)
int cov_run(CovCall& c, const vsl_ba_options* opt, BaState& st, std::vector<char>& host_in, std::vector<char>& host_out) {
  vsl_ctx* ctx = c.ctx;
  BaCaller caller{c.global ? BaUse::GLOBAL_COVARIANCE : BaUse::COVARIANCE};
  if (c.global) {
    caller.plan_extra = cov_plan_extra;
    caller.plan_extra_self = &c;
  } else {
    cov_size_buffers(c, 0);
    caller.extra_bytes = c.B.total;
  }
  int rc;
  if ((rc = ba_setup(ctx, c.prob, opt, st, caller))) return rc;
  const CovPlan& P = c.P;
  const CovBuffers& B = c.B;
  const int n = 6 * P.nfree, m = 6 * P.nQ, nblk = (m + COV_COLS - 1) / COV_COLS;
  const BaDims& D = st.D;
  if (D.nfree != P.nfree || st.banded != c.band) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: the set-up and the plan disagree", c.name);
  char* dev = st.extra;
  host_in.assign(B.in_bytes, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(host_in.data() + off, src, bytes);
  };
  const int one = 1;
  put(B.off_ok, &one, sizeof(int));
  if (!c.band) {
    std::vector<int> col_unk((size_t)nblk * COV_COLS, -1);
    for (int j = 0; j < m; j++) col_unk[j] = 6 * P.q_free[j / 6] + j % 6;
    put(B.off_col_unk, col_unk.data(), sizeof(int) * col_unk.size());
    put(B.off_qpos, P.qpos.data(), sizeof(int) * P.qpos.size());
  }
  put(B.off_q_free, P.q_free.data(), sizeof(int) * P.q_free.size());
  put(B.off_u_lm, P.u_lm.data(), sizeof(int) * P.u_lm.size());
  put(B.off_u_start, P.u_start.data(), sizeof(int) * P.u_start.size());
  put(B.off_o_cam, P.o_cam.data(), sizeof(int) * P.o_cam.size());
  put(B.off_o_uv, P.o_uv.data(), sizeof(double) * P.o_uv.size());
  VSL_HIP(ctx, hipMemcpyAsync(dev, host_in.data(), B.in_bytes, hipMemcpyHostToDevice, ctx->stream));
  int* ok = (int*)(dev + B.off_ok);
  double* X = (double*)(dev + B.off_X);
  double* Sdiag = (double*)(dev + B.off_Sdiag);
  double* Zs = (double*)(dev + B.off_Z);  // band route: the storage base of the band of S^-1
  if (c.band ? P.need_inverse : P.nQ > 0) {
    // S as vsl_ba_linearize forms it, in the layout of the set-up
    if ((rc = ba_linearize(ctx, st, st.sb, false))) return rc;
    if ((rc = ba_columns(ctx, st, st.sb))) return rc;
    if ((rc = ba_schur(ctx, st, st.sb, false, 1.0, 0, D.L, false, false))) return rc;
    VslStage s(ctx, VSL_STAGE_BA_SOLVE);
    // dense: the factor and the columns of S^-1; band: the band of S^-1 (no columns: a pose block lies inside it)
    const int ld = c.band ? st.ldS : 0;
    const VslCovInverse inv{n, ld, st.bw, st.S, c.band ? Zs : nullptr, c.band ? nullptr : (double*)(dev + B.off_Linv), Sdiag,
                            c.band ? nullptr : (const int*)(dev + B.off_col_unk), nullptr, c.band ? 0 : nblk, X, ok};
    if ((rc = vsl_cov_inverse_dev(ctx, inv))) return rc;
    if ((rc = vsl_cov_diag_blocks_dev(ctx, n, P.nQ, (const int*)(dev + B.off_q_free), ld, Zs, X, ok,
                                      (double*)(dev + B.out_off + B.off_pose))))
      return rc;
  }
  if (P.nu > 0) {
    BlArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D;
    a.poses = st.poses;
    a.points = st.points;
    a.intr = st.intr;
    a.cam_intr = st.cam_intr;
    a.cam_free = st.cam_free;
    const size_t lds = sizeof(double) * 27 * (size_t)std::max(P.kmax, 1);
    if (c.band)
      hipLaunchKernelGGL(ba_cov_landmark_kernel<CovBandInverse>, dim3(P.nu), dim3(64), lds, ctx->stream, a,
                         (const int*)(dev + B.off_u_lm), (const int*)(dev + B.off_u_start), (const int*)(dev + B.off_o_cam),
                         (const double*)(dev + B.off_o_uv), CovBandInverse{st.ldS, Zs + st.ldS}, ok,
                         (double*)(dev + B.out_off + B.off_point), (int*)(dev + B.out_off + B.off_deg));
    else
      hipLaunchKernelGGL(ba_cov_landmark_kernel<CovDenseInverse>, dim3(P.nu), dim3(64), lds, ctx->stream, a,
                         (const int*)(dev + B.off_u_lm), (const int*)(dev + B.off_u_start), (const int*)(dev + B.off_o_cam),
                         (const double*)(dev + B.off_o_uv), CovDenseInverse{n, (const int*)(dev + B.off_qpos), X}, ok,
                         (double*)(dev + B.out_off + B.off_point), (int*)(dev + B.out_off + B.off_deg));
    VSL_CHECK_LAUNCH(ctx);
  }
  host_out.assign(B.out_bytes + sizeof(int), 0);
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data(), dev + B.out_off, B.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(host_out.data() + B.out_bytes, ok, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int ok_host;
  memcpy(&ok_host, host_out.data() + B.out_bytes, sizeof(int));
  if (!ok_host) return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: the reduced camera system is not positive definite", c.name);
  return VSL_OK;
}

// both entry points: the argument rules, the run, the query -> output maps.  storage: null for vsl_ba_covariance
int cov_call(CovCall& c, const vsl_ba_options* opt, double* cov_pose, double* cov_point, int* n_degenerate, int* storage) {
  vsl_ctx* ctx = c.ctx;
  const vsl_ba_problem* prob = c.prob;
  const int32_t *cams = c.cams, *lms = c.lms;
  const int n_cam_q = c.n_cam_q, n_lm_q = c.n_lm_q;
  int rc = ba_validate(ctx, prob);  // an empty problem (n_lms = 0, n_obs = 0) ends here
  if (rc) return rc;
  if (!opt || n_cam_q < 0 || n_lm_q < 0 || (n_cam_q > 0 && (!cams || !cov_pose)) || (n_lm_q > 0 && (!lms || !cov_point)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null argument or negative count", c.name);
  for (int q = 0; q < n_cam_q; q++) {
    if (cams[q] < 0 || cams[q] >= prob->n_cams) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: camera %d out of range", c.name, cams[q]);
    if (prob->cam_fixed[cams[q]]) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: camera %d is fixed", c.name, cams[q]);
  }
  for (int q = 0; q < n_lm_q; q++)
    if (lms[q] < 0 || lms[q] >= prob->n_lms) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: landmark %d out of range", c.name, lms[q]);
  if (n_degenerate) *n_degenerate = 0;
  if (n_cam_q == 0 && n_lm_q == 0) {
    // nothing is launched; the route is still the problem's own (decided on the host)
    if (storage) {
      bool banded = false;
      if ((rc = ba_layout_of(ctx, prob, BaCaller{BaUse::GLOBAL_COVARIANCE}, &banded))) return rc;
      *storage = banded ? 1 : 0;
    }
    return VSL_OK;
  }
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  if (!c.global) {
    try {
      c.P = cov_plan(prob, cams, n_cam_q, lms, n_lm_q);
    } catch (const std::bad_alloc&) {
      return vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    if ((rc = cov_check_kmax(c))) return rc;
  }
  std::vector<char> host_in, host_out;  // read / written by copies on the stream: they outlive the synchronisation below
  {
    BaState st;  // holds the loan of the context's arena
    try {
      rc = cov_run(c, opt, st, host_in, host_out);
    } catch (const std::bad_alloc&) {
      rc = vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    // an error return may leave kernels and copies queued that use the arena and the host buffers: drain the stream
    // before the loan ends (a later solve on this context gets the same block)
    if (rc) (void)hipStreamSynchronize(ctx->stream);
  }
  if (rc) return rc;
  const CovPlan& P = c.P;
  const double* pose = (const double*)(host_out.data() + c.B.off_pose);
  const double* point = (const double*)(host_out.data() + c.B.off_point);
  const int* deg = (const int*)(host_out.data() + c.B.off_deg);
  for (int q = 0; q < n_cam_q; q++) memcpy(cov_pose + 36 * (size_t)q, pose + 36 * (size_t)P.cam_q2Q[q], 36 * sizeof(double));
  int nd = 0;
  for (int q = 0; q < n_lm_q; q++) {
    memcpy(cov_point + 9 * (size_t)q, point + 9 * (size_t)P.lm_q2u[q], 9 * sizeof(double));
    nd += deg[P.lm_q2u[q]] ? 1 : 0;
  }
  if (n_degenerate) *n_degenerate = nd;
  if (storage) *storage = c.band ? 1 : 0;
  return VSL_OK;
}

// ------------------------------------------------------------------ relative-pose covariances of camera pairs
// vsl_ba_relative_pose_covariance / vsl_global_ba_relative_pose_covariance: the chains of the file header up to the
// factor (dense) or the band of S^-1 (band), then
//   dense  ba_cov_solve_kernel for the six unit columns of every distinct queried free camera
//   band   cov_band_solve_kernel for the PGC_SOLVE pairs (the camera with the larger band position), fed by the inverted
//          diagonal blocks the selected inversion left in its scratch
//   ba_pair_blocks_kernel   the 12 x 12 joint blocks
//   ba_relpose_kernel       (above; the functor's own device code is pgo_device.h) meas, cov = J Sigma J^T, info = cov^-1
// all on the context's stream inside one arena loan, one synchronisation at the end.
struct RelCall {
  vsl_ctx* ctx;
  const char* name;
  const vsl_ba_problem* prob;
  const int32_t *a, *b;
  int n_pairs;
  bool global;
  bool band = false;
  BaPairPlan P;
};

// BaCaller::plan_extra of vsl_global_ba_relative_pose_covariance: hp.cam_free is the numbering of S (the band order on
// the band route, ascending camera id on the dense one)
int rel_plan_extra(void* self, const BaHostPlan& hp, size_t* extra_bytes) {
  RelCall& c = *static_cast<RelCall*>(self);
  c.band = hp.layout.banded;
  c.P = bpp_plan(hp.cam_free, hp.nfree, c.band, hp.layout.bw, c.ctx->ba_cov_no_band_read, c.a, c.b, c.n_pairs);
  *extra_bytes = c.P.total;
  return VSL_OK;
}

int rel_run(RelCall& c, const vsl_ba_options* opt, BaState& st, std::vector<char>& host_in, std::vector<char>& host_out) {
  vsl_ctx* ctx = c.ctx;
  BaCaller caller{c.global ? BaUse::GLOBAL_COVARIANCE : BaUse::COVARIANCE};
  if (c.global) {
    caller.plan_extra = rel_plan_extra;
    caller.plan_extra_self = &c;
  } else {
    caller.extra_bytes = c.P.total;
  }
  int rc;
  if ((rc = ba_setup(ctx, c.prob, opt, st, caller))) return rc;
  const BaPairPlan& P = c.P;
  const PgcPlan& G = P.G;
  const int n = G.n, np = c.n_pairs;
  if (st.D.nfree != G.nf || st.banded != c.band || (c.band && st.bw != G.bw))
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: the set-up and the plan disagree", c.name);
  char* dev = st.extra;
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
  const int* col_unk = (const int*)(dev + P.off_col_unk);
  double* X = (double*)(dev + P.off_X);
  double* Sdiag = (double*)(dev + P.off_Sdiag);
  double* Zs = (double*)(dev + P.off_Z);
  double* joint = (double*)(dev + P.out_off + P.off_joint);
  // S as vsl_ba_linearize forms it, in the layout of the set-up
  if ((rc = ba_linearize(ctx, st, st.sb, false))) return rc;
  if ((rc = ba_columns(ctx, st, st.sb))) return rc;
  if ((rc = ba_schur(ctx, st, st.sb, false, 1.0, 0, st.D.L, false, false))) return rc;
  {
    VslStage s(ctx, VSL_STAGE_BA_SOLVE);
    const VslCovInverse inv{n, c.band ? st.ldS : 0, st.bw, st.S, c.band ? Zs : nullptr, c.band ? nullptr : (double*)(dev + P.off_Linv),
                            Sdiag, col_unk, (const int*)(dev + P.off_row_lo), G.nblk, X, ok};
    if ((rc = vsl_cov_inverse_dev(ctx, inv))) return rc;
    if ((rc = vsl_cov_pair_blocks_dev(ctx, n, np, pairs, c.band ? 1 : 0, Zs, st.ldS, X, ok, joint))) return rc;
    // meas, cov = J Sigma J^T and info = cov^-1 of every pair, with the pose graph's functor (pgo_device.h)
    if ((rc = vsl_ba_relpose_dev(ctx, np, st.poses, pairs, joint, ok, (double*)(dev + P.out_off + P.off_meas),
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
  if (!ok_host) return vsl_fail(ctx, VSL_ERR_NUMERIC, "%s: the reduced camera system is not positive definite", c.name);
  return VSL_OK;
}

// both entry points.  storage: null for vsl_ba_relative_pose_covariance
int rel_call(RelCall& c, const vsl_ba_options* opt, double* joint, double* meas, double* cov, double* info, int* n_singular,
             int* storage) {
  vsl_ctx* ctx = c.ctx;
  const vsl_ba_problem* prob = c.prob;
  int rc = ba_validate(ctx, prob);  // an empty problem (n_lms = 0, n_obs = 0) ends here
  if (rc) return rc;
  if (!opt || c.n_pairs < 0 || (c.n_pairs > 0 && (!c.a || !c.b)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null argument or negative count", c.name);
  int bad = 0;
  switch (bpp_check_pairs(prob->n_cams, prob->cam_fixed, c.a, c.b, c.n_pairs, &bad)) {
    case PGC_PAIR_RANGE: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d (%d, %d): camera out of range", c.name, bad, c.a[bad], c.b[bad]);
    case PGC_PAIR_SAME: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d names camera %d twice", c.name, bad, c.a[bad]);
    case PGC_PAIR_BOTH_FIXED: return vsl_fail(ctx, VSL_ERR_INVALID, "%s: pair %d (%d, %d): both cameras are fixed", c.name, bad, c.a[bad], c.b[bad]);
    default: break;
  }
  if (n_singular) *n_singular = 0;
  if (c.n_pairs == 0 || (!joint && !meas && !cov && !info)) {
    // nothing is launched; the route is still the problem's own (decided on the host)
    if (storage) {
      bool banded = false;
      if ((rc = ba_layout_of(ctx, prob, BaCaller{BaUse::GLOBAL_COVARIANCE}, &banded))) return rc;
      *storage = banded ? 1 : 0;
    }
    return VSL_OK;
  }
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<char> host_in, host_out;  // read / written by copies on the stream: they outlive the synchronisation below
  {
    BaState st;  // holds the loan of the context's arena
    try {
      if (!c.global) {
        // dense S, free cameras numbered by ascending camera id (vsl_ba_linearize's numbering)
        std::vector<int> cam_free(prob->n_cams, -1);
        int nfree = 0;
        for (int i = 0; i < prob->n_cams; i++)
          if (!prob->cam_fixed[i]) cam_free[i] = nfree++;
        c.P = bpp_plan(cam_free, nfree, false, 0, false, c.a, c.b, c.n_pairs);
      }
      rc = rel_run(c, opt, st, host_in, host_out);
    } catch (const std::bad_alloc&) {
      rc = vsl_fail(ctx, VSL_ERR_NOMEM, "out of host memory");
    }
    // an error return may leave kernels and copies queued that use the arena and the host buffers: drain the stream
    // before the loan ends (a later solve on this context gets the same block)
    if (rc) (void)hipStreamSynchronize(ctx->stream);
  }
  if (rc) return rc;
  const BaPairPlan& P = c.P;
  const size_t np = (size_t)c.n_pairs;
  if (joint) memcpy(joint, host_out.data() + P.off_joint, sizeof(double) * 144 * np);
  if (meas) memcpy(meas, host_out.data() + P.off_meas, sizeof(double) * 6 * np);
  if (cov) memcpy(cov, host_out.data() + P.off_cov, sizeof(double) * 36 * np);
  if (info) memcpy(info, host_out.data() + P.off_info, sizeof(double) * 36 * np);
  const int* sing = (const int*)(host_out.data() + P.off_sing);
  int ns = 0;
  for (size_t q = 0; q < np; q++) ns += sing[q] ? 1 : 0;
  if (n_singular) *n_singular = ns;
  if (storage) *storage = c.band ? 1 : 0;
  return VSL_OK;
}

}  // namespace

int vsl_cov_unit_columns_dev(vsl_ctx* ctx, int n, const double* L, const double* Linv, const double* Sdiag, const int* col_unk,
                             int nblk, double* X, int* ok_dev) {
  if (nblk <= 0) return VSL_OK;
  hipLaunchKernelGGL(ba_cov_solve_kernel, dim3(nblk), dim3(COV_THREADS), 0, ctx->stream, n, L, Linv, Sdiag, col_unk, X, ok_dev);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_cov_band_unit_columns_dev(vsl_ctx* ctx, int n, const double* L, int ld, int bw, const double* Linv, const int* col_unk,
                                  const int* row_lo, int nblk, double* X, const int* ok_dev) {
  if (nblk <= 0 || n <= 0) return VSL_OK;
  if (bw < 0 || ld != bw + COV_NB) return vsl_fail(ctx, VSL_ERR_INVALID, "band unit columns: half bandwidth %d, leading dimension %d", bw, ld);
  hipLaunchKernelGGL(cov_band_solve_kernel<true>, dim3(nblk), dim3(COV_THREADS), 0, ctx->stream, n, L + ld, ld, bw, Linv, col_unk, row_lo,
                     X, ok_dev);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_band_rhs_solve_dev(vsl_ctx* ctx, int n, const double* L, int ld, int bw, const double* Linv, const int* row_first, int nblk,
                           double* X, const int* ok_dev) {
  if (nblk <= 0 || n <= 0) return VSL_OK;
  if (bw < 0 || ld != bw + COV_NB || !row_first) return vsl_fail(ctx, VSL_ERR_INVALID, "band solve: half bandwidth %d, leading dimension %d", bw, ld);
  hipLaunchKernelGGL(cov_band_solve_kernel<false>, dim3(nblk), dim3(COV_THREADS), 0, ctx->stream, n, L + ld, ld, bw, Linv,
                     (const int*)nullptr, row_first, X, ok_dev);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_cov_band_pivot_dev(vsl_ctx* ctx, int n, const double* L, int ld, const double* Sdiag, int* ok_dev) {
  if (n <= 0) return VSL_OK;
  hipLaunchKernelGGL(cov_band_pivot_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, L, ld, Sdiag, ok_dev);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_cov_diag_dev(vsl_ctx* ctx, int n, const double* S, int ld, double* diag) {
  if (n <= 0) return VSL_OK;
  hipLaunchKernelGGL(ba_cov_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, S, ld, diag);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_cov_inverse_dev(vsl_ctx* ctx, const VslCovInverse& a) {
  int rc;
  if ((rc = vsl_cov_diag_dev(ctx, a.n, a.S, a.ld, a.diag))) return rc;
  if (a.ld == 0) {
    if ((rc = vsl_chol_factor_dev(ctx, a.S, a.n, a.ok, a.Linv))) return rc;
    return vsl_cov_unit_columns_dev(ctx, a.n, a.S, a.Linv, a.diag, a.col_unk, a.nblk, a.X, a.ok);
  }
  // the band of S^-1 by selected inversion (S <- L in place), then the pivot test on the factor
  if ((rc = vsl_chol_selinv_band_dev(ctx, a.S + a.ld, a.Z + a.ld, a.n, a.ld, a.bw, a.ok))) return rc;
  if ((rc = vsl_cov_band_pivot_dev(ctx, a.n, a.S, a.ld, a.diag, a.ok))) return rc;
  if (a.nblk <= 0) return VSL_OK;
  return vsl_cov_band_unit_columns_dev(ctx, a.n, a.S, a.ld, a.bw, vsl_chol_selinv_linv_dev(ctx, a.n, a.bw), a.col_unk, a.row_lo,
                                       a.nblk, a.X, a.ok);
}

int vsl_cov_diag_blocks_dev(vsl_ctx* ctx, int n, int nQ, const int* q_free, int ld, const double* Z, const double* X,
                            const int* ok_dev, double* out) {
  if (nQ <= 0) return VSL_OK;
  if (ld > 0)
    hipLaunchKernelGGL(cov_band_pose_kernel, dim3((36 * nQ + 255) / 256), dim3(256), 0, ctx->stream, nQ, q_free, Z, ld, ok_dev, out);
  else
    hipLaunchKernelGGL(ba_cov_pose_kernel, dim3((36 * nQ + 255) / 256), dim3(256), 0, ctx->stream, n, nQ, q_free, X, ok_dev, out);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_cov_pair_blocks_dev(vsl_ctx* ctx, int n, int n_pairs, const PgcPairDev* pairs, int band, const double* Z, int ld,
                            const double* X, const int* ok_dev, double* out) {
  if (n_pairs <= 0) return VSL_OK;
  hipLaunchKernelGGL(ba_pair_blocks_kernel, dim3((144 * n_pairs + 255) / 256), dim3(256), 0, ctx->stream, n, n_pairs, pairs, band, Z,
                     ld, X, ok_dev, out);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

int vsl_ba_relpose_dev(vsl_ctx* ctx, int n_pairs, const double* poses, const PgcPairDev* pairs, const double* joint,
                       const int* ok_dev, double* meas, double* cov, double* info, int* singular) {
  if (n_pairs <= 0) return VSL_OK;
  hipLaunchKernelGGL(ba_relpose_kernel, dim3(n_pairs), dim3(64), 0, ctx->stream, n_pairs, poses, pairs, joint, ok_dev, meas, cov, info,
                     singular);
  VSL_CHECK_LAUNCH(ctx);
  return VSL_OK;
}

extern "C" int vsl_ba_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, const int32_t* cams,
                                 int n_cam_q, double* cov_pose, const int32_t* lms, int n_lm_q, double* cov_point,
                                 int* n_degenerate) {
  if (!ctx) return VSL_ERR_INVALID;
  CovCall c{ctx, "vsl_ba_covariance", prob, cams, n_cam_q, lms, n_lm_q, false};
  return cov_call(c, opt, cov_pose, cov_point, n_degenerate, nullptr);
}

extern "C" int vsl_global_ba_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, const int32_t* cams,
                                        int n_cam_q, double* cov_pose, const int32_t* lms, int n_lm_q, double* cov_point,
                                        int* n_degenerate, int* storage) {
  if (!ctx) return VSL_ERR_INVALID;
  CovCall c{ctx, "vsl_global_ba_covariance", prob, cams, n_cam_q, lms, n_lm_q, true};
  return cov_call(c, opt, cov_pose, cov_point, n_degenerate, storage);
}

extern "C" int vsl_ba_relative_pose_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt,
                                               const int32_t* pair_a, const int32_t* pair_b, int n_pairs, double* joint, double* meas,
                                               double* cov, double* info, int* n_singular) {
  if (!ctx) return VSL_ERR_INVALID;
  RelCall c{ctx, "vsl_ba_relative_pose_covariance", prob, pair_a, pair_b, n_pairs, false};
  return rel_call(c, opt, joint, meas, cov, info, n_singular, nullptr);
}

extern "C" int vsl_global_ba_relative_pose_covariance(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt,
                                                      const int32_t* pair_a, const int32_t* pair_b, int n_pairs, double* joint,
                                                      double* meas, double* cov, double* info, int* n_singular, int* storage) {
  if (!ctx) return VSL_ERR_INVALID;
  RelCall c{ctx, "vsl_global_ba_relative_pose_covariance", prob, pair_a, pair_b, n_pairs, true};
  return rel_call(c, opt, joint, meas, cov, info, n_singular, storage);
}
