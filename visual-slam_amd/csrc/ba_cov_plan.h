// ba_cov_plan.h -- the host half of the marginal covariances of a bundle-adjustment problem (ba_cov.hip:
// vsl_ba_covariance and vsl_global_ba_covariance): everything derived from the problem and the query before the first
// byte goes to the device.  Plain C++, no HIP, no vsl_ctx: tests/cpp/ba_cov_plan_test.cpp drives it under g++.
//   cov_plan           unique landmarks, their observation lists in ascending free index, query -> output maps
//   cov_buffers        the dense route's share of the arena (unit columns X)
//   cov_band_at        the slot of entry (i, j) of the band of S^-1
//   cov_band_buffers   the band route's share of the arena (the second band array Z)
// Allocation failures leave as std::bad_alloc.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/vslam_hip.h"
#include "chol_plan.h"

#define COV_NB VSL_CHOL_NB  // panel width of the solve = the factorisation's (its inverted diagonal blocks are reused)
#define COV_COLS 16         // right-hand sides of a workgroup: one matrix-instruction tile

inline size_t cov_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// What the host derives from the query: Q, the unique landmarks and their observation lists
struct CovPlan {
  int nfree = 0, nQ = 0, nu = 0, n_o = 0, kmax = 0;
  bool need_inverse = false;          // a camera is queried, or a queried landmark is seen by a free camera
  std::vector<int> cam_free;          // camera -> free index or -1 (the numbering of S: ascending camera id, or the band order)
  std::vector<int> q_free, qpos;      // Q in ascending free index, and free index -> position in Q or -1
  std::vector<int> cam_q2Q, lm_q2u;   // query entry -> position in Q / unique landmark
  std::vector<int> u_lm, u_start, o_cam;
  std::vector<double> o_uv;
};

// cam_free: the free-camera numbering of the reduced system the caller reads from (nfree free cameras).
// Q = the queried cameras; with lm_cams_in_Q also every free camera that observes a queried landmark (the dense route
// solves one unit column per unknown of Q; the band route reads every block it needs from the band of the inverse).
inline CovPlan cov_plan(const vsl_ba_problem* p, const std::vector<int>& cam_free, int nfree, bool lm_cams_in_Q, const int32_t* cams,
                        int n_cam_q, const int32_t* lms, int n_lm_q) {
  CovPlan P;
  P.cam_free = cam_free;
  P.nfree = nfree;
  std::vector<int> lm_slot(p->n_lms, -1);
  P.lm_q2u.resize(n_lm_q);
  for (int q = 0; q < n_lm_q; q++) {
    int& s = lm_slot[lms[q]];
    if (s < 0) {
      s = (int)P.u_lm.size();
      P.u_lm.push_back(lms[q]);
    }
    P.lm_q2u[q] = s;
  }
  P.nu = (int)P.u_lm.size();
  P.u_start.assign((size_t)P.nu + 1, 0);
  if (P.nu > 0)
    for (int i = 0; i < p->n_obs; i++) {
      const int s = lm_slot[p->obs_lm[i]];
      if (s >= 0) P.u_start[s + 1]++;
    }
  for (int u = 0; u < P.nu; u++) {
    P.kmax = std::max(P.kmax, P.u_start[u + 1]);
    P.u_start[u + 1] += P.u_start[u];
  }
  P.n_o = P.u_start[P.nu];
  std::vector<int> o_idx(P.n_o), fill(P.u_start.begin(), P.u_start.end() - 1);
  if (P.nu > 0)
    for (int i = 0; i < p->n_obs; i++) {
      const int s = lm_slot[p->obs_lm[i]];
      if (s >= 0) o_idx[fill[s]++] = i;
    }
  std::vector<char> inQ(P.nfree, 0);
  for (int q = 0; q < n_cam_q; q++) inQ[P.cam_free[cams[q]]] = 1;
  P.need_inverse = n_cam_q > 0;
  P.o_cam.resize(P.n_o);
  P.o_uv.resize(2 * (size_t)P.n_o);
  for (int u = 0; u < P.nu; u++) {
    // ascending free index (fixed cameras, -1, first), observation order within a camera
    std::stable_sort(o_idx.begin() + P.u_start[u], o_idx.begin() + P.u_start[u + 1],
                     [&](int x, int y) { return P.cam_free[p->obs_cam[x]] < P.cam_free[p->obs_cam[y]]; });
    for (int k = P.u_start[u]; k < P.u_start[u + 1]; k++) {
      const int i = o_idx[k], fc = P.cam_free[p->obs_cam[i]];
      P.o_cam[k] = p->obs_cam[i];
      P.o_uv[2 * (size_t)k] = p->obs_uv[2 * (size_t)i];
      P.o_uv[2 * (size_t)k + 1] = p->obs_uv[2 * (size_t)i + 1];
      if (fc >= 0) {
        P.need_inverse = true;
        if (lm_cams_in_Q) inQ[fc] = 1;
      }
    }
  }
  P.qpos.assign(P.nfree, -1);
  for (int c = 0; c < P.nfree; c++)
    if (inQ[c]) {
      P.qpos[c] = (int)P.q_free.size();
      P.q_free.push_back(c);
    }
  P.nQ = (int)P.q_free.size();
  P.cam_q2Q.resize(n_cam_q);
  for (int q = 0; q < n_cam_q; q++) P.cam_q2Q[q] = P.qpos[P.cam_free[cams[q]]];
  return P;
}

// the dense route of vsl_ba_covariance: free cameras numbered by ascending camera id (vsl_ba_linearize's numbering)
inline CovPlan cov_plan(const vsl_ba_problem* p, const int32_t* cams, int n_cam_q, const int32_t* lms, int n_lm_q) {
  std::vector<int> cam_free(p->n_cams, -1);
  int nfree = 0;
  for (int c = 0; c < p->n_cams; c++)
    if (!p->cam_fixed[c]) cam_free[c] = nfree++;
  return cov_plan(p, cam_free, nfree, true, cams, n_cam_q, lms, n_lm_q);
}

// the caller's share of the arena (BaCommon::extra): [inputs, uploaded in one copy | work | outputs, one copy back]
struct CovBuffers {
  size_t in_bytes = 0, out_off = 0, out_bytes = 0, total = 0;
  size_t off_ok = 0, off_col_unk = 0, off_q_free = 0, off_qpos = 0, off_u_lm = 0, off_u_start = 0, off_o_cam = 0, off_o_uv = 0;  // inputs
  size_t off_Linv = 0, off_Sdiag = 0, off_X = 0;  // work: dense route
  size_t off_Z = 0;                               // work: band route (the STORAGE base of the band array; its origin is + ld doubles)
  size_t off_pose = 0, off_point = 0, off_deg = 0;  // outputs (relative to out_off)
};

// dense route: n unknowns, nblk workgroups of COV_COLS unit columns
inline CovBuffers cov_buffers(const CovPlan& P, int n, int nblk) {
  CovBuffers B;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += cov_pad(bytes);
    return o;
  };
  B.off_ok = take(sizeof(int));
  B.off_col_unk = take(sizeof(int) * (size_t)nblk * COV_COLS);
  B.off_q_free = take(sizeof(int) * (size_t)P.nQ);
  B.off_qpos = take(sizeof(int) * (size_t)P.nfree);
  B.off_u_lm = take(sizeof(int) * (size_t)P.nu);
  B.off_u_start = take(sizeof(int) * ((size_t)P.nu + 1));
  B.off_o_cam = take(sizeof(int) * (size_t)P.n_o);
  B.off_o_uv = take(sizeof(double) * 2 * (size_t)P.n_o);
  B.in_bytes = at;
  B.off_Linv = take(sizeof(double) * (size_t)((n + COV_NB - 1) / COV_NB) * COV_NB * COV_NB);
  B.off_Sdiag = take(sizeof(double) * (size_t)n);
  B.off_X = take(sizeof(double) * (size_t)nblk * n * COV_COLS);
  B.out_off = at;
  B.off_pose = take(sizeof(double) * 36 * (size_t)P.nQ) - B.out_off;
  B.off_point = take(sizeof(double) * 9 * (size_t)P.nu) - B.out_off;
  B.off_deg = take(sizeof(int) * (size_t)P.nu) - B.out_off;
  B.out_bytes = at - B.out_off;
  B.total = at;
  return B;
}

// ---- band route.  Z is a band array of the layout of S (chol.hip "BAND FORM"): n rows of ld + 1 slots, ld = bw +
// VSL_CHOL_NB, the diagonal in the last slot of its row; only the lower triangle of the inverse is stored.
// Slot of entry (i, j), |i - j| <= bw, relative to the ORIGIN of the array (storage base + ld doubles): entry (i, j)
// and its mirror (j, i) are one slot.
inline size_t cov_band_at(int ld, int i, int j) { return (size_t)std::max(i, j) * ld + std::min(i, j); }

// is the whole 6 x 6 block (ci, cj) inside the band: max |i - j| = 6 |ci - cj| + 5
inline bool cov_band_holds_block(int bw, int ci, int cj) { return 6 * std::abs(ci - cj) + 5 <= bw; }

inline CovBuffers cov_band_buffers(const CovPlan& P, int n, int bw) {
  CovBuffers B;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += cov_pad(bytes);
    return o;
  };
  B.off_ok = take(sizeof(int));
  B.off_q_free = take(sizeof(int) * (size_t)P.nQ);
  B.off_u_lm = take(sizeof(int) * (size_t)P.nu);
  B.off_u_start = take(sizeof(int) * ((size_t)P.nu + 1));
  B.off_o_cam = take(sizeof(int) * (size_t)P.n_o);
  B.off_o_uv = take(sizeof(double) * 2 * (size_t)P.n_o);
  B.in_bytes = at;
  B.off_Sdiag = take(sizeof(double) * (size_t)n);
  B.off_Z = take(sizeof(double) * chol_selinv_plan(n, bw, false).z_elems);
  B.out_off = at;
  B.off_pose = take(sizeof(double) * 36 * (size_t)P.nQ) - B.out_off;
  B.off_point = take(sizeof(double) * 9 * (size_t)P.nu) - B.out_off;
  B.off_deg = take(sizeof(int) * (size_t)P.nu) - B.out_off;
  B.out_bytes = at - B.out_off;
  B.total = at;
  return B;
}
