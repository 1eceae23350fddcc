// ba_rig_cov_plan.h -- the host half of the covariances of a RIG-constrained bundle adjustment (ba_rig.hip "COVARIANCES":
// vsl_ba_rig_covariance, vsl_ba_rig_relative_pose_covariance): everything derived from the rig plan (ba_rig_plan.h) and
// the query before the first byte goes to the device.  Plain C++, no HIP, no vsl_ctx:
// tests/cpp/ba_rig_cov_plan_test.cpp drives it under g++.
//   rcp_plan        the argument rules of a marginal query; the union Q of free bodies whose six unit columns of S^-1 are
//                   solved (queried bodies, bodies of queried cameras, every free body with a group at a queried
//                   landmark), in ascending free-body slot; slot -> position in Q; one ITEM per pose query (position in
//                   Q, extrinsic or none); the unique queried landmarks; the call's share of the arena
//   rcp_groups      the group list of a landmark: the groups lm_grp[l] .. lm_grp[l + 1] of the rig plan ARE that list, in
//                   ascending free-body slot, each with its adjacent observation range [grp_begin, grp_end) -- a landmark
//                   seen by both cameras of a body is ONE group of two observations.  Nothing is copied: the kernel
//                   reads the arrays the rig solve uploads.
//   rcp_pair_plan   a pair query: bpp_check_pairs / bpp_plan of ba_pair_plan.h, unchanged, on the bodies' fixed mask
//                   and the free-body numbering (bodies stand in place of cameras)
// Duplicates in a query are allowed (each entry is answered on its own from the same columns: duplicate bits); counts
// may be zero.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ba_pair_plan.h"
#include "ba_rig_plan.h"

#define RCP_GMAX 256  // groups of a queried landmark (27 doubles of LDS each)

enum RigCovPlanStatus {
  RCP_OK = 0,
  RCP_ARGUMENT,    // a negative count, or a null list with a positive count
  RCP_BODY_RANGE,  // a queried body out of range
  RCP_BODY_FIXED,  // a queried body is fixed
  RCP_CAM_RANGE,   // a queried camera out of range
  RCP_CAM_FIXED,   // a queried camera's body is fixed
  RCP_LM_RANGE,    // a queried landmark out of range
  RCP_LM_GROUPS    // a queried landmark has more than RCP_GMAX groups
};

inline const char* rcp_message(int status) {
  switch (status) {
    case RCP_OK: return "ok";
    case RCP_ARGUMENT: return "null list or negative count";
    case RCP_BODY_RANGE: return "body out of range";
    case RCP_BODY_FIXED: return "body is fixed";
    case RCP_CAM_RANGE: return "camera out of range";
    case RCP_CAM_FIXED: return "camera of a fixed body";
    case RCP_LM_RANGE: return "landmark out of range";
    default: return "a queried landmark has more than 256 groups";
  }
}

struct RigCovGroups { int first, count; };
inline RigCovGroups rcp_groups(const RigPlan& rp, int lm) { return RigCovGroups{rp.lm_grp[lm], rp.lm_grp[lm + 1] - rp.lm_grp[lm]}; }

struct RigCovPlan {
  int n_free = 0, nQ = 0, n_items = 0, nu = 0, gmax = 0, nblk = 0;
  int first_bad = -1;               // query entry (or its id) the status is about
  std::vector<int> q_free;          // Q: free-body slots, ascending; right-hand sides 6 k .. 6 k + 5 belong to q_free[k]
  std::vector<int> qpos;            // [n_free] slot -> position in Q, -1: not in Q
  std::vector<int> col_unk;         // [16 nblk] unknown of each unit column, -1: an empty column
  std::vector<int> item_q, item_ext;  // [n_items] body queries then camera queries: position in Q; extrinsic 0 / 1, -1: the body block
  std::vector<int> u_lm, lm_q2u;    // unique queried landmarks in order of first appearance; query entry -> unique landmark
  // the call's share of the arena: [inputs, one copy up | work | outputs, one copy back]
  size_t off_ok = 0, off_col_unk = 0, off_q_free = 0, off_qpos = 0, off_item_q = 0, off_item_ext = 0, off_u_lm = 0, in_bytes = 0;
  size_t off_Linv = 0, off_Sdiag = 0, off_X = 0;
  size_t out_off = 0, off_pose = 0, off_point = 0, off_deg = 0, out_bytes = 0, total = 0;  // outputs relative to out_off
};

// rp: the rig plan of the problem (rig_plan_build succeeded); cam_intr: [n_cams].  RCP_OK and the
// plan, or the first rule broken (only first_bad is then meaningful).
inline int rcp_plan(const RigPlan& rp, int n_bodies, int n_cams, int n_lms, const int32_t* cam_intr,
                    const int32_t* bodies, int n_body_q, const int32_t* cams, int n_cam_q, const int32_t* lms, int n_lm_q,
                    RigCovPlan& P) {
  P = RigCovPlan();
  if (n_body_q < 0 || n_cam_q < 0 || n_lm_q < 0 || (n_body_q > 0 && !bodies) || (n_cam_q > 0 && !cams) || (n_lm_q > 0 && !lms))
    return RCP_ARGUMENT;
  for (int q = 0; q < n_body_q; q++) {
    P.first_bad = bodies[q];
    if (bodies[q] < 0 || bodies[q] >= n_bodies) return RCP_BODY_RANGE;
    if (rp.body_slot[bodies[q]] < 0) return RCP_BODY_FIXED;
  }
  for (int q = 0; q < n_cam_q; q++) {
    P.first_bad = cams[q];
    if (cams[q] < 0 || cams[q] >= n_cams) return RCP_CAM_RANGE;
    if (rp.cam_slot[cams[q]] < 0) return RCP_CAM_FIXED;
  }
  for (int q = 0; q < n_lm_q; q++) {
    P.first_bad = lms[q];
    if (lms[q] < 0 || lms[q] >= n_lms) return RCP_LM_RANGE;
    if (rcp_groups(rp, lms[q]).count > RCP_GMAX) return RCP_LM_GROUPS;
  }
  P.first_bad = -1;
  P.n_free = rp.n_free;
  std::vector<char> inQ(rp.n_free, 0);
  for (int q = 0; q < n_body_q; q++) inQ[rp.body_slot[bodies[q]]] = 1;
  for (int q = 0; q < n_cam_q; q++) inQ[rp.cam_slot[cams[q]]] = 1;
  std::vector<int> lm_slot(n_lm_q > 0 ? n_lms : 0, -1);
  P.lm_q2u.resize(n_lm_q);
  for (int q = 0; q < n_lm_q; q++) {
    int& s = lm_slot[lms[q]];
    if (s < 0) {
      s = (int)P.u_lm.size();
      P.u_lm.push_back(lms[q]);
      const RigCovGroups g = rcp_groups(rp, lms[q]);
      P.gmax = std::max(P.gmax, g.count);
      for (int k = g.first; k < g.first + g.count; k++) inQ[rp.grp_slot[k]] = 1;
    }
    P.lm_q2u[q] = s;
  }
  P.nu = (int)P.u_lm.size();
  P.qpos.assign(rp.n_free, -1);
  for (int s = 0; s < rp.n_free; s++)
    if (inQ[s]) {
      P.qpos[s] = (int)P.q_free.size();
      P.q_free.push_back(s);
    }
  P.nQ = (int)P.q_free.size();
  const int m = 6 * P.nQ;
  P.nblk = (m + PGC_COLS - 1) / PGC_COLS;
  P.col_unk.assign((size_t)P.nblk * PGC_COLS, -1);
  for (int j = 0; j < m; j++) P.col_unk[j] = 6 * P.q_free[j / 6] + j % 6;
  P.n_items = n_body_q + n_cam_q;
  P.item_q.resize(P.n_items);
  P.item_ext.resize(P.n_items);
  for (int q = 0; q < n_body_q; q++) {
    P.item_q[q] = P.qpos[rp.body_slot[bodies[q]]];
    P.item_ext[q] = -1;
  }
  for (int q = 0; q < n_cam_q; q++) {
    P.item_q[n_body_q + q] = P.qpos[rp.cam_slot[cams[q]]];
    P.item_ext[n_body_q + q] = cam_intr[cams[q]];
  }
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += pgc_align(bytes);
    return o;
  };
  const size_t n = 6 * (size_t)rp.n_free;
  P.off_ok = take(sizeof(int));
  P.off_col_unk = take(sizeof(int) * P.col_unk.size());
  P.off_q_free = take(sizeof(int) * (size_t)P.nQ);
  P.off_qpos = take(sizeof(int) * (size_t)rp.n_free);
  P.off_item_q = take(sizeof(int) * (size_t)P.n_items);
  P.off_item_ext = take(sizeof(int) * (size_t)P.n_items);
  P.off_u_lm = take(sizeof(int) * (size_t)P.nu);
  P.in_bytes = at;
  P.off_Linv = take(sizeof(double) * ((n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB);
  P.off_Sdiag = take(sizeof(double) * n);
  P.off_X = take(sizeof(double) * (size_t)P.nblk * n * PGC_COLS);
  P.out_off = at;
  P.off_pose = take(sizeof(double) * 36 * (size_t)P.n_items) - P.out_off;
  P.off_point = take(sizeof(double) * 9 * (size_t)P.nu) - P.out_off;
  P.off_deg = take(sizeof(int) * (size_t)P.nu) - P.out_off;
  P.out_bytes = at - P.out_off;
  P.total = at;
  return RCP_OK;
}

// a pair query on the bodies: the rules of bpp_check_pairs (a PgcPairError, first offender in *bad), then bpp_plan on the
// dense body system -- the pair members are the column bodies
inline int rcp_pair_plan(const RigPlan& rp, int n_bodies, const uint8_t* body_fixed, const int32_t* a, const int32_t* b, int n_pairs,
                         BaPairPlan& P, int* bad) {
  const int e = bpp_check_pairs(n_bodies, body_fixed, a, b, n_pairs, bad);
  if (e != PGC_PAIR_OK) return e;
  P = bpp_plan(rp.body_slot, rp.n_free, false, 0, false, a, b, n_pairs);
  return PGC_PAIR_OK;
}
