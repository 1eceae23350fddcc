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

// ---- the extrinsics as unknowns (ba_rig.hip "EXTRINSICS: COVARIANCES", vsl_ba_rig_ext_covariance) ----
//   rxcp_plan       the argument rules of a marginal query on the problem of vsl_bundle_adjust_rig_ext (slots = free
//                   bodies, then free blocks: RigExtPlan); the union of SLOTS whose six unit columns of S^-1 are solved, in
//                   ascending slot -- queried bodies, the body and / or block slot of a queried camera, every slot with a
//                   group at a queried landmark, every block slot when cov_ext or cov_body_ext is asked; and EVERY slot
//                   as soon as a block slot is among them (the gauge check reads the whole diagonal of S^-1) --; slot ->
//                   position; one ITEM per pose query with its kind; the unique queried landmarks; the slot PAIRS whose
//                   12 x 12 joint block vsl_cov_pair_blocks_dev gathers ((body slot, block slot) ascending, then (block 0,
//                   block 1)); the call's share of the arena.
// The statuses are RigCovPlanStatus plus RCP_CAM_HELD; the messages rxcp_message.
#define RCP_CAM_HELD (RCP_LM_GROUPS + 1)  // a queried camera of a fixed body whose extrinsic block is held

inline const char* rxcp_message(int status) {
  return status == RCP_CAM_HELD ? "camera of a fixed body in a held extrinsic block" : rcp_message(status);
}

enum RigExtCovKind {
  RXC_BODY = 0,           // the body's 6 x 6 block
  RXC_CAM_FREE_FREE = 1,  // free body, free block: A Sigma_joint A^T, A = [Ad | I], on the pair's joint block
  RXC_CAM_FREE_HELD = 2,  // free body, held block: Ad Sigma_bb Ad^T (the rig covariance's formula)
  RXC_CAM_FIXED_FREE = 3, // fixed body, free block: Sigma_ee of the block
  RXC_EXT = 4,            // the 6 x 6 block of a free extrinsic block (cov_ext with one free block)
  RXC_CROSS = 5           // [S^-1] at (body slot, block slot): the upper right block of the pair's joint block
};

// one pose item as the device reads it (four ints)
struct RigExtCovItem {
  int32_t kind;
  int32_t q;     // position in Q of the slot whose diagonal block the item reads (body; the block for kinds 3, 4); -1: kind 5
  int32_t blk;   // extrinsic block k of the camera (its Ad(T_b_c^-1)); -1: none
  int32_t pair;  // joint block of kinds 1 and 5; -1: none
};

struct RigExtCovPlan {
  int n_slots = 0, n_ext = 0, nQ = 0, n_items = 0, nu = 0, gmax = 0, nblk = 0, n_pairs = 0;
  int n_body_q = 0, n_cam_q = 0, n_ext_items = 0, n_cross = 0;  // items: bodies | cameras | extrinsic (0 / 1) | cross
  int ext_pair = -1;                // the (block 0, block 1) pair: cov_ext with both blocks free
  int first_bad = -1;
  std::vector<int> q_slot;          // Q: slots, ascending; right-hand sides 6 k .. 6 k + 5 belong to q_slot[k]
  std::vector<int> qpos;            // [n_slots] slot -> position in Q, -1: not in Q
  std::vector<int> col_unk;         // [16 nblk]
  std::vector<RigExtCovItem> items;
  std::vector<PgcPairDev> pairs;
  std::vector<int> u_lm, lm_q2u;
  size_t off_ok = 0, off_col_unk = 0, off_q_slot = 0, off_qpos = 0, off_items = 0, off_pairs = 0, off_u_lm = 0, off_tcb = 0, in_bytes = 0;
  size_t off_Linv = 0, off_Sdiag = 0, off_X = 0;
  size_t out_off = 0, off_pose = 0, off_joint = 0, off_point = 0, off_deg = 0, out_bytes = 0, total = 0;  // outputs relative to out_off
};

// rp, xp: the plans of the problem (rig_ext_plan_build succeeded, at least one block free).  want_ext / want_cross: cov_ext
// / cov_body_ext is asked.  RCP_OK and the plan, or the first rule broken (only first_bad is then meaningful).
inline int rxcp_plan(const RigPlan& rp, const RigExtPlan& xp, int n_bodies, int n_cams, int n_lms, const int32_t* cam_intr,
                     const int32_t* bodies, int n_body_q, const int32_t* cams, int n_cam_q, const int32_t* lms, int n_lm_q,
                     bool want_ext, bool want_cross, RigExtCovPlan& P) {
  P = RigExtCovPlan();
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
    if (rp.cam_slot[cams[q]] < 0 && xp.cam_eslot[cams[q]] < 0) return RCP_CAM_HELD;
  }
  for (int q = 0; q < n_lm_q; q++) {
    P.first_bad = lms[q];
    if (lms[q] < 0 || lms[q] >= n_lms) return RCP_LM_RANGE;
    if (xp.lm_grp[lms[q] + 1] - xp.lm_grp[lms[q]] > RCP_GMAX) return RCP_LM_GROUPS;
  }
  P.first_bad = -1;
  const int ns = xp.n_slots, nfb = rp.n_free;
  P.n_slots = ns;
  P.n_ext = xp.n_ext;
  P.n_body_q = n_body_q;
  P.n_cam_q = n_cam_q;
  std::vector<char> inQ(ns, 0);
  for (int q = 0; q < n_body_q; q++) inQ[rp.body_slot[bodies[q]]] = 1;
  for (int q = 0; q < n_cam_q; q++) {
    if (rp.cam_slot[cams[q]] >= 0) inQ[rp.cam_slot[cams[q]]] = 1;
    if (xp.cam_eslot[cams[q]] >= 0) inQ[xp.cam_eslot[cams[q]]] = 1;
  }
  if (want_ext || want_cross)
    for (int s = nfb; s < ns; s++) inQ[s] = 1;
  std::vector<int> lm_slot(n_lm_q > 0 ? n_lms : 0, -1);
  P.lm_q2u.resize(n_lm_q);
  for (int q = 0; q < n_lm_q; q++) {
    int& s = lm_slot[lms[q]];
    if (s < 0) {
      s = (int)P.u_lm.size();
      P.u_lm.push_back(lms[q]);
      const int g0 = xp.lm_grp[lms[q]], g1 = xp.lm_grp[lms[q] + 1];
      P.gmax = std::max(P.gmax, g1 - g0);
      for (int k = g0; k < g1; k++) inQ[xp.grp_slot[k]] = 1;
    }
    P.lm_q2u[q] = s;
  }
  P.nu = (int)P.u_lm.size();
  // an extrinsic slot among them: EVERY slot (the order-independent pivot rule reads the whole diagonal of S^-1, so that
  // a gauge direction is reported whatever the query names)
  for (int s = nfb; s < ns; s++)
    if (inQ[s]) {
      std::fill(inQ.begin(), inQ.end(), (char)1);
      break;
    }
  P.qpos.assign(ns, -1);
  for (int s = 0; s < ns; s++)
    if (inQ[s]) {
      P.qpos[s] = (int)P.q_slot.size();
      P.q_slot.push_back(s);
    }
  P.nQ = (int)P.q_slot.size();
  const int m = 6 * P.nQ;
  P.nblk = (m + PGC_COLS - 1) / PGC_COLS;
  P.col_unk.assign((size_t)P.nblk * PGC_COLS, -1);
  for (int j = 0; j < m; j++) P.col_unk[j] = 6 * P.q_slot[j / 6] + j % 6;
  // the slot pairs: (body slot, block slot) in ascending order, then (block 0, block 1)
  std::vector<char> need((size_t)nfb * std::max(xp.n_ext, 1), 0);
  for (int q = 0; q < n_cam_q; q++)
    if (rp.cam_slot[cams[q]] >= 0 && xp.cam_eslot[cams[q]] >= 0) need[(size_t)rp.cam_slot[cams[q]] * xp.n_ext + (xp.cam_eslot[cams[q]] - nfb)] = 1;
  if (want_cross)
    for (int q = 0; q < n_body_q; q++)
      for (int j = 0; j < xp.n_ext; j++) need[(size_t)rp.body_slot[bodies[q]] * xp.n_ext + j] = 1;
  std::vector<int> pair_of((size_t)nfb * std::max(xp.n_ext, 1), -1);
  auto add_pair = [&](int a, int b) {
    PgcPairDev d;
    d.fa = a; d.fb = b;
    d.ca = 6 * P.qpos[a]; d.cb = 6 * P.qpos[b];
    d.na = a; d.nb = b;
    d.kind = PGC_SOLVE; d.pad = 0;
    P.pairs.push_back(d);
    return (int)P.pairs.size() - 1;
  };
  for (int s = 0; s < nfb; s++)
    for (int j = 0; j < xp.n_ext; j++)
      if (need[(size_t)s * xp.n_ext + j]) pair_of[(size_t)s * xp.n_ext + j] = add_pair(s, nfb + j);
  if (want_ext && xp.n_ext == 2) P.ext_pair = add_pair(nfb, nfb + 1);
  P.n_pairs = (int)P.pairs.size();
  // the items: bodies | cameras | the block of a single free block | cross blocks [body query][block]
  for (int q = 0; q < n_body_q; q++) P.items.push_back(RigExtCovItem{RXC_BODY, P.qpos[rp.body_slot[bodies[q]]], -1, -1});
  for (int q = 0; q < n_cam_q; q++) {
    const int sb = rp.cam_slot[cams[q]], se = xp.cam_eslot[cams[q]], k = cam_intr[cams[q]];
    if (sb >= 0 && se >= 0) P.items.push_back(RigExtCovItem{RXC_CAM_FREE_FREE, P.qpos[sb], k, pair_of[(size_t)sb * xp.n_ext + (se - nfb)]});
    else if (sb >= 0) P.items.push_back(RigExtCovItem{RXC_CAM_FREE_HELD, P.qpos[sb], k, -1});
    else P.items.push_back(RigExtCovItem{RXC_CAM_FIXED_FREE, P.qpos[se], -1, -1});
  }
  if (want_ext && xp.n_ext == 1) {
    P.items.push_back(RigExtCovItem{RXC_EXT, P.qpos[nfb], -1, -1});
    P.n_ext_items = 1;
  }
  if (want_cross)
    for (int q = 0; q < n_body_q; q++)
      for (int j = 0; j < xp.n_ext; j++) {
        P.items.push_back(RigExtCovItem{RXC_CROSS, -1, -1, pair_of[(size_t)rp.body_slot[bodies[q]] * xp.n_ext + j]});
        P.n_cross++;
      }
  P.n_items = (int)P.items.size();
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += pgc_align(bytes);
    return o;
  };
  const size_t n = 6 * (size_t)ns;
  P.off_ok = take(sizeof(int));
  P.off_col_unk = take(sizeof(int) * P.col_unk.size());
  P.off_q_slot = take(sizeof(int) * (size_t)P.nQ);
  P.off_qpos = take(sizeof(int) * (size_t)ns);
  P.off_items = take(sizeof(RigExtCovItem) * (size_t)P.n_items);
  P.off_pairs = take(sizeof(PgcPairDev) * (size_t)P.n_pairs);
  P.off_u_lm = take(sizeof(int) * (size_t)P.nu);
  P.off_tcb = take(sizeof(double) * 24);
  P.in_bytes = at;
  P.off_Linv = take(sizeof(double) * ((n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB);
  P.off_Sdiag = take(sizeof(double) * n);
  P.off_X = take(sizeof(double) * (size_t)P.nblk * n * PGC_COLS);
  P.out_off = at;
  P.off_pose = take(sizeof(double) * 36 * (size_t)P.n_items) - P.out_off;
  P.off_joint = take(sizeof(double) * 144 * (size_t)P.n_pairs) - P.out_off;
  P.off_point = take(sizeof(double) * 9 * (size_t)P.nu) - P.out_off;
  P.off_deg = take(sizeof(int) * (size_t)P.nu) - P.out_off;
  P.out_bytes = at - P.out_off;
  P.total = at;
  return RCP_OK;
}
