// ba_rig_plan.h -- the host half of the rig-constrained bundle adjustment (ba_rig.hip): validation of a vsl_ba_rig
// against its vsl_ba_problem, the free-body numbering, the camera -> (body slot, extrinsic) table, the observations
// sorted by landmark with the observations of one body ADJACENT inside a landmark, the (landmark, free body) groups
// that the Schur reduction works on, and the body-major lists of groups and observations that the gathers walk.
// Plain C++ (no HIP, no other header of the library): tests/cpp/ba_rig_plan_test.cpp drives it on the CPU.
//
// Orders, which are the summation orders of the kernels and so part of the result's bits:
//   observations  by landmark; inside a landmark the observations of fixed bodies first, then by free-body slot; ties by
//                 the caller's index
//   groups        one per (landmark, free body) that has an observation, numbered in that order: ascending landmark,
//                 then ascending slot.  A landmark seen by both cameras of one free body gives ONE group of two
//                 observations -- the normal stereo case
//   body lists    groups / observations of a free body in ascending group / sorted-observation number (so a body's
//                 groups are in ascending landmark: the Schur gather finds a partner by bisection)
//
// The MAP route (vsl_global_bundle_adjust_rig) adds rig_map_plan_build at the end of this file: the body
// covisibility graph, its band order through camera_band_order and the storage of the reduced body system through
// ba_reduced_layout (both of ba_host_plan.h, unchanged: the camera -> body slot table stands where the free solver has
// its camera -> free-camera table), the free-body slots in band order where the layout renumbers, and the list of
// co-visible slot pairs with their segments.
//
// The EXTRINSICS as unknowns (vsl_bundle_adjust_rig_ext) add rig_ext_plan_build at the end of this file: the
// slots of the free extrinsic blocks behind the free bodies and the group / observation lists of every slot.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "ba_host_plan.h"

enum RigPlanStatus {
  RIG_PLAN_OK = 0,
  RIG_PLAN_NULL,            // a null pointer
  RIG_PLAN_EMPTY,           // no camera, landmark, observation or body
  RIG_PLAN_INDEX,           // an observation's camera / landmark or a cam_intr out of range
  RIG_PLAN_CAM_BODY,        // cam_body out of range
  RIG_PLAN_BODY_NO_CAMERA,  // a body that carries no camera
  RIG_PLAN_SHARED_INTR,     // two cameras of one body with the same intrinsics block
  RIG_PLAN_NO_FREE_BODY,    // every body is fixed
  RIG_PLAN_EXTRINSIC,       // an extrinsic that is not finite or has a zero quaternion
  RIG_PLAN_EXT_NO_CAMERA,   // (extrinsics as unknowns) a free extrinsic block that no camera carries
  RIG_PLAN_NOTHING_FREE     // (extrinsics as unknowns) no free body and no free extrinsic block
};

inline const char* rig_plan_message(int status) {
  switch (status) {
    case RIG_PLAN_OK: return "ok";
    case RIG_PLAN_NULL: return "null pointer";
    case RIG_PLAN_EMPTY: return "empty problem";
    case RIG_PLAN_INDEX: return "observation or cam_intr out of range";
    case RIG_PLAN_CAM_BODY: return "cam_body out of range";
    case RIG_PLAN_BODY_NO_CAMERA: return "a body carries no camera";
    case RIG_PLAN_SHARED_INTR: return "two cameras of one body share an intrinsics block";
    case RIG_PLAN_NO_FREE_BODY: return "no free body";
    case RIG_PLAN_EXT_NO_CAMERA: return "a free extrinsic block that no camera carries";
    case RIG_PLAN_NOTHING_FREE: return "no free body and no free extrinsic block";
    default: return "extrinsic not finite or its quaternion zero";
  }
}

// the fields of vsl_ba_problem / vsl_ba_rig that the plan reads
struct RigPlanIn {
  int n_cams = 0, n_lms = 0, n_obs = 0;
  const int32_t *cam_intr = nullptr, *obs_cam = nullptr, *obs_lm = nullptr;
  int n_bodies = 0;
  const uint8_t* body_fixed = nullptr;
  const int32_t* cam_body = nullptr;
  const double* T_b_c = nullptr;  // [2][7]
};

struct RigPlan {
  int n_free = 0, n_fixed = 0;
  int first_bad = -1;                 // camera, body or observation the status is about
  std::vector<int> body_slot;         // [bodies] free-body number, -1 fixed
  std::vector<int> free_bodies;       // [n_free] body id
  std::vector<int> cam_slot;          // [cams] slot of the carrying body
  double T_b_c[14];                   // the two extrinsics, quaternion normalised
  double T_c_b[24];                   // their inverses as rotation matrix (9, row-major) and translation (3): Ad(T_b_c^-1)
  std::vector<int> perm;              // [obs] sorted position -> caller's observation
  std::vector<int> obs_cam, obs_lm;   // [obs] in sorted order
  std::vector<int> lm_start;          // [lms + 1] sorted observations of a landmark
  std::vector<int> lm_grp;            // [lms + 1] groups of a landmark
  std::vector<int> grp_lm, grp_slot, grp_begin, grp_end;  // [groups]; sorted observations [begin, end)
  std::vector<int> bg_start, bg_grp, bg_lm;               // [n_free + 1], [groups], [groups]: a body's groups and their landmarks
  std::vector<int> bo_start, bo_obs;                      // [n_free + 1], [free observations]: a body's sorted observations
  int n_groups() const { return (int)grp_lm.size(); }
};

// 0 and the plan, or the first rule broken (nothing of `out` is then meaningful except first_bad).  slot_bodies (the map
// route): the free bodies in the order of their slots, a permutation of the free body ids; null: ascending body id.
// allow_no_free_body (rig_ext_plan_build): every body fixed is a plan with empty group and body lists, not an error.
inline int rig_plan_build(const RigPlanIn& in, RigPlan& out, const std::vector<int>* slot_bodies = nullptr,
                          bool allow_no_free_body = false) {
  out = RigPlan();
  if (in.n_cams <= 0 || in.n_lms <= 0 || in.n_obs <= 0 || in.n_bodies <= 0) return RIG_PLAN_EMPTY;
  if (!in.cam_intr || !in.obs_cam || !in.obs_lm || !in.body_fixed || !in.cam_body || !in.T_b_c) return RIG_PLAN_NULL;
  const int C = in.n_cams, L = in.n_lms, O = in.n_obs, B = in.n_bodies;
  for (int c = 0; c < C; c++)
    if (in.cam_intr[c] < 0 || in.cam_intr[c] > 1) { out.first_bad = c; return RIG_PLAN_INDEX; }
  for (int i = 0; i < O; i++)
    if (in.obs_cam[i] < 0 || in.obs_cam[i] >= C || in.obs_lm[i] < 0 || in.obs_lm[i] >= L) { out.first_bad = i; return RIG_PLAN_INDEX; }
  for (int c = 0; c < C; c++)
    if (in.cam_body[c] < 0 || in.cam_body[c] >= B) { out.first_bad = c; return RIG_PLAN_CAM_BODY; }
  std::vector<int> seen(2 * (size_t)B, 0);
  for (int c = 0; c < C; c++)
    if (seen[2 * (size_t)in.cam_body[c] + in.cam_intr[c]]++) { out.first_bad = c; return RIG_PLAN_SHARED_INTR; }
  for (int b = 0; b < B; b++)
    if (!seen[2 * (size_t)b] && !seen[2 * (size_t)b + 1]) { out.first_bad = b; return RIG_PLAN_BODY_NO_CAMERA; }
  out.body_slot.assign(B, -1);
  for (int b = 0; b < B; b++) {
    if (in.body_fixed[b]) { out.n_fixed++; continue; }
    out.body_slot[b] = out.n_free++;
    out.free_bodies.push_back(b);
  }
  if (out.n_free == 0 && !allow_no_free_body) return RIG_PLAN_NO_FREE_BODY;
  if (slot_bodies) {
    out.free_bodies = *slot_bodies;
    for (int k = 0; k < out.n_free; k++) out.body_slot[out.free_bodies[k]] = k;
  }
  for (int k = 0; k < 2; k++) {
    const double* T = in.T_b_c + 7 * k;
    double nn = 0;
    for (int j = 0; j < 7; j++)
      if (!std::isfinite(T[j])) { out.first_bad = k; return RIG_PLAN_EXTRINSIC; }
    for (int j = 0; j < 4; j++) nn += T[j] * T[j];
    nn = std::sqrt(nn);
    if (!(nn > 0.0) || !std::isfinite(nn)) { out.first_bad = k; return RIG_PLAN_EXTRINSIC; }
    double* q = out.T_b_c + 7 * k;
    for (int j = 0; j < 4; j++) q[j] = T[j] / nn;
    for (int j = 4; j < 7; j++) q[j] = T[j];
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                         2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    // T_c_b = (R^T, -R^T t)
    double* o = out.T_c_b + 12 * k;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) o[3 * i + j] = R[3 * j + i];
    for (int i = 0; i < 3; i++) o[9 + i] = -(o[3 * i] * q[4] + o[3 * i + 1] * q[5] + o[3 * i + 2] * q[6]);
  }
  out.cam_slot.resize(C);
  for (int c = 0; c < C; c++) out.cam_slot[c] = out.body_slot[in.cam_body[c]];

  out.perm.resize(O);
  std::iota(out.perm.begin(), out.perm.end(), 0);
  std::stable_sort(out.perm.begin(), out.perm.end(), [&](int a, int b) {
    if (in.obs_lm[a] != in.obs_lm[b]) return in.obs_lm[a] < in.obs_lm[b];
    return out.cam_slot[in.obs_cam[a]] < out.cam_slot[in.obs_cam[b]];
  });
  out.obs_cam.resize(O);
  out.obs_lm.resize(O);
  out.lm_start.assign(L + 1, 0);
  for (int q = 0; q < O; q++) {
    out.obs_cam[q] = in.obs_cam[out.perm[q]];
    out.obs_lm[q] = in.obs_lm[out.perm[q]];
    out.lm_start[out.obs_lm[q] + 1]++;
  }
  for (int l = 0; l < L; l++) out.lm_start[l + 1] += out.lm_start[l];

  out.lm_grp.assign(L + 1, 0);
  out.bo_start.assign(out.n_free + 1, 0);
  out.bg_start.assign(out.n_free + 1, 0);
  for (int l = 0; l < L; l++) {
    int q = out.lm_start[l];
    const int end = out.lm_start[l + 1];
    while (q < end && out.cam_slot[out.obs_cam[q]] < 0) q++;
    while (q < end) {
      const int s = out.cam_slot[out.obs_cam[q]];
      int e = q;
      while (e < end && out.cam_slot[out.obs_cam[e]] == s) e++;
      out.grp_lm.push_back(l);
      out.grp_slot.push_back(s);
      out.grp_begin.push_back(q);
      out.grp_end.push_back(e);
      out.bg_start[s + 1]++;
      out.bo_start[s + 1] += e - q;
      q = e;
    }
    out.lm_grp[l + 1] = (int)out.grp_lm.size();
  }
  for (int s = 0; s < out.n_free; s++) {
    out.bg_start[s + 1] += out.bg_start[s];
    out.bo_start[s + 1] += out.bo_start[s];
  }
  const int G = out.n_groups();
  out.bg_grp.resize(G);
  out.bg_lm.resize(G);
  out.bo_obs.resize(out.bo_start[out.n_free]);
  std::vector<int> gpos(out.bg_start.begin(), out.bg_start.end() - 1), opos(out.bo_start.begin(), out.bo_start.end() - 1);
  for (int g = 0; g < G; g++) {
    const int s = out.grp_slot[g];
    out.bg_grp[gpos[s]] = g;
    out.bg_lm[gpos[s]++] = out.grp_lm[g];
    for (int q = out.grp_begin[g]; q < out.grp_end[g]; q++) out.bo_obs[opos[s]++] = q;
  }
  return RIG_PLAN_OK;
}

// the properties the kernels rely on (used by the CPU test on every plan it builds): true when they hold
inline bool rig_plan_check(const RigPlanIn& in, const RigPlan& p) {
  const int O = in.n_obs, L = in.n_lms, G = p.n_groups();
  std::vector<int> hit(O, 0);
  for (int q = 0; q < O; q++) {
    if (p.perm[q] < 0 || p.perm[q] >= O || hit[p.perm[q]]++) return false;
    if (q > 0 && p.obs_lm[q] < p.obs_lm[q - 1]) return false;
    if (q < p.lm_start[p.obs_lm[q]] || q >= p.lm_start[p.obs_lm[q] + 1]) return false;
  }
  if (p.lm_start[L] != O || p.lm_grp[L] != G) return false;
  size_t free_obs = 0;
  for (int g = 0; g < G; g++) {
    const int l = p.grp_lm[g], s = p.grp_slot[g];
    if (s < 0 || s >= p.n_free || g < p.lm_grp[l] || g >= p.lm_grp[l + 1]) return false;
    if (p.grp_begin[g] >= p.grp_end[g] || p.grp_begin[g] < p.lm_start[l] || p.grp_end[g] > p.lm_start[l + 1]) return false;
    if (g > 0 && (p.grp_lm[g - 1] > l || (p.grp_lm[g - 1] == l && (p.grp_slot[g - 1] >= s || p.grp_end[g - 1] != p.grp_begin[g])))) return false;
    for (int q = p.grp_begin[g]; q < p.grp_end[g]; q++)
      if (p.cam_slot[p.obs_cam[q]] != s) return false;
    free_obs += p.grp_end[g] - p.grp_begin[g];
  }
  size_t want = 0;
  for (int q = 0; q < O; q++) want += p.cam_slot[p.obs_cam[q]] >= 0;
  if (free_obs != want || p.bo_obs.size() != want || p.bg_start[p.n_free] != G) return false;
  for (int s = 0; s < p.n_free; s++) {
    for (int k = p.bg_start[s]; k < p.bg_start[s + 1]; k++) {
      if (p.grp_slot[p.bg_grp[k]] != s || p.bg_lm[k] != p.grp_lm[p.bg_grp[k]]) return false;
      if (k > p.bg_start[s] && p.bg_lm[k - 1] >= p.bg_lm[k]) return false;  // strictly ascending: bisection finds at most one
    }
    for (int k = p.bo_start[s]; k < p.bo_start[s + 1]; k++) {
      if (p.cam_slot[p.obs_cam[p.bo_obs[k]]] != s) return false;
      if (k > p.bo_start[s] && p.bo_obs[k - 1] >= p.bo_obs[k]) return false;
    }
  }
  return true;
}

// ------------------------------------------------------------------------------------------------ the map route
#if defined(__HIPCC__)
#define RIG_PLAN_HD __host__ __device__
#else
#define RIG_PLAN_HD
#endif

// Where entry (x, y) of the 6 x 6 block S_(hi, lo), hi >= lo in slot order, lives in the storage of a layout, as an
// offset from the START of the allocation (BaLayout::offS included); -1: the entry is not stored (y > x of a diagonal
// block in the band forms: only the lower triangle exists).  form 0 dense (ldS = n, the caller mirrors), 1 linear band,
// 2 cyclic band: a pair further apart than half_cyc slots is a neighbour AROUND the ring and its block is stored
// TRANSPOSED in row block lo at the negative column block hi - n_free (BaCommon in ba_state.h, ba_pair_list_kernel).
// The kernel and the host (expansion, tests) share this one rule.
RIG_PLAN_HD inline long long rig_map_entry_at(int form, int ldS, int offS, int n_free, int half_cyc, int hi, int lo, int x, int y) {
  if (form == 0) return (long long)(6 * hi + x) * ldS + 6 * lo + y;
  if (hi == lo && y > x) return -1;
  if (form == 2 && hi - lo > half_cyc) return (long long)(6 * lo + y) * ldS + (6 * (hi - n_free) + x) + offS;
  return (long long)(6 * hi + x) * ldS + (6 * lo + y) + offS;
}

struct RigMapPlan {
  BaLayout layout;
  int form = 0;                      // 0 dense / 1 linear band / 2 cyclic band: what vsl_ctx_last_ba_layout reports
  int half_lin = 0, half_cyc = 0;    // block half-bandwidths of the body graph (0 where the layout did not ask)
  std::vector<int> natural_slot;     // [n_free] k-th free body in ascending id -> slot (the identity unless layout.renumber)
  std::vector<int> pair_hi, pair_lo; // co-visible slot pairs, hi >= lo: the n_free diagonal pairs first (ascending slot),
                                     // then the others ascending in (hi, lo)
  std::vector<int> pair_first;       // [pairs + 1] first (pair, segment) item of a pair = first 42-entry partial sum
  std::vector<int> item_pair;        // [items] pair of an item (its segment: item - pair_first[pair])
  int n_pairs() const { return (int)pair_hi.size(); }
  int n_items() const { return (int)item_pair.size(); }
};

// segments of a gather over a list of `len` entries: one per 512, at most 64 (the rule of the dense rig route)
inline int rig_segments(int len) { return std::min(64, std::max(1, (len + 511) / 512)); }

// The plan of the map route: `plan` as rig_plan_build gives it, except that the slots follow the band order where the
// layout renumbers; returns rig_plan_build's status.
inline int rig_map_plan_build(const RigPlanIn& in, const BaLayoutSwitches& sw, RigPlan& plan, RigMapPlan& mp,
                              const HostTeamConfig& threads = HostTeamConfig()) {
  mp = RigMapPlan();
  int st = rig_plan_build(in, plan);
  if (st != RIG_PLAN_OK) return st;
  const int nf = plan.n_free, n = 6 * nf;
  mp.natural_slot.resize(nf);
  std::iota(mp.natural_slot.begin(), mp.natural_slot.end(), 0);
  if (ba_layout_considers_band(n, sw)) {
    // the body graph: camera_band_order reads the counts and the two index arrays of the problem and nothing else
    vsl_ba_problem gp;
    memset(&gp, 0, sizeof(gp));
    gp.n_cams = in.n_cams; gp.n_lms = in.n_lms; gp.n_obs = in.n_obs;
    gp.obs_cam = in.obs_cam; gp.obs_lm = in.obs_lm;
    std::vector<int> start((size_t)in.n_lms + 1), order;
    const bool sorted_in = ba_landmark_csr(&gp, start.data());
    mp.half_lin = camera_band_order(&gp, start.data(), sorted_in, plan.cam_slot, nf, order, &mp.half_cyc, threads);
    mp.layout = ba_reduced_layout(n, mp.half_lin, mp.half_cyc, sw);
    if (mp.layout.renumber) {
      std::vector<int> slot_bodies(nf);
      for (int k = 0; k < nf; k++) {
        slot_bodies[k] = plan.free_bodies[order[k]];
        mp.natural_slot[order[k]] = k;
      }
      if ((st = rig_plan_build(in, plan, &slot_bodies)) != RIG_PLAN_OK) return st;
    }
  } else {
    mp.layout = ba_reduced_layout(n, 0, 0, sw);
  }
  mp.form = mp.layout.cyclic ? 2 : (mp.layout.banded ? 1 : 0);
  // co-visible pairs: the groups of a landmark come in ascending slot
  std::vector<long long> keys;
  for (int l = 0; l < in.n_lms; l++)
    for (int g = plan.lm_grp[l]; g < plan.lm_grp[l + 1]; g++)
      for (int h = g + 1; h < plan.lm_grp[l + 1]; h++) keys.push_back((long long)plan.grp_slot[h] * nf + plan.grp_slot[g]);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  mp.pair_hi.reserve(nf + keys.size());
  mp.pair_lo.reserve(nf + keys.size());
  for (int s = 0; s < nf; s++) {
    mp.pair_hi.push_back(s);
    mp.pair_lo.push_back(s);
  }
  for (long long k : keys) {
    mp.pair_hi.push_back((int)(k / nf));
    mp.pair_lo.push_back((int)(k % nf));
  }
  mp.pair_first.assign(1, 0);
  for (int p = 0; p < mp.n_pairs(); p++) {
    const int hi = mp.pair_hi[p], lo = mp.pair_lo[p];
    const int nseg = rig_segments(std::max(plan.bg_start[hi + 1] - plan.bg_start[hi], plan.bg_start[lo + 1] - plan.bg_start[lo]));
    for (int q = 0; q < nseg; q++) mp.item_pair.push_back(p);
    mp.pair_first.push_back(mp.n_items());
  }
  return RIG_PLAN_OK;
}

// S of the map route, as the device leaves it in the layout's storage (s_elems doubles), to dense row-major n x n in
// ASCENDING-BODY order.  Every stored position of a row is read, the padding between bw and bw + VSL_CHOL_NB included:
// what the storage holds that the solver would see is what comes out (mirrored: the band keeps the lower triangle).
inline void rig_map_expand(const RigMapPlan& mp, int n_free, const double* store, double* dense) {
  const int n = 6 * n_free;
  const BaLayout& y = mp.layout;
  std::vector<double> slot((size_t)n * n, 0.0);
  if (!y.banded) {
    std::copy(store, store + (size_t)n * n, slot.begin());
  } else {
    for (int i = 0; i < n; i++)
      for (int c = i - y.ldS; c <= i; c++) {
        const double v = store[(size_t)i * y.ldS + c + y.offS];  // (c + offS >= i - ldS + offS = i >= 0)
        int j = c;
        if (j < 0) {
          if (!y.cyclic) continue;  // outside the matrix: never read by the linear forms
          j += n;  // the wrap-around corner (the ring has at least 8 blocks wider than the band: j > i + ldS)
        }
        slot[(size_t)i * n + j] = slot[(size_t)j * n + i] = v;
      }
  }
  for (int a = 0; a < n_free; a++)
    for (int b = 0; b < n_free; b++)
      for (int x = 0; x < 6; x++)
        for (int z = 0; z < 6; z++)
          dense[(size_t)(6 * a + x) * n + 6 * b + z] = slot[(size_t)(6 * mp.natural_slot[a] + x) * n + 6 * mp.natural_slot[b] + z];
}

// a vector of the slot order (6 per slot) to ascending-body order
inline void rig_map_unpermute(const RigMapPlan& mp, int n_free, const double* in_slots, double* out) {
  for (int a = 0; a < n_free; a++)
    for (int x = 0; x < 6; x++) out[6 * a + x] = in_slots[6 * mp.natural_slot[a] + x];
}

// ------------------------------------------------------------------------------------------------ EXTRINSICS
// The extrinsics as unknowns (vsl_bundle_adjust_rig_ext, ba_rig.hip "EXTRINSICS").  A free extrinsic
// block k is one more 6-dof POSE SLOT behind the free bodies: slot n_free + (number of free blocks below k).  An
// observation in a camera of block k touches the slot of its body (when that body is free) AND the slot of block k
// (when that block is free, whether the body is free or not).  The plan is rig_plan_build's (observation order, body
// slots, body groups, every body fixed allowed) plus
//   cam_eslot   camera -> slot of its extrinsic block, -1 when that block is held
//   pose_free   the pose-block array of the solver is [bodies | block 0 | block 1]: block -> slot or -1
//   groups      one per (landmark, slot) with an observation: the landmark's body groups in rig_plan_build's order
//               (ascending slot), then its extrinsic groups in ascending block.  The observations of an extrinsic group
//               are NOT adjacent in the sorted order (they are spread over the bodies), so EVERY group names its
//               observations through an index list, grp_obs[grp_first[g] .. grp_first[g + 1]), ascending
//   slot lists  sg_*: a slot's groups in ascending landmark (the Schur gather's bisection and the back-substitution
//               serve the border through the same lists); so_*: a slot's sorted observations, ascending
struct RigExtPlan {
  int n_ext = 0, n_slots = 0;
  int ext_slot[2] = {-1, -1};
  std::vector<int> cam_eslot;                      // [cams]
  std::vector<int> pose_free;                      // [bodies + 2]
  std::vector<int> lm_grp;                         // [lms + 1]
  std::vector<int> grp_lm, grp_slot, grp_first;    // [groups], [groups], [groups + 1]
  std::vector<int> grp_obs;                        // [sum of group sizes]
  std::vector<int> sg_start, sg_grp, sg_lm;        // [n_slots + 1], [groups], [groups]
  std::vector<int> so_start, so_obs;               // [n_slots + 1], [sum of slot list sizes]
  int n_groups() const { return (int)grp_lm.size(); }
};

// 0 and the two plans, or the first rule broken: whatever rig_plan_build refuses (except "no free body" while a block
// is free), a null ext_free, a free block that no camera carries, nothing free at all.  in.T_b_c is the explicit
// extrinsic argument of the call.
inline int rig_ext_plan_build(const RigPlanIn& in, const uint8_t* ext_free, RigPlan& base, RigExtPlan& x) {
  x = RigExtPlan();
  if (!ext_free) { base = RigPlan(); return RIG_PLAN_NULL; }
  const int st = rig_plan_build(in, base, nullptr, true);
  if (st != RIG_PLAN_OK) return st;
  const int C = in.n_cams, L = in.n_lms, B = in.n_bodies, nfb = base.n_free;
  for (int k = 0; k < 2; k++) {
    if (!ext_free[k]) continue;
    bool carried = false;
    for (int c = 0; c < C && !carried; c++) carried = in.cam_intr[c] == k;
    if (!carried) { base.first_bad = k; return RIG_PLAN_EXT_NO_CAMERA; }
    x.ext_slot[k] = nfb + x.n_ext++;
  }
  x.n_slots = nfb + x.n_ext;
  if (x.n_slots == 0) return RIG_PLAN_NOTHING_FREE;
  x.cam_eslot.resize(C);
  for (int c = 0; c < C; c++) x.cam_eslot[c] = x.ext_slot[in.cam_intr[c]];
  x.pose_free.assign(base.body_slot.begin(), base.body_slot.end());
  x.pose_free.push_back(x.ext_slot[0]);
  x.pose_free.push_back(x.ext_slot[1]);
  (void)B;

  x.lm_grp.assign(L + 1, 0);
  x.sg_start.assign(x.n_slots + 1, 0);
  x.so_start.assign(x.n_slots + 1, 0);
  x.grp_first.assign(1, 0);
  for (int l = 0; l < L; l++) {
    for (int g = base.lm_grp[l]; g < base.lm_grp[l + 1]; g++) {
      x.grp_lm.push_back(l);
      x.grp_slot.push_back(base.grp_slot[g]);
      for (int q = base.grp_begin[g]; q < base.grp_end[g]; q++) x.grp_obs.push_back(q);
      x.grp_first.push_back((int)x.grp_obs.size());
    }
    for (int k = 0; k < 2; k++) {
      if (x.ext_slot[k] < 0) continue;
      const size_t before = x.grp_obs.size();
      for (int q = base.lm_start[l]; q < base.lm_start[l + 1]; q++)
        if (in.cam_intr[base.obs_cam[q]] == k) x.grp_obs.push_back(q);
      if (x.grp_obs.size() == before) continue;
      x.grp_lm.push_back(l);
      x.grp_slot.push_back(x.ext_slot[k]);
      x.grp_first.push_back((int)x.grp_obs.size());
    }
    x.lm_grp[l + 1] = x.n_groups();
  }
  const int G = x.n_groups();
  for (int g = 0; g < G; g++) {
    x.sg_start[x.grp_slot[g] + 1]++;
    x.so_start[x.grp_slot[g] + 1] += x.grp_first[g + 1] - x.grp_first[g];
  }
  for (int s = 0; s < x.n_slots; s++) {
    x.sg_start[s + 1] += x.sg_start[s];
    x.so_start[s + 1] += x.so_start[s];
  }
  x.sg_grp.resize(G);
  x.sg_lm.resize(G);
  x.so_obs.resize(x.so_start[x.n_slots]);
  std::vector<int> gpos(x.sg_start.begin(), x.sg_start.end() - 1), opos(x.so_start.begin(), x.so_start.end() - 1);
  for (int g = 0; g < G; g++) {
    const int s = x.grp_slot[g];
    x.sg_grp[gpos[s]] = g;
    x.sg_lm[gpos[s]++] = x.grp_lm[g];
    for (int q = x.grp_first[g]; q < x.grp_first[g + 1]; q++) x.so_obs[opos[s]++] = x.grp_obs[q];
  }
  return RIG_PLAN_OK;
}

// the properties the EXTRINSICS kernels rely on -- every index they form stays inside its array: true when they hold
inline bool rig_ext_plan_check(const RigPlanIn& in, const RigPlan& base, const RigExtPlan& x) {
  const int O = in.n_obs, L = in.n_lms, G = x.n_groups(), ns = x.n_slots;
  if (ns != base.n_free + x.n_ext || ns <= 0) return false;
  if ((int)x.cam_eslot.size() != in.n_cams || (int)x.pose_free.size() != in.n_bodies + 2) return false;
  for (int p : x.pose_free)
    if (p < -1 || p >= ns) return false;
  if ((int)x.lm_grp.size() != L + 1 || x.lm_grp[0] != 0 || x.lm_grp[L] != G) return false;
  if ((int)x.grp_first.size() != G + 1 || x.grp_first[0] != 0 || x.grp_first[G] != (int)x.grp_obs.size()) return false;
  for (int g = 0; g < G; g++) {
    const int l = x.grp_lm[g], s = x.grp_slot[g];
    if (l < 0 || l >= L || s < 0 || s >= ns || g < x.lm_grp[l] || g >= x.lm_grp[l + 1]) return false;
    if (x.grp_first[g] >= x.grp_first[g + 1]) return false;
    if (g > 0 && (x.grp_lm[g - 1] > l || (x.grp_lm[g - 1] == l && x.grp_slot[g - 1] >= s))) return false;
    for (int k = x.grp_first[g]; k < x.grp_first[g + 1]; k++) {
      const int q = x.grp_obs[k];
      if (q < base.lm_start[l] || q >= base.lm_start[l + 1]) return false;
      if (k > x.grp_first[g] && x.grp_obs[k - 1] >= q) return false;
      const int cam = base.obs_cam[q];
      if ((s < base.n_free ? base.cam_slot[cam] : x.cam_eslot[cam]) != s) return false;
    }
  }
  if ((int)x.sg_start.size() != ns + 1 || (int)x.so_start.size() != ns + 1 || x.sg_start[0] != 0 || x.so_start[0] != 0) return false;
  if (x.sg_start[ns] != G || x.so_start[ns] != (int)x.so_obs.size() || x.so_obs.size() != x.grp_obs.size()) return false;
  for (int s = 0; s < ns; s++) {
    if (x.sg_start[s] > x.sg_start[s + 1] || x.so_start[s] > x.so_start[s + 1]) return false;
    for (int k = x.sg_start[s]; k < x.sg_start[s + 1]; k++) {
      if (x.sg_grp[k] < 0 || x.sg_grp[k] >= G || x.grp_slot[x.sg_grp[k]] != s || x.sg_lm[k] != x.grp_lm[x.sg_grp[k]]) return false;
      if (k > x.sg_start[s] && x.sg_lm[k - 1] >= x.sg_lm[k]) return false;  // strictly ascending: bisection finds at most one
    }
    for (int k = x.so_start[s]; k < x.so_start[s + 1]; k++) {
      const int q = x.so_obs[k];
      if (q < 0 || q >= O) return false;
      if (k > x.so_start[s] && x.so_obs[k - 1] >= q) return false;
      const int cam = base.obs_cam[q];
      if ((s < base.n_free ? base.cam_slot[cam] : x.cam_eslot[cam]) != s) return false;
    }
  }
  return true;
}
