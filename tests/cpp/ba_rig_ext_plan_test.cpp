// Drives the EXTRINSICS part of visual-slam_amd/csrc/ba_rig_plan.h (rig_ext_plan_build) on the CPU (plain C++, no HIP):
// tests/test_ba_rig_ext_plan_cpu.py.
//   ba_rig_ext_plan_test plan e0 e1 < problem   prints the extrinsic plan's arrays, one "name v v v" line each, after
//                                               checking it against the brute-force construction below
//   ba_rig_ext_plan_test check e0 e1 < problem  prints "status first_bad"
//   ba_rig_ext_plan_test sweep                  random problems of many shapes (every body fixed among them) x the three
//                                               choices of free blocks: every plan must equal the brute-force one and
//                                               hold rig_ext_plan_check
// problem: n_bodies / body_fixed / n_cams / cam_body / cam_intr / n_lms / n_obs / obs_cam / obs_lm, whitespace separated.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "ba_rig_plan.h"

static const double kTbc[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, std::sqrt(0.5) * 2, std::sqrt(0.5) * 2, 1, 2, 3};

struct Problem {
  std::vector<uint8_t> body_fixed;
  std::vector<int32_t> cam_body, cam_intr, obs_cam, obs_lm;
  int n_lms = 0;
  RigPlanIn in() const {
    RigPlanIn r;
    r.n_cams = (int)cam_body.size(); r.n_lms = n_lms; r.n_obs = (int)obs_cam.size();
    r.cam_intr = cam_intr.data(); r.obs_cam = obs_cam.data(); r.obs_lm = obs_lm.data();
    r.n_bodies = (int)body_fixed.size(); r.body_fixed = body_fixed.data(); r.cam_body = cam_body.data(); r.T_b_c = kTbc;
    return r;
  }
};

static bool read_problem(Problem& p) {
  int B, C, O, v;
  if (scanf("%d", &B) != 1) return false;
  for (int i = 0; i < B; i++) { if (scanf("%d", &v) != 1) return false; p.body_fixed.push_back((uint8_t)v); }
  if (scanf("%d", &C) != 1) return false;
  for (int i = 0; i < C; i++) { if (scanf("%d", &v) != 1) return false; p.cam_body.push_back(v); }
  for (int i = 0; i < C; i++) { if (scanf("%d", &v) != 1) return false; p.cam_intr.push_back(v); }
  if (scanf("%d %d", &p.n_lms, &O) != 2) return false;
  for (int i = 0; i < O; i++) { if (scanf("%d", &v) != 1) return false; p.obs_cam.push_back(v); }
  for (int i = 0; i < O; i++) { if (scanf("%d", &v) != 1) return false; p.obs_lm.push_back(v); }
  return true;
}

static void line(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

// The lists from their definitions, with maps and sets and no shared code: slot numbering, then for every sorted
// observation the (landmark, slot) pairs it belongs to.
static bool brute_force_equal(const Problem& p, const uint8_t* ef, const RigPlan& base, const RigExtPlan& x) {
  const int B = (int)p.body_fixed.size(), C = (int)p.cam_body.size(), O = (int)p.obs_cam.size(), L = p.n_lms;
  std::vector<int> body_slot(B, -1);
  int ns = 0;
  for (int b = 0; b < B; b++)
    if (!p.body_fixed[b]) body_slot[b] = ns++;
  const int nfb = ns;
  int es[2] = {-1, -1};
  for (int k = 0; k < 2; k++)
    if (ef[k]) es[k] = ns++;
  if (x.n_slots != ns || x.n_ext != ns - nfb || x.ext_slot[0] != es[0] || x.ext_slot[1] != es[1]) return false;
  for (int c = 0; c < C; c++)
    if (x.cam_eslot[c] != es[p.cam_intr[c]]) return false;
  for (int b = 0; b < B; b++)
    if (x.pose_free[b] != body_slot[b]) return false;
  if (x.pose_free[B] != es[0] || x.pose_free[B + 1] != es[1]) return false;
  // (landmark, slot) -> sorted observation numbers (ascending: q runs upwards)
  std::map<std::pair<int, int>, std::vector<int>> groups;
  std::vector<std::vector<int>> slot_obs(ns);
  for (int q = 0; q < O; q++) {
    const int cam = base.obs_cam[q], l = base.obs_lm[q];
    if (cam != p.obs_cam[base.perm[q]] || l != p.obs_lm[base.perm[q]]) return false;
    const int sb = body_slot[p.cam_body[cam]], se = es[p.cam_intr[cam]];
    if (sb >= 0) { groups[{l, sb}].push_back(q); slot_obs[sb].push_back(q); }
    if (se >= 0) { groups[{l, se}].push_back(q); slot_obs[se].push_back(q); }
  }
  if ((int)groups.size() != x.n_groups()) return false;
  int g = 0;
  std::vector<std::vector<int>> slot_grp(ns), slot_lm(ns);
  std::vector<int> per_lm(L + 1, 0);
  for (const auto& kv : groups) {  // the map's order IS ascending landmark, then ascending slot
    if (x.grp_lm[g] != kv.first.first || x.grp_slot[g] != kv.first.second) return false;
    if (std::vector<int>(x.grp_obs.begin() + x.grp_first[g], x.grp_obs.begin() + x.grp_first[g + 1]) != kv.second) return false;
    slot_grp[kv.first.second].push_back(g);
    slot_lm[kv.first.second].push_back(kv.first.first);
    per_lm[kv.first.first + 1]++;
    g++;
  }
  for (int l = 0; l < L; l++) {
    per_lm[l + 1] += per_lm[l];
    if (x.lm_grp[l + 1] != per_lm[l + 1]) return false;
  }
  for (int s = 0; s < ns; s++) {
    if (std::vector<int>(x.sg_grp.begin() + x.sg_start[s], x.sg_grp.begin() + x.sg_start[s + 1]) != slot_grp[s]) return false;
    if (std::vector<int>(x.sg_lm.begin() + x.sg_start[s], x.sg_lm.begin() + x.sg_start[s + 1]) != slot_lm[s]) return false;
    if (std::vector<int>(x.so_obs.begin() + x.so_start[s], x.so_obs.begin() + x.so_start[s + 1]) != slot_obs[s]) return false;
  }
  // the body slots' lists are the rig plan's own
  for (int s = 0; s < nfb; s++) {
    if (x.so_start[s + 1] - x.so_start[s] != base.bo_start[s + 1] - base.bo_start[s]) return false;
    for (int k = 0; k < base.bo_start[s + 1] - base.bo_start[s]; k++)
      if (x.so_obs[x.so_start[s] + k] != base.bo_obs[base.bo_start[s] + k]) return false;
  }
  return true;
}

static int sweep() {
  std::mt19937 rng(11);
  long checked = 0, groups = 0, no_free_body = 0, refused = 0;
  for (int B = 1; B <= 7; B++)
    for (int fixed_mode = 0; fixed_mode < 4; fixed_mode++)  // none fixed, the first, random, ALL fixed
      for (int L : {1, 2, 7, 33})
        for (int e = 1; e < 4; e++)
          for (int rep = 0; rep < 3; rep++) {
            Problem p;
            p.n_lms = L;
            for (int b = 0; b < B; b++)
              p.body_fixed.push_back(fixed_mode == 0 ? 0 : (fixed_mode == 1 ? b == 0 : (fixed_mode == 2 ? rng() % 2 : 1)));
            for (int b = 0; b < B; b++) {
              const int which = rng() % 3;  // both cameras, only block 0, only block 1
              if (which != 2) { p.cam_body.push_back(b); p.cam_intr.push_back(0); }
              if (which != 1) { p.cam_body.push_back(b); p.cam_intr.push_back(1); }
            }
            const int C = (int)p.cam_body.size();
            for (int l = 0; l < L; l++)
              for (int c = 0; c < C; c++)
                if (rng() % 3) { p.obs_cam.push_back(c); p.obs_lm.push_back(l); }
            if (p.obs_cam.empty()) { p.obs_cam.push_back(0); p.obs_lm.push_back(0); }
            for (size_t i = p.obs_cam.size(); i > 1; i--) {  // the caller's order is arbitrary
              const size_t j = rng() % i;
              std::swap(p.obs_cam[i - 1], p.obs_cam[j]);
              std::swap(p.obs_lm[i - 1], p.obs_lm[j]);
            }
            const uint8_t ef[2] = {(uint8_t)(e & 1), (uint8_t)(e >> 1)};
            RigPlan base;
            RigExtPlan x;
            const RigPlanIn in = p.in();
            const int st = rig_ext_plan_build(in, ef, base, x);
            bool carried[2] = {false, false};
            for (int c = 0; c < C; c++) carried[p.cam_intr[c]] = true;
            const bool want_refused = (ef[0] && !carried[0]) || (ef[1] && !carried[1]);
            if (want_refused) {
              if (st != RIG_PLAN_EXT_NO_CAMERA) { fprintf(stderr, "a free block without a camera passed (B %d L %d)\n", B, L); return 1; }
              refused++;
              continue;
            }
            if (st != RIG_PLAN_OK) { fprintf(stderr, "status %d (B %d L %d mode %d)\n", st, B, L, fixed_mode); return 1; }
            if (!rig_plan_check(in, base) || !rig_ext_plan_check(in, base, x) || !brute_force_equal(p, ef, base, x)) {
              fprintf(stderr, "plan differs from the brute-force construction (B %d L %d mode %d blocks %d)\n", B, L, fixed_mode, e);
              return 1;
            }
            if (base.n_free == 0) {  // the empty lists of calibration against fixed poses
              if (!base.bo_obs.empty() || !base.bg_grp.empty() || x.so_start[0] != 0 || x.n_slots != x.n_ext) return 1;
              no_free_body++;
            }
            checked++;
            groups += x.n_groups();
          }
  printf("checked %ld groups %ld no_free_body %ld refused %ld\n", checked, groups, no_free_body, refused);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc < 4) return 2;
  const uint8_t ef[2] = {(uint8_t)atoi(argv[2]), (uint8_t)atoi(argv[3])};
  Problem p;
  if (!read_problem(p)) return 2;
  RigPlan base;
  RigExtPlan x;
  const RigPlanIn in = p.in();
  const int st = rig_ext_plan_build(in, ef, base, x);
  if (!strcmp(argv[1], "check")) {
    printf("%d %d\n", st, base.first_bad);
    return 0;
  }
  if (st != RIG_PLAN_OK || !rig_ext_plan_check(in, base, x) || !brute_force_equal(p, ef, base, x)) return 1;
  printf("dims %d %d %d\n", x.n_slots, x.n_ext, x.n_groups());
  line("ext_slot", {x.ext_slot[0], x.ext_slot[1]});
  line("cam_eslot", x.cam_eslot);
  line("pose_free", x.pose_free);
  line("lm_grp", x.lm_grp);
  line("grp_lm", x.grp_lm);
  line("grp_slot", x.grp_slot);
  line("grp_first", x.grp_first);
  line("grp_obs", x.grp_obs);
  line("sg_start", x.sg_start);
  line("sg_grp", x.sg_grp);
  line("sg_lm", x.sg_lm);
  line("so_start", x.so_start);
  line("so_obs", x.so_obs);
  return 0;
}
