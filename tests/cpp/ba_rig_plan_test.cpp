// Drives visual-slam_amd/csrc/ba_rig_plan.h on the CPU (plain C++, no HIP): tests/test_ba_rig_plan_cpu.py.
//   ba_rig_plan_test plan  < problem   prints the plan's arrays, one "name v v v" line each, after checking its properties
//   ba_rig_plan_test check < problem   prints "status first_bad"
//   ba_rig_plan_test sweep             random problems of many shapes: every plan must hold rig_plan_check
// problem: n_bodies / body_fixed / n_cams / cam_body / cam_intr / n_lms / n_obs / obs_cam / obs_lm, whitespace separated;
// the extrinsics are fixed here (block 0 the identity, block 1 a quarter turn about z and a shift).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "ba_rig_plan.h"

static const double kTbc[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, std::sqrt(0.5) * 2, std::sqrt(0.5) * 2, 1, 2, 3};  // block 1 unnormalised on purpose

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

static int sweep() {
  std::mt19937 rng(7);
  long checked = 0, groups = 0, doubles = 0;
  for (int B = 1; B <= 9; B++)
    for (int fixed_mode = 0; fixed_mode < 3; fixed_mode++)
      for (int L : {1, 2, 7, 33})
        for (int rep = 0; rep < 4; rep++) {
          Problem p;
          p.n_lms = L;
          for (int b = 0; b < B; b++) p.body_fixed.push_back(fixed_mode == 0 ? 0 : (fixed_mode == 1 ? (b == 0 && B > 1) : (rng() % 2 && b + 1 < B)));
          for (int b = 0; b < B; b++) {
            const int which = rng() % 3;  // both cameras, only block 0, only block 1
            if (which != 2) { p.cam_body.push_back(b); p.cam_intr.push_back(0); }
            if (which != 1) { p.cam_body.push_back(b); p.cam_intr.push_back(1); }
          }
          const int C = (int)p.cam_body.size();
          for (int l = 0; l < L; l++)
            for (int c = 0; c < C; c++) {
              const int times = rng() % 4 == 0 ? 0 : (rng() % 9 == 0 ? 2 : 1);  // missing, once, the same camera twice
              for (int t = 0; t < times; t++) { p.obs_cam.push_back(c); p.obs_lm.push_back(l); }
            }
          if (p.obs_cam.empty()) { p.obs_cam.push_back(0); p.obs_lm.push_back(0); }
          // the caller's order is arbitrary
          for (size_t i = p.obs_cam.size(); i > 1; i--) {
            const size_t j = rng() % i;
            std::swap(p.obs_cam[i - 1], p.obs_cam[j]);
            std::swap(p.obs_lm[i - 1], p.obs_lm[j]);
          }
          RigPlan plan;
          const RigPlanIn in = p.in();
          if (rig_plan_build(in, plan) != RIG_PLAN_OK || !rig_plan_check(in, plan)) {
            fprintf(stderr, "sweep: plan of B=%d fixed_mode=%d L=%d rep=%d fails\n", B, fixed_mode, L, rep);
            return 1;
          }
          checked++;
          groups += plan.n_groups();
          for (int g = 0; g < plan.n_groups(); g++) doubles += plan.grp_end[g] - plan.grp_begin[g] >= 2;
        }
  printf("checked %ld groups %ld multi %ld\n", checked, groups, doubles);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "sweep")) return sweep();
  Problem p;
  if (!read_problem(p)) return 2;
  const RigPlanIn in = p.in();
  RigPlan plan;
  const int st = rig_plan_build(in, plan);
  if (!strcmp(argv[1], "check")) {
    printf("%d %d\n", st, plan.first_bad);
    return 0;
  }
  if (st != RIG_PLAN_OK || !rig_plan_check(in, plan)) return 1;
  printf("dims %d %d %d\n", plan.n_free, plan.n_fixed, plan.n_groups());
  line("body_slot", plan.body_slot);
  line("free_bodies", plan.free_bodies);
  line("cam_slot", plan.cam_slot);
  line("perm", plan.perm);
  line("lm_start", plan.lm_start);
  line("lm_grp", plan.lm_grp);
  line("grp_lm", plan.grp_lm);
  line("grp_slot", plan.grp_slot);
  line("grp_begin", plan.grp_begin);
  line("grp_end", plan.grp_end);
  line("bg_start", plan.bg_start);
  line("bg_grp", plan.bg_grp);
  line("bg_lm", plan.bg_lm);
  line("bo_start", plan.bo_start);
  line("bo_obs", plan.bo_obs);
  // extrinsics: block 1's quaternion normalised, T_c_b T_b_c = identity to rounding
  double worst = 0;
  for (int k = 0; k < 2; k++) {
    const double* q = plan.T_b_c + 7 * k;
    const double* o = plan.T_c_b + 12 * k;
    worst = std::fmax(worst, std::fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0));
    for (int i = 0; i < 3; i++) worst = std::fmax(worst, std::fabs(o[3 * i] * q[4] + o[3 * i + 1] * q[5] + o[3 * i + 2] * q[6] + o[9 + i]));
  }
  printf("extrinsic_error_below_1e-15 %d\n", worst < 1e-15 ? 1 : 0);
  return 0;
}
