// Drives visual-slam_amd/csrc/lm_policy.h (as plain C++) with a scripted sequence of step outcomes, through a loop of
// the shape every solver has, and prints what the policy did; tests/test_lm_policy_cpu.py holds the expected values.
//
// stdin:  max_iterations initial_cost
//         gmax step_ok cand_cost model_change step_norm x_norm        (one line per step; hex floats allowed)
// stdout: one line per judged step: verdict radius decrease invalid cost_change rel   (doubles as %a)
//         last line: end iterations termination successful_steps cost radius
//
// With the argument "loop": lm_speculative_loop, the host loop of vsl_bundle_adjust and vsl_bundle_adjust_rig, on
// scripted callables.
// stdin:  max_iterations initial_cost initial_gmax
//         enqueue_rc flag0 flag1 model_change step2 x2 cand_cost cand_gmax   (one line per iteration; step2 / x2: SQUARED norms)
// stdout: "enqueue <radius %a>" / "settle <0|1>" in call order
//         last line: end rc iterations termination successful_steps final_cost   (the four fields as the loop left them:
//         it does not write them on an error)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lm_policy.h"

static int run_loop() {
  int max_iterations = 0;
  double cost = 0, gmax = 0;
  if (scanf("%d %lf %lf", &max_iterations, &cost, &gmax) != 3) return 2;
  int enqueue_rc = 0, flag0 = 0, flag1 = 0;
  double model_change = 0, step2 = 0, x2 = 0, cand_cost = 0, cand_gmax = 0;
  bool short_script = false;
  auto enqueue = [&](double radius) -> int {
    if (scanf("%d %d %d %lf %lf %lf %lf %lf", &enqueue_rc, &flag0, &flag1, &model_change, &step2, &x2, &cand_cost, &cand_gmax) != 8) {
      short_script = true;
      return -99;
    }
    printf("enqueue %a\n", radius);
    return enqueue_rc;
  };
  auto fetch = [&](double* sc, int* flags) -> int {
    for (int k = 0; k < 16; k++) sc[k] = -1.0;  // slots the loop must not read
    sc[2] = model_change; sc[3] = step2; sc[4] = x2; sc[5] = cand_cost; sc[6] = cand_gmax;
    flags[0] = flag0; flags[1] = flag1;
    return 0;
  };
  auto settle = [&](bool accepted) { printf("settle %d\n", accepted ? 1 : 0); };
  LmLoopResult out;
  out.iterations = out.successful_steps = out.termination = -7;
  out.final_cost = -7.0;
  const int rc = lm_speculative_loop(max_iterations, 0, cost, gmax, enqueue, fetch, settle, &out);
  if (short_script) return 3;
  printf("end %d %d %d %d %a\n", rc, out.iterations, out.termination, out.successful_steps, out.final_cost);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "loop")) return run_loop();
  int max_iterations = 0;
  double cost = 0;
  if (scanf("%d %lf", &max_iterations, &cost) != 2) return 2;
  LmState lm;
  int iteration = 0, successful = 0, termination = -1;
  while (true) {
    if (iteration >= max_iterations) { termination = 0; break; }
    double gmax, cand_cost, model_change, step_norm, x_norm;
    int ok;
    if (scanf("%lf %d %lf %lf %lf %lf", &gmax, &ok, &cand_cost, &model_change, &step_norm, &x_norm) != 6) return 3;  // script too short
    if ((termination = lm_gate(lm, gmax)) >= 0) break;
    iteration++;
    LmInfo info;
    const int verdict = lm_judge(lm, ok != 0, cost, cand_cost, model_change, step_norm, x_norm, &info);
    const char* name = verdict == LM_ACCEPTED ? "accepted" : verdict == LM_REJECTED ? "rejected" : verdict == LM_INVALID ? "invalid" : "terminated";
    printf("%s %a %a %d %a %a\n", name, lm.radius, lm.decrease, lm.invalid, info.cost_change, info.rel);
    if (verdict >= 0) { termination = verdict; break; }
    if (verdict == LM_ACCEPTED) {
      cost = cand_cost;
      successful++;
    }
  }
  printf("end %d %d %d %a %a\n", iteration, termination, successful, cost, lm.radius);
  return 0;
}
