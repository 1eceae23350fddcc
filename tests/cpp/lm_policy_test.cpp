// Drives visual-slam_amd/csrc/lm_policy.h (as plain C++) with a scripted sequence of step outcomes, through a loop of
// the shape every solver has, and prints what the policy did; tests/test_lm_policy_cpu.py holds the expected values.
//
// stdin:  max_iterations initial_cost
//         gmax step_ok cand_cost model_change step_norm x_norm        (one line per step; hex floats allowed)
// stdout: one line per judged step: verdict radius decrease invalid cost_change rel   (doubles as %a)
//         last line: end iterations termination successful_steps cost radius
#include <cstdio>
#include <cstdlib>

#include "lm_policy.h"

int main() {
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
