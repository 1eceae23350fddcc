// The Levenberg-Marquardt step policy of every solver loop in the library, stated once: the host loops of ba.hip,
// ba_fused.hip and pgo.hip and baf_decide_kernel call these functions (host code, device code, and plain C++ in
// tests/cpp/lm_policy_test.cpp).  The oracle keeps its own restatement on purpose.  [upstream] ceres::Solve, TRUST_REGION /
// LEVENBERG_MARQUARDT, monotonic steps, default options: initial_trust_region_radius 1e4, max_ / min_trust_region_radius
// 1e16 / 1e-32, min_relative_decrease 1e-3, function_ / gradient_ / parameter_tolerance 1e-6 / 1e-10 / 1e-8,
// max_num_consecutive_invalid_steps 5 (max_num_iterations is tested by the caller: its place differs from loop to loop).
#pragma once
#include <cmath>
#include <cstdio>

#if defined(__HIPCC__)
#define LM_HD __host__ __device__
#else
#define LM_HD
#endif

constexpr double LM_INITIAL_RADIUS = 1e4;
constexpr double LM_MAX_RADIUS = 1e16;
constexpr double LM_MIN_RADIUS = 1e-32;
constexpr double LM_MIN_RELATIVE_DECREASE = 1e-3;
constexpr double LM_FUNCTION_TOLERANCE = 1e-6;
constexpr double LM_GRADIENT_TOLERANCE = 1e-10;
constexpr double LM_PARAMETER_TOLERANCE = 1e-8;
constexpr int LM_MAX_INVALID_STEPS = 5;
constexpr double LM_INITIAL_DECREASE = 2.0;  // a rejected step divides the radius by this, then doubles it

struct LmState {
  double radius = LM_INITIAL_RADIUS, decrease = LM_INITIAL_DECREASE;
  int invalid = 0;  // consecutive invalid steps
};
struct LmInfo { double cost_change, rel; };  // for the iteration table (zero where the verdict fell before the value existed)

// Verdicts.  A value >= 0 is a termination code of vsl_ba_summary: 0 max_num_iterations (the caller's), 1 function
// tolerance, 2 gradient tolerance, 3 parameter tolerance, 4 radius below the minimum / too many invalid steps.  Below 0:
// LM_GO (lm_gate) take a step; LM_ACCEPTED the candidate is the new point; LM_REJECTED keep the point, smaller radius;
// LM_INVALID no usable step (factorisation failed, not finite, no model decrease): retry at half the radius.
enum : int { LM_GO = -1, LM_ACCEPTED = -2, LM_REJECTED = -3, LM_INVALID = -4 };

// before a step: gradient tolerance, then the radius
LM_HD inline int lm_gate(const LmState& s, double gmax) {
  if (gmax <= LM_GRADIENT_TOLERANCE) return 2;
  if (s.radius <= LM_MIN_RADIUS) return 4;
  return LM_GO;
}

// (2 rho - 1)^3 of the radius update.  The host loops have always taken it from the C library's pow, the device loop
// from an fma expansion (y^2 = p + pe, p y = q + qe, one final rounding).  The two differ by one ulp for about 0.08 %
// of the arguments the policy produces, and the trajectories are pinned bit for bit, so each side keeps its form.
LM_HD inline double lm_cube(double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double p = y * y, pe = fma(y, y, -p);
  const double q = p * y, qe = fma(p, y, -q);
  return q + (qe + pe * y);
#else
  return pow(y, 3);
#endif
}

// after a step: updates radius / decrease / invalid.  cost, iteration and successful-step counts stay with the caller
// (some loops take the accepted point's cost from their re-linearisation, not from cand_cost).
LM_HD inline int lm_judge(LmState& s, bool step_ok, double cost, double cand_cost, double model_change, double step_norm, double x_norm, LmInfo* info) {
  info->cost_change = info->rel = 0.0;
  if (!step_ok) {
    if (++s.invalid >= LM_MAX_INVALID_STEPS) return 4;
    s.radius *= 0.5;
    return LM_INVALID;
  }
  s.invalid = 0;
  info->cost_change = cost - cand_cost;
  if (step_norm <= LM_PARAMETER_TOLERANCE * (x_norm + LM_PARAMETER_TOLERANCE)) return 3;
  if (fabs(info->cost_change) <= LM_FUNCTION_TOLERANCE * cost) return 1;
  info->rel = info->cost_change / model_change;
  if (info->rel > LM_MIN_RELATIVE_DECREASE) {
    s.radius = s.radius / fmax(1.0 / 3.0, 1.0 - lm_cube(2.0 * info->rel - 1.0));
    s.radius = fmin(LM_MAX_RADIUS, s.radius);
    s.decrease = LM_INITIAL_DECREASE;
    return LM_ACCEPTED;
  }
  s.radius = s.radius / s.decrease;
  s.decrease *= 2.0;
  return LM_REJECTED;
}

// the iteration table of verbosity 2 (host only)
inline void lm_print_header() { fprintf(stderr, "iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n"); }
inline void lm_print_header(double initial_cost) { lm_print_header(); fprintf(stderr, "%4d % .6e\n", 0, initial_cost); }
inline void lm_print_row(int it, double cand_cost, double cost_change, double gmax, double step_norm, double rel, double radius_used) {
  fprintf(stderr, "%4d % .6e % .3e % .3e % .3e % .3e % .3e\n", it, cand_cost, cost_change, gmax, step_norm, rel, radius_used);
}
inline void lm_print_invalid(int iteration, double radius) { fprintf(stderr, "%4d  invalid step, radius %.3e\n", iteration, radius); }
