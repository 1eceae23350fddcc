// The Levenberg-Marquardt step policy of every solver loop in the library, stated once: the host loops of ba.hip,
// ba_fused.hip and pgo.hip and baf_decide_kernel call these functions (host code, device code, and plain C++ in
// tests/cpp/lm_policy_test.cpp).  The oracle keeps its own restatement on purpose.  [upstream] ceres::Solve, TRUST_REGION /
// LEVENBERG_MARQUARDT, monotonic steps, default options: initial_trust_region_radius 1e4, max_ / min_trust_region_radius
// 1e16 / 1e-32, min_relative_decrease 1e-3, function_ / gradient_ / parameter_tolerance 1e-6 / 1e-10 / 1e-8,
// max_num_consecutive_invalid_steps 5 (max_num_iterations is tested by the caller: its place differs from loop to loop).
// lm_speculative_loop at the end is the whole host loop of the two solvers whose loops have one shape (ba.hip's host path,
// ba_rig.hip).
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

// The speculative host loop of vsl_bundle_adjust (ba.hip, "ba_no_fused" and mid-size windows) and vsl_bundle_adjust_rig
// (ba_rig.hip), host only and free of HIP types (tests/cpp/lm_policy_test.cpp drives it with scripted callables).  ONE
// host round trip per iteration:
//   enqueue(radius) -> rc   Schur complement, solve, step, candidate AND the candidate's linearisation into the solver's
//                           second set of blocks, nothing waited for
//   fetch(sc, flags) -> rc  the one copy and synchronisation: sc[2] model cost change, sc[3] / sc[4] squared step / x norms,
//                           sc[5] / sc[6] cost / max |gradient| at the candidate; flags[0] step finite, flags[1]
//                           factorisation succeeded
//   settle(accepted)        after the verdict: the candidate's set becomes the current one, or stays the spare
// cost / gmax: of the starting point.  A non-zero rc of enqueue or fetch is returned at once, out untouched, settle not
// called.
struct LmLoopResult {
  int iterations = 0, successful_steps = 0, termination = 0;
  double final_cost = 0.0;
};

template <class Enqueue, class Fetch, class Settle>
int lm_speculative_loop(int max_num_iterations, int verbosity, double cost, double gmax, Enqueue&& enqueue, Fetch&& fetch,
                        Settle&& settle, LmLoopResult* out) {
  LmState lm;
  LmLoopResult res;
  if (verbosity >= 2) lm_print_header(cost);
  while (true) {
    if (res.iterations >= max_num_iterations) { res.termination = 0; break; }
    const int gate = lm_gate(lm, gmax);
    if (gate >= 0) { res.termination = gate; break; }
    res.iterations++;
    int rc;
    double sc[16];
    int flags[2];
    if ((rc = enqueue(lm.radius))) return rc;
    if ((rc = fetch(sc, flags))) return rc;
    const double model_change = sc[2], step_norm = sqrt(sc[3]), x_norm = sqrt(sc[4]), cand_cost = sc[5];
    const bool ok = flags[0] != 0 && flags[1] != 0 && model_change > 0.0;
    const double radius_used = lm.radius;
    LmInfo info;
    const int verdict = lm_judge(lm, ok, cost, cand_cost, model_change, step_norm, x_norm, &info);
    settle(verdict == LM_ACCEPTED);
    if (verdict >= 0) { res.termination = verdict; break; }
    if (verdict == LM_INVALID) {
      if (verbosity >= 2) lm_print_invalid(res.iterations, lm.radius);
      continue;  // the LM diagonal is reused (the Jacobian is unchanged)
    }
    if (verbosity >= 2) lm_print_row(res.iterations, cand_cost, info.cost_change, gmax, step_norm, info.rel, radius_used);
    if (verdict == LM_ACCEPTED) {
      cost = cand_cost;
      gmax = sc[6];
      res.successful_steps++;
    }
  }
  res.final_cost = cost;
  *out = res;
  return 0;
}
