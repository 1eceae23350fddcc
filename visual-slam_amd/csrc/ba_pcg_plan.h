// ba_pcg_plan.h -- what the host alone decides about the matrix-free PCG on the reduced camera system (ba_pcg.h,
// DESIGN.md section 22): the stopping rule's numbers and the cadence of the host's polls.  Plain C++
// (tests/cpp/ba_pcg_plan_test.cpp drives it on the CPU); the kernels and their launchers are in ba_pcg.h / ba_session.hip.
#pragma once
#include <climits>
#include <cmath>

// the record a solve keeps on the device; the host reads it once per batch of enqueued iterations
enum : int { BPCG_RUNNING = 0, BPCG_CONVERGED = 1, BPCG_NUMERIC = 2, BPCG_CAP = 3 };
struct BpcgRec {
  double rho, alpha, beta, bb, rr, tol2, pq, pad0;
  int done, status, iterations, max_it, pivot_fail, pad1[3];
};

constexpr double BA_PCG_DEFAULT_TOL = 0.1;  // inexact-Newton forcing term: the default eta of the Ceres solver this replaces
constexpr int BA_PCG_DEFAULT_POLL = 8, BA_PCG_MAX_POLL = 1024;
constexpr int BA_PCG_MAX_TOL_EXP = 15;  // 1e-15: below it the test ||r|| <= tau ||b|| asks more than fp64 holds

// iteration cap of a solve with n unknowns: exact arithmetic needs at most n, the factor 4 is headroom for rounding
inline int ba_pcg_cap(long long n) {
  if (n <= 0) return 0;
  return 4 * n > (long long)INT_MAX ? INT_MAX : (int)(4 * n);
}

// tau of the solver loop from the diagnostic "ba_pcg_tol_exp": 0 (unset) = the forcing term, e > 0 = 10^-e
inline double ba_pcg_tol_of_exp(int e) {
  if (e <= 0) return BA_PCG_DEFAULT_TOL;
  if (e > BA_PCG_MAX_TOL_EXP) e = BA_PCG_MAX_TOL_EXP;
  return std::pow(10.0, -e);
}

// iterations the host enqueues between two reads of the record (diagnostic "ba_pcg_poll"; 0 = default)
inline int ba_pcg_poll_of(int k) {
  if (k <= 0) return BA_PCG_DEFAULT_POLL;
  return k > BA_PCG_MAX_POLL ? BA_PCG_MAX_POLL : k;
}

// Most batches a solve can take: the device stops counting at `cap`, and every batch that is not the last one ran
// `poll` live iterations.  The host loop is bounded by this as well, so that a record that never reports `done`
// (which the kernels do not produce) cannot keep it enqueueing.
inline long long ba_pcg_max_batches(int cap, int poll) {
  if (cap <= 0) return 0;
  return ((long long)cap + poll - 1) / poll;
}

// what the host makes of a record it has read: relative residual ||r|| / ||b|| (0 for b = 0)
inline double ba_pcg_rel_residual(const BpcgRec& r) {
  if (!(r.bb > 0.0)) return 0.0;
  return std::sqrt(r.rr / r.bb);
}
