// guided_search.h -- the device logic of landmark projection and guided descriptor matching, each piece once: the
// kernels of vo.hip (per-frame tracking, the two host-buffer operators and the all-views search of landmark fusion) say
// where their operands come from and call these.
//
//   project_in_view       world point -> camera frame -> project_exact -> z / image-bounds test (vo_utils.h:48-81)
//   wg1024_ordered_slot   order-preserving compaction inside one 1024-thread workgroup
//   guided_search_wave    one wavefront per keypoint (vo_utils.h:83-167): the 2-D radius test, the per-landmark minimum
//                         Hamming distance, the reference's top-2 selection and its threshold / second-best decision
//   sqrt_less_threshold   host side of the radius test
#pragma once
#include <cmath>

#include "cam_device.h"  // quat_rotate_d, project_exact
#include "vsl_common.h"

namespace {

// p (world) seen from `pose` (qx qy qz qw tx ty tz, camera -> world): fp64 in the oracle's operation order, operand for
// operand (no FMA: -ffp-contract=off); true when the point is kept, u / v as the oracle leaves them (bit patterns).
__device__ __forceinline__ bool project_in_view(const double* __restrict__ pose, int model, const double* __restrict__ intr,
                                                int width, int height, const double* __restrict__ p, double z_thr, double& u,
                                                double& v) {
  const double qi[4] = {-pose[0], -pose[1], -pose[2], pose[3]};
  const double nt[3] = {pose[4] * -1.0, pose[5] * -1.0, pose[6] * -1.0};
  double ti[3], rp[3];
  quat_rotate_d(qi, nt, ti);
  quat_rotate_d(qi, p, rp);
  const double pc[3] = {rp[0] + ti[0], rp[1] + ti[1], rp[2] + ti[2]};
  u = 0;
  v = 0;
  if (pc[2] < z_thr) return false;
  project_exact(model, intr, pc[0], pc[1], pc[2], u, v);
  return !(u > (double)width || v > (double)height || u < 0 || v < 0);
}

// For a 1024-thread workgroup: the rank of this thread's `ok` among the workgroup's `ok`s in thread order, and their
// number.  The sixteen wave totals live in LDS until the next call rewrites them: a caller that loops puts a
// __syncthreads() between two calls.
__device__ __forceinline__ int wg1024_ordered_slot(bool ok, int& total) {
  __shared__ int wave_tot[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(ok);
  if (lane == 0) wave_tot[wave] = __popcll(m);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < 16; w++) {
    const int t = wave_tot[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

// One wavefront matches one keypoint (position kx, ky, descriptor d) against the n_proj compacted projections
// proj_uv / proj_lm; landmark l owns the observation descriptors obs_desc[o], o in [lm_obs_start[l], lm_obs_start[l + 1]),
// read through obs_index[o] when obs_index is given (wave-uniform).  Returns the matched landmark or -1, in every lane.
//
// Lanes test 64 projected points at a time against the 2-D radius.  The reference tests (p_2d - kp).norm() <
// match_max_dist_2d (vo_utils.h:108, Eigen's norm(): sqrt(dx*dx + dy*dy)); max_dist_sq is the host-computed double T with
// sqrt(x) < match_max_dist_2d <=> x < T for every x >= 0 (sqrt_less_threshold below): the same decisions bit for bit
// without ~40 instructions of fp64 square root per lane and chunk.  For every hit, in ascending projected position, the
// lanes stride the landmark's observation descriptors and a wave-wide minimum gives the landmark distance.
//
// The reference then calls std::partial_sort(first, first + 2, last) on the (landmark, distance) list; which of two
// EQUALLY distant landmarks comes first is libstdc++'s heap-select behaviour, reproduced here as the equivalent streaming
// state machine over the list:
//     first two:   top = (d1 < d0) ? e0 : e1,  other = the other one
//     each later e with d(e) < d(top):   (top, other) = d(other) < d(e) ? (e, other) : (other, e)
//     result[0] = other, result[1] = top
// so ties are broken exactly like the reference (pinned against the oracle, which calls the real std::partial_sort).
__device__ __forceinline__ int guided_search_wave(double kx, double ky, const uint32_t (&d)[8],
                                                  const double* __restrict__ proj_uv, const int32_t* __restrict__ proj_lm,
                                                  int n_proj, const int32_t* __restrict__ lm_obs_start,
                                                  const uint64_t* __restrict__ obs_desc, const int32_t* __restrict__ obs_index,
                                                  double max_dist_sq, int threshold, double dist_2_best, int lane) {
  int count = 0, top_d = 0, other_d = 0, other_id = 0;
  for (int base = 0; base < n_proj; base += 64) {
    const int j = base + lane;
    bool hit = false;
    if (j < n_proj) {
      const double dx = kx - proj_uv[2 * (size_t)j], dy = ky - proj_uv[2 * (size_t)j + 1];
      hit = dx * dx + dy * dy < max_dist_sq;
    }
    unsigned long long mask = __ballot(hit);
    while (mask) {
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int l = proj_lm[base + b];
      const int o0 = lm_obs_start[l], o1 = lm_obs_start[l + 1];
      int best = 256;  // minimal_dist, vo_utils.h:116
      for (int o = o0 + lane; o < o1; o += 64) {
        const uint32_t* od = (const uint32_t*)(obs_desc + 4 * (size_t)(obs_index ? obs_index[o] : o));
        int dist = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) dist += __builtin_popcount(d[q] ^ od[q]);
        best = min(best, dist);
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) best = min(best, __shfl_xor(best, s));
      if (count == 0) {
        other_d = best;
        other_id = l;
      } else if (count == 1) {
        // e0 = (other_id, other_d) so far, e1 = (l, best)
        if (best < other_d) {  // d1 < d0: top = e0, other = e1
          top_d = other_d;
          other_d = best;
          other_id = l;
        } else {  // top = e1, other = e0
          top_d = best;
        }
      } else if (best < top_d) {
        if (other_d < best) {
          top_d = best;
        } else {
          top_d = other_d;
          other_d = best;
          other_id = l;
        }
      }
      count++;
    }
  }
  if (count == 0 || other_d >= threshold) return -1;
  const double second = count < 2 ? 256.0 : (double)top_d;  // vo_utils.h:146-160
  return second < (double)other_d * dist_2_best ? -1 : other_id;
}

// The smallest double T with !(sqrt(T) < m): for x >= 0, sqrt(x) < m <=> x < T, because the correctly rounded square
// root is monotone (host libm and the device's fp64 sqrt are both correctly rounded).  Bisection over the bit patterns
// of the non-negative doubles (they order like the values).
static inline double sqrt_less_threshold(double m) {
  if (!(m > 0.0)) return 0.0;  // sqrt(x) < m never holds for x >= 0
  if (std::isinf(m)) return m;
  uint64_t lo = 0, hi;          // invariant: sqrt(value(lo)) < m, !(sqrt(value(hi)) < m)
  {
    const double inf = INFINITY;
    memcpy(&hi, &inf, 8);
  }
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    double v;
    memcpy(&v, &mid, 8);
    if (std::sqrt(v) < m) lo = mid; else hi = mid;
  }
  double T;
  memcpy(&T, &hi, 8);
  return T;
}

}  // namespace
