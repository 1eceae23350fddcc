// chol_plan.h -- everything the SPD solvers of chol.hip decide on the host: which solver takes a system, the storage
// arithmetic their callers need, the split of the two-ended form and the schedule of the block cyclic reduction.  Plain
// C++17, no HIP (vsl_common.h includes it; ba_host_plan.h and tests/cpp/chol_plan_test.cpp use it on their own).
//   chol_choose           THE rule: dense / band panels, fused, two-ended, block cyclic reduction (chain or ring)
//   chol_ring_available   may a caller lay a cyclic band out for the ring solver at all
//   chol_two_ended_plan   chunks, separator and scratch of the two-ended form
//   bcr_plan_build        block layout, level lists, product targets, scratch and device block of a reduction
//   chol_fold_plan        a cyclic band folded into a linear one (selected inversion: the ring is never inverted as such)
//   chol_selinv_plan      launches and scratch of the selected inversion
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "../../include/vslam_hip.h"  // VSL_SPD_PATH_*

// LAPACK-style lower band storage (chol.hip, "BAND FORM"): S = storage + bws, ld = bws = bw + VSL_CHOL_NB
#define VSL_CHOL_NB 32
#define BCR_MAXB 256   // block size limit of the cyclic reduction: static LDS Us[256][33] + Lp[32][257] = 133 KB (dynamic LDS above 64 KiB is refused by the runtime)
#define CBF_MAXBW 512  // widest band of the single-workgroup kernels (their LDS window holds 32 + CBF_MAXBW + 1 rows)

// Block layout of the cyclic form: nblk blocks of floor / ceil (n / nblk) unknowns, every one >= bw + 1 (a block couples
// with its two ring neighbours only) and <= B (the kernels' block size, a multiple of 32 <= BCR_MAXB).  false: no such layout.
inline bool vsl_chol_bcr_cyclic_layout(int n, int bw, int* B_out, int* nblk_out) {
  const int most = n / (bw + 1);  // blocks of >= bw + 1 unknowns each
  for (int B = (bw + 1 + 31) / 32 * 32; B <= BCR_MAXB; B += 32) {
    const int nblk = std::max(8, (n + B - 1) / B);  // the fewest blocks of <= B unknowns (fewer blocks: fewer levels)
    if (nblk <= most) {
      *B_out = B;
      *nblk_out = nblk;
      return true;
    }
  }
  return false;
}

// ------------------------------------------------------------------------------------------------ which solver
struct CholSwitches {  // the context's diagnostics "chol_no_fused", "chol_no_bcr", "chol_one_ended"
  bool no_fused = false, no_bcr = false, one_ended = false;
};

struct CholChoice {
  int path = VSL_SPD_PATH_NONE;
  int B = 0, nblk = 0, levels = 0;  // the two reductions: block size, blocks, levels (every level keeps ceil(m / 2) of m blocks)
};

inline int bcr_level_count(int nblk) {
  int levels = 0;
  for (; nblk > 1; nblk = (nblk + 1) / 2) levels++;
  return levels;
}

// The test entry points' reading of a declared half bandwidth: band storage, unless the band is the whole matrix.
inline bool chol_band_declared(int n, int half_bandwidth) { return half_bandwidth >= 0 && half_bandwidth < n - 1; }

// The solver of n unknowns with half bandwidth bw.  band: LAPACK-style band storage (else dense, bw = n).  cyclic: the
// band closes on itself and the caller has laid it out for the ring (chol_ring_available); path NONE: there is no ring.
inline CholChoice chol_choose(int n, bool band, int bw, bool cyclic, const CholSwitches& sw) {
  CholChoice c;
  if (cyclic) {
    if (!vsl_chol_bcr_cyclic_layout(n, bw, &c.B, &c.nblk)) return c;
    c.path = VSL_SPD_PATH_BCR_CYCLIC;
    c.levels = bcr_level_count(c.nblk);
    return c;
  }
  if (!band) {
    c.path = VSL_SPD_PATH_DENSE_PANELS;
    return c;
  }
  const int B = (bw + 1 + 31) / 32 * 32;
  if (!sw.no_fused && !sw.no_bcr && B <= BCR_MAXB && n >= 8 * B) {  // long narrow band: the reduction spreads over the whole chip
    c.path = VSL_SPD_PATH_BCR;
    c.B = B;
    c.nblk = (n + B - 1) / B;
    c.levels = bcr_level_count(c.nblk);
  } else if (sw.no_fused || bw > CBF_MAXBW) {
    c.path = VSL_SPD_PATH_BAND_PANELS;  // one launch per panel step
  } else if (!sw.one_ended && bw + VSL_CHOL_NB - 1 <= CBF_MAXBW && n >= 8 * (bw + VSL_CHOL_NB)) {
    c.path = VSL_SPD_PATH_BAND_TWO_ENDED;  // (the separator system, bw .. bw + 31 unknowns, is solved by the fused kernel)
  } else {
    c.path = VSL_SPD_PATH_BAND_FUSED;
  }
  return c;
}

// Would a solve of the cyclic band (n, bw) take the ring?  What the layouts of the bundle adjustment and of the pose
// graph ask before they order a camera loop along its trajectory; their own conditions (is the ring narrower) stay theirs.
inline bool chol_ring_available(int n, int bw, const CholSwitches& sw, int* B_out, int* nblk_out) {
  return !sw.no_bcr && !sw.no_fused && vsl_chol_bcr_cyclic_layout(n, bw, B_out, nblk_out);
}

// ------------------------------------------------------------------------------------------------ two-ended form
// Top chunk [0, s), bottom chunk [n - sp, n) (both whole panels), separator [s, s + sepn) with bw <= sepn <= bw + 31,
// solved as a dense system in band storage of its own (half bandwidth bwm, leading dimension ldm).  Scratch offsets in
// doubles: per-view intermediate vectors and reciprocal pivots, the bottom chunk's update of the separator (M3, then
// b3: cleared together), the separator system (bm, ym, dinvm, band storage Am_store of mid_elems doubles: cleared).
struct TwoEndedPlan {
  int s, sp, sepn, bwm, ldm;
  size_t mid_elems;
  size_t y_top, dinv_top, y_rev, dinv_rev, M3, b3, bm, ym, dinvm, Am_store, doubles;
};

inline TwoEndedPlan chol_two_ended_plan(int n, int bw) {
  TwoEndedPlan t;
  t.s = ((n - bw) / 2) / VSL_CHOL_NB * VSL_CHOL_NB;
  t.sp = (n - t.s - bw) / VSL_CHOL_NB * VSL_CHOL_NB;
  t.sepn = n - t.s - t.sp;
  t.bwm = t.sepn - 1;
  t.ldm = t.bwm + VSL_CHOL_NB;
  t.mid_elems = (size_t)t.sepn * (t.ldm + 1) + 64;
  const size_t N = (size_t)n, sepn = (size_t)t.sepn;
  t.y_top = 0;
  t.dinv_top = N;
  t.y_rev = 2 * N;
  t.dinv_rev = 3 * N;
  t.M3 = 4 * N;
  t.b3 = t.M3 + sepn * sepn;
  t.bm = t.b3 + sepn;
  t.ym = t.bm + sepn;
  t.dinvm = t.ym + sepn;
  t.Am_store = t.dinvm + sepn;
  t.doubles = t.Am_store + t.mid_elems + 64;
  return t;
}

// ------------------------------------------------------------------------------------------------ selected inversion
// The band of the inverse (chol.hip, "SELECTED INVERSION") exists for LINEAR bands only.  A cyclic band is FOLDED into a
// linear one instead of being inverted on the ring solver's reduction: ring position p goes to 2 p on the way out
// (p < ceil(n / 2)) and to 2 (n - 1 - p) + 1 on the way back, so the two halves of the ring interleave and two positions
// at cyclic distance d land at most 2 d apart.  A diagonal block of the inverse does not move under the relabelling.
inline int chol_fold_pos(int n, int p) { return p < (n + 1) / 2 ? 2 * p : 2 * (n - 1 - p) + 1; }

struct FoldPlan {
  int n = 0;
  int bw = 0;       // linear half bandwidth of the folded matrix: min(2 * cyclic half bandwidth, n - 1)
  bool band = false;  // the folded band is narrower than the matrix (chol_band_declared): else the caller inverts densely
  std::vector<int> pos;   // ring position -> folded position
  std::vector<int> ring;  // folded position -> ring position
};

inline FoldPlan chol_fold_plan(int n, int cyclic_bw) {
  FoldPlan f;
  f.n = n;
  f.bw = std::max(0, std::min(2 * cyclic_bw, n - 1));
  f.band = chol_band_declared(n, 2 * cyclic_bw);
  f.pos.resize(n);
  f.ring.resize(n);
  for (int p = 0; p < n; p++) {
    f.pos[p] = chol_fold_pos(n, p);
    f.ring[f.pos[p]] = p;
  }
  return f;
}

// How the recurrence of the selected inversion is launched: bands the single-workgroup kernels take run all panel steps
// in ONE launch; wider ones go panel by panel (three launches per step, the products spread over several workgroups).
// scratch_doubles: the inverted diagonal blocks, then G = L_WK L_KK^-1 of the current step (window rows x VSL_CHOL_NB).
struct SelinvPlan {
  int n_panels = 0;
  bool fused = false;
  int window = 0;  // most rows below a panel that a step reaches: min(bw, n - VSL_CHOL_NB), at least 0
  size_t Linv = 0, G = 0, scratch_doubles = 0;
  size_t z_elems = 0;  // doubles of a band array of this system: n rows of bw + VSL_CHOL_NB + 1 slots, plus 64
};

inline SelinvPlan chol_selinv_plan(int n, int bw, bool no_fused) {
  SelinvPlan s;
  s.n_panels = (n + VSL_CHOL_NB - 1) / VSL_CHOL_NB;
  s.fused = !no_fused && bw <= CBF_MAXBW;
  s.window = std::max(0, std::min(bw, n - VSL_CHOL_NB));
  s.Linv = 0;
  s.G = (size_t)s.n_panels * VSL_CHOL_NB * VSL_CHOL_NB;
  s.scratch_doubles = s.G + (size_t)(s.window + 16) * VSL_CHOL_NB + 16;
  s.z_elems = (size_t)n * (bw + VSL_CHOL_NB + 1) + 64;
  return s;
}

// ------------------------------------------------------------------------------------------------ cyclic reduction
struct BcrJob {
  int e, p, q;      // eliminated block and its two active neighbours (q = -1: none below)
  int kp, kq;       // indices of K(e, p) and K(q, e) in this level's coupling array
  int knew;         // index of K(q, p) in the next level's coupling array (-1: none)
  int u;            // slot of U1 / U2
};

struct BcrTarget {
  int c_is_k, c_idx;  // destination: Knext[c_idx] (assigned) or D[c_idx] (updated, lower tiles)
  int m1, n1;         // first product  M^T N: U block slots (2 u + 0 / 1)
  int m2, n2;         // second product (-1: none)
  int pad0, pad1;
};

// Everything a reduction derives from (n, bw, cyclic).  Block i holds the unknowns [off[i], off[i + 1]).  Level l
// eliminates jobs[job_off[l] .. job_off[l + 1]), its products are targets[tgt_off[l] .. tgt_off[l + 1]) and its ncoup[l]
// couplings start at block k_off[l] of the coupling array; combine: c[0] += c[1]^T before the solves (a ring of two is
// one coupling), carry: c[m - 1] -> the next level's c[m' - 1] (the wrap coupling of an odd ring moves on unchanged).
struct BcrPlan {
  int B = 0, nblk = 0;
  int last = 0;  // the block that remains: the whole solve of what is left
  int n_u = 0;   // eliminated blocks = slots of (U1, U2)
  std::vector<int> off;
  std::vector<int> combine, carry, ncoup;
  std::vector<size_t> job_off, tgt_off, k_off;
  std::vector<BcrJob> jobs;
  std::vector<BcrTarget> targets;
  // scratch, offsets in doubles: D | K (all levels) | U | bb | yy | dinv | pend [nblk][2][B] | Linv (per eliminated block + the last one)
  size_t D = 0, K = 0, U = 0, bb = 0, yy = 0, dinv = 0, pend = 0, Linv = 0, scratch_doubles = 0;
  // device block, offsets in bytes: jobs | targets | off
  size_t dev_targets = 0, dev_off = 0, dev_bytes = 0;

  int levels() const { return (int)ncoup.size(); }
  int level_jobs(int l) const { return (int)(job_off[l + 1] - job_off[l]); }
  int level_targets(int l) const { return (int)(tgt_off[l + 1] - tgt_off[l]); }
};

// false: a cyclic band without a ring layout
inline bool bcr_plan_build(int n, int bw, bool cyclic, BcrPlan* plan) {
  BcrPlan& p = *plan;
  p = BcrPlan();
  p.B = (bw + 1 + 31) / 32 * 32;
  p.nblk = (n + p.B - 1) / p.B;
  if (cyclic && !vsl_chol_bcr_cyclic_layout(n, bw, &p.B, &p.nblk)) return false;
  const int nblk = p.nblk;
  p.off.resize(nblk + 1);
  for (int i = 0; i <= nblk; i++) p.off[i] = cyclic ? (int)((long long)i * n / nblk) : std::min(n, i * p.B);
  std::vector<int> active(nblk), next, slot_of;
  for (int i = 0; i < nblk; i++) active[i] = i;
  size_t n_k = 0;
  while (active.size() > 1) {
    const int m = (int)active.size();
    const bool ring = cyclic && m >= 3;  // a ring of two is handled as a chain with one (combined) coupling
    p.combine.push_back(cyclic && m == 2);
    p.carry.push_back(ring && (m & 1));
    p.job_off.push_back(p.jobs.size());
    p.k_off.push_back(n_k);
    next.clear();
    for (int j = 0; j < m; j++) {
      if (j & 1) {
        BcrJob jb;
        jb.e = active[j];
        jb.p = active[j - 1];
        jb.q = j + 1 < m ? active[j + 1] : (ring ? active[0] : -1);
        jb.kp = j - 1;
        jb.kq = j;
        jb.knew = jb.q >= 0 ? (j - 1) / 2 : -1;
        jb.u = p.n_u++;
        p.jobs.push_back(jb);
      } else {
        next.push_back(active[j]);
      }
    }
    p.ncoup.push_back(cyclic ? m : m - 1);
    n_k += (size_t)p.ncoup.back();
    active = next;
  }
  p.job_off.push_back(p.jobs.size());
  p.last = active[0];
  // product targets per level (bcr_gemm_targets_kernel): the remaining blocks with their one or two updates, the new
  // couplings.  Jobs in block order: the update from the block above (as its q) comes first -- the order of the sum.
  const int levels = p.levels();
  for (int l = 0; l < levels; l++) {
    const size_t t0 = p.targets.size();
    p.tgt_off.push_back(t0);
    slot_of.assign(nblk, -1);
    for (size_t j = p.job_off[l]; j < p.job_off[l + 1]; j++) {
      const BcrJob& jb = p.jobs[j];
      for (int side = 0; side < 2; side++) {
        const int x = side ? jb.q : jb.p, us = 2 * jb.u + side;
        if (x < 0) continue;
        if (slot_of[x] < 0) {
          slot_of[x] = (int)(p.targets.size() - t0);
          p.targets.push_back(BcrTarget{0, x, us, us, -1, -1, 0, 0});
        } else {
          p.targets[t0 + slot_of[x]].m2 = p.targets[t0 + slot_of[x]].n2 = us;
        }
      }
      if (jb.knew >= 0 && l + 1 < levels) p.targets.push_back(BcrTarget{1, jb.knew, 2 * jb.u + 1, 2 * jb.u, -1, -1, 0, 0});
    }
  }
  p.tgt_off.push_back(p.targets.size());
  const size_t B = (size_t)p.B, BB = B * B, NB = (size_t)nblk;
  p.D = 0;
  p.K = p.D + NB * BB;
  p.U = p.K + n_k * BB;
  p.bb = p.U + (size_t)2 * p.n_u * BB;
  p.yy = p.bb + NB * B;
  p.dinv = p.yy + NB * B;
  p.pend = p.dinv + NB * B;
  p.Linv = p.pend + 2 * NB * B;
  p.scratch_doubles = p.Linv + ((size_t)p.n_u + 1) * (B / 32) * 1024 + 16;
  p.dev_targets = ((p.jobs.size() + 1) * sizeof(BcrJob) + 63) / 64 * 64;
  p.dev_off = p.dev_targets + ((p.targets.size() + 1) * sizeof(BcrTarget) + 63) / 64 * 64;
  p.dev_bytes = p.dev_off + sizeof(int) * (NB + 1);
  return true;
}

// One slot on the context: the plan of the last reduction and its device block, kept while (n, bw, cyclic) stay the same.
struct BcrPlanCache {
  BcrPlan plan;
  void* dev = nullptr;  // hipMalloc'ed by chol.hip, freed by ctx.hip
  size_t dev_cap = 0;
  int n = -1, bw = -1, cyclic = -1;  // what `plan` and the contents of `dev` were built for (n = -1: nothing)
};
