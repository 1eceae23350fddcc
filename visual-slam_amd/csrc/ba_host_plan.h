// ba_host_plan.h -- the host half of the bundle adjustment's set-up (ba.hip ba_setup): everything it derives from the
// problem before the first byte goes to the device.  Plain C++, no HIP, no vsl_ctx: tests/cpp/ba_host_plan_test.cpp
// drives it under g++.
//   HostTeam            a few threads over one parallel region, with a barrier that counts the threads that exist
//   ba_reduced_layout   dense / linear band / cyclic band storage of the reduced camera system, as a pure function
//   camera_band_order   reverse Cuthill-McKee on the covisibility graph
//   ba_host_plan        free-camera numbering, layout, observations sorted by landmark, both CSRs, landmark runs
//   ba_sub_problem      the observations of a landmark range (a session rank's share)
// Allocation failures leave as std::bad_alloc: the callers in ba.hip turn them into VSL_ERR_NOMEM.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/vslam_hip.h"
#include "chol_plan.h"

// ------------------------------------------------------------------------------------------------ thread team
// Host loops of the set-up on a few threads (the set-up of a 1000-camera solve was ~15 ms of single-threaded loops
// over 881k observations next to LM iterations of 2.5 ms).  Starting the threads costs ~0.4 ms: worth it for the
// global problems only -- a local window of 157k observations went from 6.0 to 8.1 ms per solve with them -- hence
// the size thresholds of the callers.
#define HOST_TEAM_MAX 8
using HostThreadEntry = void (*)(void* team, int t);
using HostThreadStart = std::thread (*)(HostThreadEntry entry, void* team, int t);
inline std::thread host_thread_start(HostThreadEntry entry, void* team, int t) { return std::thread(entry, team, t); }

struct HostTeamConfig {
  int threads = 0;                           // 0: one per hardware thread; either way at most HOST_TEAM_MAX
  HostThreadStart start = host_thread_start;  // every thread start goes through here (tests make it fail; the library never sets it)
};

// run(work) calls work(t, nt) once for every t in [0, nt): t = 0 on the calling thread, the others on threads of their
// own.  nt is the number of threads that EXIST: it is published after the last start, and a started thread waits for
// it before it touches the work.  A start that throws std::system_error (EAGAIN under a thread limit) ends the
// starting: the team is the caller plus the threads it has, down to the caller alone, so barrier() never waits for a
// participant that will not come, and nothing propagates.  work must not throw (the callers allocate before run).
class HostTeam {
 public:
  HostTeam(long long n_items, long long min_parallel, const HostTeamConfig& cfg) : start_(cfg.start) {
    const int hw = (int)std::thread::hardware_concurrency();
    const int want = cfg.threads > 0 ? cfg.threads : (hw > 0 ? hw : 1);
    planned_ = n_items < min_parallel ? 1 : std::max(1, std::min(HOST_TEAM_MAX, want));
  }
  int planned() const { return planned_; }  // upper bound of nt: what per-thread storage is sized by

  template <class Work>
  void run(Work work) {
    work_ = &work;
    call_ = [](void* w, int t, int nt) { (*static_cast<Work*>(w))(t, nt); };
    std::thread th[HOST_TEAM_MAX];
    int nt = 1;
    try {
      for (; nt < planned_; nt++) th[nt] = start_(&HostTeam::entry, this, nt);
    } catch (const std::system_error&) {
    }
    nt_.store(nt, std::memory_order_release);
    work(0, nt);
    for (int t = 1; t < nt; t++) th[t].join();
    nt_.store(0, std::memory_order_relaxed);
  }

  // every participant of the running region calls it the same number of times
  void barrier() {
    const int nt = nt_.load(std::memory_order_acquire);
    const int gen = gen_.load(std::memory_order_acquire);
    if (arrived_.fetch_add(1, std::memory_order_acq_rel) + 1 == nt) {
      arrived_.store(0, std::memory_order_relaxed);
      gen_.store(gen + 1, std::memory_order_release);
    } else {
      while (gen_.load(std::memory_order_acquire) == gen) std::this_thread::yield();
    }
  }

 private:
  static void entry(void* team, int t) {
    HostTeam* me = static_cast<HostTeam*>(team);
    int nt;
    while ((nt = me->nt_.load(std::memory_order_acquire)) == 0) std::this_thread::yield();
    me->call_(me->work_, t, nt);
  }
  HostThreadStart start_;
  int planned_ = 1;
  void* work_ = nullptr;
  void (*call_)(void*, int, int) = nullptr;
  std::atomic<int> nt_{0}, arrived_{0}, gen_{0};
};

// thread t's share of [0, n)
inline void host_team_range(int n, int t, int nt, int* a, int* b) {
  *a = (int)((long long)n * t / nt);
  *b = (int)((long long)n * (t + 1) / nt);
}

// ------------------------------------------------------------------------------- layout of the reduced system
// Dense (ldS = n, offset 0) or, for large systems whose cameras order into a narrow band, LAPACK-style lower band
// storage (see BaCommon in ba_state.h).  The switches are the caller's diagnostics, spelled out: every rank of a
// distributed solve must pass the same ones.
struct BaLayoutSwitches {
  bool allow_band = false;  // the entry point can use band storage at all
  bool force_dense = false, no_cyclic = false, schur_atomics = false, chol_no_bcr = false, chol_no_fused = false;
};

struct BaLayout {
  bool banded = false;
  bool cyclic = false;    // band form whose band closes on itself (camera loop in trajectory order)
  bool renumber = false;  // linear band: the free cameras are renumbered into the band order
  int bw = 0, ldS = 0, offS = 0;
  size_t s_elems = 0;  // doubles to allocate / clear / exchange for S
};

// does the layout depend on the band order at all (else the two half-bandwidths need not be computed)
inline bool ba_layout_considers_band(int n, const BaLayoutSwitches& sw) { return sw.allow_band && n > 128 && !sw.force_dense; }

// half_lin: block half-bandwidth in reverse Cuthill-McKee order; half_cyc: in the cameras' own order, distances around the ring
inline BaLayout ba_reduced_layout(int n, int half_lin, int half_cyc, const BaLayoutSwitches& sw) {
  BaLayout y;
  y.ldS = n;
  y.bw = n;
  y.s_elems = (size_t)n * n;
  if (!ba_layout_considers_band(n, sw)) return y;
  const int bw = 6 * half_lin + 5, bws = bw + VSL_CHOL_NB;
  // CYCLIC band: in the cameras' own order with distances around the ring.  Taken when the ring solver has a block
  // layout for it and its blocks are at most 3/4 of the linear form's (the solve costs ~ block size squared per
  // level): the 500-keyframe loop of configs[4] has half bandwidth 18 cameras around the ring, 36 in its best line
  const int bwc = 6 * half_cyc + 5, B_lin = (bw + 1 + 31) / 32 * 32;
  int B_cyc = 0, nblk_cyc = 0;
  if (!sw.no_cyclic && !sw.schur_atomics && chol_ring_available(n, bwc, CholSwitches{sw.chol_no_fused, sw.chol_no_bcr, false}, &B_cyc, &nblk_cyc) &&
      4 * B_cyc <= 3 * B_lin) {
    y.banded = y.cyclic = true;
    y.bw = bwc;
    y.ldS = y.offS = bwc + VSL_CHOL_NB;
    y.s_elems = (size_t)n * (bwc + VSL_CHOL_NB + 1) + 64;
  } else if ((size_t)(bws + 1) * 2 < (size_t)n) {  // worth it: the band holds less than half of the matrix
    y.banded = y.renumber = true;
    y.bw = bw;
    y.ldS = y.offS = bws;
    y.s_elems = (size_t)n * (bws + 1) + 64;  // + slack: the diagonal kernels read (never use) a few entries past a row
  }
  return y;
}

// ------------------------------------------------------------------------------------------ landmark CSR
// lm_start[l] .. lm_start[l + 1] = the positions of landmark l's observations in landmark order (lm_start: n_lms + 1
// ints); returns whether the caller's order IS landmark order.  cam_start (nullable, n_cams + 1 ints): the same
// count-and-prefix by camera, gathered in the same pass.
inline bool ba_landmark_csr(const vsl_ba_problem* p, int* lm_start, int* cam_start = nullptr) {
  std::fill(lm_start, lm_start + p->n_lms + 1, 0);
  if (cam_start) std::fill(cam_start, cam_start + p->n_cams + 1, 0);
  bool sorted_in = true;
  for (int i = 0; i < p->n_obs; i++) {
    lm_start[p->obs_lm[i] + 1]++;
    if (cam_start) cam_start[p->obs_cam[i] + 1]++;
    if (i > 0 && p->obs_lm[i] < p->obs_lm[i - 1]) sorted_in = false;
  }
  for (int l = 0; l < p->n_lms; l++) lm_start[l + 1] += lm_start[l];
  if (cam_start)
    for (int c = 0; c < p->n_cams; c++) cam_start[c + 1] += cam_start[c];
  return sorted_in;
}

// ---------------------------------------------------------------------------------------------- band order
// Band order of the free cameras: reverse Cuthill-McKee on the covisibility graph (two free cameras are adjacent iff
// some landmark is observed by both: exactly the non-zero 6 x 6 blocks of the reduced camera system).  gp = the
// problem whose observations define the graph (a session passes the FULL problem so that every rank derives the same
// order), start / sorted_in = its ba_landmark_csr.  order[position] = free index in ascending-camera numbering;
// returns the block half-bandwidth (max |position difference| over the edges).  A 500-keyframe loop comes out as a
// band of a few dozen cameras with no corner blocks (the breadth-first levels run both ways round the loop).
inline int camera_band_order(const vsl_ba_problem* gp, const int* start, bool sorted_in, const std::vector<int>& cam_free0,
                             int nfree, std::vector<int>& order, int* half_cyclic_natural, const HostTeamConfig& threads) {
  const size_t words = ((size_t)nfree + 63) / 64;
  std::vector<uint64_t> adj((size_t)nfree * words, 0);
  {
    // free-camera index of every observation in landmark order; the reference's own order is landmark order already:
    // then the threads below look the cameras up themselves (no gathered copy)
    std::vector<int> cams_v;
    if (!sorted_in) {
      cams_v.resize(gp->n_obs);
      std::vector<int> fill(start, start + gp->n_lms);
      for (int i = 0; i < gp->n_obs; i++) cams_v[fill[gp->obs_lm[i]]++] = cam_free0[gp->obs_cam[i]];
    }
    const int* cams_p = sorted_in ? nullptr : cams_v.data();
    const int32_t* ocam = gp->obs_cam;
    auto cam_at = [&](int a) { return cams_p ? cams_p[a] : cam_free0[ocam[a]]; };
    // a private bit matrix per thread, OR-ed together afterwards (shared atomics made the threads fight over its lines)
    HostTeam team(gp->n_lms, 1 << 15, threads);  // ~k^2 = 80 bit operations per landmark: parallel from 32k landmarks
    std::vector<std::vector<uint64_t>> priv(team.planned(), std::vector<uint64_t>(adj.size(), 0));
    team.run([&](int t, int nt) {
      std::vector<uint64_t>& my = priv[t];
      int l0, l1;
      host_team_range(gp->n_lms, t, nt, &l0, &l1);
      for (int l = l0; l < l1; l++)
        for (int a = start[l]; a < start[l + 1]; a++) {
          const int ca = cam_at(a);
          if (ca < 0) continue;
          for (int b = a + 1; b < start[l + 1]; b++) {
            const int cb = cam_at(b);
            if (cb < 0 || cb == ca) continue;
            my[(size_t)ca * words + (cb >> 6)] |= 1ull << (cb & 63);
            my[(size_t)cb * words + (ca >> 6)] |= 1ull << (ca & 63);
          }
        }
    });
    for (auto& my : priv)
      for (size_t i = 0; i < adj.size(); i++) adj[i] |= my[i];
  }
  std::vector<std::vector<int>> nb(nfree);
  std::vector<int> deg(nfree, 0);
  for (int c = 0; c < nfree; c++)
    for (size_t w = 0; w < words; w++) {
      uint64_t m = adj[(size_t)c * words + w];
      while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        nb[c].push_back((int)(w * 64) + b);
      }
    }
  for (int c = 0; c < nfree; c++) deg[c] = (int)nb[c].size();
  for (int c = 0; c < nfree; c++) std::sort(nb[c].begin(), nb[c].end(), [&](int x, int y) { return deg[x] != deg[y] ? deg[x] < deg[y] : x < y; });
  std::vector<char> seen(nfree, 0);
  order.clear();
  order.reserve(nfree);
  auto bfs = [&](int root, std::vector<int>& out) {  // Cuthill-McKee from root over the unseen part; returns the last level's first node
    const size_t first = out.size();
    out.push_back(root);
    seen[root] = 1;
    for (size_t h = first; h < out.size(); h++)
      for (int v : nb[out[h]])
        if (!seen[v]) {
          seen[v] = 1;
          out.push_back(v);
        }
    return out.back();
  };
  for (;;) {
    int root = -1;
    for (int c = 0; c < nfree; c++)
      if (!seen[c] && (root < 0 || deg[c] < deg[root])) root = c;
    if (root < 0) break;
    // pseudo-peripheral start: two sweeps (the far end of a sweep from a minimum-degree node)
    std::vector<int> probe;
    const int far_end = bfs(root, probe);
    for (int v : probe) seen[v] = 0;
    bfs(far_end, order);
  }
  std::reverse(order.begin(), order.end());
  std::vector<int> pos(nfree);
  for (int k = 0; k < nfree; k++) pos[order[k]] = k;
  int half = 0;
  for (int c = 0; c < nfree; c++)
    for (int v : nb[c]) half = std::max(half, std::abs(pos[c] - pos[v]));
  if (half_cyclic_natural) {
    // the cameras as they come (ascending index = the reference's keyframe order, i.e. along the trajectory), distances
    // taken AROUND the ring: a closed loop has half the bandwidth of its best linear order this way
    int hc = 0;
    for (int c = 0; c < nfree; c++)
      for (int v : nb[c]) {
        const int d = std::abs(c - v);
        hc = std::max(hc, std::min(d, nfree - d));
      }
    *half_cyclic_natural = hc;
  }
  return half;
}

// ------------------------------------------------------------------------------------------------- the plan
// kernel limits the plan is cut to (ba_setup passes SCH_CMAX, SCH_KMAX of ba.hip and, for a session, BL_THREADS, BL_LMW of ba_large.h)
struct BaPlanLimits {
  int small_max_free_cams;  // the small-system Schur kernel: free cameras ...
  int small_max_lm_free;    // ... and observations of one landmark that hit free cameras
  int run_max_obs;          // the recompute-form kernels: observations ...
  int run_max_lms;          // ... and landmarks of a workgroup's landmark run
};

struct BaHostPlan {
  std::vector<int> cam_free, free_cams;  // camera -> free index or -1, and back (after band renumbering)
  int nfree = 0;
  int half_lin = 0, half_cyc = 0;  // block half-bandwidths of the band order (0 where the layout did not ask)
  BaLayout layout;
  std::vector<int> lm_start, cam_start;
  std::vector<int> perm;  // sorted position -> caller observation index; empty = identity (the input is in landmark order)
  // observations sorted by landmark: the caller's own arrays when they are sorted already, the vectors below otherwise
  const int32_t *obs_cam = nullptr, *obs_lm = nullptr;
  const double* obs_uv = nullptr;
  std::vector<int> cam_obs, cam_pos;  // camera CSR over the sorted positions, and its inverse
  int kmax_free = 0;                  // most free-camera observations of one landmark
  size_t n_pairs = 0;                 // (observation, observation) pairs of the block lists of the gather-form Schur complement (upper bound)
  bool small = true;
  std::vector<int> wg_lm;  // landmark runs of the recompute form (empty when small, or when one landmark exceeds a run)
  int n_wg = 0;
  std::vector<int> s_cam_v, s_lm_v;
  std::vector<double> s_uv_v;
  BaHostPlan() = default;
  BaHostPlan(BaHostPlan&&) = default;  // (moving a vector keeps its buffer: the pointers above stay good; a copy would not)
  BaHostPlan& operator=(BaHostPlan&&) = default;
};

// p: the problem; gp: the problem whose observations define the covisibility graph (the full problem for a session
// rank; null or p: the problem itself).  lap(name) is called where a set-up phase ends (BaTrace in ba_state.h).
template <class Lap>
BaHostPlan ba_host_plan(const vsl_ba_problem* p, const vsl_ba_problem* gp, const BaLayoutSwitches& sw, const BaPlanLimits& lim,
                        Lap lap, const HostTeamConfig& threads = HostTeamConfig()) {
  BaHostPlan P;
  const int C = p->n_cams, L = p->n_lms, O = p->n_obs;
  P.cam_free.assign(C, -1);
  for (int c = 0; c < C; c++)
    if (!p->cam_fixed[c]) {
      P.cam_free[c] = (int)P.free_cams.size();
      P.free_cams.push_back(c);
    }
  P.nfree = (int)P.free_cams.size();
  const int n = 6 * P.nfree;
  P.lm_start.resize((size_t)L + 1);
  P.cam_start.resize((size_t)C + 1);
  const bool sorted_in = ba_landmark_csr(p, P.lm_start.data(), P.cam_start.data());
  if (ba_layout_considers_band(n, sw)) {
    std::vector<int> order, g_start;
    bool g_sorted = sorted_in;
    if (gp && gp != p) {
      g_start.resize((size_t)gp->n_lms + 1);
      g_sorted = ba_landmark_csr(gp, g_start.data());
    }
    P.half_lin = camera_band_order(g_start.empty() ? p : gp, g_start.empty() ? P.lm_start.data() : g_start.data(), g_sorted,
                                   P.cam_free, P.nfree, order, &P.half_cyc, threads);
    P.layout = ba_reduced_layout(n, P.half_lin, P.half_cyc, sw);
    if (P.layout.renumber) {
      std::vector<int> renum(P.nfree);
      for (int k = 0; k < P.nfree; k++) renum[k] = P.free_cams[order[k]];
      P.free_cams = renum;
      for (int k = 0; k < P.nfree; k++) P.cam_free[P.free_cams[k]] = k;
    }
  } else {
    P.layout = ba_reduced_layout(n, 0, 0, sw);
  }
  lap("free cameras + band order");
  // sort observations by landmark (stable: keeps the caller's order inside a landmark).  The reference's own order
  // (map_utils.h:373 / loop_closure_utils.h:700: landmarks, then their observations) -- what
  // include/visnav_amd/bundle_adjustment.h hands over -- is sorted already: then the caller's arrays ARE the sorted ones
  // (no permutation, no 24 MB of gathered copies at 881 k observations; perm stays empty = identity)
  P.obs_cam = p->obs_cam;
  P.obs_lm = p->obs_lm;
  P.obs_uv = p->obs_uv;
  if (!sorted_in) {
    P.perm.resize(O);
    {
      std::vector<int> fill(P.lm_start.begin(), P.lm_start.end() - 1);
      for (int i = 0; i < O; i++) P.perm[fill[p->obs_lm[i]]++] = i;
    }
    P.s_cam_v.resize(O);
    P.s_lm_v.resize(O);
    P.s_uv_v.resize(2 * (size_t)O);
    HostTeam(O, 1 << 19, threads).run([&](int t, int nt) {
      int q0, q1;
      host_team_range(O, t, nt, &q0, &q1);
      for (int q = q0; q < q1; q++) {
        const int i = P.perm[q];
        P.s_cam_v[q] = p->obs_cam[i];
        P.s_lm_v[q] = p->obs_lm[i];
        P.s_uv_v[2 * (size_t)q] = p->obs_uv[2 * (size_t)i];
        P.s_uv_v[2 * (size_t)q + 1] = p->obs_uv[2 * (size_t)i + 1];
      }
    });
    P.obs_cam = P.s_cam_v.data();
    P.obs_lm = P.s_lm_v.data();
    P.obs_uv = P.s_uv_v.data();
  }
  // camera CSR over the sorted observation positions (counts gathered with the landmark counts above) and its inverse:
  // position of an observation in camera-major order (the gather-form Schur kernels keep their blocks in that order,
  // so that the blocks of one camera row read one contiguous segment).  ONE parallel region (three regions and a
  // serial scatter were 3.9 ms at 881 k observations, of which 1.2 ms starting threads): every thread counts the pairs
  // of its landmark range and the cameras of its observation chunk; after a barrier thread 0 turns the chunk histograms
  // into cursors; after another every thread scatters its chunk -- a stable counting sort, the caller's order inside a
  // camera.  The sums are integers and the sort is stable: the result does not depend on the number of threads.
  P.cam_obs.resize(O);
  P.cam_pos.resize(O);
  {
    HostTeam team(O, 1 << 19, threads);
    std::vector<std::vector<int>> hist(team.planned(), std::vector<int>((size_t)C, 0));
    size_t np_t[HOST_TEAM_MAX] = {0};
    int km_t[HOST_TEAM_MAX] = {0};
    const int32_t* s_cam = P.obs_cam;
    team.run([&](int t, int nt) {
      int l0, l1, q0, q1;
      host_team_range(L, t, nt, &l0, &l1);
      host_team_range(O, t, nt, &q0, &q1);
      size_t np = 0;
      int km = 0;
      for (int l = l0; l < l1; l++) {
        int k = 0;
        for (int q = P.lm_start[l]; q < P.lm_start[l + 1]; q++) k += P.cam_free[s_cam[q]] >= 0;
        km = std::max(km, k);
        np += (size_t)k * k;  // upper bound (k (k + 1) / 2 when no camera observes a landmark twice)
      }
      np_t[t] = np;
      km_t[t] = km;
      std::vector<int>& h = hist[t];
      for (int q = q0; q < q1; q++) h[s_cam[q]]++;
      team.barrier();
      if (t == 0)
        for (int c = 0; c < C; c++) {
          int at = P.cam_start[c];
          for (int u = 0; u < nt; u++) {
            const int cnt = hist[u][c];
            hist[u][c] = at;  // becomes thread u's cursor for camera c
            at += cnt;
          }
        }
      team.barrier();
      for (int q = q0; q < q1; q++) {
        const int k = h[s_cam[q]]++;
        P.cam_obs[k] = q;
        P.cam_pos[q] = k;
      }
    });
    for (int t = 0; t < HOST_TEAM_MAX; t++) {
      P.n_pairs += np_t[t];
      P.kmax_free = std::max(P.kmax_free, km_t[t]);
    }
  }
  lap("sort + CSRs");
  P.small = n <= 128 && P.nfree <= lim.small_max_free_cams && P.kmax_free <= lim.small_max_lm_free;
  // landmark runs of the recompute-form kernels: <= run_max_obs observations and <= run_max_lms landmarks per workgroup
  if (!P.small) {
    P.wg_lm.push_back(0);
    for (int l = 0, a = 0; l < L; l++) {
      if (P.lm_start[l + 1] - P.lm_start[l] > lim.run_max_obs) {  // a landmark seen by more cameras than a workgroup has threads
        P.wg_lm.clear();
        break;
      }
      if (P.lm_start[l + 1] - P.lm_start[a] > lim.run_max_obs || l - a == lim.run_max_lms) {
        P.wg_lm.push_back(l);
        a = l;
      }
      if (l == L - 1) P.wg_lm.push_back(L);
    }
  }
  P.n_wg = P.wg_lm.empty() ? 0 : (int)P.wg_lm.size() - 1;
  return P;
}

// The form of a session's iteration, from the plan and the caller's diagnostics alone (so it is known before the device
// arena is planned): the recompute form (ba_large.h) for large systems in gather form whose landmarks all fit a
// workgroup's run; the chain over stored r / F / E blocks otherwise (small systems, "ba_no_fused", "ba_schur_atomics",
// pair lists beyond 32-bit positions, a landmark seen more often than a run has observations).
inline bool ba_recompute_form(const BaHostPlan& hp, bool no_fused, bool schur_atomics) {
  return !hp.small && hp.n_wg > 0 && hp.nfree > 0 && !no_fused && !schur_atomics && hp.n_pairs < ((size_t)1 << 31);
}

// --------------------------------------------------------------------------------- a session's sub-problem
struct BaSubObs {
  std::vector<int32_t> obs_cam, obs_lm;
  std::vector<double> obs_uv;
};

// The problem restricted to the landmarks [lm_first, lm_first + lm_count), all cameras: their observations in the
// caller's order with the landmark index rebased, held by `store`.  n_obs = 0: the range has no observations.
inline vsl_ba_problem ba_sub_problem(const vsl_ba_problem* prob, int lm_first, int lm_count, BaSubObs& store) {
  for (int i = 0; i < prob->n_obs; i++) {
    const int l = prob->obs_lm[i];
    if (l >= lm_first && l < lm_first + lm_count) {
      store.obs_cam.push_back(prob->obs_cam[i]);
      store.obs_lm.push_back(l - lm_first);
      store.obs_uv.push_back(prob->obs_uv[2 * (size_t)i]);
      store.obs_uv.push_back(prob->obs_uv[2 * (size_t)i + 1]);
    }
  }
  vsl_ba_problem sub = *prob;
  sub.n_lms = lm_count;
  sub.n_obs = (int32_t)store.obs_cam.size();
  sub.points = prob->points + 3 * (size_t)lm_first;
  sub.obs_cam = store.obs_cam.data();
  sub.obs_lm = store.obs_lm.data();
  sub.obs_uv = store.obs_uv.data();
  return sub;
}
