// Drives the map route of visual-slam_amd/csrc/ba_rig_plan.h (rig_map_plan_build) on the CPU, plain C++ without HIP:
// tests/test_ba_rig_map_plan_cpu.py.
//   ba_rig_map_plan_test plan [force_dense] [no_cyclic] < problem
//       checks the plan against brute force (below) and prints "name v v v" lines: layout, half, slots, pairs, segments
//   ba_rig_map_plan_test sweep      random problems of many shapes, every switch combination: the same checks
// problem: the format of ba_rig_plan_test.cpp (n_bodies / body_fixed / n_cams / cam_body / cam_intr / n_lms / n_obs /
// obs_cam / obs_lm).  The checks, none of which reads the plan's own pair list or graph to decide what is right:
//   pairs      the listed pairs = the brute-force set of free-body pairs that share a landmark (plus every diagonal),
//              diagonal first, the rest strictly ascending in (hi, lo)
//   slots      natural_slot is a bijection and agrees with free_bodies / body_slot; the renumbered plan holds rig_plan_check
//   layout     every field equals ba_reduced_layout on the brute-force graph's half-bandwidths (the cyclic one recomputed
//              here; the linear one is the plan's order measured on the brute-force edges)
//   storage    every listed pair's 36 (21 on a band's diagonal) positions lie inside the allocation and no two collide;
//              the storage expanded by rig_map_expand is non-zero exactly on the blocks of co-visible pairs -- every
//              other in-band position, the padding and the slack are left to the clear
//   segments   per pair one per 512 entries of the longer of its two body lists, at most 64; items consecutive
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>

#include "ba_rig_plan.h"

static const double kTbc[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 2, 3};

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

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "check failed, line %d: %s\n", __LINE__, #cond);       \
      return false;                                                          \
    }                                                                        \
  } while (0)

// every property of the header comment; true when all hold
static bool check(const Problem& p, const BaLayoutSwitches& sw, const RigPlan& plan, const RigMapPlan& mp) {
  const RigPlanIn in = p.in();
  const int B = in.n_bodies, nf = plan.n_free, n = 6 * nf;
  REQUIRE(rig_plan_check(in, plan));
  // brute force: free bodies in ascending id = natural index; adjacency from the raw observations
  std::vector<int> nat(B, -1);
  int k = 0;
  for (int b = 0; b < B; b++)
    if (!p.body_fixed[b]) nat[b] = k++;
  REQUIRE(k == nf);
  std::vector<char> adj((size_t)nf * nf, 0);
  for (int l = 0; l < in.n_lms; l++) {
    std::vector<int> seen;
    for (int i = 0; i < in.n_obs; i++)
      if (in.obs_lm[i] == l && nat[in.cam_body[in.obs_cam[i]]] >= 0) seen.push_back(nat[in.cam_body[in.obs_cam[i]]]);
    for (int a : seen)
      for (int b : seen)
        if (a != b) adj[(size_t)a * nf + b] = 1;
  }
  // slots
  REQUIRE((int)mp.natural_slot.size() == nf && (int)plan.free_bodies.size() == nf);
  std::vector<int> hit(nf, 0);
  for (int a = 0; a < nf; a++) {
    const int s = mp.natural_slot[a];
    REQUIRE(s >= 0 && s < nf && !hit[s]++);
    REQUIRE(nat[plan.free_bodies[s]] == a && plan.body_slot[plan.free_bodies[s]] == s);
    if (!mp.layout.renumber) REQUIRE(s == a);
  }
  // layout
  int half_cyc = 0, half_order = 0;
  for (int a = 0; a < nf; a++)
    for (int b = 0; b < nf; b++)
      if (adj[(size_t)a * nf + b]) {
        half_cyc = std::max(half_cyc, std::min(std::abs(a - b), nf - std::abs(a - b)));
        half_order = std::max(half_order, std::abs(mp.natural_slot[a] - mp.natural_slot[b]));
      }
  if (ba_layout_considers_band(n, sw)) {
    REQUIRE(mp.half_cyc == half_cyc);
    if (mp.layout.renumber) REQUIRE(mp.half_lin == half_order);  // the slots ARE the band order
  } else {
    REQUIRE(mp.half_lin == 0 && mp.half_cyc == 0);
  }
  const BaLayout want = ba_reduced_layout(n, mp.half_lin, mp.half_cyc, sw);
  const BaLayout& y = mp.layout;
  REQUIRE(y.banded == want.banded && y.cyclic == want.cyclic && y.renumber == want.renumber && y.bw == want.bw &&
          y.ldS == want.ldS && y.offS == want.offS && y.s_elems == want.s_elems);
  REQUIRE(mp.form == (y.cyclic ? 2 : (y.banded ? 1 : 0)));
  if (y.banded && !y.cyclic) REQUIRE(6 * half_order + 5 <= y.bw);
  if (y.cyclic) REQUIRE(6 * half_cyc + 5 <= y.bw);
  // pairs
  std::set<std::pair<int, int>> brute;
  for (int a = 0; a < nf; a++)
    for (int b = 0; b < nf; b++)
      if (adj[(size_t)a * nf + b]) {
        const int sa = mp.natural_slot[a], sb = mp.natural_slot[b];
        brute.insert({std::max(sa, sb), std::min(sa, sb)});
      }
  const int P = mp.n_pairs();
  REQUIRE(P == nf + (int)brute.size() && (int)mp.pair_lo.size() == P && (int)mp.pair_first.size() == P + 1);
  for (int q = 0; q < nf; q++) REQUIRE(mp.pair_hi[q] == q && mp.pair_lo[q] == q);
  for (int q = nf; q < P; q++) {
    REQUIRE(mp.pair_hi[q] > mp.pair_lo[q] && brute.count({mp.pair_hi[q], mp.pair_lo[q]}));
    if (q > nf) REQUIRE(std::make_pair(mp.pair_hi[q - 1], mp.pair_lo[q - 1]) < std::make_pair(mp.pair_hi[q], mp.pair_lo[q]));
  }
  // segments
  REQUIRE(mp.pair_first[0] == 0 && mp.pair_first[P] == mp.n_items());
  for (int q = 0; q < P; q++) {
    const int la = plan.bg_start[mp.pair_hi[q] + 1] - plan.bg_start[mp.pair_hi[q]];
    const int lb = plan.bg_start[mp.pair_lo[q] + 1] - plan.bg_start[mp.pair_lo[q]];
    const int len = std::max(la, lb), nseg = len > 64 * 512 ? 64 : (len <= 512 ? 1 : (len + 511) / 512);
    REQUIRE(mp.pair_first[q + 1] - mp.pair_first[q] == nseg);
    for (int i = mp.pair_first[q]; i < mp.pair_first[q + 1]; i++) REQUIRE(mp.item_pair[i] == q);
  }
  // storage: what the finish kernel writes (the mirror of the dense form included), then the expansion
  std::vector<double> store(y.s_elems, 0.0);
  auto put = [&](long long at, double v) {
    if (at < 0 || (size_t)at >= y.s_elems || store[(size_t)at] != 0.0) return false;
    store[(size_t)at] = v;
    return true;
  };
  for (int q = 0; q < P; q++)
    for (int x = 0; x < 6; x++)
      for (int z = 0; z < 6; z++) {
        const int hi = mp.pair_hi[q], lo = mp.pair_lo[q];
        if (hi == lo && z > x) continue;
        const long long at = rig_map_entry_at(mp.form, y.ldS, y.offS, nf, mp.half_cyc, hi, lo, x, z);
        REQUIRE(put(at, 1.0 + q));
        if (mp.form == 0 && !(hi == lo && x == z)) REQUIRE(put((long long)(6 * lo + z) * y.ldS + 6 * hi + x, 1.0 + q));
      }
  std::vector<double> dense((size_t)n * n, -1.0);
  rig_map_expand(mp, nf, store.data(), dense.data());
  for (int a = 0; a < nf; a++)
    for (int b = 0; b < nf; b++) {
      const bool owned = a == b || adj[(size_t)a * nf + b];
      const int sa = mp.natural_slot[a], sb = mp.natural_slot[b];
      int q = -1;
      for (int t = 0; t < P && owned; t++)
        if (mp.pair_hi[t] == std::max(sa, sb) && mp.pair_lo[t] == std::min(sa, sb)) q = t;
      for (int x = 0; x < 6; x++)
        for (int z = 0; z < 6; z++) REQUIRE(dense[(size_t)(6 * a + x) * n + 6 * b + z] == (owned ? 1.0 + q : 0.0));
    }
  return true;
}

static void line(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

static int sweep() {
  std::mt19937 rng(11);
  long checked = 0, forms[3] = {0, 0, 0}, renumbered = 0;
  for (int B : {1, 2, 5, 23, 26, 44})
    for (int shape = 0; shape < 4; shape++)       // chain, ring, ring plus a clique, random
      for (int switches = 0; switches < 4; switches++) {
        Problem p;
        const int nfix = B > 1 ? 1 : 0, nf = B - nfix, window = 2 + shape;
        for (int b = 0; b < B; b++) p.body_fixed.push_back(b < nfix);
        for (int b = 0; b < B; b++) {
          const int which = rng() % 5;  // mostly both cameras
          if (which != 4) { p.cam_body.push_back(b); p.cam_intr.push_back(0); }
          if (which != 3) { p.cam_body.push_back(b); p.cam_intr.push_back(1); }
        }
        const int C = (int)p.cam_body.size();
        p.n_lms = shape == 0 ? std::max(1, nf - window + 1) : nf + 2;
        for (int l = 0; l < p.n_lms; l++)
          for (int c = 0; c < C; c++) {
            const int b = p.cam_body[c];
            bool sees;
            if (b < nfix) sees = l % 3 != 1;
            else if (l >= nf) sees = l == nf ? false : (b == B - 1);  // a landmark nobody sees, one a single free body sees
            else if (shape == 3) sees = rng() % 4 == 0;
            else sees = ((b - nfix) - l + 8 * nf) % nf < window || (shape == 2 && l == 0 && (b - nfix) % 3 == 0);
            if (sees) { p.obs_cam.push_back(c); p.obs_lm.push_back(l); }
          }
        if (p.obs_cam.empty()) { p.obs_cam.push_back(C - 1); p.obs_lm.push_back(0); }
        for (size_t i = p.obs_cam.size(); i > 1; i--) {
          const size_t j = rng() % i;
          std::swap(p.obs_cam[i - 1], p.obs_cam[j]);
          std::swap(p.obs_lm[i - 1], p.obs_lm[j]);
        }
        BaLayoutSwitches sw;
        sw.allow_band = true;
        sw.force_dense = switches == 1;
        sw.no_cyclic = switches == 2;
        sw.chol_no_bcr = switches == 3;
        RigPlan plan;
        RigMapPlan mp;
        if (rig_map_plan_build(p.in(), sw, plan, mp) != RIG_PLAN_OK || !check(p, sw, plan, mp)) {
          fprintf(stderr, "sweep: B=%d shape=%d switches=%d fails\n", B, shape, switches);
          return 1;
        }
        checked++;
        forms[mp.form]++;
        renumbered += mp.layout.renumber;
      }
  printf("checked %ld dense %ld band %ld cyclic %ld renumbered %ld\n", checked, forms[0], forms[1], forms[2], renumbered);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "sweep")) return sweep();
  if (strcmp(argv[1], "plan")) return 2;
  BaLayoutSwitches sw;
  sw.allow_band = true;
  for (int i = 2; i < argc; i++) {
    if (!strcmp(argv[i], "force_dense")) sw.force_dense = true;
    if (!strcmp(argv[i], "no_cyclic")) sw.no_cyclic = true;
  }
  Problem p;
  if (!read_problem(p)) return 2;
  RigPlan plan;
  RigMapPlan mp;
  const int st = rig_map_plan_build(p.in(), sw, plan, mp);
  if (st != RIG_PLAN_OK) {
    printf("status %d %d\n", st, plan.first_bad);
    return 0;
  }
  if (!check(p, sw, plan, mp)) return 1;
  printf("status 0 -1\n");
  printf("layout %d %d %d %d %lld %d\n", mp.form, mp.layout.bw, mp.layout.ldS, mp.layout.offS, (long long)mp.layout.s_elems,
         mp.layout.renumber ? 1 : 0);
  printf("half %d %d\n", mp.half_lin, mp.half_cyc);
  int B_ring = 0, nblk = 0;
  if (mp.form == 2 && chol_ring_available(6 * plan.n_free, mp.layout.bw, CholSwitches{}, &B_ring, &nblk)) printf("ring %d %d\n", B_ring, nblk);
  printf("dims %d %d %d %d\n", plan.n_free, plan.n_groups(), mp.n_pairs(), mp.n_items());
  line("natural_slot", mp.natural_slot);
  line("free_bodies", plan.free_bodies);
  line("pair_hi", mp.pair_hi);
  line("pair_lo", mp.pair_lo);
  line("pair_first", mp.pair_first);
  return 0;
}
