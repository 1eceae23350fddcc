// Drives visual-slam_amd/csrc/ba_rig_cov_plan.h (the host half of the rig covariances) as plain C++: no HIP, no library.
//   query   stdin "nb b.. nc c.. nl l.." on the hand problem below: "status first_bad", then the plan's fields
//   pairs   stdin "np a b a b ..": "status bad", then fa fb ca cb na nb of every pair and the column bodies
//   cap     a landmark with 256 / 257 groups: prints the two statuses
//   sweep   random problems and queries (duplicates, empty lists): the properties the device code relies on
// tests/test_ba_rig_cov_plan_cpu.py builds it twice (the second time under the address and undefined-behaviour
// sanitizers) and checks the literal values, worked out by hand.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "ba_rig_cov_plan.h"

namespace {

struct Problem {
  std::vector<uint8_t> fixed;
  std::vector<int32_t> cam_body, cam_intr, obs_cam, obs_lm;
  int n_lms = 0;
  double T[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0.1, 0, 0};
  RigPlan plan;
  int build() {
    RigPlanIn in;
    in.n_cams = (int)cam_body.size(); in.n_lms = n_lms; in.n_obs = (int)obs_cam.size();
    in.cam_intr = cam_intr.data(); in.obs_cam = obs_cam.data(); in.obs_lm = obs_lm.data();
    in.n_bodies = (int)fixed.size(); in.body_fixed = fixed.data(); in.cam_body = cam_body.data(); in.T_b_c = T;
    return rig_plan_build(in, plan);
  }
  int query(const std::vector<int32_t>& b, const std::vector<int32_t>& c, const std::vector<int32_t>& l, RigCovPlan& P) const {
    return rcp_plan(plan, (int)fixed.size(), (int)cam_body.size(), n_lms, cam_intr.data(), b.empty() ? nullptr : b.data(), (int)b.size(),
                    c.empty() ? nullptr : c.data(), (int)c.size(), l.empty() ? nullptr : l.data(), (int)l.size(), P);
  }
};

// four bodies, body 0 fixed; body 2 carries a right camera only; landmark 0 is seen by both cameras of body 1 (one group
// of two) and by body 2; landmark 1 by the fixed body and both cameras of body 1; landmark 2 by the fixed body only;
// landmark 3 by bodies 2 and 3
Problem hand() {
  Problem p;
  p.fixed = {1, 0, 0, 0};
  p.cam_body = {0, 0, 1, 1, 2, 3, 3};
  p.cam_intr = {0, 1, 0, 1, 1, 0, 1};
  p.n_lms = 4;
  const int obs[][2] = {{3, 1}, {0, 0}, {4, 0}, {2, 1}, {2, 0}, {1, 1}, {3, 0}, {0, 2}, {1, 2}, {6, 3}, {4, 3}, {5, 3}};
  for (auto& o : obs) {
    p.obs_cam.push_back(o[0]);
    p.obs_lm.push_back(o[1]);
  }
  if (p.build() != RIG_PLAN_OK) abort();
  return p;
}

void print(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

std::vector<int32_t> read_list() {
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 0) abort();
  std::vector<int32_t> v(n);
  for (auto& x : v)
    if (scanf("%d", &x) != 1) abort();
  return v;
}

// what rig_cov_pose_kernel / rig_cov_landmark_kernel index with
bool check(const Problem& p, const std::vector<int32_t>& b, const std::vector<int32_t>& c, const std::vector<int32_t>& l,
           const RigCovPlan& P) {
  const RigPlan& rp = p.plan;
  std::set<int> want;
  for (int x : b) want.insert(rp.body_slot[x]);
  for (int x : c) want.insert(rp.cam_slot[x]);
  for (int x : l)
    for (int g = rp.lm_grp[x]; g < rp.lm_grp[x + 1]; g++) want.insert(rp.grp_slot[g]);
  if (std::vector<int>(want.begin(), want.end()) != P.q_free || P.nQ != (int)want.size()) return false;  // the union, ascending
  if ((int)P.qpos.size() != rp.n_free) return false;
  for (int s = 0; s < rp.n_free; s++)
    if ((P.qpos[s] >= 0) != (want.count(s) > 0) || (P.qpos[s] >= 0 && P.q_free[P.qpos[s]] != s)) return false;
  if (P.nblk != (6 * P.nQ + 15) / 16 || (int)P.col_unk.size() != 16 * P.nblk) return false;
  for (int j = 0; j < 16 * P.nblk; j++)
    if (P.col_unk[j] != (j < 6 * P.nQ ? 6 * P.q_free[j / 6] + j % 6 : -1)) return false;
  if (P.n_items != (int)(b.size() + c.size())) return false;
  for (size_t q = 0; q < b.size(); q++)
    if (P.item_ext[q] != -1 || P.q_free[P.item_q[q]] != rp.body_slot[b[q]]) return false;
  for (size_t q = 0; q < c.size(); q++)
    if (P.item_ext[b.size() + q] != p.cam_intr[c[q]] || P.q_free[P.item_q[b.size() + q]] != rp.cam_slot[c[q]]) return false;
  std::set<int> ul(l.begin(), l.end());
  if (P.nu != (int)ul.size() || P.lm_q2u.size() != l.size()) return false;
  int gmax = 0;
  for (size_t q = 0; q < l.size(); q++) {
    if (P.u_lm[P.lm_q2u[q]] != l[q]) return false;
    const RigCovGroups g = rcp_groups(rp, l[q]);
    gmax = std::max(gmax, g.count);
    for (int k = g.first; k < g.first + g.count; k++) {
      if (P.qpos[rp.grp_slot[k]] < 0) return false;                                   // every group's body has its columns
      if (k > g.first && rp.grp_slot[k - 1] >= rp.grp_slot[k]) return false;          // ascending slot
      if (rp.grp_begin[k] >= rp.grp_end[k]) return false;
    }
  }
  if (gmax != P.gmax) return false;
  // the arena: inputs, work, outputs in this order, nothing overlapping
  const size_t offs[] = {P.off_ok, P.off_col_unk, P.off_q_free, P.off_qpos, P.off_item_q, P.off_item_ext, P.off_u_lm, P.in_bytes,
                         P.off_Linv, P.off_Sdiag, P.off_X, P.out_off, P.out_off + P.off_pose, P.out_off + P.off_point,
                         P.out_off + P.off_deg, P.total};
  for (size_t k = 1; k < sizeof(offs) / sizeof(offs[0]); k++)
    if (offs[k] < offs[k - 1] || offs[k] % 256) return false;
  return P.total - (P.out_off + P.off_deg) >= sizeof(int) * (size_t)P.nu && P.out_off - P.off_X >= 8 * (size_t)P.nblk * 6 * rp.n_free * 16;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "query")) {
    Problem p = hand();
    const std::vector<int32_t> b = read_list(), c = read_list(), l = read_list();
    RigCovPlan P;
    const int st = p.query(b, c, l, P);
    printf("status %d %d\n", st, P.first_bad);
    if (st != RCP_OK) return 0;
    if (!check(p, b, c, l, P)) return 2;
    printf("dims %d %d %d %d %d %d\n", P.n_free, P.nQ, P.n_items, P.nu, P.gmax, P.nblk);
    print("q_free", P.q_free); print("qpos", P.qpos); print("col_unk", P.col_unk);
    print("item_q", P.item_q); print("item_ext", P.item_ext); print("u_lm", P.u_lm); print("lm_q2u", P.lm_q2u);
    for (int u : P.u_lm) {
      const RigCovGroups g = rcp_groups(p.plan, u);
      printf("groups_%d", u);
      for (int k = g.first; k < g.first + g.count; k++) printf(" %d %d %d", p.plan.grp_slot[k], p.plan.grp_begin[k], p.plan.grp_end[k]);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(mode, "null")) {  // a positive count with a null list, a negative count
    Problem p = hand();
    RigCovPlan P;
    const int32_t one = 1;
    printf("%d %d %d\n", rcp_plan(p.plan, 4, 7, 4, p.cam_intr.data(), nullptr, 1, nullptr, 0, nullptr, 0, P),
           rcp_plan(p.plan, 4, 7, 4, p.cam_intr.data(), &one, -1, nullptr, 0, nullptr, 0, P),
           rcp_plan(p.plan, 4, 7, 4, p.cam_intr.data(), nullptr, 0, nullptr, 0, nullptr, 1, P));
    return 0;
  }
  if (!strcmp(mode, "pairs")) {
    Problem p = hand();
    const std::vector<int32_t> ab = read_list();
    std::vector<int32_t> a, b;
    for (size_t k = 0; k + 1 < ab.size(); k += 2) {
      a.push_back(ab[k]);
      b.push_back(ab[k + 1]);
    }
    BaPairPlan P;
    int bad = -1;
    const int st = rcp_pair_plan(p.plan, 4, p.fixed.data(), a.data(), b.data(), (int)a.size(), P, &bad);
    printf("status %d %d\n", st, bad);
    if (st != PGC_PAIR_OK) return 0;
    for (const PgcPairDev& d : P.G.pairs) printf("pair %d %d %d %d %d %d\n", d.fa, d.fb, d.ca, d.cb, d.na, d.nb);
    print("col_nodes", P.G.col_nodes);
    printf("dims %d %d %d\n", P.G.nf, P.G.n, P.G.nblk);
    return 0;
  }
  if (!strcmp(mode, "cap")) {
    for (int free_bodies : {256, 257}) {
      Problem p;
      p.fixed.assign(free_bodies + 1, 0);
      p.fixed[0] = 1;
      p.n_lms = 2;
      for (int b = 0; b <= free_bodies; b++) {
        p.cam_body.push_back(b);
        p.cam_intr.push_back(0);
        p.obs_cam.push_back(b);
        p.obs_lm.push_back(0);
      }
      p.obs_cam.push_back(1);
      p.obs_lm.push_back(1);
      if (p.build() != RIG_PLAN_OK) return 2;
      RigCovPlan P, Q;
      const int s0 = p.query({}, {}, {0}, P), s1 = p.query({1}, {}, {1, 1}, Q);
      printf("%d %d %d %d\n", free_bodies, s0, s0 == RCP_OK ? P.gmax : -1, s1);
      if (s0 == RCP_OK && !check(p, {}, {}, {0}, P)) return 2;
    }
    return 0;
  }
  if (!strcmp(mode, "sweep")) {
    std::mt19937 rng(7);
    int plans = 0, empties = 0;
    for (int trial = 0; trial < 400; trial++) {
      Problem p;
      const int B = 2 + (int)(rng() % 7), L = 1 + (int)(rng() % 9);
      p.fixed.assign(B, 0);
      for (int b = 0; b < B - 1; b++) p.fixed[b] = rng() % 3 == 0;
      p.n_lms = L;
      for (int b = 0; b < B; b++) {
        const int kind = (int)(rng() % 3);  // left only, right only, both
        if (kind != 1) { p.cam_body.push_back(b); p.cam_intr.push_back(0); }
        if (kind != 0) { p.cam_body.push_back(b); p.cam_intr.push_back(1); }
      }
      const int Cn = (int)p.cam_body.size();
      for (int c = 0; c < Cn; c++)
        for (int l = 0; l < L; l++)
          if (rng() % 3) { p.obs_cam.push_back(c); p.obs_lm.push_back(l); }
      if (p.obs_cam.empty()) { p.obs_cam.push_back(0); p.obs_lm.push_back(0); }
      if (p.build() != RIG_PLAN_OK) return 2;
      std::vector<int32_t> fb, fc, b, c, l;
      for (int x = 0; x < B; x++) if (!p.fixed[x]) fb.push_back(x);
      for (int x = 0; x < Cn; x++) if (!p.fixed[p.cam_body[x]]) fc.push_back(x);
      for (int k = (int)(rng() % 4); k > 0; k--) b.push_back(fb[rng() % fb.size()]);
      for (int k = (int)(rng() % 4); k > 0; k--) c.push_back(fc[rng() % fc.size()]);
      for (int k = (int)(rng() % 5); k > 0; k--) l.push_back((int)(rng() % L));
      RigCovPlan P;
      if (p.query(b, c, l, P) != RCP_OK || !check(p, b, c, l, P)) {
        fprintf(stderr, "trial %d\n", trial);
        return 2;
      }
      plans++;
      empties += b.empty() && c.empty() && l.empty();
    }
    printf("checked %d plans %d empty\n", plans, empties);
    return 0;
  }
  fprintf(stderr, "usage: %s query|null|pairs|cap|sweep\n", argv[0]);
  return 1;
}
