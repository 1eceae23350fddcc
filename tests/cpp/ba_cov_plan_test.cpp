// Drives visual-slam_amd/csrc/ba_cov_plan.h (with ba_host_plan.h and chol_plan.h, as plain C++, no HIP);
// tests/test_ba_cov_plan_cpu.py holds the expected values.
//
//   ba_cov_plan_test slot ld i j            -> the slot of entry (i, j) relative to the origin of the band array
//   ba_cov_plan_test buffers n bw nQ nu n_o -> the band route's carve-up: "in_bytes out_off out_bytes total" and the offsets
//   ba_cov_plan_test plan band              -> the tiny problem below planned for the query on stdin
//                                              ("n_cam_q n_lm_q / cams / lms"), with the free cameras in ascending
//                                              order (band = 0, Q holds the landmarks' cameras) or in the scrambled
//                                              order below (band = 1): one "name values..." line per field
//   ba_cov_plan_test sweep                  -> generated chains and rings through ba_host_plan (band allowed, cyclic
//                                              not) and cov_plan; every property is checked here, "checked N band M"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "ba_host_plan.h"
#include "ba_cov_plan.h"

namespace {

struct Problem {
  std::vector<uint8_t> fixed;
  std::vector<int32_t> cam, lm, intr_of;
  std::vector<double> uv, poses, points;
  double intr[16] = {0};
  vsl_ba_problem p;
  void finish(int C, int L) {
    const int O = (int)cam.size();
    uv.resize(2 * (size_t)O);
    for (int i = 0; i < O; i++) {
      uv[2 * (size_t)i] = i;
      uv[2 * (size_t)i + 1] = -i;
    }
    intr_of.assign(C, 0);
    poses.assign(7 * (size_t)C, 0.0);
    points.assign(3 * (size_t)L, 0.0);
    memset(&p, 0, sizeof p);
    p.n_cams = C;
    p.n_lms = L;
    p.n_obs = O;
    p.poses = poses.data();
    p.cam_fixed = fixed.data();
    p.cam_intr = intr_of.data();
    p.intr = intr;
    p.points = points.data();
    p.obs_cam = cam.data();
    p.obs_lm = lm.data();
    p.obs_uv = uv.data();
  }
};

void line(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, what); \
      return false;                                                       \
    }                                                                     \
  } while (0)

// landmark l is seen by k cameras from camera (l C / L) on, `stride` apart: clamped to the chain or wrapped round the
// ring; every third landmark in descending camera order, every fifth twice by its first camera
void gen(int C, int L, int k, int stride, bool ring, const std::vector<int>& fixed, Problem& pr) {
  pr.fixed.assign(C, 0);
  for (int c : fixed) pr.fixed[c] = 1;
  for (int l = 0; l < L; l++) {
    const int c0 = (int)((long long)l * C / L);
    std::vector<int> cs;
    for (int d = 0; d < k; d++) {
      const int c = c0 + d * stride;
      if (ring) cs.push_back(c % C);
      else if (c < C) cs.push_back(c);
    }
    if (l % 5 == 0) cs.push_back(cs[0]);
    if (l % 3 == 0) std::reverse(cs.begin(), cs.end());
    for (int c : cs) {
      pr.cam.push_back(c);
      pr.lm.push_back(l);
    }
  }
  pr.finish(C, L);
}

bool check_buffers(const CovBuffers& B, bool band, const char* what) {
  std::vector<size_t> in = {B.off_ok};
  if (!band) in.push_back(B.off_col_unk);
  in.push_back(B.off_q_free);
  if (!band) in.push_back(B.off_qpos);
  in.insert(in.end(), {B.off_u_lm, B.off_u_start, B.off_o_cam, B.off_o_uv});
  for (size_t i = 0; i < in.size(); i++) {
    CHECK(in[i] % 256 == 0 && in[i] <= B.in_bytes);
    if (i) CHECK(in[i] >= in[i - 1]);  // (an empty array takes no room)
  }
  CHECK(B.in_bytes % 256 == 0 && B.out_off % 256 == 0 && B.in_bytes <= B.out_off);
  CHECK(B.off_Sdiag >= B.in_bytes && B.off_Sdiag < B.out_off);
  if (band) CHECK(B.off_Z > B.off_Sdiag && B.off_Z < B.out_off);
  CHECK(B.off_pose == 0 && B.off_point >= B.off_pose && B.off_deg >= B.off_point && B.off_deg <= B.out_bytes);
  CHECK(B.total == B.out_off + B.out_bytes);
  return true;
}

// one generated problem, one query: every property the device code relies on.  *was_band: the layout took the band form
bool check_problem(const Problem& pr, const std::vector<int32_t>& cams, const std::vector<int32_t>& lms, bool* was_band,
                   const char* what) {
  BaLayoutSwitches sw;
  sw.allow_band = true;
  sw.no_cyclic = true;
  const BaPlanLimits lim = {22, 24, 512, 256};
  const BaHostPlan hp = ba_host_plan(&pr.p, nullptr, sw, lim, [](const char*) {});
  const BaLayout& y = hp.layout;
  CHECK(!y.cyclic);
  const int n = 6 * hp.nfree;
  *was_band = y.banded;
  const CovPlan P = cov_plan(&pr.p, hp.cam_free, hp.nfree, !y.banded, cams.data(), (int)cams.size(), lms.data(), (int)lms.size());
  // the numbering: fixed cameras -1, the free ones a permutation of 0 .. nfree - 1
  {
    std::vector<char> seen(hp.nfree, 0);
    for (int c = 0; c < pr.p.n_cams; c++) {
      const int f = P.cam_free[c];
      if (pr.fixed[c]) CHECK(f == -1);
      else {
        CHECK(f >= 0 && f < hp.nfree && !seen[f]);
        seen[f] = 1;
      }
    }
  }
  // query -> output maps (duplicates and permutations map back)
  CHECK((int)P.cam_q2Q.size() == (int)cams.size() && (int)P.lm_q2u.size() == (int)lms.size());
  for (size_t q = 0; q < cams.size(); q++) CHECK(P.cam_q2Q[q] >= 0 && P.cam_q2Q[q] < P.nQ && P.q_free[P.cam_q2Q[q]] == P.cam_free[cams[q]]);
  for (size_t q = 0; q < lms.size(); q++) CHECK(P.lm_q2u[q] >= 0 && P.lm_q2u[q] < P.nu && P.u_lm[P.lm_q2u[q]] == lms[q]);
  CHECK((int)std::set<int>(lms.begin(), lms.end()).size() == P.nu && (int)std::set<int>(P.u_lm.begin(), P.u_lm.end()).size() == P.nu);
  for (int q = 1; q < P.nQ; q++) CHECK(P.q_free[q] > P.q_free[q - 1]);
  if (y.banded) CHECK(P.nQ == (int)std::set<int>(cams.begin(), cams.end()).size());
  // observation lists: all of the landmark's observations, fixed cameras first, ascending position, the pixel with it
  CHECK((int)P.u_start.size() == P.nu + 1 && P.u_start[0] == 0 && P.u_start[P.nu] == P.n_o);
  bool any_free = false;
  for (int u = 0; u < P.nu; u++) {
    int cnt = 0;
    for (int i = 0; i < pr.p.n_obs; i++) cnt += pr.p.obs_lm[i] == P.u_lm[u];
    CHECK(P.u_start[u + 1] - P.u_start[u] == cnt && cnt <= P.kmax);
    for (int k = P.u_start[u]; k < P.u_start[u + 1]; k++) {
      const int i = (int)P.o_uv[2 * (size_t)k];  // (the pixel of observation i is (i, -i))
      CHECK(i >= 0 && i < pr.p.n_obs && P.o_uv[2 * (size_t)k + 1] == -(double)i);
      CHECK(pr.p.obs_lm[i] == P.u_lm[u] && pr.p.obs_cam[i] == P.o_cam[k]);
      const int f = P.cam_free[P.o_cam[k]];
      any_free |= f >= 0;
      if (k > P.u_start[u]) {
        const int i0 = (int)P.o_uv[2 * (size_t)(k - 1)], f0 = P.cam_free[P.o_cam[k - 1]];
        CHECK(f0 < f || (f0 == f && i0 < i));  // ascending position; the caller's order inside a camera
      }
      if (!y.banded && f >= 0) CHECK(P.qpos[f] >= 0 && P.q_free[P.qpos[f]] == f);
    }
  }
  CHECK(P.need_inverse == (!cams.empty() || any_free));
  if (!y.banded) return check_buffers(cov_buffers(P, n, (6 * P.nQ + COV_COLS - 1) / COV_COLS), false, what);
  // the band: the layout of chol.hip's band arrays, and every block a landmark's sum reads inside it
  const int bw = y.bw, ld = y.ldS;
  const SelinvPlan sp = chol_selinv_plan(n, bw, false);
  CHECK(ld == bw + VSL_CHOL_NB && y.offS == ld && bw == 6 * hp.half_lin + 5 && y.s_elems == sp.z_elems);
  CHECK(sp.z_elems == (size_t)n * (ld + 1) + 64);
  for (int u = 0; u < P.nu; u++)
    for (int a = P.u_start[u]; a < P.u_start[u + 1]; a++)
      for (int b = P.u_start[u]; b < P.u_start[u + 1]; b++) {
        const int ci = P.cam_free[P.o_cam[a]], cj = P.cam_free[P.o_cam[b]];
        if (ci < 0 || cj < 0) continue;
        CHECK(cov_band_holds_block(bw, ci, cj));
        for (int r = 0; r < 6; r++)
          for (int c = 0; c < 6; c++) {
            const int i = 6 * ci + r, j = 6 * cj + c, hi = std::max(i, j), lo = std::min(i, j);
            const size_t s = cov_band_at(ld, i, j);
            CHECK(hi - lo <= bw && s == cov_band_at(ld, j, i));
            // row hi of the storage holds columns hi - ld .. hi in its ld + 1 slots, the diagonal last
            CHECK(s + ld == (size_t)hi * (ld + 1) + (size_t)(ld - (hi - lo)) && s + ld < sp.z_elems - 64);
          }
      }
  for (int q = 0; q < P.nQ; q++) CHECK(cov_band_at(ld, 6 * P.q_free[q] + 5, 6 * P.q_free[q]) + ld < sp.z_elems - 64);
  const CovBuffers B = cov_band_buffers(P, n, bw);
  CHECK(B.out_off - B.off_Z >= sizeof(double) * sp.z_elems);
  return check_buffers(B, true, what);
}

// the tiny problem of "plan": 6 cameras, camera 2 fixed (in the middle); landmark -> cameras (the caller's order)
//   0: 4 0 2     1: 1 3     2: 2     3: 5 4 5     4: 0 1
// band order of "plan 1": camera -> position 0:3 1:4 2:- 3:0 4:2 5:1
const int kTinyObs[][2] = {{4, 0}, {1, 1}, {0, 0}, {2, 2}, {5, 3}, {3, 1}, {4, 3}, {2, 0}, {5, 3}, {0, 4}, {1, 4}};
const int kTinyBand[6] = {3, 4, -1, 0, 2, 1};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "slot" && argc == 5) {
    printf("%zu\n", cov_band_at(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])));
    return 0;
  }
  if (cmd == "buffers" && argc == 7) {
    CovPlan P;
    const int n = atoi(argv[2]), bw = atoi(argv[3]);
    P.nfree = n / 6;
    P.nQ = atoi(argv[4]);
    P.nu = atoi(argv[5]);
    P.n_o = atoi(argv[6]);
    const CovBuffers B = cov_band_buffers(P, n, bw);
    printf("%zu %zu %zu %zu\n", B.in_bytes, B.out_off, B.out_bytes, B.total);
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", B.off_ok, B.off_q_free, B.off_u_lm, B.off_u_start, B.off_o_cam, B.off_o_uv,
           B.off_Sdiag, B.off_Z, B.off_pose, B.off_point, B.off_deg);
    return check_buffers(B, true, "buffers") ? 0 : 1;
  }
  if (cmd == "plan" && argc == 3) {
    const bool band = atoi(argv[2]) != 0;
    Problem pr;
    pr.fixed = {0, 0, 1, 0, 0, 0};
    for (const auto& o : kTinyObs) {
      pr.cam.push_back(o[0]);
      pr.lm.push_back(o[1]);
    }
    pr.finish(6, 5);
    int nc, nl;
    if (scanf("%d %d", &nc, &nl) != 2) return 2;
    std::vector<int32_t> cams(nc), lms(nl);
    for (int& c : cams)
      if (scanf("%d", &c) != 1) return 2;
    for (int& l : lms)
      if (scanf("%d", &l) != 1) return 2;
    CovPlan P;
    if (band)
      P = cov_plan(&pr.p, std::vector<int>(kTinyBand, kTinyBand + 6), 5, false, cams.data(), nc, lms.data(), nl);
    else
      P = cov_plan(&pr.p, cams.data(), nc, lms.data(), nl);
    printf("dims %d %d %d %d %d %d\n", P.nfree, P.nQ, P.nu, P.n_o, P.kmax, (int)P.need_inverse);
    line("cam_free", P.cam_free);
    line("q_free", P.q_free);
    line("qpos", P.qpos);
    line("cam_q2Q", P.cam_q2Q);
    line("lm_q2u", P.lm_q2u);
    line("u_lm", P.u_lm);
    line("u_start", P.u_start);
    line("o_cam", P.o_cam);
    printf("o_obs");  // the caller's index of each listed observation
    for (int k = 0; k < P.n_o; k++) printf(" %d", (int)P.o_uv[2 * (size_t)k]);
    printf("\n");
    return 0;
  }
  if (cmd == "sweep") {
    int checked = 0, n_band = 0;
    char what[128];
    for (int ring = 0; ring < 2; ring++)
      for (int C : {9, 23, 30, 47, 64, 120})
        for (int k : {2, 4, 7})
          for (int variant = 0; variant < 3; variant++) {
            // fixed cameras: the first two; two in the middle as well; none (the plan does not care about the gauge)
            std::vector<int> fixed;
            if (variant == 0) fixed = {0, 1};
            if (variant == 1) fixed = {0, 1, C / 2, C / 2 + 1};
            const int L = 3 * C + 1, stride = variant == 2 ? 2 : 1;
            Problem pr;
            gen(C, L, k, stride, ring != 0, fixed, pr);
            snprintf(what, sizeof what, "ring %d C %d k %d variant %d", ring, C, k, variant);
            // queries: everything; a permuted subset with duplicates; landmarks only; cameras only
            std::vector<int32_t> free_cams, all_lms(L);
            for (int c = 0; c < C; c++)
              if (!pr.fixed[c]) free_cams.push_back(c);
            for (int l = 0; l < L; l++) all_lms[l] = l;
            std::vector<int32_t> sub_c, sub_l;
            for (size_t q = 0; q < free_cams.size(); q += 3) sub_c.push_back(free_cams[(q * 7 + 2) % free_cams.size()]);
            for (int l = 0; l < L; l += 4) sub_l.push_back((l * 11 + 5) % L);
            sub_c.push_back(sub_c[0]);
            sub_l.push_back(sub_l[0]);
            const std::vector<int32_t> none;
            bool band = false;
            if (!check_problem(pr, free_cams, all_lms, &band, what) || !check_problem(pr, sub_c, sub_l, &band, what) ||
                !check_problem(pr, none, sub_l, &band, what) || !check_problem(pr, sub_c, none, &band, what))
              return 1;
            checked += 4;
            n_band += band;
          }
    printf("checked %d band %d\n", checked, n_band);
    return 0;
  }
  return 3;
}
