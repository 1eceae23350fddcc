// Stand-alone driver of visual-slam_amd/csrc/ba_pair_plan.h (plain C++, no HIP): tests/test_ba_pair_plan_cpu.py builds it
// with g++ -- once plainly, once under the address and undefined-behaviour sanitizers -- and compares what it prints with
// values worked out by hand.
//   check                       stdin: n_cams, cam_free (-1: fixed), n_pairs, the pairs -> "<error> <index>"
//   plan <band> <bw> <no_read>  stdin as above -> the plan's fields, one per line
//   sweep                       properties over random band orders of many sizes -> "checked <n> solve <m>"
// cam_free is the numbering of the reduced camera system: ANY bijection of the free cameras onto [0, nfree).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "ba_pair_plan.h"

namespace {

struct Input {
  int n_cams = 0, n_pairs = 0, nfree = 0;
  std::vector<int> cam_free;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> a, b;
};

bool read_input(Input& in) {
  if (std::scanf("%d", &in.n_cams) != 1 || in.n_cams < 0) return false;
  in.cam_free.resize(in.n_cams);
  in.fixed.resize(in.n_cams);
  for (int i = 0; i < in.n_cams; i++) {
    if (std::scanf("%d", &in.cam_free[i]) != 1) return false;
    in.fixed[i] = in.cam_free[i] < 0;
    in.nfree += in.cam_free[i] >= 0;
  }
  if (std::scanf("%d", &in.n_pairs) != 1 || in.n_pairs < 0) return false;
  in.a.resize(in.n_pairs);
  in.b.resize(in.n_pairs);
  for (int q = 0; q < in.n_pairs; q++)
    if (std::scanf("%d %d", &in.a[q], &in.b[q]) != 2) return false;
  return true;
}

void line(const char* name, const std::vector<int>& v) {
  std::printf("%s", name);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "%s:%d: requirement failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

// every property the device code relies on
void verify(const Input& in, const BaPairPlan& P, bool band, int bw, bool no_read) {
  const PgcPlan& G = P.G;
  REQUIRE(P.band == band && G.dense == !band && G.nf == in.nfree && G.n == 6 * in.nfree && (int)G.pairs.size() == in.n_pairs);
  REQUIRE(G.bw == (band ? bw : 0));
  REQUIRE(G.n_fixed + G.n_read + G.n_solve == in.n_pairs);
  REQUIRE(std::is_sorted(G.col_nodes.begin(), G.col_nodes.end()));
  REQUIRE(std::adjacent_find(G.col_nodes.begin(), G.col_nodes.end()) == G.col_nodes.end());
  REQUIRE(G.nblk == (6 * (int)G.col_nodes.size() + PGC_COLS - 1) / PGC_COLS);
  REQUIRE((int)G.col_unk.size() == PGC_COLS * G.nblk && (int)G.row_lo.size() == G.nblk);
  for (size_t j = 0; j < G.col_unk.size(); j++) {
    REQUIRE(j < 6 * G.col_nodes.size() ? G.col_unk[j] == 6 * G.col_nodes[j / 6] + (int)(j % 6) : G.col_unk[j] == -1);
    REQUIRE(G.col_unk[j] < G.n);  // a unit row inside the system
  }
  std::set<int> used;
  for (int q = 0; q < in.n_pairs; q++) {
    const PgcPairDev& d = G.pairs[q];
    // free indices are those of S, node ids stay camera ids (rows of the problem's poses)
    REQUIRE(d.fa == in.cam_free[in.a[q]] && d.fb == in.cam_free[in.b[q]] && d.na == in.a[q] && d.nb == in.b[q]);
    REQUIRE(d.fa < in.nfree && d.fb < in.nfree);
    const bool one_fixed = d.fa < 0 || d.fb < 0;
    const bool in_band = !one_fixed && band && 6 * std::abs(d.fa - d.fb) + 5 <= bw;
    REQUIRE(d.kind == (one_fixed ? PGC_ONE_FIXED : (in_band && !no_read ? PGC_READ : PGC_SOLVE)));
    auto columns_of = [&](int c, int f) { return c >= 0 && c % 6 == 0 && c / 6 < (int)G.col_nodes.size() && G.col_nodes[c / 6] == f; };
    if (!band) {
      REQUIRE(d.fa < 0 ? d.ca == -1 : columns_of(d.ca, d.fa));
      REQUIRE(d.fb < 0 ? d.cb == -1 : columns_of(d.cb, d.fb));
      if (d.ca >= 0) used.insert(d.ca / 6);
      if (d.cb >= 0) used.insert(d.cb / 6);
    } else if (d.kind == PGC_SOLVE) {
      // the camera with the larger BAND POSITION, whichever way round the pair is given; the block's rows reach the other
      const int hi = std::max(d.fa, d.fb), lo = std::min(d.fa, d.fb), c = d.fa > d.fb ? d.ca : d.cb;
      REQUIRE(columns_of(c, hi) && (d.fa > d.fb ? d.cb : d.ca) == -1);
      for (int blk = c / PGC_COLS; blk <= (c + 5) / PGC_COLS; blk++) REQUIRE(G.row_lo[blk] <= 6 * lo);
      used.insert(c / 6);
    } else {
      REQUIRE(d.ca == -1 && d.cb == -1);
      // what the block kernel reads from the band of the inverse lies inside it
      if (d.kind == PGC_READ) REQUIRE(6 * std::abs(d.fa - d.fb) + 5 <= bw);
    }
  }
  REQUIRE(used.size() == G.col_nodes.size());  // no column is solved that no pair reads
  for (int blk = 0; blk < G.nblk; blk++) REQUIRE(G.row_lo[blk] >= 0 && G.row_lo[blk] <= G.n);
  // the arena: 256-byte aligned, in order, nothing overlaps
  const size_t np = (size_t)in.n_pairs, n = (size_t)G.n;
  const size_t offs[] = {P.off_ok, P.off_pairs, P.off_col_unk, P.off_row_lo, P.in_bytes, P.off_Sdiag, P.off_Linv, P.off_X, P.off_Z,
                         P.out_off, P.out_off + P.off_joint, P.out_off + P.off_meas, P.out_off + P.off_cov, P.out_off + P.off_info,
                         P.out_off + P.off_sing, P.total};
  const size_t need[] = {4, sizeof(PgcPairDev) * np, sizeof(int) * G.col_unk.size(), sizeof(int) * G.row_lo.size(), 0, 8 * n,
                         band ? 0 : 8 * ((n + 31) / 32) * 1024, 8 * (size_t)G.nblk * n * PGC_COLS,
                         band ? 8 * (n * (size_t)(bw + 33) + 64) : 0, 0, 1152 * np, 48 * np, 288 * np, 288 * np, 4 * np};
  for (int i = 0; i < 15; i++) REQUIRE(offs[i] % 256 == 0 && offs[i] + need[i] <= offs[i + 1]);
  REQUIRE(P.out_bytes == P.total - P.out_off);
}

int sweep() {
  long checked = 0, solve = 0;
  unsigned rng = 4321u;
  auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
  for (int n_cams : {2, 3, 7, 23, 60, 128})
    for (int n_fixed : {0, 1, 2, 5})
      for (int shuffled = 0; shuffled < 2; shuffled++)  // ascending camera id | a band order that is not the camera id
        for (int mode = 0; mode < 3; mode++)            // dense | band | band with the diagnostic
          for (int bw : {5, 11, 59}) {
            if (n_fixed >= n_cams) continue;
            Input in;
            in.n_cams = n_cams;
            in.fixed.assign(n_cams, 0);
            for (int k = 0; k < n_fixed; k++) in.fixed[next() % n_cams] = 1;
            std::vector<int> order;
            for (int c = 0; c < n_cams; c++)
              if (!in.fixed[c]) order.push_back(c);
            in.nfree = (int)order.size();
            if (shuffled)
              for (int k = in.nfree - 1; k > 0; k--) std::swap(order[k], order[next() % (k + 1)]);
            in.cam_free.assign(n_cams, -1);
            for (int k = 0; k < in.nfree; k++) in.cam_free[order[k]] = k;
            const int np = (int)(next() % 40);
            for (int q = 0; q < np; q++) {
              const int a = (int)(next() % n_cams), b = (int)(next() % n_cams);
              if (a == b || (in.fixed[a] && in.fixed[b])) continue;
              in.a.push_back(a);
              in.b.push_back(b);
            }
            in.n_pairs = (int)in.a.size();
            REQUIRE(bpp_check_pairs(n_cams, in.fixed.data(), in.a.data(), in.b.data(), in.n_pairs, nullptr) == PGC_PAIR_OK);
            const BaPairPlan P = bpp_plan(in.cam_free, in.nfree, mode != 0, bw, mode == 2, in.a.data(), in.b.data(), in.n_pairs);
            verify(in, P, mode != 0, bw, mode == 2);
            // a pair alone gets the same class and columns as in company, either way round
            for (int q = 0; q < in.n_pairs; q += 5) {
              const int32_t a1[2] = {in.a[q], in.b[q]}, b1[2] = {in.b[q], in.a[q]};
              const BaPairPlan S = bpp_plan(in.cam_free, in.nfree, mode != 0, bw, mode == 2, a1, b1, 2);
              REQUIRE(S.G.pairs[0].kind == P.G.pairs[q].kind && S.G.pairs[1].kind == P.G.pairs[q].kind);
              REQUIRE((S.G.pairs[0].ca >= 0) == (P.G.pairs[q].ca >= 0) && (S.G.pairs[0].cb >= 0) == (P.G.pairs[q].cb >= 0));
              REQUIRE(S.G.pairs[0].ca == S.G.pairs[1].cb && S.G.pairs[0].cb == S.G.pairs[1].ca);
            }
            checked++;
            solve += P.G.n_solve;
          }
  std::printf("checked %ld solve %ld\n", checked, solve);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "sweep") return sweep();
  Input in;
  if (!read_input(in)) {
    std::fprintf(stderr, "bad input\n");
    return 2;
  }
  if (cmd == "check") {
    int bad = -1;
    const int e = bpp_check_pairs(in.n_cams, in.fixed.data(), in.a.data(), in.b.data(), in.n_pairs, &bad);
    std::printf("%d %d\n", e, bad);
    return 0;
  }
  if (cmd == "plan" && argc == 5) {
    const bool band = std::atoi(argv[2]) != 0, no_read = std::atoi(argv[4]) != 0;
    const int bw = std::atoi(argv[3]);
    REQUIRE(bpp_check_pairs(in.n_cams, in.fixed.data(), in.a.data(), in.b.data(), in.n_pairs, nullptr) == PGC_PAIR_OK);
    const BaPairPlan P = bpp_plan(in.cam_free, in.nfree, band, bw, no_read, in.a.data(), in.b.data(), in.n_pairs);
    verify(in, P, band, bw, no_read);
    const PgcPlan& G = P.G;
    line("dims", {G.nf, G.n, G.bw, G.nblk, G.n_fixed, G.n_read, G.n_solve});
    line("col_nodes", G.col_nodes);
    line("col_unk", G.col_unk);
    line("row_lo", G.row_lo);
    std::vector<int> kind, fa, fb, ca, cb, na, nb;
    for (const PgcPairDev& d : G.pairs) {
      kind.push_back(d.kind);
      fa.push_back(d.fa);
      fb.push_back(d.fb);
      ca.push_back(d.ca);
      cb.push_back(d.cb);
      na.push_back(d.na);
      nb.push_back(d.nb);
    }
    line("kind", kind);
    line("fa", fa);
    line("fb", fb);
    line("ca", ca);
    line("cb", cb);
    line("na", na);
    line("nb", nb);
    return 0;
  }
  std::fprintf(stderr, "usage: ba_pair_plan_test check | plan <band> <bw> <no_read> | sweep\n");
  return 2;
}
