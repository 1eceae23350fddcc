// Stand-alone driver of visual-slam_amd/csrc/relpose_math.h (plain C++, no HIP): the 6 x 6 factor / invert / pivot
// steps of ba_relpose_kernel on hand-built matrices, the failure branches included -- no bundle-adjustment input was
// found that reaches them on the device.  tests/test_relpose_math_cpu.py builds it with g++, and once more under the
// address and undefined-behaviour sanitizers.  Prints one line per group; a violated requirement exits with 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "relpose_math.h"

#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "%s:%d: requirement failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

namespace {

// Sigma = L L^T exactly for L = I + e_5 e_0^T with L_55 = 2^-k: the last pivot is 2^-2k, Sigma_55 = 1 + 2^-2k
void near_singular(int k, double* S) {
  const double s = std::ldexp(1.0, -k);
  double L[6][6] = {};
  for (int i = 0; i < 6; i++) L[i][i] = 1.0;
  L[5][0] = 1.0;
  L[5][5] = s;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double v = 0.0;
      for (int c = 0; c < 6; c++) v += L[i][c] * L[j][c];
      S[6 * i + j] = v;
    }
}

bool all_nan(const double* m) {
  for (int i = 0; i < 36; i++)
    if (m[i] == m[i]) return false;
  return true;
}

// the arithmetic of pgo_edge_whiten_kernel, restated: what the consumer does with an information matrix
bool consumer_accepts(const double* W) {
  double L[6][6];
  for (int j = 0; j < 6; j++) {
    const double wjj = W[7 * j];
    double d = wjj;
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
    if (!std::isfinite(d) || !(d > 0x1p-36 * wjj)) return false;
    const double l = std::sqrt(d);
    L[j][j] = l;
    for (int i = j + 1; i < 6; i++) {
      double s = 0.5 * (W[6 * i + j] + W[6 * j + i]);
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  return true;
}

double check_inverse(const double* S, const double* W) {
  double worst = 0.0;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      REQUIRE(std::memcmp(&W[6 * i + j], &W[6 * j + i], sizeof(double)) == 0);  // exactly symmetric
      double v = 0.0;
      for (int c = 0; c < 6; c++) v += W[6 * i + c] * S[6 * c + j];
      worst = std::fmax(worst, std::fabs(v - (i == j ? 1.0 : 0.0)));
    }
  return worst;
}

}  // namespace

int main() {
  double S[36], W[36];
  int stage = -1;
  // ---- identity and a diagonal: exact
  for (int i = 0; i < 36; i++) S[i] = i % 7 == 0 ? 1.0 : 0.0;
  REQUIRE(rpm_information(S, W, &stage) && stage == 0 && std::memcmp(S, W, sizeof(S)) == 0);
  for (int i = 0; i < 6; i++) S[7 * i] = std::ldexp(1.0, 2 * i - 20);  // powers of four: badly SCALED, not singular
  REQUIRE(rpm_information(S, W, &stage) && stage == 0);
  for (int i = 0; i < 6; i++) REQUIRE(W[7 * i] == std::ldexp(1.0, 20 - 2 * i));
  std::printf("exact ok\n");

  // ---- the pivot boundary, exactly: the last pivot of Sigma is 2^-2k of a diagonal entry 1 + 2^-2k
  int first_fail = -1;
  for (int k = 8; k <= 26; k++) {
    near_singular(k, S);
    REQUIRE(S[35] == 1.0 + std::ldexp(1.0, -2 * k));
    const bool ok = rpm_information(S, W, &stage);
    if (k <= 17) {  // 2^-2k / (1 + 2^-2k) > 2^-36
      REQUIRE(ok && stage == 0 && consumer_accepts(W));
      REQUIRE(check_inverse(S, W) <= 64 * std::ldexp(1.0, 2 * k) * 0x1p-52 * 4);  // cond ~ 4 x 2^2k
    } else {        // k = 18: the ratio is 2^-36 / (1 + 2^-36), NOT above 2^-36
      REQUIRE(!ok && stage == 1 && all_nan(W));
      if (first_fail < 0) first_fail = k;
    }
  }
  REQUIRE(first_fail == 18);
  std::printf("boundary ok: last accepted k 17, first refused k %d\n", first_fail);

  // ---- refused inputs: rank deficient, indefinite, negative, zero, non-finite entries; always 36 NaN
  near_singular(10, S);
  for (int j = 0; j < 6; j++) S[6 * 5 + j] = S[6 * 0 + j], S[6 * j + 5] = S[6 * j + 0];  // row / column 5 = row / column 0
  S[35] = S[0];
  REQUIRE(!rpm_information(S, W, &stage) && stage == 1 && all_nan(W));
  for (int i = 0; i < 36; i++) S[i] = i % 7 == 0 ? 1.0 : 0.0;
  S[7 * 3] = -1.0;
  REQUIRE(!rpm_information(S, W, &stage) && stage == 1 && all_nan(W));
  for (int i = 0; i < 36; i++) S[i] = 0.0;
  REQUIRE(!rpm_information(S, W, &stage) && stage == 1 && all_nan(W));
  for (int bad = 0; bad < 3; bad++) {
    for (int i = 0; i < 36; i++) S[i] = i % 7 == 0 ? 2.0 : 0.0;
    const double v = bad == 0 ? std::nan("") : (bad == 1 ? INFINITY : -INFINITY);
    S[7 * 2] = v;
    REQUIRE(!rpm_information(S, W, &stage) && stage == 1 && all_nan(W));
    for (int i = 0; i < 36; i++) S[i] = i % 7 == 0 ? 2.0 : 0.0;
    S[6 * 4 + 1] = S[6 * 1 + 4] = v;  // off the diagonal: the pivot of row 4 is not finite
    REQUIRE(!rpm_information(S, W, &stage) && stage == 1 && all_nan(W));
  }
  REQUIRE(!rpm_finite(std::nan("")) && !rpm_finite(INFINITY) && !rpm_finite(-INFINITY) && rpm_finite(0.0) && rpm_finite(-1e308));
  // the consumer's rule on Omega (stage 2), called as the kernel calls it: the same boundary, and agreement with the
  // restated consumer on both sides of it
  for (int k = 15; k <= 20; k++) {
    double Wm[6][6], Ls[6][6];
    near_singular(k, &Wm[0][0]);
    REQUIRE(rpm_accepts(Wm, Ls) == (k <= 17) && consumer_accepts(&Wm[0][0]) == (k <= 17));
    Wm[2][2] = std::nan("");
    REQUIRE(!rpm_accepts(Wm, Ls));
  }
  std::printf("refusals ok\n");

  // ---- random symmetric positive definite matrices, one pivot graded from 1 down to 2^-59: whatever is returned as
  // finite is exactly symmetric and accepted by the consumer's own test; whatever is refused is NaN
  unsigned rng = 99u;
  auto unit = [&]() { return rng = rng * 1664525u + 1013904223u, ((rng >> 8) & 0xffff) / 65536.0 - 0.5; };
  int accepted = 0, refused_cov = 0, refused_info = 0;
  for (int t = 0; t < 4000; t++) {
    const int e = t % 60, at = (t / 60) % 6;  // Sigma = L D L^T, L unit lower triangular, D = 1 but 2^-e at `at`
    double L[6][6] = {}, D[6];
    for (int i = 0; i < 6; i++) {
      D[i] = i == at ? std::ldexp(1.0, -e) : 1.0;
      L[i][i] = 1.0;
      for (int j = 0; j < i; j++) L[i][j] = unit();
    }
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++) {
        double v = 0.0;
        for (int c = 0; c <= j; c++) v += L[i][c] * D[c] * L[j][c];
        S[6 * i + j] = S[6 * j + i] = v;
      }
    const bool ok = rpm_information(S, W, &stage);
    if (ok) {
      REQUIRE(stage == 0 && consumer_accepts(W));
      for (int i = 0; i < 36; i++) REQUIRE(std::isfinite(W[i]));
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) REQUIRE(std::memcmp(&W[6 * i + j], &W[6 * j + i], sizeof(double)) == 0);
      accepted++;
    } else {
      REQUIRE((stage == 1 || stage == 2) && all_nan(W));
      (stage == 1 ? refused_cov : refused_info)++;
    }
  }
  REQUIRE(accepted > 100 && refused_cov > 100);
  std::printf("sweep ok: accepted %d, refused at Sigma %d, refused at Omega %d\n", accepted, refused_cov, refused_info);
  return 0;
}
