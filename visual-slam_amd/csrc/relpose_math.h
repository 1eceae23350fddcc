// relpose_math.h -- the 6 x 6 arithmetic of ba_relpose_kernel (ba_cov.hip): Sigma_r -> Omega = Sigma_r^-1 with the pivot
// rules that decide "singular".  Plain C++ that compiles for the host and the device alike, so that the branches no
// bundle-adjustment input reaches (a failing pivot, a non-finite entry, an Omega the _w entry points would refuse) are
// driven by tests/cpp/relpose_math_test.cpp under g++ on hand-built matrices.  The kernel calls the three steps on
// matrices it keeps in LDS; rpm_information is the same three steps in sequence.
//   rpm_factor_invert   A = L L^T in place (lower triangle), Li = L^-1 by forward substitution; false when a pivot
//                       L_ii^2 <= 2^-36 A_ii or is not finite (the rule of vsl_ba_covariance)
//   rpm_info_entry      Omega_ij = sum_{k >= max(i, j)} Li_ki Li_kj, k ascending: (i, j) and (j, i) are the same sum
//   rpm_accepts         the test of pgo_edge_whiten_kernel on an exactly symmetric W: would the _w calls take it
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RPM_HD __host__ __device__
#else
#define RPM_HD
#endif

#define RPM_PIVOT_TOL 0x1p-36

RPM_HD inline bool rpm_finite(double x) { return x - x == 0.0; }  // false for infinities and NaN

RPM_HD inline bool rpm_factor_invert(double (*A)[6], double (*Li)[6]) {
  for (int j = 0; j < 6; j++) {
    const double ajj = A[j][j];
    double d = ajj;
    for (int k = 0; k < j; k++) d -= A[j][k] * A[j][k];
    if (!rpm_finite(d) || !(d > RPM_PIVOT_TOL * ajj)) return false;
    const double l = sqrt(d);
    A[j][j] = l;
    for (int i = j + 1; i < 6; i++) {
      double s = A[i][j];
      for (int k = 0; k < j; k++) s -= A[i][k] * A[j][k];
      A[i][j] = s / l;
    }
  }
  for (int c = 0; c < 6; c++) {
    for (int i = 0; i < c; i++) Li[i][c] = 0.0;
    Li[c][c] = 1.0 / A[c][c];
    for (int i = c + 1; i < 6; i++) {
      double s = 0.0;
      for (int k = c; k < i; k++) s -= A[i][k] * Li[k][c];
      Li[i][c] = s / A[i][i];
    }
  }
  return true;
}

RPM_HD inline double rpm_info_entry(const double (*Li)[6], int i, int j) {
  double s = 0.0;
  for (int k = i > j ? i : j; k < 6; k++) s += Li[k][i] * Li[k][j];
  return s;
}

// W: exactly symmetric; L: scratch (its lower triangle is written)
RPM_HD inline bool rpm_accepts(const double (*W)[6], double (*L)[6]) {
  for (int j = 0; j < 6; j++) {
    const double wjj = W[j][j];
    double d = wjj;
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
    if (!rpm_finite(d) || !(d > RPM_PIVOT_TOL * wjj)) return false;
    const double l = sqrt(d);
    L[j][j] = l;
    for (int i = j + 1; i < 6; i++) {
      double s = W[i][j];
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  return true;
}

// cov (row-major, exactly symmetric) -> info; false and 36 NaN when either test fails.  *stage (nullable): 0 fine,
// 1 the factorisation of cov failed, 2 Omega failed the test of the _w entry points.
RPM_HD inline bool rpm_information(const double* cov, double* info, int* stage) {
  double A[6][6], Li[6][6], W[6][6] = {};
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) A[i][j] = cov[6 * i + j];
  int st = 0;
  if (!rpm_factor_invert(A, Li)) {
    st = 1;
  } else {
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) W[i][j] = rpm_info_entry(Li, i, j);
    if (!rpm_accepts(W, A)) st = 2;
  }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) info[6 * i + j] = st ? nan("") : W[i][j];
  if (stage) *stage = st;
  return st == 0;
}
