// chol_layout.h -- the arithmetic of the band solvers' storage (chol.hip) that their callers need on the host: plain
// C++, no HIP (vsl_common.h includes it; ba_host_plan.h and the CPU tests use it on their own).
#pragma once
#include <algorithm>

// LAPACK-style lower band storage (chol.hip, "BAND FORM"): S = storage + bws, ld = bws = bw + VSL_CHOL_NB
#define VSL_CHOL_NB 32
#define BCR_MAXB 256  // block size limit of the cyclic reduction: static LDS Us[256][33] + Lp[32][257] = 133 KB (dynamic LDS above 64 KiB is refused by the runtime)

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
