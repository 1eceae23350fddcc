// ba_pair_plan.h -- the host half of vsl_ba_relative_pose_covariance and vsl_global_ba_relative_pose_covariance
// (ba_cov.hip): everything derived from the problem's fixed mask, the free-camera numbering of the reduced camera
// system and the queried pairs before the first byte goes to the device.  Plain C++, no HIP, no vsl_ctx:
// tests/cpp/ba_pair_plan_test.cpp drives it under g++.
//   bpp_check_pairs   the argument rules of a pair list (pgc_check_pairs on the cameras' fixed mask)
//   bpp_plan          the class of every pair, the unique column cameras, the unit-column blocks (pgc_classify of
//                     pgo_cov_plan.h on the numbering S has), and the call's share of the arena
// THE ORDER THE DEVICE SEES is the numbering of S: ascending camera id on the dense route, BaHostPlan::cam_free (reverse
// Cuthill-McKee on the covisibility graph) on the band route.  The classes, and with them which camera of a pair is
// solved for, follow the band position, not the camera id.  Camera ids stay what they are: PgcPairDev::na / nb index
// the poses of the problem.
#pragma once
#include "chol_plan.h"
#include "pgo_cov_plan.h"

inline int bpp_check_pairs(int n_cams, const uint8_t* cam_fixed, const int32_t* a, const int32_t* b, int n_pairs, int* bad) {
  return pgc_check_pairs(n_cams, cam_fixed, a, b, n_pairs, bad);
}

struct BaPairPlan {
  PgcPlan G;  // nf, n, bw, classes, pairs, col_unk, row_lo (its own arena offsets are not used)
  bool band = false;
  // the caller's share of the arena: [inputs, one copy up | work | outputs, one copy back]
  size_t off_ok = 0, off_pairs = 0, off_col_unk = 0, off_row_lo = 0, in_bytes = 0;
  size_t off_Sdiag = 0, off_Linv = 0, off_X = 0, off_Z = 0;  // Linv: dense route; Z: band route, the STORAGE base of the band of S^-1
  size_t out_off = 0, off_joint = 0, off_meas = 0, off_cov = 0, off_info = 0, off_sing = 0, out_bytes = 0, total = 0;  // outputs relative to out_off
};

// cam_free: [n_cams] camera -> free index of S or -1 (nfree free cameras); band / bw: the layout of S (bw: half
// bandwidth in unknowns); no_band_read: the diagnostic that sends in-band pairs through the solve.  The pairs have
// passed bpp_check_pairs.
inline BaPairPlan bpp_plan(const std::vector<int>& cam_free, int nfree, bool band, int bw, bool no_band_read, const int32_t* a,
                           const int32_t* b, int n_pairs) {
  BaPairPlan P;
  P.band = band;
  PgcPlan& G = P.G;
  G.nf = nfree;
  G.n = 6 * nfree;
  G.dev_free = cam_free;
  G.dev_node.resize(cam_free.size());
  for (size_t c = 0; c < cam_free.size(); c++) G.dev_node[c] = (int)c;
  pgc_classify(G, !band, bw, no_band_read, a, b, n_pairs);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += pgc_align(bytes);
    return o;
  };
  const size_t np = (size_t)n_pairs, n = (size_t)G.n;
  P.off_ok = take(sizeof(int));
  P.off_pairs = take(sizeof(PgcPairDev) * np);
  P.off_col_unk = take(sizeof(int) * G.col_unk.size());
  P.off_row_lo = take(sizeof(int) * G.row_lo.size());
  P.in_bytes = at;
  P.off_Sdiag = take(sizeof(double) * n);
  P.off_Linv = take(band ? 0 : sizeof(double) * ((n + VSL_CHOL_NB - 1) / VSL_CHOL_NB) * VSL_CHOL_NB * VSL_CHOL_NB);
  P.off_X = take(sizeof(double) * (size_t)G.nblk * n * PGC_COLS);
  P.off_Z = take(band ? sizeof(double) * chol_selinv_plan(G.n, bw, false).z_elems : 0);
  P.out_off = at;
  P.off_joint = take(sizeof(double) * 144 * np) - P.out_off;
  P.off_meas = take(sizeof(double) * 6 * np) - P.out_off;
  P.off_cov = take(sizeof(double) * 36 * np) - P.out_off;
  P.off_info = take(sizeof(double) * 36 * np) - P.out_off;
  P.off_sing = take(sizeof(int) * np) - P.out_off;
  P.out_bytes = at - P.out_off;
  P.total = at;
  return P;
}
