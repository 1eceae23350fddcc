// visnav::global_bundle_adjustment_iterative through the drop-in wrapper (include/visnav_amd/bundle_adjustment.h) beside
// visnav::global_bundle_adjustment on the same mirror-type map.
//   ba_pcg_test <ba.bin> <out.bin>   ba.bin as written by tests/test_ba_pcg_dropin.py; out = [iterative poses | iterative
//                                    points | direct poses | direct points] (camera / landmark order of the file), then
//                                    the "ba_iterative_schur" diagnostic before and after each of the two wrapper calls
//                                    (it is tried at 0 and at 1), the layout code and the PCG solve count behind the
//                                    iterative call and behind the direct call, as doubles
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "visnav_amd/bundle_adjustment.h"

using namespace visnav;

template <class T>
static void put(std::ofstream& o, const T* p, size_t n) { o.write(reinterpret_cast<const char*>(p), sizeof(T) * n); }
template <class T>
static void get(std::ifstream& i, T* p, size_t n) { i.read(reinterpret_cast<char*>(p), sizeof(T) * n); }

#define REQUIRE(c)                                                     \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

struct Map {
  Cameras cameras;
  Landmarks landmarks;
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t nc, nl, no;
  get(in, &nc, 1); get(in, &nl, 1); get(in, &no, 1);
  std::vector<double> poses(7 * nc), points(3 * nl), uv(2 * no), intr(16);
  std::vector<uint8_t> fixed(nc);
  std::vector<int32_t> ocam(no), olm(no);
  get(in, poses.data(), poses.size()); get(in, fixed.data(), fixed.size()); get(in, intr.data(), 16);
  get(in, points.data(), points.size()); get(in, ocam.data(), no); get(in, olm.data(), no); get(in, uv.data(), uv.size());
  REQUIRE(in.good());
  Corners corners;
  std::set<FrameCamId> fixed_set;
  Calibration calib;
  for (int k = 0; k < 2; k++) {
    auto c = std::make_shared<AbstractCameraD>();
    c->model = "ds";
    for (int j = 0; j < 8; j++) c->param[j] = intr[8 * k + j];
    calib.intrinsics.push_back(c);
  }
  auto track = [](int l) { return (TrackId)(1000 + 7 * l); };
  Map base;
  for (int c = 0; c < nc; c++) {
    FrameCamId fcid(c / 2, c % 2);
    for (int j = 0; j < 7; j++) base.cameras[fcid].T_w_c.data()[j] = poses[7 * c + j];
    if (fixed[c]) fixed_set.insert(fcid);
    corners[fcid];
  }
  for (int l = 0; l < nl; l++) base.landmarks[track(l)].p = Eigen::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
  for (int i = 0; i < no; i++) {
    FrameCamId fcid(ocam[i] / 2, ocam[i] % 2);
    auto& kd = corners[fcid];
    const int fid = (int)kd.corners.size();
    kd.corners.emplace_back(uv[2 * i], uv[2 * i + 1]);
    base.landmarks[track(olm[i])].all_obs[fcid] = fid;
  }
  GlobalBundleAdjustmentOptions opts;
  opts.verbosity_level = 0;
  opts.max_num_iterations = 20;

  auto diag = [](int* v) { return vsl_ctx_get_diagnostic(amd::ctx(), "ba_iterative_schur", v); };
  double tail[8];
  // tight PCG tolerance: the wrapper's result is compared with the direct route's at the bars of the LM parity tests
  REQUIRE(vsl_ctx_set_diagnostic(amd::ctx(), "ba_pcg_tol_exp", 12) == VSL_OK);
  Map it = base, it_on = base, direct = base;
  int before = -1, after = -1, banded = -1;
  int64_t solves = -1;
  REQUIRE(diag(&before) == VSL_OK);
  global_bundle_adjustment_iterative(corners, opts, fixed_set, calib, it.cameras, it.landmarks);
  REQUIRE(diag(&after) == VSL_OK);
  tail[0] = before; tail[1] = after;
  REQUIRE(vsl_ctx_last_ba_layout(amd::ctx(), nullptr, &banded, nullptr) == VSL_OK);
  REQUIRE(vsl_ctx_last_ba_pcg(amd::ctx(), &solves, nullptr, nullptr, nullptr) == VSL_OK);
  tail[4] = banded; tail[5] = (double)solves;
  // a caller that already has the switch on keeps it on
  REQUIRE(vsl_ctx_set_diagnostic(amd::ctx(), "ba_iterative_schur", 1) == VSL_OK);
  REQUIRE(diag(&before) == VSL_OK);
  global_bundle_adjustment_iterative(corners, opts, fixed_set, calib, it_on.cameras, it_on.landmarks);
  REQUIRE(diag(&after) == VSL_OK);
  tail[2] = before; tail[3] = after;
  REQUIRE(vsl_ctx_set_diagnostic(amd::ctx(), "ba_iterative_schur", 0) == VSL_OK);
  global_bundle_adjustment(corners, opts, fixed_set, calib, direct.cameras, direct.landmarks);
  REQUIRE(vsl_ctx_last_ba_layout(amd::ctx(), nullptr, &banded, nullptr) == VSL_OK);
  REQUIRE(vsl_ctx_last_ba_pcg(amd::ctx(), &solves, nullptr, nullptr, nullptr) == VSL_OK);
  tail[6] = banded; tail[7] = (double)solves;
  // the two iterative calls are the same solve: the same bits
  for (int c = 0; c < nc; c++)
    for (int j = 0; j < 7; j++)
      REQUIRE(it.cameras[FrameCamId(c / 2, c % 2)].T_w_c.data()[j] == it_on.cameras[FrameCamId(c / 2, c % 2)].T_w_c.data()[j]);

  std::ofstream out(argv[2], std::ios::binary);
  for (Map* m : {&it, &direct}) {
    for (int c = 0; c < nc; c++) put(out, m->cameras[FrameCamId(c / 2, c % 2)].T_w_c.data(), 7);
    for (int l = 0; l < nl; l++) put(out, m->landmarks[track(l)].p.data(), 3);
  }
  put(out, tail, 8);
  return 0;
}
