// visnav::bundle_adjustment_rig_extrinsics through the drop-in wrapper (include/visnav_amd/bundle_adjustment.h) on a
// mirror-type map.
//   ba_rig_ext_dropin_test <rig.bin> <out.bin> <camera>   rig.bin as written by tests/test_ba_rig_ext_dropin.py: counts,
//                                                T_i_c [2][7], and per camera (frame id, camera id, fixed, pose); the
//                                                extrinsic of <camera> (0 or 1) is free.  out = [camera poses | points |
//                                                T_i_c[0] | T_i_c[1]] in the file's order, then the same after a second
//                                                call with every frame fixed and no extrinsic free
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

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int free_cam = std::atoi(argv[3]);
  std::ifstream in(argv[1], std::ios::binary);
  int32_t nc, nl, no;
  get(in, &nc, 1); get(in, &nl, 1); get(in, &no, 1);
  std::vector<double> tic(14), poses(7 * nc), points(3 * nl), uv(2 * no), intr(16);
  std::vector<int32_t> frame(nc), camid(nc), fixed(nc), ocam(no), olm(no);
  get(in, tic.data(), 14); get(in, frame.data(), nc); get(in, camid.data(), nc); get(in, fixed.data(), nc);
  get(in, poses.data(), poses.size()); get(in, intr.data(), 16); get(in, points.data(), points.size());
  get(in, ocam.data(), no); get(in, olm.data(), no); get(in, uv.data(), uv.size());
  REQUIRE(in.good());
  Corners corners;
  std::set<FrameCamId> fixed_set, all_set;
  Calibration calib;
  for (int k = 0; k < 2; k++) {
    auto c = std::make_shared<AbstractCameraD>();
    c->model = "ds";
    for (int j = 0; j < 8; j++) c->param[j] = intr[8 * k + j];
    calib.intrinsics.push_back(c);
    Sophus::SE3d T;
    for (int j = 0; j < 7; j++) T.data()[j] = tic[7 * k + j];
    calib.T_i_c.push_back(T);
  }
  auto track = [](int l) { return (TrackId)(500 + 3 * l); };
  auto fcid = [&](int c) { return FrameCamId(frame[c], (CamId)camid[c]); };
  Cameras cameras;
  Landmarks landmarks;
  for (int c = 0; c < nc; c++) {
    for (int j = 0; j < 7; j++) cameras[fcid(c)].T_w_c.data()[j] = poses[7 * c + j];
    if (fixed[c]) fixed_set.insert(fcid(c));
    all_set.insert(fcid(c));
    corners[fcid(c)];
  }
  for (int l = 0; l < nl; l++) landmarks[track(l)].p = Eigen::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
  for (int i = 0; i < no; i++) {
    auto& kd = corners[fcid(ocam[i])];
    const int fid = (int)kd.corners.size();
    kd.corners.emplace_back(uv[2 * i], uv[2 * i + 1]);
    landmarks[track(olm[i])].obs[fcid(ocam[i])] = fid;
  }
  BundleAdjustmentOptions opts;
  opts.verbosity_level = 0;
  std::ofstream out(argv[2], std::ios::binary);
  auto dump = [&] {
    for (int c = 0; c < nc; c++) put(out, cameras[fcid(c)].T_w_c.data(), 7);
    for (int l = 0; l < nl; l++) put(out, landmarks[track(l)].p.data(), 3);
    for (int k = 0; k < 2; k++) put(out, calib.T_i_c[k].data(), 7);
  };
  bundle_adjustment_rig_extrinsics(corners, opts, fixed_set, calib, cameras, landmarks, free_cam);
  dump();
  bundle_adjustment_rig_extrinsics(corners, opts, all_set, calib, cameras, landmarks, -1);  // nothing free: returns untouched
  dump();
  int threw = 0;
  try {
    bundle_adjustment_rig_extrinsics(corners, opts, fixed_set, calib, cameras, landmarks, 2);
  } catch (const std::invalid_argument&) {
    threw++;
  }
  opts.optimize_intrinsics = true;
  try {
    bundle_adjustment_rig_extrinsics(corners, opts, fixed_set, calib, cameras, landmarks, 1);
  } catch (const std::invalid_argument&) {
    threw++;
  }
  REQUIRE(threw == 2);
  return 0;
}
