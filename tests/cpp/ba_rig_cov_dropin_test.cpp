// visnav::bundle_adjustment_rig_covariance, rig_relative_pose_covariance and rig_map_edge_information through the drop-in
// header (include/visnav_amd/bundle_adjustment.h) on a mirror-type map.
//   ba_rig_cov_dropin_test <rig.bin> <out.bin>   rig.bin as written by tests/test_ba_rig_cov_dropin.py (the layout of
//       ba_rig_dropin_test); out = body blocks of the free frames (ascending) | camera blocks of their cameras (file order)
//       | landmark blocks (file order) | per pair of frames (a < b, not both fixed): meas 6, cov 36, info 36
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

static bool same66(const PoseCovariance& a, const PoseCovariance& b) {
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++)
      if (!(a(i, j) == b(i, j))) return false;
  return true;
}

#define REQUIRE(c)                                                     \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) return 2;
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
  std::set<FrameCamId> fixed_set;
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
  std::set<FrameId> fixed_frames, frames;
  for (int c = 0; c < nc; c++) {
    for (int j = 0; j < 7; j++) cameras[fcid(c)].T_w_c.data()[j] = poses[7 * c + j];
    if (fixed[c]) {
      fixed_set.insert(fcid(c));
      fixed_frames.insert(frame[c]);
    }
    frames.insert(frame[c]);
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
  std::vector<FrameId> qf;
  std::vector<FrameCamId> qc;
  std::vector<TrackId> ql;
  for (const FrameId f : frames)
    if (!fixed_frames.count(f)) qf.push_back(f);
  for (int c = 0; c < nc; c++)
    if (!fixed_frames.count(frame[c])) qc.push_back(fcid(c));
  for (int l = 0; l < nl; l++) ql.push_back(track(l));
  std::map<FrameId, PoseCovariance> cb;
  std::map<FrameCamId, PoseCovariance> cc;
  std::unordered_map<TrackId, Eigen::Matrix3d> cl;
  const Cameras before = cameras;
  REQUIRE(bundle_adjustment_rig_covariance(corners, opts, fixed_set, calib, cameras, landmarks, qf, qc, ql, cb, cc, cl) == 0);
  REQUIRE(cb.size() == qf.size() && cc.size() == qc.size() && cl.size() == ql.size());
  for (const auto& kv : before)  // nothing is written to the map
    for (int j = 0; j < 7; j++) REQUIRE(kv.second.T_w_c.data()[j] == cameras.at(kv.first).T_w_c.data()[j]);
  std::ofstream out(argv[2], std::ios::binary);
  auto put66 = [&](const PoseCovariance& m) {
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) { const double v = m(i, j); put(out, &v, 1); }
  };
  for (const FrameId f : qf) put66(cb.at(f));
  for (const FrameCamId& c : qc) put66(cc.at(c));
  for (const TrackId t : ql)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) { const double v = cl.at(t)(i, j); put(out, &v, 1); }
  // camera 0 is the body frame: its block is the body's, compared with ==
  for (const FrameCamId& c : qc)
    if (c.cam_id == 0) REQUIRE(same66(cc.at(c), cb.at(c.frame_id)));
  std::vector<std::pair<FrameId, FrameId>> pairs;
  for (const FrameId a : frames)
    for (const FrameId b : frames)
      if (a < b && !(fixed_frames.count(a) && fixed_frames.count(b))) pairs.emplace_back(a, b);
  std::vector<RelativePoseCovariance> rel;
  REQUIRE(rig_relative_pose_covariance(corners, opts, fixed_set, calib, cameras, landmarks, pairs, rel) == 0);
  REQUIRE(rel.size() == pairs.size());
  for (const RelativePoseCovariance& r : rel) {
    REQUIRE(r.valid);
    put(out, r.measurement, 6);
    put66(r.cov);
    put66(r.info);
  }
  // the edge table: map pairs answered with the bits of the pair call, everything else with the default
  std::vector<std::pair<FrameId, FrameId>> edges = pairs;
  edges.emplace_back(*frames.begin(), *frames.begin());  // the same frame twice
  edges.emplace_back(*frames.begin(), (FrameId)9999);    // not in the map
  PoseCovariance dflt;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) dflt(i, j) = i == j ? 7.0 : 0.0;
  const RigEdgeInformation e = rig_map_edge_information(corners, opts, fixed_set, calib, cameras, landmarks, edges, dflt);
  REQUIRE(e.n_map_edges == pairs.size() && e.edge_info.size() == edges.size());
  for (size_t q = 0; q < pairs.size(); q++) {
    REQUIRE(e.from_map[q] && same66(e.edge_info[q], rel[q].info));
    for (int i = 0; i < 6; i++) REQUIRE(e.edge_meas[q][i] == rel[q].measurement[i]);
  }
  for (size_t q = pairs.size(); q < edges.size(); q++) REQUIRE(!e.from_map[q] && same66(e.edge_info[q], dflt));
  // refusals: an unknown frame, a fixed frame, an empty query
  bool threw = false;
  try {
    bundle_adjustment_rig_covariance(corners, opts, fixed_set, calib, cameras, landmarks, {(FrameId)9999}, {}, {}, cb, cc, cl);
  } catch (const std::out_of_range&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try {
    bundle_adjustment_rig_covariance(corners, opts, fixed_set, calib, cameras, landmarks, {*fixed_frames.begin()}, {}, {}, cb, cc, cl);
  } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  REQUIRE(bundle_adjustment_rig_covariance(corners, opts, fixed_set, calib, cameras, landmarks, {}, {}, {}, cb, cc, cl) == 0 && cb.empty());
  return 0;
}
