// visnav::relative_pose_covariance (both overloads, include/visnav_amd/bundle_adjustment.h) beside
// vsl_ba_relative_pose_covariance / vsl_global_ba_relative_pose_covariance called directly on the same flattened problem,
// and visnav::map_edge_information (include/visnav_amd/loop_closure.h) handed to pose_graph_optimization.
//   relative_pose_covariance_test <ba.bin>   ba.bin as written by tests/test_relative_pose_covariance_dropin.py: the
//                                            problem of ba_covariance_test.cpp; the queried camera ids are read two by two
//                                            as pairs (a, b).
// The keyframe map: the left camera of every frame, the last frame is the current keyframe (not in `keyframes`), the
// spanning tree runs back frame by frame, every keyframe is covisible with the two before it (weight above the essential
// threshold) with the relative pose of the map, the loop candidate is frame 0.
// Without a device only the host part runs (argument "host" after the file): the enumeration of the map's edges.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "visnav_amd/loop_closure.h"

using namespace visnav;

template <class T>
static void get(std::ifstream& i, T* p, size_t n) { i.read(reinterpret_cast<char*>(p), sizeof(T) * n); }

#define REQUIRE(c)                                                     \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static bool same(const PoseCovariance& m, const double* d) {
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++)
      if (std::memcmp(&m(i, j), d + 6 * i + j, sizeof(double))) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) return 2;
  const bool host_only = argc == 3;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t nc, nl, no, nqc, nql;
  get(in, &nc, 1); get(in, &nl, 1); get(in, &no, 1); get(in, &nqc, 1); get(in, &nql, 1);
  std::vector<double> poses(7 * nc), points(3 * nl), uv(2 * no), intr(16);
  std::vector<uint8_t> fixed(nc);
  std::vector<int32_t> ocam(no), olm(no), qc(nqc), ql(nql);
  get(in, poses.data(), poses.size()); get(in, fixed.data(), fixed.size()); get(in, intr.data(), 16);
  get(in, points.data(), points.size()); get(in, ocam.data(), no); get(in, olm.data(), no); get(in, uv.data(), uv.size());
  get(in, qc.data(), nqc); get(in, ql.data(), nql);
  REQUIRE(in.good() && nqc % 2 == 0 && nc % 2 == 0 && nc >= 8);
  Cameras cameras;
  Landmarks landmarks;
  Corners corners;
  std::set<FrameCamId> fixed_set;
  Calibration calib;
  for (int k = 0; k < 2; k++) {
    auto c = std::make_shared<AbstractCameraD>();
    c->model = "ds";
    for (int j = 0; j < 8; j++) c->param[j] = intr[8 * k + j];
    calib.intrinsics.push_back(c);
  }
  for (int c = 0; c < nc; c++) {
    FrameCamId fcid(c / 2, c % 2);
    for (int j = 0; j < 7; j++) cameras[fcid].T_w_c.data()[j] = poses[7 * c + j];
    if (fixed[c]) fixed_set.insert(fcid);
    corners[fcid];
  }
  auto track = [](int l) { return (TrackId)(1000 + 7 * l); };
  for (int l = 0; l < nl; l++) landmarks[track(l)].p = Eigen::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
  for (int i = 0; i < no; i++) {
    FrameCamId fcid(ocam[i] / 2, ocam[i] % 2);
    auto& kd = corners[fcid];
    const int fid = (int)kd.corners.size();
    kd.corners.emplace_back(uv[2 * i], uv[2 * i + 1]);
    landmarks[track(olm[i])].obs[fcid] = fid;
    landmarks[track(olm[i])].all_obs[fcid] = fid;
  }
  std::vector<std::pair<FrameCamId, FrameCamId>> pairs;
  for (int q = 0; q < nqc; q += 2) pairs.emplace_back(FrameCamId(qc[q] / 2, qc[q] % 2), FrameCamId(qc[q + 1] / 2, qc[q + 1] % 2));
  const size_t np = pairs.size();

  // ---- the keyframe map
  const int F = nc / 2, essential = 50;
  std::vector<Camera> kf(F);
  for (int i = 0; i < F; i++) {
    kf[i].T_w_c = cameras.at(FrameCamId(i, 0)).T_w_c;
    kf[i].last_fcid = FrameCamId(i - 1, 0);  // frame 0: -1 = none
    for (int j = std::max(0, i - 2); j < i; j++) {
      kf[i].covisible_weights[FrameCamId(j, 0)] = 100;
      kf[i].covisible_rel_poses[FrameCamId(j, 0)] =
          amd::se3_of(amd::rt_mul(amd::rt_inv(amd::rt_of(kf[i].T_w_c)), amd::rt_of(cameras.at(FrameCamId(j, 0)).T_w_c)));
    }
  }
  Cameras keyframes;
  for (int i = 0; i < F - 1; i++) keyframes[FrameCamId(i, 0)] = kf[i];
  Camera cur = kf[F - 1];
  const FrameCamId cur_id(F - 1, 0), cand_id(0, 0);
  // the Sim(3) constraint as the reference forms it: T_candidate^-1 T_current at the poses as they stand
  const Sophus::SE3d sim3 = amd::se3_of(amd::rt_mul(amd::rt_inv(amd::rt_of(kf[0].T_w_c)), amd::rt_of(cur.T_w_c)));
  LoopClosureOptions lc;
  lc.verbosity_level = 0;
  lc.set_current_kf_fixed = true;

  // host: the edges the map can answer -- every covisibility edge (i, i - 1), (i, i - 2), less the pair of the two fixed
  // cameras if both are left cameras; never the loop edge
  const auto map_pairs = amd::map_edge_pairs(cur_id, cur, cand_id, sim3, keyframes, essential, lc, fixed_set, cameras);
  size_t expect = 0;
  for (int i = 0; i < F; i++)
    for (int j = std::max(0, i - 2); j < i; j++)
      expect += !(fixed_set.count(FrameCamId(i, 0)) && fixed_set.count(FrameCamId(j, 0)));
  REQUIRE(map_pairs.size() == expect && expect >= 3);
  for (const auto& p : map_pairs) REQUIRE(!(p.first == cur_id && p.second == cand_id) && p.first.cam_id == 0 && p.second.cam_id == 0);
  {
    Cameras few = cameras;  // a camera that is not in the bundle adjustment: its edges leave the list
    few.erase(FrameCamId(1, 0));
    const auto fewer = amd::map_edge_pairs(cur_id, cur, cand_id, sim3, keyframes, essential, lc, fixed_set, few);
    REQUIRE(fewer.size() < map_pairs.size());
    for (const auto& p : fewer) REQUIRE(!(p.first == FrameCamId(1, 0)) && !(p.second == FrameCamId(1, 0)));
  }
  if (host_only) {
    std::printf("host ok: %zu map edges of %d keyframes\n", map_pairs.size(), F);
    return 0;
  }

  // ---- both overloads against the C ABI on the same flattened problem, bit for bit
  vsl_ba_options o;
  o.use_huber = 1; o.huber_parameter = 1.0; o.max_num_iterations = 0; o.verbosity = 0;
  for (int global = 0; global < 2; global++) {
    std::vector<RelativePoseCovariance> out;
    int storage = -1, ns;
    if (global) {
      GlobalBundleAdjustmentOptions g;
      ns = relative_pose_covariance(corners, g, fixed_set, calib, cameras, landmarks, pairs, out, &storage);
    } else {
      BundleAdjustmentOptions b;
      b.verbosity_level = 0;
      ns = relative_pose_covariance(corners, b, fixed_set, calib, cameras, landmarks, pairs, out);
    }
    REQUIRE(ns == 0 && out.size() == np && (!global || storage == 0));
    amd::BaFlat f;
    REQUIRE(global ? amd::flatten_ba<true>(corners, fixed_set, calib, cameras, landmarks, f)
                   : amd::flatten_ba<false>(corners, fixed_set, calib, cameras, landmarks, f));
    std::vector<int32_t> a, b;  // (FrameCamId(c / 2, c % 2) sorts like c: the flattened index is the file's camera id)
    for (int q = 0; q < nqc; q += 2) {
      a.push_back(qc[q]);
      b.push_back(qc[q + 1]);
    }
    for (size_t q = 0; q < np; q++) REQUIRE(f.cam_id[a[q]] == pairs[q].first && f.cam_id[b[q]] == pairs[q].second);
    std::vector<double> meas(6 * np), cov(36 * np), info(36 * np);
    int ns_direct = -1, st_direct = -1;
    const int rc = global ? vsl_global_ba_relative_pose_covariance(amd::ctx(), &f.prob, &o, a.data(), b.data(), (int)np, nullptr,
                                                                   meas.data(), cov.data(), info.data(), &ns_direct, &st_direct)
                          : vsl_ba_relative_pose_covariance(amd::ctx(), &f.prob, &o, a.data(), b.data(), (int)np, nullptr, meas.data(),
                                                            cov.data(), info.data(), &ns_direct);
    REQUIRE(rc == VSL_OK && ns_direct == 0);
    for (size_t q = 0; q < np; q++) {
      REQUIRE(out[q].valid && !std::memcmp(out[q].measurement, meas.data() + 6 * q, 6 * sizeof(double)));
      REQUIRE(same(out[q].cov, cov.data() + 36 * q) && same(out[q].info, info.data() + 36 * q));
    }
  }
  {  // an unknown camera
    std::vector<RelativePoseCovariance> out;
    BundleAdjustmentOptions b;
    bool thrown = false;
    try {
      relative_pose_covariance(corners, b, fixed_set, calib, cameras, landmarks, {{FrameCamId(2, 0), FrameCamId(F + 5, 0)}}, out);
    } catch (const std::out_of_range&) {
      thrown = true;
    }
    REQUIRE(thrown);
  }

  // ---- map_edge_information: the map's edges from one query, the default for the loop edge, and the solve takes it
  PoseCovariance dflt;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) dflt(i, j) = i == j ? 123.0 : 0.0;
  GlobalBundleAdjustmentOptions g;
  size_t n_map = 0;
  const EdgeInformation information = map_edge_information(cur_id, cur, cand_id, sim3, keyframes, essential, lc, corners, g, fixed_set,
                                                           calib, cameras, landmarks, dflt, &n_map);
  REQUIRE(n_map == map_pairs.size());
  const PoseCovariance loop = information(cur_id, cand_id), off_map = information(FrameCamId(0, 0), FrameCamId(F - 1, 0));
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) REQUIRE(loop(i, j) == dflt(i, j) && off_map(i, j) == dflt(i, j));
  {
    std::vector<RelativePoseCovariance> out;
    relative_pose_covariance(corners, g, fixed_set, calib, cameras, landmarks, map_pairs, out);
    for (size_t q = 0; q < map_pairs.size(); q++) {
      const PoseCovariance W = information(map_pairs[q].first, map_pairs[q].second);
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) REQUIRE(!std::memcmp(&W(i, j), &out[q].info(i, j), sizeof(double)) && W(i, j) == W(j, i));
      REQUIRE(W(0, 0) > 0 && W(0, 0) != 123.0);
    }
  }
  // every edge of the flattened graph gets a matrix, exactly one of them the default (the loop edge)
  amd::PgoFlat f;
  amd::flatten_pose_graph(cur_id, cur, cand_id, sim3, keyframes, essential, lc, information, f);
  int defaults = 0;
  for (int e = 0; e < f.prob.n_edges; e++) defaults += f.info[36 * (size_t)e] == 123.0;
  REQUIRE(f.info.size() == 36 * (size_t)f.prob.n_edges);
  REQUIRE(defaults == 1);
  pose_graph_optimization(cur_id, cur, cand_id, sim3, keyframes, essential, lc, information);  // throws if an Omega is refused
  for (int i = 0; i < F - 1; i++)
    for (int c = 0; c < 7; c++) REQUIRE(std::isfinite(keyframes[FrameCamId(i, 0)].T_w_c.data()[c]));
  std::printf("drop-in ok: %zu pairs on both overloads, %zu map edges, loop edge answered with the default\n", np, n_map);
  return 0;
}
