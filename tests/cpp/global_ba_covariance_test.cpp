// visnav::global_bundle_adjustment_covariance through the drop-in wrapper (include/visnav_amd/bundle_adjustment.h)
// beside vsl_global_ba_covariance called directly on the same problem.
//   global_ba_covariance_test <ba.bin> <out.bin>   ba.bin as written by tests/test_global_ba_covariance_dropin.py (the
//                                           problem, then the queried camera and landmark ids); out = [wrapper pose
//                                           blocks | wrapper landmark blocks | direct pose blocks | direct landmark
//                                           blocks], row-major, then the two degenerate counts and the two storages as
//                                           doubles
//   global_ba_covariance_test <ba.bin>      host only: runs the flattening helper (all observations: Landmark::all_obs)
//                                           that global_bundle_adjustment and the wrapper share and checks its arrays
//                                           against the file (no device call)
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
  if (argc != 2 && argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t nc, nl, no, nqc, nql;
  get(in, &nc, 1); get(in, &nl, 1); get(in, &no, 1); get(in, &nqc, 1); get(in, &nql, 1);
  std::vector<double> poses(7 * nc), points(3 * nl), uv(2 * no), intr(16);
  std::vector<uint8_t> fixed(nc);
  std::vector<int32_t> ocam(no), olm(no), qc(nqc), ql(nql), cam_intr(nc);
  get(in, poses.data(), poses.size()); get(in, fixed.data(), fixed.size()); get(in, intr.data(), 16);
  get(in, points.data(), points.size()); get(in, ocam.data(), no); get(in, olm.data(), no); get(in, uv.data(), uv.size());
  get(in, qc.data(), nqc); get(in, ql.data(), nql);
  REQUIRE(in.good());
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
    cam_intr[c] = c % 2;
  }
  // track ids that are not the landmark indices, so that a mix-up of the two shows
  auto track = [](int l) { return (TrackId)(1000 + 7 * l); };
  for (int l = 0; l < nl; l++) landmarks[track(l)].p = Eigen::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
  for (int i = 0; i < no; i++) {
    FrameCamId fcid(ocam[i] / 2, ocam[i] % 2);
    auto& kd = corners[fcid];
    const int fid = (int)kd.corners.size();
    kd.corners.emplace_back(uv[2 * i], uv[2 * i + 1]);
    Landmark& lm = landmarks[track(olm[i])];
    lm.all_obs[fcid] = fid;
    if (lm.obs.empty()) lm.obs[fcid] = fid;  // the window's inlier set is NOT what the global calls flatten
  }

  if (argc == 2) {  // the flattening helper alone
    amd::BaFlat f;
    REQUIRE(amd::flatten_ba<true>(corners, fixed_set, calib, cameras, landmarks, f));
    REQUIRE(f.prob.n_cams == nc && f.prob.n_lms == nl && f.prob.n_obs == no);
    REQUIRE(f.lm_id.size() == (size_t)nl && f.cam_id.size() == (size_t)nc);
    for (int c = 0; c < nc; c++) {
      REQUIRE(f.cam_id[c] == FrameCamId(c / 2, c % 2) && f.fixed[c] == fixed[c] && f.cam_intr[c] == c % 2);
      for (int j = 0; j < 7; j++) REQUIRE(f.poses[7 * c + j] == poses[7 * c + j]);
    }
    std::vector<int> seen(no, 0);
    for (int q = 0; q < no; q++) {  // every flattened observation is one of the file's, with its pixel
      const int c = f.obs_cam[q], l = (int)((f.lm_id[f.obs_lm[q]] - 1000) / 7);
      REQUIRE(c >= 0 && c < nc && l >= 0 && l < nl && track(l) == f.lm_id[f.obs_lm[q]]);
      for (int j = 0; j < 3; j++) REQUIRE(f.points[3 * f.obs_lm[q] + j] == points[3 * l + j]);
      int hit = -1;
      for (int i = 0; i < no && hit < 0; i++)
        if (!seen[i] && ocam[i] == c && olm[i] == l && uv[2 * i] == f.uv[2 * q] && uv[2 * i + 1] == f.uv[2 * q + 1]) hit = i;
      REQUIRE(hit >= 0);
      seen[hit] = 1;
    }
    Cameras none;
    amd::BaFlat g;
    REQUIRE(!amd::flatten_ba<true>(corners, fixed_set, calib, none, landmarks, g));
    std::printf("flatten ok: %d cameras, %d landmarks, %d observations\n", nc, nl, no);
    return 0;
  }

  GlobalBundleAdjustmentOptions opts;
  opts.verbosity_level = 0;
  std::vector<FrameCamId> query_cameras;
  std::vector<TrackId> query_landmarks;
  for (int c : qc) query_cameras.emplace_back(c / 2, c % 2);
  for (int l : ql) query_landmarks.push_back(track(l));
  std::map<FrameCamId, PoseCovariance> pose_cov;
  std::unordered_map<TrackId, Eigen::Matrix3d> landmark_cov;
  int storage_wrapper = -1, storage_direct = -1;
  const int nd_wrapper = global_bundle_adjustment_covariance(corners, opts, fixed_set, calib, cameras, landmarks, query_cameras,
                                                             query_landmarks, pose_cov, landmark_cov, &storage_wrapper);
  // (a map has one entry per id: duplicated ids of the query share it)
  REQUIRE(pose_cov.size() == std::set<int32_t>(qc.begin(), qc.end()).size());
  REQUIRE(landmark_cov.size() == std::set<int32_t>(ql.begin(), ql.end()).size());
  for (int c = 0; c < nc; c++)  // nothing is optimised
    for (int j = 0; j < 7; j++) REQUIRE(cameras[FrameCamId(c / 2, c % 2)].T_w_c.data()[j] == poses[7 * c + j]);

  vsl_ba_problem prob;
  prob.n_cams = nc; prob.n_lms = nl; prob.n_obs = no;
  prob.cam_model[0] = prob.cam_model[1] = VSL_CAM_DS;
  prob.poses = poses.data(); prob.cam_fixed = fixed.data(); prob.cam_intr = cam_intr.data(); prob.intr = intr.data();
  prob.points = points.data(); prob.obs_cam = ocam.data(); prob.obs_lm = olm.data(); prob.obs_uv = uv.data();
  vsl_ba_options o;
  o.use_huber = 1; o.huber_parameter = 1.0; o.max_num_iterations = 0; o.verbosity = 0;
  std::vector<double> cp(36 * nqc), cl(9 * nql);
  int nd_direct = -1;
  REQUIRE(vsl_global_ba_covariance(amd::ctx(), &prob, &o, qc.data(), nqc, cp.data(), ql.data(), nql, cl.data(), &nd_direct,
                                   &storage_direct) == VSL_OK);

  std::ofstream out(argv[2], std::ios::binary);
  for (int q = 0; q < nqc; q++)
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) put(out, &pose_cov.at(query_cameras[q])(i, j), 1);
  for (int q = 0; q < nql; q++)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) put(out, &landmark_cov.at(query_landmarks[q])(i, j), 1);
  put(out, cp.data(), cp.size());
  put(out, cl.data(), cl.size());
  const double nd[4] = {(double)nd_wrapper, (double)nd_direct, (double)storage_wrapper, (double)storage_direct};
  put(out, nd, 4);
  return 0;
}
