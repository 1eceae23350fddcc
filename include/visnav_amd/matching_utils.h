// visnav_amd/matching_utils.h -- drop-in for the two stereo helpers of include/visnav/matching_utils.h that
// src/slam.cpp calls on every keyframe (:1136-1150): computeEssential (:56-62) and findInliersEssential (:64-88).
// Same names, arguments and outputs.  computeEssential is three lines of host arithmetic, restated here with the
// rotation built from the pose's quaternion like include/visnav_amd/harness/geometry.h quat_to_rot, so that the nine
// values are those of harness::compute_essential bit for bit.  findInliersEssential flattens the keypoints and the
// match list and calls vsl_find_inliers_essential (include/vslam_hip.h), the device stereo stage.
// (findInliersRansac, :90-135, is OpenGV RANSAC and is not replaced.)
#pragma once
#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "vo_utils.h"  // AmdCameraD, camera_model_id, context holder, types

namespace visnav {

// include/visnav/matching_utils.h:56-62: E = skew(t_0_1 / |t_0_1|) * R_0_1
inline void computeEssential(const Sophus::SE3d& T_0_1, Eigen::Matrix3d& E) {
  const double* d = T_0_1.data();  // qx qy qz qw tx ty tz
  double qx = d[0], qy = d[1], qz = d[2], qw = d[3];
  const double qn = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx /= qn;
  qy /= qn;
  qz /= qn;
  qw /= qn;
  const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)},
                          {2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)},
                          {2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)}};
  const double tn = std::sqrt(d[4] * d[4] + d[5] * d[5] + d[6] * d[6]);
  const double s = 1.0 / tn;
  const double w[3] = {s * d[4], s * d[5], s * d[6]};
  const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double acc = 0;
      for (int k = 0; k < 3; k++) acc += K[i][k] * R[k][j];
      E(i, j) = acc;
    }
}

// include/visnav/matching_utils.h:64-88
inline void findInliersEssential(const KeypointsData& kd1, const KeypointsData& kd2, const std::shared_ptr<AmdCameraD>& cam1,
                                 const std::shared_ptr<AmdCameraD>& cam2, const Eigen::Matrix3d& E,
                                 double epipolar_error_threshold, MatchData& md) {
  md.inliers.clear();
  const int n = (int)md.matches.size();
  if (n == 0) return;
  double e9[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) e9[3 * i + j] = E(i, j);
  std::vector<int32_t> m(2 * (size_t)n), out(2 * (size_t)n);
  for (int k = 0; k < n; k++) {
    m[2 * k] = md.matches[k].first;
    m[2 * k + 1] = md.matches[k].second;
  }
  std::vector<double> xy1, xy2;
  xy1.reserve(2 * kd1.corners.size());
  xy2.reserve(2 * kd2.corners.size());
  for (const auto& c : kd1.corners) xy1.insert(xy1.end(), {c[0], c[1]});
  for (const auto& c : kd2.corners) xy2.insert(xy2.end(), {c[0], c[1]});
  int n_in = 0;
  amd::check(vsl_find_inliers_essential(amd::ctx(), amd::camera_model_id(cam1->name()), cam1->data(),
                                        amd::camera_model_id(cam2->name()), cam2->data(), e9, xy1.data(), (int)kd1.corners.size(),
                                        xy2.data(), (int)kd2.corners.size(), m.data(), n, epipolar_error_threshold, nullptr,
                                        nullptr, out.data(), nullptr, &n_in),
             "findInliersEssential");
  for (int k = 0; k < n_in; k++) md.inliers.emplace_back(out[2 * k], out[2 * k + 1]);
}

}  // namespace visnav
