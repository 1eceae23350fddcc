// visnav_amd/bundle_adjustment.h -- drop-in for visnav::bundle_adjustment
// (include/visnav/map_utils.h:319-421) and visnav::global_bundle_adjustment
// (include/visnav/loop_closure_utils.h:651-748).  The wrappers flatten the reference's node-based
// containers (Cameras = std::map, Landmarks = unordered_map, Corners = concurrent map) into the SoA
// arrays of vsl_ba_problem, call the MI355X solver, and write poses / landmark positions back in
// place -- the contract of the Ceres version (parameter blocks are the containers' own storage).
#pragma once
#include <stdexcept>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <array>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <map>
#include <utility>
#include <vector>

#include "keypoints.h"  // context holder + types

// relative_pose_covariance (below) references its entry points weakly, like the _w ones of loop_closure.h
#pragma weak vsl_ba_relative_pose_covariance
#pragma weak vsl_global_ba_relative_pose_covariance
// bundle_adjustment_rig (below): likewise
#pragma weak vsl_bundle_adjust_rig
// bundle_adjustment_rig_extrinsics (below): likewise
#pragma weak vsl_bundle_adjust_rig_ext
// global_bundle_adjustment_rig (below): likewise
#pragma weak vsl_global_bundle_adjust_rig
// bundle_adjustment_rig_covariance, rig_relative_pose_covariance, rig_map_edge_information (below): likewise
#pragma weak vsl_ba_rig_covariance
#pragma weak vsl_ba_rig_relative_pose_covariance
#pragma weak vsl_ba_rig_ext_covariance

namespace visnav {

// include/visnav/map_utils.h:319-334
struct BundleAdjustmentOptions {
  int verbosity_level = 1;
  bool optimize_intrinsics = false;
  bool use_huber = true;
  double huber_parameter = 1.0;
  int max_num_iterations = 20;
};
// include/visnav/loop_closure_utils.h:651-663
struct GlobalBundleAdjustmentOptions {
  int verbosity_level = 1;
  bool use_huber = true;
  double huber_parameter = 1.0;
  int max_num_iterations = 20;
};

namespace amd {
inline int camera_model_id(const std::string& name) {
  if (name == "ds") return VSL_CAM_DS;
  if (name == "pinhole") return VSL_CAM_PINHOLE;
  if (name == "eucm") return VSL_CAM_EUCM;
  if (name == "kb4") return VSL_CAM_KB4;
  std::fprintf(stderr, "Camera model %s is not implemented.\n", name.c_str());  // camera_models.h:493-495
  std::abort();
}

// The flattened problem: the SoA arrays of vsl_ba_problem with the containers' entries they came from.  `prob` points
// into the vectors, so a BaFlat stays where it was filled.
struct BaFlat {
  std::vector<double> poses, points, uv, intr = std::vector<double>(16, 0.0);
  std::vector<uint8_t> fixed;
  std::vector<int32_t> cam_intr, obs_cam, obs_lm;
  std::vector<Camera*> cam_ptr;      // camera index -> the map's entry (std::map order)
  std::vector<Landmark*> lm_ptr;     // landmark index -> the map's entry (the container's iteration order)
  std::vector<FrameCamId> cam_id;
  std::vector<TrackId> lm_id;
  vsl_ba_problem prob;
};

// Cameras / Landmarks / Corners -> f (run_ba and bundle_adjustment_covariance share it).  false: nothing to solve (no
// camera, no landmark or no observation).
template <bool kAllObs>
inline bool flatten_ba(const Corners& feature_corners, const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam,
                       Cameras& cameras, Landmarks& landmarks, BaFlat& f) {
  if (cameras.empty() || landmarks.empty()) return false;
  // cameras in std::map order; an observation list (std::map<FrameCamId, FeatureId>) is walked against it with two
  // cursors instead of two tree lookups per observation (20 k observations per local window)
  std::vector<const KeypointsData*> cam_kd;
  for (auto& kv : cameras) {  // std::map order == the order Ceres receives the blocks (map_utils.h:359)
    f.cam_id.push_back(kv.first);
    const auto kd = feature_corners.find(kv.first);
    cam_kd.push_back(kd == feature_corners.end() ? nullptr : &kd->second);
    f.cam_ptr.push_back(&kv.second);
    const double* d = kv.second.T_w_c.data();
    f.poses.insert(f.poses.end(), d, d + 7);
    f.fixed.push_back(fixed_cameras.count(kv.first) ? 1 : 0);
    f.cam_intr.push_back((int32_t)kv.first.cam_id);
  }
  for (auto& kv : landmarks) {
    Landmark& lm = kv.second;
    const auto& track = kAllObs ? lm.all_obs : lm.obs;  // loop_closure_utils.h:706 vs map_utils.h:373
    const int li = (int)f.lm_ptr.size();
    f.lm_ptr.push_back(&lm);
    f.lm_id.push_back(kv.first);
    f.points.insert(f.points.end(), lm.p.data(), lm.p.data() + 3);
    size_t ci = 0;
    for (const auto& ob : track) {
      while (ci < f.cam_id.size() && f.cam_id[ci] < ob.first) ci++;
      if (ci == f.cam_id.size() || ob.first < f.cam_id[ci] || !cam_kd[ci])  // .at(): std::out_of_range like the reference
        throw std::out_of_range("bundle_adjustment: an observation refers to a camera / keypoint set that is not there");
      const auto& p_2d = cam_kd[ci]->corners[ob.second];
      f.obs_cam.push_back((int32_t)ci);
      f.obs_lm.push_back(li);
      f.uv.push_back(p_2d[0]);
      f.uv.push_back(p_2d[1]);
    }
  }
  if (f.obs_cam.empty()) return false;
  vsl_ba_problem& prob = f.prob;
  prob.n_cams = (int32_t)f.cam_ptr.size();
  prob.n_lms = (int32_t)f.lm_ptr.size();
  prob.n_obs = (int32_t)f.obs_cam.size();
  for (int k = 0; k < 2; k++) {
    prob.cam_model[k] = camera_model_id(calib_cam.intrinsics[k]->name());
    const double* p = calib_cam.intrinsics[k]->data();
    for (int j = 0; j < 8; j++) f.intr[8 * k + j] = p[j];
  }
  prob.poses = f.poses.data();
  prob.cam_fixed = f.fixed.data();
  prob.cam_intr = f.cam_intr.data();
  prob.intr = f.intr.data();
  prob.points = f.points.data();
  prob.obs_cam = f.obs_cam.data();
  prob.obs_lm = f.obs_lm.data();
  prob.obs_uv = f.uv.data();
  return true;
}

template <bool kAllObs>
inline void run_ba(const Corners& feature_corners, bool use_huber, double huber_parameter, int max_num_iterations,
                   int verbosity_level, const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam,
                   Cameras& cameras, Landmarks& landmarks, bool optimize_intrinsics = false) {
  BaFlat f;
  if (!flatten_ba<kAllObs>(feature_corners, fixed_cameras, calib_cam, cameras, landmarks, f)) return;
  std::vector<double>&poses = f.poses, &points = f.points, &intr = f.intr;
  std::vector<Camera*>& cam_ptr = f.cam_ptr;
  std::vector<Landmark*>& lm_ptr = f.lm_ptr;
  vsl_ba_problem& prob = f.prob;
  vsl_ba_options opt;
  opt.use_huber = use_huber ? 1 : 0;
  opt.huber_parameter = huber_parameter;
  opt.max_num_iterations = max_num_iterations;
  opt.verbosity = 0;
  vsl_ba_summary sum;
#ifdef VISNAV_AMD_HAVE_RCCL
  // multi-GPU global bundle adjustment: every rank runs this call on the same map (rccl_world.h)
  if (kAllObs && RcclWorld::instance().enabled()) {
    RcclWorld& w = RcclWorld::instance();
    check(vsl_global_bundle_adjust(ctx(), &prob, &opt, &RcclWorld::allreduce, &w, w.rank(), w.world(), &sum),
          "global_bundle_adjustment (RCCL)");
  } else
#endif
  if (optimize_intrinsics) {  // map_utils.h:397-403: the intrinsics blocks stay variable and are written back
    check(vsl_bundle_adjust_intrinsics(ctx(), &prob, &opt, intr.data(), &sum), "bundle_adjustment (optimize_intrinsics)");
    for (int k = 0; k < 2; k++)
      for (int j = 0; j < 8; j++) calib_cam.intrinsics[k]->data()[j] = intr[8 * k + j];
  } else if (std::getenv("VISNAV_AMD_BA_SELFCHECK")) {  // diagnostic: the same problem solved twice must give the same bits
    const std::vector<double> poses0 = poses, points0 = points;
    check(vsl_bundle_adjust(ctx(), &prob, &opt, &sum), "bundle_adjustment");
    const std::vector<double> poses1 = poses, points1 = points;
    const int it1 = sum.iterations;
    poses = poses0;
    points = points0;
    prob.poses = poses.data();
    prob.points = points.data();
    check(vsl_bundle_adjust(ctx(), &prob, &opt, &sum), "bundle_adjustment");
    double dmax = 0;
    size_t nd = 0;
    for (size_t i = 0; i < poses.size(); i++) if (poses[i] != poses1[i]) { nd++; dmax = std::max(dmax, std::fabs(poses[i] - poses1[i])); }
    for (size_t i = 0; i < points.size(); i++) if (points[i] != points1[i]) { nd++; dmax = std::max(dmax, std::fabs(points[i] - points1[i])); }
    std::fprintf(stderr, "  BA selfcheck: %d cameras %d landmarks %d observations, iterations %d / %d, %zu values differ (max %.3g)\n", prob.n_cams, prob.n_lms,
                 prob.n_obs, it1, (int)sum.iterations, nd, dmax);
  } else
    check(vsl_bundle_adjust(ctx(), &prob, &opt, &sum), "bundle_adjustment");
  for (size_t c = 0; c < cam_ptr.size(); c++) {
    double* d = cam_ptr[c]->T_w_c.data();
    for (int j = 0; j < 7; j++) d[j] = poses[7 * c + j];
  }
  for (size_t l = 0; l < lm_ptr.size(); l++)
    for (int j = 0; j < 3; j++) lm_ptr[l]->p.data()[j] = points[3 * l + j];
  if (verbosity_level >= 1)  // stands in for summary.BriefReport() (map_utils.h:414-415)
    std::printf("vslam_hip BA: iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n",
                sum.iterations, sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
}
}  // namespace amd

// include/visnav/map_utils.h:337-421, including options.optimize_intrinsics (:397-403; the reference wires it to a
// hidden GUI variable that defaults to false, src/slam.cpp:304, :1545): the two intrinsics blocks are then optimised
// with the poses and landmarks and calib_cam.intrinsics is updated.
inline void bundle_adjustment(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                              const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                              Landmarks& landmarks) {
  amd::run_ba<false>(feature_corners, options.use_huber, options.huber_parameter, options.max_num_iterations,
                     options.verbosity_level, fixed_cameras, calib_cam, cameras, landmarks, options.optimize_intrinsics);
}

// Rig-constrained bundle adjustment (vsl_bundle_adjust_rig; the reference has no counterpart: src/slam.cpp:1215 sets
// T_w_c_right = pose * T_0_1 once and Ceres then moves the two cameras of a frame apart).  One SE(3) block per FRAME,
// the calibrated extrinsics held fixed.  Bodies are the FrameIds of `cameras` in ascending order; the body frame is
// camera 0: T_b_c[k] = T_i_c[0]^-1 * T_i_c[k] (k = 0: the identity, exactly).  A body is fixed if any of its cameras is
// in fixed_cameras.  The body pose handed in is T_w_c of camera 0 where the frame has it, else T_w_c[k] * T_b_c[k]^-1 of
// the camera that is there.  The problem is flattened by flatten_ba exactly as for bundle_adjustment (lm.obs).  ALL
// camera poses are written back, derived from the optimised bodies (a frame whose cameras had drifted apart comes back
// on the calibration), and the landmarks.  A window whose frames are all fixed returns untouched.  optimize_intrinsics is not offered in rig form (std::invalid_argument).
namespace amd {
inline void se3_mul7(const double* a, const double* b, double* o) {  // o = a * b, qx qy qz qw tx ty tz
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
  const double q[4] = {aw * b[0] + ax * b[3] + ay * b[2] - az * b[1], aw * b[1] - ax * b[2] + ay * b[3] + az * b[0],
                       aw * b[2] + ax * b[1] - ay * b[0] + az * b[3], aw * b[3] - ax * b[0] - ay * b[1] - az * b[2]};
  const double R[9] = {1 - 2 * (ay * ay + az * az), 2 * (ax * ay - az * aw),     2 * (ax * az + ay * aw),
                       2 * (ax * ay + az * aw),     1 - 2 * (ax * ax + az * az), 2 * (ay * az - ax * aw),
                       2 * (ax * az - ay * aw),     2 * (ay * az + ax * aw),     1 - 2 * (ax * ax + ay * ay)};
  double t[3];
  for (int i = 0; i < 3; i++) t[i] = a[4 + i] + R[3 * i] * b[4] + R[3 * i + 1] * b[5] + R[3 * i + 2] * b[6];
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) o[i] = q[i] / n;
  for (int i = 0; i < 3; i++) o[4 + i] = t[i];
}
inline void se3_inv7(const double* a, double* o) {  // o = a^-1
  const double c[7] = {-a[0], -a[1], -a[2], a[3], 0, 0, 0}, mt[7] = {0, 0, 0, 1, -a[4], -a[5], -a[6]};
  se3_mul7(c, mt, o);
}
}  // namespace amd

namespace amd {
// What the rig calls share: the flattening of bundle_adjustment (flatten_ba, lm.obs) plus the rig of the rules above.
// Not copyable once filled (prob and rig point into the members).
struct RigFlat {
  BaFlat f;
  double T_b_c[14] = {0, 0, 0, 1, 0, 0, 0}, T_c_b[14] = {0, 0, 0, 1, 0, 0, 0};
  std::vector<double> body_poses;
  std::vector<uint8_t> body_fixed;
  std::vector<int32_t> cam_body;
  std::vector<FrameId> body_frame;  // ascending
  vsl_ba_rig rig;
  bool any_free = false;
  RigFlat() = default;
  RigFlat(const RigFlat&) = delete;
  RigFlat& operator=(const RigFlat&) = delete;
  int32_t body_of(FrameId frame) const {  // -1: not a frame of the problem
    const auto it = std::lower_bound(body_frame.begin(), body_frame.end(), frame);
    return it == body_frame.end() || *it != frame ? -1 : (int32_t)(it - body_frame.begin());
  }
};
// false: the map has no observation (nothing is filled).  GLOBAL: the flattening of global_bundle_adjustment (ALL
// observations of the landmarks) instead of bundle_adjustment's
template <bool GLOBAL = false>
inline bool flatten_rig(const char* what, const Corners& feature_corners, const std::set<FrameCamId>& fixed_cameras,
                        Calibration& calib_cam, Cameras& cameras, Landmarks& landmarks, RigFlat& r) {
  if (calib_cam.T_i_c.size() < 2) throw std::invalid_argument(std::string(what) + ": the calibration needs two extrinsics");
  BaFlat& f = r.f;
  if (!flatten_ba<GLOBAL>(feature_corners, fixed_cameras, calib_cam, cameras, landmarks, f)) return false;
  double inv0[7];
  se3_inv7(calib_cam.T_i_c[0].data(), inv0);
  se3_mul7(inv0, calib_cam.T_i_c[1].data(), r.T_b_c + 7);
  se3_inv7(r.T_b_c + 7, r.T_c_b + 7);
  // bodies = frames, ascending: cam_id is in std::map order, i.e. by frame, camera 0 before camera 1
  r.cam_body.resize(f.cam_id.size());
  for (size_t c = 0; c < f.cam_id.size(); c++) {
    const bool first = c == 0 || f.cam_id[c - 1].frame_id != f.cam_id[c].frame_id;
    if (first) {
      double b[7];
      const int k = (int)f.cam_id[c].cam_id;
      if (k == 0) std::copy(&f.poses[7 * c], &f.poses[7 * c] + 7, b);
      else se3_mul7(&f.poses[7 * c], r.T_c_b + 7 * k, b);
      r.body_poses.insert(r.body_poses.end(), b, b + 7);
      r.body_fixed.push_back(0);
      r.body_frame.push_back(f.cam_id[c].frame_id);
    }
    r.cam_body[c] = (int32_t)r.body_fixed.size() - 1;
    if (f.fixed[c]) r.body_fixed.back() = 1;
  }
  r.any_free = std::find(r.body_fixed.begin(), r.body_fixed.end(), (uint8_t)0) != r.body_fixed.end();
  r.rig.n_bodies = (int32_t)r.body_fixed.size();
  r.rig.body_poses = r.body_poses.data();
  r.rig.body_fixed = r.body_fixed.data();
  r.rig.cam_body = r.cam_body.data();
  r.rig.T_b_c = r.T_b_c;
  return true;
}
}  // namespace amd

inline void bundle_adjustment_rig(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                  const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                  Landmarks& landmarks) {
  if (&vsl_bundle_adjust_rig == nullptr) throw std::runtime_error("bundle_adjustment_rig: libvslam_hip.so has no vsl_bundle_adjust_rig");
  if (options.optimize_intrinsics) throw std::invalid_argument("bundle_adjustment_rig: optimize_intrinsics is not offered in rig form");
  amd::RigFlat r;
  if (!amd::flatten_rig("bundle_adjustment_rig", feature_corners, fixed_cameras, calib_cam, cameras, landmarks, r)) return;
  // a window of fixed frames only (the application's first keyframe): nothing to optimise, as on the default path
  if (!r.any_free) return;
  amd::BaFlat& f = r.f;
  vsl_ba_options opt;
  opt.use_huber = options.use_huber ? 1 : 0;
  opt.huber_parameter = options.huber_parameter;
  opt.max_num_iterations = options.max_num_iterations;
  opt.verbosity = 0;
  vsl_ba_summary sum;
  amd::check(vsl_bundle_adjust_rig(amd::ctx(), &f.prob, &r.rig, &opt, &sum), "bundle_adjustment_rig");
  for (size_t c = 0; c < f.cam_ptr.size(); c++) std::copy(&f.poses[7 * c], &f.poses[7 * c] + 7, f.cam_ptr[c]->T_w_c.data());
  for (size_t l = 0; l < f.lm_ptr.size(); l++)
    for (int j = 0; j < 3; j++) f.lm_ptr[l]->p.data()[j] = f.points[3 * l + j];
  if (options.verbosity_level >= 1)
    std::printf("vslam_hip rig BA: %d bodies, iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n",
                (int)r.rig.n_bodies, sum.iterations, sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
}

// bundle_adjustment_rig with the extrinsic of ONE camera estimated beside the bodies (vsl_bundle_adjust_rig_ext, online
// extrinsic refinement): the argument list of bundle_adjustment_rig plus free_extrinsic_camera, the camera (0 or 1) whose
// T_i_c is an unknown; -1: none, which is bundle_adjustment_rig itself.  The flattening and the body rules are
// bundle_adjustment_rig's (amd::flatten_rig: the body frame is camera 0 AT THE CALIBRATION HANDED IN).  On return
// calib_cam.T_i_c[free_extrinsic_camera] = T_i_c[0] * (refined T_b_c) -- for camera 0 itself the refined T_b_c[0] is no
// longer the identity --, every camera pose is body * refined T_b_c, and the landmarks are updated.  A window whose
// frames are all fixed is still solved when an extrinsic is free (calibration against fixed poses); with none free it
// returns untouched.  The baseline's LENGTH is observable only with two fixed frames at different places (the header's
// gauge statement).  optimize_intrinsics is not offered (std::invalid_argument).
inline void bundle_adjustment_rig_extrinsics(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                             const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                             Landmarks& landmarks, int free_extrinsic_camera) {
  if (&vsl_bundle_adjust_rig_ext == nullptr)
    throw std::runtime_error("bundle_adjustment_rig_extrinsics: libvslam_hip.so has no vsl_bundle_adjust_rig_ext");
  if (options.optimize_intrinsics)
    throw std::invalid_argument("bundle_adjustment_rig_extrinsics: optimize_intrinsics is not offered in rig form");
  if (free_extrinsic_camera < -1 || free_extrinsic_camera > 1)
    throw std::invalid_argument("bundle_adjustment_rig_extrinsics: free_extrinsic_camera is -1, 0 or 1");
  amd::RigFlat r;
  if (!amd::flatten_rig("bundle_adjustment_rig_extrinsics", feature_corners, fixed_cameras, calib_cam, cameras, landmarks, r)) return;
  if (!r.any_free && free_extrinsic_camera < 0) return;
  amd::BaFlat& f = r.f;
  vsl_ba_options opt;
  opt.use_huber = options.use_huber ? 1 : 0;
  opt.huber_parameter = options.huber_parameter;
  opt.max_num_iterations = options.max_num_iterations;
  opt.verbosity = 0;
  vsl_ba_summary sum;
  const uint8_t ext_free[2] = {(uint8_t)(free_extrinsic_camera == 0), (uint8_t)(free_extrinsic_camera == 1)};
  double T_b_c[14];
  std::copy(r.T_b_c, r.T_b_c + 14, T_b_c);
  amd::check(vsl_bundle_adjust_rig_ext(amd::ctx(), &f.prob, &r.rig, ext_free, T_b_c, &opt, &sum), "bundle_adjustment_rig_extrinsics");
  if (free_extrinsic_camera >= 0) {
    double T_i_c[7];
    amd::se3_mul7(calib_cam.T_i_c[0].data(), T_b_c + 7 * free_extrinsic_camera, T_i_c);
    std::copy(T_i_c, T_i_c + 7, calib_cam.T_i_c[free_extrinsic_camera].data());
  }
  for (size_t c = 0; c < f.cam_ptr.size(); c++) std::copy(&f.poses[7 * c], &f.poses[7 * c] + 7, f.cam_ptr[c]->T_w_c.data());
  for (size_t l = 0; l < f.lm_ptr.size(); l++)
    for (int j = 0; j < 3; j++) f.lm_ptr[l]->p.data()[j] = f.points[3 * l + j];
  if (options.verbosity_level >= 1)
    std::printf("vslam_hip rig BA (extrinsic of camera %d): %d bodies, iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n",
                free_extrinsic_camera, (int)r.rig.n_bodies, sum.iterations, sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
}

// The rig form of global_bundle_adjustment (vsl_global_bundle_adjust_rig): the reference's global_bundle_adjustment
// signature (include/visnav/loop_closure_utils.h:672-748) on ALL observations of the landmarks, with bundle_adjustment_rig's
// body conventions -- body = FrameId, camera 0 is the body frame, a frame with one camera derives its body from it, a body
// is fixed if any of its cameras is in fixed_cameras.  The reduced body system is gathered over co-visible frames only and
// stored dense / band / cyclic band.  All camera poses come back ON the calibration.  One GPU.
inline void global_bundle_adjustment_rig(const Corners& feature_corners, const GlobalBundleAdjustmentOptions& options,
                                         const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                         Landmarks& landmarks) {
  if (&vsl_global_bundle_adjust_rig == nullptr)
    throw std::runtime_error("global_bundle_adjustment_rig: libvslam_hip.so has no vsl_global_bundle_adjust_rig");
  amd::RigFlat r;
  if (!amd::flatten_rig<true>("global_bundle_adjustment_rig", feature_corners, fixed_cameras, calib_cam, cameras, landmarks, r)) return;
  if (!r.any_free) return;
  amd::BaFlat& f = r.f;
  vsl_ba_options opt;
  opt.use_huber = options.use_huber ? 1 : 0;
  opt.huber_parameter = options.huber_parameter;
  opt.max_num_iterations = options.max_num_iterations;
  opt.verbosity = 0;
  vsl_ba_summary sum;
  amd::check(vsl_global_bundle_adjust_rig(amd::ctx(), &f.prob, &r.rig, &opt, &sum), "global_bundle_adjustment_rig");
  for (size_t c = 0; c < f.cam_ptr.size(); c++) std::copy(&f.poses[7 * c], &f.poses[7 * c] + 7, f.cam_ptr[c]->T_w_c.data());
  for (size_t l = 0; l < f.lm_ptr.size(); l++)
    for (int j = 0; j < 3; j++) f.lm_ptr[l]->p.data()[j] = f.points[3 * l + j];
  if (options.verbosity_level >= 1)
    std::printf("vslam_hip rig global BA: %d bodies, iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms\n",
                (int)r.rig.n_bodies, sum.iterations, sum.initial_cost, sum.final_cost, sum.termination, sum.total_ms);
}

// Marginal covariances of the map as it stands (vsl_ba_covariance; the reference has no counterpart, Ceres offers it as
// ceres::Covariance beside the ceres::Solve of map_utils.h:405-411).  Nothing is optimised.  The problem is flattened by
// the same code as bundle_adjustment (inlier observations of the window, Landmark::obs); options: use_huber and
// huber_parameter.  query_cameras must be free cameras of `cameras`, query_landmarks ids of `landmarks` (else
// std::out_of_range).  pose_cov_out: 6 x 6 over the tangent (upsilon, omega) of T_w_c exp(delta); landmark_cov_out:
// 3 x 3 in world coordinates, NaN for a landmark whose own block is singular (a single observation).  Unit: 1 px^2 of
// observation noise.  Returns the number of such landmarks; std::domain_error when the reduced camera system is singular
// to working precision (VSL_ERR_NUMERIC: e.g. no fixed camera).
using PoseCovariance = Eigen::Matrix<double, 6, 6>;
namespace amd {
// what the two covariance wrappers share: the flattening (kAllObs as in run_ba), the id -> index maps, the call, the
// blocks.  kAllObs = false: vsl_ba_covariance on the window's inlier observations; true: vsl_global_ba_covariance on
// all of them.  *storage_out (nullable): the route of the global call (0 dense, 1 linear band).
template <bool kAllObs>
inline int run_ba_covariance(const char* what, const Corners& feature_corners, bool use_huber, double huber_parameter,
                             const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                             Landmarks& landmarks, const std::vector<FrameCamId>& query_cameras,
                             const std::vector<TrackId>& query_landmarks, std::map<FrameCamId, PoseCovariance>& pose_cov_out,
                             std::unordered_map<TrackId, Eigen::Matrix3d>& landmark_cov_out, int* storage_out) {
  pose_cov_out.clear();
  landmark_cov_out.clear();
  if (query_cameras.empty() && query_landmarks.empty()) return 0;
  BaFlat f;
  if (!flatten_ba<kAllObs>(feature_corners, fixed_cameras, calib_cam, cameras, landmarks, f))
    throw std::out_of_range(std::string(what) + ": the map has no observation");
  std::vector<int32_t> cams, lms;
  for (const FrameCamId& id : query_cameras) {
    const auto it = std::lower_bound(f.cam_id.begin(), f.cam_id.end(), id);
    if (it == f.cam_id.end() || !(*it == id)) throw std::out_of_range(std::string(what) + ": unknown camera");
    cams.push_back((int32_t)(it - f.cam_id.begin()));
  }
  if (!query_landmarks.empty()) {
    std::unordered_map<TrackId, int32_t> index;
    for (size_t l = 0; l < f.lm_id.size(); l++) index.emplace(f.lm_id[l], (int32_t)l);
    for (const TrackId id : query_landmarks) lms.push_back(index.at(id));
  }
  vsl_ba_options opt;
  opt.use_huber = use_huber ? 1 : 0;
  opt.huber_parameter = huber_parameter;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  std::vector<double> cp(36 * cams.size()), cl(9 * lms.size());
  int n_degenerate = 0;
  const int rc = kAllObs ? vsl_global_ba_covariance(ctx(), &f.prob, &opt, cams.data(), (int)cams.size(), cp.data(), lms.data(),
                                                    (int)lms.size(), cl.data(), &n_degenerate, storage_out)
                         : vsl_ba_covariance(ctx(), &f.prob, &opt, cams.data(), (int)cams.size(), cp.data(), lms.data(),
                                             (int)lms.size(), cl.data(), &n_degenerate);
  // a reduced camera system that is singular to working precision is a property of the map, not a failure of the call
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(ctx()));
  check(rc, what);
  for (size_t q = 0; q < cams.size(); q++) {
    PoseCovariance& m = pose_cov_out[query_cameras[q]];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) m(i, j) = cp[36 * q + 6 * i + j];
  }
  for (size_t q = 0; q < lms.size(); q++) {
    Eigen::Matrix3d& m = landmark_cov_out[query_landmarks[q]];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) m(i, j) = cl[9 * q + 3 * i + j];
  }
  return n_degenerate;
}
}  // namespace amd

inline int bundle_adjustment_covariance(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                        const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                        Landmarks& landmarks, const std::vector<FrameCamId>& query_cameras,
                                        const std::vector<TrackId>& query_landmarks,
                                        std::map<FrameCamId, PoseCovariance>& pose_cov_out,
                                        std::unordered_map<TrackId, Eigen::Matrix3d>& landmark_cov_out) {
  return amd::run_ba_covariance<false>("bundle_adjustment_covariance", feature_corners, options.use_huber, options.huber_parameter,
                                       fixed_cameras, calib_cam, cameras, landmarks, query_cameras, query_landmarks, pose_cov_out,
                                       landmark_cov_out, nullptr);
}

// include/visnav/loop_closure_utils.h:672-748.  With rccl_world.h included first and VISNAV_AMD_WORLD > 1 (one process
// per GPU, every rank calling this on the same map) the solve is partitioned over the ranks and all-reduced through
// RCCL; otherwise it is the single-GPU solver.
inline void global_bundle_adjustment(const Corners& feature_corners, const GlobalBundleAdjustmentOptions& options,
                                     const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                     Landmarks& landmarks) {
  amd::run_ba<true>(feature_corners, options.use_huber, options.huber_parameter, options.max_num_iterations,
                    options.verbosity_level, fixed_cameras, calib_cam, cameras, landmarks);
}

// global_bundle_adjustment by the matrix-free PCG on the reduced camera system (iterative Schur, include/vslam_hip.h:
// what ceres::ITERATIVE_SCHUR is to SPARSE_SCHUR) -- for maps whose cameras do not order into a narrow band.  Sets the
// context's "ba_iterative_schur" diagnostic for the call and puts it back as it found it, also when the call throws.
// Single GPU: with VISNAV_AMD_WORLD > 1 the call fails (VSL_ERR_INVALID) on every rank alike.
inline void global_bundle_adjustment_iterative(const Corners& feature_corners, const GlobalBundleAdjustmentOptions& options,
                                               const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam,
                                               Cameras& cameras, Landmarks& landmarks) {
  struct Restore {
    int was = 0;
    Restore() {
      amd::check(vsl_ctx_get_diagnostic(amd::ctx(), "ba_iterative_schur", &was), "global_bundle_adjustment_iterative");
      amd::check(vsl_ctx_set_diagnostic(amd::ctx(), "ba_iterative_schur", 1), "global_bundle_adjustment_iterative");
    }
    ~Restore() { (void)vsl_ctx_set_diagnostic(amd::ctx(), "ba_iterative_schur", was); }
  } restore;
  global_bundle_adjustment(feature_corners, options, fixed_cameras, calib_cam, cameras, landmarks);
}

// Marginal covariances of the map that global_bundle_adjustment works on (vsl_global_ba_covariance): the contract of
// bundle_adjustment_covariance above, on ALL observations of the landmarks (the flattening of global_bundle_adjustment),
// with the reduced camera system of a large map kept in band storage.  storage_out (nullable): 0 = the dense route of
// bundle_adjustment_covariance, 1 = linear band.  Single GPU.
inline int global_bundle_adjustment_covariance(const Corners& feature_corners, const GlobalBundleAdjustmentOptions& options,
                                               const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam,
                                               Cameras& cameras, Landmarks& landmarks,
                                               const std::vector<FrameCamId>& query_cameras,
                                               const std::vector<TrackId>& query_landmarks,
                                               std::map<FrameCamId, PoseCovariance>& pose_cov_out,
                                               std::unordered_map<TrackId, Eigen::Matrix3d>& landmark_cov_out,
                                               int* storage_out = nullptr) {
  return amd::run_ba_covariance<true>("global_bundle_adjustment_covariance", feature_corners, options.use_huber,
                                      options.huber_parameter, fixed_cameras, calib_cam, cameras, landmarks, query_cameras,
                                      query_landmarks, pose_cov_out, landmark_cov_out, storage_out);
}

// Covariance and information of the relative poses of camera pairs under the bundle adjustment's posterior
// (vsl_ba_relative_pose_covariance / vsl_global_ba_relative_pose_covariance): the weights of pose-graph edges whose
// measurement is read off the map.  Nothing is optimised.  The problem is flattened by flatten_ba exactly as for
// bundle_adjustment (BundleAdjustmentOptions: inlier observations, the dense route) or global_bundle_adjustment
// (GlobalBundleAdjustmentOptions: all observations, dense or linear band, *storage_out = 0 / 1).  pairs: (a, b) with a
// the pose-graph functor's T_w_c and b its T_w_n; both must be cameras of `cameras` (else std::out_of_range), a != b,
// not both fixed (else std::runtime_error from the call).  out[q]: measurement = log(T_a^-1 T_b) as (upsilon, omega),
// cov = the covariance of the pose-graph residual, info = cov^-1; valid = false (info NaN) where cov is singular to
// working precision.  Returns the number of such pairs; std::domain_error when the reduced camera system is singular
// (no fixed camera).  Each info is a marginal: edges that share a camera are correlated, which per-edge matrices
// cannot express.  The new C symbols are referenced weakly: a build of this header on a C ABI without them links, and
// calling these functions there throws.
struct RelativePoseCovariance {
  double measurement[6];
  PoseCovariance cov, info;
  bool valid = false;
};
namespace amd {
template <bool kAllObs>
inline int run_relative_pose_covariance(const char* what, const Corners& feature_corners, bool use_huber, double huber_parameter,
                                        const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                        Landmarks& landmarks, const std::vector<std::pair<FrameCamId, FrameCamId>>& pairs,
                                        std::vector<RelativePoseCovariance>& out, int* storage_out) {
  out.clear();
  if (kAllObs ? !vsl_global_ba_relative_pose_covariance : !vsl_ba_relative_pose_covariance)
    throw std::runtime_error(std::string(what) + ": this library has no relative-pose covariances");
  BaFlat f;
  if (!flatten_ba<kAllObs>(feature_corners, fixed_cameras, calib_cam, cameras, landmarks, f))
    throw std::out_of_range(std::string(what) + ": the map has no observation");
  std::vector<int32_t> a, b;
  auto index = [&](const FrameCamId& id) {
    const auto it = std::lower_bound(f.cam_id.begin(), f.cam_id.end(), id);
    if (it == f.cam_id.end() || !(*it == id)) throw std::out_of_range(std::string(what) + ": unknown camera");
    return (int32_t)(it - f.cam_id.begin());
  };
  for (const auto& p : pairs) {
    a.push_back(index(p.first));
    b.push_back(index(p.second));
  }
  vsl_ba_options opt;
  opt.use_huber = use_huber ? 1 : 0;
  opt.huber_parameter = huber_parameter;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  const size_t n = pairs.size();
  std::vector<double> meas(6 * n), cov(36 * n), info(36 * n);
  int n_singular = 0;
  const int rc = kAllObs ? vsl_global_ba_relative_pose_covariance(ctx(), &f.prob, &opt, a.data(), b.data(), (int)n, nullptr, meas.data(),
                                                                  cov.data(), info.data(), &n_singular, storage_out)
                         : vsl_ba_relative_pose_covariance(ctx(), &f.prob, &opt, a.data(), b.data(), (int)n, nullptr, meas.data(),
                                                           cov.data(), info.data(), &n_singular);
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(ctx()));
  check(rc, what);
  out.resize(n);
  for (size_t q = 0; q < n; q++) {
    RelativePoseCovariance& r = out[q];
    r.valid = true;
    for (int i = 0; i < 6; i++) {
      r.measurement[i] = meas[6 * q + i];
      for (int j = 0; j < 6; j++) {
        r.cov(i, j) = cov[36 * q + 6 * i + j];
        r.info(i, j) = info[36 * q + 6 * i + j];
        if (!(r.info(i, j) == r.info(i, j))) r.valid = false;  // NaN: the singular pair
      }
    }
  }
  return n_singular;
}
}  // namespace amd

inline int relative_pose_covariance(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                    const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                    Landmarks& landmarks, const std::vector<std::pair<FrameCamId, FrameCamId>>& pairs,
                                    std::vector<RelativePoseCovariance>& out) {
  return amd::run_relative_pose_covariance<false>("relative_pose_covariance", feature_corners, options.use_huber,
                                                  options.huber_parameter, fixed_cameras, calib_cam, cameras, landmarks, pairs, out,
                                                  nullptr);
}
inline int relative_pose_covariance(const Corners& feature_corners, const GlobalBundleAdjustmentOptions& options,
                                    const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                    Landmarks& landmarks, const std::vector<std::pair<FrameCamId, FrameCamId>>& pairs,
                                    std::vector<RelativePoseCovariance>& out, int* storage_out = nullptr) {
  return amd::run_relative_pose_covariance<true>("relative_pose_covariance (global)", feature_corners, options.use_huber,
                                                 options.huber_parameter, fixed_cameras, calib_cam, cameras, landmarks, pairs, out,
                                                 storage_out);
}

// Covariances of the RIG posterior (vsl_ba_rig_covariance / vsl_ba_rig_relative_pose_covariance): what
// bundle_adjustment_covariance and relative_pose_covariance are to bundle_adjustment, for a map adjusted by
// bundle_adjustment_rig.  The rules and the flattening are bundle_adjustment_rig's (amd::flatten_rig): bodies are the
// FrameIds, the body frame is camera 0, a body is fixed if any of its cameras is in fixed_cameras.  Nothing is
// optimised and nothing is written to the map; the body poses are derived from `cameras` as they stand.
// query_frames: free frames of `cameras`; query_cameras: cameras of free frames; query_landmarks: ids of `landmarks`
// (else std::out_of_range; a fixed frame or a camera of one: std::invalid_argument).  body_cov_out: 6 x 6 over the tangent
// (upsilon, omega) of T_w_b exp(delta); cam_cov_out: the same for the camera's own right perturbation, comparable with
// bundle_adjustment_covariance; landmark_cov_out: 3 x 3, NaN for a landmark whose own block is singular.  Returns the
// number of such landmarks; std::domain_error when the reduced body system is singular to working precision or no frame
// is fixed (VSL_ERR_NUMERIC).
inline int bundle_adjustment_rig_covariance(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                            const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                            Landmarks& landmarks, const std::vector<FrameId>& query_frames,
                                            const std::vector<FrameCamId>& query_cameras, const std::vector<TrackId>& query_landmarks,
                                            std::map<FrameId, PoseCovariance>& body_cov_out,
                                            std::map<FrameCamId, PoseCovariance>& cam_cov_out,
                                            std::unordered_map<TrackId, Eigen::Matrix3d>& landmark_cov_out) {
  const char* what = "bundle_adjustment_rig_covariance";
  body_cov_out.clear();
  cam_cov_out.clear();
  landmark_cov_out.clear();
  if (&vsl_ba_rig_covariance == nullptr) throw std::runtime_error(std::string(what) + ": this library has no rig covariances");
  if (query_frames.empty() && query_cameras.empty() && query_landmarks.empty()) return 0;
  amd::RigFlat r;
  if (!amd::flatten_rig(what, feature_corners, fixed_cameras, calib_cam, cameras, landmarks, r))
    throw std::out_of_range(std::string(what) + ": the map has no observation");
  const amd::BaFlat& f = r.f;
  std::vector<int32_t> bodies, cams, lms;
  for (const FrameId id : query_frames) {
    bodies.push_back(r.body_of(id));
    if (bodies.back() < 0) throw std::out_of_range(std::string(what) + ": unknown frame");
    if (r.body_fixed[bodies.back()]) throw std::invalid_argument(std::string(what) + ": a queried frame is fixed");
  }
  for (const FrameCamId& id : query_cameras) {
    const auto it = std::lower_bound(f.cam_id.begin(), f.cam_id.end(), id);
    if (it == f.cam_id.end() || !(*it == id)) throw std::out_of_range(std::string(what) + ": unknown camera");
    cams.push_back((int32_t)(it - f.cam_id.begin()));
    if (r.body_fixed[r.cam_body[cams.back()]]) throw std::invalid_argument(std::string(what) + ": a queried camera's frame is fixed");
  }
  if (!query_landmarks.empty()) {
    std::unordered_map<TrackId, int32_t> index;
    for (size_t l = 0; l < f.lm_id.size(); l++) index.emplace(f.lm_id[l], (int32_t)l);
    for (const TrackId id : query_landmarks) lms.push_back(index.at(id));
  }
  vsl_ba_options opt;
  opt.use_huber = options.use_huber ? 1 : 0;
  opt.huber_parameter = options.huber_parameter;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  std::vector<double> cb(36 * bodies.size()), cc(36 * cams.size()), cl(9 * lms.size());
  int n_degenerate = 0;
  const int rc = vsl_ba_rig_covariance(amd::ctx(), &f.prob, &r.rig, &opt, bodies.data(), (int)bodies.size(), cb.data(), cams.data(),
                                       (int)cams.size(), cc.data(), lms.data(), (int)lms.size(), cl.data(), &n_degenerate);
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(amd::ctx()));
  amd::check(rc, what);
  auto block = [](const std::vector<double>& v, size_t q, PoseCovariance& m) {
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) m(i, j) = v[36 * q + 6 * i + j];
  };
  for (size_t q = 0; q < bodies.size(); q++) block(cb, q, body_cov_out[query_frames[q]]);
  for (size_t q = 0; q < cams.size(); q++) block(cc, q, cam_cov_out[query_cameras[q]]);
  for (size_t q = 0; q < lms.size(); q++) {
    Eigen::Matrix3d& m = landmark_cov_out[query_landmarks[q]];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) m(i, j) = cl[9 * q + 3 * i + j];
  }
  return n_degenerate;
}

// Covariances of the posterior bundle_adjustment_rig_extrinsics adjusts (vsl_ba_rig_ext_covariance): how well the window
// determines the extrinsic of free_extrinsic_camera (0 or 1), and the frame / camera / landmark blocks with that
// extrinsic NOT taken as known.  Flattening and rules are bundle_adjustment_rig_extrinsics' (amd::flatten_rig); nothing is
// optimised, nothing is written to the map.  query_frames: free frames; query_cameras: any camera but one of a fixed frame
// whose extrinsic is held; query_landmarks: ids of `landmarks` (unknown id: std::out_of_range; a rule broken:
// std::invalid_argument).  extrinsic_cov: 6 x 6 over the tangent (upsilon, omega) of T_b_c * exp(eps), T_b_c =
// T_i_c[0]^-1 T_i_c[camera] at the calibration handed in.  A window that does not determine the extrinsic -- one fixed
// frame: the baseline's length is a gauge direction; no fixed frame -- is EXPECTED input: observable = false, `reason`
// says why, every map is empty, nothing is thrown.
struct RigExtrinsicsCovariance {
  bool observable = false;
  std::string reason;
  PoseCovariance extrinsic_cov;
  std::map<FrameId, PoseCovariance> body_cov;
  std::map<FrameId, PoseCovariance> body_extrinsic_cov;  // [S^-1] at (frame, extrinsic): rows the frame's tangent
  std::map<FrameCamId, PoseCovariance> cam_cov;
  std::unordered_map<TrackId, Eigen::Matrix3d> landmark_cov;  // NaN for a landmark whose own block is singular
  int n_degenerate = 0;
};
inline RigExtrinsicsCovariance bundle_adjustment_rig_extrinsics_covariance(
    const Corners& feature_corners, const BundleAdjustmentOptions& options, const std::set<FrameCamId>& fixed_cameras,
    Calibration& calib_cam, Cameras& cameras, Landmarks& landmarks, int free_extrinsic_camera,
    const std::vector<FrameId>& query_frames, const std::vector<FrameCamId>& query_cameras,
    const std::vector<TrackId>& query_landmarks) {
  const char* what = "bundle_adjustment_rig_extrinsics_covariance";
  RigExtrinsicsCovariance out;
  if (&vsl_ba_rig_ext_covariance == nullptr) throw std::runtime_error(std::string(what) + ": this library has no vsl_ba_rig_ext_covariance");
  if (options.optimize_intrinsics) throw std::invalid_argument(std::string(what) + ": optimize_intrinsics is not offered in rig form");
  if (free_extrinsic_camera != 0 && free_extrinsic_camera != 1) throw std::invalid_argument(std::string(what) + ": free_extrinsic_camera is 0 or 1");
  amd::RigFlat r;
  if (!amd::flatten_rig(what, feature_corners, fixed_cameras, calib_cam, cameras, landmarks, r))
    throw std::out_of_range(std::string(what) + ": the map has no observation");
  const amd::BaFlat& f = r.f;
  std::vector<int32_t> bodies, cams, lms;
  for (const FrameId id : query_frames) {
    bodies.push_back(r.body_of(id));
    if (bodies.back() < 0) throw std::out_of_range(std::string(what) + ": unknown frame");
    if (r.body_fixed[bodies.back()]) throw std::invalid_argument(std::string(what) + ": a queried frame is fixed");
  }
  for (const FrameCamId& id : query_cameras) {
    const auto it = std::lower_bound(f.cam_id.begin(), f.cam_id.end(), id);
    if (it == f.cam_id.end() || !(*it == id)) throw std::out_of_range(std::string(what) + ": unknown camera");
    cams.push_back((int32_t)(it - f.cam_id.begin()));
    if (r.body_fixed[r.cam_body[cams.back()]] && (int)id.cam_id != free_extrinsic_camera)
      throw std::invalid_argument(std::string(what) + ": a queried camera's frame is fixed and its extrinsic is held");
  }
  if (!query_landmarks.empty()) {
    std::unordered_map<TrackId, int32_t> index;
    for (size_t l = 0; l < f.lm_id.size(); l++) index.emplace(f.lm_id[l], (int32_t)l);
    for (const TrackId id : query_landmarks) lms.push_back(index.at(id));
  }
  vsl_ba_options opt;
  opt.use_huber = options.use_huber ? 1 : 0;
  opt.huber_parameter = options.huber_parameter;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  const uint8_t ext_free[2] = {(uint8_t)(free_extrinsic_camera == 0), (uint8_t)(free_extrinsic_camera == 1)};
  std::vector<double> cb(36 * bodies.size()), cc(36 * cams.size()), cl(9 * lms.size()), ce(36), cx(36 * bodies.size());
  const int rc = vsl_ba_rig_ext_covariance(amd::ctx(), &f.prob, &r.rig, ext_free, r.T_b_c, &opt, bodies.data(), (int)bodies.size(),
                                           cb.data(), cams.data(), (int)cams.size(), cc.data(), lms.data(), (int)lms.size(), cl.data(),
                                           ce.data(), cx.data(), &out.n_degenerate);
  if (rc == VSL_ERR_NUMERIC) {  // a gauge window: an answer, not a failure
    out.reason = vsl_last_error(amd::ctx());
    return out;
  }
  amd::check(rc, what);
  out.observable = true;
  auto block = [](const std::vector<double>& v, size_t q, PoseCovariance& m) {
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) m(i, j) = v[36 * q + 6 * i + j];
  };
  block(ce, 0, out.extrinsic_cov);
  for (size_t q = 0; q < bodies.size(); q++) {
    block(cb, q, out.body_cov[query_frames[q]]);
    block(cx, q, out.body_extrinsic_cov[query_frames[q]]);
  }
  for (size_t q = 0; q < cams.size(); q++) block(cc, q, out.cam_cov[query_cameras[q]]);
  for (size_t q = 0; q < lms.size(); q++) {
    Eigen::Matrix3d& m = out.landmark_cov[query_landmarks[q]];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) m(i, j) = cl[9 * q + 3 * i + j];
  }
  return out;
}

// relative_pose_covariance for pairs of FRAMES (bodies) of the rig posterior: out[q] as there, measurement =
// log(T_a^-1 T_b) of the body poses.  Both frames must be frames of `cameras` (else std::out_of_range), a != b, not both
// fixed (else std::invalid_argument).  Returns the number of singular pairs.
inline int rig_relative_pose_covariance(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                        const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                        Landmarks& landmarks, const std::vector<std::pair<FrameId, FrameId>>& pairs,
                                        std::vector<RelativePoseCovariance>& out) {
  const char* what = "rig_relative_pose_covariance";
  out.clear();
  if (&vsl_ba_rig_relative_pose_covariance == nullptr) throw std::runtime_error(std::string(what) + ": this library has no rig covariances");
  amd::RigFlat r;
  if (!amd::flatten_rig(what, feature_corners, fixed_cameras, calib_cam, cameras, landmarks, r))
    throw std::out_of_range(std::string(what) + ": the map has no observation");
  std::vector<int32_t> a, b;
  for (const auto& p : pairs) {
    a.push_back(r.body_of(p.first));
    b.push_back(r.body_of(p.second));
    if (a.back() < 0 || b.back() < 0) throw std::out_of_range(std::string(what) + ": unknown frame");
    if (a.back() == b.back() || (r.body_fixed[a.back()] && r.body_fixed[b.back()]))
      throw std::invalid_argument(std::string(what) + ": a pair names one frame twice or two fixed frames");
  }
  vsl_ba_options opt;
  opt.use_huber = options.use_huber ? 1 : 0;
  opt.huber_parameter = options.huber_parameter;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  const size_t n = pairs.size();
  std::vector<double> meas(6 * n), cov(36 * n), info(36 * n);
  int n_singular = 0;
  const int rc = vsl_ba_rig_relative_pose_covariance(amd::ctx(), &r.f.prob, &r.rig, &opt, a.data(), b.data(), (int)n, nullptr, meas.data(),
                                                     cov.data(), info.data(), &n_singular);
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(amd::ctx()));
  amd::check(rc, what);
  out.resize(n);
  for (size_t q = 0; q < n; q++) {
    RelativePoseCovariance& o = out[q];
    o.valid = true;
    for (int i = 0; i < 6; i++) {
      o.measurement[i] = meas[6 * q + i];
      for (int j = 0; j < 6; j++) {
        o.cov(i, j) = cov[36 * q + 6 * i + j];
        o.info(i, j) = info[36 * q + 6 * i + j];
        if (!(o.info(i, j) == o.info(i, j))) o.valid = false;  // NaN: the singular pair
      }
    }
  }
  return n_singular;
}

// The rig counterpart of map_edge_information (loop_closure.h): edge_meas / edge_info of pose-graph edges between
// keyframes (FrameIds: the graph's nodes are bodies) from a map adjusted in rig form.  The pairs whose two frames are in
// `cameras`, differ and are not both fixed are queried in ONE call of rig_relative_pose_covariance; every other pair and
// every singular pair keeps from_map = false, a zero measurement and default_information.
struct RigEdgeInformation {
  std::vector<std::array<double, 6>> edge_meas;  // log(T_a^-1 T_b) of the bodies, (upsilon, omega)
  std::vector<PoseCovariance> edge_info;
  std::vector<bool> from_map;
  size_t n_map_edges = 0;
};
inline RigEdgeInformation rig_map_edge_information(const Corners& feature_corners, const BundleAdjustmentOptions& options,
                                                   const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam,
                                                   Cameras& cameras, Landmarks& landmarks,
                                                   const std::vector<std::pair<FrameId, FrameId>>& edges,
                                                   const PoseCovariance& default_information) {
  RigEdgeInformation e;
  e.edge_meas.assign(edges.size(), std::array<double, 6>{{0, 0, 0, 0, 0, 0}});
  e.edge_info.assign(edges.size(), default_information);
  e.from_map.assign(edges.size(), false);
  std::set<FrameId> frames, fixed;
  for (const auto& kv : cameras) frames.insert(kv.first.frame_id);
  for (const FrameCamId& id : fixed_cameras) fixed.insert(id.frame_id);
  std::vector<std::pair<FrameId, FrameId>> pairs;
  std::vector<size_t> edge_of;
  for (size_t q = 0; q < edges.size(); q++) {
    const FrameId a = edges[q].first, b = edges[q].second;
    if (a == b || !frames.count(a) || !frames.count(b) || (fixed.count(a) && fixed.count(b))) continue;
    pairs.push_back(edges[q]);
    edge_of.push_back(q);
  }
  if (pairs.empty()) return e;
  std::vector<RelativePoseCovariance> out;
  rig_relative_pose_covariance(feature_corners, options, fixed_cameras, calib_cam, cameras, landmarks, pairs, out);
  for (size_t k = 0; k < pairs.size(); k++) {
    if (!out[k].valid) continue;
    const size_t q = edge_of[k];
    for (int i = 0; i < 6; i++) e.edge_meas[q][i] = out[k].measurement[i];
    e.edge_info[q] = out[k].info;
    e.from_map[q] = true;
    e.n_map_edges++;
  }
  return e;
}

}  // namespace visnav
