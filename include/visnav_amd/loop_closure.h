// visnav_amd/loop_closure.h -- drop-ins for the two pieces of include/visnav/loop_closure_utils.h that SURVEY.md
// 8(f) ranks next after the per-frame path:
//   construct_visibility_graph (:52-96)   host graph bookkeeping, restated as is (it is a counting loop over the
//                                          landmarks' observation lists; no device work)
//   pose_graph_optimization    (:446-587)  the edge selection is the reference's (spanning-tree edges, covisibility
//                                          edges above the essential threshold, the loop constraint), the
//                                          optimisation itself runs on the MI355X (vsl_pose_graph_optimize)
// Same names, arguments and in-place update convention as the reference.  pose_graph_covariance (no counterpart in the
// reference) returns the marginal covariances of that graph's keyframes (vsl_pgo_covariance).
// Round 2 adds the loop DETECTION half (host graph / inverted-file bookkeeping restated; the BoW scores of the
// surviving candidates go to the GPU in one batched launch, ORBVocabularyAmd::score_batch):
//   compute_min_connected_covisible (:109-126), detect_loop_candidates (:141-263), insert_new_kf_to_db (:269-276),
//   detect_loop_closure (:294-388), loop_align (:398-416), update_stereo_pair (:593-601),
//   update_landmark_position (:607-621), loop_closure (:633-648)
// landmark_fusion (:417-427) is declared and left empty upstream; the six-argument form stays that no-op, and an overload
// does the work: one batched guided search on the device (vsl_fuse_search), then the map edits of fusion_plan.h.
#pragma once
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include <unordered_map>

#include "bow.h"
#include "bundle_adjustment.h"
#include "fusion_plan.h"

// The weighted pose-graph entry points (the EdgeInformation overloads below) are referenced weakly, like the optional
// entry points of bow.h: a build of the same headers on a C ABI without them links, and asking for weights there throws.
#pragma weak vsl_pose_graph_optimize_w
#pragma weak vsl_pgo_covariance_w
#pragma weak vsl_pgo_joint_covariance_w
#pragma weak vsl_pgo_edge_consistency_w
// ... and so are the read-out and the parity hook of the far-edge route (pose_graph_optimization_far_edges below)
#pragma weak vsl_ctx_last_pgo_far
#pragma weak vsl_pgo_far_solve

namespace visnav {

// loop_closure_utils.h:430-436
struct LoopClosureOptions {
  int verbosity_level = 1;
  bool set_current_kf_fixed = true;
};

namespace amd {
// rigid-transform helpers on the Sophus::SE3d storage order (qx qy qz qw tx ty tz) -- only what the edge
// assembly needs when the real Sophus headers are not available
struct Rt {
  double q[4], t[3];
};
inline Rt rt_of(const Sophus::SE3d& T) {
  Rt r;
  const double* d = T.data();
  for (int i = 0; i < 4; i++) r.q[i] = d[i];
  for (int i = 0; i < 3; i++) r.t[i] = d[4 + i];
  return r;
}
inline void qrot(const double* q, const double* p, double* o) {
  double uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int i = 0; i < 3; i++) uv[i] += uv[i];
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) o[i] = p[i] + q[3] * uv[i] + c[i];
}
inline Rt rt_inv(const Rt& a) {
  Rt r;
  r.q[0] = -a.q[0];
  r.q[1] = -a.q[1];
  r.q[2] = -a.q[2];
  r.q[3] = a.q[3];
  double m[3] = {-a.t[0], -a.t[1], -a.t[2]};
  qrot(r.q, m, r.t);
  return r;
}
inline Rt rt_mul(const Rt& a, const Rt& b) {
  Rt r;
  r.q[0] = a.q[3] * b.q[0] + a.q[0] * b.q[3] + a.q[1] * b.q[2] - a.q[2] * b.q[1];
  r.q[1] = a.q[3] * b.q[1] - a.q[0] * b.q[2] + a.q[1] * b.q[3] + a.q[2] * b.q[0];
  r.q[2] = a.q[3] * b.q[2] + a.q[0] * b.q[1] - a.q[1] * b.q[0] + a.q[2] * b.q[3];
  r.q[3] = a.q[3] * b.q[3] - a.q[0] * b.q[0] - a.q[1] * b.q[1] - a.q[2] * b.q[2];
  double rb[3];
  qrot(a.q, b.t, rb);
  for (int i = 0; i < 3; i++) r.t[i] = rb[i] + a.t[i];
  return r;
}
inline Sophus::SE3d se3_of(const Rt& a) {
  Sophus::SE3d T;
  double* d = T.data();
  const double n = std::sqrt(a.q[0] * a.q[0] + a.q[1] * a.q[1] + a.q[2] * a.q[2] + a.q[3] * a.q[3]);
  for (int i = 0; i < 4; i++) d[i] = a.q[i] / n;
  for (int i = 0; i < 3; i++) d[4 + i] = a.t[i];
  return T;
}
// Sophus::SE3::log: (upsilon, omega)
inline void rt_log(const Rt& a, double* out) {
  const double* q = a.q;
  const double sq_n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2], w = q[3];
  double two_atan, c = 1.0 / 12.0;
  if (sq_n < 1e-20) {
    two_atan = 2.0 / w - 2.0 / 3.0 * sq_n / (w * w * w);
  } else {
    const double n = std::sqrt(sq_n);
    const double half = w < 0 ? std::atan2(-n, -w) : std::atan2(n, w);
    two_atan = 2.0 * half / n;
    const double theta = two_atan * n;
    if (std::fabs(theta) >= 1e-6) c = (1.0 - theta * std::cos(0.5 * theta) / (2.0 * std::sin(0.5 * theta))) / (theta * theta);
  }
  const double om[3] = {two_atan * q[0], two_atan * q[1], two_atan * q[2]};
  const double* t = a.t;
  const double x[3] = {om[1] * t[2] - om[2] * t[1], om[2] * t[0] - om[0] * t[2], om[0] * t[1] - om[1] * t[0]};
  const double y[3] = {om[1] * x[2] - om[2] * x[1], om[2] * x[0] - om[0] * x[2], om[0] * x[1] - om[1] * x[0]};
  for (int i = 0; i < 3; i++) {
    out[i] = t[i] - 0.5 * x[i] + c * y[i];
    out[3 + i] = om[i];
  }
}
}  // namespace amd

// loop_closure_utils.h:52-96
inline void construct_visibility_graph(const FrameCamId& new_fcid, const Cameras& cameras, const Landmarks& landmarks,
                                       Camera& new_camera, CovisibilityGraph& graph, int threshold) {
  std::map<FrameCamId, int> share_lm_count;
  for (const auto& tid_lm : landmarks) {
    const Landmark& lm = tid_lm.second;
    const auto it = lm.all_obs.find(new_fcid);
    if (it == lm.all_obs.end()) continue;
    new_camera.map_points.emplace(tid_lm.first, it->second);
    for (const auto& ob : lm.all_obs)  // every camera that also observes this landmark (and is in `cameras`)
      if (cameras.count(ob.first)) share_lm_count[ob.first] += 1;
  }
  std::set<FrameCamId> new_edges;
  const amd::Rt T_c_w = amd::rt_inv(amd::rt_of(new_camera.T_w_c));
  for (const auto& fcid_count : share_lm_count) {
    if (fcid_count.first.cam_id != 0 || fcid_count.second < threshold) continue;
    new_camera.covisible_weights.emplace(fcid_count.first, fcid_count.second);
    new_camera.covisible_rel_poses.emplace(fcid_count.first,
                                           amd::se3_of(amd::rt_mul(T_c_w, amd::rt_of(cameras.at(fcid_count.first).T_w_c))));
    new_edges.insert(fcid_count.first);
    graph[fcid_count.first].insert(new_fcid);
  }
  graph[new_fcid] = new_edges;
}

namespace amd {
// The pose graph of loop_closure_utils.h:446-587 as the flat arrays of vsl_pgo_problem: what pose_graph_optimization and
// pose_graph_covariance both start from.  Node 0 = the current keyframe (not part of `keyframes`: the reference adds it
// as its own block), further nodes in the order the edges touch them; edges: per keyframe along the spanning tree from
// the current one, its tree edge (unless the covisibility loop adds it anyway) and its covisibility edges above the
// essential threshold, and the Sim(3) loop constraint.
struct PgoFlat {
  std::vector<Camera*> node_cam;
  std::map<FrameCamId, int> node_of;  // keyframes only: the current keyframe is node 0
  std::vector<int32_t> ea, eb;
  std::vector<double> meas, poses;
  std::vector<uint8_t> fixed;
  std::vector<double> info;  // [n_edges][36] when an EdgeInformation was given, else empty
  vsl_pgo_problem prob;
  const double* edge_info() const { return info.empty() ? nullptr : info.data(); }  // what the _w entry points take
};
}  // namespace amd
// Information matrix (6 x 6 over (upsilon, omega), the inverse covariance of the edge's measurement) of the pose-graph
// edge between keyframes a (the functor's T_w_c) and b (T_w_n); an empty function: every edge has identity weight and
// the calls below ARE the unweighted ones.
using EdgeInformation = std::function<PoseCovariance(const FrameCamId& a, const FrameCamId& b)>;
namespace amd {
inline void flatten_pose_graph(Camera& cur_kf, const FrameCamId& loop_candidate_fcid, const Sophus::SE3d& sim3, Cameras& keyframes,
                               int essential_threshold, const LoopClosureOptions& options, PgoFlat& f) {
  f.node_cam.assign(1, &cur_kf);
  auto node = [&](const FrameCamId& id) {
    auto it = f.node_of.find(id);
    if (it != f.node_of.end()) return it->second;
    f.node_cam.push_back(&keyframes.at(id));  // .at(): std::out_of_range like the reference
    f.node_of.emplace(id, (int)f.node_cam.size() - 1);
    return (int)f.node_cam.size() - 1;
  };
  auto add_edge = [&](int a, int b, const Rt& rel) {
    double l[6];
    rt_log(rel, l);
    f.ea.push_back(a);
    f.eb.push_back(b);
    f.meas.insert(f.meas.end(), l, l + 6);
  };
  auto tree_and_covisibility_edges = [&](int a, const Camera& K) {
    const bool strong = K.covisible_weights.count(K.last_fcid) && K.covisible_weights.at(K.last_fcid) > essential_threshold;
    if (!strong && K.last_fcid.frame_id != -1)  // the spanning-tree edge, unless the covisibility loop adds it anyway
      add_edge(a, node(K.last_fcid), rt_mul(rt_inv(rt_of(K.T_w_c)), rt_of(keyframes.at(K.last_fcid).T_w_c)));
    for (const auto& kv : K.covisible_weights)
      if (kv.second > essential_threshold) add_edge(a, node(kv.first), rt_of(K.covisible_rel_poses.at(kv.first)));
  };
  tree_and_covisibility_edges(0, cur_kf);
  add_edge(0, node(loop_candidate_fcid), rt_inv(rt_of(sim3)));  // the Sim(3) constraint (:514-521)
  for (FrameCamId id = cur_kf.last_fcid; id.frame_id != -1; id = keyframes.at(id).last_fcid) tree_and_covisibility_edges(node(id), keyframes.at(id));

  const int N = (int)f.node_cam.size();
  f.poses.resize(7 * (size_t)N);
  f.fixed.assign(N, 0);
  for (int i = 0; i < N; i++)
    for (int c = 0; c < 7; c++) f.poses[7 * (size_t)i + c] = f.node_cam[i]->T_w_c.data()[c];
  f.fixed[0] = options.set_current_kf_fixed ? 1 : 0;
  f.prob.n_nodes = N;
  f.prob.n_edges = (int32_t)f.ea.size();
  f.prob.poses = f.poses.data();
  f.prob.node_fixed = f.fixed.data();
  f.prob.edge_a = f.ea.data();
  f.prob.edge_b = f.eb.data();
  f.prob.edge_meas = f.meas.data();
}
// ... with the edges' information matrices: cur_kf_fcid names node 0 for the callback
inline void flatten_pose_graph(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                               const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                               const LoopClosureOptions& options, const EdgeInformation& information, PgoFlat& f) {
  flatten_pose_graph(cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, f);
  f.info.clear();
  if (!information) return;
  if (!vsl_pose_graph_optimize_w) throw std::runtime_error("pose graph: this library has no per-edge information matrices");
  std::vector<FrameCamId> id_of(f.node_cam.size(), cur_kf_fcid);
  for (const auto& kv : f.node_of) id_of[kv.second] = kv.first;
  f.info.resize(36 * f.ea.size());
  for (size_t e = 0; e < f.ea.size(); e++) {
    const PoseCovariance W = information(id_of[f.ea[e]], id_of[f.eb[e]]);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) f.info[36 * e + 6 * i + j] = W(i, j);
  }
}
}  // namespace amd

// loop_closure_utils.h:446-587.  cur_kf is not part of `keyframes` (the reference adds it as its own block).
// The overload with `information` weights every edge (vsl_pose_graph_optimize_w): a loop edge gated with Sigma_m by
// loop_candidate_consistency enters the solve with Omega = Sigma_m^-1.  std::invalid_argument when a matrix is not
// positive definite; no pose is written then.
inline void pose_graph_optimization(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                    const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                    const LoopClosureOptions& options, const EdgeInformation& information) {
  amd::PgoFlat f;
  amd::flatten_pose_graph(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, information, f);
  const int N = f.prob.n_nodes;
  vsl_ba_options opt;
  opt.use_huber = 1;
  opt.huber_parameter = 1.0;
  opt.max_num_iterations = 20;
  opt.verbosity = 0;
  vsl_ba_summary sum;
  const int rc = f.edge_info() ? vsl_pose_graph_optimize_w(amd::ctx(), &f.prob, f.edge_info(), &opt, &sum)
                               : vsl_pose_graph_optimize(amd::ctx(), &f.prob, &opt, &sum);
  if (rc == VSL_ERR_INVALID && f.edge_info()) throw std::invalid_argument(vsl_last_error(amd::ctx()));
  amd::check(rc, "pose_graph_optimization");
  for (int i = 0; i < N; i++)
    for (int c = 0; c < 7; c++) f.node_cam[i]->T_w_c.data()[c] = f.poses[7 * (size_t)i + c];
  if (options.verbosity_level >= 1)  // stands in for summary.BriefReport() (:585)
    std::printf("vslam_hip PGO: %d nodes, %d edges, iterations %d, initial cost %.6e, final cost %.6e, termination %d\n", N,
                f.prob.n_edges, sum.iterations, sum.initial_cost, sum.final_cost, sum.termination);
}
inline void pose_graph_optimization(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                    const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                    const LoopClosureOptions& options) {
  pose_graph_optimization(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, EdgeInformation());
}

// pose_graph_optimization for graphs with MORE THAN ONE long edge (a second loop closure, a revisit, a second session):
// the normal equations as a band factor of the near edges plus a low-rank update for the far ones instead of a dense
// matrix (include/vslam_hip.h "FAR EDGES").  Sets the context's "pgo_far_edges" diagnostic for the
// call and puts it back as it found it, also when the call throws.  A graph that takes the band or the ring today, or
// has no admissible split, is solved exactly as by pose_graph_optimization.  report (nullable): what
// vsl_ctx_last_pgo_far says after the solve (all zero on a library without it: the symbol is referenced weakly).
struct PoseGraphFarEdges {
  int taken = 0, far_edges = 0, half_bandwidth = 0, columns = 0;
  int64_t solves = 0;
};
inline void pose_graph_optimization_far_edges(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                              const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                              const LoopClosureOptions& options, const EdgeInformation& information = EdgeInformation(),
                                              PoseGraphFarEdges* report = nullptr) {
  struct Restore {
    int was = 0;
    Restore() {
      amd::check(vsl_ctx_get_diagnostic(amd::ctx(), "pgo_far_edges", &was), "pose_graph_optimization_far_edges");
      amd::check(vsl_ctx_set_diagnostic(amd::ctx(), "pgo_far_edges", 1), "pose_graph_optimization_far_edges");
    }
    ~Restore() { (void)vsl_ctx_set_diagnostic(amd::ctx(), "pgo_far_edges", was); }
  } restore;
  pose_graph_optimization(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, information);
  if (report) {
    *report = PoseGraphFarEdges();
    if (vsl_ctx_last_pgo_far)
      amd::check(vsl_ctx_last_pgo_far(amd::ctx(), &report->taken, &report->far_edges, &report->half_bandwidth, &report->columns,
                                      &report->solves),
                 "pose_graph_optimization_far_edges");
  }
}

// The EdgeInformation of that pose graph from the bundle-adjusted map: the edges amd::flatten_pose_graph creates for
// this current keyframe and loop candidate are enumerated, and those whose measurement is a relative pose of the map --
// spanning-tree and covisibility edges between two cameras of the bundle-adjustment problem, not both fixed -- are
// queried in ONE call of relative_pose_covariance (the global overload: all observations, dense or band).  The returned
// callable answers those edges with Omega = the inverse covariance of the relative pose under the BA posterior, and every
// other edge with default_information: the Sim(3) loop edge (current keyframe -> loop candidate: its measurement does
// not come from the map), a pair that is not in the BA problem with both cameras or has both of them fixed, and a pair
// whose covariance is singular.  *n_map_edges (nullable): the edges answered from the map.
namespace amd {
// the distinct (a, b) of the graph's edges that the map can answer, in edge order
inline std::vector<std::pair<FrameCamId, FrameCamId>> map_edge_pairs(const FrameCamId& cur_kf_fcid, Camera& cur_kf,
                                                                      const FrameCamId& loop_candidate_fcid, const Sophus::SE3d& sim3,
                                                                      Cameras& keyframes, int essential_threshold,
                                                                      const LoopClosureOptions& options,
                                                                      const std::set<FrameCamId>& fixed_cameras, const Cameras& cameras) {
  PgoFlat f;
  flatten_pose_graph(cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, f);
  std::vector<FrameCamId> id_of(f.node_cam.size(), cur_kf_fcid);
  for (const auto& kv : f.node_of) id_of[kv.second] = kv.first;
  std::vector<std::pair<FrameCamId, FrameCamId>> pairs;
  std::set<std::pair<FrameCamId, FrameCamId>> seen;
  for (size_t e = 0; e < f.ea.size(); e++) {
    const FrameCamId &a = id_of[f.ea[e]], &b = id_of[f.eb[e]];
    if (a == b || (a == cur_kf_fcid && b == loop_candidate_fcid)) continue;
    if (!cameras.count(a) || !cameras.count(b) || (fixed_cameras.count(a) && fixed_cameras.count(b))) continue;
    if (seen.insert(std::make_pair(a, b)).second) pairs.emplace_back(a, b);
  }
  return pairs;
}
}  // namespace amd
inline EdgeInformation map_edge_information(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                            const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                            const LoopClosureOptions& options, const Corners& feature_corners,
                                            const GlobalBundleAdjustmentOptions& ba_options,
                                            const std::set<FrameCamId>& fixed_cameras, Calibration& calib_cam, Cameras& cameras,
                                            Landmarks& landmarks, const PoseCovariance& default_information,
                                            size_t* n_map_edges = nullptr, int* storage_out = nullptr) {
  const std::vector<std::pair<FrameCamId, FrameCamId>> pairs = amd::map_edge_pairs(
      cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, fixed_cameras, cameras);
  auto table = std::make_shared<std::map<std::pair<FrameCamId, FrameCamId>, PoseCovariance>>();
  if (!pairs.empty()) {
    std::vector<RelativePoseCovariance> out;
    relative_pose_covariance(feature_corners, ba_options, fixed_cameras, calib_cam, cameras, landmarks, pairs, out, storage_out);
    for (size_t q = 0; q < pairs.size(); q++)
      if (out[q].valid) table->emplace(pairs[q], out[q].info);
  }
  if (n_map_edges) *n_map_edges = table->size();
  return [table, default_information](const FrameCamId& a, const FrameCamId& b) {
    const auto it = table->find(std::make_pair(a, b));
    return it == table->end() ? default_information : it->second;
  };
}

// Marginal covariances of the keyframes of that pose graph as it stands (vsl_pgo_covariance; the reference has no
// counterpart -- g2o and gtsam offer marginals, Ceres ceres::Covariance): what a caller gates the next loop candidate
// with after a closure.  Same arguments as pose_graph_optimization and the same graph (amd::flatten_pose_graph, HuberLoss
// 1.0); nothing is optimised, no pose is written.  query: keyframes of the graph -- cur_kf_fcid for the current one,
// which must then be free (options.set_current_kf_fixed = false); a keyframe the graph does not reach is
// std::out_of_range.  cov_out: 6 x 6 over the tangent (upsilon, omega) of T_w_c exp(delta), in the unit of the edge
// residuals.  std::domain_error when the normal equations are singular to working precision (VSL_ERR_NUMERIC: no fixed
// node).  Returns the route the device took: 0 dense, 1 band, 2 folded ring.
inline int pose_graph_covariance(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                 const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                 const LoopClosureOptions& options, const std::vector<FrameCamId>& query,
                                 std::map<FrameCamId, PoseCovariance>& cov_out, const EdgeInformation& information = EdgeInformation()) {
  cov_out.clear();
  amd::PgoFlat f;
  amd::flatten_pose_graph(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, information, f);
  std::vector<int32_t> nodes;
  for (const FrameCamId& id : query) nodes.push_back(id == cur_kf_fcid ? 0 : f.node_of.at(id));
  vsl_ba_options opt;
  opt.use_huber = 1;
  opt.huber_parameter = 1.0;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  std::vector<double> cov(36 * nodes.size());
  int storage = 0;
  const int rc = f.edge_info() ? vsl_pgo_covariance_w(amd::ctx(), &f.prob, f.edge_info(), &opt, nodes.data(), (int)nodes.size(), cov.data(), &storage)
                               : vsl_pgo_covariance(amd::ctx(), &f.prob, &opt, nodes.data(), (int)nodes.size(), cov.data(), &storage);
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(amd::ctx()));
  amd::check(rc, "pose_graph_covariance");
  for (size_t q = 0; q < nodes.size(); q++) {
    PoseCovariance& m = cov_out[query[q]];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) m(i, j) = cov[36 * q + 6 * i + j];
  }
  return storage;
}

// JOINT covariance of pairs of keyframes of that graph (vsl_pgo_joint_covariance; gtsam's jointMarginalCovariance): 12 x 12
// over the tangents of (first, second), [[S_aa, S_ab], [S_ba, S_bb]].  Same arguments and the same graph as
// pose_graph_covariance; one keyframe of a pair may be the fixed current one (cur_kf_fcid with
// options.set_current_kf_fixed): its rows and columns are zero.  cov_out: one block per entry of `pairs`, in order.
// Returns the route.
using JointPoseCovariance = Eigen::Matrix<double, 12, 12>;
inline int pose_graph_joint_covariance(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                       const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                       const LoopClosureOptions& options,
                                       const std::vector<std::pair<FrameCamId, FrameCamId>>& pairs,
                                       std::vector<JointPoseCovariance>& cov_out,
                                       const EdgeInformation& information = EdgeInformation()) {
  cov_out.clear();
  amd::PgoFlat f;
  amd::flatten_pose_graph(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, information, f);
  auto node = [&](const FrameCamId& id) { return (int32_t)(id == cur_kf_fcid ? 0 : f.node_of.at(id)); };
  std::vector<int32_t> a, b;
  for (const auto& p : pairs) {
    a.push_back(node(p.first));
    b.push_back(node(p.second));
  }
  vsl_ba_options opt;
  opt.use_huber = 1;
  opt.huber_parameter = 1.0;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  std::vector<double> cov(144 * pairs.size());
  int storage = 0;
  const int rc = f.edge_info() ? vsl_pgo_joint_covariance_w(amd::ctx(), &f.prob, f.edge_info(), &opt, a.data(), b.data(), (int)pairs.size(), cov.data(), &storage)
                               : vsl_pgo_joint_covariance(amd::ctx(), &f.prob, &opt, a.data(), b.data(), (int)pairs.size(), cov.data(), &storage);
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(amd::ctx()));
  amd::check(rc, "pose_graph_joint_covariance");
  cov_out.resize(pairs.size());
  for (size_t q = 0; q < pairs.size(); q++)
    for (int i = 0; i < 12; i++)
      for (int j = 0; j < 12; j++) cov_out[q](i, j) = cov[144 * q + 12 * i + j];
  return storage;
}

// Is a measured relative pose between two keyframes consistent with that graph (vsl_pgo_edge_consistency): the
// chi-square gate of a loop candidate, where the reference accepts on the sum of the relative translation alone.
// Same arguments and the same graph as pose_graph_covariance, plus the candidate: T_a_b = the measured T_w_a^-1 T_w_b of
// the keyframes a, b (either may be cur_kf_fcid), meas_cov its 6 x 6 covariance over (upsilon, omega) or null for
// none.  residual = log(T_w_a^-1 T_w_b) - log(T_a_b) at the poses as they stand, residual_cov its first-order
// covariance from the graph, chi2 = r^T (residual_cov + meas_cov)^-1 r with six degrees of freedom (NaN when that sum
// is not positive definite).  Returns the route.
struct LoopCandidateConsistency {
  double residual[6] = {0, 0, 0, 0, 0, 0};
  PoseCovariance residual_cov;
  double chi2 = 0;
};
inline int loop_candidate_consistency(const FrameCamId& cur_kf_fcid, Camera& cur_kf, const FrameCamId& loop_candidate_fcid,
                                      const Sophus::SE3d& sim3, Cameras& keyframes, int essential_threshold,
                                      const LoopClosureOptions& options, const FrameCamId& cand_a, const FrameCamId& cand_b,
                                      const Sophus::SE3d& T_a_b, const PoseCovariance* meas_cov, LoopCandidateConsistency& out,
                                      const EdgeInformation& information = EdgeInformation()) {
  amd::PgoFlat f;
  amd::flatten_pose_graph(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options, information, f);
  const int32_t a = cand_a == cur_kf_fcid ? 0 : f.node_of.at(cand_a), b = cand_b == cur_kf_fcid ? 0 : f.node_of.at(cand_b);
  double meas[6], mc[36], rc36[36];
  amd::rt_log(amd::rt_of(T_a_b), meas);
  if (meas_cov)
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) mc[6 * i + j] = (*meas_cov)(i, j);
  vsl_ba_options opt;
  opt.use_huber = 1;
  opt.huber_parameter = 1.0;
  opt.max_num_iterations = 0;
  opt.verbosity = 0;
  int storage = 0;
  const int rc = f.edge_info() ? vsl_pgo_edge_consistency_w(amd::ctx(), &f.prob, f.edge_info(), &opt, &a, &b, meas, meas_cov ? mc : nullptr, 1,
                                                            out.residual, rc36, &out.chi2, &storage)
                               : vsl_pgo_edge_consistency(amd::ctx(), &f.prob, &opt, &a, &b, meas, meas_cov ? mc : nullptr, 1, out.residual, rc36,
                                                          &out.chi2, &storage);
  if (rc == VSL_ERR_NUMERIC) throw std::domain_error(vsl_last_error(amd::ctx()));
  amd::check(rc, "loop_candidate_consistency");
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) out.residual_cov(i, j) = rc36[6 * i + j];
  return storage;
}

// loop_closure_utils.h:109-126
inline double compute_min_connected_covisible(const Camera& new_kf, const Cameras& keyframes, const ORBVocabularyAmd* voc, int threshold) {
  std::vector<const DBoW2::BowVector*> bows;
  for (const auto& kv : new_kf.covisible_weights)
    if (kv.second > threshold) bows.push_back(&keyframes.at(kv.first).bow_vector);
  double min_score = 1;
  for (double s : voc->score_batch(new_kf.bow_vector, bows))
    if (s < min_score) min_score = s;
  return min_score;
}
// ... with the keyframes' vectors in the device database: the neighbours are scored by index, nothing is uploaded twice
inline double compute_min_connected_covisible(const Camera& new_kf, const KeyframeDatabaseAmd& recognition_database, int threshold) {
  std::vector<FrameCamId> nbs;
  for (const auto& kv : new_kf.covisible_weights)
    if (kv.second > threshold) nbs.push_back(kv.first);
  double min_score = 1;
  for (double s : recognition_database.score(new_kf.bow_vector, nbs))
    if (s < min_score) min_score = s;
  return min_score;
}

namespace amd {
// detect_loop_candidates behind the vote (loop_closure_utils.h:199-263): `scored` = the keyframes whose count is above
// 0.8 of the maximum, in the order of the walk, with their scores.  A graph neighbour adds to the accumulated score
// when its own count is above the threshold -- that is, when it is one of `scored`.
inline std::vector<FrameCamId> loop_candidates_of_scored(const FrameCamId& new_kf_fcid, const Camera& new_kf, const CovisibilityGraph& graph,
                                                         double min_score, const std::vector<FrameCamId>& scored,
                                                         const std::vector<double>& scores, size_t n_sharing, int max_num_sharing_words) {
  if (std::getenv("VISNAV_AMD_TRACE")) {
    std::fprintf(stderr, "  loop candidates of %lld: %zu keyframes share words (max %d), %zu above 0.8 max:", (long long)new_kf_fcid.frame_id,
                 n_sharing, max_num_sharing_words, scored.size());
    for (size_t i = 0; i < scored.size(); i++) std::fprintf(stderr, " %lld=%.3f", (long long)scored[i].frame_id, scores[i]);
    std::fprintf(stderr, " | connected: %zu, bow nnz %zu\n", graph.at(new_kf_fcid).size(), new_kf.bow_vector.size());
  }
  std::vector<std::pair<double, FrameCamId>> loop_score_and_match;
  std::unordered_map<FrameCamId, double, FrameCamIdHash> loop_score;
  for (size_t i = 0; i < scored.size(); i++) {
    loop_score[scored[i]] = scores[i];
    if (scores[i] >= min_score) loop_score_and_match.emplace_back(scores[i], scored[i]);
  }
  if (loop_score_and_match.empty()) return {};
  double best_acc_score = min_score;
  for (const auto& score_fcid : loop_score_and_match) {
    double acc_score = score_fcid.first;
    for (const auto& nb : graph.at(score_fcid.second)) {
      auto it = loop_score.find(nb);
      if (it != loop_score.end()) acc_score += it->second;
    }
    if (acc_score > best_acc_score) best_acc_score = acc_score;
  }
  const double min_score_to_retain = 0.75f * best_acc_score;
  std::set<FrameCamId> already_added_kf;
  std::vector<FrameCamId> loop_candidates;
  for (const auto& score_fcid : loop_score_and_match)
    if (score_fcid.first > min_score_to_retain && !already_added_kf.count(score_fcid.second)) {
      loop_candidates.push_back(score_fcid.second);
      already_added_kf.insert(score_fcid.second);
    }
  return loop_candidates;
}
}  // namespace amd

// loop_closure_utils.h:141-263.  The reference walks unordered_maps; here candidates are visited in the order their
// first shared word was met (deterministic), everything else -- the counting quirk (a keyframe's first shared word counts
// 0), the 0.8 / 0.75 fractions, the accumulation over graph neighbours -- is the reference's.
inline std::vector<FrameCamId> detect_loop_candidates(const FrameCamId& new_kf_fcid, const Camera& new_kf, const Cameras& keyframes,
                                                      const CovisibilityGraph& graph, double min_score,
                                                      DBoWInvertedFile& recognition_database, const ORBVocabularyAmd* voc) {
  const std::set<FrameCamId>& connected_frames = graph.at(new_kf_fcid);
  std::unordered_map<FrameCamId, int, FrameCamIdHash> num_sharing_words;
  std::vector<FrameCamId> first_seen;
  bool has_any_sharing_words = false;
  auto bump = [&](const FrameCamId& f) {
    auto it = num_sharing_words.find(f);
    if (it != num_sharing_words.end()) {
      it->second += 1;
    } else {
      num_sharing_words[f] = 0;
      first_seen.push_back(f);
    }
  };
  for (const auto& wv : new_kf.bow_vector) {
    if (wv.first >= recognition_database.size()) continue;
    has_any_sharing_words = true;
    for (const auto& lkf : recognition_database[wv.first]) {
      if (!connected_frames.count(lkf)) {
        bump(lkf);
      } else if (new_kf.covisible_weights.at(lkf) < 30) {
        bump(lkf);
      }
    }
  }
  if (!has_any_sharing_words || num_sharing_words.empty()) return {};
  int max_num_sharing_words = 0;
  for (const auto& kv : num_sharing_words) max_num_sharing_words = std::max(max_num_sharing_words, kv.second);
  const int sharing_words_threshold = (int)(max_num_sharing_words * 0.8f);
  std::vector<FrameCamId> scored;
  std::vector<const DBoW2::BowVector*> bows;
  for (const auto& f : first_seen)
    if (num_sharing_words.at(f) > sharing_words_threshold) {
      scored.push_back(f);
      bows.push_back(&keyframes.at(f).bow_vector);
    }
  const std::vector<double> scores = voc->score_batch(new_kf.bow_vector, bows);  // ONE launch for all candidates
  return amd::loop_candidates_of_scored(new_kf_fcid, new_kf, graph, min_score, scored, scores, num_sharing_words.size(),
                                        max_num_sharing_words);
}
// ... with the device database: the walk, the 0.8 rule and the scores are ONE query (vsl_bowdb_query); a connected
// keyframe takes part in the vote only when its covisible weight is below 30
inline std::vector<FrameCamId> detect_loop_candidates(const FrameCamId& new_kf_fcid, const Camera& new_kf, const Cameras& keyframes,
                                                      const CovisibilityGraph& graph, double min_score,
                                                      KeyframeDatabaseAmd& recognition_database, const ORBVocabularyAmd* voc) {
  (void)keyframes;
  (void)voc;
  std::vector<FrameCamId> excluded;
  for (const auto& f : graph.at(new_kf_fcid))
    if (recognition_database.contains(f) && new_kf.covisible_weights.at(f) >= 30) excluded.push_back(f);
  // with the device BoW (OdometryOptions::device_bow) the keyframe's own vector is already stored: it takes no part
  if (recognition_database.contains(new_kf_fcid)) excluded.push_back(new_kf_fcid);
  const KeyframeDatabaseAmd::Survivors sv = recognition_database.query_loop(new_kf.bow_vector, excluded);
  if (sv.n_sharing == 0) return {};
  return amd::loop_candidates_of_scored(new_kf_fcid, new_kf, graph, min_score, sv.fcids, sv.scores, (size_t)sv.n_sharing, sv.max_count);
}

// loop_closure_utils.h:269-276
inline void insert_new_kf_to_db(const FrameCamId& new_kf_fcid, const Camera& new_kf, DBoWInvertedFile& recognition_database) {
  for (const auto& wv : new_kf.bow_vector)
    if (wv.first < recognition_database.size()) recognition_database[wv.first].push_back(new_kf_fcid);
}
inline void insert_new_kf_to_db(const FrameCamId& new_kf_fcid, const Camera& new_kf, KeyframeDatabaseAmd& recognition_database) {
  recognition_database.insert(new_kf_fcid, new_kf.bow_vector);
}

namespace amd {
inline double min_connected_score(const Camera& new_kf, const Cameras& keyframes, const ORBVocabularyAmd* voc, const DBoWInvertedFile&, int threshold) {
  return compute_min_connected_covisible(new_kf, keyframes, voc, threshold);
}
inline double min_connected_score(const Camera& new_kf, const Cameras&, const ORBVocabularyAmd*, const KeyframeDatabaseAmd& db, int threshold) {
  return compute_min_connected_covisible(new_kf, db, threshold);
}

// loop_closure_utils.h:294-388 over either form of the recognition database
template <class Database>
inline bool detect_loop_closure_on(const FrameCamId& new_kf_fcid, const Camera& new_kf, const Cameras& keyframes,
                                   Database& recognition_database, const ORBVocabularyAmd* voc, const CovisibilityGraph& graph,
                                   ConsistentGroups& consistent_groups, std::vector<FrameCamId>& enough_consistent_candidates, int threshold,
                                   int num_consistency_threshold) {
  const double min_score = min_connected_score(new_kf, keyframes, voc, recognition_database, threshold);
  const std::vector<FrameCamId> loop_candidates =
      detect_loop_candidates(new_kf_fcid, new_kf, keyframes, graph, min_score, recognition_database, voc);
  if (std::getenv("VISNAV_AMD_TRACE")) {
    std::fprintf(stderr, "loop detection keyframe %lld: min covisible score %.4f, %zu candidates:", (long long)new_kf_fcid.frame_id, min_score, loop_candidates.size());
    for (const auto& c : loop_candidates) std::fprintf(stderr, " %lld", (long long)c.frame_id);
    std::fprintf(stderr, " (groups %zu)\n", consistent_groups.size());
  }
  if (loop_candidates.empty()) {
    consistent_groups.clear();
    if (new_kf_fcid.cam_id == 0) insert_new_kf_to_db(new_kf_fcid, new_kf, recognition_database);
    return false;
  }
  enough_consistent_candidates.clear();
  ConsistentGroups current_consistent_groups;
  std::vector<bool> is_old_groups_consistent(consistent_groups.size(), false);
  for (const FrameCamId& candidate_fcid : loop_candidates) {
    std::set<FrameCamId> candidate_group = graph.at(candidate_fcid);
    candidate_group.insert(candidate_fcid);
    bool enough_consistent = false, consistent_in_some_groups = false;
    int idx = 0;
    for (auto& g : consistent_groups) {
      bool is_consistent = false;
      for (const auto& f : candidate_group)
        if (g.first.count(f)) {
          is_consistent = true;
          consistent_in_some_groups = true;
          break;
        }
      if (is_consistent) {
        const int num_curr_consistency = g.second + 1;
        if (!is_old_groups_consistent[(size_t)idx]) {
          current_consistent_groups.emplace_back(candidate_group, num_curr_consistency);
          is_old_groups_consistent[(size_t)idx] = true;
        }
        if (num_curr_consistency >= num_consistency_threshold && !enough_consistent) {
          enough_consistent_candidates.push_back(candidate_fcid);
          enough_consistent = true;
        }
      }
      idx++;
    }
    if (!consistent_in_some_groups) current_consistent_groups.emplace_back(candidate_group, 0);
  }
  consistent_groups = current_consistent_groups;
  if (new_kf_fcid.cam_id == 0) insert_new_kf_to_db(new_kf_fcid, new_kf, recognition_database);
  return !enough_consistent_candidates.empty();
}
}  // namespace amd

// loop_closure_utils.h:294-388
inline bool detect_loop_closure(const FrameCamId& new_kf_fcid, const Camera& new_kf, const Cameras& keyframes,
                                DBoWInvertedFile& recognition_database, const ORBVocabularyAmd* voc, const CovisibilityGraph& graph,
                                ConsistentGroups& consistent_groups, std::vector<FrameCamId>& enough_consistent_candidates, int threshold,
                                int num_consistency_threshold) {
  return amd::detect_loop_closure_on(new_kf_fcid, new_kf, keyframes, recognition_database, voc, graph, consistent_groups,
                                     enough_consistent_candidates, threshold, num_consistency_threshold);
}
inline bool detect_loop_closure(const FrameCamId& new_kf_fcid, const Camera& new_kf, const Cameras& keyframes,
                                KeyframeDatabaseAmd& recognition_database, const ORBVocabularyAmd* voc, const CovisibilityGraph& graph,
                                ConsistentGroups& consistent_groups, std::vector<FrameCamId>& enough_consistent_candidates, int threshold,
                                int num_consistency_threshold) {
  return amd::detect_loop_closure_on(new_kf_fcid, new_kf, keyframes, recognition_database, voc, graph, consistent_groups,
                                     enough_consistent_candidates, threshold, num_consistency_threshold);
}

// loop_closure_utils.h:398-416
inline void loop_align(const FrameCamId& cur_kf_fcid, Camera cur_kf, const FrameCamId& loop_candidate_fcid, const Sophus::SE3d& T_0_1,
                       const Sophus::SE3d& sim3, Cameras& keyframes, Landmarks& landmarks) {
  (void)cur_kf_fcid;
  (void)landmarks;
  const amd::Rt cur = amd::rt_of(cur_kf.T_w_c);
  // cur_kf.T_w_c * (cur_kf.T_w_c^-1 * T_w_candidate * sim3) = T_w_candidate * sim3
  const amd::Rt aligned = amd::rt_mul(cur, amd::rt_mul(amd::rt_mul(amd::rt_inv(cur), amd::rt_of(keyframes.at(loop_candidate_fcid).T_w_c)), amd::rt_of(sim3)));
  for (const auto& kv : cur_kf.covisible_rel_poses) {
    keyframes.at(kv.first).T_w_c = amd::se3_of(amd::rt_mul(aligned, amd::rt_of(kv.second)));
    keyframes.at(FrameCamId(kv.first.frame_id, 1)).T_w_c = amd::se3_of(amd::rt_mul(amd::rt_of(keyframes.at(kv.first).T_w_c), amd::rt_of(T_0_1)));
  }
}

// loop_closure_utils.h:593-601
inline void update_stereo_pair(const FrameCamId& cur_kf_fcid, Camera cur_kf, const Sophus::SE3d T_0_1, Cameras& keyframes) {
  (void)cur_kf_fcid;
  (void)cur_kf;
  for (auto& kv : keyframes)
    if (kv.first.cam_id == 1)
      kv.second.T_w_c = amd::se3_of(amd::rt_mul(amd::rt_of(keyframes.at(FrameCamId(kv.first.frame_id, 0)).T_w_c), amd::rt_of(T_0_1)));
}

// loop_closure_utils.h:607-621
inline void update_landmark_position(const FrameCamId& cur_kf_fcid, const Camera& cur_kf, const Cameras& keyframes, Landmarks& landmarks) {
  for (auto& kv : landmarks) {
    const Camera* from = nullptr;
    auto it = keyframes.find(kv.second.from_fcid);
    if (it != keyframes.end())
      from = &it->second;
    else if (cur_kf_fcid == kv.second.from_fcid)
      from = &cur_kf;
    if (!from) continue;
    const amd::Rt T = amd::rt_of(from->T_w_c);
    double o[3];
    amd::qrot(T.q, kv.second.p_c.data(), o);
    for (int i = 0; i < 3; i++) kv.second.p.data()[i] = o[i] + T.t[i];
  }
}

// loop_closure_utils.h:633-648.  cur_kf is taken BY VALUE like the reference does: the optimised pose of the current
// keyframe is dropped (with set_current_kf_fixed it does not move anyway) and the caller inserts its own copy afterwards.
inline void loop_closure(const FrameCamId& cur_kf_fcid, Camera cur_kf, const FrameCamId& loop_candidate_fcid, const Sophus::SE3d T_0_1,
                         const Sophus::SE3d& sim3, Cameras& keyframes, Landmarks& landmarks, int essential_threshold,
                         const LoopClosureOptions& options) {
  loop_align(cur_kf_fcid, cur_kf, loop_candidate_fcid, T_0_1, sim3, keyframes, landmarks);
  pose_graph_optimization(cur_kf_fcid, cur_kf, loop_candidate_fcid, sim3, keyframes, essential_threshold, options);
  update_stereo_pair(cur_kf_fcid, cur_kf, T_0_1, keyframes);
  update_landmark_position(cur_kf_fcid, cur_kf, keyframes, landmarks);
}

// loop_closure_utils.h:417-427: "Not implemented..." upstream, and the same no-op here
inline void landmark_fusion(const FrameCamId& cur_kf_fcid, Camera cur_kf, const FrameCamId& loop_candidate_fcid, const Sophus::SE3d& sim3,
                            Cameras& keyframes, Landmarks& landmarks) {
  (void)cur_kf_fcid;
  (void)cur_kf;
  (void)loop_candidate_fcid;
  (void)sim3;
  (void)keyframes;
  (void)landmarks;
}

struct LandmarkFusionOptions {  // the matching parameters of project_landmarks / find_matches_landmarks (src/slam.cpp:258-309)
  double cam_z_threshold = 0.1;
  double match_max_dist_2d = 20.0;
  int feature_match_threshold = 70;
  double feature_match_dist_2_best = 1.2;
  int max_views = 32;  // at most 64 (vsl_fuse_search)
};

// The working form, meant to run after loop_closure() has aligned the poses (they are read as they are): the landmarks
// seen from the loop candidate's neighbourhood (targets, ascending TrackId, with all their all_obs descriptors) are
// searched in the current keyframe and its covisible left keyframes (views) by ONE vsl_fuse_search call, and the matches
// become added observations or merged tracks by the rules of fusion_plan.h.
inline void landmark_fusion(const FrameCamId& cur_kf_fcid, Camera cur_kf, const FrameCamId& loop_candidate_fcid, const Sophus::SE3d& sim3,
                            Cameras& keyframes, Landmarks& landmarks, const Corners& feature_corners, const Calibration& calib_cam,
                            const CovisibilityGraph& graph, const LandmarkFusionOptions& options = LandmarkFusionOptions(),
                            LandmarkFusionResult* result = nullptr) {
  (void)sim3;
  if (result) *result = LandmarkFusionResult();
  // ---- views: the current left keyframe + its covisible left keyframes, the strongest max_views of them
  std::vector<std::pair<int, FrameCamId>> nbs;  // (-weight, fcid): ascending = heaviest first, ties by FrameCamId
  for (const auto& kv : cur_kf.covisible_rel_poses) {
    if (kv.first.cam_id != 0 || kv.first == cur_kf_fcid || !keyframes.count(kv.first) || !feature_corners.count(kv.first)) continue;
    const auto w = cur_kf.covisible_weights.find(kv.first);
    nbs.emplace_back(w == cur_kf.covisible_weights.end() ? 0 : -w->second, kv.first);
  }
  std::sort(nbs.begin(), nbs.end());
  const size_t max_views = (size_t)std::max(1, std::min(options.max_views, 64));
  std::vector<FrameCamId> view_ids;
  if (feature_corners.count(cur_kf_fcid)) view_ids.push_back(cur_kf_fcid);
  for (const auto& nb : nbs)
    if (view_ids.size() < max_views) view_ids.push_back(nb.second);
  std::sort(view_ids.begin(), view_ids.end());
  // ---- targets: every landmark observed from the loop candidate or one of its graph neighbours
  std::set<FrameCamId> old_group;
  old_group.insert(loop_candidate_fcid);
  const auto g = graph.find(loop_candidate_fcid);
  if (g != graph.end()) old_group.insert(g->second.begin(), g->second.end());
  std::vector<TrackId> table;
  for (const auto& kv : landmarks)
    for (const auto& ob : kv.second.all_obs)
      if (old_group.count(ob.first)) {
        table.push_back(kv.first);
        break;
      }
  std::sort(table.begin(), table.end());
  if (view_ids.empty() || table.empty()) return;

  std::vector<double> pose7, kp_xy, points;
  std::vector<int32_t> kp_start(1, 0), obs_start(1, 0);
  std::vector<uint64_t> kp_desc, obs_desc;
  for (const FrameCamId& v : view_ids) {
    const auto kf = keyframes.find(v);
    const double* T = (kf != keyframes.end() ? kf->second.T_w_c : cur_kf.T_w_c).data();
    pose7.insert(pose7.end(), T, T + 7);
    const KeypointsData& kd = feature_corners.at(v);
    const size_t n = std::min(kd.corners.size(), kd.corner_descriptors.size());
    for (size_t i = 0; i < n; i++) {
      kp_xy.push_back(kd.corners[i][0]);
      kp_xy.push_back(kd.corners[i][1]);
      const uint64_t* w = reinterpret_cast<const uint64_t*>(&kd.corner_descriptors[i]);
      kp_desc.insert(kp_desc.end(), w, w + 4);
    }
    kp_start.push_back((int32_t)(kp_xy.size() / 2));
  }
  for (const TrackId tid : table) {
    const Landmark& lm = landmarks.at(tid);
    points.insert(points.end(), lm.p.data(), lm.p.data() + 3);
    for (const auto& ob : lm.all_obs) {
      const auto kd = feature_corners.find(ob.first);
      if (kd == feature_corners.end() || (size_t)ob.second >= kd->second.corner_descriptors.size()) continue;
      const uint64_t* w = reinterpret_cast<const uint64_t*>(&kd->second.corner_descriptors[(size_t)ob.second]);
      obs_desc.insert(obs_desc.end(), w, w + 4);
    }
    obs_start.push_back((int32_t)(obs_desc.size() / 4));
  }
  const auto& cam = calib_cam.intrinsics[0];
  const int n_views = (int)view_ids.size();
  std::vector<int32_t> pairs(2 * (size_t)kp_start.back() + 2), pair_start((size_t)n_views + 1, 0);
  amd::check(vsl_fuse_search(amd::ctx(), n_views, pose7.data(), amd::camera_model_id(cam->name()), cam->data(), cam->width(),
                             cam->height(), kp_start.data(), kp_xy.data(), kp_desc.data(), (int)table.size(), points.data(),
                             obs_start.data(), obs_desc.data(), options.cam_z_threshold, options.match_max_dist_2d,
                             options.feature_match_threshold, options.feature_match_dist_2_best, pairs.data(), pair_start.data(),
                             nullptr),
             "landmark_fusion");
  std::vector<amd::FusionView> views((size_t)n_views);
  for (int v = 0; v < n_views; v++) {
    views[(size_t)v].fcid = view_ids[(size_t)v];
    for (int32_t i = pair_start[(size_t)v]; i < pair_start[(size_t)v + 1]; i++)
      views[(size_t)v].pairs.emplace_back((FeatureId)pairs[2 * (size_t)i], pairs[2 * (size_t)i + 1]);
  }
  const LandmarkFusionResult r = amd::apply_fusion_plan(
      views, amd::fusion_obs_lookup(landmarks, std::set<FrameCamId>(view_ids.begin(), view_ids.end())), table, keyframes, landmarks);
  if (result) *result = r;
}

}  // namespace visnav
