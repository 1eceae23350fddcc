// Drives the overloads of include/visnav_amd/loop_closure.h that take an EdgeInformation -- flatten_pose_graph,
// pose_graph_optimization, pose_graph_covariance, pose_graph_joint_covariance, loop_candidate_consistency -- on a keyframe
// map written by tests/test_pgo_weighted_dropin.py (the format of pgo_joint_covariance_test.cpp), beside the _w entry
// points of the C ABI called directly on the flattened problem, and the existing signatures beside the unweighted C ABI.
// The information: diag(1e2 x 3, 1e4 x 3) on every edge, 50 I on the loop constraint (current keyframe -> candidate).
//   pgo_weighted_test in.bin           host only: flattens with the callback and prints the graph's size
//   pgo_weighted_test in.bin out.bin   two records, weighted then unweighted, each
//                                      [wrapper | direct] x (poses 7 K, covariances 36 nq, joint 144 nq, r Sigma_r chi2 43)
#include <cstdio>
#include <fstream>
#include <vector>

#include "visnav_amd/loop_closure.h"

using namespace visnav;

template <class T>
static void get(std::ifstream& f, T* p, size_t n) {
  f.read(reinterpret_cast<char*>(p), sizeof(T) * n);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t K, essential, fixed_cur, loop_cand;
  get(in, &K, 1);
  get(in, &essential, 1);
  get(in, &fixed_cur, 1);
  get(in, &loop_cand, 1);
  std::vector<Camera> cams(K);
  for (int i = 0; i < K; i++) {
    get(in, cams[i].T_w_c.data(), 7);
    int32_t last, ncov;
    get(in, &last, 1);
    get(in, &ncov, 1);
    cams[i].last_fcid = FrameCamId(last, 0);
    for (int c = 0; c < ncov; c++) {
      int32_t other, weight;
      Sophus::SE3d rel;
      get(in, &other, 1);
      get(in, &weight, 1);
      get(in, rel.data(), 7);
      cams[i].covisible_weights[FrameCamId(other, 0)] = weight;
      cams[i].covisible_rel_poses[FrameCamId(other, 0)] = rel;
    }
  }
  Sophus::SE3d sim3;
  get(in, sim3.data(), 7);
  int32_t nq;
  get(in, &nq, 1);
  std::vector<int32_t> qf(2 * (size_t)nq);
  get(in, qf.data(), qf.size());
  if (!in) return 3;
  const FrameCamId cur_id(K - 1, 0), cand_id(loop_cand, 0);
  LoopClosureOptions opt;
  opt.verbosity_level = 0;
  opt.set_current_kf_fixed = fixed_cur != 0;
  const EdgeInformation info = [&](const FrameCamId& a, const FrameCamId& b) {
    PoseCovariance W;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) W(i, j) = i != j ? 0.0 : (a == cur_id && b == cand_id ? 50.0 : (i < 3 ? 1e2 : 1e4));
    return W;
  };
  auto fresh = [&](Cameras& keyframes, Camera& cur) {
    keyframes.clear();
    for (int i = 0; i < K - 1; i++) keyframes[FrameCamId(i, 0)] = cams[i];
    cur = cams[K - 1];
  };
  Cameras keyframes;
  Camera cur;
  fresh(keyframes, cur);
  {
    amd::PgoFlat f;
    amd::flatten_pose_graph(cur_id, cur, cand_id, sim3, keyframes, essential, opt, info, f);
    if (f.prob.n_nodes != K || f.info.size() != 36 * (size_t)f.prob.n_edges) return 4;
    int loops = 0;
    for (int e = 0; e < f.prob.n_edges; e++) loops += f.info[36 * (size_t)e] == 50.0;
    amd::PgoFlat plain;
    amd::flatten_pose_graph(cur_id, cur, cand_id, sim3, keyframes, essential, opt, EdgeInformation(), plain);
    if (loops != 1 || plain.edge_info() != nullptr || plain.prob.n_edges != f.prob.n_edges) return 4;
    if (argc < 3) {
      std::printf("flatten ok: %d nodes, %d edges, %d weighted as the loop constraint\n", f.prob.n_nodes, f.prob.n_edges, loops);
      return 0;
    }
  }
  if (nq < 1) return 3;
  std::vector<std::pair<FrameCamId, FrameCamId>> pairs;
  std::vector<FrameCamId> query;
  for (int q = 0; q < nq; q++) {
    pairs.emplace_back(FrameCamId(qf[2 * q], 0), FrameCamId(qf[2 * q + 1], 0));
    query.push_back(pairs.back().first == cur_id ? pairs.back().second : pairs.back().first);  // a free keyframe of the pair
  }
  std::ofstream out(argv[2], std::ios::binary);
  auto put = [&](const double* p, size_t n) { out.write(reinterpret_cast<const char*>(p), sizeof(double) * n); };
  vsl_ba_options o;
  o.use_huber = 1;
  o.huber_parameter = 1.0;
  o.verbosity = 0;
  for (int weighted = 1; weighted >= 0; weighted--) {
    // ---- wrappers: marginals at the poses as they stand, then the solve
    fresh(keyframes, cur);
    std::map<FrameCamId, PoseCovariance> cov;
    std::vector<JointPoseCovariance> joint;
    LoopCandidateConsistency cons;
    if (weighted) {
      pose_graph_covariance(cur_id, cur, cand_id, sim3, keyframes, essential, opt, query, cov, info);
      pose_graph_joint_covariance(cur_id, cur, cand_id, sim3, keyframes, essential, opt, pairs, joint, info);
      loop_candidate_consistency(cur_id, cur, cand_id, sim3, keyframes, essential, opt, pairs[0].first, pairs[0].second, sim3, nullptr, cons, info);
      pose_graph_optimization(cur_id, cur, cand_id, sim3, keyframes, essential, opt, info);
    } else {
      pose_graph_covariance(cur_id, cur, cand_id, sim3, keyframes, essential, opt, query, cov);
      pose_graph_joint_covariance(cur_id, cur, cand_id, sim3, keyframes, essential, opt, pairs, joint);
      loop_candidate_consistency(cur_id, cur, cand_id, sim3, keyframes, essential, opt, pairs[0].first, pairs[0].second, sim3, nullptr, cons);
      pose_graph_optimization(cur_id, cur, cand_id, sim3, keyframes, essential, opt);
    }
    for (int i = 0; i < K; i++) put((i == K - 1 ? cur : keyframes[FrameCamId(i, 0)]).T_w_c.data(), 7);
    // ---- the C ABI on the flattened problem of the same map
    fresh(keyframes, cur);
    amd::PgoFlat f;
    amd::flatten_pose_graph(cur_id, cur, cand_id, sim3, keyframes, essential, opt, weighted ? info : EdgeInformation(), f);
    auto node = [&](const FrameCamId& id) { return (int32_t)(id == cur_id ? 0 : f.node_of.at(id)); };
    std::vector<int32_t> a, b, nodes;
    for (int q = 0; q < nq; q++) {
      a.push_back(node(pairs[q].first));
      b.push_back(node(pairs[q].second));
      nodes.push_back(node(query[q]));
    }
    std::vector<double> dcov(36 * (size_t)nq), djoint(144 * (size_t)nq);
    double meas[6], dr[6], dc[36], dx = 0;
    amd::rt_log(amd::rt_of(sim3), meas);
    o.max_num_iterations = 0;
    int rc;
    if (weighted) {
      rc = vsl_pgo_covariance_w(amd::ctx(), &f.prob, f.edge_info(), &o, nodes.data(), nq, dcov.data(), nullptr);
      if (!rc) rc = vsl_pgo_joint_covariance_w(amd::ctx(), &f.prob, f.edge_info(), &o, a.data(), b.data(), nq, djoint.data(), nullptr);
      if (!rc) rc = vsl_pgo_edge_consistency_w(amd::ctx(), &f.prob, f.edge_info(), &o, a.data(), b.data(), meas, nullptr, 1, dr, dc, &dx, nullptr);
      o.max_num_iterations = 20;
      if (!rc) rc = vsl_pose_graph_optimize_w(amd::ctx(), &f.prob, f.edge_info(), &o, nullptr);
    } else {
      rc = vsl_pgo_covariance(amd::ctx(), &f.prob, &o, nodes.data(), nq, dcov.data(), nullptr);
      if (!rc) rc = vsl_pgo_joint_covariance(amd::ctx(), &f.prob, &o, a.data(), b.data(), nq, djoint.data(), nullptr);
      if (!rc) rc = vsl_pgo_edge_consistency(amd::ctx(), &f.prob, &o, a.data(), b.data(), meas, nullptr, 1, dr, dc, &dx, nullptr);
      o.max_num_iterations = 20;
      if (!rc) rc = vsl_pose_graph_optimize(amd::ctx(), &f.prob, &o, nullptr);
    }
    if (rc) {
      std::fprintf(stderr, "C ABI (%s): %s\n", weighted ? "weighted" : "unweighted", vsl_last_error(amd::ctx()));
      return 6;
    }
    for (int i = 0; i < K; i++) put(f.poses.data() + 7 * (size_t)(i == K - 1 ? 0 : f.node_of.at(FrameCamId(i, 0))), 7);
    for (int q = 0; q < nq; q++)
      for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) put(&cov.at(query[q])(i, j), 1);
    put(dcov.data(), dcov.size());
    for (const JointPoseCovariance& m : joint)
      for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) put(&m(i, j), 1);
    put(djoint.data(), djoint.size());
    put(cons.residual, 6);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) put(&cons.residual_cov(i, j), 1);
    put(&cons.chi2, 1);
    put(dr, 6);
    put(dc, 36);
    put(&dx, 1);
  }
  // a matrix that is not positive definite: std::invalid_argument, no pose written
  fresh(keyframes, cur);
  const EdgeInformation bad = [&](const FrameCamId&, const FrameCamId&) {
    PoseCovariance W;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) W(i, j) = 0.0;
    return W;
  };
  bool thrown = false;
  try {
    pose_graph_optimization(cur_id, cur, cand_id, sim3, keyframes, essential, opt, bad);
  } catch (const std::invalid_argument&) {
    thrown = true;
  }
  for (int i = 0; i < K - 1; i++)
    for (int c = 0; c < 7; c++)
      if (cams[i].T_w_c.data()[c] != keyframes[FrameCamId(i, 0)].T_w_c.data()[c]) return 5;
  return thrown ? 0 : 7;
}
