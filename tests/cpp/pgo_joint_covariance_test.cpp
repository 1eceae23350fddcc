// Drives visnav::pose_graph_joint_covariance and visnav::loop_candidate_consistency (include/visnav_amd/loop_closure.h)
// on a keyframe map written by tests/test_pgo_joint_covariance_dropin.py (the format of pgo_covariance_test.cpp; the
// query is a list of frame-id pairs), beside vsl_pgo_joint_covariance / vsl_pgo_edge_consistency called directly on the
// problem amd::flatten_pose_graph makes of the same map.  The candidate is the FIRST pair with the measurement sim3.
//   pgo_joint_covariance_test in.bin           host only: flattens and prints the graph's size
//   pgo_joint_covariance_test in.bin out.bin   [wrapper blocks | direct blocks | wrapper r, Sigma_r, chi2 | direct r, Sigma_r,
//                                              chi2 | routes: joint wrapper, joint direct, consistency wrapper, direct]
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
  Cameras keyframes;
  for (int i = 0; i < K - 1; i++) keyframes[FrameCamId(i, 0)] = cams[i];
  Camera cur = cams[K - 1];
  const FrameCamId cur_id(K - 1, 0);
  LoopClosureOptions opt;
  opt.verbosity_level = 0;
  opt.set_current_kf_fixed = fixed_cur != 0;

  amd::PgoFlat f;
  amd::flatten_pose_graph(cur, FrameCamId(loop_cand, 0), sim3, keyframes, essential, opt, f);
  if (f.prob.n_nodes != K || (int)f.node_of.size() != K - 1) return 4;
  if (argc < 3) {
    std::printf("flatten ok: %d nodes, %d edges\n", f.prob.n_nodes, f.prob.n_edges);
    return 0;
  }
  if (nq < 1) return 3;
  std::vector<std::pair<FrameCamId, FrameCamId>> pairs;
  for (int q = 0; q < nq; q++) pairs.emplace_back(FrameCamId(qf[2 * q], 0), FrameCamId(qf[2 * q + 1], 0));
  std::vector<Sophus::SE3d> before;
  for (int i = 0; i < K - 1; i++) before.push_back(keyframes[FrameCamId(i, 0)].T_w_c);
  std::vector<JointPoseCovariance> cov;
  const int route = pose_graph_joint_covariance(cur_id, cur, FrameCamId(loop_cand, 0), sim3, keyframes, essential, opt, pairs, cov);
  LoopCandidateConsistency cons;
  const int route_c = loop_candidate_consistency(cur_id, cur, FrameCamId(loop_cand, 0), sim3, keyframes, essential, opt, pairs[0].first,
                                                 pairs[0].second, sim3, nullptr, cons);
  for (int i = 0; i < K - 1; i++)
    for (int c = 0; c < 7; c++)
      if (before[i].data()[c] != keyframes[FrameCamId(i, 0)].T_w_c.data()[c]) return 5;  // nothing is optimised

  auto node = [&](const FrameCamId& id) { return (int32_t)(id == cur_id ? 0 : f.node_of.at(id)); };
  std::vector<int32_t> a, b;
  for (const auto& p : pairs) {
    a.push_back(node(p.first));
    b.push_back(node(p.second));
  }
  vsl_ba_options o;
  o.use_huber = 1;
  o.huber_parameter = 1.0;
  o.max_num_iterations = 0;
  o.verbosity = 0;
  std::vector<double> direct(144 * pairs.size());
  int route_direct = -1, route_direct_c = -1;
  if (vsl_pgo_joint_covariance(amd::ctx(), &f.prob, &o, a.data(), b.data(), nq, direct.data(), &route_direct) != VSL_OK) {
    std::fprintf(stderr, "vsl_pgo_joint_covariance: %s\n", vsl_last_error(amd::ctx()));
    return 6;
  }
  double meas[6], dr[6], dc[36], dx = 0;
  amd::rt_log(amd::rt_of(sim3), meas);
  if (vsl_pgo_edge_consistency(amd::ctx(), &f.prob, &o, a.data(), b.data(), meas, nullptr, 1, dr, dc, &dx, &route_direct_c) != VSL_OK) {
    std::fprintf(stderr, "vsl_pgo_edge_consistency: %s\n", vsl_last_error(amd::ctx()));
    return 7;
  }
  std::ofstream out(argv[2], std::ios::binary);
  auto put = [&](const double* p, size_t n) { out.write(reinterpret_cast<const char*>(p), sizeof(double) * n); };
  for (const JointPoseCovariance& m : cov)
    for (int i = 0; i < 12; i++)
      for (int j = 0; j < 12; j++) put(&m(i, j), 1);
  put(direct.data(), direct.size());
  put(cons.residual, 6);
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) put(&cons.residual_cov(i, j), 1);
  put(&cons.chi2, 1);
  put(dr, 6);
  put(dc, 36);
  put(&dx, 1);
  const double tail[4] = {(double)route, (double)route_direct, (double)route_c, (double)route_direct_c};
  put(tail, 4);
  return 0;
}
