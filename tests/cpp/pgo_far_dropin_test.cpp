// Drives visnav::pose_graph_optimization_far_edges (include/visnav_amd/loop_closure.h) on a keyframe map written by
// tests/test_pgo_far_dropin.py (the format of pgo_joint_covariance_test.cpp), beside vsl_pose_graph_optimize called
// directly on the flattened problem with the "pgo_far_edges" diagnostic set.
//   pgo_far_dropin_test in.bin           host only: flattens and prints the graph's size
//   pgo_far_dropin_test in.bin out.bin   [wrapper poses 7 K | direct poses 7 K | wrapper report 5 | direct report 5 |
//                                        diagnostic before, after (found off), before, after (found on)]
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
  if (!in) return 3;
  const FrameCamId cur_id(K - 1, 0), cand_id(loop_cand, 0);
  LoopClosureOptions opt;
  opt.verbosity_level = 0;
  opt.set_current_kf_fixed = fixed_cur != 0;
  Cameras keyframes;
  Camera cur;
  auto fresh = [&]() {
    keyframes.clear();
    for (int i = 0; i < K - 1; i++) keyframes[FrameCamId(i, 0)] = cams[i];
    cur = cams[K - 1];
  };
  fresh();
  if (argc < 3) {
    amd::PgoFlat f;
    amd::flatten_pose_graph(cur, cand_id, sim3, keyframes, essential, opt, f);
    std::printf("flatten ok: %d nodes, %d edges\n", f.prob.n_nodes, f.prob.n_edges);
    return 0;
  }
  std::ofstream out(argv[2], std::ios::binary);
  auto put = [&](const double* p, size_t n) { out.write(reinterpret_cast<const char*>(p), sizeof(double) * n); };
  auto diag = [](int* v) { return vsl_ctx_get_diagnostic(amd::ctx(), "pgo_far_edges", v); };
  // ---- the wrapper, found off
  int before_off = -1, after_off = -1, before_on = -1, after_on = -1;
  if (diag(&before_off)) return 4;
  PoseGraphFarEdges rep;
  pose_graph_optimization_far_edges(cur_id, cur, cand_id, sim3, keyframes, essential, opt, EdgeInformation(), &rep);
  if (diag(&after_off)) return 4;
  for (int i = 0; i < K; i++) put((i == K - 1 ? cur : keyframes[FrameCamId(i, 0)]).T_w_c.data(), 7);
  // ---- the C ABI on the flattened problem of the same map, the switch set by hand
  fresh();
  amd::PgoFlat f;
  amd::flatten_pose_graph(cur, cand_id, sim3, keyframes, essential, opt, f);
  vsl_ba_options o;
  o.use_huber = 1;
  o.huber_parameter = 1.0;
  o.max_num_iterations = 20;
  o.verbosity = 0;
  if (vsl_ctx_set_diagnostic(amd::ctx(), "pgo_far_edges", 1)) return 4;
  if (diag(&before_on)) return 4;
  if (vsl_pose_graph_optimize(amd::ctx(), &f.prob, &o, nullptr)) {
    std::fprintf(stderr, "C ABI: %s\n", vsl_last_error(amd::ctx()));
    return 6;
  }
  PoseGraphFarEdges drep;
  if (vsl_ctx_last_pgo_far(amd::ctx(), &drep.taken, &drep.far_edges, &drep.half_bandwidth, &drep.columns, &drep.solves)) return 4;
  for (int i = 0; i < K; i++) put(f.poses.data() + 7 * (size_t)(i == K - 1 ? 0 : f.node_of.at(FrameCamId(i, 0))), 7);
  // ---- the wrapper once more, found on: it stays on
  fresh();
  pose_graph_optimization_far_edges(cur_id, cur, cand_id, sim3, keyframes, essential, opt);
  if (diag(&after_on)) return 4;
  if (vsl_ctx_set_diagnostic(amd::ctx(), "pgo_far_edges", 0)) return 4;
  for (const PoseGraphFarEdges* r : {&rep, &drep}) {
    const double v[5] = {(double)r->taken, (double)r->far_edges, (double)r->half_bandwidth, (double)r->columns, (double)r->solves};
    put(v, 5);
  }
  const double d[4] = {(double)before_off, (double)after_off, (double)before_on, (double)after_on};
  put(d, 4);
  return 0;
}
