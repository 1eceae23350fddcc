// Driver of include/visnav_amd/fusion_plan.h for tests/test_fusion_plan_cpu.py: reads a small map and the search
// result as text from stdin, applies the plan, prints the map in sorted order.  Plain C++: no HIP, no device.
//
//   cam  frame cam active
//   lm   tid x y z from_frame from_cam
//   obs | all | out   tid frame cam feature          (an entry of Landmark::obs / all_obs / outlier_obs)
//   mp   frame cam tid feature                       (an entry of Camera::map_points)
//   table n tid...                                   (the landmark table order of the search)
//   view frame cam n (feature index)...              (one view's pairs)
#include <visnav_amd/fusion_plan.h>

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace visnav;

static void print_track(const char* name, TrackId tid, const FeatureTrack& t) {
  std::printf("%s %lld", name, (long long)tid);
  for (const auto& ob : t) std::printf(" %lld %d %d", (long long)ob.first.frame_id, (int)ob.first.cam_id, (int)ob.second);
  std::printf("\n");
}

int main() {
  Cameras cameras;
  Landmarks landmarks;
  std::vector<TrackId> table;
  std::vector<amd::FusionView> views;
  std::string line, w;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    if (!(in >> w)) continue;
    long long a, b, c, d;
    if (w == "cam") {
      in >> a >> b >> c;
      cameras[FrameCamId(a, (CamId)b)].active = c != 0;
    } else if (w == "lm") {
      double x, y, z;
      in >> a >> x >> y >> z >> b >> c;
      Landmark& lm = landmarks[a];
      lm.p = Eigen::Vector3d(x, y, z);
      lm.p_c = Eigen::Vector3d(-x, -y, -z);
      lm.from_fcid = FrameCamId(b, (CamId)c);
    } else if (w == "obs" || w == "all" || w == "out") {
      in >> a >> b >> c >> d;
      Landmark& lm = landmarks.at(a);
      (w == "obs" ? lm.obs : w == "all" ? lm.all_obs : lm.outlier_obs)[FrameCamId(b, (CamId)c)] = (FeatureId)d;
    } else if (w == "mp") {
      in >> a >> b >> c >> d;
      cameras.at(FrameCamId(a, (CamId)b)).map_points[c] = (FeatureId)d;
    } else if (w == "table") {
      in >> a;
      for (long long i = 0; i < a; i++) {
        in >> b;
        table.push_back(b);
      }
    } else if (w == "view") {
      amd::FusionView v;
      in >> a >> b >> c;
      v.fcid = FrameCamId(a, (CamId)b);
      for (long long i = 0; i < c; i++) {
        long long f, idx;
        in >> f >> idx;
        v.pairs.emplace_back((FeatureId)f, (int32_t)idx);
      }
      views.push_back(v);
    } else {
      std::fprintf(stderr, "unknown line: %s\n", line.c_str());
      return 2;
    }
  }
  std::set<FrameCamId> view_ids;
  for (const auto& v : views) view_ids.insert(v.fcid);
  const LandmarkFusionResult r = amd::apply_fusion_plan(views, amd::fusion_obs_lookup(landmarks, view_ids), table, cameras, landmarks);
  std::printf("counts %d %d %d %d\n", r.added, r.merged, r.conflicts, r.refused);
  std::map<TrackId, const Landmark*> sorted;
  for (const auto& kv : landmarks) sorted[kv.first] = &kv.second;
  for (const auto& kv : sorted) {
    const Landmark& lm = *kv.second;
    std::printf("lm %lld %.17g %.17g %.17g %.17g %lld %d\n", (long long)kv.first, lm.p[0], lm.p[1], lm.p[2], lm.p_c[0],
                (long long)lm.from_fcid.frame_id, (int)lm.from_fcid.cam_id);
    print_track("obs", kv.first, lm.obs);
    print_track("all", kv.first, lm.all_obs);
    print_track("out", kv.first, lm.outlier_obs);
  }
  for (const auto& cam : cameras) {
    std::printf("mp %lld %d", (long long)cam.first.frame_id, (int)cam.first.cam_id);
    for (const auto& mp : cam.second.map_points) std::printf(" %lld %d", (long long)mp.first, (int)mp.second);
    std::printf("\n");
  }
  return 0;
}
