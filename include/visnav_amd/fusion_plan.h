// visnav_amd/fusion_plan.h -- the host half of landmark fusion (loop_closure.h landmark_fusion): turns the result of the
// guided search (vsl_fuse_search: per view, (feature, landmark index) pairs) into edits of the map.  Plain C++, no HIP,
// no device: tests/cpp/fusion_plan_test.cpp drives it on hand-written maps.
//
// The outcome is a function of the SET of pairs: they are put in (view, feature, track) order first, merge requests are
// processed in ascending (min id, max id) order, and no step walks an unordered_map.
//
// For a pair (view k, feature f, target track A):
//   f already observes A                              nothing
//   f observes nothing, A has no observation in k     (k, f) joins A.all_obs (and A.obs when camera k is active)
//   f observes nothing, A has another feature in k    skipped, counted as a conflict (a FeatureTrack holds one feature per
//                                                     camera)
//   f observes B != A                                 merge request {A, B}
// A merge folds the larger TrackId into the smallest one of its set (union-find): the survivor keeps p, p_c and
// from_fcid and receives the union of obs, all_obs and outlier_obs (an fcid now in obs leaves outlier_obs); every
// Camera::map_points entry that names the loser is re-pointed; the loser is erased.  A merge whose two sets name the same
// FrameCamId with DIFFERENT features in all_obs is refused and counted.  The covisibility containers are not touched: the
// next construct_visibility_graph sees the merged tracks.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#if __has_include(<pangolin/image/managed_image.h>) && __has_include(<visnav/common_types.h>)
#include <visnav/common_types.h>
#else
#include "mirror_types.h"
#endif

namespace visnav {

struct LandmarkFusionResult {
  int added = 0;      // observations added to an existing track
  int merged = 0;     // tracks folded into another one (= landmarks erased)
  int conflicts = 0;  // pairs skipped: the target already has another feature in that camera
  int refused = 0;    // merges refused: the two sets disagree on the feature of a camera
  // the edits themselves, in the order they were made (a caller that mirrors the map elsewhere replays them)
  std::vector<std::tuple<TrackId, FrameCamId, FeatureId>> additions;  // (track, camera, feature)
  std::vector<std::pair<TrackId, TrackId>> merges;                    // (erased track, its survivor)
};

namespace amd {

struct FusionView {
  FrameCamId fcid;
  std::vector<std::pair<FeatureId, int32_t>> pairs;  // (feature of this view, index into the landmark table)
};

// (camera, feature) -> the track that observes it
using FusionObsLookup = std::map<std::pair<FrameCamId, FeatureId>, TrackId>;

// the lookup for the given cameras, from the landmarks' all_obs; should two tracks name one feature the smaller id stays
inline FusionObsLookup fusion_obs_lookup(const Landmarks& landmarks, const std::set<FrameCamId>& views) {
  FusionObsLookup lookup;
  for (const auto& kv : landmarks)
    for (const auto& ob : kv.second.all_obs) {
      if (!views.count(ob.first)) continue;
      auto ins = lookup.emplace(std::make_pair(ob.first, ob.second), kv.first);
      if (!ins.second && kv.first < ins.first->second) ins.first->second = kv.first;
    }
  return lookup;
}

inline LandmarkFusionResult apply_fusion_plan(const std::vector<FusionView>& views, const FusionObsLookup& lookup,
                                              const std::vector<TrackId>& table, Cameras& cameras, Landmarks& landmarks) {
  LandmarkFusionResult res;
  std::set<std::tuple<FrameCamId, FeatureId, TrackId>> todo;  // the pairs as a set, in (view, feature, track) order
  for (const FusionView& v : views)
    for (const auto& p : v.pairs) {
      if (p.second < 0 || (size_t)p.second >= table.size()) continue;
      todo.emplace(v.fcid, p.first, table[(size_t)p.second]);
    }
  FusionObsLookup added;  // observations this call created
  std::set<std::pair<TrackId, TrackId>> requests;
  for (const auto& t : todo) {
    const FrameCamId& k = std::get<0>(t);
    const FeatureId f = std::get<1>(t);
    const TrackId a = std::get<2>(t);
    auto lm = landmarks.find(a);
    if (lm == landmarks.end()) continue;
    const auto key = std::make_pair(k, f);
    auto seen = lookup.find(key);
    if (seen == lookup.end()) {
      seen = added.find(key);
      if (seen == added.end()) {  // f observes nothing
        const auto has = lm->second.all_obs.find(k);
        if (has != lm->second.all_obs.end()) {
          if (has->second != f) res.conflicts++;
          continue;
        }
        lm->second.all_obs.emplace(k, f);
        const auto cam = cameras.find(k);
        if (cam != cameras.end() && cam->second.active) lm->second.obs.emplace(k, f);
        added.emplace(key, a);
        res.additions.emplace_back(a, k, f);
        res.added++;
        continue;
      }
    }
    const TrackId b = seen->second;
    if (b != a) requests.emplace(std::min(a, b), std::max(a, b));
  }

  std::map<TrackId, TrackId> parent;  // union-find; the root of a set is its smallest id
  auto find = [&](TrackId x) {
    for (auto it = parent.find(x); it != parent.end() && it->second != x; it = parent.find(x)) x = it->second;
    return x;
  };
  for (const auto& r : requests) {
    const TrackId ra = find(r.first), rb = find(r.second);
    if (ra == rb) continue;
    const TrackId s = std::min(ra, rb), l = std::max(ra, rb);
    auto ls = landmarks.find(s), ll = landmarks.find(l);
    if (ls == landmarks.end() || ll == landmarks.end()) continue;
    Landmark& keep = ls->second;
    const Landmark& gone = ll->second;
    bool clash = false;
    for (const auto& ob : gone.all_obs) {
      const auto it = keep.all_obs.find(ob.first);
      if (it != keep.all_obs.end() && it->second != ob.second) clash = true;
    }
    if (clash) {
      res.refused++;
      continue;
    }
    keep.all_obs.insert(gone.all_obs.begin(), gone.all_obs.end());
    keep.obs.insert(gone.obs.begin(), gone.obs.end());
    keep.outlier_obs.insert(gone.outlier_obs.begin(), gone.outlier_obs.end());
    for (const auto& ob : keep.obs) keep.outlier_obs.erase(ob.first);
    for (auto& cam : cameras) {
      const auto mp = cam.second.map_points.find(l);
      if (mp == cam.second.map_points.end()) continue;
      cam.second.map_points.emplace(s, mp->second);  // an entry of the survivor's stays
      cam.second.map_points.erase(l);
    }
    landmarks.erase(ll);
    parent[l] = s;
    res.merges.emplace_back(l, s);
    res.merged++;
  }
  return res;
}

}  // namespace amd
}  // namespace visnav
