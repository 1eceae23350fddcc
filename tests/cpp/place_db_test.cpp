// The place-recognition drop-ins over both forms of the recognition database -- the host inverted file
// (DBoWInvertedFile) and the device keyframe database (KeyframeDatabaseAmd, one vsl_bowdb_query per call) -- on the
// scenario of loop_detect_test.cpp, extended: keyframes 0..9 along a path, keyframes 20..24 revisit places 3..6 with
// weak (< 30) and strong (>= 30) covisibility edges to the old keyframes, keyframes 40..45 revisit places 2, 3, 6, 7, 8
// (two stored keyframes for some places by then), and three relocalisation queries.  Prints, per keyframe,
//   <tag> kf <frame> min <min_score> cand <list> | found <0/1> enough <list> | groups <size:count ...>
// and per relocalisation query  <tag> reloc <q> found <0/1> top <list>,  with tag = host / dev.  The two transcripts
// must be identical; the exit status is 1 when they are not.
#include <cstdio>
#include <string>
#include <vector>

#include "visnav_amd/harness/odometry.h"

using namespace visnav;

static const unsigned kWords = 20000;  // recognition_database.size()

static DBoW2::BowVector place_vector(int place, int variant) {
  DBoW2::BowVector v;
  for (int w = 0; w < 10; w++) v[(unsigned)w] = 1.0;                                 // words every image has
  for (int w = 0; w < 50; w++) v[(unsigned)(100 * (place + 1) + w)] = 1.0 + 0.01 * ((w * 7 + variant) % 13);  // the place's own words
  for (int w = 0; w < 10; w++) v[(unsigned)(5000 + 50 * variant + w)] = 1.0;          // view-specific clutter
  for (int w = 0; w < 5; w++) v[(unsigned)(kWords + 100 + w)] = 0.5 + 0.1 * (variant % 3);  // beyond the inverted file: scored, not voted
  double s = 0;
  for (auto& kv : v) s += kv.second;
  for (auto& kv : v) kv.second /= s;
  return v;
}

struct Edge {
  int frame, weight;
};

static std::string list_of(const std::vector<FrameCamId>& v) {
  std::string s;
  for (const auto& f : v) s += " " + std::to_string((long long)f.frame_id);
  return s.empty() ? " -" : s;
}

template <class Database>
static std::vector<std::string> drive(Database& db) {
  std::vector<std::string> out;
  ORBVocabularyAmd voc;  // score() needs no tree
  Cameras keyframes;
  CovisibilityGraph graph;
  ConsistentGroups groups;
  std::vector<FrameCamId> enough;
  char buf[256];
  auto add = [&](int frame, int place, int variant, const std::vector<Edge>& edges_in) {
    Camera cam;
    cam.bow_vector = place_vector(place, variant);
    const FrameCamId f(frame, 0);
    std::set<FrameCamId> edges;
    for (const Edge& e : edges_in) {
      const FrameCamId p(e.frame, 0);
      cam.covisible_weights[p] = e.weight;
      edges.insert(p);
      graph[p].insert(f);
    }
    graph[f] = edges;
    const double min_score = amd::min_connected_score(cam, keyframes, &voc, db, 20);
    const std::vector<FrameCamId> cands = detect_loop_candidates(f, cam, keyframes, graph, min_score, db, &voc);
    const bool found = detect_loop_closure(f, cam, keyframes, db, &voc, graph, groups, enough, /*threshold*/ 20, /*num_consistency*/ 3);
    std::snprintf(buf, sizeof buf, "kf %d min %.17g cand", frame, min_score);
    std::string line = buf + list_of(cands) + " | found " + (found ? "1" : "0") + " enough" + list_of(enough) + " | groups";
    for (const auto& g : groups) line += " " + std::to_string(g.first.size()) + ":" + std::to_string(g.second);
    out.push_back(line);
    keyframes[f] = cam;
  };
  for (int i = 0; i < 10; i++) {  // first pass: no place is seen twice; the keyframe before the last one is weakly connected
    std::vector<Edge> e;
    if (i > 0) e.push_back({i - 1, 40});
    if (i > 1) e.push_back({i - 2, 22});
    add(i, i, i, e);
  }
  add(20, 3, 100, {{9, 40}});            // the revisit starts (covisible with its predecessor only)
  add(21, 4, 101, {{20, 40}, {4, 25}});  // weakly connected to the old keyframe of the place: it still votes
  add(22, 5, 102, {{21, 40}, {5, 35}});  // strongly connected to it: it is left out of the vote
  add(23, 6, 103, {{22, 40}, {21, 29}});
  add(24, 30, 104, {{23, 40}});          // a new place
  add(40, 2, 200, {{24, 40}});           // the second revisit: places 2, 3, 6, 7, 8 -- up to two stored keyframes per place
  add(41, 3, 201, {{40, 40}});
  add(42, 6, 202, {{41, 40}, {23, 30}});  // exactly 30: keyframe 23 is left out, keyframe 6 remains
  add(43, 7, 203, {{42, 40}});           // fourth consistent detection: 0, 1, 2, 3 >= 3
  add(44, 8, 204, {{43, 40}, {8, 29}});  // 29: the old keyframe of the place votes
  add(45, 31, 205, {{44, 40}});          // a new place again
  const DBoW2::BowVector far_words = [] {
    DBoW2::BowVector v;
    for (int w = 0; w < 20; w++) v[kWords + 100 + (unsigned)w] = 0.05;
    return v;
  }();
  const DBoW2::BowVector queries[3] = {place_vector(4, 300), place_vector(77, 301), far_words};
  for (int q = 0; q < 3; q++) {
    std::vector<FrameCamId> top;
    const bool found = harness::detect_relocalization_candidate(&voc, db, queries[q], keyframes, top);
    out.push_back("reloc " + std::to_string(q) + " found " + (found ? "1" : "0") + " top" + list_of(top));
  }
  return out;
}

int main() {
  if (!KeyframeDatabaseAmd::available()) {
    std::fprintf(stderr, "this build's C ABI has no device keyframe database\n");
    return 2;
  }
  DBoWInvertedFile inverted(kWords);
  const std::vector<std::string> host = drive(inverted);
  KeyframeDatabaseAmd device(kWords);
  const std::vector<std::string> dev = drive(device);
  for (const auto& l : host) std::printf("host %s\n", l.c_str());
  for (const auto& l : dev) std::printf("dev %s\n", l.c_str());
  std::printf("stored %zu\n", device.keyframes());
  device.release();
  amd::release_thread_ctx();
  return host == dev ? 0 : 1;
}
