// Place recognition, one query: the host inverted-file walk + score_batch of the survivors
// (detect_relocalization_candidate over DBoWInvertedFile) next to the device keyframe database (the same function over
// KeyframeDatabaseAmd: one vsl_bowdb_query), in one process, at N stored keyframes of ~1500 words over the 1,000,000
// words of the k = 10, L = 6 tree shape.  Keyframes come in places of 10 views that share 400 words, so a query has a
// handful of survivors like a revisit has.  Wall time per query (host arrays in, candidate list out), median of 30.
//   g++ -O2 -std=c++17 -I include tools/place_db_probe.cpp -o place_db_probe -L visual-slam_amd -lvslam_hip
//       -Wl,-rpath,$PWD/visual-slam_amd   (one line)
//   ./place_db_probe [N ...]        (default 100 1000 10000)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "visnav_amd/harness/odometry.h"

using namespace visnav;

static const unsigned kWords = 1000000;

static DBoW2::BowVector view_of(const std::vector<unsigned>& place_words, std::mt19937& rng) {
  DBoW2::BowVector v;
  for (unsigned w : place_words) v[w] = 1.0 + 0.001 * (rng() % 100);
  while (v.size() < 1500) v[rng() % kWords] = 1.0 + 0.001 * (rng() % 100);
  double s = 0;
  for (auto& kv : v) s += kv.second;
  for (auto& kv : v) kv.second /= s;
  return v;
}

template <class F>
static double median_us(F&& f, int reps = 30) {
  std::vector<double> t;
  for (int i = 0; i < reps + 3; i++) {
    const auto a = std::chrono::steady_clock::now();
    f();
    const auto b = std::chrono::steady_clock::now();
    if (i >= 3) t.push_back(std::chrono::duration<double, std::micro>(b - a).count());
  }
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

int main(int argc, char** argv) {
  std::vector<int> sizes;
  for (int i = 1; i < argc; i++) sizes.push_back(std::atoi(argv[i]));
  if (sizes.empty()) sizes = {100, 1000, 10000};
  ORBVocabularyAmd voc;  // score() needs no tree
  for (int N : sizes) {
    std::mt19937 rng(7);
    Cameras keyframes;
    DBoWInvertedFile inverted(kWords);
    KeyframeDatabaseAmd device(kWords);
    std::vector<unsigned> place;
    for (int i = 0; i < N; i++) {
      if (i % 10 == 0) {
        place.clear();
        for (int w = 0; w < 400; w++) place.push_back(rng() % kWords);
      }
      Camera cam;
      cam.bow_vector = view_of(place, rng);
      const FrameCamId f(i, 0);
      insert_new_kf_to_db(f, cam, inverted);
      insert_new_kf_to_db(f, cam, device);
      keyframes[f] = cam;
    }
    const DBoW2::BowVector q = view_of(place, rng);  // a new view of the last place
    std::vector<FrameCamId> top_host, top_dev;
    const double host_us = median_us([&] {
      top_host.clear();
      harness::detect_relocalization_candidate(&voc, inverted, q, keyframes, top_host);
    });
    const double dev_us = median_us([&] {
      top_dev.clear();
      harness::detect_relocalization_candidate(&voc, device, q, keyframes, top_dev);
    });
    const KeyframeDatabaseAmd::Survivors sv = device.query_reloc(q);
    std::printf("{\"stored\": %d, \"host_walk_plus_score_batch_us\": %.1f, \"device_query_us\": %.1f, \"survivors\": %zu, \"sharing\": %d, "
                "\"same_candidates\": %s}\n",
                N, host_us, dev_us, sv.fcids.size(), sv.n_sharing, top_host == top_dev ? "true" : "false");
    std::fflush(stdout);
  }
  amd::release_thread_ctx();
  return 0;
}
