// The batched compute_bow_vector overloads of include/visnav_amd/bow.h (frame-store range -> std::vector<BowVector> /
// FeatureVector, and the overload that appends to KeyframeDatabaseAmd) against the single-image compute_bow_vector +
// KeyframeDatabaseAmd::insert they batch.  argv[1] = a vocabulary file.  Prints one line per check and "ok" at the end.
#include <cstdio>
#include <cstring>
#include <vector>

#include "visnav_amd/bow.h"

using namespace visnav;

namespace {
constexpr int W = 161, H = 123, N = 5, NF = 300;

void fill(uint8_t* px, int kind) {  // 6 x 6 blocks of pseudo-random grey; kind 3 is flat (no features at all)
  uint32_t s = 12345u + 977u * (uint32_t)kind;
  uint8_t block[(H / 6 + 1) * (W / 6 + 1)];
  for (auto& b : block) {
    s = s * 1664525u + 1013904223u;
    b = (uint8_t)(s >> 24);
  }
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) px[y * W + x] = kind == 3 ? 90 : block[(y / 6) * (W / 6 + 1) + x / 6];
}

bool same_bits(const DBoW2::BowVector& a, const DBoW2::BowVector& b) {
  if (a.size() != b.size()) return false;
  auto ia = a.begin();
  auto ib = b.begin();
  for (; ia != a.end(); ++ia, ++ib)
    if (ia->first != ib->first || std::memcmp(&ia->second, &ib->second, 8) != 0) return false;
  return true;
}

bool same_survivors(const KeyframeDatabaseAmd::Survivors& a, const KeyframeDatabaseAmd::Survivors& b) {
  return a.fcids == b.fcids && a.counts == b.counts && a.n_sharing == b.n_sharing && a.max_count == b.max_count &&
         a.scores.size() == b.scores.size() && std::memcmp(a.scores.data(), b.scores.data(), 8 * a.scores.size()) == 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!frames_bow_available() || !KeyframeDatabaseAmd::available()) {
    std::printf("the library has no vsl_frames_bow_vectors\n");
    return 3;
  }
  ORBVocabularyAmd voc;
  if (!voc.loadFromTextFile(argv[1])) return 2;
  std::vector<uint8_t> px((size_t)N * W * H);
  for (int i = 0; i < N; i++) fill(&px[(size_t)i * W * H], i);
  vsl_frames* frames = nullptr;
  amd::check(vsl_frames_create(amd::ctx(), N, W, H, 64, 1, &frames), "vsl_frames_create");
  amd::check(vsl_frames_upload(amd::ctx(), frames, 0, N, px.data(), W, (size_t)W * H), "vsl_frames_upload");
  amd::check(vsl_ctx_synchronize(amd::ctx()), "vsl_ctx_synchronize");

  // the single-image way: one call and one insert per keyframe
  std::vector<DBoW2::BowVector> v1(N);
  std::vector<DBoW2::FeatureVector> f1(N);
  std::vector<FrameCamId> fcids;
  KeyframeDatabaseAmd one(voc.size()), batch(voc.size());
  for (int i = 0; i < N; i++) {
    pangolin::ManagedImage<uint8_t> img(W, H);
    std::memcpy(img.ptr, &px[(size_t)i * W * H], (size_t)W * H);
    compute_bow_vector(img, NF, &voc, v1[i], f1[i]);
    fcids.emplace_back(10 * i, 0);
    one.insert(fcids.back(), v1[i]);
  }
  int with_words = 0;
  for (int i = 0; i < N; i++) with_words += !v1[i].empty();
  std::printf("single: %d of %d images have words, image 3 has %zu\n", with_words, N, v1[3].size());
  if (with_words != N - 1 || !v1[3].empty()) return 1;

  // the batched overload: a sub-range, then the whole store
  std::vector<DBoW2::BowVector> v2;
  std::vector<DBoW2::FeatureVector> f2;
  compute_bow_vector(frames, 1, 3, NF, &voc, v2, f2);
  bool ok = v2.size() == 3 && f2.size() == 3;
  for (int i = 0; ok && i < 3; i++) ok = same_bits(v2[i], v1[1 + i]) && f2[i] == f1[1 + i];
  std::printf("range [1, 4): %s\n", ok ? "same" : "DIFFERENT");
  if (!ok) return 1;
  compute_bow_vector(frames, 0, NF, &voc, batch, fcids, v2, f2);
  ok = v2.size() == (size_t)N && batch.keyframes() == (size_t)N;
  for (int i = 0; ok && i < N; i++) ok = same_bits(v2[i], v1[i]) && f2[i] == f1[i] && batch.contains(fcids[i]);
  std::printf("whole store into the database: %s\n", ok ? "same" : "DIFFERENT");
  if (!ok) return 1;

  // the two databases answer alike
  for (int i = 0; i < N; i++) {
    if (v1[i].empty()) continue;
    const bool q = same_survivors(one.query_reloc(v1[i]), batch.query_reloc(v1[i])) &&
                   same_survivors(one.query_loop(v1[i], {fcids[i]}), batch.query_loop(v1[i], {fcids[i]}));
    const std::vector<double> sa = one.score(v1[i], fcids), sb = batch.score(v1[i], fcids);
    ok = ok && q && std::memcmp(sa.data(), sb.data(), 8 * sa.size()) == 0 && one.query_reloc(v1[i]).fcids.size() > 0;
  }
  std::printf("queries and scores: %s\n", ok ? "same" : "DIFFERENT");
  vsl_frames_destroy(frames);
  if (!ok) return 1;
  std::printf("ok\n");
  return 0;
}
