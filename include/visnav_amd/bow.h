// visnav_amd/bow.h -- drop-in for the DBoW2 calls the reference makes when scoring loop-closure
// candidates: ORBVocabulary::loadFromTextFile / transform / score
// (thirdparty/DBoW2_ORBSLAM/DBoW2/TemplatedVocabulary.h:1338, :1127, :1199; call sites
// include/visnav/keypoints.h:253, include/visnav/loop_closure_utils.h:119, :201, include/visnav/tracking.h:208).
// BowVector / FeatureVector keep DBoW2's container types (std::map), so the callers' code that walks
// them (inverted file at loop_closure_utils.h:156) is unchanged.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "dbow2_types.h"
#include "keypoints.h"

// The device keyframe database (KeyframeDatabaseAmd below) is referenced weakly: the CPU-baseline build of the
// application links a C ABI without the vsl_bowdb_* entries (oracle/Makefile cpu_baseline) and refuses the option there.
#pragma weak vsl_bowdb_create
#pragma weak vsl_bowdb_destroy
#pragma weak vsl_bowdb_append
#pragma weak vsl_bowdb_score
#pragma weak vsl_bowdb_query
// ... and so are the batched keyframe BoW on the frame store and the reserve its device append needs: the headers
// still link against a library from before them, and frames_bow_available() tells
#pragma weak vsl_frames_bow_vectors
#pragma weak vsl_bowdb_reserve
#pragma weak vsl_bowdb_info

namespace visnav {

inline bool frames_bow_available() {
  return &vsl_frames_bow_vectors != nullptr && &vsl_bowdb_reserve != nullptr && &vsl_bowdb_info != nullptr;
}

class ORBVocabularyAmd {
 public:
  ORBVocabularyAmd() = default;
  ORBVocabularyAmd(const ORBVocabularyAmd&) = delete;
  ~ORBVocabularyAmd() { vsl_voc_destroy(voc_); }

  // TemplatedVocabulary.h:1338: returns false on failure like the original
  bool loadFromTextFile(const std::string& filename) {
    vsl_voc_destroy(voc_);
    voc_ = nullptr;
    return vsl_voc_load_text(amd::ctx(), filename.c_str(), &voc_) == VSL_OK;
  }
  unsigned int size() const {
    int w = 0;
    if (voc_) vsl_voc_info(voc_, nullptr, nullptr, nullptr, &w);
    return (unsigned)w;
  }
  bool empty() const { return size() == 0; }

  // transform(features, v, fv, levelsup): features are 32-byte rows in cv::Mat / DBoW2 byte order.
  void transform(const std::vector<const uint8_t*>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv,
                 int levelsup) const {
    std::vector<uint8_t> flat(32 * features.size());
    for (size_t i = 0; i < features.size(); i++) std::memcpy(&flat[32 * i], features[i], 32);
    transform(flat.data(), (int)features.size(), v, fv, levelsup);
  }
  void transform(const uint8_t* desc32, int n, DBoW2::BowVector& v, DBoW2::FeatureVector& fv, int levelsup) const {
    v.clear();
    fv.clear();
    if (!voc_ || n <= 0) return;
    std::vector<uint32_t> ids(n), fn(n), ff(n);
    std::vector<double> vals(n);
    int nnz = 0, fvn = 0;
    amd::check(vsl_bow_transform(amd::ctx(), voc_, desc32, n, levelsup, ids.data(), vals.data(), &nnz, fn.data(),
                                 ff.data(), &fvn), "ORBVocabulary::transform");
    for (int i = 0; i < nnz; i++) v.emplace_hint(v.end(), ids[i], vals[i]);
    for (int i = 0; i < fvn; i++) fv[fn[i]].push_back(ff[i]);
  }
  // descriptors straight from KeypointsData (bitset<256>), converted with converter.h's bit order
  void transform(const std::vector<std::bitset<256>>& desc, DBoW2::BowVector& v, DBoW2::FeatureVector& fv,
                 int levelsup) const {
    std::vector<uint8_t> flat(32 * desc.size());
    vsl_desc_bitset_to_bytes(reinterpret_cast<const uint64_t*>(desc.data()), (int)desc.size(), flat.data());
    transform(flat.data(), (int)desc.size(), v, fv, levelsup);
  }

  // compute_bow_vector of include/visnav/keypoints.h:243-254 in one device pass: the ORB front end
  // (cv::ORB::create(num_features, 1.2, 8, 19, 0, 2, FAST_SCORE)->detectAndCompute, restated -- see
  // oracle/orc_orb.cpp for the arithmetic conventions) followed by transform(..., levelsup = 4)
  void compute_bow_vector(const pangolin::ManagedImage<uint8_t>& img_raw, int num_features, DBoW2::BowVector& v,
                          DBoW2::FeatureVector& fv, int levelsup = 4) const {
    v.clear();
    fv.clear();
    if (!voc_) return;
    int cap = 2 * num_features + 512;
    std::vector<uint32_t> ids(cap), fn(cap), ff(cap);
    std::vector<double> vals(cap);
    int nnz = 0, fvn = 0;
    int rc = vsl_compute_bow_vector(amd::ctx(), voc_, img_raw.ptr, (int)img_raw.w, (int)img_raw.h, img_raw.pitch, num_features,
                                    levelsup, cap, ids.data(), vals.data(), &nnz, fn.data(), ff.data(), &fvn);
    if (rc == VSL_ERR_CAPACITY && fvn > cap) {  // retainBest keeps every tie: once more with the reported feature count
      cap = fvn;
      ids.resize(cap), fn.resize(cap), ff.resize(cap), vals.resize(cap);
      rc = vsl_compute_bow_vector(amd::ctx(), voc_, img_raw.ptr, (int)img_raw.w, (int)img_raw.h, img_raw.pitch, num_features,
                                  levelsup, cap, ids.data(), vals.data(), &nnz, fn.data(), ff.data(), &fvn);
    }
    amd::check(rc, "compute_bow_vector");
    for (int i = 0; i < nnz; i++) v.emplace_hint(v.end(), ids[i], vals[i]);
    for (int i = 0; i < fvn; i++) fv[fn[i]].push_back(ff[i]);
  }

  // compute_bow_vector for the images in slots [first, first + n) of a frame store in one batched device pass
  // (vsl_frames_bow_vectors): v[i] / fv[i] are what the single-image call gives for the image in slot first + i.  With
  // db the vectors are also appended to that device database, in slot order, without coming through the host;
  // db_index[i] = the index of vector i there.  The database must have room (vsl_bowdb_reserve).
  void compute_bow_vectors(vsl_frames* frames, int first, int n, int num_features, std::vector<DBoW2::BowVector>& v,
                           std::vector<DBoW2::FeatureVector>& fv, int levelsup = 4, vsl_bowdb* db = nullptr,
                           int32_t* db_index = nullptr) const {
    v.assign((size_t)(n > 0 ? n : 0), DBoW2::BowVector());
    fv.assign((size_t)(n > 0 ? n : 0), DBoW2::FeatureVector());
    if (!voc_ || n <= 0) return;
    if (!frames_bow_available()) amd::check(VSL_ERR_INVALID, "compute_bow_vectors: this libvslam_hip.so has no vsl_frames_bow_vectors");
    size_t cap = 2 * (size_t)num_features + 512;
    std::vector<uint32_t> ids, fn, ff;
    std::vector<double> vals;
    std::vector<int32_t> nnz((size_t)n), fvn((size_t)n), nfeat((size_t)n);
    int rc = VSL_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
      ids.resize(cap * n), fn.resize(cap * n), ff.resize(cap * n), vals.resize(cap * n);
      rc = vsl_frames_bow_vectors(amd::ctx(), frames, first, n, voc_, num_features, levelsup, db, db_index, (int)cap, ids.data(),
                                  vals.data(), nnz.data(), fn.data(), ff.data(), fvn.data(), nfeat.data());
      size_t need = 0;
      for (int32_t c : nfeat) need = std::max(need, (size_t)(c > 0 ? c : 0));
      if (rc != VSL_ERR_CAPACITY || need <= cap) break;  // retainBest keeps every tie: once more with the reported counts
      cap = need;                                         // (on the error nothing was appended to db)
    }
    amd::check(rc, "compute_bow_vectors");
    for (int i = 0; i < n; i++) {
      const size_t o = cap * (size_t)i;
      for (int j = 0; j < nnz[(size_t)i]; j++) v[(size_t)i].emplace_hint(v[(size_t)i].end(), ids[o + j], vals[o + j]);
      for (int j = 0; j < fvn[(size_t)i]; j++) fv[(size_t)i][fn[o + j]].push_back(ff[o + j]);
    }
  }
  const vsl_voc* handle() const { return voc_; }

  // TemplatedVocabulary.h:1199-1203
  double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const {
    std::vector<const DBoW2::BowVector*> one(1, &b);
    return score_batch(a, one)[0];
  }
  // one query against many candidates in ONE launch (what detect_loop_candidates does in a loop,
  // include/visnav/loop_closure_utils.h:199-211)
  std::vector<double> score_batch(const DBoW2::BowVector& q, const std::vector<const DBoW2::BowVector*>& cands) const {
    std::vector<uint32_t> qi, ci;
    std::vector<double> qv, cv;
    std::vector<int32_t> off(1, 0);
    for (const auto& kv : q) { qi.push_back(kv.first); qv.push_back(kv.second); }
    for (const auto* c : cands) {
      for (const auto& kv : *c) { ci.push_back(kv.first); cv.push_back(kv.second); }
      off.push_back((int32_t)ci.size());
    }
    std::vector<double> s(cands.size(), 0.0);
    if (cands.empty()) return s;
    amd::check(vsl_bow_score_batch(amd::ctx(), qi.data(), qv.data(), (int)qi.size(), ci.data(), cv.data(), off.data(),
                                   (int)cands.size(), s.data()), "ORBVocabulary::score");
    return s;
  }

 private:
  vsl_voc* voc_ = nullptr;
};

// The recognition database on the device: what the reference keeps as an inverted file (DBoWInvertedFile, one list of
// keyframes per vocabulary word, src/slam.cpp:380) plus the keyframes' BowVectors, as ONE device store of vectors
// (vsl_bowdb).  The walk of the inverted file, the 0.8 rule and the scores of the survivors are one vsl_bowdb_query;
// index <-> FrameCamId in insertion order, which is the order of every inverted-file list.  Like the inverted file,
// nothing is ever removed.
class KeyframeDatabaseAmd {
 public:
  struct Survivors {  // the keyframes above the 0.8 rule, in the order the reference's walk first meets them
    std::vector<FrameCamId> fcids;
    std::vector<int> counts;      // num_sharing_words (the first shared word counts 0)
    std::vector<double> scores;   // voc->score(query, keyframe)
    int n_sharing = 0;            // num_sharing_words.size()
    int max_count = 0;            // max_num_sharing_words
  };
  // n_words = recognition_database.size(): query words at or above it are skipped by the vote
  explicit KeyframeDatabaseAmd(unsigned n_words = 0) : n_words_(n_words) {}
  KeyframeDatabaseAmd(const KeyframeDatabaseAmd&) = delete;
  KeyframeDatabaseAmd& operator=(const KeyframeDatabaseAmd&) = delete;
  ~KeyframeDatabaseAmd() { release(); }
  static bool available() {
    return &vsl_bowdb_create != nullptr && &vsl_bowdb_destroy != nullptr && &vsl_bowdb_append != nullptr &&
           &vsl_bowdb_score != nullptr && &vsl_bowdb_query != nullptr;
  }
  void release() {
    if (db_) vsl_bowdb_destroy(db_);
    db_ = nullptr;
    fcids_.clear();
    index_.clear();
  }
  void resize(unsigned n_words) { n_words_ = n_words; }  // recognition_database.resize(voc->size())
  unsigned size() const { return n_words_; }
  size_t keyframes() const { return fcids_.size(); }
  bool contains(const FrameCamId& f) const { return index_.count(f) != 0; }

  // insert_new_kf_to_db: the keyframe's vector is uploaded once
  void insert(const FrameCamId& fcid, const DBoW2::BowVector& v) {
    if (index_.count(fcid)) return;  // insert_from_frames already appended this keyframe's vector on the device
    if (!db_) amd::check(vsl_bowdb_create(amd::ctx(), 1 << 20, 1024, &db_), "KeyframeDatabaseAmd");
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(v, ids, vals);
    int idx = -1;
    amd::check(vsl_bowdb_append(amd::ctx(), db_, ids.data(), vals.data(), (int)ids.size(), &idx), "KeyframeDatabaseAmd::insert");
    fcids_.push_back(fcid);
    index_[fcid] = idx;  // a keyframe is inserted once, when it is taken (src/slam.cpp:1219-1258)
  }
  // insert_new_kf_to_db for keyframes whose images lie in slots [first, first + n) of a frame store: their BowVectors
  // are computed by the batched call and appended on the device (fcids[i] <-> slot first + i); v / fv receive them for
  // the callers that keep them per keyframe.  Same stored vectors, same indices as n compute_bow_vector + insert calls.
  void insert_from_frames(const std::vector<FrameCamId>& fcids, const ORBVocabularyAmd& voc, vsl_frames* frames, int first,
                          int num_features, std::vector<DBoW2::BowVector>& v, std::vector<DBoW2::FeatureVector>& fv,
                          int levelsup = 4) {
    const int n = (int)fcids.size();
    if (n == 0) return;
    if (!db_) amd::check(vsl_bowdb_create(amd::ctx(), 1 << 20, 1024, &db_), "KeyframeDatabaseAmd");
    if (!frames_bow_available()) amd::check(VSL_ERR_INVALID, "KeyframeDatabaseAmd::insert_from_frames: this libvslam_hip.so has no vsl_frames_bow_vectors");
    // the device append does not grow the database: room for the most these keyframes can bring (vsl_bowdb_reserve
    // does nothing while there is room and grows geometrically otherwise).  Features beyond the usual bound --
    // unbounded ties -- come back as a capacity error of the call.
    int stored = 0;
    int64_t entries = 0;
    amd::check(vsl_bowdb_info(db_, &stored, &entries), "vsl_bowdb_info");
    amd::check(vsl_bowdb_reserve(amd::ctx(), db_, entries + (int64_t)n * (2 * (int64_t)num_features + 512), stored + n), "vsl_bowdb_reserve");
    std::vector<int32_t> idx((size_t)n, -1);
    voc.compute_bow_vectors(frames, first, n, num_features, v, fv, levelsup, db_, idx.data());
    for (int i = 0; i < n; i++) {
      fcids_.push_back(fcids[(size_t)i]);
      index_[fcids[(size_t)i]] = idx[(size_t)i];
    }
  }
  // detect_loop_candidates' vote: `excluded` = the connected keyframes with covisible weight >= 30
  // (a keyframe that insert_from_frames stored before its own query is passed in `excluded` by the caller)
  Survivors query_loop(const DBoW2::BowVector& q, const std::vector<FrameCamId>& excluded) const {
    std::vector<int32_t> ex;
    for (const auto& f : excluded) {
      auto it = index_.find(f);
      if (it != index_.end()) ex.push_back(it->second);
    }
    return query(q, ex);
  }
  // detect_relocalization_candidate's vote: every stored keyframe takes part
  Survivors query_reloc(const DBoW2::BowVector& q) const { return query(q, {}); }
  // voc->score(q, keyframe) for stored keyframes, by index: no stored vector is uploaded again
  std::vector<double> score(const DBoW2::BowVector& q, const std::vector<FrameCamId>& fcids) const {
    std::vector<double> s(fcids.size(), 0.0);
    if (fcids.empty()) return s;
    std::vector<int32_t> idx;
    for (const auto& f : fcids) idx.push_back(index_.at(f));
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(q, ids, vals);
    amd::check(vsl_bowdb_score(amd::ctx(), db_, ids.data(), vals.data(), (int)ids.size(), idx.data(), (int)idx.size(), s.data()),
               "KeyframeDatabaseAmd::score");
    return s;
  }

 private:
  static void flatten(const DBoW2::BowVector& v, std::vector<uint32_t>& ids, std::vector<double>& vals) {
    for (const auto& kv : v) {
      ids.push_back(kv.first);
      vals.push_back(kv.second);
    }
  }
  Survivors query(const DBoW2::BowVector& q, const std::vector<int32_t>& ex) const {
    Survivors out;
    if (!db_) return out;
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(q, ids, vals);
    const int cap = (int)fcids_.size();
    std::vector<int32_t> idx(cap), cnt(cap);
    out.scores.resize(cap);
    int n = 0;
    amd::check(vsl_bowdb_query(amd::ctx(), db_, ids.data(), vals.data(), (int)ids.size(), n_words_, ex.data(), (int)ex.size(), 0.8f, cap,
                               idx.data(), cnt.data(), out.scores.data(), &n, &out.n_sharing, &out.max_count),
               "KeyframeDatabaseAmd::query");
    out.scores.resize(n);
    for (int i = 0; i < n; i++) {
      out.fcids.push_back(fcids_[(size_t)idx[i]]);
      out.counts.push_back(cnt[i]);
    }
    return out;
  }
  vsl_bowdb* db_ = nullptr;
  unsigned n_words_ = 0;
  std::vector<FrameCamId> fcids_;
  std::map<FrameCamId, int> index_;
};

// include/visnav/keypoints.h:243-254 with the reference's argument order; the cv::Ptr<cv::ORB> argument of the
// reference is re-created inside it on every call with fixed parameters, so it carries no state and is dropped.
inline void compute_bow_vector(const pangolin::ManagedImage<uint8_t>& img_raw, int num_features, const ORBVocabularyAmd* voc,
                               DBoW2::BowVector& bow_vector, DBoW2::FeatureVector& feature_vector) {
  voc->compute_bow_vector(img_raw, num_features, bow_vector, feature_vector, 4);
}

// The same for the images in slots [first, first + n) of a frame store, in one batched device pass ...
inline void compute_bow_vector(vsl_frames* frames, int first, int n, int num_features, const ORBVocabularyAmd* voc,
                               std::vector<DBoW2::BowVector>& bow_vectors, std::vector<DBoW2::FeatureVector>& feature_vectors) {
  voc->compute_bow_vectors(frames, first, n, num_features, bow_vectors, feature_vectors, 4);
}
// ... which also appends them to the device keyframe database as keyframes fcids[0 .. n)
inline void compute_bow_vector(vsl_frames* frames, int first, int num_features, const ORBVocabularyAmd* voc,
                               KeyframeDatabaseAmd& db, const std::vector<FrameCamId>& fcids,
                               std::vector<DBoW2::BowVector>& bow_vectors, std::vector<DBoW2::FeatureVector>& feature_vectors) {
  db.insert_from_frames(fcids, *voc, frames, first, num_features, bow_vectors, feature_vectors, 4);
}

}  // namespace visnav
