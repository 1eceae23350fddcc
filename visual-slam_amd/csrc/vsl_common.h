// vsl_common.h -- internal definitions shared by the HIP translation units of libvslam_hip.so.
// Written for gfx950 (MI355X) only: 64-lane wavefronts are assumed everywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vslam_hip.h"
#include "chol_plan.h"  // VSL_CHOL_NB, BCR_MAXB, chol_choose / chol_ring_available, the plans of the SPD solvers (chol.hip)

#define VSL_WAVE 64
#define VSL_META_STRIDE 32  // ints: 128 bytes per image
#define VSL_META_MAX 0      // order-preserving int encoding of the fp32 response maximum
#define VSL_META_NCAND 1    // number of corner candidates
#define VSL_META_NEXACT 3   // rBRIEF bits whose rotated coordinates need the exact (integer) rounding
// MAX / NCAND / NEXACT are consumed and reset by the kernel that reads them (selection, exact bits), so a
// detect / describe call needs no separate clearing launch; the last values stay readable here:
#define VSL_META_NCAND_LAST 4
#define VSL_META_NEXACT_LAST 5
#define VSL_META_MAX_LAST 6
#define VSL_EXACT_CAP 16384 // capacity of that per-image list
#ifndef VSL_TILE_LX
#define VSL_TILE_LX 7  // log2 width / height of the keypoint tiles of the batched describe kernel (describe.hip)
#endif
#ifndef VSL_TILE_LY
#define VSL_TILE_LY 7
#endif
#define VSL_TIE_OVERFLOW_FLAG 0x40000000u  // set in tie_count by exact_bits_kernel when an image's list overflowed

// wall clock in milliseconds (host timings of the summaries and traces)
inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct vsl_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  char err[512] = {0};
  // per-stage profiling
  bool profiling = false;
  struct StageEv {
    hipEvent_t a, b;
    int stage;
  };
  std::vector<StageEv> pending;
  std::vector<hipEvent_t> ev_pool;
  double stage_ms[VSL_STAGE_COUNT] = {0};
  int64_t stage_launches[VSL_STAGE_COUNT] = {0};
  // scratch frame store used by the host-buffer entry points (lazily created)
  struct vsl_frames* scratch = nullptr;
  int scratch_w = 0, scratch_h = 0, scratch_feat = 0;
  // generic device / pinned scratch
  void* dscratch = nullptr;
  size_t dscratch_cap = 0;
  void* hpinned = nullptr;
  size_t hpinned_cap = 0;
  // plan of the block-cyclic-reduction solver (chol.hip) and its job lists on the device, kept while (n, bandwidth, form) stay the same
  BcrPlanCache bcr;
  // branch of the last SPD solve (chol.hip; read-out: vsl_ctx_last_spd_path): VSL_SPD_PATH_*, and for the cyclic
  // reductions the block size, block count and level count
  int last_spd_path = 0, last_spd_block = 0, last_spd_nblk = 0, last_spd_levels = 0;
  // device arena lent to vsl_bundle_adjust calls on this context (one allocation reused across solves)
  void* ba_arena = nullptr;
  size_t ba_arena_cap = 0;
  bool ba_arena_busy = false;
  // pinned, device-mapped mailbox of the fused local-BA iteration (ba_fused.hip): kernels post their scalars there
  int64_t last_ba_s_elems = 0;  // layout of the reduced camera system of the last general-path solve set up on this context
  int last_ba_banded = 0, last_ba_bw = 0;
  // matrix-free PCG of the last general-path solve on this context (vsl_ctx_last_ba_pcg): solves, iterations in all of
  // them and in the last one, the last one's ||r|| / ||b||
  int64_t last_pcg_solves = 0, last_pcg_iterations = 0;
  int last_pcg_iterations_last = 0;
  double last_pcg_rel_residual = 0.0;
  void* ba_pin = nullptr;   // [plan of the solve | mailbox]: one copy carries the plan to the device
  size_t ba_pin_cap = 0;    // bytes
  bool select_attr_set = false;
  bool bow_score_attr_set = false;  // per context, hence per device: hipFuncSetAttribute is a per-device setting
  bool bow_query_attr_set = false;  // the same for the place-recognition query kernel
  double* status_word = nullptr;    // 64 device bytes allocated with the context: the flag of status exchanges between ranks (never null in a live context)
  double tie_eps = 1e-12;  // rBRIEF near-tie guard band (describe.hip)
  bool match_use_i8 = false;            // diagnostic: int8 matrix-core matcher even where the FP4 one applies (<= 2048 features)
  bool match_no_stagger = false;        // diagnostic: all waves of a matcher workgroup in the same phase order (the pre-stagger kernel)
  bool match_two_pass = false;          // diagnostic: forward + reverse passes of the FP4 matcher even for launches of fewer than 8 pairs (which default to one launch with both full directions)
  bool match_use_valu = false;          // diagnostic: VALU popcount matcher instead of the MFMA one
  bool force_generic_describe = false;  // diagnostic: use the f64 kernel for every describe call
  int select_bucket_cap = 128;          // diagnostic: fullest response bin the counting sort of the selection kernel accepts (0: always the bitonic network)
  bool chol_no_bcr = false;             // diagnostic: long narrow bands by the (two-ended) band Cholesky instead of block cyclic reduction
  bool chol_one_ended = false;          // diagnostic: narrow-band Cholesky by one workgroup from the top only (no two-ended split)
  bool chol_no_fused = false;           // diagnostic: band Cholesky as one launch per panel step instead of the fused single-launch kernel
  bool ba_force_dense = false;          // diagnostic: dense reduced camera system even where the band form applies
  bool pgo_cov_no_band_read = false;    // diagnostic: vsl_pgo_joint_covariance / vsl_pgo_edge_consistency solve unit columns for in-band pairs too instead of reading the band of the inverse
  bool ba_cov_no_band_read = false;     // diagnostic: the same for vsl_global_ba_relative_pose_covariance on its band route
  bool pgo_far_edges = false;           // diagnostic / VSL_PGO_FAR_EDGES: pose graphs that would be stored densely because of a few long edges by a band factor plus a low-rank update (pgo.hip "FAR EDGES")
  // that route in the last pose-graph solve on this context (vsl_ctx_last_pgo_far): taken, far edges, half bandwidth of
  // the near band, right-hand-side columns per solve, solves
  int last_pgo_far_taken = 0, last_pgo_far_k = 0, last_pgo_far_bw = 0, last_pgo_far_cols = 0;
  int64_t last_pgo_far_solves = 0;
  bool ba_schur_atomics = false;       // diagnostic: large-system Schur complement by fp64 atomics (one wavefront per landmark) instead of the per-block gather
  bool ba_no_fused = false;             // diagnostic: local windows by the operator-by-operator kernels of ba.hip instead of the fused iteration (ba_fused.hip)
  bool ba_schur_entries = false;        // diagnostic: single-entry ownership in the small-system Schur kernel instead of 3 x 3 sub-blocks
  int describe_tile_min_images = 96;   // describe launches of at least this many images use the shared-tile kernel (measured break-even ~64 images; diagnostic: 1 forces it, 0 disables it)
  bool ba_iterative_schur = false;      // diagnostic / VSL_BA_ITERATIVE: large maps by the matrix-free PCG on the reduced camera system (ba_pcg.h) instead of forming and factorising S
  int ba_pcg_poll = 0;                  // diagnostic: PCG iterations enqueued between two reads of the solve's record (0: 8)
  int ba_pcg_tol_exp = 0;               // diagnostic: the solver loop's PCG stops at ||r|| <= 10^-e ||b|| (0: the forcing term 0.1)
  bool ba_no_cyclic = false;            // diagnostic: large reduced camera systems in the linear band form (reverse Cuthill-McKee order) even when the cyclic form is narrower
  bool ba_host_lm = false;              // diagnostic: the fused local iteration with the Levenberg-Marquardt decision on the HOST (one synchronisation per iteration) instead of on the device (ba_fused.hip baf_decide_kernel)
  bool bow_no_wg_score = false;         // diagnostic: wave-per-candidate scoring kernel also for few candidates
  bool bow_keys64 = false;              // diagnostic: 64-bit sort keys in the BowVector assembly even where (id, feature) fits 32 bits
  int vo_chain_ticket = 0;              // diagnostic: vsl_map_track draws chain positions from the atomic ticket at every map size
  int pending_desc_max = 64;            // unresolved describe launches a frame store queues before it settles them itself (diagnostic: tests lower it)
  int exact_list_cap = VSL_EXACT_CAP;   // diagnostic: per-image exact-rounding list entries the describe kernels use (tests shrink it to hit the overflow fallback)
  int frames_bow_chunk = 0;             // diagnostic: images per pass of vsl_frames_bow_vectors (0: as many as the scratch budget holds)
  int k1_list_cap = -1;                // diagnostic: per-wave LDS candidate slots in K1 (tests shrink it to hit the overflow path)
};

int vsl_fail(vsl_ctx* ctx, int code, const char* fmt, ...);

// ba_fused.hip: the local-window LM loop in four launches per iteration; *handled = 0 when the problem does not fit it
int vsl_ba_fused_solve(vsl_ctx* ctx, const vsl_ba_problem* prob, const vsl_ba_options* opt, vsl_ba_summary* summary, int* handled);

#define VSL_HIP(ctx, call)                                                                        \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return vsl_fail((ctx), VSL_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,            \
                      hipGetErrorString(e_));                                                     \
  } while (0)

#define VSL_CHECK_LAUNCH(ctx)                                                                     \
  do {                                                                                            \
    hipError_t e_ = hipGetLastError();                                                            \
    if (e_ != hipSuccess)                                                                         \
      return vsl_fail((ctx), VSL_ERR_HIP, "%s:%d kernel launch -> %s", __FILE__, __LINE__,        \
                      hipGetErrorString(e_));                                                     \
  } while (0)

// Grow-only device / pinned-host scratch owned by the context.
int vsl_ctx_dscratch(vsl_ctx* ctx, size_t bytes, void** out);
int vsl_ctx_hpinned(vsl_ctx* ctx, size_t bytes, void** out);

// RAII stage timer: records events around a stage when profiling is enabled.
struct VslStage {
  vsl_ctx* ctx;
  int idx = -1;
  VslStage(vsl_ctx* c, int stage);
  ~VslStage();
};

// ---------------------------------------------------------------------------------------------
// Device-resident frame store (see include/vslam_hip.h "device-resident batched frame store").
// SoA per image slot; F = max_features; every array is dense so a range of slots is one launch.
struct vsl_frames {
  int device = 0;
  int max_images = 0, w = 0, h = 0, F = 0, max_pairs = 0;
  size_t cand_cap = 0;          // candidate capacity per image (w*h: every pixel may be a candidate)
  uint8_t* images = nullptr;    // [max_images][h][w]
  float* response = nullptr;    // [max_images][h][w]            K1 output
  int32_t* meta = nullptr;      // [max_images][VSL_META_STRIDE]: per-image counters on their own 128-B lines
  uint64_t* cand = nullptr;     // [max_images][cand_cap]        (fp32 bits << 32 | pixel index)
  int32_t* kp_xy = nullptr;     // [max_images][F][2]            selected corners, response-descending
  int32_t* kp_count = nullptr;  // [max_images]
  int32_t* kp_moments = nullptr;  // [max_images][F][2]          (m01, m10), exact
  double* kp_angle = nullptr;   // [max_images][F]
  uint64_t* kp_desc = nullptr;  // [max_images][F][4]
  // matcher
  int32_t* pair_slots = nullptr;   // [max_pairs][2]
  uint32_t* best_key = nullptr;    // [max_pairs][2][F]   (distance << 22 | index), direction 0: a->b
  uint32_t* second_key = nullptr;  // [max_pairs][2][F]
  int32_t* matches = nullptr;      // [max_pairs][F][2]
  int32_t* match_count = nullptr;  // [max_pairs]
  uint32_t* exact_list = nullptr;  // [max_images][VSL_EXACT_CAP]: (keypoint << 8) | bit, see describe.hip
  int32_t* tile_off = nullptr;     // [max_images][tiles + 1]: keypoints of an image by 64 x 64 tile (describe.hip), null when the tile kernel does not apply
  uint32_t* tile_ent = nullptr;    // [max_images][F]: (keypoint << 12) | (y in tile << 6) | x in tile, tile-major
  int tiles_x = 0, tiles = 0;
  uint32_t* sel_grid = nullptr;    // [max_images][cells]: packed selection grid (u16 accepted slots, then u16 list heads) of images too large for LDS (lazy)
  // rBRIEF near-tie records (see describe.hip)
  int32_t* tie_count = nullptr;    // [1]
  int32_t* tie_rec = nullptr;      // [tie_cap][4]  (slot, keypoint, bit, unused)
  int tie_cap = 0;
  bool ties_pending = false, ties_from_angles = false;
  bool detect_meta_dirty = true;    // MAX / NCAND not in their reset state (first use, or a failed launch)
  bool describe_meta_dirty = true;  // same for NEXACT
  // slot ranges described by the fast kernels since the last vsl_resolve_ties, in launch order: an exact-list overflow
  // in ANY of them is redone by the generic f64 kernel there (several asynchronous launches may precede one resolve)
  struct DescRange {
    int first, n, rotate;
  };
  std::vector<DescRange> pending_desc;
  // the guard's count was read as zero (or the descriptors are not handed out): nothing queued is left to verify.
  // Every fast path that skips vsl_resolve_ties ends here, so stale ranges do not pile up frame after frame.
  void ties_settled() {
    ties_pending = false;
    pending_desc.clear();
  }
  int exact_fallbacks = 0;            // how often that fallback ran (diagnostic)
  bool store_response = false;  // K1 writes the fp32 response image only for the parity hook
  std::vector<int32_t> pair_cache;  // host copy of pair_slots (skip the upload when unchanged)
  // stereo stage (stereo.hip), allocated by its first call: epipolar inliers of each pair and their triangulated points
  int32_t* st_pairs = nullptr;        // [max_pairs][F][2]  (left id, right id), match order
  double* st_points = nullptr;        // [max_pairs][F][3]  p_c in the left camera's frame (first triangulating call)
  int32_t* st_count = nullptr;        // [max_pairs]
  std::vector<uint8_t> st_has_points; // [max_pairs]: the pair's last stage call triangulated
};

int vsl_frames_alloc(vsl_ctx* ctx, int max_images, int w, int h, int F, int max_pairs, vsl_frames** out);

// internal launchers (asynchronous on ctx->stream)
int vsl_launch_detect(vsl_ctx* ctx, vsl_frames* f, int first, int n, int num_features);
int vsl_launch_describe(vsl_ctx* ctx, vsl_frames* f, int first, int n, int rotate_features,
                        int from_angles);
int vsl_launch_match(vsl_ctx* ctx, vsl_frames* f, int n_pairs, int threshold, double dist_2_best, int db_bound);
int vsl_resolve_ties(vsl_ctx* ctx, vsl_frames* f, int* n_resolved);
int vsl_set_pairs(vsl_ctx* ctx, vsl_frames* f, const int32_t* slot_pairs, int n_pairs);

// dense fp64 Cholesky solve on the device (chol.hip): S x = b in place, *ok_dev = 0 if not SPD
int vsl_chol_solve_dev(vsl_ctx* ctx, double* S, double* b, int n, int* ok_dev);
// the same on LAPACK-style lower band storage (chol.hip, "BAND FORM"): S = storage + bws, ld = bws = bw + VSL_CHOL_NB
int vsl_chol_solve_band_dev(vsl_ctx* ctx, double* S, double* b, int n, int ld, int bw, int* ok_dev, int cyclic = 0, double* neg_out = nullptr);

// the dense factorisation alone: S <- L in place, Linv <- the inverted VSL_CHOL_NB x VSL_CHOL_NB diagonal blocks of L
// (one per panel, identity-padded; device memory of the caller), *ok_dev = 0 if S is not SPD
int vsl_chol_factor_dev(vsl_ctx* ctx, double* S, int n, int* ok_dev, double* Linv);
// SELECTED INVERSION (chol.hip): the band of S^-1.  S and Z are band arrays of the same layout (S = storage + bws,
// Z = its own storage + bws, ld = bws = bw + VSL_CHOL_NB, chol_selinv_plan(n, bw).z_elems doubles each).  S <- L in
// place; Z receives every entry (i, j), 0 <= i - j <= bw, of S^-1 and zeros in all other slots.  *ok_dev = 0 (and Z
// undefined) if S is not positive definite by the factorisation's own pivot test.  Enqueued on the context's stream.
int vsl_chol_selinv_band_dev(vsl_ctx* ctx, double* S, double* Z, int n, int ld, int bw, int* ok_dev);
// The inverted VSL_CHOL_NB x VSL_CHOL_NB diagonal blocks of L (one per panel, identity-padded) that the last
// vsl_chol_selinv_band_dev(n, bw) on this context left in the context's device scratch: valid in stream order until the
// next call that takes that scratch (any band / ring solve or selected inversion).
const double* vsl_chol_selinv_linv_dev(vsl_ctx* ctx, int n, int bw);
// Columns of the inverse of a DENSE factor (ba_cov.hip: the solve behind vsl_ba_covariance): L L^T X = E for the unit
// columns col_unk[0 .. 16 nblk) (device; -1: an empty column), sixteen per workgroup.  X: nblk blocks of n x 16 doubles,
// entry (row i, column j) at vsl_cov_x_at(n, i, j).  L, Linv: what vsl_chol_factor_dev left.  Sdiag (nullable): diag S
// before the factorisation -- a pivot L_ii^2 <= 2^-36 Sdiag_i clears *ok_dev and nothing is written.
int vsl_cov_unit_columns_dev(vsl_ctx* ctx, int n, const double* L, const double* Linv, const double* Sdiag, const int* col_unk,
                             int nblk, double* X, int* ok_dev);
// The band routes of the covariance calls (ba_cov.hip).  L, Z: the STORAGE base of a band array (rows of ld + 1 slots,
// the diagonal last).
// pivot: the factor left by vsl_chol_selinv_band_dev against diag S before the factorisation -- a pivot L_ii^2 <=
// 2^-36 Sdiag_i clears *ok_dev.
// unit columns: L L^T X = E against the band factor for the unit columns col_unk[0 .. 16 nblk) (device; -1: an empty
// column), sixteen per workgroup, X as for vsl_cov_unit_columns_dev -- entries of the inverse outside the band.  Linv:
// vsl_chol_selinv_linv_dev.  row_lo (device, nullable = 0): per block the lowest row a caller reads; the rows above its
// 32-row panel are left unwritten.  Nothing is written when *ok_dev = 0: run it behind the pivot test.
int vsl_cov_band_unit_columns_dev(vsl_ctx* ctx, int n, const double* L, int ld, int bw, const double* Linv, const int* col_unk,
                                  const int* row_lo, int nblk, double* X, const int* ok_dev);
int vsl_cov_band_pivot_dev(vsl_ctx* ctx, int n, const double* L, int ld, const double* Sdiag, int* ok_dev);
// GENERAL right-hand sides against a band factor (ba_cov.hip, the same kernel with dense columns in place of unit
// ones): L L^T X = B in place, X holding B on entry in nblk blocks of n x 16 (vsl_cov_x_at).  L: the storage base, Linv:
// the inverted diagonal blocks of vsl_chol_factor_band_dev.  row_first (device, [nblk]): the block's first non-zero row
// (n: the block is zero), where its forward pass starts.  Nothing is done when *ok_dev = 0.
int vsl_band_rhs_solve_dev(vsl_ctx* ctx, int n, const double* L, int ld, int bw, const double* Linv, const int* row_first, int nblk,
                           double* X, const int* ok_dev);
// The band factorisation alone (chol.hip, the panel factor behind the selected inversion): S = storage + ld, ld = bw +
// VSL_CHOL_NB; S <- L in place, Linv <- the inverted diagonal blocks (VSL_CHOL_NB^2 doubles per panel, identity-padded;
// device memory of the caller), *ok_dev = 1 / 0.
int vsl_chol_factor_band_dev(vsl_ctx* ctx, double* S, int n, int ld, int bw, int* ok_dev, double* Linv);
// THE COVARIANCE CHAIN (ba_cov.hip "THE SHARED LAYER"), one statement for the reduced camera system of a bundle
// adjustment and the H of a pose graph.  Everything is enqueued on the context's stream; the caller keeps its own
// VslStage scope and its own ok word (preset to 1 where the factorisation does not set it).
// diag: diag[i] = S_ii of the storage as built -- ld = 0: dense n x n, else band rows of ld + 1 slots, the diagonal last.
int vsl_cov_diag_dev(vsl_ctx* ctx, int n, const double* S, int ld, double* diag);
// inverse: diag S, then by the route ld names
//   dense (ld = 0)  vsl_chol_factor_dev (S <- L, Linv <- the inverted diagonal blocks), vsl_cov_unit_columns_dev into X
//   band  (ld > 0)  vsl_chol_selinv_band_dev (S <- L, Z <- the band of S^-1), vsl_cov_band_pivot_dev, and -- nblk > 0
//                   only -- vsl_cov_band_unit_columns_dev into X with the inverted blocks the inversion left
struct VslCovInverse {
  int n = 0, ld = 0, bw = 0;
  double* S = nullptr;             // the storage base of the matrix
  double* Z = nullptr;             // band: the storage base of the band of the inverse (same layout as S); dense: null
  double* Linv = nullptr;          // dense: VSL_CHOL_NB^2 doubles per panel of the caller's; band: not used
  double* diag = nullptr;          // n doubles
  const int* col_unk = nullptr;    // [16 nblk] unit columns (device)
  const int* row_lo = nullptr;     // band: [nblk], see above
  int nblk = 0;
  double* X = nullptr;
  int* ok = nullptr;
};
int vsl_cov_inverse_dev(vsl_ctx* ctx, const VslCovInverse& a);
// diagonal blocks: out[36 q ..] = the 6 x 6 block of camera / node q_free[q] (device) of the inverse.  Dense: from X,
// whose right-hand sides 6 q .. 6 q + 5 belong to q_free[q], the two mirror entries averaged; band (ld > 0): from Z, the
// lower triangle mirrored.  Exactly symmetric either way; nothing written when *ok_dev = 0.
int vsl_cov_diag_blocks_dev(vsl_ctx* ctx, int n, int nQ, const int* q_free, int ld, const double* Z, const double* X,
                            const int* ok_dev, double* out);
// pair blocks: out[144 q ..] = the 12 x 12 joint block of pair q (device; pgo_cov_plan.h) -- see ba_pair_blocks_kernel
struct PgcPairDev;
int vsl_cov_pair_blocks_dev(vsl_ctx* ctx, int n, int n_pairs, const PgcPairDev* pairs, int band, const double* Z, int ld,
                            const double* X, const int* ok_dev, double* out);
// relative poses: ba_relpose_kernel (ba_cov.hip), one wavefront per pair -- meas [6], cov [36], info [36], singular [1]
// per pair from its joint block; poses: [7 per node] indexed by PgcPairDev::na / nb (cameras of a free problem, bodies of
// a rig).  Nothing written when *ok_dev = 0.
int vsl_ba_relpose_dev(vsl_ctx* ctx, int n_pairs, const double* poses, const PgcPairDev* pairs, const double* joint,
                       const int* ok_dev, double* meas, double* cov, double* info, int* singular);
__host__ __device__ inline size_t vsl_cov_x_at(int n, int i, int col) {
  return (size_t)(col / 16) * n * 16 + (size_t)i * 16 + (col % 16);
}

// scratch store of the host-buffer API
int vsl_ctx_scratch_frames(vsl_ctx* ctx, int w, int h, int feat, vsl_frames** out);

// order-preserving float <-> int mapping for atomicMax on fp32 values of any sign
__host__ __device__ inline int32_t vsl_float_to_ordered(float f) {
  int32_t i;
  memcpy(&i, &f, 4);
  return i >= 0 ? i : (int32_t)(i ^ 0x7fffffff);
}
__host__ __device__ inline float vsl_ordered_to_float(int32_t i) {
  int32_t j = i >= 0 ? i : (int32_t)(i ^ 0x7fffffff);
  float f;
  memcpy(&f, &j, 4);
  return f;
}

// ---------------------------------------------------------------------------------------------
// The ORB front end as passes of k images (orb.hip): vsl_frames_bow_vectors (bow.hip) drives it pass by pass on the frame
// store's images, vsl_orb_detect_describe as a pass of one image from the host.
// Per-image keypoint segments and the compact feature numbering of a pass, one 128-byte record per image on the device.
struct VslOrbImgSeg {
  int32_t seg_base[8], seg_cap[8];  // keypoint slots of each pyramid level inside the image's slot range
  int32_t feat_off[8];              // first feature of the level, relative to feat_base
  int32_t feat_base, n_feat;        // the image's features are rows [feat_base, feat_base + n_feat) of the pass's descriptor array
  int32_t pad[6];
};
struct VslOrbBatch {
  // in
  const uint8_t* images = nullptr;  // k dense w x h images, image_stride bytes apart (device)
  size_t image_stride = 0;
  const uint8_t* host_image = nullptr;  // instead of `images`, k = 1: one w x h image in host memory, rows host_pitch bytes apart
  size_t host_pitch = 0;
  int w = 0, h = 0, k = 0, nfeatures = 0, max_feat = 0;  // max_feat: most features of an image that can be described
  void* scratch = nullptr;          // device, pinned: the sizes vsl_orb_batch_bytes reports
  void* pinned = nullptr;
  // out (count): features per image and their place in the pass's compact arrays (feat_base is a multiple of 4)
  std::vector<int32_t> n_feat, feat_base;
  int n_rows = 0;                   // rows of the compact arrays = feat_base + n_feat of the last image, rounded up to 4
  // out (describe): valid in stream order
  const uint8_t* desc = nullptr;        // [n_rows][32]
  const VslOrbImgSeg* seg = nullptr;    // [k]
  // internal
  std::vector<int32_t> full;        // [k][8] keypoints per level
  std::vector<uint8_t> overflow;    // [k] more ties than the first segments hold
};
void vsl_orb_batch_bytes(int w, int h, int nfeatures, int k, int max_feat, size_t* device_bytes, size_t* pinned_bytes);
// stages up to the keypoint angles of all k images, ONE stream synchronisation: n_feat / feat_base / n_rows
int vsl_orb_batch_count(vsl_ctx* ctx, VslOrbBatch& b);
// second emit of the overflowing images (one more synchronisation, only then), libm cos / sin of all angles, describe launch
int vsl_orb_batch_describe(vsl_ctx* ctx, VslOrbBatch& b);
