// ba_state.h -- host-side state of the general bundle-adjustment path (ba.hip) and the host launchers that ba.hip, the
// home of the ba_* kernels, shares with the session solver (ba_session.hip), the covariances (ba_cov.hip) and the
// rig-constrained solver (ba_rig.hip).  The build has no relocatable device code: a kernel is launched from the file that
// defines it, so the other files reach the ba_* kernels through these -- the session and the covariances through the
// BaCommon launchers, the rig chain (its own state) through the plain-pointer launchers at the end of this file.
#pragma once
#include <algorithm>
#include <vector>

#include "vsl_common.h"
#include "dev_arena.h"
#include "ba_device.h"
#include "ba_pcg_plan.h"

// What the caller of ba_setup runs.  It decides who pays for the arena, whether S may take a band form and which
// buffers exist:
//   PARITY_HOOK       vsl_ba_residuals_jacobians: raw blocks of one evaluation          (owned arena, dense S)
//   SINGLE_LINEARIZE  vsl_ba_linearize, vsl_bundle_adjust_intrinsics: stored blocks     (owned arena, dense S)
//   HOST_LOOP         vsl_bundle_adjust: stored blocks in TWO sets (the candidate is linearised speculatively)
//                                                                                       (the context's arena, band forms)
//   SESSION           vsl_global_bundle_adjust: stored blocks OR the recompute form (ba_recompute_form decides), and the
//                     camera LM diagonal kept across rejected steps                     (owned arena, band forms)
//   COVARIANCE        vsl_ba_covariance (ba_cov.hip): stored blocks of one linearisation, plus `extra_bytes` of the
//                     caller's own in the same block (BaCommon::extra)                  (the context's arena, dense S)
//   GLOBAL_COVARIANCE vsl_global_ba_covariance (ba_cov.hip): as COVARIANCE, but S may take the LINEAR band form (never
//                     the cyclic one: selected inversion has no ring recurrence).  The caller's share depends on the
//                     layout and on the band order, so it is asked for through BaCaller::plan_extra once the host plan
//                     exists                                                            (the context's arena, dense or linear band)
enum class BaUse { PARITY_HOOK, SINGLE_LINEARIZE, HOST_LOOP, SESSION, COVARIANCE, GLOBAL_COVARIANCE };

struct BaHostPlan;  // ba_host_plan.h

struct BaCaller {
  BaUse use;
  const vsl_ba_problem* graph_prob = nullptr;  // the problem whose observations define the covisibility graph (a session rank: the FULL problem); null: the problem itself
  int run_max_obs = 0, run_max_lms = 0;        // SESSION: limits of a landmark run of the recompute-form kernels (ba_large.h BL_THREADS, BL_LMW)
  size_t extra_bytes = 0;                      // COVARIANCE: bytes the caller carves up itself, at BaCommon::extra
  // GLOBAL_COVARIANCE: called once the host plan exists and before the arena is planned, with the layout of S and the
  // free-camera numbering it implies (hp.cam_free: the band order when hp.layout.renumber).  Sets *extra_bytes;
  // a return other than VSL_OK ends ba_setup with it.  May throw std::bad_alloc.
  int (*plan_extra)(void* self, const BaHostPlan& hp, size_t* extra_bytes) = nullptr;
  void* plan_extra_self = nullptr;
  // SESSION, matrix-free (ba_pcg.h): S is not allocated, no pair lists; the PCG's vectors are (BaRecompute::pcg_*).
  // Needs the recompute form: ba_setup fails with VSL_ERR_INVALID where the plan cannot give it.
  bool matrix_free = false;
  bool runs_at_any_size = false;  // matrix-free hooks: landmark runs (and with them the recompute form) also at <= 128 unknowns
};

// Buffers of the STORED-BLOCKS form: r / F / E of every observation, written by ba_linearize_kernel and read by the
// operator-by-operator chain.  Everything but a recompute-form session has them.
struct BaStored {
  double *r = nullptr, *F = nullptr, *E = nullptr, *grad_l = nullptr, *diag_c = nullptr, *diag_l = nullptr, *gabs = nullptr;
  double *dl = nullptr, *partials = nullptr;
  double *S_part = nullptr, *rhs_part = nullptr;  // small systems: per-workgroup partial matrices
  double* Wg = nullptr;                           // large systems, gather form: per-observation W blocks (Yg is common)
  // second linearisation set (HOST_LOOP: vsl_bundle_adjust linearises the CANDIDATE point speculatively, before the host
  // has read the step's verdict; an accepted step swaps the sets, a rejected one leaves the current set untouched)
  double *r2 = nullptr, *F2 = nullptr, *E2 = nullptr, *n2l2 = nullptr, *grad_l2 = nullptr, *H2 = nullptr, *g_c2 = nullptr;
  double *diag_c2 = nullptr, *diag_l2 = nullptr;
};

// Buffers of the RECOMPUTE form of a session's iteration (ba_large.h): landmark runs of the workgroups, their partial
// sums, camera-major copies of (landmark, pixel)
struct BaRecompute {
  int n_wg = 0;
  int bl_seg = 1;  // workgroups per free camera in bal_cam_kernel (an observation is a chain of dependent gathers, one per thread)
  int *wg_lm = nullptr, *cam_lm = nullptr;
  double *lpart = nullptr, *cam_uv = nullptr;
  double* pbs = nullptr;  // pbs[3 l + x] = scale_l (P^-1 b)_l: what the reduced right-hand side needs of a landmark
  // matrix-free route only (ba_pcg.h): iterate, residual, M^-1 r, direction, S p (n each), t (3 L), segment partials
  // (6 per free camera and segment), M^-1 (36 per free camera), the solve's record
  double *pcg_x = nullptr, *pcg_r = nullptr, *pcg_z = nullptr, *pcg_p = nullptr, *pcg_q = nullptr, *pcg_t = nullptr;
  double *pcg_part = nullptr, *pcg_minv = nullptr;
  BpcgRec* pcg_rec = nullptr;
};

// What every form names.  The launchers of a form take this and the form's own struct, nothing else: naming a buffer
// of the other form does not compile.
struct BaCommon {
  BaDims D;
  int G = 1, lm_per_wg = 1, nb_obs = 1, nb_upd = 1;
  int cb_seg = 1;  // workgroups per free camera in ba_cam_block_kernel
  bool small = true;
  std::vector<int> perm;  // sorted position -> caller observation index
  // ONE device allocation per solve (dev_arena.h), carved into the buffers below and the form's: vsl_bundle_adjust
  // borrows the context's cached arena, a session and the parity hooks own theirs
  DevArena arena;
  double *poses = nullptr, *cand_poses = nullptr, *points = nullptr, *cand_points = nullptr, *intr = nullptr, *obs_uv = nullptr;
  double *scale_c = nullptr, *scale_l = nullptr, *n2l = nullptr;
  double *H = nullptr, *g_c = nullptr, *S = nullptr, *rhs = nullptr;
  double *Pinv = nullptr, *bl = nullptr, *dc = nullptr;
  double *scalars = nullptr, *cam_part = nullptr;
  int *cam_intr = nullptr, *cam_free = nullptr, *free_cams = nullptr, *obs_cam = nullptr, *obs_lm = nullptr;
  int *lm_start = nullptr, *cam_start = nullptr, *cam_obs = nullptr;
  int* flag = nullptr;           // 128 bytes behind scalars: one copy brings both back
  double* diagc_keep = nullptr;  // SESSION: clamp(diag H_full), reused across rejected steps
  char* extra = nullptr;         // COVARIANCE, GLOBAL_COVARIANCE: the caller's bytes of the same block
  // large systems, gather form of the Schur complement (ba_schur_gather_kernel): per-block pair lists, built on the
  // first use for the landmark range they cover, and the per-observation Y blocks of the current linearisation
  int *pair_cnt = nullptr, *pair_start = nullptr, *pairs = nullptr, *cam_pos = nullptr;
  double* Yg = nullptr;
  int n_slots = 0, hbp1 = 0;
  size_t n_pairs_cap = 0;
  int pair_l0 = -1, pair_lc = -1;
  // Layout of the reduced camera system S: dense (ldS = n, offset 0) or, for large systems whose cameras can be
  // ordered into a narrow band (reverse Cuthill-McKee on the covisibility graph, ba_setup), LAPACK-style lower band
  // storage -- row i keeps columns [i - bws, i], bws = bw + VSL_CHOL_NB, entry (i, j) at S[i * ldS + j + offS] with
  // ldS = offS = bws (chol.hip "BAND FORM").  The free-camera numbering IS the band order.
  bool banded = false;
  bool cyclic = false;  // band form whose band closes on itself (camera loop in trajectory order): wrap blocks in the leading slots of the first rows
  int ldS = 0, offS = 0, bw = 0;
  size_t s_elems = 0;  // doubles to allocate / clear / exchange for S
  bool matrix_free = false;  // S does not exist: the camera step comes from the PCG of ba_pcg.h (S = nullptr, s_elems = 0)
  double* S_eff() { return S + offS; }
};

struct BaState : BaCommon {
  bool recompute = false;  // which of the two below ba_setup requested from the arena
  BaStored sb;
  BaRecompute rc;
  void swap_sets() {
    std::swap(sb.r, sb.r2); std::swap(sb.F, sb.F2); std::swap(sb.E, sb.E2); std::swap(n2l, sb.n2l2);
    std::swap(sb.grad_l, sb.grad_l2); std::swap(H, sb.H2); std::swap(g_c, sb.g_c2); std::swap(sb.diag_c, sb.diag_c2);
    std::swap(sb.diag_l, sb.diag_l2);
    std::swap(poses, cand_poses); std::swap(points, cand_points);
  }
};

// set-up phase times on stderr when VSL_BA_TRACE is set (developer aid)
struct BaTrace {
  bool on;
  double t0;
  BaTrace() : on(getenv("VSL_BA_TRACE") != nullptr), t0(now_ms()) {}
  void lap(const char* what, size_t bytes = 0) {
    if (!on) return;
    const double t = now_ms();
    if (bytes) fprintf(stderr, "  [ba set-up] %-28s %8.3f ms, %zu bytes\n", what, t - t0, bytes);
    else fprintf(stderr, "  [ba set-up] %-28s %8.3f ms\n", what, t - t0);
    t0 = t;
  }
};

// ---- ba.hip: set-up, and the launchers of its kernels (all asynchronous on ctx->stream unless they say otherwise)
int ba_validate(vsl_ctx* ctx, const vsl_ba_problem* p);
// host plan, ONE arena for the caller's use, uploads; synchronises
int ba_setup(vsl_ctx* ctx, const vsl_ba_problem* p, const vsl_ba_options* o, BaState& st, const BaCaller& caller);
// the layout of S that ba_setup chooses for this caller, decided on the host alone (no device work)
int ba_layout_of(vsl_ctx* ctx, const vsl_ba_problem* p, const BaCaller& caller, bool* banded);
// linearize at (poses, points): r, F, E (scaled when `scaled`), cost -> scalars[cost_slot]
int ba_linearize(vsl_ctx* ctx, BaCommon& st, BaStored& sb, bool scaled, int cost_slot = 0);
// per-landmark and per-camera column statistics of the stored blocks: n2l, grad_l, H, g_c
int ba_columns(vsl_ctx* ctx, BaCommon& st, BaStored& sb);
// F, E *= the Jacobi scaling (scale_c, scale_l)
int ba_apply_scale(vsl_ctx* ctx, BaCommon& st, BaStored& sb);
// Schur complement of the landmark blocks over landmarks [l0, l0 + lc); damping (sb.diag_l, sb.diag_c) when `damp`
int ba_schur(vsl_ctx* ctx, BaCommon& st, BaStored& sb, bool damp, double radius, int l0, int lc, bool keep_backsub, bool lower_only);
// block pair lists of the gather-form Schur complement for landmarks [l0, l0 + lc): built once per solve
int ba_pair_lists(vsl_ctx* ctx, BaCommon& st, int l0, int lc);
// S += sum over the pair lists of Y_i W_j^T (ba_schur_gather_kernel)
int ba_schur_gather(vsl_ctx* ctx, BaCommon& st, const double* W, const double* Y, int lower_mode);
// dc = -(S^-1 rhs), enqueued only: flag[0] = 1 (the finite check clears it), flag[1] = Cholesky succeeded.
// flags_set: the caller's previous kernel has set both flags (saves the launch)
int ba_solve_enqueue(vsl_ctx* ctx, BaCommon& st, bool flags_set = false);
// from dc, the step chain of the stored-blocks form (the host loop and the session both run it): back-substitution (dl),
// flag[0] &= dc and dl finite, scalars[2] = model cost change, candidate (cand_poses, cand_points), scalars[3] / [4] =
// squared step / x norms
int ba_step_from_dc(vsl_ctx* ctx, BaCommon& st, BaStored& sb);
// ba_step_from_dc and what only a session needs: scalars[6] / [7] = the norms of the cameras alone, [5] = cost at the
// candidate
int ba_candidate(vsl_ctx* ctx, BaCommon& st, BaStored& sb);
// dst[0] = max of the n values of v (ba_reduce_kernel, one workgroup)
int ba_max_of(vsl_ctx* ctx, const double* v, int n, double* dst);
// the first n scalars, on the host.  Synchronises.
int read_scalars(vsl_ctx* ctx, BaCommon& st, double* out, int n);

// ---- ba.hip: plain-pointer launchers.  They take device pointers and counts, no BaCommon / BaStored, so the rig chain
// (ba_rig.hip, its own state and plan) runs on the same kernels; the launchers above are written on them, and each of
// these kernels has this one launch site.  All enqueue on ctx->stream and check the launch.
// dc = -(S^-1 rhs) for n <= 128 by one workgroup; *ok_flag (device-visible memory) = 1 / 0
int vsl_ba_chol_small_launch(vsl_ctx* ctx, int n, const double* S, const double* rhs, double* dc, int* ok_flag);
// ba_linearize_kernel over the D.O observations (reads O, model0 / model1, use_huber, huber of D): robustified r, F, E,
// scaled when scale_c / scale_l are given, cost partials [(O + 255) / 256].  tcb == nullptr: F against the camera pose
// (cam_free: camera -> free-camera slot).  tcb = T_c_b tables [2][12] (rig): poses are the cameras derived from the
// bodies, cam_free maps a camera to its body's slot, F = F_c Ad(T_c_b) against the body pose
int vsl_ba_linearize_launch(vsl_ctx* ctx, const BaDims& D, const double* poses, const double* points, const double* intr,
                            const double* tcb, const int* cam_intr, const int* cam_free, const int* obs_cam, const int* obs_lm,
                            const double* obs_uv, const double* scale_c, const double* scale_l, double* r, double* F, double* E,
                            double* partials);
// scalars[slot] = sum (or max) of partials[0, n) in a fixed order
int vsl_ba_reduce_launch(vsl_ctx* ctx, const double* partials, int n, double* scalars, int slot, bool is_max);
// scalars[slot], scalars[slot + 1] = sums of partials[0, n), partials[n, 2 n)
int vsl_ba_reduce2_launch(vsl_ctx* ctx, const double* partials, int n, double* scalars, int slot);
// per landmark: squared column norms of E (n2l) and E^T r (grad_l)
int vsl_ba_lm_cols_launch(vsl_ctx* ctx, int L, const int* lm_start, const double* r, const double* E, double* n2l, double* grad_l);
// part[(block, segment)][27] -> H (6 x 6, mirrored) and g per pose block, segments in order
int vsl_ba_block_finish_launch(vsl_ctx* ctx, int nfree, int nseg, const double* part, double* H, double* g);
// Jacobi scaling 1 / (1 + sqrt(column norm^2)) from diag H and n2l
int vsl_ba_make_scale_launch(vsl_ctx* ctx, int nfree, int L, const double* H, const double* n2l, double* scale_c, double* scale_l);
// LM diagonals clamp(column norm^2, 1e-6, 1e32) and scalars[slot] = max |gradient| of the unscaled problem; gabs: one
// double per 256 of max(6 nfree, 3 L)
int vsl_ba_diag_gmax_launch(vsl_ctx* ctx, int nfree, int L, const double* H, const double* n2l, const double* g_c, const double* grad_l,
                            const double* scale_c, const double* scale_l, double* diag_c, double* diag_l, double* gabs,
                            double* scalars, int slot);
// model cost change partials [(O + 255) / 256]; cam_free: camera -> slot of its pose block in dc (-1: fixed)
int vsl_ba_model_launch(vsl_ctx* ctx, int O, const int* obs_cam, const int* obs_lm, const int* cam_free, const double* r,
                        const double* F, const double* E, const double* dc, const double* dl, double* partials);
// candidate pose blocks T * exp(step .* scale) (n_poses of them, pose_free: block -> slot or -1) and points; scalars[slot] /
// [slot + 1] = squared step / x norms; partials: 2 * ((max(n_poses, L) + 255) / 256)
int vsl_ba_update_launch(vsl_ctx* ctx, int n_poses, int L, const int* pose_free, const double* poses, const double* points,
                         const double* dc, const double* dl, const double* scale_c, const double* scale_l, double* cand_poses,
                         double* cand_points, double* partials, double* scalars, int slot);

// ---- ba.hip: what the two speculative host loops (vsl_bundle_adjust, vsl_bundle_adjust_rig) share besides
// lm_speculative_loop (lm_policy.h)
// the loop's one copy per iteration: the 16 scalars and the two flags behind them, through the context's pinned block.
// Synchronises.
int ba_fetch_step(vsl_ctx* ctx, const double* scalars, double* sc16, int* flags2);
// taken before the first stage of a solve; ba_finish_summary fills the times of `sum` from it (stage times only under
// profiling), prints "<label> iterations ..." at verbosity >= 1 and copies sum to *out when out is not null
struct BaSolveTimes {
  double t_start, base_ms[3];
  bool prof_was;
  BaSolveTimes(vsl_ctx* ctx, double t_start_ms);
};
void ba_finish_summary(vsl_ctx* ctx, const BaSolveTimes& t, int verbosity, const char* label, vsl_ba_summary& sum, vsl_ba_summary* out);
