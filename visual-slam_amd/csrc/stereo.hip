// stereo.hip -- the stereo stage of a keyframe after the matcher: epipolar inliers + midpoint triangulation.
//
// Reference: src/slam.cpp:1136-1150 filters the stereo matches with computeEssential / findInliersEssential
// (include/visnav/matching_utils.h:56-88); add_new_landmarks (include/visnav/vo_utils.h:232-317) then triangulates
// every stereo inlier in the left camera's frame.  The contract is the host restatement the pipeline runs
// (include/visnav_amd/harness/odometry.h find_inliers_essential, harness/pnp.h triangulate_midpoint):
//   p0 = unproject(cam_a, corner_a), p1 = unproject(cam_b, corner_b), err = p0 . (E p1),
//   inlier iff !(|err| > threshold)   (a NaN error is an inlier, as in the reference's `if (abs(err) > thr) {} else`),
//   p_c = triangulate_midpoint(p0, p1, R_0_1, t_0_1).
// Inliers come out in match order (ascending left feature id).  Shape: one workgroup of four waves per pair walks
// its match list in chunks of 256; each lane evaluates one match, a wave ballot + popcount of the lanes below gives
// the lane's rank in its wave, the four wave totals in LDS give the wave's offset.  No atomics: the output is the
// same for any schedule.  See DESIGN.md "Stereo inliers and triangulation".
#include "cam_device.h"

#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / VSL_WAVE)

namespace {

struct StereoParams {
  int model_a, model_b, triangulate;
  double intr_a[8], intr_b[8], E[9], R[9], t[3];
  double threshold;
};

// pair p = first_pair + blockIdx.x.  Keypoints of slot s: kp_xy + s * kp_stride * 2 (x, y); slots from pair_slots
// (null: slot 0 = a, slot 1 = b).  Matches and outputs of pair p at p * pair_stride entries.
template <class XY>
__global__ __launch_bounds__(ST_THREADS) void stereo_inliers_kernel(StereoParams prm_arg, const int32_t* __restrict__ pair_slots,
                                                                    int first_pair, const XY* __restrict__ kp_xy, int64_t kp_stride,
                                                                    const int32_t* __restrict__ matches,
                                                                    const int32_t* __restrict__ match_count, int64_t pair_stride,
                                                                    int32_t* __restrict__ out_pairs, double* __restrict__ out_points,
                                                                    int32_t* __restrict__ out_count) {
  __shared__ int wave_total[ST_WAVES];
  // the 38 doubles of the parameters live in LDS: held in scalar registers they would not fit (SGPR spills)
  __shared__ StereoParams sp;
  static_assert(sizeof(StereoParams) % 4 == 0 && sizeof(StereoParams) / 4 <= ST_THREADS, "one word per thread");
  if (threadIdx.x < sizeof(StereoParams) / 4)
    reinterpret_cast<uint32_t*>(&sp)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&prm_arg)[threadIdx.x];
  __syncthreads();
  const StereoParams& prm = sp;
  const int p = first_pair + (int)blockIdx.x;
  const int lane = threadIdx.x & (VSL_WAVE - 1), wave = threadIdx.x / VSL_WAVE;
  const int n = match_count[p];
  int sa = 0, sb = 1;
  if (pair_slots && n > 0) {
    sa = pair_slots[2 * p];
    sb = pair_slots[2 * p + 1];
  }
  const XY* xa = kp_xy + (size_t)sa * kp_stride * 2;
  const XY* xb = kp_xy + (size_t)sb * kp_stride * 2;
  const int32_t* m = matches + (size_t)p * pair_stride * 2;
  int32_t* op = out_pairs + (size_t)p * pair_stride * 2;
  double* opt = out_points ? out_points + (size_t)p * pair_stride * 3 : nullptr;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += ST_THREADS) {
    const int k = c0 + (int)threadIdx.x;
    bool in = false;
    int32_t i = 0, j = 0;
    CamVec3 pc = {0.0, 0.0, 0.0};
    if (k < n) {
      i = m[2 * k];
      j = m[2 * k + 1];
      const CamVec3 p0 = cam_unproject(prm.model_a, prm.intr_a, (double)xa[2 * i], (double)xa[2 * i + 1]);
      const CamVec3 p1 = cam_unproject(prm.model_b, prm.intr_b, (double)xb[2 * j], (double)xb[2 * j + 1]);
      const CamVec3 q = cam_mul(prm.E, p1);
      const double err = p0.x * q.x + p0.y * q.y + p0.z * q.z;
      in = !(fabs(err) > prm.threshold);
      if (in && prm.triangulate) pc = cam_triangulate_midpoint(p0, p1, prm.R, prm.t);
    }
    const uint64_t bal = __ballot(in);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(bal);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; w++) {
      const int c = wave_total[w];
      if (w < wave) off += c;
      total += c;
    }
    if (in) {
      const int r = off + below;
      op[2 * r] = i;
      op[2 * r + 1] = j;
      if (prm.triangulate) {
        opt[3 * r] = pc.x;
        opt[3 * r + 1] = pc.y;
        opt[3 * r + 2] = pc.z;
      }
    }
    base += total;
    __syncthreads();  // wave_total is rewritten by the next chunk
  }
  if (threadIdx.x == 0) out_count[p] = base;
}

int fill_params(vsl_ctx* ctx, const char* who, StereoParams& prm, int model_a, const double* intr8_a, int model_b,
                const double* intr8_b, const double* E9, const double* R9_0_1, const double* t3_0_1, double threshold,
                int triangulate) {
  if (!intr8_a || !intr8_b || !E9) return vsl_fail(ctx, VSL_ERR_INVALID, "%s: null intrinsics or E", who);
  if (model_a < VSL_CAM_DS || model_a > VSL_CAM_KB4 || model_b < VSL_CAM_DS || model_b > VSL_CAM_KB4)
    return vsl_fail(ctx, VSL_ERR_INVALID, "%s: unknown camera model (%d, %d)", who, model_a, model_b);
  prm.model_a = model_a;
  prm.model_b = model_b;
  prm.triangulate = (triangulate && R9_0_1 && t3_0_1) ? 1 : 0;
  memcpy(prm.intr_a, intr8_a, sizeof(prm.intr_a));
  memcpy(prm.intr_b, intr8_b, sizeof(prm.intr_b));
  memcpy(prm.E, E9, sizeof(prm.E));
  memset(prm.R, 0, sizeof(prm.R));
  memset(prm.t, 0, sizeof(prm.t));
  if (prm.triangulate) {
    memcpy(prm.R, R9_0_1, sizeof(prm.R));
    memcpy(prm.t, t3_0_1, sizeof(prm.t));
  }
  prm.threshold = threshold;
  return VSL_OK;
}

}  // namespace

extern "C" int vsl_frames_stereo_inliers(vsl_ctx* ctx, vsl_frames* f, int first_pair, int n_pairs, int model_a,
                                         const double* intr8_a, int model_b, const double* intr8_b, const double* E9,
                                         const double* R9_0_1, const double* t3_0_1, double threshold, int triangulate) {
  if (!ctx || !f) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_stereo_inliers: null argument");
  if (first_pair < 0 || n_pairs < 0 || (int64_t)first_pair + n_pairs > f->max_pairs)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_stereo_inliers: pairs [%d, %d) outside [0, %d)", first_pair,
                    first_pair + n_pairs, f->max_pairs);
  StereoParams prm;
  int rc = fill_params(ctx, "vsl_frames_stereo_inliers", prm, model_a, intr8_a, model_b, intr8_b, E9, R9_0_1, t3_0_1, threshold,
                       triangulate);
  if (rc) return rc;
  if (n_pairs == 0) return VSL_OK;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  // the stage's outputs exist only in stores that use it (allocated on the first call; the points on the first
  // call that triangulates)
  const size_t P = (size_t)f->max_pairs, F = (size_t)f->F;
  if (!f->st_count) VSL_HIP(ctx, hipMalloc((void**)&f->st_count, P * sizeof(int32_t)));
  if (!f->st_pairs) {
    VSL_HIP(ctx, hipMalloc((void**)&f->st_pairs, P * F * 2 * sizeof(int32_t)));
    VSL_HIP(ctx, hipMemsetAsync(f->st_count, 0, P * sizeof(int32_t), ctx->stream));
    f->st_has_points.assign(P, 0);
  }
  if (prm.triangulate && !f->st_points) VSL_HIP(ctx, hipMalloc((void**)&f->st_points, P * F * 3 * sizeof(double)));
  hipLaunchKernelGGL(stereo_inliers_kernel<int32_t>, dim3(n_pairs), dim3(ST_THREADS), 0, ctx->stream, prm, f->pair_slots, first_pair,
                     f->kp_xy, (int64_t)F, f->matches, f->match_count, (int64_t)F, f->st_pairs,
                     prm.triangulate ? f->st_points : nullptr, f->st_count);
  VSL_CHECK_LAUNCH(ctx);
  for (int p = first_pair; p < first_pair + n_pairs; p++) f->st_has_points[p] = (uint8_t)prm.triangulate;
  return VSL_OK;
}

extern "C" int vsl_frames_download_inliers(vsl_ctx* ctx, vsl_frames* f, int pair, int cap_pairs, int32_t* pairs, double* points_c,
                                           int* n_out) {
  if (!ctx || !f || pair < 0 || pair >= f->max_pairs || !n_out || cap_pairs < 0)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_download_inliers: bad arguments");
  if (!f->st_pairs) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_download_inliers: the stereo stage has not run on this store");
  if (points_c && !f->st_has_points[pair])
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_download_inliers: pair %d was not triangulated", pair);
  // one round trip: the count, the pair list and the points at full capacity into pinned memory together
  const size_t F = (size_t)f->F;
  void* hp = nullptr;
  int rc = vsl_ctx_hpinned(ctx, 64 + 8 * F + 24 * F, &hp);
  if (rc) return rc;
  int32_t* hdr = (int32_t*)hp;
  int32_t* hpairs = (int32_t*)((char*)hp + 64);
  double* hpts = (double*)((char*)hp + 64 + 8 * F);
  VSL_HIP(ctx, hipMemcpyAsync(hdr, f->st_count + pair, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (pairs)
    VSL_HIP(ctx, hipMemcpyAsync(hpairs, f->st_pairs + (size_t)pair * F * 2, sizeof(int32_t) * 2 * F, hipMemcpyDeviceToHost, ctx->stream));
  if (points_c)
    VSL_HIP(ctx, hipMemcpyAsync(hpts, f->st_points + (size_t)pair * F * 3, sizeof(double) * 3 * F, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = hdr[0];
  *n_out = n;
  if (n > cap_pairs) return vsl_fail(ctx, VSL_ERR_CAPACITY, "inlier capacity %d < %d", cap_pairs, n);
  if (n > 0 && pairs) memcpy(pairs, hpairs, sizeof(int32_t) * 2 * (size_t)n);
  if (n > 0 && points_c) memcpy(points_c, hpts, sizeof(double) * 3 * (size_t)n);
  return VSL_OK;
}

extern "C" int vsl_frames_download_inlier_counts(vsl_ctx* ctx, vsl_frames* f, int n_pairs, int32_t* counts) {
  if (!ctx || !f || n_pairs < 0 || n_pairs > f->max_pairs || (n_pairs > 0 && !counts))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_download_inlier_counts: bad arguments");
  if (!f->st_pairs) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_frames_download_inlier_counts: the stereo stage has not run on this store");
  if (n_pairs == 0) return VSL_OK;
  VSL_HIP(ctx, hipMemcpyAsync(counts, f->st_count, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VSL_OK;
}

extern "C" int vsl_find_inliers_essential(vsl_ctx* ctx, int model_a, const double* intr8_a, int model_b, const double* intr8_b,
                                          const double* E9, const double* kp_a_xy, int n_a, const double* kp_b_xy, int n_b,
                                          const int32_t* matches, int n_matches, double threshold, const double* R9_0_1,
                                          const double* t3_0_1, int32_t* pairs_out, double* points_out, int* n_out) {
  if (!ctx || !n_out || n_a < 0 || n_b < 0 || n_matches < 0 || (n_matches > 0 && (!matches || !pairs_out || !kp_a_xy || !kp_b_xy)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_find_inliers_essential: bad arguments");
  *n_out = 0;
  StereoParams prm;
  int rc = fill_params(ctx, "vsl_find_inliers_essential", prm, model_a, intr8_a, model_b, intr8_b, E9, R9_0_1, t3_0_1, threshold,
                       points_out ? 1 : 0);
  if (rc) return rc;
  if (points_out && !prm.triangulate)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_find_inliers_essential: points need R_0_1 and t_0_1");
  for (int k = 0; k < 2 * n_matches; k++) {
    const int32_t v = matches[k], lim = (k & 1) ? n_b : n_a;
    if (v < 0 || v >= lim)
      return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_find_inliers_essential: match %d index %d outside [0, %d)", k / 2, v, lim);
  }
  if (n_matches == 0) return VSL_OK;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  // one staging buffer, one copy each way: [keypoints a | keypoints b (kp_stride = n_a)] [matches] [count] [pairs] [points]
  const size_t kp_bytes = sizeof(double) * 2 * ((size_t)n_a + n_b), m_bytes = sizeof(int32_t) * 2 * (size_t)n_matches;
  const size_t in_bytes = kp_bytes + m_bytes + 64;
  const size_t out_bytes = 64 + m_bytes + (points_out ? sizeof(double) * 3 * (size_t)n_matches : 0);
  void* dp = nullptr;
  void* hp = nullptr;
  if ((rc = vsl_ctx_dscratch(ctx, in_bytes + out_bytes, &dp))) return rc;
  if ((rc = vsl_ctx_hpinned(ctx, in_bytes > out_bytes ? in_bytes : out_bytes, &hp))) return rc;
  char* h = (char*)hp;
  memcpy(h, kp_a_xy, sizeof(double) * 2 * (size_t)n_a);
  memcpy(h + sizeof(double) * 2 * (size_t)n_a, kp_b_xy, sizeof(double) * 2 * (size_t)n_b);
  memcpy(h + kp_bytes, matches, m_bytes);
  *(int32_t*)(h + kp_bytes + m_bytes) = n_matches;
  char* d = (char*)dp;
  VSL_HIP(ctx, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  char* dout = d + in_bytes;
  hipLaunchKernelGGL(stereo_inliers_kernel<double>, dim3(1), dim3(ST_THREADS), 0, ctx->stream, prm, (const int32_t*)nullptr, 0,
                     (const double*)d, (int64_t)n_a, (const int32_t*)(d + kp_bytes), (const int32_t*)(d + kp_bytes + m_bytes),
                     (int64_t)n_matches, (int32_t*)(dout + 64), points_out ? (double*)(dout + 64 + m_bytes) : nullptr,
                     (int32_t*)dout);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpyAsync(h, dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = *(int32_t*)h;
  *n_out = n;
  memcpy(pairs_out, h + 64, sizeof(int32_t) * 2 * (size_t)n);
  if (points_out) memcpy(points_out, h + 64 + m_bytes, sizeof(double) * 3 * (size_t)n);
  return VSL_OK;
}
