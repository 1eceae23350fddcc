// vo.hip -- landmark projection and guided descriptor matching: per frame and, after a loop
// closure, for all views of a covisibility neighbourhood at once (DESIGN.md "Landmark fusion").
//
// Replaces visnav::project_landmarks (include/visnav/vo_utils.h:48-81) and visnav::find_matches_landmarks
// (include/visnav/vo_utils.h:83-167), which src/slam.cpp runs on EVERY frame (:1099-1114, :1159, :1339).  The device
// logic -- the fp64 projection in the oracle's operation order, the order-preserving compaction, the wavefront search
// with the reference's partial_sort tie order as a state machine -- is in guided_search.h, once; the kernels here say
// where the operands come from:
//
//   project_kernel             grid (1024-landmark chunk, view), pose of the view from pose8 + 8 * view -> keep, uv
//   compact_projection_kernel  one workgroup per view loops over the view's row: (uv, landmark) of the kept ones in
//                              ascending landmark order (the caller's order, the reference iterates its unordered_map;
//                              that order decides ties in the search) + their count
//   find_matches_kernel        grid (4 keypoints, view), one wavefront per keypoint: result = landmark index or -1
//   compact_matches_kernel     one workgroup per view: (feature, landmark) pairs in feature order into the view's own
//                              segment + their count
//                              -- these four serve vsl_project_landmarks / vsl_find_matches_landmarks (one view) and
//                              vsl_fuse_search (all views)
//   project_compact_kernel     the tracker's projection + compaction in one launch (chained workgroups)
//   track_matches_kernel       the tracker's search: keypoints of a frame store slot, descriptors through the map's
//                              pool index, results into the pinned mailbox
#include "guided_search.h"
#include "vsl_common.h"

#define VSL_FUSE_MAX_VIEWS 64

namespace {

__global__ __launch_bounds__(1024) void project_kernel(const double* __restrict__ pose8, int model,
                                                       const double* __restrict__ intr, int width, int height,
                                                       const double* __restrict__ points, int n, double z_thr,
                                                       double* __restrict__ uv, uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * 1024 + threadIdx.x;
  if (i >= n) return;
  const size_t o = (size_t)blockIdx.y * (size_t)n + (size_t)i;
  double u, v;
  const bool ok = project_in_view(pose8 + 8 * (size_t)blockIdx.y, model, intr, width, height, points + 3 * (size_t)i, z_thr, u, v);
  uv[2 * o] = u;
  uv[2 * o + 1] = v;
  keep[o] = ok ? 1 : 0;
}

// view = blockIdx.x, on the view's row (n entries) of uv / keep / out_uv / out_idx
__global__ __launch_bounds__(1024) void compact_projection_kernel(const double* __restrict__ uv, const uint8_t* __restrict__ keep,
                                                                  int n, double* __restrict__ out_uv, int32_t* __restrict__ out_idx,
                                                                  int32_t* __restrict__ n_out) {
  const size_t row = (size_t)blockIdx.x * (size_t)n;
  uv += 2 * row;
  keep += row;
  out_uv += 2 * row;
  out_idx += row;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const bool ok = i < n && keep[i];
    int total;
    const int p = base + wg1024_ordered_slot(ok, total);
    if (ok) {
      out_uv[2 * (size_t)p] = uv[2 * (size_t)i];
      out_uv[2 * (size_t)p + 1] = uv[2 * (size_t)i + 1];
      out_idx[p] = i;
    }
    base += total;
    __syncthreads();  // the next chunk rewrites the wave totals
  }
  if (threadIdx.x == 0) n_out[blockIdx.x] = base;
}

// Projection + the order-preserving compaction in ONE launch (vsl_map_track): a workgroup projects 1024 landmarks,
// compacts them in landmark order, and takes its base offset from the chain of its predecessors' totals ("stream
// scan": block b waits for block b - 1's running total, published as one 64-bit word (epoch << 32 | total) with
// release / acquire at device scope -- no flags to reset between calls, the epoch changes).  Forward progress of the
// wait: up to VO_CHAIN_RESIDENT_BLOCKS workgroups (one per compute unit: every one of them is resident from the start)
// the hardware's index-order dispatch makes blockIdx the chain position; larger maps (> 262 k landmarks) draw their
// chain position from an atomic ticket instead, so a workgroup only ever waits for workgroups that have STARTED --
// the decoupled look-back rule -- whatever the dispatch order (the ticket word is reset by the workgroup that draws
// the last one).  The all-views search does not use it: the argument needs ONE chain per grid.
#define VO_CHAIN_RESIDENT_BLOCKS 256
struct PoseIntr {
  double v[16];  // pose (qx qy qz qw tx ty tz, pad) | intrinsics (8)
};
__global__ __launch_bounds__(1024) void project_compact_kernel(PoseIntr pi, int model, int width, int height,
                                                               const double* __restrict__ points, int n, double z_thr,
                                                               double* __restrict__ out_uv, int32_t* __restrict__ out_idx,
                                                               int32_t* __restrict__ n_out, unsigned long long* __restrict__ chain,
                                                               unsigned int epoch, unsigned int* __restrict__ ticket) {
  __shared__ int base_s;
  __shared__ unsigned int bid_s;
  unsigned int bid = blockIdx.x;
  if (ticket) {  // workgroup-uniform
    if (threadIdx.x == 0) {
      const unsigned int t = atomicAdd(ticket, 1u);
      if (t == gridDim.x - 1) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all drawn: ready for the next call
      bid_s = t;
    }
    __syncthreads();
    bid = bid_s;
  }
  const int i = (int)bid * 1024 + threadIdx.x;
  double u = 0, v = 0;
  const bool ok = i < n && project_in_view(pi.v, model, pi.v + 8, width, height, points + 3 * (size_t)i, z_thr, u, v);
  int total;
  const int slot = wg1024_ordered_slot(ok, total);
  if (threadIdx.x == 0) {
    unsigned long long prev = 0;
    if (bid > 0) {
      do {
        prev = __hip_atomic_load(&chain[bid - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      } while ((unsigned int)(prev >> 32) != epoch);
    }
    const int base = (int)(unsigned int)prev;
    __hip_atomic_store(&chain[bid], ((unsigned long long)epoch << 32) | (unsigned int)(base + total), __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_AGENT);
    base_s = base;
    if (bid == gridDim.x - 1) *n_out = base + total;
  }
  __syncthreads();
  if (ok) {
    const int p = base_s + slot;
    out_uv[2 * (size_t)p] = u;
    out_uv[2 * (size_t)p + 1] = v;
    out_idx[p] = i;
  }
}

__device__ __forceinline__ void load_descriptor(const uint64_t* __restrict__ desc, uint32_t (&d)[8]) {
  const uint32_t* p = (const uint32_t*)desc;
#pragma unroll
  for (int q = 0; q < 8; q++) d[q] = p[q];
}

// view = blockIdx.y, keypoint = 4 * blockIdx.x + wave; result[k0 + k] = landmark index or -1 for the view's keypoints
// [k0, k0 + n_kp) = [kp_start[view], kp_start[view + 1]), against the view's row (stride n_lms) of compacted
// projections, n_proj_dev[view] of them (read through L2: a row is shared by every workgroup of the view; DESIGN.md
// "Landmark fusion" on why it is not staged through LDS).  The one-view host-buffer call passes its header as
// arguments: a null kp_start means [0, n_kp), a null n_proj_dev means n_proj.
__global__ __launch_bounds__(256) void find_matches_kernel(const int32_t* __restrict__ kp_start, int n_kp,
                                                           const double* __restrict__ kp_xy, const uint64_t* __restrict__ kp_desc,
                                                           const double* __restrict__ proj_uv, const int32_t* __restrict__ proj_lm,
                                                           const int32_t* __restrict__ n_proj_dev, int n_proj, int n_lms,
                                                           const int32_t* __restrict__ lm_obs_start,
                                                           const uint64_t* __restrict__ obs_desc, double max_dist_sq,
                                                           int threshold, double dist_2_best, int32_t* __restrict__ result) {
  const int view = blockIdx.y;
  const int k0 = kp_start ? kp_start[view] : 0;
  if (kp_start) n_kp = kp_start[view + 1] - k0;
  if (n_proj_dev) n_proj = n_proj_dev[view];
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= n_kp) return;  // wave-uniform
  const size_t kg = (size_t)k0 + (size_t)k;
  const size_t row = (size_t)view * (size_t)n_lms;
  uint32_t d[8];
  load_descriptor(kp_desc + 4 * kg, d);
  const int res = guided_search_wave(kp_xy[2 * kg], kp_xy[2 * kg + 1], d, proj_uv + 2 * row, proj_lm + row, n_proj, lm_obs_start,
                                     obs_desc, nullptr, max_dist_sq, threshold, dist_2_best, lane);
  if (lane == 0) result[kg] = res;
}

// The tracker's search (vsl_map_track_corners): the keypoints of a frame store slot (int32 positions, count on the
// device), the number of projected landmarks on the device, observation descriptors through obs_index into the map's
// descriptor pool.  result and mail_hdr are the caller's pinned mailbox: every slot below result_cap gets its landmark
// or -1 (nobody memsets the array), the header is (n_proj, the frame store's near-tie count, n_kp), and with mail_xy
// the keypoint's position rides along (the host needs it for PnP).
__global__ __launch_bounds__(256) void track_matches_kernel(const int32_t* __restrict__ kp_xy, const uint64_t* __restrict__ kp_desc,
                                                            const int32_t* __restrict__ n_kp_dev, int result_cap,
                                                            const double* __restrict__ proj_uv, const int32_t* __restrict__ proj_lm,
                                                            const int32_t* __restrict__ n_proj_dev,
                                                            const int32_t* __restrict__ lm_obs_start,
                                                            const uint64_t* __restrict__ obs_desc,
                                                            const int32_t* __restrict__ obs_index, double max_dist_sq,
                                                            int threshold, double dist_2_best, int32_t* __restrict__ result,
                                                            int32_t* __restrict__ mail_hdr, const int32_t* __restrict__ tie_count_dev,
                                                            int32_t* __restrict__ mail_xy) {
  const int n_kp = *n_kp_dev, n_proj = *n_proj_dev;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    mail_hdr[0] = n_proj;
    mail_hdr[1] = *tie_count_dev;
    mail_hdr[2] = n_kp;
  }
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= n_kp) {  // wave-uniform
    if (lane == 0 && k < result_cap) result[k] = -1;
    return;
  }
  const int x = kp_xy[2 * (size_t)k], y = kp_xy[2 * (size_t)k + 1];
  if (mail_xy && lane == 0) {
    mail_xy[2 * (size_t)k] = x;
    mail_xy[2 * (size_t)k + 1] = y;
  }
  uint32_t d[8];
  load_descriptor(kp_desc + 4 * (size_t)k, d);
  const int res = guided_search_wave((double)x, (double)y, d, proj_uv, proj_lm, n_proj, lm_obs_start, obs_desc, obs_index,
                                     max_dist_sq, threshold, dist_2_best, lane);
  if (lane == 0) result[k] = res;
}

// view = blockIdx.x: the matched keypoints of the view's range (as in find_matches_kernel: a null kp_start means
// [0, n_kp)), in feature order, as (feature, landmark) pairs at pairs[2 * k0 ..) and their number in n_pairs[view]
__global__ __launch_bounds__(1024) void compact_matches_kernel(const int32_t* __restrict__ kp_start, int n_kp,
                                                               const int32_t* __restrict__ result, int32_t* __restrict__ pairs,
                                                               int32_t* __restrict__ n_pairs) {
  const int k0 = kp_start ? kp_start[blockIdx.x] : 0;
  const int n = kp_start ? kp_start[blockIdx.x + 1] - k0 : n_kp;
  result += k0;
  pairs += 2 * (size_t)k0;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const int r = i < n ? result[i] : -1;
    int total;
    const int p = base + wg1024_ordered_slot(r >= 0, total);
    if (r >= 0) {
      pairs[2 * (size_t)p] = i;
      pairs[2 * (size_t)p + 1] = r;
    }
    base += total;
    __syncthreads();  // the next chunk rewrites the wave totals
  }
  if (threadIdx.x == 0) n_pairs[blockIdx.x] = base;
}

inline size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

}  // namespace

extern "C" int vsl_project_landmarks(vsl_ctx* ctx, const double* pose7, int cam_model, const double* intr8, int width,
                                     int height, const double* points, int n, double cam_z_threshold, double* proj_uv,
                                     int32_t* proj_idx, int* n_out) {
  if (!ctx || !pose7 || !intr8 || !n_out || n < 0 || (n > 0 && (!points || !proj_uv || !proj_idx)) || cam_model < 0 ||
      cam_model > 3)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_project_landmarks: bad arguments");
  *n_out = 0;
  if (n == 0) return VSL_OK;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n;
  void* d = nullptr;
  // pose (8) | intr (8) | points (3N) | uv (2N) | out_uv (2N) | out_idx (N i32) | n_out | keep (N u8)
  int rc = vsl_ctx_dscratch(ctx, 8 * (16 + 7 * N) + 4 * (N + 4) + N + 64, &d);
  if (rc) return rc;
  double* dpose = (double*)d;
  double* dintr = dpose + 8;
  double* dpts = dintr + 8;
  double* duv = dpts + 3 * N;
  double* douv = duv + 2 * N;
  int32_t* didx = (int32_t*)(douv + 2 * N);
  int32_t* dn = didx + N;
  uint8_t* dkeep = (uint8_t*)(dn + 4);
  VSL_HIP(ctx, hipMemcpyAsync(dpose, pose7, 56, hipMemcpyHostToDevice, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(dintr, intr8, 64, hipMemcpyHostToDevice, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(dpts, points, 24 * N, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(project_kernel, dim3((n + 1023) / 1024), dim3(1024), 0, ctx->stream, dpose, cam_model, dintr, width, height,
                     dpts, n, cam_z_threshold, duv, dkeep);
  hipLaunchKernelGGL(compact_projection_kernel, dim3(1), dim3(1024), 0, ctx->stream, duv, dkeep, n, douv, didx, dn);
  VSL_CHECK_LAUNCH(ctx);
  // one round trip: count and full-capacity outputs into pinned memory together
  void* hp = nullptr;
  rc = vsl_ctx_hpinned(ctx, 64 + 20 * N, &hp);
  if (rc) return rc;
  int32_t* hn = (int32_t*)hp;
  double* huv = (double*)((char*)hp + 64);
  int32_t* hidx = (int32_t*)(huv + 2 * N);
  VSL_HIP(ctx, hipMemcpyAsync(hn, dn, 4, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(huv, douv, 16 * N, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hidx, didx, 4 * N, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t m = hn[0];
  *n_out = m;
  if (m > 0) {
    std::memcpy(proj_uv, huv, 16 * (size_t)m);
    std::memcpy(proj_idx, hidx, 4 * (size_t)m);
  }
  return VSL_OK;
}

extern "C" int vsl_find_matches_landmarks(vsl_ctx* ctx, const double* kp_xy, const uint64_t* kp_desc, int n_kp,
                                          const double* proj_uv, const int32_t* proj_lm, int n_proj,
                                          const int32_t* lm_obs_start, int n_lms, const uint64_t* obs_desc,
                                          double match_max_dist_2d, int feature_match_threshold,
                                          double feature_match_dist_2_best, int32_t* pairs, int* n_out) {
  if (!ctx || !n_out || n_kp < 0 || n_proj < 0 || n_lms < 0 || (n_kp > 0 && (!kp_xy || !kp_desc || !pairs)) ||
      (n_proj > 0 && (!proj_uv || !proj_lm || !lm_obs_start)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_find_matches_landmarks: bad arguments");
  *n_out = 0;
  if (n_kp == 0 || n_proj == 0) return VSL_OK;
  for (int j = 0; j < n_proj; j++)
    if (proj_lm[j] < 0 || proj_lm[j] >= n_lms) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_find_matches_landmarks: landmark index %d out of range", proj_lm[j]);
  const int total = lm_obs_start[n_lms];
  if (total < 0 || (total > 0 && !obs_desc)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_find_matches_landmarks: bad observation arrays");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t K = (size_t)n_kp, P = (size_t)n_proj, L = (size_t)n_lms, T = (size_t)total;
  void* d = nullptr;
  int rc = vsl_ctx_dscratch(ctx, 8 * (2 * K + 4 * K + 2 * P + 4 * T) + 4 * (P + L + 1 + K + 2 * K + 4) + 64, &d);
  if (rc) return rc;
  double* dkxy = (double*)d;
  uint64_t* dkd = (uint64_t*)(dkxy + 2 * K);
  double* dpuv = (double*)(dkd + 4 * K);
  uint64_t* dod = (uint64_t*)(dpuv + 2 * P);
  int32_t* dplm = (int32_t*)(dod + 4 * T);
  int32_t* dstart = dplm + P;
  int32_t* dres = dstart + L + 1;
  int32_t* dpairs = dres + K;
  int32_t* dn = dpairs + 2 * K;
  VSL_HIP(ctx, hipMemcpyAsync(dkxy, kp_xy, 16 * K, hipMemcpyHostToDevice, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(dkd, kp_desc, 32 * K, hipMemcpyHostToDevice, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(dpuv, proj_uv, 16 * P, hipMemcpyHostToDevice, ctx->stream));
  if (T) VSL_HIP(ctx, hipMemcpyAsync(dod, obs_desc, 32 * T, hipMemcpyHostToDevice, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(dplm, proj_lm, 4 * P, hipMemcpyHostToDevice, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(dstart, lm_obs_start, 4 * (L + 1), hipMemcpyHostToDevice, ctx->stream));
  // one view: its header (keypoints [0, n_kp), n_proj projections) travels as kernel arguments
  hipLaunchKernelGGL(find_matches_kernel, dim3((n_kp + 3) / 4), dim3(256), 0, ctx->stream, (const int32_t*)nullptr, n_kp, dkxy, dkd,
                     dpuv, dplm, (const int32_t*)nullptr, n_proj, n_proj, dstart, dod, sqrt_less_threshold(match_max_dist_2d),
                     feature_match_threshold, feature_match_dist_2_best, dres);
  hipLaunchKernelGGL(compact_matches_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t*)nullptr, n_kp, dres, dpairs, dn);
  VSL_CHECK_LAUNCH(ctx);
  void* hp = nullptr;
  rc = vsl_ctx_hpinned(ctx, 64 + 8 * K, &hp);
  if (rc) return rc;
  int32_t* hn = (int32_t*)hp;
  int32_t* hpairs = (int32_t*)((char*)hp + 64);
  VSL_HIP(ctx, hipMemcpyAsync(hn, dn, 4, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipMemcpyAsync(hpairs, dpairs, 8 * K, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t m = hn[0];
  *n_out = m;
  if (m > 0) std::memcpy(pairs, hpairs, 8 * (size_t)m);
  return VSL_OK;
}

// ------------------------------------------------------------------------------------------------
// Device-resident map: landmark positions, the per-landmark lists of observation descriptors and the
// descriptor pool stay in HBM between frames; a frame is tracked against it with ONE call that chains
// projection, compaction and guided matching on the context's stream and returns only the matches.
// Same kernels, same results as vsl_project_landmarks + vsl_find_matches_landmarks on the same inputs
// (tests/test_vo_gpu.py::test_map_track_equals_host_buffer_path).
struct vsl_map {
  vsl_ctx* ctx = nullptr;
  int cap_lms = 0, cap_refs = 0, cap_pool = 0, cap_kp = 0;
  int n_lms = 0, n_refs = 0, n_pool = 0;
  double* points = nullptr;     // [cap_lms][3]
  int32_t* obs_start = nullptr;  // [cap_lms + 1]
  int32_t* obs_index = nullptr;  // [cap_refs] -> pool
  uint64_t* pool = nullptr;      // [cap_pool][4]
  // per-call scratch
  double* uv = nullptr;       // [cap_lms][2]
  double* out_uv = nullptr;   // [cap_lms][2]
  int32_t* out_idx = nullptr;  // [cap_lms]
  uint8_t* keep = nullptr;    // [cap_lms]
  double* pose_intr = nullptr;  // 16 doubles
  int32_t* counters = nullptr;  // [0] = n_proj, [1] = n_matches
  int32_t* result = nullptr;    // [cap_kp]
  int32_t* pairs = nullptr;     // [cap_kp][2]
  int32_t* gather_ids = nullptr;  // [cap_kp]
  unsigned long long* chain = nullptr;  // [cap_lms / 1024 + 1] running totals of project_compact_kernel
  int chain_cap = 0;
  unsigned int epoch = 0;
  int32_t* mailbox = nullptr;  // pinned host memory the matching kernel writes: [n_proj, tie_count, n_kp, pad | result[cap_kp]]
  int mailbox_cap = 0;
};

namespace {

template <class T>
int map_grow(vsl_ctx* ctx, T** p, size_t old_n, size_t new_n) {
  T* q = nullptr;
  VSL_HIP(ctx, hipMalloc((void**)&q, sizeof(T) * (new_n ? new_n : 1)));
  if (*p && old_n) VSL_HIP(ctx, hipMemcpyAsync(q, *p, sizeof(T) * old_n, hipMemcpyDeviceToDevice, ctx->stream));
  if (*p) {
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(*p);
  }
  *p = q;
  return VSL_OK;
}

int map_reserve_lms(vsl_map* m, int n, int refs) {
  vsl_ctx* ctx = m->ctx;
  int rc;
  if (n > m->cap_lms) {
    const int c = n + n / 2 + 1024;
    if ((rc = map_grow(ctx, &m->points, 0, 3 * (size_t)c))) return rc;
    if ((rc = map_grow(ctx, &m->obs_start, 0, (size_t)c + 1))) return rc;
    if ((rc = map_grow(ctx, &m->uv, 0, 2 * (size_t)c))) return rc;
    if ((rc = map_grow(ctx, &m->out_uv, 0, 2 * (size_t)c))) return rc;
    if ((rc = map_grow(ctx, &m->out_idx, 0, (size_t)c))) return rc;
    if ((rc = map_grow(ctx, &m->keep, 0, (size_t)c))) return rc;
    m->cap_lms = c;
  }
  if (refs > m->cap_refs) {
    const int c = refs + refs / 2 + 4096;
    if ((rc = map_grow(ctx, &m->obs_index, 0, (size_t)c))) return rc;
    m->cap_refs = c;
  }
  return VSL_OK;
}

int map_reserve_pool(vsl_map* m, int n) {
  if (n <= m->cap_pool) return VSL_OK;
  const int c = n + n / 2 + 4096;
  int rc = map_grow(m->ctx, &m->pool, 4 * (size_t)m->n_pool, 4 * (size_t)c);
  if (rc) return rc;
  m->cap_pool = c;
  return VSL_OK;
}

int map_reserve_kp(vsl_map* m, int n) {
  if (n <= m->cap_kp) return VSL_OK;
  int rc;
  if ((rc = map_grow(m->ctx, &m->result, 0, (size_t)n))) return rc;
  if ((rc = map_grow(m->ctx, &m->pairs, 0, 2 * (size_t)n))) return rc;
  if ((rc = map_grow(m->ctx, &m->gather_ids, 0, (size_t)n))) return rc;
  m->cap_kp = n;
  return VSL_OK;
}

__global__ void map_gather_desc_kernel(const uint64_t* __restrict__ frame_desc, const int32_t* __restrict__ ids, int n,
                                       uint64_t* __restrict__ pool_out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * n) return;
  pool_out[t] = frame_desc[4 * (size_t)ids[t >> 2] + (t & 3)];
}

}  // namespace

extern "C" int vsl_map_create(vsl_ctx* ctx, int cap_landmarks, int cap_descriptors, vsl_map** out) {
  if (!ctx || !out || cap_landmarks < 0 || cap_descriptors < 0) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_map_create: bad arguments");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  vsl_map* m = new vsl_map();
  m->ctx = ctx;
  int rc = map_reserve_lms(m, cap_landmarks > 0 ? cap_landmarks : 1, cap_descriptors > 0 ? cap_descriptors : 1);
  if (!rc) rc = map_reserve_pool(m, cap_descriptors > 0 ? cap_descriptors : 1);
  if (!rc) rc = map_grow(ctx, &m->pose_intr, 0, 16);
  if (!rc) rc = map_grow(ctx, &m->counters, 0, 4);
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return VSL_OK;
}

extern "C" void vsl_map_destroy(vsl_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  void* ptrs[] = {m->points, m->obs_start, m->obs_index, m->pool, m->uv, m->out_uv, m->out_idx, m->keep,
                  m->pose_intr, m->counters, m->result, m->pairs, m->gather_ids, m->chain};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (m->mailbox) (void)hipHostFree(m->mailbox);
  delete m;
}

extern "C" int vsl_map_append_descriptors(vsl_map* m, int n, const uint64_t* desc, int* first_index) {
  if (!m || n < 0 || (n > 0 && !desc) || !first_index) return VSL_ERR_INVALID;
  vsl_ctx* ctx = m->ctx;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = map_reserve_pool(m, m->n_pool + n);
  if (rc) return rc;
  *first_index = m->n_pool;
  if (n > 0) {
    VSL_HIP(ctx, hipMemcpyAsync(m->pool + 4 * (size_t)m->n_pool, desc, 32 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's buffer may go away
  }
  m->n_pool += n;
  return VSL_OK;
}

extern "C" int vsl_map_append_descriptors_from_frame(vsl_map* m, vsl_frames* f, int slot, int n, const int32_t* feature_ids,
                                                     int* first_index) {
  if (!m || !f || n < 0 || (n > 0 && !feature_ids) || !first_index || slot < 0 || slot >= f->max_images) return VSL_ERR_INVALID;
  vsl_ctx* ctx = m->ctx;
  for (int i = 0; i < n; i++)
    if (feature_ids[i] < 0 || feature_ids[i] >= f->F) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_map_append_descriptors_from_frame: feature id %d out of range", feature_ids[i]);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = map_reserve_pool(m, m->n_pool + n);
  if (!rc) rc = map_reserve_kp(m, n > f->F ? n : f->F);
  if (rc) return rc;
  if ((rc = vsl_resolve_ties(ctx, f, nullptr))) return rc;  // the descriptors copied must be final
  *first_index = m->n_pool;
  if (n > 0) {
    VSL_HIP(ctx, hipMemcpyAsync(m->gather_ids, feature_ids, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(map_gather_desc_kernel, dim3((4 * n + 255) / 256), dim3(256), 0, ctx->stream,
                       f->kp_desc + 4 * (size_t)slot * f->F, m->gather_ids, n, m->pool + 4 * (size_t)m->n_pool);
    VSL_CHECK_LAUNCH(ctx);
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));  // feature_ids is the caller's
  }
  m->n_pool += n;
  return VSL_OK;
}

extern "C" int vsl_map_set_landmarks(vsl_map* m, int n, const double* points, const int32_t* obs_start,
                                     const int32_t* obs_pool_index) {
  if (!m || n < 0 || (n > 0 && (!points || !obs_start))) return VSL_ERR_INVALID;
  vsl_ctx* ctx = m->ctx;
  const int refs = n > 0 ? obs_start[n] : 0;
  if (n > 0 && obs_start[0] != 0) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_map_set_landmarks: obs_start[0] must be 0");
  for (int i = 0; i < n; i++)
    if (obs_start[i + 1] < obs_start[i]) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_map_set_landmarks: obs_start not monotone at %d", i);
  if (refs > 0 && !obs_pool_index) return VSL_ERR_INVALID;
  for (int i = 0; i < refs; i++)
    if (obs_pool_index[i] < 0 || obs_pool_index[i] >= m->n_pool)
      return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_map_set_landmarks: descriptor index %d outside the pool (%d)", obs_pool_index[i], m->n_pool);
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = map_reserve_lms(m, n, refs);
  if (rc) return rc;
  if (n > 0) {
    VSL_HIP(ctx, hipMemcpyAsync(m->points, points, 24 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    VSL_HIP(ctx, hipMemcpyAsync(m->obs_start, obs_start, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (refs) VSL_HIP(ctx, hipMemcpyAsync(m->obs_index, obs_pool_index, 4 * (size_t)refs, hipMemcpyHostToDevice, ctx->stream));
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  m->n_lms = n;
  m->n_refs = refs;
  return VSL_OK;
}

extern "C" int vsl_map_info(const vsl_map* m, int* n_landmarks, int* n_observation_refs, int* n_descriptors) {
  if (!m) return VSL_ERR_INVALID;
  if (n_landmarks) *n_landmarks = m->n_lms;
  if (n_observation_refs) *n_observation_refs = m->n_refs;
  if (n_descriptors) *n_descriptors = m->n_pool;
  return VSL_OK;
}

extern "C" int vsl_map_track(vsl_map* m, vsl_frames* f, int slot, const double* pose7, int cam_model, const double* intr8,
                             int width, int height, double cam_z_threshold, double match_max_dist_2d,
                             int feature_match_threshold, double feature_match_dist_2_best, int32_t* pairs, int* n_pairs,
                             int* n_projected) {
  return vsl_map_track_corners(m, f, slot, pose7, cam_model, intr8, width, height, cam_z_threshold, match_max_dist_2d,
                               feature_match_threshold, feature_match_dist_2_best, pairs, n_pairs, n_projected, nullptr, nullptr);
}

// vsl_map_track + the slot's keypoint positions (corners_xy[2 * max_features], *n_corners) in the same round trip:
// what the host needs for PnP without a second download.
extern "C" int vsl_map_track_corners(vsl_map* m, vsl_frames* f, int slot, const double* pose7, int cam_model, const double* intr8,
                                     int width, int height, double cam_z_threshold, double match_max_dist_2d,
                                     int feature_match_threshold, double feature_match_dist_2_best, int32_t* pairs,
                                     int* n_pairs, int* n_projected, double* corners_xy, int* n_corners) {
  if (!m || !f || !pose7 || !intr8 || !n_pairs || slot < 0 || slot >= f->max_images || cam_model < 0 || cam_model > 3)
    return VSL_ERR_INVALID;
  vsl_ctx* ctx = m->ctx;
  *n_pairs = 0;
  if (n_projected) *n_projected = 0;
  if (n_corners) *n_corners = 0;
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = map_reserve_kp(m, f->F);
  if (rc) return rc;
  const int n = m->n_lms;
  if (n == 0) {
    if ((rc = vsl_resolve_ties(ctx, f, nullptr))) return rc;
    if (corners_xy && n_corners)
      return vsl_frames_download_keypoints(ctx, f, slot, f->F, corners_xy, nullptr, nullptr, n_corners);
    return VSL_OK;
  }
  // Two launches and one synchronisation per call (round 3; it was a tie-guard round trip, a pose upload, four kernels,
  // a memset and two copies): the pose travels as a kernel argument, projection + ordered compaction are one kernel,
  // the matching kernel writes its per-keypoint results, the projected count and the frame store's near-tie count
  // straight into pinned host memory, and the match list is compacted on the host (<= F entries).
  const int n_blocks = (n + 1023) / 1024;
  if (n_blocks + 1 > m->chain_cap) {
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (m->chain) (void)hipFree(m->chain);
    m->chain = nullptr;
    m->chain_cap = 0;
    const int cap = 2 * n_blocks + 64;
    VSL_HIP(ctx, hipMalloc((void**)&m->chain, 8 * (size_t)cap));
    VSL_HIP(ctx, hipMemsetAsync(m->chain, 0, 8 * (size_t)cap, ctx->stream));
    m->chain_cap = cap;
    m->epoch = 0;
  }
  if (3 * f->F + 4 > m->mailbox_cap) {
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (m->mailbox) (void)hipHostFree(m->mailbox);
    m->mailbox = nullptr;
    m->mailbox_cap = 0;
    VSL_HIP(ctx, hipHostMalloc((void**)&m->mailbox, 4 * (3 * (size_t)f->F + 4), hipHostMallocMapped | hipHostMallocCoherent));
    m->mailbox_cap = 3 * f->F + 4;
  }
  PoseIntr pi;
  for (int i = 0; i < 7; i++) pi.v[i] = pose7[i];
  pi.v[7] = 0;
  for (int i = 0; i < 8; i++) pi.v[8 + i] = intr8[i];
  if (++m->epoch == 0) {  // 2^32 calls later: the chain words of epoch 0 are the freshly cleared ones
    VSL_HIP(ctx, hipMemsetAsync(m->chain, 0, 8 * (size_t)m->chain_cap, ctx->stream));
    m->epoch = 1;
  }
  // chain position = blockIdx while every workgroup is resident from the start, an atomic ticket beyond (kernel header);
  // the ticket word is the last word of the chain allocation (zero between calls)
  unsigned int* ticket = (n_blocks > VO_CHAIN_RESIDENT_BLOCKS || ctx->vo_chain_ticket) ? (unsigned int*)(m->chain + (m->chain_cap - 1)) : nullptr;
  hipLaunchKernelGGL(project_compact_kernel, dim3(n_blocks), dim3(1024), 0, ctx->stream, pi, cam_model, width, height, m->points, n,
                     cam_z_threshold, m->out_uv, m->out_idx, m->counters, m->chain, m->epoch, ticket);
  int32_t* mail = m->mailbox;
  const double max_dist_sq = sqrt_less_threshold(match_max_dist_2d);
  for (int attempt = 0; attempt < 2; attempt++) {
    hipLaunchKernelGGL(track_matches_kernel, dim3((f->F + 3) / 4), dim3(256), 0, ctx->stream, f->kp_xy + 2 * (size_t)slot * f->F,
                       f->kp_desc + 4 * (size_t)slot * f->F, f->kp_count + slot, f->F, m->out_uv, m->out_idx, m->counters,
                       m->obs_start, m->pool, m->obs_index, max_dist_sq, feature_match_threshold, feature_match_dist_2_best,
                       mail + 4, mail, f->tie_count, corners_xy ? mail + 4 + f->F : (int32_t*)nullptr);
    VSL_CHECK_LAUNCH(ctx);
    VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // The descriptors of the slot must be final (rBRIEF near-tie guard, describe.hip).  The guard's count came along
    // with the results: zero (all but ~3 in a million frames) -> done, no second round trip; otherwise resolve the
    // ties the usual way and match once more.
    if (!f->ties_pending) break;
    if (mail[1] == 0) {
      f->ties_settled();
      break;
    }
    if ((rc = vsl_resolve_ties(ctx, f, nullptr))) return rc;
  }
  if (n_projected) *n_projected = mail[0];
  int np = 0;
  const int32_t* res = mail + 4;
  for (int k = 0; k < f->F; k++)
    if (res[k] >= 0) {
      if (!pairs) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_map_track: pairs is null");
      pairs[2 * np] = k;
      pairs[2 * np + 1] = res[k];
      np++;
    }
  *n_pairs = np;
  if (corners_xy && n_corners) {
    const int nk = mail[2] < f->F ? mail[2] : f->F;
    const int32_t* xy = mail + 4 + f->F;
    for (int k = 0; k < 2 * nk; k++) corners_xy[k] = (double)xy[k];
    *n_corners = nk;
  }
  return VSL_OK;
}

// ------------------------------------------------------------------------------------------------
// The guided search of landmark fusion after a loop closure, for ALL views in one call (DESIGN.md "Landmark fusion"):
// vsl_fuse_search(view v) == vsl_project_landmarks(pose v) followed by vsl_find_matches_landmarks(keypoints of v), pair
// for pair -- the same four kernels with a view dimension.  One packed upload (landmark points and observation
// descriptors once, shared by all views), four launches on the context's stream with nothing between them, one download.
// No workgroup waits for another one: every scan is private to one workgroup, and the prefix over the <= 64 per-view
// pair counts is taken by the host while it copies the segments out of the pinned download buffer.
extern "C" int vsl_fuse_search(vsl_ctx* ctx, int n_views, const double* pose7, int cam_model, const double* intr8, int width,
                               int height, const int32_t* kp_start, const double* kp_xy, const uint64_t* kp_desc, int n_lms,
                               const double* points, const int32_t* lm_obs_start, const uint64_t* obs_desc,
                               double cam_z_threshold, double match_max_dist_2d, int feature_match_threshold,
                               double feature_match_dist_2_best, int32_t* pairs, int32_t* pair_start, int32_t* n_projected) {
  if (!ctx) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: null context");
  if (n_views < 0 || n_lms < 0 || cam_model < 0 || cam_model > 3 || !intr8 || !pair_start)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: bad arguments");
  if (n_views > VSL_FUSE_MAX_VIEWS)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: %d views (at most %d)", n_views, VSL_FUSE_MAX_VIEWS);
  if (n_views > 0 && (!pose7 || !kp_start)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: null pose7 / kp_start with %d views", n_views);
  if (n_lms > 0 && (!points || !lm_obs_start)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: null points / lm_obs_start with %d landmarks", n_lms);
  int max_kp = 0;
  if (n_views > 0) {
    if (kp_start[0] != 0) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: kp_start[0] must be 0");
    for (int v = 0; v < n_views; v++) {
      if (kp_start[v + 1] < kp_start[v]) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: kp_start not monotone at view %d", v);
      if (kp_start[v + 1] - kp_start[v] > max_kp) max_kp = kp_start[v + 1] - kp_start[v];
    }
  }
  const int n_kp = n_views > 0 ? kp_start[n_views] : 0;
  if (n_kp > 0 && (!kp_xy || !kp_desc || !pairs)) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: null kp_xy / kp_desc / pairs with %d keypoints", n_kp);
  int n_obs = 0;
  if (n_lms > 0) {
    if (lm_obs_start[0] != 0) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: lm_obs_start[0] must be 0");
    for (int l = 0; l < n_lms; l++)
      if (lm_obs_start[l + 1] < lm_obs_start[l]) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: lm_obs_start not monotone at landmark %d", l);
    n_obs = lm_obs_start[n_lms];
  }
  if (n_obs > 0 && !obs_desc) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_fuse_search: null obs_desc with %d observations", n_obs);
  for (int v = 0; v <= n_views; v++) pair_start[v] = 0;
  if (n_projected)
    for (int v = 0; v < n_views; v++) n_projected[v] = 0;
  if (n_views == 0 || n_lms == 0) return VSL_OK;

  VSL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t V = (size_t)n_views, N = (size_t)n_lms, K = (size_t)n_kp, T = (size_t)n_obs;
  // the upload block, one layout on the host (pinned) and on the device:
  //   pose (8 V) | intr (8) | points (3 N) | kp_xy (2 K) | kp_desc (4 K) | obs_desc (4 T) | kp_start (V + 1) | lm_obs_start (N + 1)
  const size_t o_pose = 0, o_intr = o_pose + 64 * V, o_pts = o_intr + 64, o_kxy = up64(o_pts + 24 * N), o_kd = up64(o_kxy + 16 * K),
               o_od = up64(o_kd + 32 * K), o_ks = up64(o_od + 32 * T), o_ls = up64(o_ks + 4 * (V + 1)),
               up_bytes = up64(o_ls + 4 * (N + 1));
  // the download block: n_proj (V) | n_pairs (V) | pairs (2 K, every view's segment at its kp_start)
  const size_t o_np = 0, o_nm = up64(4 * V), o_pairs = up64(o_nm + 4 * V), down_bytes = up64(o_pairs + 8 * K);
  // device-only scratch: uv (2 V N) | out_uv (2 V N) | out_idx (V N) | result (K) | keep (V N)
  const size_t o_uv = 0, o_ouv = o_uv + up64(16 * V * N), o_oidx = o_ouv + up64(16 * V * N), o_res = o_oidx + up64(4 * V * N),
               o_keep = o_res + up64(4 * K), scr_bytes = o_keep + up64(V * N);
  void* dv = nullptr;
  int rc = vsl_ctx_dscratch(ctx, up_bytes + down_bytes + scr_bytes, &dv);
  if (rc) return rc;
  void* hv = nullptr;
  if ((rc = vsl_ctx_hpinned(ctx, up_bytes + down_bytes, &hv))) return rc;
  char* h_up = (char*)hv;
  char* h_down = h_up + up_bytes;
  char* d_up = (char*)dv;
  char* d_down = d_up + up_bytes;
  char* d_scr = d_down + down_bytes;

  for (size_t v = 0; v < V; v++) {
    std::memcpy(h_up + o_pose + 64 * v, pose7 + 7 * v, 56);
    std::memset(h_up + o_pose + 64 * v + 56, 0, 8);
  }
  std::memcpy(h_up + o_intr, intr8, 64);
  std::memcpy(h_up + o_pts, points, 24 * N);
  if (K) std::memcpy(h_up + o_kxy, kp_xy, 16 * K);
  if (K) std::memcpy(h_up + o_kd, kp_desc, 32 * K);
  if (T) std::memcpy(h_up + o_od, obs_desc, 32 * T);
  std::memcpy(h_up + o_ks, kp_start, 4 * (V + 1));
  std::memcpy(h_up + o_ls, lm_obs_start, 4 * (N + 1));
  VSL_HIP(ctx, hipMemcpyAsync(d_up, h_up, up_bytes, hipMemcpyHostToDevice, ctx->stream));

  const double* d_pose = (const double*)(d_up + o_pose);
  const double* d_intr = (const double*)(d_up + o_intr);
  const double* d_pts = (const double*)(d_up + o_pts);
  const double* d_kxy = (const double*)(d_up + o_kxy);
  const uint64_t* d_kd = (const uint64_t*)(d_up + o_kd);
  const uint64_t* d_od = (const uint64_t*)(d_up + o_od);
  const int32_t* d_ks = (const int32_t*)(d_up + o_ks);
  const int32_t* d_ls = (const int32_t*)(d_up + o_ls);
  int32_t* d_np = (int32_t*)(d_down + o_np);
  int32_t* d_nm = (int32_t*)(d_down + o_nm);
  int32_t* d_pairs = (int32_t*)(d_down + o_pairs);
  double* d_uv = (double*)(d_scr + o_uv);
  double* d_ouv = (double*)(d_scr + o_ouv);
  int32_t* d_oidx = (int32_t*)(d_scr + o_oidx);
  int32_t* d_res = (int32_t*)(d_scr + o_res);
  uint8_t* d_keep = (uint8_t*)(d_scr + o_keep);

  hipLaunchKernelGGL(project_kernel, dim3((n_lms + 1023) / 1024, n_views), dim3(1024), 0, ctx->stream, d_pose, cam_model, d_intr,
                     width, height, d_pts, n_lms, cam_z_threshold, d_uv, d_keep);
  hipLaunchKernelGGL(compact_projection_kernel, dim3(n_views), dim3(1024), 0, ctx->stream, d_uv, d_keep, n_lms, d_ouv, d_oidx, d_np);
  if (max_kp > 0)
    hipLaunchKernelGGL(find_matches_kernel, dim3((max_kp + 3) / 4, n_views), dim3(256), 0, ctx->stream, d_ks, 0, d_kxy, d_kd, d_ouv,
                       d_oidx, d_np, 0, n_lms, d_ls, d_od, sqrt_less_threshold(match_max_dist_2d), feature_match_threshold,
                       feature_match_dist_2_best, d_res);
  hipLaunchKernelGGL(compact_matches_kernel, dim3(n_views), dim3(1024), 0, ctx->stream, d_ks, 0, d_res, d_pairs, d_nm);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpyAsync(h_down, d_down, down_bytes, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));

  const int32_t* h_np = (const int32_t*)(h_down + o_np);
  const int32_t* h_nm = (const int32_t*)(h_down + o_nm);
  const int32_t* h_pairs = (const int32_t*)(h_down + o_pairs);
  for (size_t v = 0; v < V; v++) {
    if (n_projected) n_projected[v] = h_np[v];
    const int32_t m = h_nm[v];
    if (m > 0) std::memcpy(pairs + 2 * (size_t)pair_start[v], h_pairs + 2 * (size_t)kp_start[v], 8 * (size_t)m);
    pair_start[v + 1] = pair_start[v] + m;
  }
  return VSL_OK;
}
