// fuse.hip -- the guided search of landmark fusion after a loop closure, for ALL views in one call (DESIGN.md
// "Landmark fusion").
//
// vsl_fuse_search(view v) == vsl_project_landmarks(pose v) followed by vsl_find_matches_landmarks(keypoints of v), pair
// for pair, for every view of a covisibility neighbourhood at once: one packed upload (landmark points and observation
// descriptors once, shared by all views), four launches on the context's stream with nothing between them, one download.
//
//   fuse_project_kernel   grid (1024-landmark chunk, view): fp64 projection in the oracle's operation order -> keep, uv
//   fuse_compact_kernel   one workgroup per view loops over its chunks: order-preserving compaction (ascending landmark
//                         index inside a view -- the order that decides ties in the search)
//   fuse_search_kernel    grid (4 keypoints, view), one wavefront per keypoint: the radius test, the per-landmark minimum
//                         Hamming distance and the streaming top-2 of find_matches_kernel (vo.hip: libstdc++'s
//                         partial_sort(first, first + 2, last) as a state machine)
//   fuse_pairs_kernel     one workgroup per view: (feature, landmark) pairs in feature order into the view's own
//                         segment + their count
//
// No workgroup waits for another one: every scan is private to one workgroup (the chained look-back of
// project_compact_kernel needs ONE chain per grid for its forward-progress argument), and the prefix over the <= 64
// per-view pair counts is taken by the host while it copies the segments out of the pinned download buffer.
#include "cam_device.h"
#include "vsl_common.h"

#define VSL_FUSE_MAX_VIEWS 64

namespace {

__global__ __launch_bounds__(1024) void fuse_project_kernel(const double* __restrict__ pose8, int model,
                                                            const double* __restrict__ intr, int width, int height,
                                                            const double* __restrict__ points, int n, double z_thr,
                                                            double* __restrict__ uv, uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * 1024 + threadIdx.x;
  if (i >= n) return;
  const double* pose = pose8 + 8 * (size_t)blockIdx.y;
  const size_t o = (size_t)blockIdx.y * (size_t)n + (size_t)i;
  const double qi[4] = {-pose[0], -pose[1], -pose[2], pose[3]};
  const double nt[3] = {pose[4] * -1.0, pose[5] * -1.0, pose[6] * -1.0};
  double ti[3], rp[3];
  quat_rotate_d(qi, nt, ti);
  const double p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
  quat_rotate_d(qi, p, rp);
  const double pc[3] = {rp[0] + ti[0], rp[1] + ti[1], rp[2] + ti[2]};
  bool ok = !(pc[2] < z_thr);
  double u = 0, v = 0;
  if (ok) {
    project_exact(model, intr, pc[0], pc[1], pc[2], u, v);
    ok = !(u > (double)width || v > (double)height || u < 0 || v < 0);
  }
  uv[2 * o] = u;
  uv[2 * o + 1] = v;
  keep[o] = ok ? 1 : 0;
}

// view = blockIdx.x; the pattern of compact_projection_kernel (vo.hip) on the view's row of uv / keep
__global__ __launch_bounds__(1024) void fuse_compact_kernel(const double* __restrict__ uv, const uint8_t* __restrict__ keep, int n,
                                                            double* __restrict__ out_uv, int32_t* __restrict__ out_idx,
                                                            int32_t* __restrict__ n_proj) {
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  const size_t row = (size_t)blockIdx.x * (size_t)n;
  uv += 2 * row;
  keep += row;
  out_uv += 2 * row;
  out_idx += row;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const bool ok = i < n && keep[i];
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; w++) off += wave_tot[w];
    if (ok) {
      const int p = off + __popcll(m & ((1ull << lane) - 1ull));
      out_uv[2 * (size_t)p] = uv[2 * (size_t)i];
      out_uv[2 * (size_t)p + 1] = uv[2 * (size_t)i + 1];
      out_idx[p] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; w++) t += wave_tot[w];
      base_s += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) n_proj[blockIdx.x] = base_s;
}

// view = blockIdx.y, keypoint = 4 * blockIdx.x + wave; result[kp_start[view] + k] = landmark index or -1.  The body is
// find_matches_kernel's (vo.hip), on the view's keypoints and the view's row of compacted projections (read through L2:
// a row is shared by every workgroup of the view; DESIGN.md "Landmark fusion" on why it is not staged through LDS).
__global__ __launch_bounds__(256) void fuse_search_kernel(const int32_t* __restrict__ kp_start, const double* __restrict__ kp_xy,
                                                          const uint64_t* __restrict__ kp_desc,
                                                          const double* __restrict__ proj_uv_all,
                                                          const int32_t* __restrict__ proj_lm_all,
                                                          const int32_t* __restrict__ n_proj_dev, int n_lms,
                                                          const int32_t* __restrict__ lm_obs_start,
                                                          const uint64_t* __restrict__ obs_desc, double max_dist_sq,
                                                          int threshold, double dist_2_best, int32_t* __restrict__ result) {
  const int view = blockIdx.y;
  const int k0 = kp_start[view];
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= kp_start[view + 1] - k0) return;  // wave-uniform
  const size_t kg = (size_t)k0 + (size_t)k;
  const size_t row = (size_t)view * (size_t)n_lms;
  const double* __restrict__ proj_uv = proj_uv_all + 2 * row;
  const int32_t* __restrict__ proj_lm = proj_lm_all + row;
  const int n_proj = n_proj_dev[view];
  const double kx = kp_xy[2 * kg], ky = kp_xy[2 * kg + 1];
  uint32_t d[8];
  {
    const uint32_t* p = (const uint32_t*)(kp_desc + 4 * kg);
#pragma unroll
    for (int q = 0; q < 8; q++) d[q] = p[q];
  }
  int count = 0, top_d = 0, other_d = 0, other_id = 0;
  for (int base = 0; base < n_proj; base += 64) {
    const int j = base + lane;
    bool hit = false;
    if (j < n_proj) {
      const double dx = kx - proj_uv[2 * (size_t)j], dy = ky - proj_uv[2 * (size_t)j + 1];
      hit = dx * dx + dy * dy < max_dist_sq;  // sqrt(..) < match_max_dist_2d, decision for decision (sqrt_less_threshold)
    }
    unsigned long long mask = __ballot(hit);
    while (mask) {
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int l = proj_lm[base + b];
      const int o0 = lm_obs_start[l], o1 = lm_obs_start[l + 1];
      int best = 256;  // minimal_dist, vo_utils.h:116
      for (int o = o0 + lane; o < o1; o += 64) {
        const uint32_t* od = (const uint32_t*)(obs_desc + 4 * (size_t)o);
        int dist = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) dist += __builtin_popcount(d[q] ^ od[q]);
        best = min(best, dist);
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) best = min(best, __shfl_xor(best, s));
      // libstdc++ partial_sort(first, first + 2, last) as a streaming state machine (vo.hip file header)
      if (count == 0) {
        other_d = best;
        other_id = l;
      } else if (count == 1) {
        if (best < other_d) {
          top_d = other_d;
          other_d = best;
          other_id = l;
        } else {
          top_d = best;
        }
      } else if (best < top_d) {
        if (other_d < best) {
          top_d = best;
        } else {
          top_d = other_d;
          other_d = best;
          other_id = l;
        }
      }
      count++;
    }
  }
  if (lane == 0) {
    int res = -1;
    if (count > 0 && !(other_d >= threshold)) {
      const double second = count < 2 ? 256.0 : (double)top_d;  // vo_utils.h:146-160
      if (!(second < (double)other_d * dist_2_best)) res = other_id;
    }
    result[kg] = res;
  }
}

// view = blockIdx.x: the matched keypoints of the view, in feature order, as (feature, landmark) pairs at
// pairs[2 * kp_start[view] ..) and their number in n_pairs[view]
__global__ __launch_bounds__(1024) void fuse_pairs_kernel(const int32_t* __restrict__ kp_start, const int32_t* __restrict__ result,
                                                          int32_t* __restrict__ pairs, int32_t* __restrict__ n_pairs) {
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  const int k0 = kp_start[blockIdx.x];
  const int n = kp_start[blockIdx.x + 1] - k0;
  result += k0;
  pairs += 2 * (size_t)k0;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const int r = i < n ? result[i] : -1;
    const bool ok = r >= 0;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; w++) off += wave_tot[w];
    if (ok) {
      const int p = off + __popcll(m & ((1ull << lane) - 1ull));
      pairs[2 * (size_t)p] = i;
      pairs[2 * (size_t)p + 1] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; w++) t += wave_tot[w];
      base_s += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) n_pairs[blockIdx.x] = base_s;
}

inline size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

}  // namespace

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

  hipLaunchKernelGGL(fuse_project_kernel, dim3((n_lms + 1023) / 1024, n_views), dim3(1024), 0, ctx->stream, d_pose, cam_model,
                     d_intr, width, height, d_pts, n_lms, cam_z_threshold, d_uv, d_keep);
  hipLaunchKernelGGL(fuse_compact_kernel, dim3(n_views), dim3(1024), 0, ctx->stream, d_uv, d_keep, n_lms, d_ouv, d_oidx, d_np);
  if (max_kp > 0)
    hipLaunchKernelGGL(fuse_search_kernel, dim3((max_kp + 3) / 4, n_views), dim3(256), 0, ctx->stream, d_ks, d_kxy, d_kd, d_ouv,
                       d_oidx, d_np, n_lms, d_ls, d_od, sqrt_less_threshold(match_max_dist_2d), feature_match_threshold,
                       feature_match_dist_2_best, d_res);
  hipLaunchKernelGGL(fuse_pairs_kernel, dim3(n_views), dim3(1024), 0, ctx->stream, d_ks, d_res, d_pairs, d_nm);
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
