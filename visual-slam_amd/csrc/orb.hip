// orb.hip -- the ORB front end behind compute_bow_vector (include/visnav/keypoints.h:243-254:
// cv::ORB::create(num_features, 1.2, 8, 19, 0, 2, cv::ORB::FAST_SCORE)->detectAndCompute), SURVEY.md 8(f) rank 3.
//
// cv::ORB is [upstream] OpenCV; the arithmetic conventions this file implements are spelled out in
// oracle/orc_orb.cpp (parity with the OpenCV binary is unpinned; parity with that restatement is bit-exact
// and tested).  One set of kernels works on a pass of k images at once: the image index rides in the grid and every
// array is [image][...], so one launch (and one memset, one copy) covers a stage of the whole pass.  A pass takes its
// images from the frame store (vsl_frames_bow_vectors); vsl_orb_detect_describe -- the reference runs
// this once per keyframe -- is a pass of one image that comes from the host.  The stages:
//   pyramid (7 chained bilinear resizes, OpenCV's 8-bit fixed-point weights)  ->  per level: FAST-9/16
//   score image, strict 3x3 non-maximum suppression + border filter + score histogram, retainBest by the
//   histogram cut with an order-preserving compaction (count / scan / emit over 1024-pixel chunks), 7x7 Gaussian blur  ->
//   intensity-centroid orientation (one wavefront per keypoint)  ->  rotated BRIEF tests on the blurred
//   level (one thread per descriptor byte).  cos / sin of the keypoint angles are evaluated by the host's
//   libm between the last two kernels (device cos/sin are not bit-identical to glibc).
#include <algorithm>
#include <cmath>
#include <vector>

#include "vsl_common.h"

namespace {

#define ORB_LEVELS 8
#define ORB_EDGE 19
#define ORB_FAST_THR 20
#define ORB_HALF_PATCH 15

struct OrbPat {
  int xa, ya, xb, yb;
};
__constant__ OrbPat c_orb_pattern[256] = {
#include "rbrief_pattern.inc"
};
__constant__ int c_umax[16];
__constant__ float c_gauss7[7];

__device__ __forceinline__ int d_reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

struct OrbLevels {
  int W[ORB_LEVELS], H[ORB_LEVELS];
  int quota[ORB_LEVELS];
  int seg_base[ORB_LEVELS];  // first keypoint slot of the level's output segment
  int seg_cap[ORB_LEVELS];
  size_t pix_off[ORB_LEVELS];  // offset of the level in the pyramid-shaped buffers
  float scale[ORB_LEVELS];
  int chunk_base[ORB_LEVELS + 1];  // 1024-pixel chunks of the level = [chunk_base[l], chunk_base[l + 1])
};

__device__ __forceinline__ int orb_level_of_chunk(const OrbLevels& L, int chunk) {
  int l = 0;
  while (l + 1 < ORB_LEVELS && chunk >= L.chunk_base[l + 1]) l++;
  return l;
}

__device__ __forceinline__ float d_fast_atan2(float y, float x) {
  const float p1 = 0.9997878412794807f * (float)(180 / M_PI), p3 = -0.3258083974640975f * (float)(180 / M_PI),
              p5 = 0.1555786518463281f * (float)(180 / M_PI), p7 = -0.04432655554792128f * (float)(180 / M_PI);
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + (float)2.220446049250313e-16);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + (float)2.220446049250313e-16);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

bool g_orb_tables_ready[16] = {false};

int orb_upload_tables(vsl_ctx* ctx) {
  if (ctx->device >= 0 && ctx->device < 16 && g_orb_tables_ready[ctx->device]) return VSL_OK;
  int umax[16] = {0};
  const int hp = ORB_HALF_PATCH;
  const int vmax = (int)std::floor(hp * std::sqrt(2.0) / 2 + 1), vmin = (int)std::ceil(hp * std::sqrt(2.0) / 2);
  for (int v = 0; v <= vmax; v++) umax[v] = (int)std::lrint(std::sqrt((double)hp * hp - v * v));
  for (int v = hp, v0 = 0; v >= vmin; --v) {
    while (umax[v0] == umax[v0 + 1]) ++v0;
    umax[v] = v0;
    ++v0;
  }
  float k[7];
  double kd[7], sum = 0;
  for (int i = 0; i < 7; i++) {
    const double x = i - 3;
    kd[i] = std::exp(-x * x / (2.0 * 2.0 * 2.0));
    sum += kd[i];
  }
  for (int i = 0; i < 7; i++) k[i] = (float)(kd[i] / sum);
  VSL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_umax), umax, sizeof(umax)));
  VSL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_gauss7), k, sizeof(k)));
  if (ctx->device >= 0 && ctx->device < 16) g_orb_tables_ready[ctx->device] = true;
  return VSL_OK;
}

// seg_base / n_slots from seg_cap
int orb_place_segments(OrbLevels& L) {
  int n_slots = 0;
  for (int l = 0; l < ORB_LEVELS; l++) {
    L.seg_base[l] = n_slots;
    n_slots += L.seg_cap[l];
  }
  return n_slots;
}

// the geometry of one image's pass: levels, quotas, first keypoint segments, 1024-pixel chunks
struct OrbPlan {
  OrbLevels L;
  size_t total_pix;
  int n_slots, n_chunks;
};

void orb_plan_levels(int w, int h, int nfeatures, OrbPlan& P) {
  OrbLevels& L = P.L;
  P.total_pix = 0;
  const float factor = (float)(1.0 / 1.2f);
  float ndesired = (float)(nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)ORB_LEVELS)));
  int sum = 0;
  for (int l = 0; l < ORB_LEVELS; l++) {
    const float s = (float)std::pow((double)1.2f, (double)l);
    L.scale[l] = s;
    L.W[l] = (int)std::lrintf((float)w / s);
    L.H[l] = (int)std::lrintf((float)h / s);
    if (l < ORB_LEVELS - 1) {
      L.quota[l] = (int)std::lrintf(ndesired);
      sum += L.quota[l];
      ndesired *= factor;
    } else {
      L.quota[l] = nfeatures - sum > 0 ? nfeatures - sum : 0;
    }
    L.pix_off[l] = P.total_pix;
    P.total_pix += (size_t)L.W[l] * L.H[l];
    P.total_pix = (P.total_pix + 255) & ~(size_t)255;
    L.seg_cap[l] = 2 * L.quota[l] + 64;  // enough unless more than quota + 64 keypoints tie with the last one kept
  }
  P.n_slots = orb_place_segments(L);
  L.chunk_base[0] = 0;
  for (int l = 0; l < ORB_LEVELS; l++) L.chunk_base[l + 1] = L.chunk_base[l] + (L.W[l] * L.H[l] + 1023) / 1024;
  P.n_chunks = L.chunk_base[ORB_LEVELS];
}

bool orb_image_args_ok(vsl_ctx* ctx, const uint8_t* img, int w, int h, size_t pitch) {
  return ctx && img && w >= 64 && h >= 64 && pitch >= (size_t)w;
}

// The device arrays of a pass of k images.  The level geometry is one OrbLevels for the whole pass; what differs per
// image -- the keypoint segments once an image overflowed its first ones, and the place of its features in the pass's
// compact arrays -- is a VslOrbImgSeg record.
struct OrbBatchDev {
  uint8_t *pyr, *score, *flag, *blurred;  // [k][pix_stride]
  float* tmp;                             // [k][pix_stride]
  int* ints;                              // [k][n_ints]: hist (256 x levels) | level_count | cuts | level_full | pad
  int32_t *chunk_count, *chunk_offset;    // [k][n_chunks]
  int32_t *kp_xy, *kp_sl;                 // [k][slot_stride] keypoint slots
  float* angle;                           // [k][slot_stride]
  float* cs;                              // [rows][2]  compact (feature order)
  uint8_t* desc;                          // [rows][32] compact
  VslOrbImgSeg* seg;                      // [k]
  int32_t* img_list;                      // [k] images of the second emit
  size_t pix_stride;
  int n_ints, n_chunks, slot_stride;
};
#define ORB_INTS_COUNT (256 * ORB_LEVELS)
#define ORB_INTS_CUTS (256 * ORB_LEVELS + ORB_LEVELS)
#define ORB_INTS_FULL (256 * ORB_LEVELS + 2 * ORB_LEVELS)

// one pyramid level from the one above it, blockIdx.z = image
__global__ void orb_resize_kernel(OrbBatchDev D, size_t src_off, int sw, int sh, size_t dst_off, int dw, int dh, double scale_x,
                                  double scale_y) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= dw) return;
  const uint8_t* src = D.pyr + blockIdx.z * D.pix_stride + src_off;
  uint8_t* dst = D.pyr + blockIdx.z * D.pix_stride + dst_off;
  float fx = (float)((dx + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= sx;
  if (sx < 0) {
    fx = 0;
    sx = 0;
  }
  if (sx >= sw - 1) {
    fx = 0;
    sx = sw - 1;
  }
  float fy = (float)((dy + 0.5) * scale_y - 0.5);
  const int sy = (int)floorf(fy);
  fy -= sy;
  const int a0 = (short)(int)rintf((1.f - fx) * 2048.f), a1 = (short)(int)rintf(fx * 2048.f);
  const int b0 = (short)(int)rintf((1.f - fy) * 2048.f), b1 = (short)(int)rintf(fy * 2048.f);
  const int sy0 = min(max(sy, 0), sh - 1), sy1 = min(max(sy + 1, 0), sh - 1);
  const int sx1 = min(sx + 1, sw - 1);
  const int S0 = src[(size_t)sy0 * sw + sx] * a0 + src[(size_t)sy0 * sw + sx1] * a1;
  const int S1 = src[(size_t)sy1 * sw + sx] * a0 + src[(size_t)sy1 * sw + sx1] * a1;
  const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
  dst[(size_t)dy * dw + dx] = (uint8_t)min(max(v, 0), 255);
}

// FAST-9/16 score of every pixel: the largest threshold at which it is still a corner, 0 if it is not one at
// ORB_FAST_THR.  16 x 16 pixel tiles staged in LDS with a 3-pixel apron.
// All levels of all images in one launch: blockIdx.z = image * ORB_LEVELS + level in the four image-shaped stages, the
// grid is sized for level 0 and the workgroups beyond a smaller level's extent leave at once.
__global__ __launch_bounds__(256) void orb_fast_kernel(OrbLevels L, OrbBatchDev D) {
  __shared__ uint8_t tile[22][24];
  const int l = blockIdx.z % ORB_LEVELS, W = L.W[l], H = L.H[l];
  const size_t img_off = (size_t)(blockIdx.z / ORB_LEVELS) * D.pix_stride + L.pix_off[l];
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  if (x0 >= W || y0 >= H) return;
  const uint8_t* img = D.pyr + img_off;
  uint8_t* score = D.score + img_off;
  for (int t = threadIdx.x; t < 22 * 22; t += 256) {
    const int ty = t / 22, tx = t - ty * 22;
    const int gx = min(max(x0 + tx - 3, 0), W - 1), gy = min(max(y0 + ty - 3, 0), H - 1);
    tile[ty][tx] = img[(size_t)gy * W + gx];
  }
  __syncthreads();
  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= W || y >= H) return;
  int out = 0;
  if (x >= 3 && y >= 3 && x < W - 3 && y < H - 3) {
    const int cx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    const int cy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int v = tile[ly + 3][lx + 3];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] = (int)tile[ly + 3 + cy[k]][lx + 3 + cx[k]] - v;
    int best = -1;
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int mn = 1 << 20, mx = -(1 << 20);
#pragma unroll
      for (int k = 0; k < 9; k++) {
        const int dv = d[(s + k) & 15];
        mn = min(mn, dv);
        mx = max(mx, dv);
      }
      best = max(best, max(mn, -mx));
    }
    out = best > ORB_FAST_THR ? best - 1 : 0;
  }
  score[(size_t)y * W + x] = (uint8_t)out;
}

// strict 3x3 maximum + border filter; flags the survivors and histograms their scores
__global__ void orb_nms_kernel(OrbLevels L, OrbBatchDev D) {
  const int l = blockIdx.z % ORB_LEVELS, img = blockIdx.z / ORB_LEVELS, W = L.W[l], H = L.H[l];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W || y >= H) return;
  const size_t img_off = (size_t)img * D.pix_stride + L.pix_off[l];
  const uint8_t* score = D.score + img_off;
  uint8_t* flag = D.flag + img_off;
  int* hist = D.ints + (size_t)img * D.n_ints + 256 * l;
  uint8_t f = 0;
  if (x >= ORB_EDGE && y >= ORB_EDGE && x < W - ORB_EDGE && y < H - ORB_EDGE) {
    const int s = score[(size_t)y * W + x];
    if (s > 0) {
      bool ok = true;
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++)
          if (dx || dy) ok = ok && (s > score[(size_t)(y + dy) * W + x + dx]);
      if (ok) {
        f = 1;
        atomicAdd(&hist[s], 1);
      }
    }
  }
  flag[(size_t)y * W + x] = f;
}

__global__ void orb_blur_rows_kernel(OrbLevels L, OrbBatchDev D) {
  const int l = blockIdx.z % ORB_LEVELS, W = L.W[l], H = L.H[l];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W || y >= H) return;
  const size_t img_off = (size_t)(blockIdx.z / ORB_LEVELS) * D.pix_stride + L.pix_off[l];
  const uint8_t* src = D.pyr + img_off;
  float* tmp = D.tmp + img_off;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 7; i++) s = s + c_gauss7[i] * (float)src[(size_t)y * W + d_reflect101(x + i - 3, W)];
  tmp[(size_t)y * W + x] = s;
}

__global__ void orb_blur_cols_kernel(OrbLevels L, OrbBatchDev D) {
  const int l = blockIdx.z % ORB_LEVELS, W = L.W[l], H = L.H[l];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W || y >= H) return;
  const size_t img_off = (size_t)(blockIdx.z / ORB_LEVELS) * D.pix_stride + L.pix_off[l];
  const float* tmp = D.tmp + img_off;
  uint8_t* dst = D.blurred + img_off;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 7; i++) s = s + c_gauss7[i] * tmp[(size_t)d_reflect101(y + i - 3, H) * W + x];
  const int v = (int)rintf(s);
  dst[(size_t)y * W + x] = (uint8_t)min(max(v, 0), 255);
}

// retainBest + order-preserving compaction in three small launches over 1024-pixel chunks of all levels:
//   count (kept keypoints per chunk)  ->  scan (exclusive offsets per level, one workgroup per image)  ->  emit.
// cut = the score of the quota-th best keypoint of the level: everything at or above it is kept (ties included).
// The cuts in one small launch: workgroup = (level, image), thread s = suffix count of the scores >= s
__global__ __launch_bounds__(256) void orb_cut_kernel(OrbLevels L, OrbBatchDev D) {
  __shared__ int h[256];
  __shared__ int cut_s, total_s;
  const int l = blockIdx.x, s = threadIdx.x, quota = L.quota[l];
  int* ints = D.ints + (size_t)blockIdx.y * D.n_ints;
  h[s] = s ? ints[256 * l + s] : 0;
  if (s == 0) cut_s = 0;
  __syncthreads();
  int acc = 0;
  for (int k = 255; k >= s; k--) acc += h[k];
  if (s == 1) total_s = acc;
  if (s >= 1 && acc >= quota) atomicMax(&cut_s, s);
  __syncthreads();
  if (s == 0) ints[ORB_INTS_CUTS + l] = quota == 0 ? 256 : (total_s <= quota ? 0 : cut_s);
}

// workgroup = (1024-pixel chunk, image); with a list, blockIdx.y walks the list (the second emit of the images that
// overflowed) and the segments are those of the image's record
template <bool EMIT>
__global__ __launch_bounds__(1024) void orb_compact_kernel(OrbLevels L, OrbBatchDev D, const int32_t* __restrict__ img_list) {
  __shared__ int wave_tot[16];
  const int chunk = blockIdx.x;
  const int img = img_list ? img_list[blockIdx.y] : (int)blockIdx.y;
  const int l = orb_level_of_chunk(L, chunk);
  const int cut_s = D.ints[(size_t)img * D.n_ints + ORB_INTS_CUTS + l];
  const int W = L.W[l], n_pix = W * L.H[l];
  const int i = (chunk - L.chunk_base[l]) * 1024 + threadIdx.x;
  const size_t img_off = (size_t)img * D.pix_stride + L.pix_off[l];
  const uint8_t* score = D.score + img_off;
  const bool ok = i < n_pix && D.flag[img_off + i] && score[i] >= cut_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(ok);
  if (lane == 0) wave_tot[wave] = __popcll(m);
  __syncthreads();
  if (!EMIT) {
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; w++) t += wave_tot[w];
      D.chunk_count[(size_t)img * D.n_chunks + chunk] = t;
    }
    return;
  }
  if (ok) {
    int off = D.chunk_offset[(size_t)img * D.n_chunks + chunk];
    for (int w = 0; w < wave; w++) off += wave_tot[w];
    const int p = off + __popcll(m & ((1ull << lane) - 1ull));
    const VslOrbImgSeg& S = D.seg[img];
    if (p < S.seg_cap[l]) {
      const int y = i / W, x = i - y * W;
      const size_t slot = (size_t)img * D.slot_stride + S.seg_base[l] + p;
      D.kp_xy[2 * slot] = x;
      D.kp_xy[2 * slot + 1] = y;
      D.kp_sl[slot] = (int)score[i] | (l << 8);
    }
  }
}

// exclusive scan of the chunk counts within each level: one workgroup per image, levels one after the other.
// level_full = the keypoints of the level, level_count = those that fit its first segment: the host redoes the emit
// with exact segments when the two differ (retainBest keeps ties without limit).
__global__ __launch_bounds__(1024) void orb_scan_kernel(OrbLevels L, OrbBatchDev D) {
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* chunk_count = D.chunk_count + (size_t)blockIdx.x * D.n_chunks;
  int32_t* chunk_offset = D.chunk_offset + (size_t)blockIdx.x * D.n_chunks;
  int* ints = D.ints + (size_t)blockIdx.x * D.n_ints;
  for (int l = 0; l < ORB_LEVELS; l++) {
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    const int c0 = L.chunk_base[l], c1 = L.chunk_base[l + 1];
    for (int cb = c0; cb < c1; cb += 1024) {
      const int c = cb + threadIdx.x;
      const int v = c < c1 ? chunk_count[c] : 0;
      int x = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
      }
      if (lane == 63) wave_tot[wave] = x;
      __syncthreads();
      int off = base_s;
      for (int w = 0; w < wave; w++) off += wave_tot[w];
      if (c < c1) chunk_offset[c] = off + x - v;
      __syncthreads();
      if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < 16; w++) t += wave_tot[w];
        base_s += t;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      ints[ORB_INTS_FULL + l] = base_s;
      ints[ORB_INTS_COUNT + l] = min(base_s, L.seg_cap[l]);
    }
    __syncthreads();
  }
}

// the level of a keypoint slot of an image and whether the slot holds a keypoint
__device__ __forceinline__ bool orb_batch_slot_level(const VslOrbImgSeg& S, const int* __restrict__ ints, int slot, int* l_out) {
  int l = 0;
  while (l + 1 < ORB_LEVELS && slot >= S.seg_base[l + 1]) l++;
  *l_out = l;
  return slot - S.seg_base[l] < min(ints[ORB_INTS_FULL + l], S.seg_cap[l]);
}

// one wavefront per (keypoint slot, image): intensity centroid over the radius-15 disc, exact integer moments; the rows
// v = -15 .. 15 go over the lanes, each lane walks its row's columns
__global__ __launch_bounds__(256) void orb_angle_kernel(OrbLevels L, OrbBatchDev D, const int32_t* __restrict__ img_list, int n_slots) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (slot >= n_slots) return;
  const int img = img_list ? img_list[blockIdx.y] : (int)blockIdx.y;
  int l;
  if (!orb_batch_slot_level(D.seg[img], D.ints + (size_t)img * D.n_ints, slot, &l)) return;  // wave-uniform
  const int W = L.W[l];
  const size_t gslot = (size_t)img * D.slot_stride + slot;
  const uint8_t* center = D.pyr + (size_t)img * D.pix_stride + L.pix_off[l] + (size_t)D.kp_xy[2 * gslot + 1] * W + D.kp_xy[2 * gslot];
  int m_01 = 0, m_10 = 0;
  if (lane < 31) {
    const int v = lane - ORB_HALF_PATCH;
    const int d = c_umax[v < 0 ? -v : v];
    int row_sum = 0;
    for (int u = -d; u <= d; ++u) {
      const int val = center[u + v * W];
      row_sum += val;
      m_10 += u * val;
    }
    m_01 = v * row_sum;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m_01 += __shfl_xor(m_01, o);
    m_10 += __shfl_xor(m_10, o);
  }
  if (lane == 0) D.angle[gslot] = d_fast_atan2((float)m_01, (float)m_10);
}

// one thread per (keypoint slot, descriptor byte), blockIdx.y = image; cos / sin are read and the descriptor is written
// at the keypoint's FEATURE index (level-major, the order vsl_orb_detect_describe returns): the vocabulary descent reads
// the descriptors of the whole pass as one dense array
__global__ __launch_bounds__(256) void orb_describe_kernel(OrbLevels L, OrbBatchDev D, int n_slots) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int slot = t >> 5, j = t & 31;
  if (slot >= n_slots) return;
  const int img = blockIdx.y;
  const VslOrbImgSeg& S = D.seg[img];
  int l;
  if (!orb_batch_slot_level(S, D.ints + (size_t)img * D.n_ints, slot, &l)) return;
  const int W = L.W[l];
  const size_t gslot = (size_t)img * D.slot_stride + slot;
  const size_t feat = (size_t)S.feat_base + S.feat_off[l] + (slot - S.seg_base[l]);
  const uint8_t* bc = D.blurred + (size_t)img * D.pix_stride + L.pix_off[l] + (size_t)D.kp_xy[2 * gslot + 1] * W + D.kp_xy[2 * gslot];
  const float a = D.cs[2 * feat], b = D.cs[2 * feat + 1];
  int byte = 0;
#pragma unroll
  for (int bit = 0; bit < 8; bit++) {
    const OrbPat p = c_orb_pattern[8 * j + bit];
    const float xa = (float)p.xa * a - (float)p.ya * b, ya = (float)p.xa * b + (float)p.ya * a;
    const float xb = (float)p.xb * a - (float)p.yb * b, yb = (float)p.xb * b + (float)p.yb * a;
    const int t0 = bc[(int)rintf(ya) * W + (int)rintf(xa)], t1 = bc[(int)rintf(yb) * W + (int)rintf(xb)];
    byte |= (t0 < t1) << bit;
  }
  D.desc[32 * feat + j] = (uint8_t)byte;
}

size_t orb_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the carve-up of a pass's device scratch and pinned buffer
struct OrbBatchLayout {
  OrbPlan P;
  OrbBatchDev D;
  size_t device_bytes, pinned_bytes;
  int rows_cap;                 // rows of the compact arrays
  VslOrbImgSeg* h_seg;          // pinned [k]
  int32_t* h_list;              // pinned [k]
  int32_t* h_tail;              // pinned [k][3 * ORB_LEVELS]: level_count | cuts | level_full
  float* h_angle;               // pinned [k][slot_stride]
  float* h_cs;                  // pinned [rows_cap][2]
};

void orb_batch_layout(int w, int h, int nfeatures, int k, int max_feat, uint8_t* dev, uint8_t* pin, OrbBatchLayout& Y) {
  orb_plan_levels(w, h, nfeatures, Y.P);
  OrbBatchDev& D = Y.D;
  const size_t K = (size_t)k;
  D.pix_stride = Y.P.total_pix;  // a multiple of 256
  D.n_ints = 256 * ORB_LEVELS + 32;
  D.n_chunks = Y.P.n_chunks;
  D.slot_stride = (std::max(Y.P.n_slots, max_feat) + 3) & ~3;
  Y.rows_cap = k * ((max_feat + 3) & ~3);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    uint8_t* p = dev + o;
    o += orb_align256(bytes);
    return p;
  };
  D.pyr = take(K * D.pix_stride);
  D.score = take(K * D.pix_stride);
  D.flag = take(K * D.pix_stride);
  D.blurred = take(K * D.pix_stride);
  D.tmp = (float*)take(4 * K * D.pix_stride);
  D.ints = (int*)take(4 * K * D.n_ints);
  D.chunk_count = (int32_t*)take(4 * K * D.n_chunks);
  D.chunk_offset = (int32_t*)take(4 * K * D.n_chunks);
  D.kp_xy = (int32_t*)take(8 * K * D.slot_stride);
  D.kp_sl = (int32_t*)take(4 * K * D.slot_stride);
  D.angle = (float*)take(4 * K * D.slot_stride);
  D.cs = (float*)take(8 * (size_t)Y.rows_cap);
  D.desc = take(32 * (size_t)Y.rows_cap);
  D.seg = (VslOrbImgSeg*)take(sizeof(VslOrbImgSeg) * K);
  D.img_list = (int32_t*)take(4 * K);
  Y.device_bytes = o;
  o = 0;
  auto takeh = [&](size_t bytes) {
    uint8_t* p = pin + o;
    o += orb_align256(bytes);
    return p;
  };
  Y.h_seg = (VslOrbImgSeg*)takeh(sizeof(VslOrbImgSeg) * K);
  Y.h_list = (int32_t*)takeh(4 * K);
  Y.h_tail = (int32_t*)takeh(4 * K * 3 * ORB_LEVELS);
  Y.h_angle = (float*)takeh(4 * K * D.slot_stride);
  Y.h_cs = (float*)takeh(8 * (size_t)Y.rows_cap);
  Y.pinned_bytes = o;
}

}  // namespace

void vsl_orb_batch_bytes(int w, int h, int nfeatures, int k, int max_feat, size_t* device_bytes, size_t* pinned_bytes) {
  OrbBatchLayout Y;
  orb_batch_layout(w, h, nfeatures, k, max_feat, nullptr, nullptr, Y);
  *device_bytes = Y.device_bytes;
  *pinned_bytes = Y.pinned_bytes;
}

int vsl_orb_batch_count(vsl_ctx* ctx, VslOrbBatch& b) {
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = orb_upload_tables(ctx);
  if (rc) return rc;
  OrbBatchLayout Y;
  orb_batch_layout(b.w, b.h, b.nfeatures, b.k, b.max_feat, (uint8_t*)b.scratch, (uint8_t*)b.pinned, Y);
  const OrbLevels& L = Y.P.L;
  const OrbBatchDev& D = Y.D;
  const int k = b.k, n_slots = Y.P.n_slots;
  hipStream_t st = ctx->stream;
  // every image starts with the segments of the plan
  for (int i = 0; i < k; i++) {
    VslOrbImgSeg& S = Y.h_seg[i];
    std::memset(&S, 0, sizeof(S));
    for (int l = 0; l < ORB_LEVELS; l++) {
      S.seg_base[l] = L.seg_base[l];
      S.seg_cap[l] = L.seg_cap[l];
    }
  }
  VSL_HIP(ctx, hipMemcpyAsync(D.seg, Y.h_seg, sizeof(VslOrbImgSeg) * k, hipMemcpyHostToDevice, st));
  const size_t wh = (size_t)b.w * b.h;
  if (b.host_image)  // level 0 of the pass's one image, row by row out of host memory
    VSL_HIP(ctx, hipMemcpy2DAsync(D.pyr, b.w, b.host_image, b.host_pitch, b.w, b.h, hipMemcpyHostToDevice, st));
  else
    VSL_HIP(ctx, hipMemcpy2DAsync(D.pyr, D.pix_stride, b.images, b.image_stride, wh, k, hipMemcpyDeviceToDevice, st));
  VSL_HIP(ctx, hipMemsetAsync(D.ints, 0, sizeof(int) * (size_t)k * D.n_ints, st));
  for (int l = 1; l < ORB_LEVELS; l++)
    hipLaunchKernelGGL(orb_resize_kernel, dim3((L.W[l] + 255) / 256, L.H[l], k), dim3(256), 0, st, D, L.pix_off[l - 1], L.W[l - 1],
                       L.H[l - 1], L.pix_off[l], L.W[l], L.H[l], (double)L.W[l - 1] / L.W[l], (double)L.H[l - 1] / L.H[l]);
  {
    const int W = L.W[0], H = L.H[0];
    const unsigned z = (unsigned)(ORB_LEVELS * k);
    hipLaunchKernelGGL(orb_fast_kernel, dim3((W + 15) / 16, (H + 15) / 16, z), dim3(256), 0, st, L, D);
    hipLaunchKernelGGL(orb_nms_kernel, dim3((W + 255) / 256, H, z), dim3(256), 0, st, L, D);
    hipLaunchKernelGGL(orb_blur_rows_kernel, dim3((W + 255) / 256, H, z), dim3(256), 0, st, L, D);
    hipLaunchKernelGGL(orb_blur_cols_kernel, dim3((W + 255) / 256, H, z), dim3(256), 0, st, L, D);
  }
  hipLaunchKernelGGL(orb_cut_kernel, dim3(ORB_LEVELS, k), dim3(256), 0, st, L, D);
  hipLaunchKernelGGL(orb_compact_kernel<false>, dim3(D.n_chunks, k), dim3(1024), 0, st, L, D, (const int32_t*)nullptr);
  hipLaunchKernelGGL(orb_scan_kernel, dim3(k), dim3(1024), 0, st, L, D);
  hipLaunchKernelGGL(orb_compact_kernel<true>, dim3(D.n_chunks, k), dim3(1024), 0, st, L, D, (const int32_t*)nullptr);
  hipLaunchKernelGGL(orb_angle_kernel, dim3((n_slots + 3) / 4, k), dim3(256), 0, st, L, D, (const int32_t*)nullptr, n_slots);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpy2DAsync(Y.h_angle, 4 * (size_t)D.slot_stride, D.angle, 4 * (size_t)D.slot_stride, 4 * (size_t)n_slots, k,
                                hipMemcpyDeviceToHost, st));
  VSL_HIP(ctx, hipMemcpy2DAsync(Y.h_tail, 4 * 3 * ORB_LEVELS, D.ints + ORB_INTS_COUNT, 4 * (size_t)D.n_ints, 4 * 3 * ORB_LEVELS, k,
                                hipMemcpyDeviceToHost, st));
  VSL_HIP(ctx, hipStreamSynchronize(st));
  b.n_feat.assign(k, 0);
  b.feat_base.assign(k, 0);
  b.full.assign((size_t)k * ORB_LEVELS, 0);
  b.overflow.assign(k, 0);
  int rows = 0;
  for (int i = 0; i < k; i++) {
    int total = 0;
    for (int l = 0; l < ORB_LEVELS; l++) {
      const int f = Y.h_tail[(size_t)i * 3 * ORB_LEVELS + 2 * ORB_LEVELS + l];
      b.full[(size_t)i * ORB_LEVELS + l] = f;
      if (f > L.seg_cap[l]) b.overflow[i] = 1;
      total += f;
    }
    b.n_feat[i] = total;
    b.feat_base[i] = rows;
    rows = (rows + std::min(total, b.max_feat) + 3) & ~3;  // an image beyond max_feat is never described
  }
  b.n_rows = rows;
  return VSL_OK;
}

int vsl_orb_batch_describe(vsl_ctx* ctx, VslOrbBatch& b) {
  OrbBatchLayout Y;
  orb_batch_layout(b.w, b.h, b.nfeatures, b.k, b.max_feat, (uint8_t*)b.scratch, (uint8_t*)b.pinned, Y);
  const OrbLevels& L = Y.P.L;
  const OrbBatchDev& D = Y.D;
  const int k = b.k;
  hipStream_t st = ctx->stream;
  int n_over = 0, over_slots = 0, max_slots = Y.P.n_slots;
  for (int i = 0; i < k; i++) {
    if (b.n_feat[i] > b.max_feat) return vsl_fail(ctx, VSL_ERR_CAPACITY, "orb batch: image %d has %d features, at most %d are described", i, b.n_feat[i], b.max_feat);
    VslOrbImgSeg& S = Y.h_seg[i];
    const int32_t* full = &b.full[(size_t)i * ORB_LEVELS];
    if (b.overflow[i]) {
      // more ties than a segment holds: segments of exactly the counted sizes (the chunk offsets are relative to the
      // level and stay valid); the sum is n_feat <= max_feat <= the image's slot range
      int base = 0;
      for (int l = 0; l < ORB_LEVELS; l++) {
        S.seg_base[l] = base;
        S.seg_cap[l] = full[l];
        base += full[l];
      }
      Y.h_list[n_over++] = i;
      over_slots = std::max(over_slots, base);
    }
    int off = 0;
    for (int l = 0; l < ORB_LEVELS; l++) {
      S.feat_off[l] = off;
      off += full[l];
    }
    S.feat_base = b.feat_base[i];
    S.n_feat = b.n_feat[i];
  }
  VSL_HIP(ctx, hipMemcpyAsync(D.seg, Y.h_seg, sizeof(VslOrbImgSeg) * k, hipMemcpyHostToDevice, st));
  if (n_over) {
    VSL_HIP(ctx, hipMemcpyAsync(D.img_list, Y.h_list, 4 * (size_t)n_over, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(orb_compact_kernel<true>, dim3(D.n_chunks, n_over), dim3(1024), 0, st, L, D, (const int32_t*)D.img_list);
    hipLaunchKernelGGL(orb_angle_kernel, dim3((over_slots + 3) / 4, n_over), dim3(256), 0, st, L, D, (const int32_t*)D.img_list,
                       over_slots);
    VSL_CHECK_LAUNCH(ctx);
    // one strided copy for the pass: the rows of the other images arrive again unchanged
    const int cols = std::max(over_slots, Y.P.n_slots);
    VSL_HIP(ctx, hipMemcpy2DAsync(Y.h_angle, 4 * (size_t)D.slot_stride, D.angle, 4 * (size_t)D.slot_stride, 4 * (size_t)cols, k,
                                  hipMemcpyDeviceToHost, st));
    VSL_HIP(ctx, hipStreamSynchronize(st));
    max_slots = cols;
  }
  // host: cos / sin of every angle with libm (fp32 radians -> double cos -> fp32, like the oracle), once for the pass
  for (int i = 0; i < k; i++) {
    const VslOrbImgSeg& S = Y.h_seg[i];
    const float* ang = Y.h_angle + (size_t)i * D.slot_stride;
    for (int l = 0; l < ORB_LEVELS; l++) {
      float* cs = Y.h_cs + 2 * ((size_t)S.feat_base + S.feat_off[l]);
      const int n = b.full[(size_t)i * ORB_LEVELS + l];
      for (int q = 0; q < n; q++) {
        const float rad = ang[S.seg_base[l] + q] * (float)(M_PI / 180.0);
        cs[2 * q] = (float)std::cos((double)rad);
        cs[2 * q + 1] = (float)std::sin((double)rad);
      }
    }
  }
  if (b.n_rows > 0) {
    VSL_HIP(ctx, hipMemcpyAsync(D.cs, Y.h_cs, 8 * (size_t)b.n_rows, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(orb_describe_kernel, dim3((max_slots * 32 + 255) / 256, k), dim3(256), 0, st, L, D, max_slots);
    VSL_CHECK_LAUNCH(ctx);
  }
  b.desc = D.desc;
  b.seg = D.seg;
  return VSL_OK;
}

namespace {

// The count half of a pass of ONE image that lies in host memory, on the context's scratch and pinned buffer, with room
// for max_feat features or the plan's keypoint slots (2 * nfeatures + 64 per level), whichever is more.  Y is the pass's
// carve-up; behind its staging the pinned buffer has 44 bytes per keypoint slot for the caller's downloads.
int orb_count_one(vsl_ctx* ctx, const uint8_t* img, int w, int h, size_t pitch, int nfeatures, int max_feat, VslOrbBatch& b,
                  OrbBatchLayout& Y) {
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  orb_plan_levels(w, h, nfeatures, Y.P);
  max_feat = std::max(max_feat, Y.P.n_slots);
  orb_batch_layout(w, h, nfeatures, 1, max_feat, nullptr, nullptr, Y);  // the sizes
  int rc = vsl_ctx_dscratch(ctx, Y.device_bytes, &b.scratch);
  if (rc) return rc;
  if ((rc = vsl_ctx_hpinned(ctx, Y.pinned_bytes + 44 * (size_t)Y.D.slot_stride, &b.pinned))) return rc;
  orb_batch_layout(w, h, nfeatures, 1, max_feat, (uint8_t*)b.scratch, (uint8_t*)b.pinned, Y);
  b.host_image = img;
  b.host_pitch = pitch;
  b.w = w;
  b.h = h;
  b.k = 1;
  b.nfeatures = nfeatures;
  b.max_feat = max_feat;
  return vsl_orb_batch_count(ctx, b);
}

}  // namespace

// kp5: (x, y in level-0 pixels, angle in degrees, response, octave) per keypoint; desc32: 32 bytes each.
// *n_out = the number of keypoints found, also when it exceeds cap (VSL_ERR_CAPACITY, the first cap are filled).
// A pass of one image.  retainBest keeps every tie, so an image can hold more keypoints than the plan has slots: the
// pass is then done once more with room for the counted total (the rare adversarial image costs two passes).
extern "C" int vsl_orb_detect_describe(vsl_ctx* ctx, const uint8_t* img, int w, int h, size_t pitch, int nfeatures, int cap,
                                       float* kp5, uint8_t* desc32, int* n_out) {
  if (!orb_image_args_ok(ctx, img, w, h, pitch) || !n_out || nfeatures < 1 || cap < 0 || (cap > 0 && (!kp5 || !desc32)))
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_orb_detect_describe: bad arguments (w, h >= 64 required)");
  *n_out = 0;
  VslOrbBatch b;
  OrbBatchLayout Y;
  int rc = orb_count_one(ctx, img, w, h, pitch, nfeatures, 0, b, Y);
  if (!rc && b.n_feat[0] > b.max_feat) rc = orb_count_one(ctx, img, w, h, pitch, nfeatures, b.n_feat[0], b, Y);
  if (rc) return rc;
  const int total = b.n_feat[0], n = std::min(total, cap);
  *n_out = total;
  if (total == 0) return VSL_OK;
  if ((rc = vsl_orb_batch_describe(ctx, b))) return rc;
  const OrbLevels& L = Y.P.L;
  const OrbBatchDev& D = Y.D;
  const VslOrbImgSeg& S = Y.h_seg[0];  // the segments the keypoints were emitted into
  const size_t n_slots = (size_t)D.slot_stride;
  int32_t* h_xy = (int32_t*)((uint8_t*)b.pinned + Y.pinned_bytes);
  int32_t* h_sl = h_xy + 2 * n_slots;
  uint8_t* h_desc = (uint8_t*)(h_sl + n_slots);
  hipStream_t st = ctx->stream;
  VSL_HIP(ctx, hipMemcpyAsync(h_xy, D.kp_xy, 8 * n_slots, hipMemcpyDeviceToHost, st));
  VSL_HIP(ctx, hipMemcpyAsync(h_sl, D.kp_sl, 4 * n_slots, hipMemcpyDeviceToHost, st));
  if (n > 0) VSL_HIP(ctx, hipMemcpyAsync(h_desc, D.desc, 32 * (size_t)n, hipMemcpyDeviceToHost, st));
  VSL_HIP(ctx, hipStreamSynchronize(st));
  // the features are level-major, the order of the pass's compact descriptors
  for (int l = 0; l < ORB_LEVELS; l++)
    for (int i = 0, f = S.feat_off[l]; i < b.full[l] && f < n; i++, f++) {
      const int slot = S.seg_base[l] + i;
      float* k = kp5 + 5 * (size_t)f;
      k[0] = (float)h_xy[2 * (size_t)slot] * L.scale[l];
      k[1] = (float)h_xy[2 * (size_t)slot + 1] * L.scale[l];
      k[2] = Y.h_angle[slot];
      k[3] = (float)(h_sl[slot] & 255);
      k[4] = (float)l;
    }
  if (n > 0) std::memcpy(desc32, h_desc, 32 * (size_t)n);
  if (n < total) return vsl_fail(ctx, VSL_ERR_CAPACITY, "vsl_orb_detect_describe: %d keypoints, capacity %d", total, cap);
  return VSL_OK;
}

extern "C" int vsl_orb_level_sizes(int w, int h, int* level_w, int* level_h) {
  if (w < 1 || h < 1 || !level_w || !level_h) return VSL_ERR_INVALID;
  OrbPlan P;
  orb_plan_levels(w, h, 1, P);
  for (int l = 0; l < ORB_LEVELS; l++) {
    level_w[l] = P.L.W[l];
    level_h[l] = P.L.H[l];
  }
  return VSL_OK;
}

// Test and diagnostic entry: the stage images of one pyramid level after the count half of vsl_orb_detect_describe's pass.
extern "C" int vsl_orb_stage_images(vsl_ctx* ctx, const uint8_t* img, int w, int h, size_t pitch, int level, uint8_t* pyr,
                                    uint8_t* score, uint8_t* nms_flag, uint8_t* blurred) {
  if (!orb_image_args_ok(ctx, img, w, h, pitch) || level < 0 || level >= ORB_LEVELS)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_orb_stage_images: bad arguments (w, h >= 64, level in [0, %d) required)", ORB_LEVELS);
  VslOrbBatch b;
  OrbBatchLayout Y;
  // the stage images do not depend on the number of features; 1000 sizes the keypoint segments of the pass
  int rc = orb_count_one(ctx, img, w, h, pitch, 1000, 0, b, Y);
  if (rc) return rc;
  const size_t n = (size_t)Y.P.L.W[level] * Y.P.L.H[level], off = Y.P.L.pix_off[level];
  uint8_t* const dst[4] = {pyr, score, nms_flag, blurred};
  const uint8_t* const src[4] = {Y.D.pyr, Y.D.score, Y.D.flag, Y.D.blurred};
  for (int i = 0; i < 4; i++)
    if (dst[i]) VSL_HIP(ctx, hipMemcpyAsync(dst[i], src[i] + off, n, hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VSL_OK;
}

// compute_bow_vector (include/visnav/keypoints.h:243-254): ORB front end + vocabulary transform.
// More features than cap: VSL_ERR_CAPACITY with *nnz = *fv_n = the number of features (the capacity that suffices).
extern "C" int vsl_compute_bow_vector(vsl_ctx* ctx, const vsl_voc* voc, const uint8_t* img, int w, int h, size_t pitch,
                                      int num_features, int levelsup, int cap, uint32_t* word_ids, double* word_vals, int* nnz,
                                      uint32_t* fv_node, uint32_t* fv_feat, int* fv_n) {
  if (!ctx || !voc || !nnz || !fv_n || cap < 0) return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_compute_bow_vector: bad arguments");
  int kcap = 2 * num_features + 64 * ORB_LEVELS;
  std::vector<float> kp(5 * (size_t)kcap);
  std::vector<uint8_t> desc(32 * (size_t)kcap);
  int n = 0;
  int rc = vsl_orb_detect_describe(ctx, img, w, h, pitch, num_features, kcap, kp.data(), desc.data(), &n);
  if (rc == VSL_ERR_CAPACITY) {  // ties beyond the usual bound: once more with the reported total
    kcap = n;
    kp.resize(5 * (size_t)kcap);
    desc.resize(32 * (size_t)kcap);
    rc = vsl_orb_detect_describe(ctx, img, w, h, pitch, num_features, kcap, kp.data(), desc.data(), &n);
  }
  if (rc) return rc;
  if (n > cap) {
    *nnz = *fv_n = n;
    return vsl_fail(ctx, VSL_ERR_CAPACITY, "vsl_compute_bow_vector: %d features, output capacity %d", n, cap);
  }
  return vsl_bow_transform(ctx, voc, desc.data(), n, levelsup, word_ids, word_vals, nnz, fv_node, fv_feat, fv_n);
}
