// detect.hip -- K1 (min-eigenvalue response), K2a (candidate extraction), K2b (ordered greedy
// min-distance selection).  Together they replace the cv::goodFeaturesToTrack call and the border
// filter of visnav::detectKeypoints (include/visnav/keypoints.h:133-150).
//
// Arithmetic contract (identical, operation for operation, to oracle/orc_keypoints.cpp; the whole
// library is compiled with -ffp-contract=off so no multiply-add is fused):
//   s = (float)(1/3060); s2 = 2s
//   row filter at row yr:  rx = I(x+1) - I(x-1);  ry = ((s*I(x-1)) + (s2*I(x))) + (s*I(x+1))
//   dx = (rx(y-1) + rx(y+1))*s + rx(y)*s2;   dy = ry(y+1) - ry(y-1)              (fp32)
//   cov = (dx*dx, dx*dy, dy*dy)                                                   (fp32)
//   R(x,y) = ((double)c(x-1,y) + c(x,y)) + c(x+1,y);  A = (R(x,y-1) + R(x,y)) + R(x,y+1)  (fp64)
//   a = (float)A_xx*0.5f, b = (float)A_xy, c = (float)A_yy*0.5f
//   response = (a + c) - sqrtf((a-c)*(a-c) + b*b)                                 (fp32)
// (the kernel evaluates the last two lines as  t = fma(0.25, fl((X-Y)^2), fl(b*b)),  fma(0.5, fl(X+Y), -sqrt(t))  with
// X = (float)A_xx, Y = (float)A_yy: halving is exact, so these two explicit FMAs round exactly the sums above)
// BORDER_REFLECT_101 is applied to the image for the derivative and to the cov image for the box
// sum (a lane or row outside the image evaluates the cov of its mirror position).
#include <type_traits>

#include "vsl_common.h"

// rows per wave strip.  Every strip recomputes 4 halo rows and pays one reloading step, one maximum reduction, one
// quality cut and one list flush, so taller strips waste less (a 480-row image: 60 rows = 512 row steps, 120 = 496,
// 160 = 492, 240 = 488).  The strips of an image are numbered column strip by column strip and dealt to workgroups
// four at a time (see the kernel), so any height fills the waves; DESIGN.md 8.2 has the measured table.
#ifndef K1_ROWS
#define K1_ROWS 120
#endif
#ifndef K1_ROWS_SMALL
#define K1_ROWS_SMALL 30  // strips of launches of fewer than 8 images (16 strips of a 480-row image)
#endif
// goodFeaturesToTrack's qualityLevel as the reference passes it (keypoints.h:138): threshold = max response * 0.01
#define VSL_QUALITY_LEVEL 0.01
#define K1_WLIST 384  // LDS candidate slots per wave; a strip that collects more drains its list on the way (K1_FLUSH_ROOM)
// the list is checked once per six row steps and drained when fewer than this many slots are left (noise images make
// ~7 candidates per row step, real frames 2 to 3); a plateau that outruns it takes the direct global append
#define K1_FLUSH_ROOM 96
#define K1_COLS 60  // owned columns per wave: 64 lanes minus two halo lanes on each side

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

struct RowF {
  float rx, ry;
};

struct RowRaw {
  unsigned l, m, r;
};

// yr is wave-uniform: buffer loads through the image's descriptor take the row base as the scalar offset and the
// lane's column as the 32-bit vector offset -- no per-load 64-bit address arithmetic on the VALU (K1 is VALU-bound)
typedef __amdgpu_buffer_rsrc_t ImgSrd;
__device__ __forceinline__ RowRaw rowload(ImgSrd img, int w, int yr, unsigned xm, unsigned xe, unsigned xp) {
  const int row = yr * w;
  RowRaw o;
  o.l = __builtin_amdgcn_raw_buffer_load_b8(img, (int)xm, row, 0);
  o.m = __builtin_amdgcn_raw_buffer_load_b8(img, (int)xe, row, 0);
  o.r = __builtin_amdgcn_raw_buffer_load_b8(img, (int)xp, row, 0);
  return o;
}

__device__ __forceinline__ RowF rowfilt(RowRaw p, float s, float s2) {
  const float l = (float)p.l, m = (float)p.m, r = (float)p.r;
  RowF o;
  o.rx = r - l;
  float t = s * l;
  t = t + s2 * m;
  t = t + s * r;
  o.ry = t;
  return o;
}

// value of the lane below / above (wave-wide shift by one lane, a full-rate DPP move; lane 0 / 63
// receive 0 and are halo lanes whose results are never used)
__device__ __forceinline__ float from_lane_below(float v) {  // lane i <- lane i-1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_lane_above(float v) {  // lane i <- lane i+1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

// K1 is bound by VALU issue slots.  Measured on gfx950 at 8 waves per SIMD (tools/probes/valu_rate.hip, valu_rate2.hip),
// cycles per wave-instruction per SIMD: v_add_f32 / v_fma_f32 / v_mov_b32 / integer add 2.3; every DPP form (a move or
// an ALU operation with a DPP source), v_cvt_*, v_cmp_*, v_add_f64, v_pk_*_f32 and v_max3_f32 4.2; v_sqrt_f32 /
// v_rsq_f32 8.2.  So each product is widened to fp64 ONCE and its neighbours' copies are fetched as fp64 -- through LDS
// memory where the LDS pipe has room, by two DPP moves per direction otherwise (see the row step).
// the fp64 value of the lane below as two DPP moves
__device__ __forceinline__ double dpp_below_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, 0x138, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), 0x138, 0xf, 0xf, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// ... and of the lane above
__device__ __forceinline__ double dpp_above_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, 0x130, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), 0x130, 0xf, 0xf, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// one-instruction maximum of three finite floats (fmaxf chains compile to v_max_f32 pairs with
// canonicalisation; the responses here are never NaN)
__device__ __forceinline__ float fmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ float fmax2(float a, float b) {  // no NaN canonicalisation moves
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// Correctly rounded fp32 square root (what sqrtf is under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt) in
// six issue slots: y = v_rsq_f32(t) (1 ulp), r = t * y (within ~2 ulp of the root), then one Markstein correction
// r' = fma(fma(-r, r, t), y / 2, r): the residual t - r^2 is exact in the fused multiply-add, the corrected value is
// within 2^-44 relative of the root before its single rounding.  That this IS the correctly rounded root for every
// float in [2^-100, 2^128) on gfx950 is not argued but checked exhaustively (tools/probes/sqrt_exhaustive.hip, and
// tests/test_keypoints_gpu.py::test_fast_sqrt_is_correctly_rounded_everywhere through vsl_diag_sqrt_check): 0
// mismatches with sqrtf over all 2^31 bit patterns of that range.  v_sqrt_f32 + the two neighbour residuals used before
// cost two more v_cmp / v_cndmask pairs (4.2 + 3.1 cycles each against 2.3 for an fma).
//  * t = 0 (flat patches): rsq sees K1_SQRT_FLOOR instead (no infinity), r = 0 * y = 0, residual 0, result 0.
//  * 0 < t < 2^-100 (cannot arise from the sums above other than through cancellation to the last bits): wave-uniform
//    branch to the library expansion; a wave that only holds zeros leaves it after one more compare.
#define K1_SQRT_FLOOR 0x1p-100f
__device__ __forceinline__ float fast_sqrt_rn(float t) {
  const float y = __builtin_amdgcn_rsqf(__builtin_fmaxf(t, K1_SQRT_FLOOR));
  const float r = t * y;
  const float e = __builtin_fmaf(-r, r, t);
  return __builtin_fmaf(e, 0.5f * y, r);
}
__device__ __forceinline__ float sqrt_rn(float t) {
  float r = fast_sqrt_rn(t);
  const bool small = t < K1_SQRT_FLOOR;
  if (__builtin_amdgcn_ballot_w64(small) != 0ull) {  // keeps the library expansion off the common path
    asm volatile("" ::: "memory");  // not speculatable: stops the compiler from flattening the branch
    const bool rare = small && t > 0.f;
    if (__builtin_amdgcn_ballot_w64(rare) != 0ull) {
      asm volatile("" ::: "memory");
      if (rare) r = sqrtf(t);
    }
  }
  return r;
}

// diagnostic behind vsl_diag_sqrt_check: compares fast_sqrt_rn with sqrtf on every float bit pattern in [lo, hi]
__global__ void sqrt_check_kernel(uint32_t lo, uint32_t hi, unsigned long long* bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long n = 0;
  for (uint64_t b = (uint64_t)lo + blockIdx.x * blockDim.x + threadIdx.x; b <= hi; b += stride) {
    const float t = __builtin_bit_cast(float, (uint32_t)b);
    n += __builtin_bit_cast(uint32_t, fast_sqrt_rn(t)) != __builtin_bit_cast(uint32_t, sqrtf(t));
  }
  if (n) atomicAdd(bad, n);
}

__global__ void detect_init_kernel(int32_t* meta, int first, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    meta[(size_t)(first + i) * VSL_META_STRIDE + VSL_META_MAX] = INT32_MIN;
    meta[(size_t)(first + i) * VSL_META_STRIDE + VSL_META_NCAND] = 0;
  }
}

// K1 + K2a fused.  An image is cut into ceil(w/60) x ceil(h/ROWS) strips of 60 columns x ROWS rows, numbered down the
// rows of a column strip first; a workgroup of 256 threads takes four consecutive strips, one per wave (1-D grid, see
// below), so only the last workgroup of an image can hold idle waves whatever ROWS is.
// One image column per lane; rows
// are walked top to bottom with the row-filter results, the fp64 row sums and three response rows held
// in registers; column neighbours come from DPP lane shifts.  Nothing but the image is read and -- in
// the normal pipeline -- nothing but the candidate list is written: the response image (4 bytes per
// pixel) never goes to memory.
//
// Candidates.  goodFeaturesToTrack keeps a pixel iff its thresholded response is non-zero and equals the
// 3x3 maximum of the thresholded response, with threshold = 0.01 * (global maximum) -- unknown until the
// whole image has been processed.  For a positive threshold that is equivalent to
//      response > threshold   and   no 3x3 neighbour has a larger raw response,
// so this kernel emits every pixel with response > 0 and no larger neighbour ("provisional
// candidates", a superset), and the selection kernel drops those at or below the threshold once the
// maximum is known.  (A response image whose maximum is <= 0 yields no corners here; OpenCV could only
// differ on an image whose responses are all negative.)
// Key = (order-preserving fp32 bits << 32) | y << 16 | x (ordered like the pixel index y * w + x, and the selection
// kernel gets the position back without a division): a descending sort on the key is the
// reference's order (value descending, equal values by address descending).
//
// Image maximum.  A pixel that holds a positive image maximum has no larger neighbour, so it is a provisional candidate
// wherever a pixel may be one; only row 0, row h - 1, column 0 and column w - 1 may not.  The maximum over the emitted
// candidates and those border pixels is therefore the image maximum whenever that is positive, bit for bit; when it is
// not, the value stored is <= 0 as well and there are no corners either way.  Interior row steps update no maximum.

// Quality cut of a wave's LDS list against a maximum `vmax` that the image maximum is known to reach: the selection
// kernel drops every candidate at or below (float)(max * 0.01) (monotone in max), so a key at or below the threshold
// of ANY lower bound of the image maximum can never survive.  Exact: only keys the selection kernel would discard are
// removed.  In-place, order-preserving compaction by the whole wave; returns the number of keys kept.
__device__ __forceinline__ int k1_quality_cut(uint64_t* list, int have, float vmax, int lane) {
  if (!(vmax > 0.f) || have <= 0) return have;
  const float thr = (float)((double)vmax * VSL_QUALITY_LEVEL);
  const uint32_t floor_hi = (uint32_t)vsl_float_to_ordered(thr) ^ 0x80000000u;
  int kept = 0;
  for (int i0 = 0; i0 < have; i0 += 64) {
    const int i = i0 + lane;
    const uint64_t key = i < have ? list[i] : 0ull;
    const bool keep = i < have && (uint32_t)(key >> 32) > floor_hi;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
    if (keep) list[kept + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = key;
    kept += __popcll(m);
  }
  return kept;
}

template <bool STORE_RESPONSE, int ROWS>
__global__ __launch_bounds__(256) void min_eig_response_kernel(const uint8_t* __restrict__ images,
                                                               float* __restrict__ response, int32_t* __restrict__ meta,
                                                               uint64_t* __restrict__ cand, size_t cand_cap, int w, int h,
                                                               int first, int wlist_cap, int n_images, int tiles_x, int strips_y) {
  __shared__ uint64_t list[4][K1_WLIST];  // wave-private lists: appended with a scalar counter, no atomics
  __shared__ int wave_n[4], wave_max[4], g_base;
  __shared__ double xbuf[4][2][66];  // lane exchange of two of the three products: slot lane + 1 of the wave's row (slots 0 / 65 are
                                     // read by the halo lanes 0 / 63 only, whose sums are never used)
  // XCD-aware 1-D grid: workgroups are dealt round-robin over the 8 XCDs, each with its own L2, and the 39 strips of a
  // 752 x 480 image overlap in halo rows and share 128-byte lines between neighbouring column strips.  With the plain
  // (x, y, image) grid every XCD fetched most of every image (FETCH_SIZE, calibrated: 3.75 x the image bytes per
  // launch); here workgroup b works for XCD b % 8, which takes the images congruent to it modulo 8, all tiles of one
  // image consecutively -- the same trick as the describe kernel.  Speed only: any placement computes the same.
  const int strips = tiles_x * strips_y;  // of one image
  const int tiles = (strips + 3) >> 2;    // workgroups of one image
  int img_i, tile;
  if (n_images >= 8) {
    const int xcd = blockIdx.x & 7, sl = blockIdx.x >> 3;
    img_i = (sl / tiles) * 8 + xcd;
    tile = sl - (sl / tiles) * tiles;
  } else {
    img_i = blockIdx.x / tiles;
    tile = blockIdx.x - img_i * tiles;
  }
  if (img_i >= n_images) return;  // workgroup-uniform (the padded tail of the last group of eight)
  const int slot = first + img_i;
  const ImgSrd img = __builtin_amdgcn_make_buffer_rsrc((void*)(images + (size_t)slot * w * h), 0, w * h, 0x00020000);
  float* __restrict__ resp = response + (size_t)slot * w * h;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // row bookkeeping below stays scalar
  const int strip = tile * 4 + wave;  // wave-uniform, like everything derived from it
  const int bx = strip / strips_y;
  const int xs = bx * K1_COLS;
  const int y0 = (strip - bx * strips_y) * ROWS;
  int* const ncand = &meta[(size_t)slot * VSL_META_STRIDE + VSL_META_NCAND];
  uint64_t* const cand_img = cand + (size_t)slot * cand_cap;
  int n_wave = 0;  // wave-uniform
  int own_max = INT32_MIN;  // ordered bits of the wave's maximum: its candidates and its pixels on the image border
  if (strip < strips) {
    const float s = (float)(1.0 / (4.0 * 3.0 * 255.0));
    const float s2 = 2.0f * s;
    const int x = xs - 2 + lane;
    const unsigned xe = (unsigned)reflect101(min(max(x, -1), w), w);  // out-of-range lanes are parked on a valid column
    const unsigned xm = (unsigned)reflect101((int)xe - 1, w), xp = (unsigned)reflect101((int)xe + 1, w);
    const bool own_col = lane >= 2 && lane < 2 + K1_COLS && x < w;
    const bool cand_col = own_col && x >= 1 && x < w - 1;
    const unsigned long long cand_lanes = __builtin_amdgcn_ballot_w64(cand_col);
    // pixels that can hold the image maximum without being candidates (see "Image maximum" above)
    const bool edge_strip = xs == 0 || xs + K1_COLS >= w;  // the strip holds image column 0 or w - 1
    const bool edge_lane = own_col && (x == 0 || x == w - 1);

    // Register state of the walk down the strip (roles rotated by NAME, no register-to-register moves):
    //  * two generations of fp64 row sums R(x, q) and one PAIR sum.  Every fp64 sum here is exact (each product is a
    //    multiple of 2^-47 below 1; nine of them fit 53 bits), so the order is free and consecutive rows share a pair:
    //      even step q:  B = R(q-1) + R(q),  A(q-1) = R(q-2) + B        odd step q+1:  A(q) = B + R(q+1)
    //    -- three fp64 additions per product per two rows instead of four;
    //  * two response rows (period 2, tied to the parity) and three rows of horizontal 3-maxima H (period 3);
    //  * the row filters of three consecutive rows (period 3).  The row loop is therefore unrolled by six.
    struct R3 {
      double xx, xy, yy;
    };
    R3 ra = {0, 0, 0}, rb = ra, bs = ra;
    float va = 0.f, vb = 0.f, hA = 0.f, hB = 0.f, hC = 0.f;
    RowF fA = {0.f, 0.f}, fB = fA, fC = fA;  // row filters of three consecutive rows
    int prev_ye = -100, pre_row = -100;
    RowRaw pre = {0u, 0u, 0u};
    float vmax = -3.0e38f;
    const int y_end = min(h, y0 + ROWS);
    // one step: q = row whose row sums are produced (into the slot of row q-2, dead by then).  Afterwards v_dn is the
    // response of row q-1 and h_dn its horizontal 3-maximum; the candidate row is q-2 (v_mid; H rows q-3, q-2, q-1).
    // STEADY (compile-time): the caller guarantees rows q-1 .. q+1 are inside the image and that the previous
    // step was row q-1, so f0 / f1 / `pre` are already what this step needs -- no reload path, hence no join
    // whose register copies would land on the common path.
    // EVEN (compile-time): parity of the step index (see above); r2 / r1 hold R(q-2) / R(q-1).
    auto step = [&](auto steady_tag, auto even_tag, int q, R3& r2, R3& r1, float& v_mid_slot, float& v_dn_slot, float& h_up,
                    float& h_mid, float& h_dn, RowF& f0, RowF& f1, RowF& f2) {
      constexpr bool STEADY = decltype(steady_tag)::value;
      constexpr bool EVEN = decltype(even_tag)::value;
      // on entry (steady state) f0 / f1 hold rows ye-1 / ye from the previous step and f2 is the dead slot
      if (STEADY) {
        f2 = rowfilt(pre, s, s2);
        pre = rowload(img, w, min(q + 2, h - 1), xm, xe, xp);
      } else {
        const int ye = reflect101(min(max(q, -1), h), h);
        if (ye == prev_ye + 1 && ye + 1 < h) {
          if (pre_row != ye + 1) pre = rowload(img, w, ye + 1, xm, xe, xp);  // scalar branch, not taken in steady state
          f2 = rowfilt(pre, s, s2);
        } else {
          f0 = rowfilt(rowload(img, w, reflect101(ye - 1, h), xm, xe, xp), s, s2);
          f1 = rowfilt(rowload(img, w, ye, xm, xe, xp), s, s2);
          f2 = rowfilt(rowload(img, w, reflect101(ye + 1, h), xm, xe, xp), s, s2);
        }
        // bytes of the row the next step will filter: in flight during this step's arithmetic
        pre_row = min(ye + 2, h - 1);
        pre = rowload(img, w, pre_row, xm, xe, xp);
        prev_ye = ye;
      }
      const float dx = (f0.rx + f2.rx) * s + f1.rx * s2;
      const float dy = f2.ry - f0.ry;
      // fp64 row sums R(x, q) = (left + centre) + right of the three product images: each product is widened once
      // and its two neighbours' copies are fetched as fp64 (exact either way)
      const double dxx = (double)(dx * dx), dxy = (double)(dx * dy), dyy = (double)(dy * dy);
      // Lane exchange.  dxx and dxy go through LDS memory: one 8-byte write into the wave's own row, the two neighbours'
      // copies come back with one ds_read2_b64 (no VALU slot; LDS operations of one wave execute in order, so the
      // wave-private rows need no barrier -- the compiler barriers keep the reads between this step's and the next
      // step's writes).  dyy takes four DPP moves: the LDS pipe would saturate with all three (measured per 1024
      // images: DPP below + ds_bpermute above for all three 0.653 ms, LDS memory for all three 0.641, this mix 0.636,
      // DPP both ways for all three 0.712; tools/probes/valu_rate2.hip: a ds_write_b64 + ds_read2_b64 pair costs 14
      // CU-cycles of LDS time, four ds_bpermute_b32 24, a DPP move 4.2 VALU cycles).
      R3 cur;
      {
        xbuf[wave][0][lane + 1] = dxx;
        xbuf[wave][1][lane + 1] = dxy;
        asm volatile("" ::: "memory");
        const double lxx = xbuf[wave][0][lane], uxx = xbuf[wave][0][lane + 2];
        const double lxy = xbuf[wave][1][lane], uxy = xbuf[wave][1][lane + 2];
        asm volatile("" ::: "memory");
        cur.xx = (lxx + dxx) + uxx;
        cur.xy = (lxy + dxy) + uxy;
        cur.yy = (dpp_below_f64(dyy) + dyy) + dpp_above_f64(dyy);
      }
      // response of row y = q - 1 from the row sums of rows q-2, q-1, q
      const int y = q - 1;
      double Axx, Axy, Ayy;
      if (EVEN) {
        bs.xx = r1.xx + cur.xx;
        bs.xy = r1.xy + cur.xy;
        bs.yy = r1.yy + cur.yy;
        Axx = r2.xx + bs.xx;
        Axy = r2.xy + bs.xy;
        Ayy = r2.yy + bs.yy;
      } else {
        Axx = bs.xx + cur.xx;
        Axy = bs.xy + cur.xy;
        Ayy = bs.yy + cur.yy;
      }
      r2 = cur;  // the slot of row q-2 is dead
      // lambda_min = (a + c) - sqrt((a - c)^2 + b^2) with a = X/2, c = Y/2.  Halving is exact (X, Y are zero or above
      // 2^-25: never denormal), so a - c = fl(X - Y)/2 and a + c = fl(X + Y)/2: the difference is halved before it is
      // squared like the oracle does, the sum inside the last fused multiply-add (its product is exact).
      const float X = (float)Axx, b = (float)Axy, Y = (float)Ayy;
      const float xpy = X + Y, d = 0.5f * (X - Y);
      float t = d * d;
      t = t + b * b;
      const float v_dn = __builtin_fmaf(0.5f, xpy, -sqrt_rn(t));
      float h_tmp;
      // horizontal 3-maximum of the new response row: two v_max_f32 with a DPP source (bound_ctrl:0 feeds 0.0 into
      // lanes 0 / 63, halo lanes whose H is never used by an owned column).  The two wait states in front are NOT optional:
      // v_dn comes straight out of a v_fma, a VALU write of a VGPR must be two wait states old before a DPP operation
      // reads it (the ISA's list of manually inserted wait states), and the compiler's hazard recogniser does not see a
      // DPP read inside inline assembly.  Without them one-image launches (a lone wave per SIMD issues back to back; in a
      // batch the other waves' instructions space the two out) read stale neighbours at some lanes, emitted false local
      // maxima, and some of those displaced real corners: wrong on 5 of 120 synthetic frames, 5-6 runs of 6.
      asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %2, %2 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                   "v_max_f32_dpp %1, %2, %0 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
                   : "=&v"(h_tmp), "=&v"(h_dn)
                   : "v"(v_dn));
      if (STORE_RESPONSE) {
        if (own_col && y >= y0 && y < y_end) resp[y * w + x] = v_dn;
      }
      // the maximum of the border pixels; a STEADY step owns no pixel of row 0 or row h - 1
      const bool edge_row = !STEADY && (y == 0 || y == h - 1);
      if ((edge_strip || edge_row) && y >= y0 && y < y_end) {  // scalar
        if (edge_row ? own_col : edge_lane) vmax = fmax2(vmax, v_dn);
      }
      // candidate test for row yc = q - 2: v_mid > 0 and no larger value among its 8 neighbours  <=>  v_mid > 0 and
      // v_mid >= the maximum of the 3 x 3 block (itself included) = max3 of the three H rows.  The sign test waits
      // inside the branch: rows without any local maximum (most rows) never pay for it.
      const float v_mid = v_mid_slot;
      const int yc = q - 2;
      if (yc >= y0 && yc < y_end && yc >= 1 && yc < h - 1) {  // scalar
        const float m9 = fmax3(h_up, h_mid, h_dn);
        const bool ge0 = v_mid >= m9;
        if ((__builtin_amdgcn_ballot_w64(ge0) & cand_lanes) != 0ull) {
          const bool ge = ge0 && v_mid > 0.f;
          const unsigned long long mask = __builtin_amdgcn_ballot_w64(ge) & cand_lanes;
          if (cand_col && ge) {
            vmax = fmax2(vmax, v_mid);  // ... and of the candidates
            const uint32_t ob = (uint32_t)vsl_float_to_ordered(v_mid) ^ 0x80000000u;
            const uint64_t key = ((uint64_t)ob << 32) | ((uint32_t)yc << 16) | (uint32_t)x;
            const int p = n_wave + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (__builtin_expect(p < wlist_cap, 1)) {
              list[wave][p] = key;
            } else {  // the list filled up between two flush checks (plateaus): rare direct append
              const int g = atomicAdd(ncand, 1);
              if ((size_t)g < cand_cap) cand_img[g] = key;
            }
          }
          n_wave += __popcll(mask);
        }
      }
      v_dn_slot = v_dn;
    };
    // Mid-strip flush: the quality cut against the wave's running maximum (the image maximum is at least that), then
    // the survivors go to the image's global list behind one reservation.  Wave-private, no barrier; the keys are
    // unique and the selection kernel sorts them, so their order in the global list is free.
    auto flush = [&]() {
      float m = vmax;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      const int kept = k1_quality_cut(list[wave], min(n_wave, wlist_cap), m, lane);
      if (kept > 0) {
        int g = 0;
        if (lane == 0) g = atomicAdd(ncand, kept);
        g = __builtin_amdgcn_readfirstlane(g);
        for (int i = lane; i < kept; i += 64)
          if ((size_t)(g + i) < cand_cap) cand_img[g + i] = list[wave][i];
      }
      n_wave = 0;
    };
    const int q_first = y0 - 2, q_last = y_end + 1;
    typedef std::integral_constant<bool, true> Steady;
    typedef std::integral_constant<bool, false> Generic;
    typedef std::integral_constant<bool, true> Even;
    typedef std::integral_constant<bool, false> Odd;
    // step i of the strip (i = q - q_first): parity i % 2, H / row-filter roles i % 3
#define K1_STEP_E0(T, q) step(T{}, Even{}, q, ra, rb, va, vb, hA, hB, hC, fA, fB, fC)
#define K1_STEP_O1(T, q) step(T{}, Odd{}, q, rb, ra, vb, va, hB, hC, hA, fB, fC, fA)
#define K1_STEP_E2(T, q) step(T{}, Even{}, q, ra, rb, va, vb, hC, hA, hB, fC, fA, fB)
#define K1_STEP_O3(T, q) step(T{}, Odd{}, q, rb, ra, vb, va, hA, hB, hC, fA, fB, fC)
#define K1_STEP_E4(T, q) step(T{}, Even{}, q, ra, rb, va, vb, hB, hC, hA, fB, fC, fA)
#define K1_STEP_O5(T, q) step(T{}, Odd{}, q, rb, ra, vb, va, hC, hA, hB, fC, fA, fB)
    // the step of role r (any r >= 0)
#define K1_STEP_R(r, T, q)                            \
  do {                                                \
    if constexpr ((r) % 6 == 0) K1_STEP_E0(T, q);      \
    else if constexpr ((r) % 6 == 1) K1_STEP_O1(T, q); \
    else if constexpr ((r) % 6 == 2) K1_STEP_E2(T, q); \
    else if constexpr ((r) % 6 == 3) K1_STEP_O3(T, q); \
    else if constexpr ((r) % 6 == 4) K1_STEP_E4(T, q); \
    else K1_STEP_O5(T, q);                            \
  } while (0)
    // a strip is ROWS + 4 steps: K1_OPEN (4 to 9) opening steps, the first of which reloads everything, then groups of
    // six starting at role K1_OPEN.  Four at least, so that the first group starts at q >= 2 in every strip.
    constexpr int K1_OPEN = ROWS % 6 + 4;
#define K1_OPENING(T)                                          \
  K1_STEP_R(1, T, q_first + 1);                                \
  K1_STEP_R(2, T, q_first + 2);                                \
  K1_STEP_R(3, T, q_first + 3);                                \
  if constexpr (K1_OPEN > 4) K1_STEP_R(4, T, q_first + 4);     \
  if constexpr (K1_OPEN > 5) K1_STEP_R(5, T, q_first + 5);     \
  if constexpr (K1_OPEN > 6) K1_STEP_R(6, T, q_first + 6);     \
  if constexpr (K1_OPEN > 7) K1_STEP_R(7, T, q_first + 7);     \
  if constexpr (K1_OPEN > 8) K1_STEP_R(8, T, q_first + 8);
#define K1_SIX(T, q)               \
  K1_STEP_R(K1_OPEN, T, q);        \
  K1_STEP_R(K1_OPEN + 1, T, q + 1); \
  K1_STEP_R(K1_OPEN + 2, T, q + 2); \
  K1_STEP_R(K1_OPEN + 3, T, q + 3); \
  K1_STEP_R(K1_OPEN + 4, T, q + 4); \
  K1_STEP_R(K1_OPEN + 5, T, q + 5);
    // STEADY is decided per group of steps, not per strip (all scalar): rows q - 1 .. q + 1 of every step of the group
    // are interior, none of its response rows is row 0 or h - 1 (q >= 2), and the step in front of it left row q - 1's
    // state behind.  So a tall strip that touches the top or the bottom of the image runs generic steps only there: the
    // opening, then a loop of steady groups, then at most two generic groups at the bottom of the image (a loop of its
    // own: one loop with both kinds of group costs 26 more registers).
    K1_STEP_E0(Generic, q_first);
    if (q_first >= 1 && q_first + K1_OPEN < h) {
      K1_OPENING(Steady)
    } else {
      K1_OPENING(Generic)
    }
    const int flush_mark = max(wlist_cap - K1_FLUSH_ROOM, 0);
    int q = q_first + K1_OPEN;
    for (; q <= q_last && q + 6 < h; q += 6) {
      K1_SIX(Steady, q)
      if (n_wave > flush_mark) flush();
    }
    // steady steps keep no row bookkeeping: restored here for the generic ones
    prev_ye = q - 1;
    pre_row = min(q + 1, h - 1);
    for (; q <= q_last; q += 6) {
      K1_SIX(Generic, q)
    }
#undef K1_STEP_R
#undef K1_OPENING
#undef K1_SIX
#undef K1_STEP_E0
#undef K1_STEP_O1
#undef K1_STEP_E2
#undef K1_STEP_O3
#undef K1_STEP_E4
#undef K1_STEP_O5
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
    own_max = vsl_float_to_ordered(vmax);
    if (lane == 0) atomicMax(&meta[(size_t)slot * VSL_META_STRIDE + VSL_META_MAX], own_max);
  }
  if (lane == 0) wave_max[wave] = own_max;
  __syncthreads();
  // Final quality cut: the image maximum is at least the maximum of this workgroup's four waves, so what is left in the
  // lists is cut against that (k1_quality_cut) before it costs 8 bytes of traffic each way (15.5k -> ~4.7k keys per
  // synthetic frame, 17k -> ~9k on EuRoC frames).
  const float wg_max = vsl_ordered_to_float(max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3])));
  const int kept = k1_quality_cut(list[wave], min(n_wave, wlist_cap), wg_max, lane);
  if (lane == 0) wave_n[wave] = kept;
  __syncthreads();
  const int c0 = wave_n[0], c1 = wave_n[1], c2 = wave_n[2], c3 = wave_n[3];
  const int n = c0 + c1 + c2 + c3;
  if (n == 0) return;
  if (threadIdx.x == 0) g_base = atomicAdd(ncand, n);
  __syncthreads();
  const int base = g_base + (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
  const int mine = wave_n[wave];
  for (int i = lane; i < mine; i += 64)
    if ((size_t)(base + i) < cand_cap) cand_img[base + i] = list[wave][i];
}

// ------------------------------------------------------------------------------------------ K2b
// One 1024-thread workgroup per image.  The candidate keys above the quality threshold are sorted (descending) in
// LDS -- a counting sort on the top response bits plus in-bin ranking for the usual case of at most SEL_CHUNK keys,
// the bitonic network for chunks beyond that (a most-significant-digit radix select finds the chunk boundary) and
// for over-full bins -- and consumed in rank order, 1024 at a time, by an exact parallel restatement of the
// reference's sequential greedy loop:
//   a candidate is dropped if an ALREADY ACCEPTED corner lies in the 3x3 neighbouring 8-px cells at
//   squared distance < 64; among the survivors of one batch, a candidate waits for every
//   higher-ranked survivor within that distance to be decided, is rejected if one of them was
//   accepted, and is accepted otherwise (the lowest undecided rank always decides, so the rounds
//   terminate and the result is the sequential one).  Acceptance stops at num_features.
#define SEL_THREADS 1024
#define SEL_CHUNK 8192
#define SEL_BINS 1024      // response bins of the counting sort (= threads of the workgroup)
#define SEL_MAX_BLOCKERS 6  // blockers of a candidate kept in registers, 10 bits each in one 64-bit word (more: the cell lists are walked again)
static_assert(SEL_THREADS <= 1024 && SEL_MAX_BLOCKERS * 10 <= 64, "blocker packing");

struct SelShared {
  int wave_tot[16];
  int hist[256];
  unsigned long long sel_prefix;
  int sel_k;
  int n_chunk;
};

// Exclusive prefix counts of `p` (low 16 bits) and of `q` (high 16 bits) over the workgroup (thread order) and the
// two totals, packed the same way: a count is at most SEL_THREADS, so the halves never carry into each other and
// one scan serves both.  The sixteen wave totals are scanned across a row of sixteen lanes (four DPP row shifts)
// and picked by lane index: sixteen `w < wave` select masks would live in 32 SGPRs all through the greedy loop.
// One workgroup barrier, between the write of wave_tot and its reads; the CALLER keeps a barrier between the
// reads of one call and the write of the next (the greedy has two per batch).
__device__ __forceinline__ int block_scan(bool p, bool q, int* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long m = __ballot(p), mq = __ballot(q);
  const int within = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) |
                     (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mq, 0u)) << 16;
  const int mine = __popcll(m) | __popcll(mq) << 16;
  if (lane == 0) wave_tot[wave] = mine;
  __syncthreads();
  int x = wave_tot[lane & 15];
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);  // row_shr:1, lanes shifted in from outside the row read 0
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);
  total = __builtin_amdgcn_readlane(x, 15);
  return __builtin_amdgcn_readlane(x, wave) - mine + within;
}

// Static LDS: sized for up to SEL_MAX_CELLS 8x8-px cells (752x480 needs 96 x 62 = 5952 with the empty ring).  The
// workgroup must leave room on its CU for a workgroup of any other kernel of the pass (describe_tile_kernel is
// the largest at 39,344 B of the CU's 163,840 B; tests/test_select_footprint.py holds the sum), so the grid is
// packed: a corner accepted into a cell is identified by the low three bits of x and of y (the cell fixes the
// rest) -- one byte per slot, two slots = one u16 per cell -- and a list head is a batch rank < 1024 in a u16.
#define SEL_MAX_CELLS 6144
#define SEL_ACC_VALID 0x40u   // slot byte: valid | (y & 7) << 3 | (x & 7); 0 = empty
#define SEL_HEAD_EMPTY 0xFFFFu
// the key array is padded by one key per 32 (bank-conflict relief for the strided layouts of the sort)
#define SEL_KEYS_PADDED (SEL_CHUNK + SEL_CHUNK / 32)
#define SEL_PHYS(i) ((i) + ((i) >> 5))
// keys | SelShared | three SEL_THREADS-word arrays (bin counters of the sort, then batch nodes + states) | packed
// grid (2 B accepted slots + 2 B list head per cell) | pad.  The last of the three arrays, the grid and the pad
// together are the SEL_CHUNK-word staging array of the in-bin ranking when the candidate list is too long for the
// registers (the grid is initialised after it); the usual ranking from registers needs no staging array.
#define SEL_GRID_BYTES (SEL_MAX_CELLS * 2 * 2)
#define SEL_STAGE_PAD (SEL_CHUNK * 4 - SEL_THREADS * 4 - SEL_GRID_BYTES)
#define SEL_LDS_BYTES (SEL_KEYS_PADDED * 8 + 2048 + SEL_THREADS * 4 * 3 + SEL_GRID_BYTES + SEL_STAGE_PAD)
static_assert(SEL_STAGE_PAD >= 0, "ranking staging array");
// A candidate list of at most SEL_CHUNK keys is read from memory once and stays in registers through the counting
// sort, SEL_KPT keys per thread.  Up to SEL_CHUNK / 2 keys, the ranked positions (4 B) go straight to the part of the
// key array behind the last padded 8-byte key slot in use, 32-bit word SEL_POS_UPPER onwards.
#define SEL_KPT (SEL_CHUNK / SEL_THREADS)
#define SEL_POS_UPPER (2 * SEL_PHYS(SEL_CHUNK / 2))
static_assert(SEL_POS_UPPER + SEL_CHUNK / 2 <= 2 * SEL_KEYS_PADDED, "ranked positions behind the keys");
static_assert(SEL_LDS_BYTES <= 160 * 1024 - 39344, "selection kernel LDS budget: one describe_tile_kernel workgroup fits beside it");

// Exchange of the 16-bit half `idx & 1` of the 32-bit word that holds element idx of a u16 array (LDS has no
// 16-bit exchange): returns the old half.
// The per-cell arrays are volatile in global memory only (SelGrid below): a volatile access through a pointer that
// may be global or LDS compiles to a FLAT instruction with a full wait behind it, one serial round trip each, where
// the LDS grid wants plain ds_read / ds_write that are in flight together.  Workgroup barriers order the phases.
template <bool GRID_GLOBAL> struct SelGrid {
  typedef typename std::conditional<GRID_GLOBAL, volatile uint16_t, uint16_t>::type u16;
  typedef typename std::conditional<GRID_GLOBAL, volatile uint32_t, uint32_t>::type u32;
};

template <class T16>
__device__ __forceinline__ uint32_t sel_xchg16(T16* arr, int idx, uint32_t v) {
  uint32_t* word = (uint32_t*)arr + (idx >> 1);
  const int s = (idx & 1) * 16;
  uint32_t old;  // (a stale start value costs one more round)
  if constexpr (std::is_volatile<T16>::value) old = *(volatile uint32_t*)word;
  else old = *word;
  for (;;) {
    const uint32_t got = atomicCAS(word, old, (old & ~(0xFFFFu << s)) | (v << s));
    if (got == old) break;
    old = got;
  }
  return (old >> s) & 0xFFFFu;
}

// A list head as a batch rank, -1 = none.
__device__ __forceinline__ int sel_head_rank(uint32_t h) { return h == SEL_HEAD_EMPTY ? -1 : (int)h; }

// Put slot byte b into the first empty slot of cell idx (nothing if both are taken: a third corner at distance
// >= 8 from two others does not fit into an 8 x 8 cell).
template <class T16>
__device__ __forceinline__ void sel_acc_insert(T16* arr, int idx, uint32_t b) {
  uint32_t* word = (uint32_t*)arr + (idx >> 1);
  const int s = (idx & 1) * 16;
  uint32_t old;  // (slots only fill up: a stale value fails the exchange)
  if constexpr (std::is_volatile<T16>::value) old = *(volatile uint32_t*)word;
  else old = *word;
  for (;;) {
    const uint32_t cur = (old >> s) & 0xFFFFu;
    if ((cur & 0xFF00u) != 0u) break;
    const uint32_t got = atomicCAS(word, old, old | (b << (s + ((cur & 0xFFu) ? 8 : 0))));
    if (got == old) break;
    old = got;
  }
}

// Register-blocked bitonic network on N = REPS * (1024 << LOGK) keys in LDS (descending): a thread holds the
// 1 << LOGK keys whose indices differ in bits b .. b+LOGK-1, so up to LOGK consecutive sub-steps are
// compare-exchanges between its own registers; between such groups the keys pass through LDS once to change b.
// REPS = 2: a thread does this for two such sets in turn (four keys in registers, not eight, for 8192 keys).
template <int LOGK, int REPS>
__device__ __forceinline__ void sel_sort_blocked(uint64_t* keys, int tid0, int log_n) {
  constexpr int KPT = 1 << LOGK;
  for (int m = 1; m <= log_n; m++) {
    const int k = 1 << m;
    for (int top = m - 1; top >= 0;) {
      const int b = top >= LOGK - 1 ? top - (LOGK - 1) : 0;  // this group: bits top .. b
      const int nb = top - b + 1;
#pragma unroll 1
      for (int tid = tid0; tid < REPS * SEL_THREADS; tid += SEL_THREADS) {
      const int t_hi = tid >> b, t_lo = tid & ((1 << b) - 1);
      const int i0 = (t_hi << (b + LOGK)) | t_lo;  // index of the thread's key r = 0; key r sits at i0 | (r << b)
      uint64_t rk[KPT];
#pragma unroll
      for (int r = 0; r < KPT; r++) rk[r] = keys[SEL_PHYS(i0 | (r << b))];
#pragma unroll
      for (int x = LOGK - 1; x >= 0; x--) {
        if (x < nb) {
#pragma unroll
          for (int r = 0; r < KPT; r++) {
            if ((r & (1 << x)) == 0) {
              const bool desc = ((i0 | (r << b)) & k) == 0;
              const uint64_t u = rk[r], v = rk[r | (1 << x)];
              const bool sw = desc ? (u < v) : (u > v);
              rk[r] = sw ? v : u;
              rk[r | (1 << x)] = sw ? u : v;
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < KPT; r++) keys[SEL_PHYS(i0 | (r << b))] = rk[r];
      }
      __syncthreads();
      top = b - 1;
    }
  }
}

// GRID_GLOBAL = false: the accepted-corner grid and the batch list heads live in LDS (images of up to
// SEL_MAX_CELLS cells, e.g. 752 x 480).  GRID_GLOBAL = true: larger images keep the two per-cell arrays
// in a global scratch (grid_scratch, 3 words per cell per image, L2-resident) -- same algorithm, slower.
template <bool GRID_GLOBAL>
__global__ __launch_bounds__(SEL_THREADS) void select_kernel(const uint64_t* __restrict__ cand_all,
                                                             int32_t* meta,
                                                             int32_t* __restrict__ kp_xy, int32_t* __restrict__ kp_count,
                                                             int w, int h, size_t cand_cap, int F, int first,
                                                             int num_features, int border, double quality,
                                                             uint32_t* __restrict__ grid_scratch, int bucket_cap) {
  __shared__ __align__(16) unsigned char smem[SEL_LDS_BYTES];
  const int slot = first + blockIdx.x;
  const uint64_t* __restrict__ cand = cand_all + (size_t)slot * cand_cap;
  const int n_cand_raw = meta[(size_t)slot * VSL_META_STRIDE + VSL_META_NCAND];
  const int n_cand = min(n_cand_raw, (int)cand_cap);
  // 8 x 8-px cells with a ring of empty cells around the image: every 3 x 3 neighbourhood is nine fixed offsets, no
  // clamping, so its nine list heads / eighteen accepted slots are independent loads issued together
  const int gw = (w + 7) / 8 + 2, gh = (h + 7) / 8 + 2, cells = (gw * gh + 1) & ~1;  // (even: the arrays behind stay 8-byte aligned)
  // LDS carve-up (all regions 8-byte aligned)
  uint64_t* keys = (uint64_t*)smem;                 // SEL_CHUNK sorted keys (8 B), or their pixel positions (4 B, unpadded) after the in-bin ranking
  uint32_t* keys32 = (uint32_t*)smem;
  SelShared* sh = (SelShared*)(smem + SEL_KEYS_PADDED * 8);
  int* next = (int*)(smem + SEL_KEYS_PADDED * 8 + 2048);  // SEL_THREADS
  // cells u16 with the two accepted slots of a cell, then cells u16 batch list heads (SEL_HEAD_EMPTY = none); volatile
  // in the global variant, which must not keep them in registers / stale L1 lines between workgroup barriers
  typedef typename SelGrid<GRID_GLOBAL>::u16 grid_u16;
  typedef typename SelGrid<GRID_GLOBAL>::u32 grid_u32;
  grid_u16* acc = GRID_GLOBAL ? (grid_u16*)(grid_scratch + (size_t)slot * cells) : (grid_u16*)(next + 3 * SEL_THREADS);
  grid_u16* head = acc + cells;
  // batch member u: node[u] = (position x | y << 16, next member of its cell's list) -- one 8-byte read per list step
  unsigned long long* node = (unsigned long long*)next;  // SEL_THREADS (the space of `next` and the array after it)
  int* state = next + 2 * SEL_THREADS;              // SEL_THREADS: 0 undecided, 1 accepted, 2 rejected
  const int tid = threadIdx.x;

  int n_acc = 0, n_out = 0;
  unsigned long long hi = ~0ull;  // keys >= hi have been consumed
  int32_t* out = kp_xy + (size_t)slot * F * 2;
  // quality threshold (goodFeaturesToTrack: eig > maxVal * qualityLevel survives THRESH_TOZERO): the
  // provisional candidates at or below it do not exist as far as the rest of the kernel is concerned
  const float maxv = vsl_ordered_to_float(meta[(size_t)slot * VSL_META_STRIDE + VSL_META_MAX]);
  const float thr = (float)((double)maxv * quality);  // (K1's early cut uses the same expression)
  const unsigned long long floor_key =
      (((unsigned long long)((uint32_t)vsl_float_to_ordered(thr) ^ 0x80000000u)) << 32) | 0xFFFFFFFFull;
  int remaining = 0;
  // Sorting (first chunk, the normal case of at most SEL_CHUNK surviving candidates): a counting sort on the top
  // bits of the response -- SEL_BINS bins between the threshold and the maximum (both known), bin 0 = largest --
  // puts every key into its bin's slot range, and a key's final rank inside its bin is the number of larger keys
  // there (bins hold a handful of keys: the responses of real images spread over ~6 binades = ~850 bins).  Four
  // passes with a handful of workgroup barriers instead of the 49 LDS exchanges of the bitonic network for 8192
  // keys, which stays as the path for later chunks and for bins fuller than bucket_cap (plateaus of equal responses).
  int* bcount = next;                    // the three arrays alias next / cxy / state, which only the greedy uses
  int* bstart = next + SEL_THREADS;
  int* bcursor = next + 2 * SEL_THREADS;
  uint32_t* stage = (uint32_t*)bcursor;  // SEL_CHUNK positions in rank order: over bcursor (dead by then), the LDS grid and the pad
  static_assert(SEL_BINS == SEL_THREADS, "one bin per thread");
  const uint32_t hi_max = (uint32_t)vsl_float_to_ordered(maxv) ^ 0x80000000u;
  const uint32_t hi_floor = (uint32_t)vsl_float_to_ordered(thr) ^ 0x80000000u;
  int bshift = 16;
  while (bshift < 31 && (hi_max >> bshift) - (hi_floor >> bshift) >= (uint32_t)SEL_BINS) bshift++;
  const uint32_t bin_top = hi_max >> bshift;
  bool bucket_sort = false;
  // a list of at most SEL_CHUNK keys is held in registers from the histogram to the ranking: rk[k] = cand[tid + k * SEL_THREADS]
  // (compile-time indices only); a longer list takes the bucket path through memory twice, as before
  const bool in_regs = n_cand <= SEL_CHUNK;
  unsigned long long rk[SEL_KPT] = {};
  if (maxv > 0.f) {
    bcount[tid] = 0;
    if (tid == 0) sh->n_chunk = 0;
    __syncthreads();
    if (in_regs) {
      // the only read of the list: SEL_KPT independent loads per thread, issued together (0 = no key: below every floor)
#pragma unroll
      for (int k = 0; k < SEL_KPT; k++) {
        const int i = tid + k * SEL_THREADS;
        rk[k] = i < n_cand ? cand[i] : 0ull;
      }
#pragma unroll
      for (int k = 0; k < SEL_KPT; k++)
        if (rk[k] > floor_key) atomicAdd(&bcount[bin_top - min((uint32_t)(rk[k] >> 32) >> bshift, bin_top)], 1);
    } else {
      for (int i = tid; i < n_cand; i += SEL_THREADS) {
        const unsigned long long key = cand[i];
        if (key > floor_key) {
          // a provisional candidate above the image maximum cannot exist; the clamp keeps a corrupted list in range
          const uint32_t kb = min((uint32_t)(key >> 32) >> bshift, bin_top);
          atomicAdd(&bcount[bin_top - kb], 1);
        }
      }
    }
    __syncthreads();
    // exclusive prefix of the bin counts (bin 0 first = descending keys) and the fullest bin
    const int c = bcount[tid];
    int x = c;
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    int cmax = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o));
    if (lane == 63) sh->wave_tot[wv] = x;
    if (lane == 0) sh->hist[wv] = cmax;
    __syncthreads();
    int off = 0, fullest = 0;
    remaining = 0;  // number of surviving keys = the total of the bin counts (no per-thread atomic on one LDS word)
#pragma unroll
    for (int k = 0; k < 16; k++) {
      off += k < wv ? sh->wave_tot[k] : 0;
      remaining += sh->wave_tot[k];
      fullest = max(fullest, sh->hist[k]);
    }
    bstart[tid] = off + x - c;
    bcursor[tid] = 0;
    bucket_sort = remaining <= SEL_CHUNK && fullest <= bucket_cap;
    __syncthreads();
  }
  // the grid starts empty (two cells per word).  The counting sort from registers has no staging array over the grid,
  // so the grid is written here as well and the sort's own barriers stand between these writes and the greedy's
  // reads; the counting sort through memory does this itself after its staging array is dead.
  if (!bucket_sort || in_regs)
    for (int i = tid; i < cells; i += SEL_THREADS) ((grid_u32*)acc)[i] = i < (cells >> 1) ? 0u : ~0u;
  if (!bucket_sort) __syncthreads();
  bool compact = false;  // the sorted chunk is keys32[pos_off + r], not keys[SEL_PHYS(r)]
  int pos_off = 0;
  if (bucket_sort && remaining > 0) {
    if (in_regs) {
      // ---- scatter into the bins' slot ranges, then rank inside each bin (the keys come from the registers)
#pragma unroll
      for (int k = 0; k < SEL_KPT; k++)
        if (rk[k] > floor_key) {
          const int bin = (int)(bin_top - min((uint32_t)(rk[k] >> 32) >> bshift, bin_top));
          const int p = bstart[bin] + atomicAdd(&bcursor[bin], 1);  // (SEL_PHYS evaluates its argument twice)
          keys[SEL_PHYS(p)] = rk[k];
        }
      __syncthreads();
      // Only the pixel position of a key is read once it is ranked.  Up to SEL_CHUNK / 2 keys it goes straight to its
      // rank behind the key slots in use (no write meets a key that is still being compared).  Beyond that the
      // positions overwrite the keys, so a thread keeps rank << 32 | position in the key's register until every
      // thread has finished comparing (~0 = no key).  Either way there is no staging array and no copy pass: the
      // barrier that stood between the staging writes and the copy's reads, and the one between the copy and the
      // grid initialisation over the staging array, ordered accesses that no longer exist.
      // The keys are ranked by slot, not from the registers that scattered them: neighbouring slots lie in the same
      // bin, so the lanes of a wave walk the same few keys the same number of times.
      const bool upper = remaining <= SEL_CHUNK / 2;
#pragma unroll
      for (int k = 0; k < SEL_KPT; k++) {
        const int p = tid + k * SEL_THREADS;
        rk[k] = ~0ull;
        if (p < remaining) {
          const unsigned long long key = keys[SEL_PHYS(p)];
          const int bin = (int)(bin_top - min((uint32_t)(key >> 32) >> bshift, bin_top));
          const int s0 = bstart[bin], e0 = s0 + bcount[bin];
          int larger = 0;
          for (int q = s0; q < e0; q++) larger += keys[SEL_PHYS(q)] > key;
          if (upper) keys32[SEL_POS_UPPER + s0 + larger] = (uint32_t)key;
          else rk[k] = ((unsigned long long)(uint32_t)(s0 + larger) << 32) | (uint32_t)key;
        }
      }
      __syncthreads();
      if (upper) {
        pos_off = SEL_POS_UPPER;
      } else {
#pragma unroll
        for (int k = 0; k < SEL_KPT; k++)
          if ((uint32_t)(rk[k] >> 32) < (uint32_t)SEL_CHUNK) keys32[(uint32_t)(rk[k] >> 32)] = (uint32_t)rk[k];
        __syncthreads();
      }
    } else {
      // ---- the same through memory (more than SEL_CHUNK provisional candidates, at most SEL_CHUNK above the threshold)
      for (int i = tid; i < n_cand; i += SEL_THREADS) {
        const unsigned long long key = cand[i];
        if (key > floor_key) {
          const int bin = (int)(bin_top - min((uint32_t)(key >> 32) >> bshift, bin_top));
          const int p = bstart[bin] + atomicAdd(&bcursor[bin], 1);  // (SEL_PHYS evaluates its argument twice)
          keys[SEL_PHYS(p)] = key;
        }
      }
      __syncthreads();
      // the position goes to its rank in the staging array (no key is held in registers across a barrier), and the
      // staging array is copied over the keys
      for (int p = tid; p < remaining; p += SEL_THREADS) {
        const unsigned long long key = keys[SEL_PHYS(p)];
        const int bin = (int)(bin_top - min((uint32_t)(key >> 32) >> bshift, bin_top));
        const int s0 = bstart[bin], e0 = s0 + bcount[bin];
        int larger = 0;
        for (int q = s0; q < e0; q++) larger += keys[SEL_PHYS(q)] > key;
        stage[s0 + larger] = (uint32_t)key;
      }
      __syncthreads();
      for (int p = tid; p < remaining; p += SEL_THREADS) keys32[p] = stage[p];
      __syncthreads();
      for (int i = tid; i < cells; i += SEL_THREADS) ((grid_u32*)acc)[i] = i < (cells >> 1) ? 0u : ~0u;
      __syncthreads();
    }
    compact = true;
  }

  while (remaining > 0 && n_acc < num_features) {
    // ---- choose the chunk [lo, hi): all remaining keys, or the SEL_CHUNK largest of them
    unsigned long long lo = 0;
    if (remaining > SEL_CHUNK) {
      unsigned long long prefix = 0;
      int k = SEL_CHUNK;  // the k-th largest key below hi, most significant byte first
      for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += SEL_THREADS) sh->hist[i] = 0;
        __syncthreads();
        const unsigned long long pmask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (int i = tid; i < n_cand; i += SEL_THREADS) {
          const unsigned long long key = cand[i];
          if (key < hi && key > floor_key && (key & pmask) == prefix) atomicAdd(&sh->hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (tid == 0) {
          int kk = k, d = 255;
          for (; d > 0; d--) {
            if (sh->hist[d] >= kk) break;
            kk -= sh->hist[d];
          }
          sh->sel_k = kk;
          sh->sel_prefix = prefix | ((unsigned long long)d << shift);
        }
        __syncthreads();
        k = sh->sel_k;
        prefix = sh->sel_prefix;
        __syncthreads();
      }
      lo = prefix;  // = the SEL_CHUNK-th largest remaining key (keys are unique)
    }
    int n_chunk;
    if (compact) {
      n_chunk = remaining;  // the counting sort above ranked all of them (at most SEL_CHUNK: this is the only turn of the loop)
    } else {
      // ---- gather the chunk into LDS and pad to a power of two
      if (tid == 0) sh->n_chunk = 0;
      __syncthreads();
      for (int i = tid; i < n_cand; i += SEL_THREADS) {
        const unsigned long long key = cand[i];
        if (key >= lo && key < hi && key > floor_key) {
          const int p = atomicAdd(&sh->n_chunk, 1);
          if (p < SEL_CHUNK) keys[SEL_PHYS(p)] = key;
        }
      }
      __syncthreads();
      n_chunk = min(sh->n_chunk, SEL_CHUNK);
      int N = 1024;
      while (N < n_chunk) N <<= 1;
      for (int i = n_chunk + tid; i < N; i += SEL_THREADS) keys[SEL_PHYS(i)] = 0ull;
      __syncthreads();
      // ---- bitonic sort, descending.  With 2 or 4 keys per thread in registers (N = 2048; 4096 and, in two turns,
      // 8192) the network is register-blocked (sel_sort_blocked): ceil(m / log2(keys in registers)) LDS exchanges for
      // the stage k = 2^m, e.g. 49 workgroup barriers for 8192 keys instead of 91 (one per sub-step).
      if (N >= 2048) {
        if (N == 8192) sel_sort_blocked<2, 2>(keys, tid, 13);
        else if (N == 4096) sel_sort_blocked<2, 1>(keys, tid, 12);
        else sel_sort_blocked<1, 1>(keys, tid, 11);
      } else {
        for (int k = 2; k <= N; k <<= 1) {
          for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (N >> 1); t += SEL_THREADS) {
              const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
              const int l = i | j;
              const uint64_t a = keys[SEL_PHYS(i)], b = keys[SEL_PHYS(l)];
              const bool desc = (i & k) == 0;
              if (desc ? (a < b) : (a > b)) {
                keys[SEL_PHYS(i)] = b;
                keys[SEL_PHYS(l)] = a;
              }
            }
            __syncthreads();
          }
        }
      }
    }
    // ---- greedy, SEL_THREADS ranks per batch
    for (int r0 = 0; r0 < n_chunk && n_acc < num_features; r0 += SEL_THREADS) {
      const int r = r0 + tid;
      int px = 0, py = 0, cell = 0;
      bool alive = false;
      if (r < n_chunk) {
        const uint32_t pix = compact ? keys32[pos_off + r] :(uint32_t)(keys[SEL_PHYS(r)] & 0xFFFFFFFFull);
        py = (int)(pix >> 16);
        px = (int)(pix & 0xFFFFu);
        cell = ((py >> 3) + 1) * gw + (px >> 3) + 1;
        // a slot of the neighbour cell at offset (ox, oy) holds the low bits of a corner there: its distance is
        // (x & 7) - 8 ox - slot x, likewise in y -- the px - ax, py - ay of the unpacked coordinates
        const int lx = px & 7, ly = py & 7;
        int near = 0;  // branch-free: eighteen short-circuit tests compile to eighteen exec-mask branches
#pragma unroll
        for (int oy = -1; oy <= 1; oy++) {
          const int row = cell + oy * gw;
          const uint32_t t0 = acc[row - 1], t1 = acc[row], t2 = acc[row + 1];  // a row of three cells at a time
#pragma unroll
          for (int k = 0; k < 6; k++) {
            const uint32_t b = ((k >> 1) == 0 ? t0 : (k >> 1) == 1 ? t1 : t2) >> (8 * (k & 1));
            const int dx = lx - 8 * ((k >> 1) - 1) - (int)(b & 7u), dy = ly - 8 * oy - (int)((b >> 3) & 7u);
            const unsigned d2 = (unsigned)(dx * dx) + (unsigned)(dy * dy);
            near |= (int)((b & SEL_ACC_VALID) != 0u) & (int)(d2 < 64u);
          }
        }
        alive = near == 0;
      }
      state[tid] = alive ? 0 : 2;
      {
        const uint32_t prev = alive ? sel_xchg16(head, cell, (uint32_t)tid) : SEL_HEAD_EMPTY;
        const int nxt = sel_head_rank(prev);
        node[tid] = ((unsigned long long)(uint32_t)nxt << 32) | ((uint32_t)px | ((uint32_t)py << 16));
      }
      __syncthreads();
      // Blockers = higher-ranked survivors of this batch within the minimum distance.  A candidate is
      // decided once all of them are: rejected if one was accepted, accepted otherwise.  The lowest
      // undecided rank never waits, so free-running polling of the LDS state words terminates; no
      // workgroup barrier per dependency level (all 16 waves are resident and keep being scheduled).
      // The state words are read and written as relaxed workgroup-scope atomics: every turn of the polling loop
      // loads them again, as a volatile access would, but as plain ds_read / ds_write -- a blocker's six words are
      // in flight together, where six volatile reads were six serial FLAT round trips.
      int nb = 0;
      unsigned long long blk = 0ull;  // the last SEL_MAX_BLOCKERS blockers, 10 bits each (batch-local ranks): a register ARRAY
                                      // indexed by nb costs six compare / select pairs per insertion
      if (alive) {
#pragma unroll 1
        for (int oy = -1; oy <= 1; oy++) {  // a row of three list heads at a time
          const int row = cell + oy * gw;
          uint32_t h3[3];
#pragma unroll
          for (int k = 0; k < 3; k++) h3[k] = head[row + k - 1];
#pragma unroll
          for (int k = 0; k < 3; k++)
            for (int u = sel_head_rank(h3[k]); u >= 0;) {
              const unsigned long long nd = node[u];
              const int uu = u;
              u = (int)(nd >> 32);
              if (uu < tid) {
                const uint32_t q = (uint32_t)nd;
                const int dx = px - (int)(q & 0xFFFF), dy = py - (int)(q >> 16);
                if (dx * dx + dy * dy < 64) {
                  blk = (blk << 10) | (unsigned long long)(unsigned)uu;
                  nb++;
                }
              }
            }
        }
      }
      bool undecided = alive, accepted = false;  // accepted: the thread's own decision (its state word is for the others)
      while (__ballot(undecided) != 0ull) {
        if (undecided) {
          bool rej = false, blocked = false;
          if (nb <= SEL_MAX_BLOCKERS) {
#pragma unroll
            for (int k = 0; k < SEL_MAX_BLOCKERS; k++)
              if (k < nb) {
                const int su = __hip_atomic_load(&state[(int)(blk >> (10 * k)) & 1023], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                rej = rej || (su == 1);
                blocked = blocked || (su == 0);
              }
          } else {  // crowded neighbourhood: walk the cell lists again
            for (int k = 0; k < 9; k++)
                for (int u = sel_head_rank(head[cell + (k / 3 - 1) * gw + (k % 3 - 1)]), un = -1; u >= 0; u = un) {
                  const unsigned long long nd = node[u];
                  un = (int)(nd >> 32);
                  if (u < tid) {
                    const uint32_t q = (uint32_t)nd;
                    const int dx = px - (int)(q & 0xFFFF), dy = py - (int)(q >> 16);
                    if (dx * dx + dy * dy < 64) {
                      const int su = __hip_atomic_load(&state[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                      rej = rej || (su == 1);
                      blocked = blocked || (su == 0);
                    }
                  }
                }
          }
          const int ns = rej ? 2 : (blocked ? 0 : 1);
          if (ns) {
            __hip_atomic_store(&state[tid], ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            undecided = false;
            accepted = ns == 1;
          }
        }
        __builtin_amdgcn_s_sleep(1);
      }
      // One scan for both counts: accepted corners (low half) and accepted corners inside the border (high half).
      // The cap at num_features keeps a PREFIX of the accepted corners in thread order, so a kept corner has only kept
      // corners before it and its output position is the packed prefix as it stands; when the cap cuts this batch
      // (workgroup-uniform, and the last batch then), the first corner that is cut has exactly the kept ones before
      // it and publishes their number inside the border as the batch's total.
      // Barriers: the one that stood here ordered the polling loop's reads of head / node / state before the reset
      // of head below and the next batch's writes -- the scan's barrier does that now, every thread reaching it after
      // its polling loop.  The scan's former leading barrier ordered the previous scan's reads of wave_tot before this
      // write: with one scan per batch, the trailing barrier of the previous batch stands between them.
      const bool inside = px >= border && px < w - border && py >= border && py < h - border;
      int total = 0;
      const int pre = block_scan(accepted, accepted && inside, sh->wave_tot, total);
      const int lim = num_features - n_acc;       // accepted corners this batch may still keep (> 0)
      const bool cut = (total & 0xFFFF) > lim;
      const bool keep = accepted && (pre & 0xFFFF) < lim;
      const bool inb = keep && inside;
      if (inb) {
        const int pos = n_out + (pre >> 16);
        out[2 * pos] = px;
        out[2 * pos + 1] = py;
      }
      if (cut && accepted && (pre & 0xFFFF) == lim) sh->sel_k = pre >> 16;
      if (keep) sel_acc_insert(acc, cell, SEL_ACC_VALID | (uint32_t)((py & 7) << 3) | (uint32_t)(px & 7));
      if (alive) head[cell] = (uint16_t)SEL_HEAD_EMPTY;
      n_acc = min(num_features, n_acc + (total & 0xFFFF));
      __syncthreads();
      n_out += cut ? sh->sel_k : total >> 16;
    }
    hi = lo;
    remaining -= n_chunk;
  }
  if (tid == 0) {
    kp_count[slot] = n_out;
    // every thread read MAX / NCAND before the first barrier: leave them reset for the next detect call
    meta[(size_t)slot * VSL_META_STRIDE + VSL_META_NCAND_LAST] = n_cand_raw;
    meta[(size_t)slot * VSL_META_STRIDE + VSL_META_MAX_LAST] = vsl_float_to_ordered(maxv);
    meta[(size_t)slot * VSL_META_STRIDE + VSL_META_MAX] = INT32_MIN;
    meta[(size_t)slot * VSL_META_STRIDE + VSL_META_NCAND] = 0;
  }
}

// Diagnostic: the response kernel's square root against the correctly rounded library sqrtf on every float bit
// pattern in [lo_bits, hi_bits] (both must be non-negative floats); *n_mismatch = number of differing results.
extern "C" int vsl_diag_sqrt_check(vsl_ctx* ctx, uint32_t lo_bits, uint32_t hi_bits, unsigned long long* n_mismatch) {
  if (!ctx || !n_mismatch || lo_bits > hi_bits || hi_bits > 0x7f7fffffu)
    return vsl_fail(ctx, VSL_ERR_INVALID, "vsl_diag_sqrt_check: bad range");
  VSL_HIP(ctx, hipSetDevice(ctx->device));
  void* d = nullptr;
  int rc = vsl_ctx_dscratch(ctx, sizeof(unsigned long long), &d);
  if (rc) return rc;
  VSL_HIP(ctx, hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(sqrt_check_kernel, dim3(4096), dim3(256), 0, ctx->stream, lo_bits, hi_bits, (unsigned long long*)d);
  VSL_CHECK_LAUNCH(ctx);
  VSL_HIP(ctx, hipMemcpyAsync(n_mismatch, d, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  VSL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VSL_OK;
}

int vsl_launch_detect(vsl_ctx* ctx, vsl_frames* f, int first, int n, int num_features) {
  if (n <= 0) return VSL_OK;
  if (num_features < 1 || num_features > f->F)
    return vsl_fail(ctx, VSL_ERR_INVALID, "num_features %d not in [1, %d]", num_features, f->F);
  static_assert(sizeof(SelShared) <= 2048, "SelShared fits its LDS slot");
  const int cells = (((f->w + 7) / 8 + 2) * ((f->h + 7) / 8 + 2) + 1) & ~1;  // with the ring of empty cells, even (as select_kernel counts them)
  const bool grid_global = cells > SEL_MAX_CELLS;
  if (grid_global && !f->sel_grid) {
    VSL_HIP(ctx, hipMalloc((void**)&f->sel_grid, sizeof(uint32_t) * (size_t)cells * f->max_images));
  }
  const int w = f->w, h = f->h;
  {
    VslStage st(ctx, VSL_STAGE_RESPONSE);
    if (f->detect_meta_dirty)
      hipLaunchKernelGGL(detect_init_kernel, dim3((f->max_images + 255) / 256), dim3(256), 0, ctx->stream, f->meta, 0, f->max_images);
    f->detect_meta_dirty = true;  // until the selection kernel (which resets the counters) is in the queue
    // strips of K1_ROWS rows for batches; short strips for launches of a few images (the tracking loop's one-image calls):
    // a lone wave per SIMD issues one instruction per ~7 cycles, so such a launch is as long as its longest wave
    const bool small = n < 8 && !f->store_response;
    const int rows = small ? K1_ROWS_SMALL : K1_ROWS;
    const int strips_y = (h + rows - 1) / rows;
    const int tiles_x = (w + K1_COLS - 1) / K1_COLS;
    const dim3 k1_grid((unsigned)((tiles_x * strips_y + 3) / 4) * (unsigned)(n >= 8 ? 8 * ((n + 7) / 8) : n));  // four strips per workgroup
    const int wcap = ctx->k1_list_cap < 0 ? K1_WLIST : min(ctx->k1_list_cap, K1_WLIST);
    if (f->store_response)
      hipLaunchKernelGGL((min_eig_response_kernel<true, K1_ROWS>), k1_grid, dim3(256), 0, ctx->stream, f->images, f->response, f->meta,
                         f->cand, f->cand_cap, w, h, first, wcap, n, tiles_x, strips_y);
    else if (small)
      hipLaunchKernelGGL((min_eig_response_kernel<false, K1_ROWS_SMALL>), k1_grid, dim3(256), 0, ctx->stream, f->images, f->response, f->meta,
                         f->cand, f->cand_cap, w, h, first, wcap, n, tiles_x, strips_y);
    else
      hipLaunchKernelGGL((min_eig_response_kernel<false, K1_ROWS>), k1_grid, dim3(256), 0, ctx->stream, f->images, f->response, f->meta,
                         f->cand, f->cand_cap, w, h, first, wcap, n, tiles_x, strips_y);
    VSL_CHECK_LAUNCH(ctx);
  }
  {
    VslStage st(ctx, VSL_STAGE_SELECT);
    if (grid_global)
      hipLaunchKernelGGL(select_kernel<true>, dim3(n), dim3(SEL_THREADS), 0, ctx->stream, f->cand, f->meta, f->kp_xy,
                         f->kp_count, w, h, f->cand_cap, f->F, first, num_features, 19, VSL_QUALITY_LEVEL, f->sel_grid, ctx->select_bucket_cap);
    else
      hipLaunchKernelGGL(select_kernel<false>, dim3(n), dim3(SEL_THREADS), 0, ctx->stream, f->cand, f->meta, f->kp_xy,
                         f->kp_count, w, h, f->cand_cap, f->F, first, num_features, 19, VSL_QUALITY_LEVEL, (uint32_t*)nullptr,
                         ctx->select_bucket_cap);
    VSL_CHECK_LAUNCH(ctx);
  }
  f->detect_meta_dirty = false;
  return VSL_OK;
}
