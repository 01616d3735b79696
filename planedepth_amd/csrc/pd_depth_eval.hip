// Depth evaluation on the device: the Eigen metrics of evaluate_depth_HR.py (:148-166, :217-279) and the in-training
// metrics of Trainer.compute_depth_losses (trainer.py:775-810 with layers.py:356-374), one kernel family for both.
//
// The contract (every constant fp32 unless marked; `planedepth_amd/metrics.py` carries the same text):
//
// A. offline evaluation, per image i (prediction [M,h,w], or [2M,h,w] under PD_EVAL_POST_PROCESS; GT gt_h x gt_w)
//   1. post-process: d = 0.5f * (pred[i] + fliplr(pred[i+M])) at the source resolution (:51-59, only m_disp is live),
//      fused into the resize by averaging each tap pair before it is interpolated (= "average, then resize", bitwise);
//   2. cv2.resize(d, (gt_w, gt_h)), INTER_LINEAR, as OpenCV 4's coefficient setup + resizeGeneric_ state it:
//      inv = (double)gt_w / w, scale = 1.0 / inv (fp64); fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx),
//      f = fx - sx; columns: sx < 0 -> (0, f = 0), sx >= w-1 -> (w-1, f = 0, one tap); rows: the same fy / sy / f,
//      both tap rows clamped to [0, h-1] and the fraction KEPT (top / bottom: r0*(1-f) + r0*f, can be 1 ulp off r0);
//      horizontal a*(1-f) + b*f first, then vertical, fp32, no FMA contraction;
//   3. depth = disp_num / disp with disp_num = float32(0.1*0.58*width), a correctly rounded fp32 division;
//   4. PD_EVAL_EIGEN: valid = 1e-3f < gt < 80 (the clamp of GT to [1e-3, 80] cannot move a valid pixel) inside the crop
//      [y0,y1) x [x0,x1) of `meta`; otherwise valid = gt > 0 (the caller passes the whole image as the crop);
//   5. depth *= scale_factor (1 mono, 5.4 --eval_stereo);
//   6. PD_EVAL_MEDIAN: ratio = med(gt_valid) / med(depth_valid), numpy's median (even count: (a + b) fp32, then halved;
//      empty set or any NaN: NaN), depth *= ratio;
//   7. depth clamped to [1e-3, 80] by compare-and-replace (NaN stays NaN);
//   8. per image: thresh = max(gt/d, d/gt); #(thresh < 1.25^k); sums of (gt-d)^2, (log gt - log d)^2, |gt-d|/gt,
//      (gt-d)^2/gt over the fp32 terms, in fp64 and in a fixed order -> abs_rel, sq_rel, rmse, rmse_log, a1..a3.
// B. PD_EVAL_TRAINER, pooled over the whole batch (one segment): `pred` is depth [M,1,h,w] at the GT's resolution,
//   d = clamp((depth * 2) / (grid[b,0,y,gw-1] - grid[b,0,y,0]), 1e-3, 80) (one divisor per row, :784-785);
//   valid = gt > 0 inside the crop; gt_v = clamp(gt, 1e-3, 80); PD_EVAL_MEDIAN (opt.no_stereo):
//   d *= lower_median(gt_v) / lower_median(d_v) (torch.median: the lower middle value), else d *= scale_factor (5.4);
//   no clamp afterwards; the same metrics.
//
// Passes (all integer merges are vector atomicAdd on global memory; no float atomics: two launches are bit-identical):
//   gather   one workgroup per (image, tile of PD_EVAL_TILE GT pixels): 16-byte GT loads, the prediction only at valid
//            pixels, (gt, depth) pairs compacted into the tile's slot in a fixed (lane, pixel) order (one block scan);
//   select   PD_EVAL_MEDIAN only: exact radix select of the two medians, 4 passes of 8 bits over the fp32 bits mapped
//            to an order-preserving uint; LDS histograms per workgroup merged into per-segment histograms, then one
//            small kernel per pass picks the digit of each of the 4 order statistics (gt lo / hi, depth lo / hi);
//   metrics  per tile fp64 partial sums in a fixed order, then one fixed-order reduce per segment.
#include <math.h>

#include "pd_common.h"

namespace pd {

constexpr int kTile = PD_EVAL_TILE;             // GT pixels per gather workgroup (and pair slots per tile)
constexpr int kQuadIters = kTile / (4 * kBlock);   // 16 float4 per lane
static_assert(kQuadIters * 4 * kBlock == kTile, "tile = 256 lanes x 16 quads");
constexpr int kBins = 256, kTargets = 4;

struct SegState {
  uint32_t n;                  // valid pixels of the segment
  uint32_t nan_d;              // of them with a NaN depth (the gt of a valid pixel is never NaN)
  uint32_t prefix[kTargets];   // radix-select prefixes: gt lo, gt hi, depth lo, depth hi
  uint32_t rank[kTargets];     // rank still to find inside the prefix's bucket
  float med[2];                // median of gt_v, of depth_v
  float ratio;
  uint32_t pad;
};

struct EvalWs {   // workspace carve-up, shared by the size query and the launch
  size_t pairs, tile_count, tile_sums, tile_hits, state, hist, total;
  EvalWs(int M, int max_tiles, int S) {
    const size_t T = (size_t)M * max_tiles;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    pairs = take(T * kTile * sizeof(float2));
    tile_count = take(T * sizeof(int));
    tile_sums = take(T * 4 * sizeof(double));
    tile_hits = take(T * 4 * sizeof(int));
    state = take((size_t)S * sizeof(SegState));
    hist = take((size_t)S * kTargets * kBins * sizeof(uint32_t));
    total = o;
  }
};

struct EvalArgs {
  int M, h, w, flags, max_tiles, grid_w;
  float disp_num, scale_factor;
  const float* pred;
  const float* grid;
  const float* gt;
  const int64_t* meta;   // [M][8]: gt offset (floats), gt_h, gt_w, y0, y1, x0, x1, 0
  float2* pairs;
  int* tile_count;
  double* tile_sums;
  int* tile_hits;
  SegState* state;
  uint32_t* hist;
};

__device__ __forceinline__ uint32_t order_key(float v) {   // monotone map of the fp32 bits (-0 sorts just below +0)
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}

__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) {   // torch.clamp: NaN propagates
  return (v != v) ? v : fminf(fmaxf(v, lo), hi);
}

// One source tap of the (optionally post-processed) disparity: 0.5f * (l[r][c] + r[r][w-1-c]).
__device__ __forceinline__ float src_tap(const float* __restrict__ a, const float* __restrict__ b, int r, int c, int w) {
#pragma clang fp contract(off)
  const float v = a[(long)r * w + c];
  return b ? 0.5f * (v + b[(long)r * w + (w - 1 - c)]) : v;
}

// cv2.resize INTER_LINEAR at destination pixel (y, x) (contract point A2).
__device__ __forceinline__ float resize_at(const float* __restrict__ a, const float* __restrict__ b, int h, int w, int y, int x,
                                           double scale_y, double scale_x) {
#pragma clang fp contract(off)
  const float fx = (float)(((double)x + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  float ax = fx - (float)sx;
  bool one_tap = false;
  if (sx < 0) { sx = 0; ax = 0.0f; }
  if (sx >= w - 1) { sx = w - 1; ax = 0.0f; one_tap = true; }
  const float fy = (float)(((double)y + 0.5) * scale_y - 0.5);
  const int sy = (int)floorf(fy);
  const float ay = fy - (float)sy;
  const int r0 = min(max(sy, 0), h - 1), r1 = min(max(sy + 1, 0), h - 1);
  const float bx = 1.0f - ax;
  float h0 = src_tap(a, b, r0, sx, w) * bx, h1 = src_tap(a, b, r1, sx, w) * bx;
  if (!one_tap) {
    h0 = h0 + src_tap(a, b, r0, sx + 1, w) * ax;
    h1 = h1 + src_tap(a, b, r1, sx + 1, w) * ax;
  }
  return h0 * (1.0f - ay) + h1 * ay;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ uint64_t lanes_below() {
  const int l = lane_id();
  return l ? (~0ull >> (kWave - l)) : 0ull;
}

// ---- gather ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void eval_gather_kernel(EvalArgs A) {
#pragma clang fp contract(off)
  __shared__ int wave_tot[kBlock / kWave];
  __shared__ int nan_block;
  const int tile = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const int64_t* m = A.meta + (long)img * 8;
  const long off = m[0];
  const int H = (int)m[1], W = (int)m[2], y0 = (int)m[3], y1 = (int)m[4], x0 = (int)m[5], x1 = (int)m[6];
  const long HW = (long)H * W;
  const long slot = (long)img * A.max_tiles + tile;
  const long p_begin = (long)tile * kTile;
  if (p_begin >= HW) {   // a tile past this image's end (the grid is sized by the largest image)
    if (tid == 0) A.tile_count[slot] = 0;
    return;
  }
  if (tid == 0) nan_block = 0;
  const bool trainer = A.flags & PD_EVAL_TRAINER, eigen = A.flags & PD_EVAL_EIGEN;
  const float* gt = A.gt + off;
  const float* pa = A.pred + (long)img * A.h * A.w;
  const float* pb = (A.flags & PD_EVAL_POST_PROCESS) ? A.pred + (long)(img + A.M) * A.h * A.w : nullptr;
  const double scale_x = 1.0 / ((double)W / (double)A.w), scale_y = 1.0 / ((double)H / (double)A.h);

  const bool aligned = (off & 3) == 0;
  // 1. all 16 quads of the lane in flight at once; keep only the bit mask of the evaluated pixels
  float4 q[kQuadIters];
#pragma unroll
  for (int it = 0; it < kQuadIters; ++it) {
    const long p = p_begin + 4L * (it * kBlock + tid);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (pixels past the end read as 0: never valid)
    if (aligned && p + 3 < HW) {
      v = *reinterpret_cast<const float4*>(gt + p);
    } else {
      if (p < HW) v.x = gt[p];
      if (p + 1 < HW) v.y = gt[p + 1];
      if (p + 2 < HW) v.z = gt[p + 2];
      if (p + 3 < HW) v.w = gt[p + 3];
    }
    q[it] = v;
  }
  uint64_t valid = 0;   // bit 4*it + k: pixel p_begin + 4*(it*256 + tid) + k is in the evaluated set (value rule and crop)
#pragma unroll
  for (int it = 0; it < kQuadIters; ++it) {
    const int p = (int)p_begin + 4 * (it * kBlock + tid);   // (an image has < 2^31 pixels)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float g = k == 0 ? q[it].x : k == 1 ? q[it].y : k == 2 ? q[it].z : q[it].w;
      if (eigen ? (g > 1e-3f && g < 80.0f) : (g > 0.0f)) {
        const int y = (p + k) / W, x = (p + k) - y * W;
        if (y >= y0 && y < y1 && x >= x0 && x < x1) valid |= 1ull << (4 * it + k);
      }
    }
  }
  // 2. one block-wide exclusive scan of the lanes' counts: slots in (lane, pixel) order, fixed for a given input
  const int c = __popcll(valid);
  int incl = c;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(incl, d, kWave);
    if (lane_id() >= d) incl += t;
  }
  const int wave = tid >> 6;
  if (lane_id() == kWave - 1) wave_tot[wave] = incl;
  __syncthreads();
  int pos = incl - c, total = 0;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    const int t = wave_tot[w];
    pos += w < wave ? t : 0;
    total += t;
  }
  // 3. the prediction only where it is evaluated (a few per cent of the pixels); the GT value again from the cache
  float2* out = A.pairs + slot * kTile;
  int nan_d = 0;
  while (valid) {
    const int bit = __ffsll((unsigned long long)valid) - 1;
    valid &= valid - 1;
    const int pk = (int)p_begin + 4 * ((bit >> 2) * kBlock + tid) + (bit & 3);
    const int y = pk / W, x = pk - y * W;
    const float g = gt[pk];
    float gv = g, d;
    if (trainer) {
      d = __int_as_float(0x7fc00000);
      if (y < A.h && x < A.w) {   // (a GT larger than the prediction is refused by the caller; never read past it)
        const long row = (long)img * A.h + y;
        const float div = A.grid[row * A.grid_w + (A.grid_w - 1)] - A.grid[row * A.grid_w];
        d = clamp_keep_nan((pa[(long)y * A.w + x] * 2.0f) / div, 1e-3f, 80.0f);
      }
      gv = clamp_keep_nan(g, 1e-3f, 80.0f);
    } else {
      d = (A.disp_num / resize_at(pa, pb, A.h, A.w, y, x, scale_y, scale_x)) * A.scale_factor;
    }
    nan_d += d != d;
    out[pos++] = make_float2(gv, d);
  }
  const int base = total;
  if (nan_d) atomicAdd(&nan_block, nan_d);
  __syncthreads();
  if (tid == 0) {
    A.tile_count[slot] = base;
    const int seg = trainer ? 0 : img;
    if (base) atomicAdd(&A.state[seg].n, (uint32_t)base);
    if (nan_block) atomicAdd(&A.state[seg].nan_d, (uint32_t)nan_block);
  }
}

// ---- radix select -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void eval_zero_kernel(SegState* __restrict__ state, uint32_t* __restrict__ hist, int S) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < (long)S * kTargets * kBins) hist[i] = 0u;
  if (i < S) {
    SegState z = {};
    state[i] = z;
  }
}

// Histogram of digit `pass` (bits 31-24 first) of the keys that still match each target's prefix.  Targets whose prefix
// equals the previous target's (lo and hi inside one bucket: always at pass 0) share that target's histogram.
__global__ __launch_bounds__(kBlock) void eval_hist_kernel(EvalArgs A, int pass) {
  __shared__ uint32_t h[kTargets * kBins];
  const int tile = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const long slot = (long)img * A.max_tiles + tile;
  const int cnt = A.tile_count[slot];
  if (cnt == 0) return;
  const int seg = (A.flags & PD_EVAL_TRAINER) ? 0 : img;
  const SegState& st = A.state[seg];
  const int shift = 24 - 8 * pass;
  uint32_t pre[kTargets];
  bool own[kTargets];
#pragma unroll
  for (int j = 0; j < kTargets; ++j) {
    pre[j] = pass ? (st.prefix[j] >> (shift + 8)) : 0u;
    own[j] = !(j & 1) || st.prefix[j] != st.prefix[j - 1];
  }
  for (int i = tid; i < kTargets * kBins; i += kBlock) h[i] = 0u;
  __syncthreads();
  const float2* in = A.pairs + slot * kTile;
  for (int i = tid; i < cnt; i += kBlock) {
    const float2 pr = in[i];
    const uint32_t key[2] = {order_key(pr.x), order_key(pr.y)};
#pragma unroll
    for (int j = 0; j < kTargets; ++j) {
      const uint32_t k = key[j >> 1];
      if (own[j] && (pass == 0 || (k >> (shift + 8)) == pre[j])) atomicAdd(&h[j * kBins + ((k >> shift) & 255u)], 1u);
    }
  }
  __syncthreads();
  uint32_t* g = A.hist + (long)seg * kTargets * kBins;
  for (int i = tid; i < kTargets * kBins; i += kBlock)
    if (h[i]) atomicAdd(&g[i], h[i]);
}

// One workgroup per segment: the digit of each target at `pass`, then the histograms are cleared for the next pass.
// After the last pass: the medians and the ratio.
__global__ __launch_bounds__(kWave) void eval_select_kernel(SegState* __restrict__ state, uint32_t* __restrict__ hist, int pass,
                                                            int lower_median) {
  const int seg = blockIdx.x, tid = threadIdx.x;
  SegState& st = state[seg];
  uint32_t* g = hist + (long)seg * kTargets * kBins;
  const uint32_t n = st.n;
  const int shift = 24 - 8 * pass;
  uint32_t prefix = 0, rank = 0;
  int src = tid;
  if (tid < kTargets) {
    prefix = st.prefix[tid];
    rank = st.rank[tid];
    if (pass == 0) rank = (tid & 1) && !lower_median ? n / 2 : (n ? (n - 1) / 2 : 0u);
    if ((tid & 1) && prefix == st.prefix[tid - 1]) src = tid - 1;
  }
  __syncthreads();
  if (tid < kTargets && n) {
    uint32_t cum = 0, digit = 0;
    for (; digit < (uint32_t)kBins; ++digit) {
      const uint32_t c = g[src * kBins + digit];
      if (rank < cum + c) break;
      cum += c;
    }
    st.prefix[tid] = prefix | (digit << shift);
    st.rank[tid] = rank - cum;
  }
  __syncthreads();
  for (int i = tid; i < kTargets * kBins; i += kWave) g[i] = 0u;
  if (pass == 3 && tid == 0) {
#pragma clang fp contract(off)
    const float nan = __int_as_float(0x7fc00000);
    float mg = nan, md = nan;
    if (n) {
      const float g_lo = key_value(st.prefix[0]), g_hi = key_value(st.prefix[1]);
      const float d_lo = key_value(st.prefix[2]), d_hi = key_value(st.prefix[3]);
      mg = lower_median ? g_lo : (g_lo + g_hi) * 0.5f;
      md = st.nan_d ? nan : (lower_median ? d_lo : (d_lo + d_hi) * 0.5f);
    }
    st.med[0] = mg;
    st.med[1] = md;
    st.ratio = mg / md;
  }
}

// ---- metrics ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__global__ __launch_bounds__(kBlock) void eval_metrics_kernel(EvalArgs A) {
#pragma clang fp contract(off)
  __shared__ double red_s[kBlock / kWave][4];
  __shared__ int red_h[kBlock / kWave][3];
  const int tile = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const long slot = (long)img * A.max_tiles + tile;
  const int cnt = A.tile_count[slot];
  const bool trainer = A.flags & PD_EVAL_TRAINER;
  const int seg = trainer ? 0 : img;
  const float factor = (A.flags & PD_EVAL_MEDIAN) ? A.state[seg].ratio : (trainer ? A.scale_factor : 1.0f);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int hit[3] = {0, 0, 0};
  const float2* in = A.pairs + slot * kTile;
  for (int i = tid; i < cnt; i += kBlock) {
    const float2 pr = in[i];
    const float g = pr.x;
    float d = pr.y * factor;
    if (!trainer) {   // compare-and-replace: NaN stays NaN
      if (d < 1e-3f) d = 1e-3f;
      if (d > 80.0f) d = 80.0f;
    }
    const float th = fmaxf(g / d, d / g);
    const bool nan_th = th != th;   // (fmaxf drops one NaN operand; numpy's maximum propagates it)
    hit[0] += !nan_th && th < 1.25f;
    hit[1] += !nan_th && th < 1.5625f;
    hit[2] += !nan_th && th < 1.953125f;
    const float e = g - d, e2 = e * e;
    const float lg = (float)log((double)g), ld = (float)log((double)d);
    const float le = lg - ld;
    s[0] += (double)(fabsf(e) / g);
    s[1] += (double)(e2 / g);
    s[2] += (double)e2;
    s[3] += (double)(le * le);
  }
  const int wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum_d(s[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) hit[k] = wave_sum_i(hit[k]);
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red_s[wave][k] = s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) red_h[wave][k] = hit[k];
  }
  __syncthreads();
  if (tid < 4) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) v += red_s[w][tid];
    A.tile_sums[slot * 4 + tid] = v;
  } else if (tid < 7) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) v += red_h[w][tid - 4];
    A.tile_hits[slot * 4 + (tid - 4)] = v;
  }
}

// One workgroup per segment: its tiles in a fixed order -> metrics [S,7], ratio [S], medians [S,2], counts [S,4].
__global__ __launch_bounds__(kBlock) void eval_final_kernel(EvalArgs A, float* __restrict__ metrics, float* __restrict__ ratio,
                                                            float* __restrict__ medians, int32_t* __restrict__ counts) {
  __shared__ double red_s[kBlock / kWave][4];
  __shared__ int red_h[kBlock / kWave][3];
  const int seg = blockIdx.x, tid = threadIdx.x;
  const bool trainer = A.flags & PD_EVAL_TRAINER;
  const long t0 = trainer ? 0 : (long)seg * A.max_tiles;
  const long t1 = trainer ? (long)A.M * A.max_tiles : t0 + A.max_tiles;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int hit[3] = {0, 0, 0};
  for (long t = t0 + tid; t < t1; t += kBlock) {
    if (!A.tile_count[t]) continue;   // (empty tiles wrote zeros, or nothing at all past the image's end)
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += A.tile_sums[t * 4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) hit[k] += A.tile_hits[t * 4 + k];
  }
  const int wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum_d(s[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) hit[k] = wave_sum_i(hit[k]);
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red_s[wave][k] = s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) red_h[wave][k] = hit[k];
  }
  __syncthreads();
  if (tid) return;
  double S[4] = {0.0, 0.0, 0.0, 0.0};
  int Hh[3] = {0, 0, 0};
  for (int w = 0; w < kBlock / kWave; ++w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) S[k] += red_s[w][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Hh[k] += red_h[w][k];
  }
  const SegState& st = A.state[seg];
  const double n = (double)st.n;   // 0 -> every metric is 0/0 = NaN, as numpy's mean of an empty set
  float* o = metrics + (long)seg * 7;
  o[0] = (float)(S[0] / n);
  o[1] = (float)(S[1] / n);
  o[2] = (float)sqrt(S[2] / n);
  o[3] = (float)sqrt(S[3] / n);
  for (int k = 0; k < 3; ++k) o[4 + k] = (float)((double)Hh[k] / n);
  const bool median = A.flags & PD_EVAL_MEDIAN;
  const float nan = __int_as_float(0x7fc00000);
  ratio[seg] = median ? st.ratio : (trainer ? A.scale_factor : 1.0f);
  medians[seg * 2] = median ? st.med[0] : nan;
  medians[seg * 2 + 1] = median ? st.med[1] : nan;
  int32_t* c = counts + (long)seg * 4;
  c[0] = (int32_t)st.n;
  for (int k = 0; k < 3; ++k) c[1 + k] = Hh[k];
}

// ---- resize only (the map step A2 produces, for checks and for callers that want cv2.resize on the device) -------
__global__ __launch_bounds__(kBlock) void eval_resize_kernel(int M, int h, int w, const float* __restrict__ pred, int post_process,
                                                             const int64_t* __restrict__ meta, float* __restrict__ out) {
  const int img = blockIdx.y;
  const int64_t* m = meta + (long)img * 8;
  const int H = (int)m[1], W = (int)m[2];
  const long p = (long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (long)H * W) return;
  const int y = (int)p / W, x = (int)p - y * W;
  const float* pa = pred + (long)img * h * w;
  const float* pb = post_process ? pred + (long)(img + M) * h * w : nullptr;
  out[m[0] + p] = resize_at(pa, pb, h, w, y, x, 1.0 / ((double)H / (double)h), 1.0 / ((double)W / (double)w));
}

static int eval_segments(int M, int flags) { return (flags & PD_EVAL_TRAINER) ? 1 : M; }

static int check_eval_args(int M, int h, int w, int flags, int max_tiles) {
  PD_REQUIRE(M > 0 && M <= 65535 && h > 0 && w > 0 && (long)h * w < (1L << 31), "bad shape");
  PD_REQUIRE(max_tiles > 0 && (long)max_tiles * kTile < (1L << 31) && max_tiles <= (1 << 20), "bad max_tiles");
  PD_REQUIRE(!(flags & ~(PD_EVAL_POST_PROCESS | PD_EVAL_EIGEN | PD_EVAL_MEDIAN | PD_EVAL_TRAINER)), "unknown eval flags");
  PD_REQUIRE(!((flags & PD_EVAL_TRAINER) && (flags & (PD_EVAL_POST_PROCESS | PD_EVAL_EIGEN))),
             "eval flags: PD_EVAL_TRAINER takes neither PD_EVAL_POST_PROCESS nor PD_EVAL_EIGEN");
  return PD_OK;
}

}  // namespace pd

using namespace pd;

extern "C" size_t pd_depth_eval_workspace_bytes(int M, int max_tiles, int flags) {
  if (check_eval_args(M, 1, 1, flags, max_tiles) != PD_OK) return 0;
  return EvalWs(M, max_tiles, eval_segments(M, flags)).total;
}

extern "C" int pd_depth_eval(int M, int h, int w, int flags, int max_tiles, float disp_num, float scale_factor,
                             const float* pred, const float* grid, int grid_w, const float* gt, const int64_t* meta,
                             void* workspace, float* metrics, float* ratio, float* medians, int32_t* counts,
                             pd_stream_t stream) {
  const int rc = check_eval_args(M, h, w, flags, max_tiles);
  if (rc != PD_OK) return rc;
  PD_REQUIRE(pred && gt && meta && workspace && metrics && ratio && medians && counts, "NULL pointer");
  PD_REQUIRE(!(flags & PD_EVAL_TRAINER) || (grid && grid_w > 0), "PD_EVAL_TRAINER needs the grid (NULL pointer or grid_w < 1)");
  const int S = eval_segments(M, flags);
  const EvalWs L(M, max_tiles, S);
  char* ws = static_cast<char*>(workspace);
  EvalArgs A;
  A.M = M; A.h = h; A.w = w; A.flags = flags; A.max_tiles = max_tiles; A.grid_w = grid_w;
  A.disp_num = disp_num; A.scale_factor = scale_factor;
  A.pred = pred; A.grid = grid; A.gt = gt; A.meta = meta;
  A.pairs = reinterpret_cast<float2*>(ws + L.pairs);
  A.tile_count = reinterpret_cast<int*>(ws + L.tile_count);
  A.tile_sums = reinterpret_cast<double*>(ws + L.tile_sums);
  A.tile_hits = reinterpret_cast<int*>(ws + L.tile_hits);
  A.state = reinterpret_cast<SegState*>(ws + L.state);
  A.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
  hipStream_t s = (hipStream_t)stream;
  const dim3 tiles(max_tiles, M);
  eval_zero_kernel<<<ceil_div(S * kTargets * kBins, kBlock), kBlock, 0, s>>>(A.state, A.hist, S);
  eval_gather_kernel<<<tiles, kBlock, 0, s>>>(A);
  if (flags & PD_EVAL_MEDIAN) {
    for (int pass = 0; pass < 4; ++pass) {
      eval_hist_kernel<<<tiles, kBlock, 0, s>>>(A, pass);
      eval_select_kernel<<<S, kWave, 0, s>>>(A.state, A.hist, pass, (flags & PD_EVAL_TRAINER) ? 1 : 0);
    }
  }
  eval_metrics_kernel<<<tiles, kBlock, 0, s>>>(A);
  eval_final_kernel<<<S, kBlock, 0, s>>>(A, metrics, ratio, medians, counts);
  return check_launch("pd_depth_eval");
}

extern "C" int pd_depth_eval_resize(int M, int h, int w, int flags, int max_hw, const float* pred, const int64_t* meta,
                                    float* out, pd_stream_t stream) {
  PD_REQUIRE(M > 0 && M <= 65535 && h > 0 && w > 0 && (long)h * w < (1L << 31) && max_hw > 0, "bad shape");
  PD_REQUIRE(!(flags & ~PD_EVAL_POST_PROCESS), "pd_depth_eval_resize takes PD_EVAL_POST_PROCESS only (bad flags)");
  PD_REQUIRE(pred && meta && out, "NULL pointer");
  const dim3 grid(ceil_div(max_hw, kBlock), M);
  eval_resize_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(M, h, w, pred, flags & PD_EVAL_POST_PROCESS, meta, out);
  return check_launch("pd_depth_eval_resize");
}
