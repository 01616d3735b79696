// Helpers shared by the fused decoder tails (pd_decoder_tail.hip: DepthDecoder, softmax; pd_plade_tail.hip: PladeNet,
// alpha compositing; pd_tail_infer.hip: both, forward only): sigma's sigmoid + clamp, PX pixels per thread as one access per
// tensor and plane (16 bytes of fp32, 8 bytes of bf16 under PD_TAIL_BF16), the upstream gradient of disp, the block partials of
// a per-plane disparity gradient, the inference kernels' best plane and an entry point's launch shape.  The device helpers
// are free functions on the caller's own values, so a kernel compiles to what it was with the expressions written in place.
#pragma once
#include <initializer_list>
#include <stdint.h>

#include "pd_common.h"

namespace pd {

constexpr float kTailSigmaMin = 0.01f, kTailSigmaMax = 1.0f;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float clamp_sigma(float s) { return fminf(fmaxf(s, kTailSigmaMin), kTailSigmaMax); }
// depth = tail_depth_scale(W) / disp (depth_decoder.py:291, plade_net.py:340; the same constant turns disp_layered into depth layers)
__device__ __forceinline__ float tail_depth_scale(int W) { return 0.1f * 0.58f * (float)W; }

// PX pixels per thread: 4 (one access per tensor and plane: 16 bytes of fp32, 8 bytes of bf16) when H*W is a multiple of 4
// and every pointer is aligned to that access, else 1.  The arithmetic is per pixel, in fp32, either way.
template <int PX>
struct Px {
  float v[PX];
};
template <int PX>
__device__ __forceinline__ Px<PX> ldv(const float* __restrict__ p) {
  Px<PX> r;
  if (PX == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1 % PX] = t.y; r.v[2 % PX] = t.z; r.v[3 % PX] = t.w;
  } else {
    r.v[0] = p[0];
  }
  return r;
}
template <int PX>
__device__ __forceinline__ void stv(float* __restrict__ p, const Px<PX>& r) {
  if (PX == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1 % PX], r.v[2 % PX], r.v[3 % PX]);
  else p[0] = r.v[0];
}
// Storage-typed forms (PD_TAIL_BF16: raw_logits / raw_sigma, logits / sigma and their gradients hold bf16).  A load widens
// exactly; a store rounds each element once, to nearest even (pack_bf16x2).  4 pixels are one 8-byte access.
template <int PX>
__device__ __forceinline__ Px<PX> ldv(const Bf16* __restrict__ p) {
  Px<PX> r;
  if (PX == 4) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    r.v[0] = bf16_lo(t.x); r.v[1 % PX] = bf16_hi(t.x); r.v[2 % PX] = bf16_lo(t.y); r.v[3 % PX] = bf16_hi(t.y);
  } else {
    r.v[0] = __uint_as_float((unsigned)p[0] << 16);
  }
  return r;
}
template <int PX>
__device__ __forceinline__ void stv(Bf16* __restrict__ p, const Px<PX>& r) {
  if (PX == 4) *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(r.v[0], r.v[1 % PX]), pack_bf16x2(r.v[2 % PX], r.v[3 % PX]));
  else p[0] = (Bf16)pack_bf16x2(r.v[0], 0.0f);
}
template <int PX>
__device__ __forceinline__ Px<PX> splat(float x) {
  Px<PX> r;
#pragma unroll
  for (int j = 0; j < PX; ++j) r.v[j] = x;
  return r;
}

// Upstream gradient of disp at a lane's pixels (p1 = b * HW + pix): g_disp plus g_depth through depth = c / disp.  Either may be NULL.
template <int PX>
__device__ __forceinline__ Px<PX> tail_upstream(const float* __restrict__ g_disp, const float* __restrict__ g_depth, long p1,
                                                const Px<PX>& dsp, float c) {
  Px<PX> gD = splat<PX>(0.0f);
  if (g_disp) gD = ldv<PX>(g_disp + p1);
  if (g_depth) {
    const Px<PX> gz = ldv<PX>(g_depth + p1);
#pragma unroll
    for (int j = 0; j < PX; ++j) gD.v[j] -= gz.v[j] * c / (dsp.v[j] * dsp.v[j]);
  }
  return gD;
}

// Block partials of a per-plane disparity gradient (tail_bwd_kernel, plade_bwd_kernel): red[N] in LDS collects the waves' sums
// with LDS atomics, then goes to partials[b][block][N] for reduce_partials.  Every thread of the workgroup calls all three.
__device__ __forceinline__ void block_partials_zero(float* red, int N) {
  for (int i = threadIdx.x; i < N; i += kBlock) red[i] = 0.0f;
  __syncthreads();
}
__device__ __forceinline__ void block_partials_add(float* red, int n, float lane_sum) {
  const float v = wave_sum_hi(lane_sum);
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) lds_add(&red[n], v);
}
__device__ __forceinline__ void block_partials_store(const float* red, float* __restrict__ partials, int b, int N) {
  __syncthreads();
  float* dst = partials + ((long)b * gridDim.x + blockIdx.x) * N;
  for (int i = threadIdx.x; i < N; i += kBlock) dst[i] = red[i];
}

// Inference kernels: plane n's weight w against the best so far.  Strict: the lower index keeps a tie (plane 0 stands where
// every weight is 0).
__device__ __forceinline__ void keep_best(int n, float w, float& w_best, int& n_best) {
  if (n == 0 || w > w_best) {
    w_best = w; n_best = n;
  }
}
template <int PX>
__device__ __forceinline__ void stv_idx(int* __restrict__ p, const int (&r)[PX]) {
  if (PX == 4) *reinterpret_cast<int4*>(p) = make_int4(r[0], r[1 % PX], r[2 % PX], r[3 % PX]);
  else p[0] = r[0];
}

// 4 pixels per thread when every row of 4 is whole and aligned to its access in every tensor involved: `ptrs` hold fp32 (16
// bytes), `storage` the tensors that PD_TAIL_BF16 turns into bf16 (8 bytes then, 16 without the flag).  The decoder tail's row
// forms ([B,N,H] operands, read as scalars and not listed here) additionally ask for W % 4 == 0, so that the 4 pixels share a
// row (tail_launch).
static inline int tail_px(int H, int W, std::initializer_list<const void*> ptrs, std::initializer_list<const void*> storage,
                          bool bf16) {
  if (((long)H * W) % 4 != 0) return 1;
  for (const void* p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15)) return 1;
  for (const void* p : storage)
    if (p && (reinterpret_cast<uintptr_t>(p) & (bf16 ? 7 : 15))) return 1;
  return 4;
}

// The launch shape every pixel-linear tail kernel shares: the storage type, the pixels per lane (tail_px; a row form, rf != 0,
// takes 4 only when a group of 4 cannot straddle two rows) and one lane per PX pixels, one grid row per image.
struct TailLaunch {
  bool bf16;
  int px;
  dim3 grid;
};
static inline TailLaunch tail_launch(int B, int H, int W, int flags, int rf, std::initializer_list<const void*> ptrs,
                                     std::initializer_list<const void*> storage) {
  TailLaunch t;
  t.bf16 = (flags & PD_TAIL_BF16) != 0;
  t.px = (rf && W % 4 != 0) ? 1 : tail_px(H, W, ptrs, storage, t.bf16);
  t.grid = dim3(ceil_div(ceil_div(H * W, t.px), kBlock), B);
  return t;
}

}  // namespace pd
