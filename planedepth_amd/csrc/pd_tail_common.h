// Helpers shared by the fused decoder tails (pd_decoder_tail.hip: DepthDecoder, softmax; pd_plade_tail.hip: PladeNet,
// alpha compositing): sigma's sigmoid + clamp, and PX pixels per thread as one access per tensor and plane (16 bytes of
// fp32, 8 bytes of bf16 under PD_TAIL_BF16).
#pragma once
#include <initializer_list>
#include <stdint.h>

#include "pd_common.h"

namespace pd {

constexpr float kTailSigmaMin = 0.01f, kTailSigmaMax = 1.0f;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float clamp_sigma(float s) { return fminf(fmaxf(s, kTailSigmaMin), kTailSigmaMax); }

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

// 4 pixels per thread when every row of 4 is whole and aligned to its access in every tensor involved: `ptrs` hold fp32 (16
// bytes), `storage` the tensors that PD_TAIL_BF16 turns into bf16 (8 bytes then, 16 without the flag).  The decoder tail's row
// forms ([B,N,H] operands, read as scalars and not listed here) additionally ask for W % 4 == 0, so that the 4 pixels share a
// row (pd_decoder_tail.h: tail_px_rows).
static inline int tail_px(int H, int W, std::initializer_list<const void*> ptrs, std::initializer_list<const void*> storage,
                          bool bf16) {
  if (((long)H * W) % 4 != 0) return 1;
  for (const void* p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15)) return 1;
  for (const void* p : storage)
    if (p && (reinterpret_cast<uintptr_t>(p) & (bf16 ? 7 : 15))) return 1;
  return 4;
}

}  // namespace pd
