// What the decoder tail's sources share (pd_decoder_tail.hip: training forward, layers, backward; pd_tail_infer.hip: the
// forward-only inference kernel): the kernel arguments, where a lane's pixels lie, a plane's operands, one plane of the online
// softmax and its per-pixel finish (the training forward and the inference kernel call the same two functions, which is what
// makes their disp / depth / stash equal bit for bit), argument validation and the dispatch over the template parameters
// <ST, MIX, HASMASK, PX, RF>.
#pragma once
#include "pd_tail_common.h"

namespace pd {

struct TailArgs {
  int N, HW, W;
  int mix, dense;
  const float* raw_logits;
  const float* raw_sigma;
  const float* mask;   // may be NULL (all ones)
  const float* dl;     // [B,N] or [B,N,H,W]; [B,N,H] in the row form (so is `mask` then)
};

constexpr int kRowDisp = 1, kRowMask = 2;   // RF bits: disp_layered / padding_mask are [B,N,H]
// the row-form operand of plane n for a lane whose PX pixels lie in row y; `rows` = the image's [N,H] block
template <int PX>
__device__ __forceinline__ Px<PX> ld_row(const float* __restrict__ rows, int n, int H, int y) {
  return splat<PX>(rows[(long)n * H + y]);
}

// Where a lane's PX pixels lie: image b, plane 0's element `base` of a [B,N,H,W] tensor, and (row forms) row y of H with the
// image's [N,H] block at `rbase`.
struct TailLane {
  int b, H, y;
  long base, rbase;
};
// a pixel-linear lane at `pix` (row form: W % PX == 0 there, so the PX pixels share the row)
template <int RF>
__device__ __forceinline__ TailLane tail_lane(const TailArgs& a, int b, int pix) {
  TailLane ln;
  ln.b = b;
  ln.H = RF ? a.HW / a.W : 0;
  ln.y = RF ? pix / a.W : 0;
  ln.base = (long)b * a.N * a.HW + pix;
  ln.rbase = (long)b * a.N * ln.H;
  return ln;
}

// Plane n's operands at a lane: mask (ones without one), raw logit, raw sigma (mixture only) and, with DV, the disparity, each
// in the form <HASMASK, RF> and a.dense name.  `i` = ln.base + n * HW.  (Filled in place: returned by value, the struct cost
// some one-pixel kernels a register.)
template <int PX>
struct TailOperands {
  Px<PX> mk, rl, rs, dv;
};
template <class ST, bool MIX, bool HASMASK, int PX, int RF, bool DV = true>
__device__ __forceinline__ void tail_operands(const TailArgs& a, const TailLane& ln, int n, long i, TailOperands<PX>& o) {
  o.mk = !HASMASK ? splat<PX>(1.0f) : (RF & kRowMask) ? ld_row<PX>(a.mask + ln.rbase, n, ln.H, ln.y) : ldv<PX>(a.mask + i);
  o.rl = ldv<PX>(elems<ST>(a.raw_logits) + i);
  o.rs = MIX ? ldv<PX>(elems<ST>(a.raw_sigma) + i) : splat<PX>(0.0f);
  o.dv = !DV ? splat<PX>(0.0f) : (RF & kRowDisp) ? ld_row<PX>(a.dl + ln.rbase, n, ln.H, ln.y)
                                                 : a.dense ? ldv<PX>(a.dl + i) : splat<PX>(a.dl[ln.b * a.N + n]);
}

// One plane of the online softmax at one pixel.  In: the raw logit, raw sigma, mask and disparity.  Out: the masked logit l,
// the clamped sigma sg (mixture only) and the plane's weight w = e^(l-m) * mask / sigma in the units of the reference m.
// Updated: m, sum e^(l-m), sum of weights, sum w*d.  BEST (inference): w_best, the best weight so far, is kept in the units
// of m as well — rescaled with the sums when m moves; the caller compares w against it afterwards (keep_best).
template <bool MIX, bool BEST>
__device__ __forceinline__ void tail_softmax_step(float rl, float rs, float mk, float dv, float& m, float& Z, float& Sw,
                                                  float& Sd, float& w_best, float& l, float& sg, float& w) {
  l = rl * mk;                                                   // depth_decoder.py:259
  float inv = 1.0f;
  if (MIX) {
    sg = clamp_sigma(sigmoid_f(rs));                             // :278-279
    inv = mk / sg;                                               // :282-283 (mask applied to the weights)
  }
  if (l > m) {  // move the reference to the new maximum
    const float sc = __expf(m - l);
    Z *= sc; Sw *= sc; Sd *= sc;
    if (BEST) w_best *= sc;
    m = l;
  }
  const float e = __expf(l - m);
  w = e * inv;
  Z += e;
  Sw += w;
  Sd += w * dv;
}
// and the pixel's results once every plane is in (c = tail_depth_scale(W))
__device__ __forceinline__ void tail_softmax_finish(float m, float Z, float Sw, float Sd, float c, float& disp, float& depth,
                                                    float& lse, float& sn) {
  disp = Sd / Sw;                                                // :284-285, 289 (the softmax normaliser cancels)
  depth = c / disp;                                              // :291
  lse = m + __logf(Z);                                           // log-sum-exp of the masked logits
  sn = Sw / Z;                                                   // sum_N pi * mask / sigma
}

static int tail_validate(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                         const float* mask, const float* dl) {
  PD_REQUIRE(B > 0 && B <= 65535 && N > 0 && H > 0 && W > 0, "bad shape");
  PD_REQUIRE((long)H * W < (1L << 31), "image too large");
  PD_REQUIRE((flags & ~(PD_TAIL_MIXTURE | PD_TAIL_DISP_DENSE | PD_TAIL_BF16 | PD_TAIL_DISP_ROWS | PD_TAIL_MASK_ROWS)) == 0,
             "unknown flags");
  PD_REQUIRE(!((flags & PD_TAIL_DISP_ROWS) && (flags & PD_TAIL_DISP_DENSE)),
             "PD_TAIL_DISP_ROWS and PD_TAIL_DISP_DENSE exclude each other (disp_layered is [B,N,H] or [B,N,H,W])");
  // (a row form's refusal names its flag and the layout that flag announces: a caller that set bit 8 or 16 by accident — they
  // were unknown flags before the row forms existed — learns from the text what the bit made of its tensors)
  PD_REQUIRE(!(flags & PD_TAIL_DISP_ROWS) || (raw_logits && dl),
             "NULL pointer (PD_TAIL_DISP_ROWS in flags: disp_layered is read as [B,N,H])");
  PD_REQUIRE(raw_logits && dl, "NULL pointer");
  PD_REQUIRE(!(flags & PD_TAIL_MASK_ROWS) || mask, "NULL pointer (PD_TAIL_MASK_ROWS in flags: padding_mask is read as [B,N,H])");
  PD_REQUIRE(!(flags & PD_TAIL_MIXTURE) || raw_sigma, "mixture needs raw_sigma");
  return 0;
}

static TailArgs tail_args(int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                          const float* mask, const float* dl) {
  TailArgs a;
  a.N = N; a.HW = H * W; a.W = W;
  a.mix = (flags & PD_TAIL_MIXTURE) != 0;
  a.dense = (flags & PD_TAIL_DISP_DENSE) != 0;
  a.raw_logits = raw_logits; a.raw_sigma = raw_sigma; a.mask = mask; a.dl = dl;
  return a;
}

// RF of a call: which of disp_layered / padding_mask are [B,N,H]
static inline int tail_rf(int flags, const float* mask) {
  return ((flags & PD_TAIL_DISP_ROWS) ? kRowDisp : 0) | ((mask && (flags & PD_TAIL_MASK_ROWS)) ? kRowMask : 0);
}

#define PD_TAIL_DISPATCH_PX(KERNEL, T, PX, RF, mix, hasmask, grid, block, shmem, stream, ...)                \
  do {                                                                                                       \
    if (mix) {                                                                                               \
      if (hasmask) KERNEL<T, true, true, PX, RF><<<grid, block, shmem, stream>>>(__VA_ARGS__);               \
      else         KERNEL<T, true, false, PX, (RF) & ~kRowMask><<<grid, block, shmem, stream>>>(__VA_ARGS__); \
    } else {                                                                                                 \
      if (hasmask) KERNEL<T, false, true, PX, RF><<<grid, block, shmem, stream>>>(__VA_ARGS__);              \
      else         KERNEL<T, false, false, PX, (RF) & ~kRowMask><<<grid, block, shmem, stream>>>(__VA_ARGS__); \
    }                                                                                                        \
  } while (0)
#define PD_TAIL_DISPATCH_T(KERNEL, T, RF, px, mix, hasmask, grid, block, shmem, stream, ...)                 \
  do {                                                                                                       \
    if ((px) == 4) PD_TAIL_DISPATCH_PX(KERNEL, T, 4, RF, mix, hasmask, grid, block, shmem, stream, __VA_ARGS__); \
    else           PD_TAIL_DISPATCH_PX(KERNEL, T, 1, RF, mix, hasmask, grid, block, shmem, stream, __VA_ARGS__); \
  } while (0)
// RF is a constant here
#define PD_TAIL_DISPATCH(KERNEL, RF, bf16, px, mix, hasmask, grid, block, shmem, stream, ...)                \
  do {                                                                                                       \
    if (bf16) PD_TAIL_DISPATCH_T(KERNEL, Bf16, RF, px, mix, hasmask, grid, block, shmem, stream, __VA_ARGS__); \
    else      PD_TAIL_DISPATCH_T(KERNEL, float, RF, px, mix, hasmask, grid, block, shmem, stream, __VA_ARGS__); \
  } while (0)
// The run-time rf (tail_rf) of a call.  A kernel that exists for one setting of the disparity bit only (layers and the
// pixel-linear backward: DISP = 0; the row-owned backward: kRowDisp) names it and dispatches over the mask bit; a kernel with
// all four forms dispatches over both.  Only the forms named here are instantiated.
#define PD_TAIL_DISPATCH_MASK(KERNEL, DISP, rf, ...)                                                         \
  do {                                                                                                       \
    if ((rf) & kRowMask) PD_TAIL_DISPATCH(KERNEL, (DISP) | kRowMask, __VA_ARGS__);                           \
    else                 PD_TAIL_DISPATCH(KERNEL, DISP, __VA_ARGS__);                                        \
  } while (0)
#define PD_TAIL_DISPATCH_RF(KERNEL, rf, ...)                                                                 \
  do {                                                                                                       \
    if ((rf) & kRowDisp) PD_TAIL_DISPATCH_MASK(KERNEL, kRowDisp, rf, __VA_ARGS__);                           \
    else                 PD_TAIL_DISPATCH_MASK(KERNEL, 0, rf, __VA_ARGS__);                                  \
  } while (0)

}  // namespace pd
