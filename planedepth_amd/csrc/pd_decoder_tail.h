// What the decoder tail's sources share (pd_decoder_tail.hip: training forward, layers, backward; pd_tail_infer.hip: the
// forward-only inference kernel): the kernel arguments, the row-form operand, argument validation, the choice of the lane
// width for a row form and the dispatch over the template parameters <ST, MIX, HASMASK, PX, RF>.
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
// A row form takes 4 pixels per lane only when a group of 4 cannot straddle two rows
static inline int tail_px_rows(int px, int rf, int W) { return (rf && W % 4 != 0) ? 1 : px; }

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
// RF is a constant here: the callers branch on tail_rf() and name the forms their kernel has
#define PD_TAIL_DISPATCH(KERNEL, RF, bf16, px, mix, hasmask, grid, block, shmem, stream, ...)                \
  do {                                                                                                       \
    if (bf16) PD_TAIL_DISPATCH_T(KERNEL, Bf16, RF, px, mix, hasmask, grid, block, shmem, stream, __VA_ARGS__); \
    else      PD_TAIL_DISPATCH_T(KERNEL, float, RF, px, mix, hasmask, grid, block, shmem, stream, __VA_ARGS__); \
  } while (0)

}  // namespace pd
