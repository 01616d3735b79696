// What the PladeNet tail's sources share (pd_plade_tail.hip: training forward, layers, backward; pd_tail_infer.hip: the
// forward-only inference kernel): the kernel arguments, the disparity operand, argument validation and the dispatch over the
// template parameters <ST, MIX, PX>.
#pragma once
#include "pd_tail_common.h"

namespace pd {

struct PladeArgs {
  int N, HW, W;
  int mix, dense;
  const float* raw_logits;   // [B,N-1,H,W]
  const float* raw_sigma;    // [B,N,H,W]
  const float* dl;           // [B,N] or [B,N,H,W]
  const float* ray;          // [H*W]
};

template <int PX>
__device__ __forceinline__ Px<PX> plade_disp(const PladeArgs& a, int b, int n, long pix) {
  return a.dense ? ldv<PX>(a.dl + ((long)b * a.N + n) * a.HW + pix) : splat<PX>(a.dl[b * a.N + n]);
}

static int plade_validate(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                          const float* dl, const float* ray) {
  PD_REQUIRE(B > 0 && B <= 65535 && N >= 2 && H > 0 && W > 0, "bad shape (alpha compositing needs N >= 2 planes)");
  PD_REQUIRE((long)H * W < (1L << 31), "image too large");
  PD_REQUIRE((flags & ~(PD_TAIL_MIXTURE | PD_TAIL_DISP_DENSE | PD_TAIL_BF16)) == 0, "unknown flags");
  PD_REQUIRE(raw_logits && dl && ray, "NULL pointer");
  PD_REQUIRE(!(flags & PD_TAIL_MIXTURE) || raw_sigma, "mixture needs raw_sigma");
  return 0;
}

static PladeArgs plade_args(int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma, const float* dl,
                            const float* ray) {
  PladeArgs a;
  a.N = N; a.HW = H * W; a.W = W;
  a.mix = (flags & PD_TAIL_MIXTURE) != 0;
  a.dense = (flags & PD_TAIL_DISP_DENSE) != 0;
  a.raw_logits = raw_logits; a.raw_sigma = raw_sigma; a.dl = dl; a.ray = ray;
  return a;
}

#define PD_PLADE_DISPATCH_T(KERNEL, T, px, mix, grid, shmem, stream, ...)                                   \
  do {                                                                                                       \
    if ((px) == 4) { if (mix) KERNEL<T, true, 4><<<grid, kBlock, shmem, stream>>>(__VA_ARGS__);              \
                     else     KERNEL<T, false, 4><<<grid, kBlock, shmem, stream>>>(__VA_ARGS__); }           \
    else           { if (mix) KERNEL<T, true, 1><<<grid, kBlock, shmem, stream>>>(__VA_ARGS__);              \
                     else     KERNEL<T, false, 1><<<grid, kBlock, shmem, stream>>>(__VA_ARGS__); }           \
  } while (0)
#define PD_PLADE_DISPATCH(KERNEL, bf16, px, mix, grid, shmem, stream, ...)                                  \
  do {                                                                                                       \
    if (bf16) PD_PLADE_DISPATCH_T(KERNEL, Bf16, px, mix, grid, shmem, stream, __VA_ARGS__);                  \
    else      PD_PLADE_DISPATCH_T(KERNEL, float, px, mix, grid, shmem, stream, __VA_ARGS__);                 \
  } while (0)

}  // namespace pd
