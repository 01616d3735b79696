// What the PladeNet tail's sources share (pd_plade_tail.hip: training forward, layers, backward; pd_tail_infer.hip: the
// forward-only inference kernel): the kernel arguments, a plane's operands, the compositing step of one plane at one pixel, the
// mixture weight and the per-pixel finish (the training forward and the inference kernel call the same functions, which is what
// makes their disp / depth / stash equal bit for bit), argument validation and the dispatch over the template parameters
// <ST, MIX, PX>.
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

// Plane n's operands at a lane: the disparity of the NEXT plane (the last plane: its own, `dv`), the raw logit (the last plane
// has none: alpha = 1) and raw sigma (mixture only).  plade_fwd_kernel fills the struct itself (see there).
template <int PX>
struct PladeOperands {
  Px<PX> dn, rl, rs;
};
template <class ST, bool MIX, int PX>
__device__ __forceinline__ void plade_operands(const PladeArgs& a, int b, int n, long pix, const Px<PX>& dv, PladeOperands<PX>& o) {
  const bool last = (n == a.N - 1);
  if (last) {   // (branches, not ?: on the struct's members: those leave aggregate selects behind, and a register with them)
    o.dn = dv;
    o.rl = splat<PX>(0.0f);
  } else {
    o.dn = plade_disp<PX>(a, b, n + 1, pix);
    o.rl = ldv<PX>(elems<ST>(a.raw_logits) + ((long)b * (a.N - 1) + n) * a.HW + pix);
  }
  o.rs = MIX ? ldv<PX>(elems<ST>(a.raw_sigma) + ((long)b * a.N + n) * a.HW + pix) : splat<PX>(0.0f);
}

// Plane n at one pixel: the next depth layer zn, the distance to it along the ray, alpha, pi = alpha * T and e = exp(-relu(l) dist),
// which is d alpha / d (relu(l) dist) — the backward takes it from here: 1 - alpha has lost e's low bits once alpha is near 1.  zc =
// this plane's depth layer, T = the transmittance in front of it; both stay with the caller, which moves them on (T *= plade_keep(alpha),
// zc = zn) when it is done with them — the backward uses T first.  c = tail_depth_scale(W), r = the ray's length.
struct PladeStep {
  float zn, dist, alpha, p, e;
};
__device__ __forceinline__ PladeStep plade_step(bool last, float c, float dn, float rl, float r, float zc, float T) {
  PladeStep s = {zc, 0.0f, 1.0f, 0.0f, 0.0f};
  if (!last) {
    s.zn = c / dn;                                                       // plade_net.py:311
    s.dist = (s.zn - zc) * r;                                            // :312-315
    s.e = __expf(-fmaxf(rl, 0.0f) * s.dist);
    s.alpha = 1.0f - s.e;                                                // :317
  }
  s.p = s.alpha * T;                                                     // :320
  return s;
}
__device__ __forceinline__ float plade_keep(float alpha) { return (1.0f - alpha) + 1e-10f; }

// The plane's weight in disp: u = pi / sigma with the mixture (sg = the clamped sigma is an output then), pi without.  Adds it
// to the running sums and returns it.
template <bool MIX>
__device__ __forceinline__ float plade_accumulate(float p, float rs, float dv, float& Sw, float& Sd, float& sg) {
  if (MIX) {
    sg = clamp_sigma(sigmoid_f(rs));                                     // :327-328
    const float u = p / sg;                                              // :331
    Sw += u;
    Sd += u * dv;
    return u;
  }
  Sd += p * dv;
  return p;
}
// Backward: d loss / d pi_n at one pixel from gD = d loss / d disp — through u_n = pi_n / sigma_n with the mixture (d disp / d u_n =
// (d_n - disp) / S), directly without.  Both passes of plade_bwd_kernel take it from here: their sums must meet in the same values.
template <bool MIX>
__device__ __forceinline__ float plade_g_p(float gD, float dv, float dsp, float sw, float sg) {
  return MIX ? gD * (dv - dsp) / sw / sg : gD * dv;
}
// and the pixel's results once every plane is in; sw is the stash (sum of the weights, 1 without the mixture)
template <bool MIX>
__device__ __forceinline__ void plade_finish(float Sw, float Sd, float c, float& disp, float& depth, float& sw) {
  disp = MIX ? Sd / Sw : Sd;                                             // :332-333, 338
  depth = c / disp;                                                      // :340
  sw = MIX ? Sw : 1.0f;
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
