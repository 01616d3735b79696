// Inference tails: what a depth network's user needs from the decoder's conv outputs once training is over — disp, depth, the
// confidence max_n probability_n (evaluate_depth_HR.py:144-168 reads disp and probability.amax(1) only) — in ONE forward-only
// pass over the planes that writes nothing [B,N,H,W]-sized.  The training forwards (pd_decoder_tail_fwd, pd_plade_tail_fwd)
// write sigma (+ logits with a mask; logits, dists and sigma for PladeNet) for the sweep and the losses to read; none of that is
// read at inference.  Algorithmic floats per pixel, mixture, fp32, no mask: 2N reads + up to 7 writes here against 2N + N + 4.
//   disp / depth / stash   the training forward's bits: the same expressions in the same order on the same loads, so
//                          pd_*_tail_layers still serves pi / probability from the stash on demand
//   confidence             max_n probability_n (depth_decoder.py:282-285 with the mixture, pi without; plade_net.py:330-333)
//   plane_index            the plane that attains it, the lowest index among equal maxima (candidates_idx, depth_decoder.py:286)
//   disp_best              disp_layered at that plane (the commented alternative of :287)
// Decoder tail: the forward's online softmax carries one more running value, the best weight w = e^(l-m) * mask / sigma seen so
// far, in the units of the current reference m; it is rescaled with Z / Sw / Sd whenever m moves, a later plane replaces it only
// when strictly greater, and confidence = w_best / Sw (the softmax normaliser cancels as it does in disp).  A masked plane has
// l = 0 and w = 0: it takes part in the softmax (the reference's quirk) and can be the best plane only where every weight is 0.
// PladeNet tail: the weights u = pi / sigma (pi without the mixture) need no reference, so the best one is a plain running
// maximum and confidence = u_best / Sw is the division pd_plade_tail_layers does for that plane.
// PD_TAIL_BF16: raw_logits / raw_sigma hold bf16 and widen exactly on load; every output is fp32 (or int32).  No bf16 is
// stored, so the plane loop unrolls for both storage types (unrolling does not reorder a pixel's arithmetic).
#include "pd_decoder_tail.h"
#include "pd_plade_tail.h"

namespace pd {

struct InferOut {   // every pointer but disp may be NULL (that output is skipped)
  float* disp;
  float* depth;
  float* confidence;
  int* plane_index;
  float* disp_best;
  float* stash;
};

template <int PX>
__device__ __forceinline__ void stv_idx(int* __restrict__ p, const int (&r)[PX]) {
  if (PX == 4) *reinterpret_cast<int4*>(p) = make_int4(r[0], r[1 % PX], r[2 % PX], r[3 % PX]);
  else p[0] = r[0];
}

template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__global__ __launch_bounds__(kBlock) void tail_infer_kernel(TailArgs a, InferOut o) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const long base = (long)b * a.N * a.HW + pix;
  const int H = RF ? a.HW / a.W : 0, y = RF ? pix / a.W : 0;   // row form: the lane's row (W % PX == 0 there)
  const long rbase = (long)b * a.N * H;
  float m[PX], Z[PX], Sw[PX], Sd[PX];   // tail_fwd_kernel's running reference, sum e^(l-m), sum of weights, sum w*d
  float wb[PX];                         // the best weight so far, relative to m
  int nb[PX];                           // and its plane
#pragma unroll
  for (int j = 0; j < PX; ++j) { m[j] = -INFINITY; Z[j] = Sw[j] = Sd[j] = 0.0f; wb[j] = 0.0f; nb[j] = 0; }
#pragma unroll 2
  for (int n = 0; n < a.N; ++n) {
    const long i = base + (long)n * a.HW;
    const Px<PX> mk = !HASMASK ? splat<PX>(1.0f) : (RF & kRowMask) ? ld_row<PX>(a.mask + rbase, n, H, y) : ldv<PX>(a.mask + i);
    const Px<PX> rl = ldv<PX>(elems<ST>(a.raw_logits) + i);
    const Px<PX> rs = MIX ? ldv<PX>(elems<ST>(a.raw_sigma) + i) : splat<PX>(0.0f);
    const Px<PX> dv = (RF & kRowDisp) ? ld_row<PX>(a.dl + rbase, n, H, y)
                                      : a.dense ? ldv<PX>(a.dl + i) : splat<PX>(a.dl[b * a.N + n]);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float l = rl.v[j] * mk.v[j];                           // depth_decoder.py:259
      float inv = 1.0f;
      if (MIX) {
        const float sg = clamp_sigma(sigmoid_f(rs.v[j]));          // :278-279
        inv = mk.v[j] / sg;                                        // :282-283 (mask applied to the weights)
      }
      if (l > m[j]) {  // move the reference to the new maximum
        const float sc = __expf(m[j] - l);
        Z[j] *= sc; Sw[j] *= sc; Sd[j] *= sc;
        wb[j] *= sc;
        m[j] = l;
      }
      const float e = __expf(l - m[j]);
      const float w = e * inv;
      Z[j] += e;
      Sw[j] += w;
      Sd[j] += w * dv.v[j];
      if (n == 0 || w > wb[j]) {  // strict: the lower index keeps a tie (plane 0 stands where every weight is 0)
        wb[j] = w; nb[j] = n;
      }
    }
  }
  Px<PX> o_disp, o_depth, o_lse, o_sn, o_conf;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const float dsp = Sd[j] / Sw[j];                                // :284-285, 289 (the softmax normaliser cancels)
    o_disp.v[j] = dsp;
    o_depth.v[j] = 0.1f * 0.58f * (float)a.W / dsp;                 // :291
    o_lse.v[j] = m[j] + __logf(Z[j]);                               // log-sum-exp of the masked logits
    o_sn.v[j] = Sw[j] / Z[j];                                       // sum_N pi * mask / sigma
    o_conf.v[j] = wb[j] / Sw[j];                                    // max_n probability_n
  }
  const long p1 = (long)b * a.HW + pix;
  stv<PX>(o.disp + p1, o_disp);
  if (o.depth) stv<PX>(o.depth + p1, o_depth);
  if (o.confidence) stv<PX>(o.confidence + p1, o_conf);
  if (o.plane_index) stv_idx<PX>(o.plane_index + p1, nb);
  if (o.disp_best) {   // disp_layered at the best plane, read again (one element per pixel) instead of carried through the loop
    Px<PX> o_best;
#pragma unroll
    for (int j = 0; j < PX; ++j)
      o_best.v[j] = (RF & kRowDisp) ? a.dl[rbase + (long)nb[j] * H + y]
                                    : a.dense ? a.dl[base + (long)nb[j] * a.HW + j] : a.dl[b * a.N + nb[j]];
    stv<PX>(o.disp_best + p1, o_best);
  }
  if (o.stash) {
    stv<PX>(o.stash + ((long)b * 2 + 0) * a.HW + pix, o_lse);
    stv<PX>(o.stash + ((long)b * 2 + 1) * a.HW + pix, o_sn);
  }
}

template <class ST, bool MIX, int PX>
__global__ __launch_bounds__(kBlock) void plade_infer_kernel(PladeArgs a, InferOut o) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const int N = a.N;
  const float c = 0.1f * 0.58f * (float)a.W;
  const Px<PX> r = ldv<PX>(a.ray + pix);
  float T[PX], Sw[PX], Sd[PX], zc[PX];
  float ub[PX];                         // the best weight so far (pi / sigma, or pi)
  int nb[PX];                           // and its plane
  Px<PX> dv = plade_disp<PX>(a, b, 0, pix);
#pragma unroll
  for (int j = 0; j < PX; ++j) { T[j] = 1.0f; Sw[j] = Sd[j] = 0.0f; zc[j] = c / dv.v[j]; ub[j] = 0.0f; nb[j] = 0; }
  for (int n = 0; n < N; ++n) {
    const bool last = (n == N - 1);
    const Px<PX> dn = last ? dv : plade_disp<PX>(a, b, n + 1, pix);       // disparity of the NEXT plane
    const Px<PX> rl = last ? splat<PX>(0.0f) : ldv<PX>(elems<ST>(a.raw_logits) + ((long)b * (N - 1) + n) * a.HW + pix);
    const Px<PX> rs = MIX ? ldv<PX>(elems<ST>(a.raw_sigma) + ((long)b * N + n) * a.HW + pix) : splat<PX>(0.0f);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      float alpha = 1.0f, zn = zc[j];
      if (!last) {
        zn = c / dn.v[j];                                                  // plade_net.py:311
        const float dist = (zn - zc[j]) * r.v[j];                          // :312-315
        alpha = 1.0f - __expf(-fmaxf(rl.v[j], 0.0f) * dist);               // :317
      }
      const float p = alpha * T[j];                                        // :320
      T[j] *= (1.0f - alpha) + 1e-10f;
      float u = p;
      if (MIX) {
        const float sg = clamp_sigma(sigmoid_f(rs.v[j]));                  // :327-328
        u = p / sg;                                                        // :331
        Sw[j] += u;
        Sd[j] += u * dv.v[j];
      } else {
        Sd[j] += p * dv.v[j];
      }
      if (n == 0 || u > ub[j]) {  // strict: the lower index keeps a tie
        ub[j] = u; nb[j] = n;
      }
      zc[j] = zn;
    }
    dv = dn;
  }
  Px<PX> o_disp, o_depth, o_sw, o_conf;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const float dsp = MIX ? Sd[j] / Sw[j] : Sd[j];                         // :332-333, 338
    o_disp.v[j] = dsp;
    o_depth.v[j] = c / dsp;                                                // :340
    o_sw.v[j] = MIX ? Sw[j] : 1.0f;
    o_conf.v[j] = MIX ? ub[j] / Sw[j] : ub[j];                             // max_n probability_n
  }
  const long p1 = (long)b * a.HW + pix;
  stv<PX>(o.disp + p1, o_disp);
  if (o.depth) stv<PX>(o.depth + p1, o_depth);
  if (o.confidence) stv<PX>(o.confidence + p1, o_conf);
  if (o.plane_index) stv_idx<PX>(o.plane_index + p1, nb);
  if (o.disp_best) {   // disp_layered at the best plane, read again (one element per pixel)
    Px<PX> o_best;
#pragma unroll
    for (int j = 0; j < PX; ++j)
      o_best.v[j] = a.dense ? a.dl[((long)b * N + nb[j]) * a.HW + pix + j] : a.dl[b * N + nb[j]];
    stv<PX>(o.disp_best + p1, o_best);
  }
  if (o.stash) stv<PX>(o.stash + p1, o_sw);
}

}  // namespace pd

using namespace pd;

extern "C" int pd_decoder_tail_infer(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                                     const float* padding_mask, const float* disp_layered, float* disp, float* depth,
                                     float* confidence, int* plane_index, float* disp_best, float* stash, pd_stream_t stream) {
  if (int rc = tail_validate(B, N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered)) return rc;
  PD_REQUIRE(disp, "NULL output (disp is required; depth, confidence, plane_index, disp_best and stash may be NULL)");
  const TailArgs a = tail_args(N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered);
  const InferOut o = {disp, depth, confidence, plane_index, disp_best, stash};
  const bool bf16 = (flags & PD_TAIL_BF16) != 0;
  const int rf = tail_rf(flags, padding_mask);
  const int px = tail_px_rows(tail_px(H, W, {(rf & kRowMask) ? nullptr : padding_mask, a.dense ? disp_layered : nullptr, disp,
                                             depth, confidence, plane_index, disp_best, stash},
                                      {raw_logits, raw_sigma}, bf16), rf, W);
  dim3 grid(ceil_div(ceil_div(H * W, px), kBlock), B);
  const bool hasmask = padding_mask != nullptr;
#define PD_TAIL_INFER(RF) \
  PD_TAIL_DISPATCH(tail_infer_kernel, RF, bf16, px, a.mix, hasmask, grid, kBlock, 0, (hipStream_t)stream, a, o)
  switch (rf) {
    case 0: PD_TAIL_INFER(0); break;
    case kRowDisp: PD_TAIL_INFER(kRowDisp); break;
    case kRowMask: PD_TAIL_INFER(kRowMask); break;
    default: PD_TAIL_INFER(kRowDisp | kRowMask); break;
  }
#undef PD_TAIL_INFER
  return check_launch("tail_infer_kernel");
}

extern "C" int pd_plade_tail_infer(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                                   const float* disp_layered, const float* ray_norm, float* disp, float* depth,
                                   float* confidence, int* plane_index, float* disp_best, float* stash, pd_stream_t stream) {
  PD_REQUIRE(!(flags & (PD_TAIL_DISP_ROWS | PD_TAIL_MASK_ROWS)),
             "flags: PD_TAIL_DISP_ROWS / PD_TAIL_MASK_ROWS are the decoder tail's (the PladeNet tail has no row form)");
  if (int rc = plade_validate(B, N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm)) return rc;
  PD_REQUIRE(disp, "NULL output (disp is required; depth, confidence, plane_index, disp_best and stash may be NULL)");
  const PladeArgs a = plade_args(N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm);
  const InferOut o = {disp, depth, confidence, plane_index, disp_best, stash};
  const bool bf16 = (flags & PD_TAIL_BF16) != 0;
  const int px = tail_px(H, W, {a.dense ? disp_layered : nullptr, ray_norm, disp, depth, confidence, plane_index, disp_best, stash},
                         {raw_logits, raw_sigma}, bf16);
  dim3 grid(ceil_div(ceil_div(H * W, px), kBlock), B);
  PD_PLADE_DISPATCH(plade_infer_kernel, bf16, px, a.mix, grid, 0, (hipStream_t)stream, a, o);
  return check_launch("plade_infer_kernel");
}
