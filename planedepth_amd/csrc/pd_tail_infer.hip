// Inference tails: what a depth network's user needs from the decoder's conv outputs once training is over — disp, depth, the
// confidence max_n probability_n (evaluate_depth_HR.py:144-168 reads disp and probability.amax(1) only) — in ONE forward-only
// pass over the planes that writes nothing [B,N,H,W]-sized.  The training forwards (pd_decoder_tail_fwd, pd_plade_tail_fwd)
// write sigma (+ logits with a mask; logits, dists and sigma for PladeNet) for the sweep and the losses to read; none of that is
// read at inference.  Algorithmic floats per pixel, mixture, fp32, no mask: 2N reads + up to 7 writes here against 2N + N + 4.
//   disp / depth / stash   the training forward's bits by construction: both kernels load a plane's operands with the same
//                          loader and call the same per-plane step and per-pixel finish (pd_decoder_tail.h: tail_operands,
//                          tail_softmax_step, tail_softmax_finish; pd_plade_tail.h: plade_operands, plade_step, plade_accumulate,
//                          plade_finish), so pd_*_tail_layers still serves pi / probability from the stash on demand
//   confidence             max_n probability_n (depth_decoder.py:282-285 with the mixture, pi without; plade_net.py:330-333)
//   plane_index            the plane that attains it, the lowest index among equal maxima (candidates_idx, depth_decoder.py:286)
//   disp_best              disp_layered at that plane (the commented alternative of :287)
// Decoder tail: the forward's online softmax carries one more running value, the best weight w = e^(l-m) * mask / sigma seen so
// far, in the units of the current reference m; it is rescaled with Z / Sw / Sd whenever m moves (tail_softmax_step<MIX, true>), a
// later plane replaces it only when strictly greater (keep_best), and confidence = w_best / Sw (the softmax normaliser cancels as it does in disp).  A masked plane has
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

template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__global__ __launch_bounds__(kBlock) void tail_infer_kernel(TailArgs a, InferOut o) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const TailLane ln = tail_lane<RF>(a, b, pix);
  float m[PX], Z[PX], Sw[PX], Sd[PX];   // tail_fwd_kernel's running reference, sum e^(l-m), sum of weights, sum w*d
  float wb[PX];                         // the best weight so far, relative to m
  int nb[PX];                           // and its plane
#pragma unroll
  for (int j = 0; j < PX; ++j) { m[j] = -INFINITY; Z[j] = Sw[j] = Sd[j] = 0.0f; wb[j] = 0.0f; nb[j] = 0; }
#pragma unroll 2
  for (int n = 0; n < a.N; ++n) {
    TailOperands<PX> q;
    tail_operands<ST, MIX, HASMASK, PX, RF>(a, ln, n, ln.base + (long)n * a.HW, q);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      float l, sg, w;   // (logits and sigma are not written here)
      tail_softmax_step<MIX, true>(q.rl.v[j], q.rs.v[j], q.mk.v[j], q.dv.v[j], m[j], Z[j], Sw[j], Sd[j], wb[j], l, sg, w);
      keep_best(n, w, wb[j], nb[j]);
    }
  }
  Px<PX> o_disp, o_depth, o_lse, o_sn, o_conf;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    tail_softmax_finish(m[j], Z[j], Sw[j], Sd[j], tail_depth_scale(a.W), o_disp.v[j], o_depth.v[j], o_lse.v[j], o_sn.v[j]);
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
      o_best.v[j] = (RF & kRowDisp) ? a.dl[ln.rbase + (long)nb[j] * ln.H + ln.y]
                                    : a.dense ? a.dl[ln.base + (long)nb[j] * a.HW + j] : a.dl[b * a.N + nb[j]];
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
  const float c = tail_depth_scale(a.W);
  const Px<PX> r = ldv<PX>(a.ray + pix);
  float T[PX], Sw[PX], Sd[PX], zc[PX];
  float ub[PX];                         // the best weight so far (pi / sigma, or pi)
  int nb[PX];                           // and its plane
  Px<PX> dv = plade_disp<PX>(a, b, 0, pix);
#pragma unroll
  for (int j = 0; j < PX; ++j) { T[j] = 1.0f; Sw[j] = Sd[j] = 0.0f; zc[j] = c / dv.v[j]; ub[j] = 0.0f; nb[j] = 0; }
  for (int n = 0; n < N; ++n) {
    PladeOperands<PX> q;
    plade_operands<ST, MIX, PX>(a, b, n, pix, dv, q);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const PladeStep s = plade_step(n == N - 1, c, q.dn.v[j], q.rl.v[j], r.v[j], zc[j], T[j]);
      T[j] *= plade_keep(s.alpha);
      float sg;   // (sigma is not written here)
      const float u = plade_accumulate<MIX>(s.p, q.rs.v[j], dv.v[j], Sw[j], Sd[j], sg);
      keep_best(n, u, ub[j], nb[j]);
      zc[j] = s.zn;
    }
    dv = q.dn;
  }
  Px<PX> o_disp, o_depth, o_sw, o_conf;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    plade_finish<MIX>(Sw[j], Sd[j], c, o_disp.v[j], o_depth.v[j], o_sw.v[j]);
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
  const int rf = tail_rf(flags, padding_mask);
  const TailLaunch t = tail_launch(B, H, W, flags, rf, {(rf & kRowMask) ? nullptr : padding_mask, a.dense ? disp_layered : nullptr,
                                                        disp, depth, confidence, plane_index, disp_best, stash},
                                   {raw_logits, raw_sigma});
  PD_TAIL_DISPATCH_RF(tail_infer_kernel, rf, t.bf16, t.px, a.mix, padding_mask != nullptr, t.grid, kBlock, 0, (hipStream_t)stream, a, o);
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
  const TailLaunch t = tail_launch(B, H, W, flags, 0, {a.dense ? disp_layered : nullptr, ray_norm, disp, depth, confidence,
                                                       plane_index, disp_best, stash}, {raw_logits, raw_sigma});
  PD_PLADE_DISPATCH(plade_infer_kernel, t.bf16, t.px, a.mix, t.grid, 0, (hipStream_t)stream, a, o);
  return check_launch("plade_infer_kernel");
}
