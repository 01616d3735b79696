// Fused tail of PladeNet.forward with --render_probability (reference networks/plade_net.py:309-341; the only live producer
// of outputs["dists"], which the sweep's alpha-compositing branch reads, trainer.py:584-591): everything the network does
// with the outputs of conv0 (N-1 logit channels) and conv_sigma, in ONE front-to-back pass over the planes:
//   depth_layered = 0.1 * 0.58 * W / disp_layered;  dists_n = (depth_layered_{n+1} - depth_layered_n) * |K^-1 [x, y, 1]|
//   alpha_n = 1 - exp(-relu(logit_n) * dists_n)  (n < N-1),  alpha_{N-1} = 1
//   pi_n = alpha_n * prod_{m<n} (1 - alpha_m + 1e-10);  logits = cat(raw_logits, ones)
//   sigma = clamp(sigmoid(raw_sigma), .01, 1);  probability = (pi / sigma) / sum_N(pi / sigma)   [mixture]  |  pi
//   disp = sum_N probability * disp_layered;  depth = 0.1 * 0.58 * W / disp
// The reference runs ~20 full-tensor ATen passes (two cats, a cumprod, ...).  One thread owns one pixel (four with 16-byte
// accesses where the shapes allow) and streams its planes once; pi / probability are produced on demand
// (pd_plade_tail_layers).  Backward: with p_n = alpha_n T_n, g_alpha_n = g_p_n T_n - (sum_{k>n} g_p_k p_k) / (1 - alpha_n +
// 1e-10).  The sum over the planes BEHIND n is taken front to back as total - prefix_n, and it is tiny next to both wherever the
// planes in front hold the probability (an occluded plane, an opaque one): a first pass over the conv outputs forms the total of
// the very terms the second pass adds up again, both in fp64, so that the difference keeps the relative accuracy of its own terms.
// (The closed form of the total — 0 with the mixture weights, g_disp * disp without — is right to 1e-7 of the LARGEST term only,
// as is an fp32 prefix: measured per element, g_raw_logits was 5e-3 .. 3e-2 and the per-plane g_disp_layered 6e-4 away from fp64
// where the reference's own fp32 run is 4e-5; tests/test_tail_forms.py, profiles/tail_form_parity.md.)  The distance gradient
// reaches disp_layered through the two depth layers it subtracts.
// PD_TAIL_BF16: raw_logits / raw_sigma, logits / sigma and their gradients hold bf16 (storage type ST = Bf16; the rule of
// pd_decoder_tail.hip: exact widening, the fp32 arithmetic in the same order, one rounding per bf16 output element); dists and
// its gradient, the disparities and the per-pixel maps stay fp32.
#include "pd_plade_tail.h"

namespace pd {

template <class ST, bool MIX, int PX>
__global__ __launch_bounds__(kBlock) void plade_fwd_kernel(PladeArgs a, float* __restrict__ logits, float* __restrict__ dists,
                                                           float* __restrict__ sigma, float* __restrict__ disp,
                                                           float* __restrict__ depth, float* __restrict__ stash) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const int N = a.N;
  const float c = tail_depth_scale(a.W);
  const Px<PX> r = ldv<PX>(a.ray + pix);
  float T[PX], Sw[PX], Sd[PX], zc[PX];
  Px<PX> dv = plade_disp<PX>(a, b, 0, pix);
#pragma unroll
  for (int j = 0; j < PX; ++j) { T[j] = 1.0f; Sw[j] = Sd[j] = 0.0f; zc[j] = c / dv.v[j]; }
  for (int n = 0; n < N; ++n) {
    const bool last = (n == N - 1);
    // (the operands are loaded here, not through plade_operands: with the shared loader the one-pixel bf16 mixture kernel took
    // one more register)
    PladeOperands<PX> q;
    q.dn = last ? dv : plade_disp<PX>(a, b, n + 1, pix);       // disparity of the NEXT plane
    q.rl = last ? splat<PX>(0.0f) : ldv<PX>(elems<ST>(a.raw_logits) + ((long)b * (N - 1) + n) * a.HW + pix);
    q.rs = MIX ? ldv<PX>(elems<ST>(a.raw_sigma) + ((long)b * N + n) * a.HW + pix) : splat<PX>(0.0f);
    Px<PX> o_l, o_t, o_s;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const PladeStep s = plade_step(last, c, q.dn.v[j], q.rl.v[j], r.v[j], zc[j], T[j]);
      o_l.v[j] = last ? 1.0f : q.rl.v[j];                                  // :322 the appended ones channel
      o_t.v[j] = s.dist;
      T[j] *= plade_keep(s.alpha);
      plade_accumulate<MIX>(s.p, q.rs.v[j], dv.v[j], Sw[j], Sd[j], o_s.v[j]);
      zc[j] = s.zn;
    }
    stv<PX>(elems<ST>(logits) + ((long)b * N + n) * a.HW + pix, o_l);
    if (!last) stv<PX>(dists + ((long)b * (N - 1) + n) * a.HW + pix, o_t);
    if (MIX) stv<PX>(elems<ST>(sigma) + ((long)b * N + n) * a.HW + pix, o_s);
    dv = q.dn;
  }
  Px<PX> o_disp, o_depth, o_sw;
#pragma unroll
  for (int j = 0; j < PX; ++j) plade_finish<MIX>(Sw[j], Sd[j], c, o_disp.v[j], o_depth.v[j], o_sw.v[j]);
  stv<PX>(disp + (long)b * a.HW + pix, o_disp);
  stv<PX>(depth + (long)b * a.HW + pix, o_depth);
  stv<PX>(stash + (long)b * a.HW + pix, o_sw);
}

// pi and probability (plade_net.py:320, 330-333) for callers that want the tensors
template <class ST, bool MIX, int PX>
__global__ __launch_bounds__(kBlock) void plade_layers_kernel(PladeArgs a, const float* __restrict__ stash, float* __restrict__ pi,
                                                              float* __restrict__ prob) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const int N = a.N;
  const float c = tail_depth_scale(a.W);
  const Px<PX> r = ldv<PX>(a.ray + pix), sw = ldv<PX>(stash + (long)b * a.HW + pix);
  float T[PX], zc[PX];
  Px<PX> dv = plade_disp<PX>(a, b, 0, pix);
#pragma unroll
  for (int j = 0; j < PX; ++j) { T[j] = 1.0f; zc[j] = c / dv.v[j]; }
  for (int n = 0; n < N; ++n) {
    PladeOperands<PX> q;
    plade_operands<ST, MIX, PX>(a, b, n, pix, dv, q);
    Px<PX> op, oq;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const PladeStep s = plade_step(n == N - 1, c, q.dn.v[j], q.rl.v[j], r.v[j], zc[j], T[j]);
      T[j] *= plade_keep(s.alpha);
      op.v[j] = s.p;
      oq.v[j] = MIX ? s.p / clamp_sigma(sigmoid_f(q.rs.v[j])) / sw.v[j] : s.p;
      zc[j] = s.zn;
    }
    if (pi) stv<PX>(pi + ((long)b * N + n) * a.HW + pix, op);
    if (prob) stv<PX>(prob + ((long)b * N + n) * a.HW + pix, oq);
    dv = q.dn;
  }
}

template <class ST, bool MIX, int PX>
__global__ __launch_bounds__(kBlock) void plade_bwd_kernel(PladeArgs a, const float* __restrict__ stash, const float* __restrict__ disp,
                                                           const float* __restrict__ g_logits, const float* __restrict__ g_dists,
                                                           const float* __restrict__ g_sigma, const float* __restrict__ g_disp,
                                                           const float* __restrict__ g_depth, float* __restrict__ g_raw_logits,
                                                           float* __restrict__ g_raw_sigma, float* __restrict__ g_dl,
                                                           float* __restrict__ partials) {
  extern __shared__ float red[];  // [N] block sums of the per-plane disparity gradient
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  const int N = a.N;
  const bool reduce = (g_dl != nullptr) && !a.dense;
  if (reduce) block_partials_zero(red, N);
  const bool active = pix < a.HW;
  const long px0 = active ? pix : 0;
  const float c = tail_depth_scale(a.W);
  Px<PX> r = splat<PX>(0.0f), sw = splat<PX>(1.0f), dsp = splat<PX>(1.0f), gD = splat<PX>(0.0f);
  if (active) {
    r = ldv<PX>(a.ray + pix);
    sw = ldv<PX>(stash + (long)b * a.HW + pix);
    dsp = ldv<PX>(disp + (long)b * a.HW + pix);
    gD = tail_upstream<PX>(g_disp, g_depth, (long)b * a.HW + pix, dsp, c);
  }
  float T[PX], zc[PX], gprev[PX];
  double total[PX], prefix[PX];   // sum_k g_p_k p_k over all planes / over the planes up to n: products and sums in fp64
  Px<PX> dv = plade_disp<PX>(a, b, 0, px0);
#pragma unroll
  for (int j = 0; j < PX; ++j) { T[j] = 1.0f; zc[j] = c / dv.v[j]; total[j] = 0.0; }
  if (active) {   // first pass: the total, from the values the second pass forms again (plade_step, plade_g_p)
    for (int n = 0; n < N; ++n) {
      PladeOperands<PX> q;
      plade_operands<ST, MIX, PX>(a, b, n, px0, dv, q);
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const PladeStep s = plade_step(n == N - 1, c, q.dn.v[j], q.rl.v[j], r.v[j], zc[j], T[j]);
        const float sg = MIX ? clamp_sigma(sigmoid_f(q.rs.v[j])) : 1.0f;
        total[j] += (double)plade_g_p<MIX>(gD.v[j], dv.v[j], dsp.v[j], sw.v[j], sg) * (double)s.p;
        T[j] *= plade_keep(s.alpha);
        zc[j] = s.zn;
      }
      dv = q.dn;
    }
    dv = plade_disp<PX>(a, b, 0, px0);
  }
#pragma unroll
  for (int j = 0; j < PX; ++j) { T[j] = 1.0f; zc[j] = c / dv.v[j]; prefix[j] = 0.0; gprev[j] = 0.0f; }
  for (int n = 0; n < N; ++n) {
    const bool last = (n == N - 1);
    float gd_sum = 0.0f;
    if (active) {
      PladeOperands<PX> q;
    plade_operands<ST, MIX, PX>(a, b, n, px0, dv, q);
      const Px<PX> gl = (g_logits && !last) ? ldv<PX>(elems<ST>(g_logits) + ((long)b * N + n) * a.HW + pix) : splat<PX>(0.0f);
      const Px<PX> gt = (g_dists && !last) ? ldv<PX>(g_dists + ((long)b * (N - 1) + n) * a.HW + pix) : splat<PX>(0.0f);
      const Px<PX> gs = (MIX && g_sigma) ? ldv<PX>(elems<ST>(g_sigma) + ((long)b * N + n) * a.HW + pix) : splat<PX>(0.0f);
      Px<PX> o_l, o_s, o_d;
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const PladeStep s = plade_step(last, c, q.dn.v[j], q.rl.v[j], r.v[j], zc[j], T[j]);
        const float alpha = s.alpha, dist = s.dist, p = s.p, rl = q.rl.v[j];
        float sg = 1.0f, gd_direct;
        if (MIX) {
          const float sgu = sigmoid_f(q.rs.v[j]);
          sg = clamp_sigma(sgu);
          const float u = p / sg;
          const float g_u = gD.v[j] * (dv.v[j] - dsp.v[j]) / sw.v[j];      // d disp / d u_n = (d_n - disp) / S
          const float gsig = gs.v[j] - g_u * u / sg;                       // d u / d sigma = -u / sigma
          o_s.v[j] = (sgu == sg) ? gsig * sgu * (1.0f - sgu) : 0.0f;       // clamp gate (inclusive bounds), sigmoid'
          gd_direct = gD.v[j] * u / sw.v[j];                               // d disp / d d_n = probability_n
        } else {
          gd_direct = gD.v[j] * p;
        }
        const float g_p = plade_g_p<MIX>(gD.v[j], dv.v[j], dsp.v[j], sw.v[j], sg);
        prefix[j] += (double)g_p * (double)p;
        const float keep = plade_keep(alpha);
        float g_dist = 0.0f;
        if (!last) {
          const float g_alpha = g_p * T[j] - (float)(total[j] - prefix[j]) / keep;   // (the planes behind n)
          const float da = s.e;                                            // exp(-relu(l) dist) = d alpha / d (relu(l) dist)
          o_l.v[j] = gl.v[j] + ((rl > 0.0f) ? g_alpha * dist * da : 0.0f);
          g_dist = gt.v[j] + g_alpha * fmaxf(rl, 0.0f) * da;
        }
        // depth layer n is the far end of distance n-1 and the near end of distance n
        const float g_z = r.v[j] * (gprev[j] - g_dist);
        o_d.v[j] = gd_direct - g_z * c / (dv.v[j] * dv.v[j]);              // depth_layered = c / disp_layered
        gd_sum += o_d.v[j];
        T[j] *= keep;
        gprev[j] = g_dist;
        zc[j] = s.zn;
      }
      if (g_raw_logits && !last) stv<PX>(elems<ST>(g_raw_logits) + ((long)b * (N - 1) + n) * a.HW + pix, o_l);
      if (MIX && g_raw_sigma) stv<PX>(elems<ST>(g_raw_sigma) + ((long)b * N + n) * a.HW + pix, o_s);
      if (g_dl && a.dense) stv<PX>(g_dl + ((long)b * N + n) * a.HW + pix, o_d);
      dv = q.dn;
    }
    if (reduce) block_partials_add(red, n, gd_sum);
  }
  if (reduce) block_partials_store(red, partials, b, N);
}

}  // namespace pd

using namespace pd;

extern "C" int pd_plade_tail_fwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                                 const float* disp_layered, const float* ray_norm, float* logits, float* dists, float* sigma,
                                 float* disp, float* depth, float* stash, pd_stream_t stream) {
  if (int rc = plade_validate(B, N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm)) return rc;
  PD_REQUIRE(logits && dists && disp && depth && stash, "NULL output");
  PD_REQUIRE(!(flags & PD_TAIL_MIXTURE) || sigma, "mixture needs the sigma output");
  const PladeArgs a = plade_args(N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm);
  const TailLaunch t = tail_launch(B, H, W, flags, 0, {a.dense ? disp_layered : nullptr, ray_norm, dists, disp, depth, stash},
                                   {raw_logits, raw_sigma, logits, sigma});
  PD_PLADE_DISPATCH(plade_fwd_kernel, t.bf16, t.px, a.mix, t.grid, 0, (hipStream_t)stream, a, logits, dists, sigma, disp, depth, stash);
  return check_launch("plade_fwd_kernel");
}

extern "C" int pd_plade_tail_layers(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                                    const float* disp_layered, const float* ray_norm, const float* stash, float* pi,
                                    float* probability, pd_stream_t stream) {
  if (int rc = plade_validate(B, N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm)) return rc;
  PD_REQUIRE(stash && (pi || probability), "NULL pointer");
  const PladeArgs a = plade_args(N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm);
  const TailLaunch t = tail_launch(B, H, W, flags, 0, {a.dense ? disp_layered : nullptr, ray_norm, stash, pi, probability},
                                   {raw_logits, raw_sigma});
  PD_PLADE_DISPATCH(plade_layers_kernel, t.bf16, t.px, a.mix, t.grid, 0, (hipStream_t)stream, a, stash, pi, probability);
  return check_launch("plade_layers_kernel");
}

extern "C" int pd_plade_tail_bwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                                 const float* disp_layered, const float* ray_norm, const float* stash, const float* disp,
                                 const float* g_logits, const float* g_dists, const float* g_sigma, const float* g_disp,
                                 const float* g_depth, float* g_raw_logits, float* g_raw_sigma, float* g_disp_layered,
                                 float* workspace, pd_stream_t stream) {
  if (int rc = plade_validate(B, N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm)) return rc;
  PD_REQUIRE(stash && disp, "NULL pointer");
  PD_REQUIRE(g_raw_logits || g_raw_sigma || g_disp_layered, "no gradient requested");
  const PladeArgs a = plade_args(N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm);
  const bool reduce = g_disp_layered && !a.dense;
  PD_REQUIRE(!reduce || workspace, "per-plane disparity gradient needs the workspace (pd_decoder_tail_bwd_workspace_floats)");
  PD_REQUIRE((size_t)N * sizeof(float) <= 64 * 1024, "too many planes");
  const TailLaunch t = tail_launch(B, H, W, flags, 0, {a.dense ? disp_layered : nullptr, ray_norm, stash, disp, g_dists, g_disp,
                                                       g_depth, a.dense ? g_disp_layered : nullptr},
                                   {raw_logits, raw_sigma, g_logits, g_sigma, g_raw_logits, g_raw_sigma});
  const size_t shmem = reduce ? (size_t)N * sizeof(float) : 0;
  PD_PLADE_DISPATCH(plade_bwd_kernel, t.bf16, t.px, a.mix, t.grid, shmem, (hipStream_t)stream, a, stash, disp, g_logits, g_dists,
                    g_sigma, g_disp, g_depth, g_raw_logits, g_raw_sigma, g_disp_layered, workspace);
  if (int rc = check_launch("plade_bwd_kernel")) return rc;
  return reduce ? reduce_partials(workspace, g_disp_layered, (int)t.grid.x, N, B, (hipStream_t)stream) : 0;
}
