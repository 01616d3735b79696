// Fused tail of DepthDecoder.forward (reference networks/depth_decoder.py:256-260, 274-291, softmax branch; SURVEY.md
// §8f rank 1): everything the decoder does with the outputs of dispconv / sigmaconv, in ONE pass over the planes:
//   logits = raw_logits * padding_mask;  pi = softmax_N(logits);  sigma = clamp(sigmoid(raw_sigma), .01, 1)
//   probability = (pi / sigma * mask) / sum_N(...)   [mixture]   |   probability = pi   [no mixture]
//   disp = sum_N probability * disp_layered;  depth = 0.1 * 0.58 * W / disp
// The reference runs ~12 full-tensor ATen passes for this.  Here one thread owns one pixel and streams its N planes
// once: the softmax normaliser cancels in `probability`, so disp is a ratio of two running sums and neither pi nor
// probability has to exist in memory.  Training consumes logits, sigma, disp and depth only (SURVEY.md §8b B1:
// outputs["probability"] is read for its shape); pi / probability are produced on demand by pd_decoder_tail_layers
// from the per-pixel stash {log-sum-exp, sum(pi*mask/sigma)}.
// Algorithmic bytes per pixel: forward reads 2N (+N mask) floats, writes N (sigma) (+N logits when there is a mask)
// + 4; backward reads 4N (+N) and writes 2N.  HBM-bound streaming, no reuse.
// PD_TAIL_BF16 (torch.autocast: the conv outputs are bf16): raw_logits / raw_sigma, logits / sigma and the four [B,N,H,W]
// gradients hold bf16, which halves those terms.  The kernels are the same templates with the storage type ST = Bf16: every
// element widens exactly on load, the arithmetic is the fp32 kernel's in the same order, and each bf16 output element is
// rounded once from its fp32 value.  disp / depth / stash (and pi / probability) come from the UNROUNDED fp32 sigma; the
// backward recomputes the sigmoid from raw_sigma, so its clamp gate is decided in fp32 as well.
// Row form (PD_TAIL_DISP_ROWS / PD_TAIL_MASK_ROWS; template parameter RF = kRowDisp | kRowMask): xy and xz planes have a
// disparity and a padding mask that are constant along x (depth_decoder.py:153-181), so disp_layered / padding_mask come as
// [B,N,H] — one scalar load per plane and row instead of a [B,N,H,W] stream.  Per pixel the arithmetic is the dense kernels' on
// the expanded values (same expressions, same order).  4 pixels per lane are taken for a row form only when W % 4 == 0: a
// group of 4 then never straddles two rows (H*W % 4 == 0 alone does not give that: H = 2, W = 6) and one row value serves
// the lane; any other width runs one pixel per lane.  The row gradient g_disp_layered [B,N,H] is reduced by the workgroup that
// OWNS the row (tail_bwd_rows_kernel: one workgroup per (row, image), per-wave sums in LDS slots of their own, added in wave
// order): no atomics, no workspace, the same bits on every run.
#include "pd_decoder_tail.h"

namespace pd {

template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__global__ __launch_bounds__(kBlock) void tail_fwd_kernel(TailArgs a, float* __restrict__ logits, float* __restrict__ sigma,
                                                          float* __restrict__ disp, float* __restrict__ depth,
                                                          float* __restrict__ stash) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const TailLane ln = tail_lane<RF>(a, b, pix);
  float m[PX], Z[PX], Sw[PX], Sd[PX];  // running reference, sum e^(l-m), sum of weights, sum w*d
#pragma unroll
  for (int j = 0; j < PX; ++j) { m[j] = -INFINITY; Z[j] = Sw[j] = Sd[j] = 0.0f; }
  // (bf16: not unrolled.  The store's pack_bf16x2 is inline assembly, which the compiler treats as convergent and will not
  // duplicate into an unrolled body with a run-time remainder.)
  constexpr int kUnroll = sizeof(ST) == sizeof(float) ? 2 : 1;
#pragma unroll kUnroll
  for (int n = 0; n < a.N; ++n) {
    const long i = ln.base + (long)n * a.HW;
    TailOperands<PX> q;
    tail_operands<ST, MIX, HASMASK, PX, RF>(a, ln, n, i, q);
    Px<PX> lo, so;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      float none, w;   // (no best weight here)
      tail_softmax_step<MIX, false>(q.rl.v[j], q.rs.v[j], q.mk.v[j], q.dv.v[j], m[j], Z[j], Sw[j], Sd[j], none, lo.v[j], so.v[j], w);
    }
    if (HASMASK) stv<PX>(elems<ST>(logits) + i, lo);
    if (MIX) stv<PX>(elems<ST>(sigma) + i, so);
  }
  Px<PX> o_disp, o_depth, o_lse, o_sn;
#pragma unroll
  for (int j = 0; j < PX; ++j)
    tail_softmax_finish(m[j], Z[j], Sw[j], Sd[j], tail_depth_scale(a.W), o_disp.v[j], o_depth.v[j], o_lse.v[j], o_sn.v[j]);
  stv<PX>(disp + (long)b * a.HW + pix, o_disp);
  stv<PX>(depth + (long)b * a.HW + pix, o_depth);
  stv<PX>(stash + ((long)b * 2 + 0) * a.HW + pix, o_lse);
  stv<PX>(stash + ((long)b * 2 + 1) * a.HW + pix, o_sn);
}

// pi and probability (depth_decoder.py:275, 281-285) for callers that want the tensors.
template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__global__ __launch_bounds__(kBlock) void tail_layers_kernel(TailArgs a, const float* __restrict__ stash,
                                                             float* __restrict__ pi, float* __restrict__ prob) {
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  if (pix >= a.HW) return;
  const Px<PX> lse = ldv<PX>(stash + ((long)b * 2 + 0) * a.HW + pix);
  const Px<PX> sn = ldv<PX>(stash + ((long)b * 2 + 1) * a.HW + pix);
  const TailLane ln = tail_lane<RF>(a, b, pix);
#pragma unroll 2
  for (int n = 0; n < a.N; ++n) {
    const long i = ln.base + (long)n * a.HW;
    TailOperands<PX> q;
    tail_operands<ST, MIX, HASMASK, PX, RF, false>(a, ln, n, i, q);   // (no disparity here)
    Px<PX> op, oq;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float p = __expf(q.rl.v[j] * q.mk.v[j] - lse.v[j]);
      op.v[j] = p;
      oq.v[j] = MIX ? p * q.mk.v[j] / clamp_sigma(sigmoid_f(q.rs.v[j])) / sn.v[j] : p;
    }
    if (pi) stv<PX>(pi + i, op);
    if (prob) stv<PX>(prob + i, oq);
  }
}

// Backward.  With w_n = pi_n m_n / sigma_n, S = sum w, P_n = w_n / S, disp = sum P_n d_n and upstream gD = d loss/d disp
// (+ the depth term): d disp / d w_n = (d_n - disp) / S, and since sum_k pi_k (d loss / d pi_k) = gD/S * sum_k w_k
// (d_k - disp) = 0 exactly, the softmax backward needs no second reduction:
//   g_logits_n += gD (d_n - disp) P_n;   g_sigma_n -= gD (d_n - disp) P_n / sigma_n;   g_d_n = gD P_n.
// One pixel of one plane.
template <bool MIX>
__device__ __forceinline__ void tail_bwd_px(float rl, float rs, float mk, float dv, float gl, float gs, float lse, float sn,
                                            float dsp, float gD, float& o_l, float& o_s, float& o_d) {
  const float p = __expf(rl * mk - lse);
  float sgu = 1.0f, sg = 1.0f, P = p;
  if (MIX) {
    sgu = sigmoid_f(rs);
    sg = clamp_sigma(sgu);
    P = p * mk / sg / sn;
  }
  const float t = gD * (dv - dsp) * P;
  o_l = (gl + t) * mk;
  const float gsig = gs - t / sg;
  o_s = (sgu == sg) ? gsig * sgu * (1.0f - sgu) : 0.0f;   // clamp gate (inclusive bounds), sigmoid'
  o_d = gD * P;
}

// What the backward keeps per pixel over the planes: the stash, disp and the upstream gradient of disp.  An inactive lane
// (it only takes part in the reductions) gets values that are never used.
template <int PX>
struct TailBwdPixel {
  Px<PX> lse, sn, dsp, gD;
};
template <int PX>
__device__ __forceinline__ TailBwdPixel<PX> tail_bwd_pixel(const TailArgs& a, bool active, int b, int pix,
                                                           const float* __restrict__ stash, const float* __restrict__ disp,
                                                           const float* __restrict__ g_disp, const float* __restrict__ g_depth) {
  TailBwdPixel<PX> q = {splat<PX>(0.0f), splat<PX>(1.0f), splat<PX>(1.0f), splat<PX>(0.0f)};
  if (active) {
    q.lse = ldv<PX>(stash + ((long)b * 2 + 0) * a.HW + pix);
    q.sn = ldv<PX>(stash + ((long)b * 2 + 1) * a.HW + pix);
    q.dsp = ldv<PX>(disp + (long)b * a.HW + pix);
    q.gD = tail_upstream<PX>(g_disp, g_depth, (long)b * a.HW + pix, q.dsp, tail_depth_scale(a.W));
  }
  return q;
}
// One plane at an active lane: loads, tail_bwd_px per pixel, stores.  Adds the lane's disparity gradients to gd.  Each
// gradient pointer may be NULL; g_dl is written here in the dense form only (tested as the kernels always tested it: with another
// form of the test the compiler stopped contracting gd += gD * P into an fma, and the per-plane gradient's last bit moved).
template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__device__ __forceinline__ void tail_bwd_plane(const TailArgs& a, const TailLane& ln, int n, const TailBwdPixel<PX>& q,
                                               const float* __restrict__ g_logits, const float* __restrict__ g_sigma,
                                               float* __restrict__ g_raw_logits, float* __restrict__ g_raw_sigma,
                                               float* __restrict__ g_dl, float& gd) {
  const long i = ln.base + (long)n * a.HW;
  TailOperands<PX> o;
    tail_operands<ST, MIX, HASMASK, PX, RF>(a, ln, n, i, o);
  const Px<PX> gl = g_logits ? ldv<PX>(elems<ST>(g_logits) + i) : splat<PX>(0.0f);
  const Px<PX> gs = (MIX && g_sigma) ? ldv<PX>(elems<ST>(g_sigma) + i) : splat<PX>(0.0f);
  Px<PX> o_l, o_s, o_d;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    tail_bwd_px<MIX>(o.rl.v[j], o.rs.v[j], o.mk.v[j], o.dv.v[j], gl.v[j], gs.v[j], q.lse.v[j], q.sn.v[j], q.dsp.v[j], q.gD.v[j],
                     o_l.v[j], o_s.v[j], o_d.v[j]);
    gd += o_d.v[j];
  }
  if (g_raw_logits) stv<PX>(elems<ST>(g_raw_logits) + i, o_l);
  if (MIX && g_raw_sigma) stv<PX>(elems<ST>(g_raw_sigma) + i, o_s);
  if (!(RF & kRowDisp) && g_dl && a.dense) stv<PX>(g_dl + i, o_d);
}

// Pixel-linear form: per-plane or dense disparities (RF: 0, or kRowMask for a [B,N,H] mask).  The per-plane form's gradient
// goes through LDS-atomic block partials and reduce_partials.
template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__global__ __launch_bounds__(kBlock) void tail_bwd_kernel(TailArgs a, const float* __restrict__ stash, const float* __restrict__ disp,
                                                          const float* __restrict__ g_logits, const float* __restrict__ g_sigma,
                                                          const float* __restrict__ g_disp, const float* __restrict__ g_depth,
                                                          float* __restrict__ g_raw_logits, float* __restrict__ g_raw_sigma,
                                                          float* __restrict__ g_dl, float* __restrict__ partials) {
  extern __shared__ float red[];  // [N] block sums of the per-plane disparity gradient
  const int pix = (blockIdx.x * kBlock + threadIdx.x) * PX, b = blockIdx.y;
  const bool reduce = (g_dl != nullptr) && !a.dense;
  if (reduce) block_partials_zero(red, a.N);
  const bool active = pix < a.HW;
  const TailLane ln = tail_lane<RF>(a, b, active ? pix : 0);
  const TailBwdPixel<PX> q = tail_bwd_pixel<PX>(a, active, b, pix, stash, disp, g_disp, g_depth);
  for (int n = 0; n < a.N; ++n) {
    float gd = 0.0f;
    if (active) tail_bwd_plane<ST, MIX, HASMASK, PX, RF>(a, ln, n, q, g_logits, g_sigma, g_raw_logits, g_raw_sigma, g_dl, gd);
    if (reduce) block_partials_add(red, n, gd);
  }
  if (reduce) block_partials_store(red, partials, b, a.N);
}

// Row-owned form (PD_TAIL_DISP_ROWS; RF holds kRowDisp): workgroup (y, b) walks row y of image b in steps of blockDim.x * PX
// pixels, so every contribution to g_disp_layered[b,n,y] is its own.  Each wave keeps its sums in LDS slots of its own
// (red[wave][n]: plain read-add-write by one lane, no atomics), and plane n's thread adds the waves' in wave order.
template <class ST, bool MIX, bool HASMASK, int PX, int RF>
__global__ __launch_bounds__(kBlock) void tail_bwd_rows_kernel(TailArgs a, const float* __restrict__ stash,
                                                               const float* __restrict__ disp, const float* __restrict__ g_logits,
                                                               const float* __restrict__ g_sigma, const float* __restrict__ g_disp,
                                                               const float* __restrict__ g_depth, float* __restrict__ g_raw_logits,
                                                               float* __restrict__ g_raw_sigma, float* __restrict__ g_dl) {
  extern __shared__ float red[];  // [waves][N]
  const int y = blockIdx.x, b = blockIdx.y, H = gridDim.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
  const long rbase = (long)b * a.N * H;
  if (g_dl) {
    for (int i = threadIdx.x; i < nwaves * a.N; i += blockDim.x) red[i] = 0.0f;
    __syncthreads();
  }
  for (int x0 = 0; x0 < a.W; x0 += blockDim.x * PX) {   // (workgroup-uniform trip count: the wave sums below see every lane)
    const int x = x0 + threadIdx.x * PX;
    const bool active = x < a.W;
    const int pix = y * a.W + (active ? x : 0);
    const TailLane ln = {b, H, y, (long)b * a.N * a.HW + pix, rbase};
    const TailBwdPixel<PX> q = tail_bwd_pixel<PX>(a, active, b, pix, stash, disp, g_disp, g_depth);
    for (int n = 0; n < a.N; ++n) {
      float gd = 0.0f;
      if (active) tail_bwd_plane<ST, MIX, HASMASK, PX, RF>(a, ln, n, q, g_logits, g_sigma, g_raw_logits, g_raw_sigma, g_dl, gd);
      if (g_dl) {
        const float v = wave_sum_hi(gd);
        if (lane == kWave - 1) red[wave * a.N + n] += v;
      }
    }
  }
  if (g_dl) {
    __syncthreads();
    for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
      float s = red[n];
      for (int w = 1; w < nwaves; ++w) s += red[w * a.N + n];
      g_dl[rbase + (long)n * H + y] = s;
    }
  }
}

}  // namespace pd

using namespace pd;

extern "C" size_t pd_decoder_tail_bwd_workspace_floats(int B, int N, int H, int W) {
  return (size_t)B * ceil_div(H * W, kBlock) * N;   // the per-plane form's partial sums; the dense and the row forms need none
}

extern "C" int pd_decoder_tail_fwd(int B, int N, int H, int W, int flags, const float* raw_logits,
                                   const float* raw_sigma, const float* padding_mask, const float* disp_layered,
                                   float* logits, float* sigma, float* disp, float* depth, float* stash,
                                   pd_stream_t stream) {
  if (int rc = tail_validate(B, N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered)) return rc;
  PD_REQUIRE(disp && depth && stash, "NULL output");
  PD_REQUIRE(!(flags & PD_TAIL_MIXTURE) || sigma, "mixture needs the sigma output");
  PD_REQUIRE(!padding_mask || logits, "a padding mask needs the logits output");
  const TailArgs a = tail_args(N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered);
  const int rf = tail_rf(flags, padding_mask);
  const TailLaunch t = tail_launch(B, H, W, flags, rf, {(rf & kRowMask) ? nullptr : padding_mask, a.dense ? disp_layered : nullptr,
                                                        disp, depth, stash}, {raw_logits, raw_sigma, logits, sigma});
  PD_TAIL_DISPATCH_RF(tail_fwd_kernel, rf, t.bf16, t.px, a.mix, padding_mask != nullptr, t.grid, kBlock, 0, (hipStream_t)stream, a,
                      logits, sigma, disp, depth, stash);
  return check_launch("tail_fwd_kernel");
}

extern "C" int pd_decoder_tail_layers(int B, int N, int H, int W, int flags, const float* raw_logits,
                                      const float* raw_sigma, const float* padding_mask, const float* stash, float* pi,
                                      float* probability, pd_stream_t stream) {
  if (int rc = tail_validate(B, N, H, W, flags, raw_logits, raw_sigma, padding_mask, raw_logits)) return rc;
  PD_REQUIRE(stash && (pi || probability), "NULL pointer");
  const TailArgs a = tail_args(N, H, W, flags, raw_logits, raw_sigma, padding_mask, nullptr);
  const int rf = tail_rf(flags, padding_mask) & kRowMask;   // (disp_layered is not read here)
  const TailLaunch t = tail_launch(B, H, W, flags, rf, {rf ? nullptr : padding_mask, stash, pi, probability}, {raw_logits, raw_sigma});
  PD_TAIL_DISPATCH_MASK(tail_layers_kernel, 0, rf, t.bf16, t.px, a.mix, padding_mask != nullptr, t.grid, kBlock, 0,
                        (hipStream_t)stream, a, stash, pi, probability);
  return check_launch("tail_layers_kernel");
}

extern "C" int pd_decoder_tail_bwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                                   const float* padding_mask, const float* disp_layered, const float* stash, const float* disp,
                                   const float* g_logits, const float* g_sigma, const float* g_disp, const float* g_depth,
                                   float* g_raw_logits, float* g_raw_sigma, float* g_disp_layered, float* workspace, pd_stream_t stream) {
  if (int rc = tail_validate(B, N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered)) return rc;
  PD_REQUIRE(stash && disp, "NULL pointer");
  PD_REQUIRE(g_raw_logits || g_raw_sigma || g_disp_layered, "no gradient requested");
  const TailArgs a = tail_args(N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered);
  const int rf = tail_rf(flags, padding_mask);
  const bool reduce = g_disp_layered && !a.dense && !(rf & kRowDisp);
  PD_REQUIRE(!reduce || workspace, "per-plane disparity gradient needs the workspace");
  PD_REQUIRE((size_t)N * sizeof(float) <= 64 * 1024 / ((rf & kRowDisp) ? kBlock / kWave : 1), "too many planes");
  const bool hasmask = padding_mask != nullptr;
  const TailLaunch t = tail_launch(B, H, W, flags, rf, {(rf & kRowMask) ? nullptr : padding_mask, a.dense ? disp_layered : nullptr,
                                                        stash, disp, g_disp, g_depth, a.dense ? g_disp_layered : nullptr},
                                   {raw_logits, raw_sigma, g_logits, g_sigma, g_raw_logits, g_raw_sigma});
  if (rf & kRowDisp) {   // row-owned: workgroup (y, b), as many waves as the row has work for
    const int waves = ceil_div(ceil_div(W, t.px), kWave);
    const int threads = kWave * (waves < kBlock / kWave ? waves : kBlock / kWave);
    const size_t shmem = g_disp_layered ? (size_t)(threads / kWave) * N * sizeof(float) : 0;
    PD_TAIL_DISPATCH_MASK(tail_bwd_rows_kernel, kRowDisp, rf, t.bf16, t.px, a.mix, hasmask, dim3(H, B), threads, shmem,
                          (hipStream_t)stream, a, stash, disp, g_logits, g_sigma, g_disp, g_depth, g_raw_logits, g_raw_sigma,
                          g_disp_layered);
    return check_launch("tail_bwd_rows_kernel");
  }
  const size_t shmem = reduce ? (size_t)N * sizeof(float) : 0;
  PD_TAIL_DISPATCH_MASK(tail_bwd_kernel, 0, rf, t.bf16, t.px, a.mix, hasmask, t.grid, kBlock, shmem, (hipStream_t)stream, a, stash,
                        disp, g_logits, g_sigma, g_disp, g_depth, g_raw_logits, g_raw_sigma, g_disp_layered, workspace);
  if (int rc = check_launch("tail_bwd_kernel")) return rc;
  return reduce ? reduce_partials(workspace, g_disp_layered, (int)t.grid.x, N, B, (hipStream_t)stream) : 0;
}
