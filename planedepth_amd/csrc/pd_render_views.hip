// Novel views at inference: from the decoder's conv outputs (or logits / sigma a tail already produced) and the source image to up
// to PD_RENDER_MAX_VIEWS rendered views in ONE forward-only kernel — the reference's pred_novel_images (trainer.py:540-603) on the
// tail of DepthDecoder.forward (depth_decoder.py:256-291), with the disparity scaled by a baseline factor s per view:
//   logits = raw_logits * mask; sigma = clamp(sigmoid(raw_sigma), .01, 1)                       (skipped with PD_RENDER_TAIL_APPLIED)
//   per plane n: sample colour, logits_n, sigma_n and a ones image at px = x + fl(s * d_n), zeros padding, times mask_n
//   p_n = softmax_N(logit_rec) [/ clamp(sigma_rec, .01, 1), renormalised];  rgb = sum p_n colour_n;  coverage = sum p_n ones_n;
//   disp = sum p_n d_n  (the rig's disparity, seen from the new view)
// Nothing [B,N,H,W]-sized is written and the conv outputs are read from memory once per launch, however many views it renders.
//
// One workgroup owns one target row (b, y) and walks the planes once.  For each plane the source row (both rows of an inexact
// vertical round trip: make_row_sel / two_row_form, blended once, the bilinear footprint being linear in the rows) is read, put
// through the tail step once per element and staged in LDS as (logit, sigma) cells with two zero guard cells on each side; the
// staged row then serves the taps of all V views — a per-plane or per-row disparity shifts the whole row uniformly, so
// neighbouring lanes read neighbouring cells.  The source colour row is staged once per workgroup the same way, its fourth
// component holding the ones image (the coverage).  The staging is double buffered: plane n+1's loads are in flight while
// plane n's taps run, one barrier per plane.  (A register ring that kept the loads of four planes in flight was measured and is
// slower, 0.27 against 0.20 ms at 8 x 49 x 192 x 640 with one view: the latency of the row loads is not what paces the kernel.)
// Every view keeps an online-softmax state per pixel (reference maximum, sum of
// weights, three colour sums, coverage sum, disparity sum), rescaled when the maximum moves as in pd_decoder_tail_infer.
// A view's arithmetic is written with explicit fused multiply-adds and contraction off (render_step, stage_value), so it does
// not depend on which other views share the launch: the same bits alone, among four, in any slot.
// No atomics, no scratch tensor, no workspace.
#include "pd_decoder_tail.h"
#include "pd_rowshift_common.h"

namespace pd {

constexpr int kRenderThreadsMax = 1024;   // 16 waves; a lane owns CPL columns (x = lane + c * threads)
constexpr int kRenderColsMax = 2;         // so rows up to 2048 pixels are served
constexpr int kRenderTwoColsFrom = 513;    // (render_cols)

struct RenderArgs {
  int B, N, H, W;
  int applied;        // PD_RENDER_TAIL_APPLIED: logits / sigma come in as a tail wrote them
  int disp_rows;      // disp_layered is [B,N,H]
  float row_eps;      // two_row_form's threshold (pd_sweep_auto_row_eps)
  const float* logits;
  const float* sigma;
  const float* mask;  // [B,N,H] or NULL
  const float* dl;
  const float* image;
  float s[PD_RENDER_MAX_VIEWS];
  float* rgb;
  float* coverage;
  float* disp;
};

struct ViewState {   // one view at one pixel
  float m, Sw, c0, c1, c2, cov, d;
};

// The staged value of one conv-output element pair (row A, row B of the vertical footprint), after the tail step.
__device__ __forceinline__ float stage_value(float vA, float vB, const RowSel& row, bool two) {
#pragma clang fp contract(off)
  return two ? fmaf(vB, row.wB, vA * row.wA) : vA;
}

// fl(s * d) through clamp_shift: the signed, scaled disparity of a plane for one view (a product that rounds on its own)
__device__ __forceinline__ float view_shift(float s, float d, int W) {
#pragma clang fp contract(off)
  const float sd = s * d;
  return clamp_shift(sd, W, false);
}

// One plane enters one view's state at one pixel.  cells: the staged (logit, sigma) row with guard cells; lrgb: the colour row.
template <bool MIX>
__device__ __forceinline__ void render_step(ViewState& st, const float2* __restrict__ cells, const float4* __restrict__ lrgb,
                                            float xtf, float sd, float d, float mt, int W, float Wm1, float rcpWm1) {
#pragma clang fp contract(off)
  const float ix = stream_ix(xtf, sd, Wm1, rcpWm1);
  const float xf = floorf(ix);
  const float w0 = ((xf + 1.0f) - ix) * mt, w1 = (ix - xf) * mt;   // (the mask multiplies the sampled features: trainer.py:580)
  const int xc = min(max((int)xf, -2), W) + 2;                     // far-out shifts land on a guard cell
  const float2 a = cells[xc], b = cells[xc + 1];
  const float4 ca = lrgb[xc], cb = lrgb[xc + 1];
  const float l = fmaf(b.x, w1, a.x * w0);
  if (l > st.m) {   // move the reference to the new maximum
    const float sc = __expf(st.m - l);
    st.Sw *= sc; st.c0 *= sc; st.c1 *= sc; st.c2 *= sc; st.cov *= sc; st.d *= sc;
    st.m = l;
  }
  float w = __expf(l - st.m);
  if (MIX) w = w * fast_rcp(clamp_sigma(fmaf(b.y, w1, a.y * w0)));   // trainer.py:597-600
  st.Sw += w;
  st.c0 = fmaf(w, fmaf(cb.x, w1, ca.x * w0), st.c0);
  st.c1 = fmaf(w, fmaf(cb.y, w1, ca.y * w0), st.c1);
  st.c2 = fmaf(w, fmaf(cb.z, w1, ca.z * w0), st.c2);
  st.cov = fmaf(w, fmaf(cb.w, w1, ca.w * w0), st.cov);
  st.d = fmaf(w, d, st.d);
}

template <class ST, bool MIX, int V, int CPL>
__global__ __launch_bounds__(kRenderThreadsMax) void render_views_kernel(RenderArgs a) {
  extern __shared__ __attribute__((aligned(16))) char render_lds[];
  const int W = a.W, H = a.H, N = a.N, HW = H * W, RS = W + 4;
  float4* lrgb = reinterpret_cast<float4*>(render_lds);                 // [RS] colour + ones
  float2* cells = reinterpret_cast<float2*>(render_lds + (size_t)RS * sizeof(float4));   // [2][RS] (logit, sigma)
  const int b = wg_image(a.B, H), y = wg_rowid(a.B, H);
  const int T = blockDim.x, tid = threadIdx.x;
  const RowSel row = two_row_form(make_row_sel(y, H), a.row_eps);
  const bool two = row.nrows == 2;
  const int yB = two ? row.yB : row.yA;

  // the colour row(s), blended, with the ones image in .w; guard cells of every staged row
  const float* srcb = a.image + (long)b * 3 * HW;
  for (int x = tid; x < W; x += T) {
    float4 c = blended_colour(srcb, row, two, x, W, HW);
    c.w = two ? row.wA + row.wB : 1.0f;
    lrgb[2 + x] = c;
  }
  if (tid < 4) {
    const int g = (tid < 2) ? tid : W + tid;   // cells 0, 1 and W+2, W+3
    lrgb[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    cells[g] = make_float2(0.f, 0.f);
    cells[RS + g] = make_float2(0.f, 0.f);
  }

  const ST* lg = elems<ST>(a.logits) + (long)b * N * HW;
  const ST* sg = MIX ? elems<ST>(a.sigma) + (long)b * N * HW : nullptr;
  const float* mrow = a.mask ? a.mask + (long)b * N * H : nullptr;
  const float* drow = a.dl + (a.disp_rows ? (long)b * N * H + y : (long)b * N);
  const int dstep = a.disp_rows ? H : 1;

  float rl[CPL][2], rs[CPL][2];   // plane n+1's raw elements, in flight while plane n's taps run
  auto issue = [&](int n) {
    const ST* pl = plane_ptr_t(lg, n, HW);
    const ST* ps = MIX ? plane_ptr_t(sg, n, HW) : nullptr;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int x = tid + c * T;
      rl[c][0] = rl[c][1] = rs[c][0] = rs[c][1] = 0.0f;
      if (x < W) {
        rl[c][0] = elem_f32(pl, (long)row.yA * W + x);
        if (two) rl[c][1] = elem_f32(pl, (long)yB * W + x);
        if (MIX) {
          rs[c][0] = elem_f32(ps, (long)row.yA * W + x);
          if (two) rs[c][1] = elem_f32(ps, (long)yB * W + x);
        }
      }
    }
  };
  // the tail step, once per element (depth_decoder.py:259, 278-279), then the vertical blend, into buffer n & 1; the second
  // source row's share only where the row has one (three rows in four have not)
  auto stage = [&](int n) {
    float2* dst = cells + (n & 1) * RS + 2;
    const float mA = (mrow && !a.applied) ? mrow[(long)n * H + row.yA] : 1.0f;
    const float mB = (mrow && !a.applied) ? mrow[(long)n * H + yB] : 1.0f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int x = tid + c * T;
      if (x < W) {
        float sA = rs[c][0], sB = rs[c][1];
        if (MIX && !a.applied) {
          sA = clamp_sigma(sigmoid_f(sA));
          if (two) sB = clamp_sigma(sigmoid_f(sB));
        }
        dst[x] = make_float2(stage_value(rl[c][0] * mA, rl[c][1] * mB, row, two), MIX ? stage_value(sA, sB, row, two) : 0.0f);
      }
    }
  };

  ViewState st[V][CPL];
#pragma unroll
  for (int v = 0; v < V; ++v)
#pragma unroll
    for (int c = 0; c < CPL; ++c) st[v][c] = {-INFINITY, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  const float Wm1 = (float)(W - 1), rcpWm1 = refined_rcp(Wm1);
  issue(0);
  stage(0);
  __syncthreads();
  for (int n = 0; n < N; ++n) {
    if (n + 1 < N) issue(n + 1);
    const float d = drow[(long)n * dstep];
    const float mt = mrow ? mrow[(long)n * H + y] : 1.0f;
    const float2* cur = cells + (n & 1) * RS;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float sd = view_shift(a.s[v], d, W);
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int x = tid + c * T;
        if (x < W) render_step<MIX>(st[v][c], cur, lrgb, (float)x, sd, d, mt, W, Wm1, rcpWm1);
      }
    }
    if (n + 1 < N) stage(n + 1);
    __syncthreads();   // plane n+1 is staged; nobody reads buffer n & 1 any more
  }

#pragma unroll
  for (int v = 0; v < V; ++v)
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int x = tid + c * T;
      if (x >= W) continue;
      const ViewState& s = st[v][c];
      const float inv = 1.0f / s.Sw;   // (the softmax normaliser cancels; Sw >= 1: the reference plane weighs e^0 / sigma)
      const long bv = (long)b * V + v, p = (long)y * W + x;
      a.rgb[(bv * 3 + 0) * HW + p] = s.c0 * inv;
      a.rgb[(bv * 3 + 1) * HW + p] = s.c1 * inv;
      a.rgb[(bv * 3 + 2) * HW + p] = s.c2 * inv;
      if (a.coverage) a.coverage[bv * HW + p] = s.cov * inv;
      if (a.disp) a.disp[bv * HW + p] = s.d * inv;
    }
}

static size_t render_lds_bytes(int W) { return (size_t)(W + 4) * (sizeof(float4) + 2 * sizeof(float2)); }

template <class ST, bool MIX, int V, int CPL>
static int render_launch(const RenderArgs& a, hipStream_t stream) {
  static LdsGrant granted;
  const size_t shmem = render_lds_bytes(a.W);
  if (int rc = grant_dynamic_lds((const void*)render_views_kernel<ST, MIX, V, CPL>, shmem, &granted, "render_views_kernel")) return rc;
  const int threads = ceil_div(ceil_div(a.W, CPL), kWave) * kWave;
  render_views_kernel<ST, MIX, V, CPL><<<dim3(a.H, a.B), threads, shmem, stream>>>(a);
  return check_launch("render_views_kernel");
}

// Columns per lane of a launch of V views on rows of W pixels (pd_render_cols_per_lane reports it; render_cols switches on it: the
// one place that holds the rule); 0: a width the staged-row layout does not take.
// Two columns per lane: above kRenderThreadsMax pixels there is no other way; from kRenderTwoColsFrom pixels on with one or two
// views, where half as many waves per row, each with twice the loads in flight, hide the row loads' latency better (8 x 49 x 192
// x 640, fp32, one view: 0.146 against 0.183 ms; with four views the registers of eight states cost more than that gains,
// 0.391 against 0.379 ms).  A pixel's arithmetic is the same in both forms.
static int render_cols_per_lane(int W, int V) {
  if (W < 2 || W > kRenderThreadsMax * kRenderColsMax || render_lds_bytes(W) > device_lds_bytes()) return 0;
  return (W > kRenderThreadsMax || (W >= kRenderTwoColsFrom && V <= 2)) ? kRenderColsMax : 1;
}

template <class ST, bool MIX, int V>
static int render_cols(const RenderArgs& a, hipStream_t stream) {
  switch (render_cols_per_lane(a.W, V)) {
    case 1: return render_launch<ST, MIX, V, 1>(a, stream);
    case kRenderColsMax: return render_launch<ST, MIX, V, kRenderColsMax>(a, stream);
    default: pd::set_error("pd_render_views: no kernel for W = %d with %d views", a.W, V); return PD_ERR_UNSUPPORTED;
  }
}
template <class ST, bool MIX>
static int render_v(int V, const RenderArgs& a, hipStream_t stream) {
  switch (V) {
    case 1: return render_cols<ST, MIX, 1>(a, stream);
    case 2: return render_cols<ST, MIX, 2>(a, stream);
    case 3: return render_cols<ST, MIX, 3>(a, stream);
    default: return render_cols<ST, MIX, 4>(a, stream);
  }
}

}  // namespace pd

using namespace pd;

#define PD_REFUSE_UNSUPPORTED(cond, ...) \
  do {                                   \
    if (cond) {                          \
      pd::set_error(__VA_ARGS__);        \
      return PD_ERR_UNSUPPORTED;         \
    }                                    \
  } while (0)

extern "C" int pd_render_cols_per_lane(int W, int V) {
  return (V >= 1 && V <= PD_RENDER_MAX_VIEWS) ? render_cols_per_lane(W, V) : 0;
}

extern "C" int pd_render_views(int B, int N, int H, int W, int V, int flags, const float* logits_in, const float* sigma_in,
                               const float* mask_rows, const float* disp_layered, const float* image, const float* baselines,
                               float* rgb, float* coverage, float* disp, pd_stream_t stream) {
  PD_REQUIRE(B > 0 && B <= 65535 && N > 0 && H > 1 && W > 1, "bad shape (B in 1..65535, N >= 1, H >= 2, W >= 2)");
  PD_REQUIRE(V >= 1 && V <= PD_RENDER_MAX_VIEWS, "V = %d: one launch renders 1..PD_RENDER_MAX_VIEWS (%d) views", V,
             PD_RENDER_MAX_VIEWS);
  PD_REQUIRE((flags & ~(PD_TAIL_MIXTURE | PD_TAIL_DISP_DENSE | PD_TAIL_BF16 | PD_TAIL_DISP_ROWS | PD_TAIL_MASK_ROWS |
                        PD_RENDER_TAIL_APPLIED)) == 0, "unknown flags");
  PD_REFUSE_UNSUPPORTED(flags & PD_TAIL_DISP_DENSE,
                        "flags: PD_TAIL_DISP_DENSE (a dense [B,N,H,W] disp_layered, yz planes) is not served: per-plane [B,N] "
                        "or PD_TAIL_DISP_ROWS [B,N,H] only");
  PD_REQUIRE(!(flags & PD_TAIL_MASK_ROWS) || mask_rows, "NULL pointer (PD_TAIL_MASK_ROWS in flags: mask_rows is read as [B,N,H])");
  PD_REQUIRE((flags & PD_TAIL_MASK_ROWS) || !mask_rows,
             "mask_rows without PD_TAIL_MASK_ROWS in flags (the only mask form is [B,N,H]; NULL = all ones)");
  PD_REQUIRE(logits_in && disp_layered && image && baselines && rgb,
             "NULL pointer (logits_in, disp_layered, image, baselines and rgb are required; coverage and disp may be NULL)");
  PD_REQUIRE(!(flags & PD_TAIL_MIXTURE) || sigma_in, "NULL pointer (PD_TAIL_MIXTURE in flags: the mixture needs sigma_in)");
  PD_REQUIRE((long)N * H * W < (1L << 31), "N*H*W = %ld: a plane set of 2^31 elements or more is not addressable here",
             (long)N * H * W);
  for (int v = 0; v < V; ++v)
    PD_REQUIRE(isfinite(baselines[v]), "baselines[%d] is not finite", v);
  const uintptr_t st_mask = (flags & PD_TAIL_BF16) ? 1 : 3;
  PD_REQUIRE(!((reinterpret_cast<uintptr_t>(logits_in) | reinterpret_cast<uintptr_t>(sigma_in)) & st_mask),
             "misaligned pointer (logits_in / sigma_in: %d-byte elements)", (int)st_mask + 1);
  PD_REQUIRE(!((reinterpret_cast<uintptr_t>(mask_rows) | reinterpret_cast<uintptr_t>(disp_layered) | reinterpret_cast<uintptr_t>(rgb) |
                reinterpret_cast<uintptr_t>(coverage) | reinterpret_cast<uintptr_t>(disp)) & 3),
             "misaligned pointer (mask_rows, disp_layered, rgb, coverage, disp: 4-byte elements)");
  PD_REQUIRE(!(reinterpret_cast<uintptr_t>(image) & 3), "misaligned pointer (image: 4-byte elements)");
  PD_REFUSE_UNSUPPORTED(render_cols_per_lane(W, V) == 0,
                        "W = %d: a row of more than %d pixels (or %zu bytes of LDS) does not fit the staged-row layout", W,
                        kRenderThreadsMax * kRenderColsMax, render_lds_bytes(W));

  RenderArgs a;
  a.B = B; a.N = N; a.H = H; a.W = W;
  a.applied = (flags & PD_RENDER_TAIL_APPLIED) != 0;
  a.disp_rows = (flags & PD_TAIL_DISP_ROWS) != 0;
  a.row_eps = pd_sweep_auto_row_eps();
  a.logits = logits_in; a.sigma = sigma_in; a.mask = mask_rows; a.dl = disp_layered; a.image = image;
  for (int v = 0; v < PD_RENDER_MAX_VIEWS; ++v) a.s[v] = v < V ? baselines[v] : 0.0f;
  a.rgb = rgb; a.coverage = coverage; a.disp = disp;
  const hipStream_t s = (hipStream_t)stream;
  if (flags & PD_TAIL_BF16)
    return (flags & PD_TAIL_MIXTURE) ? render_v<Bf16, true>(V, a, s) : render_v<Bf16, false>(V, a, s);
  return (flags & PD_TAIL_MIXTURE) ? render_v<float, true>(V, a, s) : render_v<float, false>(V, a, s);
}
