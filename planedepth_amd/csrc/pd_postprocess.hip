// Warps of the self-distillation post-process, Trainer.generate_post_process_disp (reference trainer.py:421-466;
// SURVEY.md §8f rank 2).  The reference builds two [B*N,H,W,2] grids, calls F.grid_sample five times on [B*N,1,H,W]
// tensors, two softmaxes over the planes and three sum/clamp passes.  Both shapes it needs are fused here:
//   pd_warp_softmax   out[b,n,y,x] = softmax_n( planes[b,n] sampled at (x + s*d[b,n], y) )       (trainer.py:443-446, 451-453)
//   pd_warp_sum       out[b,0,y,x] = min(cap, sum_n planes[b,n] sampled at (x + s*d[b,n], y) )   (:447-449, 454-456, 463-465)
// with the reference's pixel -> [-1,1] -> pixel round trip (trainer.py:427-441 + grid_sample, align_corners=True,
// zeros padding) reproduced through pd_common.h's normalise_roundtrip, and PD_PP_FLIP_SRC reading the source planes
// mirrored along x (the `.flip(-1)` of trainer.py:451) without materialising the flipped tensor.  Forward only: the
// reference runs this under the fixed (no-grad) networks and detaches the result (:466).
#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>
#include "pd_common.h"
#include "pd_rowshift_common.h"

namespace pd {

struct WarpArgs {
  int N, H, W;
  int dense, flip, rows;   // rows: disp is [B,N,H] — one disparity per (plane, row): xz planes (PD_PP_DISP_ROWS)
  int dimg, dplane, ymask; // disparity of (b, n, y) when !dense: disp[b * dimg + n * dplane + (y & ymask)] — (N, 1, 0) per plane,
                           // (N H, H, ~0) per row: 32-bit, branch-free (a select between two 64-bit addresses per plane cost the
                           // unrolled segment kernels 90 scalar instructions a plane)
  float sign;
  float Wm1, rcpWm1;   // W - 1 and its correctly rounded reciprocal (host-computed: 1/(W-1) in double, rounded once)
  const float* planes;
  const float* disp;
};

typedef float v2f_u4 __attribute__((ext_vector_type(2), aligned(4)));  // 8-byte load at 4-byte alignment

// These kernels are latency-bound gathers (no reuse, one thread per pixel), so the loop is shaped for loads in flight:
// everything that depends on the row only is hoisted (the vertical taps are the same for all planes), the two column
// taps of a row come as ONE 8-byte load from a clamped, always-valid position with the out-of-image cases folded into
// the weights (no branches around loads), planes go in groups of kGroup with all loads issued before the first use,
// and a wave whose pixels all have a zero second vertical weight (three rows of four: the reference's
// y -> [-1,1] -> y round trip is exact there) runs a one-row loop that never reads the second row.  (With finite
// inputs skipping a zero-weighted row gives the same number.)
constexpr int kGroup = 4;

struct RowTaps {        // per pixel, plane-independent
  int y;                // the target row itself
  int ra, rb;           // clamped source rows
  float wa, wb;         // their weights (0 when the row is outside the image)
};
__device__ __forceinline__ RowTaps row_taps(int y, int H) {   // make_row_sel's footprint with clamped rows and zeroed weights
  const RowSel s = make_row_sel(y, H);
  // lower / upper are make_row_sel's use0 / use1: yB is always y0 + 1, and with one live row yA is y0 (!= yB) when it is the lower
  // row and y0 + 1 (== yB) when it is the upper one; wA is wy0 whenever the lower row is live, wB is wy1 always.
  const bool lower = s.nrows == 2 || (s.nrows == 1 && s.yA != s.yB), upper = s.nrows == 2 || (s.nrows == 1 && s.yA == s.yB);
  RowTaps r;
  r.y = y;
  r.ra = min(max(s.yB - 1, 0), H - 1);
  r.rb = min(max(s.yB, 0), H - 1);
  r.wa = lower ? s.wA : 0.0f;
  r.wb = upper ? s.wB : 0.0f;
  return r;
}

struct ColPair {        // per pixel and plane: where to load the column pair and how to weight its two values
  int off;              // first column of the pair, in [0, W-2]
  float e0, e1;
};
template <bool FLIP>
__device__ __forceinline__ ColPair col_pair(float ix, int W) {
  const float xf = floorf(ix), xf1 = xf + 1.0f;
  const float wx0 = xf1 - ix, wx1 = ix - xf;
  const bool v0 = (xf >= 0.0f) && (xf <= (float)(W - 1)), v1 = (xf1 >= 0.0f) && (xf1 <= (float)(W - 1));
  const int x0 = (int)fminf(fmaxf(xf, -2.0f), (float)W);
  const int c = min(max(x0, 0), W - 2);
  const float g0 = v0 ? wx0 : 0.0f, g1 = v1 ? wx1 : 0.0f;   // weights of columns x0 and x0+1
  // the loaded pair is columns (c, c+1); x0 == c in the interior, c-1 at the left border, c+1 at the right one
  const float e0 = (x0 == c) ? g0 : ((x0 == c - 1) ? g1 : 0.0f);
  const float e1 = (x0 == c) ? g1 : ((x0 == c + 1) ? g0 : 0.0f);
  ColPair p;
  if (FLIP) { p.off = W - 2 - c; p.e0 = e1; p.e1 = e0; }    // mirrored columns: the pair is read in reverse order
  else      { p.off = c;         p.e0 = e0; p.e1 = e1; }
  return p;
}

__device__ __forceinline__ float plane_ix(const WarpArgs& a, int b, int n, int x, int y) {
  const float d = a.dense ? a.disp[(((long)b * a.N + n) * a.H + y) * a.W + x]
                          : a.disp[b * a.dimg + n * a.dplane + (y & a.ymask)];
  // the division by W-1 through its refined reciprocal: the same bits as IEEE division (pd_common.h), a third of the cost
  return normalise_roundtrip_rcp((float)x + a.sign * d, a.Wm1, a.rcpWm1);
}

// Samples of planes n0 .. n0+U-1 at this pixel (all loads first).
template <bool FLIP, int NR, int U>
__device__ __forceinline__ void sample_group(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b,
                                             int n0, int x, int y, int HW, float (&out)[U]) {
  ColPair cp[U];
  v2f_u4 va[U], vb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    cp[u] = col_pair<FLIP>(plane_ix(a, b, n0 + u, x, y), a.W);
    const float* pl = pb + (long)(n0 + u) * HW;
    va[u] = *reinterpret_cast<const v2f_u4*>(pl + (long)r.ra * a.W + cp[u].off);
    if (NR == 2) vb[u] = *reinterpret_cast<const v2f_u4*>(pl + (long)r.rb * a.W + cp[u].off);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float v = (va[u].x * cp[u].e0 + va[u].y * cp[u].e1) * r.wa;
    if (NR == 2) v += (vb[u].x * cp[u].e0 + vb[u].y * cp[u].e1) * r.wb;
    out[u] = v;
  }
}

// The plane-group loop of the gather and the row kernels: f(n, value) for every plane of a pixel, in plane order, kGroup planes with
// their loads in flight and then a tail of single planes; group(n0, v) samples planes n0 .. n0 + U - 1 into v[U]
template <typename G, typename F>
__device__ __forceinline__ void for_each_plane(int N, G group, F f) {
  int n = 0;
  for (; n + kGroup <= N; n += kGroup) {
    float v[kGroup];
    group(n, v);
#pragma unroll
    for (int u = 0; u < kGroup; ++u) f(n + u, v[u]);
  }
  for (; n < N; ++n) {
    float v[1];
    group(n, v);
    f(n, v[0]);
  }
}
template <bool FLIP, int NR, typename F>
__device__ __forceinline__ void for_each_sample(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b,
                                                int x, int y, int HW, F f) {
  for_each_plane(a.N, [&](int n0, auto& v) __attribute__((always_inline)) { sample_group<FLIP, NR>(a, pb, r, b, n0, x, y, HW, v); }, f);
}

// Online softmax over the planes: pass 1 keeps the running maximum m and the sum Z of exp(l - m), pass 2 samples again and emits
// exp(l - m) / Z
__device__ __forceinline__ void softmax_accumulate(float& m, float& Z, float l) {
  if (l > m) { Z *= __expf(m - l); m = l; }
  Z += __expf(l - m);
}
__device__ __forceinline__ float softmax_emit(float l, float m, float invZ) { return __expf(l - m) * invZ; }

// Softmax over the planes of the warped logits.  Pass 1 finds max and sum, pass 2 samples again and writes the
// probabilities: N writes and (cache permitting) N reads per pixel.  Measured at 4x49x192x640: 92-100 us; parking the
// sampled logits in `out` between the passes (2N writes + 2N reads) 118 us; parking them in LDS (128-thread workgroups,
// 25 KB each) 120 us — the kernel is VALU-bound (coordinate chain + tap set-up per plane), LDS costs it occupancy.
template <bool FLIP>
__global__ __launch_bounds__(kBlock) void warp_softmax_kernel(WarpArgs a, float* __restrict__ out) {
  const int HW = a.H * a.W;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  const bool active = pix < HW;
  const int y = active ? pix / a.W : 0, x = active ? pix - y * a.W : 0;
  const RowTaps r = row_taps(y, a.H);
  const bool two_rows = __any(active && r.wb != 0.0f);   // wave-uniform
  if (!active) return;
  const float* pb = a.planes + (long)b * a.N * HW;
  float* ob = out + (long)b * a.N * HW + pix;
  float m = -INFINITY, Z = 0.0f;
  auto stat = [&](int, float l) { softmax_accumulate(m, Z, l); };
  if (two_rows) for_each_sample<FLIP, 2>(a, pb, r, b, x, y, HW, stat);
  else          for_each_sample<FLIP, 1>(a, pb, r, b, x, y, HW, stat);
  const float invZ = 1.0f / Z;
  auto emit = [&](int n, float l) { ob[(long)n * HW] = softmax_emit(l, m, invZ); };
  if (two_rows) for_each_sample<FLIP, 2>(a, pb, r, b, x, y, HW, emit);
  else          for_each_sample<FLIP, 1>(a, pb, r, b, x, y, HW, emit);
}

template <bool FLIP>
__global__ __launch_bounds__(kBlock) void warp_sum_kernel(WarpArgs a, float cap, float* __restrict__ out) {
  const int HW = a.H * a.W;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  const bool active = pix < HW;
  const int y = active ? pix / a.W : 0, x = active ? pix - y * a.W : 0;
  const RowTaps r = row_taps(y, a.H);
  const bool two_rows = __any(active && r.wb != 0.0f);
  if (!active) return;
  const float* pb = a.planes + (long)b * a.N * HW;
  float acc = 0.0f;
  auto add = [&](int, float v) { acc += v; };
  if (two_rows) for_each_sample<FLIP, 2>(a, pb, r, b, x, y, HW, add);
  else          for_each_sample<FLIP, 1>(a, pb, r, b, x, y, HW, add);
  out[(long)b * HW + pix] = fminf(acc, cap);   // o[o > 1] = 1
}

// ---------------------------------------------------------------------------------------------------------------
// Per-plane scalar disparities (the decoder's expanded [B,N,1,1] levels, the usual case): along a target row every pixel
// samples plane n at x + s*d_n, so the row-shift machinery of the sweep applies — one wave per 64-pixel segment of a
// row, the vertical taps are wave-uniform scalars, each (plane, row) gets a buffer descriptor whose hardware range
// check IS padding_mode="zeros", the two column taps come in one 8-byte load (column -1 fixed up through the
// weights), and the sampling position costs make_col_tap's 7 operations instead of the general chain — half the
// instructions of the gather kernels above in a VALU-bound loop.  FLIP reads the pair at the mirrored columns.
// ---------------------------------------------------------------------------------------------------------------
struct RowPair {   // where the pair load goes and how its two dwords are weighted
  unsigned off;
  float e0, e1;
};
template <bool FLIP>
__device__ __forceinline__ RowPair row_pair(const ColTap& t, int W) {
  // columns x0 / x0+1 carry weights w0 / w1; mirrored, they are columns W-1-x0 / W-2-x0, read as the pair at W-2-x0
  const int c = FLIP ? W - 2 - t.x0 : t.x0;
  const bool edge = (c == -1);   // the pair starts one column left of the row: load at column 0, its first dword is the second tap
  RowPair p;
  p.off = edge ? 0u : ((unsigned)c << 2);   // any other out-of-row position is range-checked to zeros by the hardware
  const float first = FLIP ? t.w1 : t.w0, second = FLIP ? t.w0 : t.w1;
  p.e0 = edge ? second : first;
  p.e1 = edge ? 0.0f : second;
  return p;
}

// the shift s*d_n, clamped like the sweep's staged shifts (clamp_shift; keeps x0*4 from aliasing)
__device__ __forceinline__ float plane_shift(const WarpArgs& a, int b, int n, int y) {
  return clamp_shift(a.sign * a.disp[b * a.dimg + n * a.dplane + (y & a.ymask)], a.W, false);
}

template <bool FLIP, int NR, int U>
__device__ __forceinline__ void rows_group(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b,
                                           int n0, int x, int HW, float (&out)[U]) {
  RowPair rp[U];
  v2f va[U], vb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    rp[u] = row_pair<FLIP>(make_col_tap((float)x + plane_shift(a, b, n0 + u, r.y), a.Wm1, a.rcpWm1), a.W);
    const float* pl = pb + (long)(n0 + u) * HW;   // wave-uniform
    va[u] = buf_load2(row_rsrc(pl + (long)r.ra * a.W, a.W), rp[u].off);
    if (NR == 2) vb[u] = buf_load2(row_rsrc(pl + (long)r.rb * a.W, a.W), rp[u].off);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float v = (va[u].x * rp[u].e0 + va[u].y * rp[u].e1) * r.wa;
    if (NR == 2) v += (vb[u].x * rp[u].e0 + vb[u].y * rp[u].e1) * r.wb;
    out[u] = v;
  }
}

template <bool FLIP, int NR, typename F>
__device__ __forceinline__ void rows_for_each(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b,
                                              int x, int HW, F f) {
  for_each_plane(a.N, [&](int n0, auto& v) __attribute__((always_inline)) { rows_group<FLIP, NR>(a, pb, r, b, n0, x, HW, v); }, f);
}

// grid (segments of 64 pixels, H, B), one wave per workgroup
template <bool FLIP>
__global__ __launch_bounds__(kWave) void warp_softmax_rows_kernel(WarpArgs a, float* __restrict__ out) {
  const int HW = a.H * a.W, y = blockIdx.y, b = blockIdx.z;
  const int x = blockIdx.x * kWave + threadIdx.x;
  const RowTaps r = row_taps(y, a.H);   // wave-uniform
  const float* pb = a.planes + (long)b * a.N * HW;
  const bool active = x < a.W;
  float* ob = out + (long)b * a.N * HW + (long)y * a.W + (active ? x : 0);
  float m = -INFINITY, Z = 0.0f;
  auto stat = [&](int, float l) { softmax_accumulate(m, Z, l); };
  if (r.wb != 0.0f) rows_for_each<FLIP, 2>(a, pb, r, b, x, HW, stat);
  else              rows_for_each<FLIP, 1>(a, pb, r, b, x, HW, stat);
  const float invZ = 1.0f / Z;
  auto emit = [&](int n, float l) { if (active) ob[(long)n * HW] = softmax_emit(l, m, invZ); };
  if (r.wb != 0.0f) rows_for_each<FLIP, 2>(a, pb, r, b, x, HW, emit);
  else              rows_for_each<FLIP, 1>(a, pb, r, b, x, HW, emit);
}

template <bool FLIP>
__global__ __launch_bounds__(kWave) void warp_sum_rows_kernel(WarpArgs a, float cap, float* __restrict__ out) {
  const int HW = a.H * a.W, y = blockIdx.y, b = blockIdx.z;
  const int x = blockIdx.x * kWave + threadIdx.x;
  const RowTaps r = row_taps(y, a.H);
  const float* pb = a.planes + (long)b * a.N * HW;
  float acc = 0.0f;
  auto add = [&](int, float v) { acc += v; };
  if (r.wb != 0.0f) rows_for_each<FLIP, 2>(a, pb, r, b, x, HW, add);
  else              rows_for_each<FLIP, 1>(a, pb, r, b, x, HW, add);
  if (x < a.W) out[(long)b * HW + (long)y * a.W + x] = fminf(acc, cap);
}

// ---------------------------------------------------------------------------------------------------------------
// Segment form of the two (round 6): the segment-stream forward's access shape (pd_plane_sweep_fwdstream.hip).  One wave owns a
// 128-pixel segment of a target row, a lane two adjacent pixels; their taps on plane n are the three source values at
// x + k .. x + k + 2, k = floor(s d_n): ONE 12-byte load per live source row (half the memory instructions per pixel of the
// 8-byte form above), coordinates through stream_ix, and — what the softmax gains most from — the sampled logits of ALL planes
// stay in registers (2 x N <= 128 VGPRs), so the planes are sampled ONCE: the kernels above sample twice (statistics, then
// probabilities).  FLIP reads the same three columns mirrored: the taps of pixels x, x+1 at mirrored columns c, c+1, c+2 are the
// actual columns W-1-c .. W-3-c, one 12-byte load at W-3-c in reverse order.  Exactness as in the forward: planes whose
// frac(s d) is within irregular_tol of an integer take the per-pixel path of the row kernels above (exact floor(ix), 8-byte
// pairs).  A lane whose load would START at column -2 or -1 (such a load reads as zeros as a whole although its last columns are
// inside the row; at -3 its last dword passes the 32-bit range check and reads the neighbouring row) aims it at column 0 and
// shifts the three values into place (seg_load) — no per-segment fallback for negative shifts.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kSegPix = 2 * kWave;   // pixels per wave
constexpr int kSegWaves = 4;         // waves per workgroup (independent items)

struct SegPlane {   // wave-uniform: one plane's shift for this segment
  float sd;
  int k;
  bool general;
};
// The shifts of planes nbase .. nbase + 63, one per lane (plane_shift's value: sign, clamp): ONE vector load per wave and 64 planes,
// whatever the disparities' layout; a plane's shift is then a v_readlane away.  (Scalar loads per plane were fine while the
// per-plane layout let the compiler fold n into the load's immediate and fetch sixteen planes at a time; with a run-time stride
// every plane waited for its own s_load: +30-50 % on the chain kernels.)
__device__ __forceinline__ float seg_shifts(const WarpArgs& a, int b, int y, int nbase) {
  const int n = min(nbase + (int)(threadIdx.x & (kWave - 1)), a.N - 1);
  return plane_shift(a, b, n, y);
}
__device__ __forceinline__ float shift_of(float shifts, int j) {   // j: wave-uniform lane index
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(shifts), j));
}
__device__ __forceinline__ SegPlane seg_plane(const WarpArgs& a, float sd) {
  SegPlane p;
  ShiftClass c;
  classify_shift(sd, a.W, c);
  p.sd = sd;
  p.k = c.k;
  p.general = c.irr;   // (a load that would start left of the row is re-aimed per lane: seg_load)
  return p;
}

// Where a lane's 12-byte load goes when its three columns start at `start` (may be negative): columns left of the row are zero
// padding, but the hardware drops a load that STARTS there as a whole (and lets the dword at byte offset -4 through).  start in
// {-2, -1}: load columns 0 .. 2 and shift them right by adj = -start when the values are used; start <= -3: nothing of it is
// inside the row — an offset beyond every row (the range check returns zeros).
struct SegAim { unsigned off; int adj; };
__device__ __forceinline__ SegAim seg_aim(int start) {
  SegAim m;
  m.adj = (start < 0 && start >= -2) ? -start : 0;
  m.off = (start <= -3) ? 0x7FFFFFF0u : ((unsigned)(start + m.adj) << 2);
  return m;
}
__device__ __forceinline__ v3f seg_place(const v3f& t, int adj) {
  v3f o;
  o.x = (adj == 0) ? t.x : 0.0f;
  o.y = (adj == 0) ? t.y : ((adj == 1) ? t.x : 0.0f);
  o.z = (adj == 0) ? t.z : ((adj == 1) ? t.y : t.x);
  return o;
}

// the two samples of a lane on one plane from its loaded taps (A = first live row, B = second)
template <bool FLIP, int NR>
__device__ __forceinline__ void seg_values(const WarpArgs& a, const RowTaps& r, const SegPlane& p, float x0f, const v3f& ta,
                                           const v3f& tb, float& v0, float& v1) {
  const float kf = (float)p.k;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float xtf = x0f + (float)i, xsf = xtf + kf;          // integers below 2^24: exact
    const float ix = stream_ix(xtf, p.sd, a.Wm1, a.rcpWm1);
    const float w1 = ix - xsf, w0 = (xsf + 1.0f) - ix;         // torch's (ix - x0), (x1 - ix) with x0 = x + k
    // plain: pixel i reads taps i (w0), i + 1 (w1); mirrored: the three columns arrive reversed
    const float a0 = FLIP ? (i == 0 ? ta.z : ta.y) : (i == 0 ? ta.x : ta.y), a1 = FLIP ? (i == 0 ? ta.y : ta.x) : (i == 0 ? ta.y : ta.z);
    float v = (a0 * w0 + a1 * w1) * r.wa;
    if (NR == 2) {
      const float b0 = FLIP ? (i == 0 ? tb.z : tb.y) : (i == 0 ? tb.x : tb.y), b1 = FLIP ? (i == 0 ? tb.y : tb.x) : (i == 0 ? tb.y : tb.z);
      v += (b0 * w0 + b1 * w1) * r.wb;
    }
    if (i == 0) v0 = v; else v1 = v;
  }
}

// f(n, v0, v1) for every plane of the lane's two pixels, in plane order; loads of kGroup planes in flight
template <bool FLIP, int NR, int G, typename F>
__device__ __forceinline__ void seg_group(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b, int x0, int HW,
                                          int n0, F& f, float shifts, int sbase, int nbase = 0, int nend = 1 << 30) {
  // planes nbase + n0 .. nbase + n0 + G - 1 (those below min(nend, N)); the callback sees the index RELATIVE to nbase, which is a
  // compile-time constant where the caller's loop is unrolled
  const float x0f = (float)x0;
  const int nlim = min(nend, a.N);
  {
    SegPlane sp[G];
    v3f ta[G], tb[G];
    int adj[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int n = min(nbase + n0 + u, a.N - 1);
      sp[u] = seg_plane(a, shift_of(shifts, n - sbase));
      const float* pl = pb + (long)n * HW;
      const SegAim aim = seg_aim(FLIP ? a.W - 3 - (x0 + sp[u].k) : x0 + sp[u].k);
      adj[u] = aim.adj;
      ta[u] = buf_load3(row_rsrc(pl + (long)r.ra * a.W, a.W), aim.off);
      if (NR == 2) tb[u] = buf_load3(row_rsrc(pl + (long)r.rb * a.W, a.W), aim.off);
      else tb[u] = ta[u];
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int n = nbase + n0 + u;
      if (n < nlim) {   // (uniform)
      float v0, v1;
      if (sp[u].general) {   // (uniform) exact per-pixel path
        float o0[1], o1[1];
        rows_group<FLIP, NR, 1>(a, pb, r, b, n, x0, HW, o0);
        rows_group<FLIP, NR, 1>(a, pb, r, b, n, x0 + 1, HW, o1);
        v0 = o0[0]; v1 = o1[0];
      } else {
        seg_values<FLIP, NR>(a, r, sp[u], x0f, seg_place(ta[u], adj[u]), seg_place(tb[u], adj[u]), v0, v1);
      }
      f(n0 + u, v0, v1);
      }
    }
  }
}
// NMAX > 0: the plane loop fully unrolled over NMAX >= N planes, group by group through an index pack (the callback then sees
// compile-time plane indices and its per-plane state stays in registers; a `break` in a pragma-unrolled loop left it in scratch);
// NMAX == 0: a run-time loop
template <bool FLIP, int NR, int G, typename F, int... I>
__device__ __forceinline__ void seg_groups(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b, int x0, int HW,
                                           F& f, std::integer_sequence<int, I...>, int nbase, int nend, float shifts) {
  ((nbase + I * G < min(nend, a.N) ? seg_group<FLIP, NR, G>(a, pb, r, b, x0, HW, I * G, f, shifts, 0, nbase, nend) : (void)0), ...);
}
template <bool FLIP, int NR, int NMAX, typename F, int G = kGroup>   // G planes' loads in flight per wave
__device__ __forceinline__ void seg_for_each(const WarpArgs& a, const float* __restrict__ pb, const RowTaps& r, int b, int x0, int HW,
                                             F f, int nbase = 0, int nend = 1 << 30) {
  if constexpr (NMAX > 0) {   // (at most 64 planes: one register of shifts)
    const float shifts = seg_shifts(a, b, r.y, 0);
    seg_groups<FLIP, NR, G>(a, pb, r, b, x0, HW, f, std::make_integer_sequence<int, (NMAX + G - 1) / G>{}, nbase, nend, shifts);
  } else {
    float shifts = 0.0f;
    for (int n0 = 0; n0 < a.N; n0 += G) {
      if ((n0 & (kWave - 1)) == 0) shifts = seg_shifts(a, b, r.y, n0);   // (G divides 64)
      seg_group<FLIP, NR, G>(a, pb, r, b, x0, HW, n0, f, shifts, n0 & ~(kWave - 1));
    }
  }
}

// which (image, row, segment) a wave serves: items row-major, kSegWaves consecutive ones per workgroup
struct SegItem { int b, y, xseg; bool on; };
__device__ __forceinline__ SegItem seg_item(const WarpArgs& a, int B) {
  const int nseg = (a.W + kSegPix - 1) / kSegPix;
  const long item = (long)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  SegItem s;
  s.on = item < (long)B * a.H * nseg;
  const long it = s.on ? item : 0;
  s.xseg = (int)(it % nseg) * kSegPix;
  s.y = (int)((it / nseg) % a.H);
  s.b = (int)(it / ((long)nseg * a.H));
  s.xseg = __builtin_amdgcn_readfirstlane(s.xseg); s.y = __builtin_amdgcn_readfirstlane(s.y); s.b = __builtin_amdgcn_readfirstlane(s.b);
  return s;
}

// The softmax with all planes of a lane's pixel pair in registers: NS slots per pixel, -inf where no plane was kept; the maxima and
// sums are the caller's locals (as members of a struct beside the slots they cost the unrolled kernels a VGPR and scratch).
template <int NS>
__device__ __forceinline__ void slots_clear(float (&l0)[NS], float (&l1)[NS]) {
#pragma unroll
  for (int n = 0; n < NS; ++n) l0[n] = l1[n] = -INFINITY;
}
template <int NS>
__device__ __forceinline__ void slots_keep(float (&l0)[NS], float (&l1)[NS], float& m0, float& m1, int n, float v0, float v1) {
#pragma unroll
  for (int q = 0; q < NS; ++q) if (q == n) { l0[q] = v0; l1[q] = v1; }   // (n is a compile-time constant once unrolled)
  m0 = fmaxf(m0, v0); m1 = fmaxf(m1, v1);
}
// slots -> exp(slot - m), Z = their sum (an empty slot adds exp(-inf) = 0).  EMPTY_OK: no slot may have been kept at all (a part
// without planes: m = -inf) — exp(-inf - -inf) is guarded to 0, Z = 0
template <bool EMPTY_OK, int NS>
__device__ __forceinline__ void slots_exp(float (&l0)[NS], float (&l1)[NS], float m0, float m1, float& Z0, float& Z1) {
  Z0 = Z1 = 0.0f;
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    l0[n] = (EMPTY_OK && m0 == -INFINITY) ? 0.0f : __expf(l0[n] - m0);
    l1[n] = (EMPTY_OK && m1 == -INFINITY) ? 0.0f : __expf(l1[n] - m1);
    Z0 += l0[n]; Z1 += l1[n];
  }
}

template <bool FLIP, int NR, int NMAX>
__device__ __forceinline__ void seg_softmax_body(const WarpArgs& a, const SegItem& it, const RowTaps& r, float* __restrict__ out) {
  const int HW = a.H * a.W, lane = threadIdx.x & (kWave - 1);
  const int x0 = it.xseg + 2 * lane;
  const float* pb = a.planes + (long)it.b * a.N * HW;
  float l0[NMAX], l1[NMAX], m0 = -INFINITY, m1 = -INFINITY, Z0, Z1;
  slots_clear(l0, l1);
  seg_for_each<FLIP, NR, NMAX>(a, pb, r, it.b, x0, HW, [&](int n, float v0, float v1) { slots_keep(l0, l1, m0, m1, n, v0, v1); });
  slots_exp<false>(l0, l1, m0, m1, Z0, Z1);
  if (x0 >= a.W) return;   // (W is even: the lane's two pixels are inside or outside together)
  const float i0 = 1.0f / Z0, i1 = 1.0f / Z1;
  float* ob = out + (long)it.b * a.N * HW + (long)it.y * a.W + x0;
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
    if (n < a.N) *reinterpret_cast<float2*>(ob + (long)n * HW) = make_float2(l0[n] * i0, l1[n] * i1);
}

// (NMAX = 64: 128 registers of samples; bounded to three waves per SIMD — unbounded the allocator takes 206 VGPRs = two waves,
// and the kernel is no faster than the row form)
template <bool FLIP, int NMAX>
__global__ __launch_bounds__(kSegWaves* kWave, NMAX > 32 ? 3 : 4) void warp_softmax_seg_kernel(WarpArgs a, int B, float* __restrict__ out) {
  const SegItem it = seg_item(a, B);
  if (!it.on) return;
  const RowTaps r = row_taps(it.y, a.H);   // wave-uniform
  if (r.wb != 0.0f) seg_softmax_body<FLIP, 2, NMAX>(a, it, r, out);
  else              seg_softmax_body<FLIP, 1, NMAX>(a, it, r, out);
}

template <bool FLIP>
__global__ __launch_bounds__(kSegWaves* kWave) void warp_sum_seg_kernel(WarpArgs a, int B, float cap, float* __restrict__ out) {
  const SegItem it = seg_item(a, B);
  if (!it.on) return;
  const RowTaps r = row_taps(it.y, a.H);
  const int HW = a.H * a.W, lane = threadIdx.x & (kWave - 1);
  const int x0 = it.xseg + 2 * lane;
  const float* pb = a.planes + (long)it.b * a.N * HW;
  float acc0 = 0.0f, acc1 = 0.0f;
  auto add = [&](int, float v0, float v1) { acc0 += v0; acc1 += v1; };
  if (r.wb != 0.0f) seg_for_each<FLIP, 2, 0>(a, pb, r, it.b, x0, HW, add);
  else              seg_for_each<FLIP, 1, 0>(a, pb, r, it.b, x0, HW, add);
  if (x0 < a.W) *reinterpret_cast<float2*>(out + (long)it.b * HW + (long)it.y * a.W + x0) = make_float2(fminf(acc0, cap), fminf(acc1, cap));
}

// ---------------------------------------------------------------------------------------------------------------
// Row chains (round 6): softmax(warp(logits)) never leaves the CU.  trainer.py:443-449 / 451-456 warp the logits, take the softmax
// over the planes, warp THAT again and sum over the planes; with per-plane disparities both warps are horizontal, so the second
// one samples, for a target row, the softmax's rows ya / yb only — and its horizontal part does not depend on the target row:
//   S_r(x) = sum_n hinterp(softmax_row_r[n], x + s2 d2_n),        o(y, x) = min(1, wa_y S_ya(x) + wb_y S_yb(x))
// (the vertical weights factor out of the plane sum; fp32 reassociation only).  One workgroup per (chain, image, row r): the
// segment form samples the row's logits (all planes of a pixel pair in registers), writes the normalised probabilities into an
// LDS row buffer [N][W + 4] (125 KB at 49 x 640: one workgroup per CU) and then takes S_r from LDS with the exact per-pixel taps
// (make_col_tap; zero guard cells are the padding).  The [B,N,H,W] intermediate of the two-kernel form — written and read back,
// twice per call: 4 N of the path's 7 N planes of traffic — is gone; what remains are S rows, and pp_rows_finish_kernel applies the
// vertical weights, the clamp and the disp_pp blend.
// ---------------------------------------------------------------------------------------------------------------
#ifndef PD_PP_CHAIN_G
#define PD_PP_CHAIN_G 4
#endif
struct ChainSide {
  WarpArgs w;             // the chain's first warp
  const float* disp2;     // the second warp's disparities [B,N] ([B,N,H] with rows2) and sign
  float sign2;
  float* S;               // [3][B,1,H,W]: S_r with the shifts of target row r, r - 1, r + 1 (the last two with rows2 only, and only
};                        // where that neighbour blends row r in)
struct ChainArgs {
  ChainSide side[2];      // chain 0 (image, plain) / chain 1 (mirrored image, PD_PP_FLIP_SRC)
  int B;
};
// Which targets need S of source row r: r itself always; with per-row shifts also the neighbours t = r -+ 1 whose vertical taps
// reach r (their shift differs from row r's) — the inexact rows of the y round trip, a quarter of them at H = 192.
__device__ __forceinline__ bool chain_needs(int r, int t, int H) {
  if (t < 0 || t >= H) return false;
  const RowTaps q = row_taps(t, H);
  return (q.ra == r && q.wa != 0.0f) || (q.rb == r && q.wb != 0.0f);
}
// the second warp's shifts of planes 0 .. 63 under target row yt, one per lane (clamp_shift, as plane_shift)
__device__ __forceinline__ float chain_shifts(const ChainSide& s, int rows2, int b, int yt) {
  const int N = s.w.N, n = min((int)(threadIdx.x & (kWave - 1)), N - 1);
  return clamp_shift(s.sign2 * s.disp2[rows2 ? (b * N + n) * s.w.H + yt : b * N + n], s.w.W, false);
}
// The row buffer [N][W + 4]: zero guard cells at columns -2, -1, W, W + 1 of every plane are the second warp's padding
__device__ __forceinline__ void chain_zero_guards(float* __restrict__ lds, int N, int W) {
  const int RS = W + 4;
  for (int i = threadIdx.x; i < 4 * N; i += blockDim.x) {
    const int n = i >> 2, g = i & 3;
    lds[n * RS + (g < 2 ? g : W + g)] = 0.0f;
  }
}
// The second warp's taps of planes [nb, ne) at the lane's pixels x0, x0 + 1, summed over the planes: from the row buffer, with the exact
// per-pixel taps (make_col_tap); sh2: chain_shifts
__device__ __forceinline__ void chain_tap_sum(const WarpArgs& a, const float* __restrict__ lds, float sh2, int nb, int ne, int x0,
                                              float& acc0, float& acc1) {
  const int W = a.W, RS = W + 4;
  acc0 = acc1 = 0.0f;
  for (int n = nb; n < ne; ++n) {
    const float sd = shift_of(sh2, n);
    const float* row = lds + n * RS;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const ColTap t = make_col_tap((float)(x0 + i) + sd, a.Wm1, a.rcpWm1);
      const int cell = min(max(t.x0, -2), W) + 2;
      const float val = row[cell] * t.w0 + row[cell + 1] * t.w1;
      if (i == 0) acc0 += val; else acc1 += val;
    }
  }
}
__device__ __forceinline__ float2* chain_S(float* __restrict__ S, int v, int B, int b, int HW, int W, int y, int x0) {   // S map v at (b, y, x0)
  return reinterpret_cast<float2*>(S + ((long)v * B + b) * HW + (long)y * W + x0);
}

template <bool FLIP, int NR, int NMAX, bool ROWS2>
__device__ __forceinline__ void chain_row(const ChainSide& s, int B, int b, int y, const RowTaps& r, float* __restrict__ lds) {
  const WarpArgs& a = s.w;
  const int W = a.W, N = a.N, HW = a.H * a.W, RS = W + 4;
  constexpr int rows2 = ROWS2 ? 1 : 0;   // (a template flag: as a run-time one it cost the per-plane case 30-50 % — NOTEBOOK 11.4)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* pb = a.planes + (long)b * N * HW;
  chain_zero_guards(lds, N, W);
  // (one segment per wave, no loop around the unrolled planes: inside a loop every plane's shift and descriptors are
  // loop-invariant, get hoisted, and 5 500 spilled SGPRs later the kernel lives in scratch)
  const int seg = wave;
  {
    const int xseg = seg * kSegPix, x0 = xseg + 2 * lane;
    float l0[NMAX], l1[NMAX], m0 = -INFINITY, m1 = -INFINITY, Z0, Z1;
    slots_clear(l0, l1);
    auto keep = [&](int n, float v0, float v1) { slots_keep(l0, l1, m0, m1, n, v0, v1); };
    // (one workgroup of nseg waves per CU: the loads in flight have to come from each wave — PD_PP_CHAIN_G planes at a time)
    seg_for_each<FLIP, NR, NMAX, decltype(keep), PD_PP_CHAIN_G>(a, pb, r, b, x0, HW, keep);
    slots_exp<false>(l0, l1, m0, m1, Z0, Z1);
    if (x0 < W) {
      const float i0 = 1.0f / Z0, i1 = 1.0f / Z1;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < N) *reinterpret_cast<float2*>(lds + n * RS + 2 + x0) = make_float2(l0[n] * i0, l1[n] * i1);
    }
  }
  __syncthreads();
  for (int v = 0; v < (rows2 ? 3 : 1); ++v) {   // S_r under the shifts of target row y, y - 1, y + 1 (workgroup-uniform)
    const int yt = (v == 0) ? y : ((v == 1) ? y - 1 : y + 1);
    if (v > 0 && !chain_needs(y, yt, a.H)) continue;
    const int x0 = seg * kSegPix + 2 * lane;
    float acc0, acc1;
    chain_tap_sum(a, lds, chain_shifts(s, rows2, b, yt), 0, N, x0, acc0, acc1);
    if (x0 < W) *chain_S(s.S, v, B, b, HW, W, y, x0) = make_float2(acc0, acc1);
  }
}

// The same with the planes of a segment dealt to P waves (P x nseg waves per workgroup: 15 at W = 640).  One workgroup per CU is
// all the row buffer allows, so the loads in flight and the issue slots of four SIMDs have to come from its own waves: with one
// wave per segment (5 per CU) the kernel ran at 1.2 TB/s.  Wave (seg, part) samples planes [part * NPART, (part + 1) * NPART),
// leaves (max, sum of exp relative to it) per pixel in LDS, takes the segment's max / sum from the P parts after a barrier, writes
// its planes' probabilities, and after the next barrier sums ITS planes' taps of the second warp; part 0 adds the partial sums.
template <bool FLIP, int NR, int NPART, int P, bool ROWS2, bool ALIAS>
__device__ __forceinline__ void chain_row_split(const ChainSide& s, int B, int b, int y, const RowTaps& r, float* __restrict__ lds) {
  const WarpArgs& a = s.w;
  const int W = a.W, N = a.N, HW = a.H * a.W, RS = W + 4;
  constexpr int rows2 = ROWS2 ? 1 : 0;   // (a template flag, as in chain_row)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nseg = (W + kSegPix - 1) / kSegPix;
  const int seg = wave % nseg, part = wave / nseg;
  const int nb = part * NPART, ne = min(nb + NPART, N);
  const int SW = nseg * kSegPix;                                 // stats row: one float2 per pixel of the padded row and part
  // ALIAS (the row buffer alone fills the CU's LDS: 63 planes x 640): the parts' statistics and, later, their partial sums live
  // INSIDE the row buffer — while no probabilities are there yet, and after the last one has been read; two more barriers
  float2* stats = ALIAS ? reinterpret_cast<float2*>(lds) : reinterpret_cast<float2*>(lds + (size_t)N * RS);
  const float* pb = a.planes + (long)b * N * HW;
  if (!ALIAS) chain_zero_guards(lds, N, W);
  const int x0 = seg * kSegPix + 2 * lane;
  float l0[NPART], l1[NPART], m0 = -INFINITY, m1 = -INFINITY, Z0, Z1;
  slots_clear(l0, l1);
  auto keep = [&](int j, float v0, float v1) { slots_keep(l0, l1, m0, m1, j, v0, v1); };
  seg_for_each<FLIP, NR, NPART, decltype(keep), kGroup>(a, pb, r, b, x0, HW, keep, nb, ne);
  slots_exp<true>(l0, l1, m0, m1, Z0, Z1);   // (a part without planes: m = -inf, Z = 0)
  stats[part * SW + x0] = make_float2(m0, Z0);
  stats[part * SW + x0 + 1] = make_float2(m1, Z1);
  __syncthreads();
  float M0 = -INFINITY, M1 = -INFINITY;
#pragma unroll
  for (int q = 0; q < P; ++q) { M0 = fmaxf(M0, stats[q * SW + x0].x); M1 = fmaxf(M1, stats[q * SW + x0 + 1].x); }
  float T0 = 0.0f, T1 = 0.0f;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const float2 s0 = stats[q * SW + x0], s1 = stats[q * SW + x0 + 1];
    T0 += (s0.x == -INFINITY) ? 0.0f : s0.y * __expf(s0.x - M0);
    T1 += (s1.x == -INFINITY) ? 0.0f : s1.y * __expf(s1.x - M1);
  }
  const float c0 = (m0 == -INFINITY) ? 0.0f : __expf(m0 - M0) / T0, c1 = (m1 == -INFINITY) ? 0.0f : __expf(m1 - M1) / T1;
  if (ALIAS) {   // every wave has its statistics in registers before the first probability overwrites them
    __syncthreads();
    chain_zero_guards(lds, N, W);
  }
  if (x0 < W) {
#pragma unroll
    for (int j = 0; j < NPART; ++j)
      if (nb + j < ne) *reinterpret_cast<float2*>(lds + (nb + j) * RS + 2 + x0) = make_float2(l0[j] * c0, l1[j] * c1);
  }
  __syncthreads();   // (every wave has read the stats by now: the buffer is free for the partial sums)
  constexpr int NV = ROWS2 ? 3 : 1;
  float accv[NV][2];
  bool need[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {   // S_r under the shifts of target row y, y - 1, y + 1 (workgroup-uniform)
    const int yt = (v == 0) ? y : ((v == 1) ? y - 1 : y + 1);
    need[v] = (v == 0) || chain_needs(y, yt, a.H);
    accv[v][0] = accv[v][1] = 0.0f;
    if (!need[v]) continue;
    float acc0, acc1;
    chain_tap_sum(a, lds, chain_shifts(s, rows2, b, yt), nb, ne, x0, acc0, acc1);
    accv[v][0] = acc0; accv[v][1] = acc1;
    if (!ALIAS) {   // the partial sums go through the statistics' buffer, variant by variant
      if (part > 0) stats[part * SW + x0] = make_float2(acc0, acc1);
      __syncthreads();
      if (part == 0 && x0 < W) {
#pragma unroll
        for (int q = 1; q < P; ++q) { const float2 o = stats[q * SW + x0]; acc0 += o.x; acc1 += o.y; }
        *chain_S(s.S, v, B, b, HW, W, y, x0) = make_float2(acc0, acc1);
      }
      if (ROWS2) __syncthreads();   // (the partial sums of the next variant go into the same buffer)
    }
  }
  if (ALIAS) {   // the probabilities have been read for the last time: the partial sums of every variant go where they were
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (need[v] && part > 0) stats[(v * P + part) * SW + x0] = make_float2(accv[v][0], accv[v][1]);
    __syncthreads();
    if (part == 0 && x0 < W) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (!need[v]) continue;
        float acc0 = accv[v][0], acc1 = accv[v][1];
#pragma unroll
        for (int q = 1; q < P; ++q) { const float2 o = stats[(v * P + q) * SW + x0]; acc0 += o.x; acc1 += o.y; }
        *chain_S(s.S, v, B, b, HW, W, y, x0) = make_float2(acc0, acc1);
      }
    }
  }
}

// (The item decode and the (FLIP, NR) dispatch are spelled out in both kernels: behind one helper that hands FLIP and NR to a generic
// lambda, the irregular planes' second-row term `A wa + B wb` was contracted the other way round in the second pixel of a lane — one
// ulp in the NR = 2 rows of S; profiles/postprocess_refactor_ab.md.)
template <int NPART, int P, bool ROWS2, bool ALIAS>
__global__ __launch_bounds__(1024) void pp_chain_split_kernel(ChainArgs c) {
  extern __shared__ float chain_lds[];
  const int H = c.side[0].w.H;
  const int item = blockIdx.x;
  const int y = item % H, b = (item / H) % c.B, chain = item / (H * c.B);
  const RowTaps r = row_taps(y, H);
  if (chain == 0) {
    if (r.wb != 0.0f) chain_row_split<false, 2, NPART, P, ROWS2, ALIAS>(c.side[0], c.B, b, y, r, chain_lds);
    else              chain_row_split<false, 1, NPART, P, ROWS2, ALIAS>(c.side[0], c.B, b, y, r, chain_lds);
  } else {
    if (r.wb != 0.0f) chain_row_split<true, 2, NPART, P, ROWS2, ALIAS>(c.side[1], c.B, b, y, r, chain_lds);
    else              chain_row_split<true, 1, NPART, P, ROWS2, ALIAS>(c.side[1], c.B, b, y, r, chain_lds);
  }
}

template <int NMAX, bool ROWS2>
__global__ __launch_bounds__(512) void pp_chain_kernel(ChainArgs c) {   // (at most 8 waves: 256 VGPRs for the sample registers)
  extern __shared__ float chain_lds[];
  const int H = c.side[0].w.H;
  const int item = blockIdx.x;                       // (chain, image, row): the rows of one image side by side
  const int y = item % H, b = (item / H) % c.B, chain = item / (H * c.B);
  const RowTaps r = row_taps(y, H);
  if (chain == 0) {
    if (r.wb != 0.0f) chain_row<false, 2, NMAX, ROWS2>(c.side[0], c.B, b, y, r, chain_lds);
    else              chain_row<false, 1, NMAX, ROWS2>(c.side[0], c.B, b, y, r, chain_lds);
  } else {
    if (r.wb != 0.0f) chain_row<true, 2, NMAX, ROWS2>(c.side[1], c.B, b, y, r, chain_lds);
    else              chain_row<true, 1, NMAX, ROWS2>(c.side[1], c.B, b, y, r, chain_lds);
  }
}

// o_l / o_fr from the S rows (vertical weights of the second warp, the clamp of trainer.py:449 / 456) and the disp_pp blend.
// S is [3][B,1,H,W]: source row rho contributes to target y through the variant computed with y's shifts — 0 for rho == y,
// 1 for rho == y + 1, 2 for rho == y - 1 (`rows2`; with per-plane shifts variant 0 serves everyone).  A zero weight reads nothing.
__device__ __forceinline__ float chain_o(const float* __restrict__ S, int B, int b, long HW, int W, int x, int y, const RowTaps& r,
                                         int rows2) {
#pragma clang fp contract(off)
  float o = 0.0f;
  if (r.wa != 0.0f) o = S[((long)((!rows2 || r.ra == y) ? 0 : ((r.ra == y + 1) ? 1 : 2)) * B + b) * HW + (long)r.ra * W + x] * r.wa;
  if (r.wb != 0.0f) o = o + S[((long)((!rows2 || r.rb == y) ? 0 : ((r.rb == y + 1) ? 1 : 2)) * B + b) * HW + (long)r.rb * W + x] * r.wb;
  return fminf(o, 1.0f);
}
// disp_pp of trainer.py:458-461 at pixel i = (b, y, x) from the two occlusion masks:
//   mean = disp[b] * 0.5 + flip(disp[B + b]) * 0.5;  pp = mean * o_fr + disp[b] * (1 - o_fr);  pp = pp * o_l + flip(disp[B + b]) * (1 - o_l)
// in torch's operation order (every product and sum rounded on its own).
__device__ __forceinline__ float pp_blend(const float* __restrict__ disp, int B, int b, long HW, int W, int x, int y, long i, float ofr,
                                          float ol) {
#pragma clang fp contract(off)
  const float d0 = disp[i], df = disp[((long)B + b) * HW + (long)y * W + (W - 1 - x)];
  const float mean = d0 * 0.5f + df * 0.5f;
  const float pp = mean * ofr + d0 * (1.0f - ofr);
  return pp * ol + df * (1.0f - ol);
}
__global__ __launch_bounds__(kBlock) void pp_rows_finish_kernel(int B, int H, int W, int rows2, const float* __restrict__ S_l,
                                                                const float* __restrict__ S_fr, const float* __restrict__ disp,
                                                                float* __restrict__ out) {
  const long HW = (long)H * W, i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long)B * HW) return;
  const int b = (int)(i / HW);
  const long p = i - (long)b * HW;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const RowTaps r = row_taps(y, H);
  const float ol = chain_o(S_l, B, b, HW, W, x, y, r, rows2), ofr = chain_o(S_fr, B, b, HW, W, x, y, r, rows2);
  out[i] = pp_blend(disp, B, b, HW, W, x, y, i, ofr, ol);
}

// the blend on its own (the single warps' o_fr / o_l): one pass instead of eight elementwise launches
__global__ __launch_bounds__(kBlock) void pp_combine_kernel(int B, int H, int W, const float* __restrict__ disp,
                                                            const float* __restrict__ o_fr, const float* __restrict__ o_l,
                                                            float* __restrict__ out) {
  const long HW = (long)H * W, i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long)B * HW) return;
  const int b = (int)(i / HW);
  const long p = i - (long)b * HW;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  out[i] = pp_blend(disp, B, b, HW, W, x, y, i, o_fr[i], o_l[i]);
}

// pixel pairs: even width, 8-byte aligned output rows; the softmax holds 2 N samples in registers
static bool seg_applicable(const WarpArgs& a, int B, const float* out, int nmax) {
  return !switches().pp_seg_off && !a.dense && (a.W % 2 == 0) && a.N <= nmax && (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
         (long)B * a.H * ((a.W + kSegPix - 1) / kSegPix) < (1L << 31) * kSegWaves && a.W <= (1 << 24);
}

// the row kernels need 32-bit byte offsets inside a row and grid dimensions within the launch limits
static bool rows_applicable(const WarpArgs& a, int B) {
  return !a.dense && a.H <= 65535 && B <= 65535 && a.W <= (1 << 24);
}

// (query: a route query — shape and flags only, no tensors)
static int warp_args(WarpArgs& a, int B, int N, int H, int W, float sign, int flags, const float* planes,
                     const float* disp, bool query = false) {
  PD_REQUIRE(B > 0 && B <= 65535 && N > 0 && H > 0 && W > 1, "bad shape");
  PD_REQUIRE((long)H * W < (1L << 31), "image too large");
  PD_REQUIRE((flags & ~(PD_PP_DISP_DENSE | PD_PP_FLIP_SRC | PD_PP_DISP_ROWS)) == 0, "unknown flags");
  PD_REQUIRE(!((flags & PD_PP_DISP_DENSE) && (flags & PD_PP_DISP_ROWS)), "PD_PP_DISP_DENSE and PD_PP_DISP_ROWS exclude each other");
  PD_REQUIRE(query || (planes && disp), "NULL pointer");
  a.N = N; a.H = H; a.W = W;
  a.dense = (flags & PD_PP_DISP_DENSE) != 0;
  a.rows = (flags & PD_PP_DISP_ROWS) != 0;
  PD_REQUIRE(!a.rows || (long)B * N * H < (1L << 31), "too many (image, plane, row) disparities for 32-bit indices");
  a.dimg = a.rows ? N * H : N; a.dplane = a.rows ? H : 1; a.ymask = a.rows ? ~0 : 0;
  a.flip = (flags & PD_PP_FLIP_SRC) != 0;
  a.sign = sign; a.planes = planes; a.disp = disp;
  a.Wm1 = (float)(W - 1);
  {  // the correctly rounded fp32 reciprocal of W-1: candidates around the double quotient, |r * d - 1| exact in double
    const double dd = (double)(W - 1);
    float best = (float)(1.0 / dd);
    const float cand[2] = {nextafterf(best, 0.0f), nextafterf(best, 2.0f)};
    for (float c : cand)
      if (fabs((double)c * dd - 1.0) < fabs((double)best * dd - 1.0)) best = c;
    a.rcpWm1 = best;
  }
  return 0;
}

// The route of pd_warp_softmax / pd_warp_sum (include/planedepth_hip.h: pd_pp_route).  The entry points switch on what this returns,
// pd_warp_route reports it: there is no second copy of a predicate.
static pd_pp_route warp_route(int kind, const WarpArgs& a, int B, const void* out) {
  pd_pp_route r = {};
  r.flip = a.flip;
  const bool softmax = kind == PD_PP_KIND_SOFTMAX;
  if (seg_applicable(a, B, static_cast<const float*>(out), softmax ? 64 : 1 << 20)) {
    r.family = PD_PP_FAMILY_SEG;
    r.nmax = !softmax ? 0 : (a.N <= 32 ? 32 : (a.N <= 52 ? 52 : 64));   // (52: the 49 planes)
  } else {
    r.family = rows_applicable(a, B) ? PD_PP_FAMILY_ROWS : PD_PP_FAMILY_GATHER;
  }
  return r;
}

// The route of pd_post_process.  Row chains where the softmax of a row fits the CU's LDS: per-plane (or per-row) disparities,
// pixel pairs, N <= 64.
static pd_pp_route post_process_route(int B, int N, int H, int W, int flags, const void* workspace, const void* disp_pp) {
  pd_pp_route r = {};
  r.family = PD_PP_FAMILY_SINGLE;
  const size_t chain_lds = (size_t)N * (W + 4) * sizeof(float);
  if (!(flags & PD_PP_DISP_DENSE) && !switches().pp_seg_off && (W % 2 == 0) && W <= 8 * kSegPix && N <= 64 && H <= 65535 &&
      chain_lds <= device_lds_bytes() && (long)2 * B * H < (1L << 31) &&
      ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(disp_pp)) & 7) == 0) {
    r.rows2 = (flags & PD_PP_DISP_ROWS) ? 1 : 0;
    const int nseg = ceil_div(W, kSegPix);
    // planes dealt to P = 3 waves per segment where the workgroup (3 nseg <= 16 waves) and its LDS (row buffer + one float2 per
    // pixel and part) fit; else one wave per segment
    const size_t side_lds = chain_lds + (size_t)3 * nseg * kSegPix * sizeof(float2);
    const bool alias = side_lds > device_lds_bytes();   // the parts' statistics / partial sums inside the row buffer (needs 9 maps of
                                                        // nseg x 128 float2 there: N >= 18 at W = 640)
    if (3 * nseg <= 16 && (!alias || (size_t)9 * nseg * kSegPix * sizeof(float2) <= chain_lds)) {
      r.family = PD_PP_FAMILY_CHAIN_SPLIT;
      r.nmax = N <= 33 ? 11 : (N <= 54 ? 18 : 22);
      r.alias = alias ? 1 : 0;
      r.lds_bytes = (uint32_t)(alias ? chain_lds : side_lds);
    } else {
      r.family = PD_PP_FAMILY_CHAIN;
      r.nmax = N <= 32 ? 32 : (N <= 52 ? 52 : 64);
      r.lds_bytes = (uint32_t)chain_lds;
    }
  }
  return r;
}

static int no_kernel(const char* what, const pd_pp_route& r) {
  set_error("%s: no kernel for route (family %d, flip %d, nmax %d, rows2 %d, alias %d)", what, r.family, r.flip, r.nmax, r.rows2, r.alias);
  return PD_ERR_UNSUPPORTED;
}

// A route's run-time values as the kernel templates' compile-time constants: dispatch_bool (pd_common.h), and f(std::integral_constant<int,
// V>{}) for the V of the list that r.nmax (NMAX or NPART) equals — no_kernel() if none does.  A generic lambda's call operator is
// instantiated once per constant, so a `static` inside it exists once per kernel instantiation.
template <int... V, typename F>
static int dispatch_nmax(const char* what, const pd_pp_route& r, F f) {
  int rc = PD_OK;
  return ((r.nmax == V && ((rc = f(std::integral_constant<int, V>{})), true)) || ...) ? rc : no_kernel(what, r);
}

// pd_warp_softmax / pd_warp_sum (`cap`: the sum's): the family switch, each family's grid once
static int launch_warp(int kind, const WarpArgs& a, int B, float cap, float* out, hipStream_t stream) {
  const bool softmax = kind == PD_PP_KIND_SOFTMAX;
  const char* what = softmax ? "pd_warp_softmax" : "pd_warp_sum";
  const pd_pp_route r = warp_route(kind, a, B, out);
  return dispatch_bool(r.flip, [&](auto flip) -> int {
    constexpr bool FLIP = decltype(flip)::value;
    switch (r.family) {
      case PD_PP_FAMILY_SEG: {
        const dim3 g((unsigned)(((long)B * a.H * ceil_div(a.W, kSegPix) + kSegWaves - 1) / kSegWaves)), block(kSegWaves * kWave);
        if (softmax)
          return dispatch_nmax<32, 52, 64>(what, r, [&](auto nmax) {
            warp_softmax_seg_kernel<FLIP, decltype(nmax)::value><<<g, block, 0, stream>>>(a, B, out);
            return check_launch("warp_softmax_seg_kernel");
          });
        if (r.nmax != 0) return no_kernel(what, r);
        warp_sum_seg_kernel<FLIP><<<g, block, 0, stream>>>(a, B, cap, out);
        return check_launch("warp_sum_seg_kernel");
      }
      case PD_PP_FAMILY_ROWS: {
        const dim3 g(ceil_div(a.W, kWave), a.H, B);
        if (softmax) warp_softmax_rows_kernel<FLIP><<<g, kWave, 0, stream>>>(a, out);
        else         warp_sum_rows_kernel<FLIP><<<g, kWave, 0, stream>>>(a, cap, out);
        return check_launch(softmax ? "warp_softmax_rows_kernel" : "warp_sum_rows_kernel");
      }
      case PD_PP_FAMILY_GATHER: {
        const dim3 g(ceil_div(a.H * a.W, kBlock), B);
        if (softmax) warp_softmax_kernel<FLIP><<<g, kBlock, 0, stream>>>(a, out);
        else         warp_sum_kernel<FLIP><<<g, kBlock, 0, stream>>>(a, cap, out);
        return check_launch(softmax ? "warp_softmax_kernel" : "warp_sum_kernel");
      }
      default: return no_kernel(what, r);
    }
  });
}

// A row-chain kernel on its dynamic LDS; `granted`: the caller's static, one per kernel instantiation
static int launch_chain(void (*kernel)(ChainArgs), LdsGrant& granted, const char* name, const ChainArgs& c, dim3 grid, dim3 block,
                        size_t lds, hipStream_t stream) {
  if (int rc = grant_dynamic_lds((const void*)kernel, lds, &granted, name)) return rc;
  kernel<<<grid, block, lds, stream>>>(c);
  return check_launch(name);
}

static int post_process_args(int B, int N, int H, int W, int flags) {   // of pd_post_process and its route query
  PD_REQUIRE(B > 0 && N > 0 && H > 0 && W > 1, "bad shape");
  PD_REQUIRE((flags & ~(PD_PP_DISP_DENSE | PD_PP_DISP_ROWS)) == 0, "unknown flags");
  return PD_OK;
}

}  // namespace pd

using namespace pd;

extern "C" int pd_warp_softmax(int B, int N, int H, int W, float sign, int flags, const float* planes,
                               const float* disp, float* out, pd_stream_t stream) {
  WarpArgs a;
  if (int rc = warp_args(a, B, N, H, W, sign, flags, planes, disp)) return rc;
  PD_REQUIRE(out && out != planes, "out must be a distinct buffer");
  return launch_warp(PD_PP_KIND_SOFTMAX, a, B, 0.0f, out, (hipStream_t)stream);
}

extern "C" int pd_warp_sum(int B, int N, int H, int W, float sign, int flags, const float* planes, const float* disp,
                           float cap, float* out, pd_stream_t stream) {
  WarpArgs a;
  if (int rc = warp_args(a, B, N, H, W, sign, flags, planes, disp)) return rc;
  PD_REQUIRE(out, "NULL output");
  return launch_warp(PD_PP_KIND_SUM, a, B, cap, out, (hipStream_t)stream);
}

extern "C" int pd_warp_route(int kind, int B, int N, int H, int W, int flags, const void* out, pd_pp_route* route) {
  PD_REQUIRE(kind == PD_PP_KIND_SOFTMAX || kind == PD_PP_KIND_SUM, "kind must be PD_PP_KIND_SOFTMAX or PD_PP_KIND_SUM");
  PD_REQUIRE(route, "NULL route");
  WarpArgs a;
  if (int rc = warp_args(a, B, N, H, W, 1.0f, flags, nullptr, nullptr, true)) return rc;
  *route = warp_route(kind, a, B, out);
  return PD_OK;
}

extern "C" int pd_pp_combine(int B, int H, int W, const float* disp, const float* o_fr, const float* o_l, float* disp_pp,
                             pd_stream_t stream) {
  PD_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31) * kBlock, "bad shape");
  PD_REQUIRE(disp && o_fr && o_l && disp_pp, "NULL pointer");
  pp_combine_kernel<<<(unsigned)(((long)B * H * W + kBlock - 1) / kBlock), kBlock, 0, (hipStream_t)stream>>>(B, H, W, disp, o_fr, o_l, disp_pp);
  return check_launch("pp_combine_kernel");
}

// The whole of trainer.py:443-465 behind one call: six launches on `stream`, no host work in between (as separate operator
// calls the ~0.2 ms of kernels at 8 x 49 x 192 x 640 were paced by the host's per-call overhead).
extern "C" size_t pd_post_process_workspace_floats(int B, int N, int H, int W) {
  return (size_t)B * N * H * W + (size_t)6 * B * H * W;   // the single warps' [B,N,H,W] intermediate + o_l / o_fr, or the chains' 2 x 3 S maps
}

extern "C" int pd_post_process(int B, int N, int H, int W, int flags, const float* logits, const float* probability,
                               const float* disp, const float* disp_layered, float* workspace, float* disp_pp, float* mask_novel,
                               pd_stream_t stream) {
  int rc;
  if ((rc = post_process_args(B, N, H, W, flags))) return rc;
  PD_REQUIRE(logits && probability && disp && disp_layered && workspace && disp_pp && mask_novel, "NULL pointer");
  const size_t P = (size_t)H * W, img = (size_t)N * P;
  const float* dl_r = disp_layered;                                                              // the image's planes
  const float* dl_l = disp_layered + ((flags & PD_PP_DISP_DENSE) ? (size_t)B * img                  // the mirrored image's
                                                                  : ((flags & PD_PP_DISP_ROWS) ? (size_t)B * N * H : (size_t)B * N));
  float* planes = workspace;
  float* o_l = workspace + (size_t)B * img;
  float* o_fr = o_l + (size_t)B * P;
  const char* what = "pd_post_process";
  const hipStream_t st = (hipStream_t)stream;
  const pd_pp_route r = post_process_route(B, N, H, W, flags, workspace, disp_pp);
  if (r.family == PD_PP_FAMILY_CHAIN_SPLIT || r.family == PD_PP_FAMILY_CHAIN) {
    ChainArgs c;
    const int rowsf = flags & PD_PP_DISP_ROWS;
    if ((rc = warp_args(c.side[0].w, B, N, H, W, +1.0f, rowsf, logits, dl_r))) return rc;
    if ((rc = warp_args(c.side[1].w, B, N, H, W, -1.0f, rowsf | PD_PP_FLIP_SRC, logits + (size_t)B * img, dl_l))) return rc;
    c.side[0].disp2 = dl_l; c.side[0].sign2 = -1.0f;
    c.side[1].disp2 = dl_r; c.side[1].sign2 = +1.0f;
    c.side[0].S = workspace; c.side[1].S = workspace + (size_t)3 * B * P;   // [3][B,1,H,W] each
    c.B = B;
    const bool split = r.family == PD_PP_FAMILY_CHAIN_SPLIT;   // planes dealt to P = 3 waves per segment; else one wave per segment
    const dim3 grid((unsigned)(2 * B * H)), block((split ? 3 : 1) * ceil_div(W, kSegPix) * kWave);
    rc = dispatch_bool(r.rows2, [&](auto r2) {
      constexpr bool R2 = decltype(r2)::value;
      if (!split)
        return dispatch_nmax<32, 52, 64>(what, r, [&](auto nmax) {
          static LdsGrant granted;
          return launch_chain(pp_chain_kernel<decltype(nmax)::value, R2>, granted, "pp_chain_kernel", c, grid, block, r.lds_bytes, st);
        });
      return dispatch_bool(r.alias, [&](auto alias) {
        return dispatch_nmax<11, 18, 22>(what, r, [&](auto npart) -> int {
          constexpr int NPART = decltype(npart)::value;
          constexpr bool ALIAS = decltype(alias)::value;
          // (the statistics fit beside the row buffer of at most 54 planes at any width the split chains take: no shape reaches
          // these at 160 KiB of LDS, tests/test_post_process_routes.py — they are not instantiated)
          if constexpr (ALIAS && NPART < 22) return no_kernel(what, r);
          else {
            static LdsGrant granted;
            return launch_chain(pp_chain_split_kernel<NPART, 3, R2, ALIAS>, granted, "pp_chain_split_kernel", c, grid, block, r.lds_bytes, st);
          }
        });
      });
    });
    if (rc) return rc;
    pp_rows_finish_kernel<<<(unsigned)(((long)B * P + kBlock - 1) / kBlock), kBlock, 0, st>>>(B, H, W, r.rows2, c.side[0].S, c.side[1].S, disp, disp_pp);
    if ((rc = check_launch("pp_rows_finish_kernel"))) return rc;
  } else if (r.family == PD_PP_FAMILY_SINGLE) {
    if ((rc = pd_warp_softmax(B, N, H, W, +1.0f, flags, logits, dl_r, planes, stream))) return rc;                         // :443-446
    if ((rc = pd_warp_sum(B, N, H, W, -1.0f, flags, planes, dl_l, 1.0f, o_l, stream))) return rc;                         // :447-449
    if ((rc = pd_warp_softmax(B, N, H, W, -1.0f, flags | PD_PP_FLIP_SRC, logits + (size_t)B * img, dl_l, planes, stream))) return rc;   // :451-453
    if ((rc = pd_warp_sum(B, N, H, W, +1.0f, flags, planes, dl_r, 1.0f, o_fr, stream))) return rc;                        // :454-456
    if ((rc = pd_pp_combine(B, H, W, disp, o_fr, o_l, disp_pp, stream))) return rc;                                        // :458-461
  } else {
    return no_kernel(what, r);
  }
  return pd_warp_sum(B, N, H, W, +1.0f, flags, probability, dl_r, 1.0f, mask_novel, stream);                             // :463-465
}

extern "C" int pd_post_process_route(int B, int N, int H, int W, int flags, const void* workspace, const void* disp_pp,
                                     pd_pp_route* route) {
  if (int rc = post_process_args(B, N, H, W, flags)) return rc;
  PD_REQUIRE(route, "NULL route");
  *route = post_process_route(B, N, H, W, flags, workspace, disp_pp);
  return PD_OK;
}
