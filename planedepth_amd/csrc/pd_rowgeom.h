// Pure geometry of a target row, shared by the row-organised kernels (pd_plane_sweep_fwdstream.hip, pd_plane_sweep_rowstream.hip,
// pd_plane_sweep_rowshift.hip with pd_rowshift_fwd.h, pd_postprocess.hip): the vertical footprint of a row and its pairing with a
// neighbour, the bit-exact horizontal sampling position of the reference, and a plane's shift along the row (clamp, classification,
// the packed form kept in LDS).  Nothing in this file touches memory: pd_rowshift_common.h is the memory layer on top of it.
#pragma once
#include <math.h>

#include "pd_sweep.h"

namespace pd {

// Vertical footprint of target row y (workgroup-uniform): up to two live source rows with their weights.
struct RowSel {
  int nrows;      // 0, 1 or 2 live rows
  int yA, yB;     // source rows (yB only if nrows == 2)
  float wA, wB;   // their bilinear weights
  float wy_main;  // weight of the workgroup's own row y (vertical adjoint)
};

__device__ __forceinline__ RowSel make_row_sel(int y, int H) {
  RowSel r;
  const float iy = normalise_roundtrip((float)y, (float)(H - 1));
  const float yf = floorf(iy);
  const float wy0 = (yf + 1.0f) - iy, wy1 = iy - yf;
  const int y0 = (int)yf;
  const bool use0 = (yf >= 0.0f) && (yf <= (float)(H - 1)) && (wy0 != 0.0f);
  const bool use1 = (yf + 1.0f >= 0.0f) && (yf + 1.0f <= (float)(H - 1)) && (wy1 != 0.0f);
  r.nrows = (int)use0 + (int)use1;
  r.yA = use0 ? y0 : y0 + 1;
  r.wA = use0 ? wy0 : (use1 ? wy1 : 0.0f);
  r.yB = y0 + 1;
  r.wB = wy1;
  if (r.nrows == 0) r.yA = min(max(y0, 0), H - 1);
  r.wy_main = (y0 == y) ? wy0 : ((y0 + 1 == y) ? wy1 : 0.0f);
  return r;
}

// The one-row bodies drop the multiplications by the vertical weight: they run only for rows whose single live source
// row is the row itself with weight exactly 1 (every row whose normalise -> un-normalise round trip is exact).  Anything
// else with one live row (weight 1 - eps at an image border) is rewritten as a two-row footprint with a zero second
// weight on the same row, which the two-row bodies handle in full generality.
// Vertical round-trip noise.  The reference's y -> normalise -> un-normalise chain returns y + e with |e| <= 6e-6 for a
// quarter of the rows (fp32 rounding; exact arithmetic gives y), which makes grid_sample blend in the NEXT source row
// with weight e.  (Forward values and per-pixel gradients always use that second row; only the ADJOINT's e-weighted
// term into the neighbouring row is dropped: pd_plane_sweep_rowshift.hip's header.)  Serving that second row exactly
// doubles the loads of those rows (measured at 8x49x192x640: forward
// 0.137 -> 0.104 ms, backward 0.31 -> 0.30 ms, HBM reads -20% without it).  It is served by default all the same:
// dropping it moves results by up to e * (range of the logits), measured 4e-5 (rgb_rec) .. 1e-4 (g_sigma) of the
// tensors' range on random inputs — the whole 1e-4 parity budget.  PD_IMPL_FAST_ROWS opts into dropping a second row
// whose weight is below 2^-16 (smooth network outputs make the difference far smaller than random test data does).
// row_eps: a second source row whose weight is BELOW it is dropped (0: none is — PD_IMPL_EXACT_ROWS).
__device__ __forceinline__ RowSel two_row_form(RowSel r, float row_eps) {
  if (row_eps > 0.0f && r.nrows == 2) {
    const bool a_main = r.wA >= r.wB;
    if ((a_main ? r.wB : r.wA) < row_eps) {
      r.nrows = 1;
      r.yA = a_main ? r.yA : r.yB;
      r.wA = 1.0f;
      r.wy_main = 1.0f;
      return r;
    }
  }
  if (r.nrows == 1 && (r.wA != 1.0f || r.wy_main != 1.0f)) {
    r.nrows = 2;
    r.yB = r.yA;
    r.wB = 0.0f;
  }
  return r;
}

// ---- row pairs (pd_rowshift_fwd.h has the full story) ------------------------------------------------------------------
// A row y whose vertical round trip is inexact samples (1 - eps) * row y + eps * row p with p = y +- 1 ("leans" on p).  When p
// is exact, or leans back on y, one workgroup serves BOTH target rows from the two source rows it loads anyway, and the
// workgroup of p retires at once.  The rule is local (rows y-1 .. y+1), so every workgroup decides its own role without a table:
//   * y leans on p, p leans back on y  -> the lower of the two leads;
//   * y leans on p, p exact            -> y leads unless p-1 also leans on p and y = p+1 (the upper neighbour wins);
//   * y leans on p, p leans elsewhere  -> y stays a single two-source-row row (a chain; rare).
// At H = 192: 48 inexact rows -> 26 pairs, 10 left alone; H = 384: 94 -> 60 + 14.
enum PairRole { kSingle = 0, kLeader = 1, kAbsorbed = 2 };

__device__ __forceinline__ int row_lean(int y, int H) {  // 0: exact; +-1: direction of the second source row
  if (y < 0 || y >= H) return 0;
  const RowSel r = make_row_sel(y, H);
  if (r.nrows != 2) return 0;
  return (r.yA == y) ? +1 : -1;  // rows (y, y+1) or (y-1, y)
}
__device__ __forceinline__ bool leads(int y, int H) {  // y is inexact and takes its partner along
  const int l = row_lean(y, H);
  if (l == 0) return false;
  const int p = y + l;
  const int lp = row_lean(p, H);
  if (lp == -l) return y < p;                       // mutual
  if (lp != 0) return false;                        // chain
  if (l == -1) return row_lean(p - 1, H) != +1;     // p = y-1 is exact: its lower neighbour has the first call on it
  return true;
}
__device__ __forceinline__ PairRole pair_role(int y, int H, int& partner) {
  partner = y;
  const int l = row_lean(y, H);
  if (l != 0) {
    partner = y + l;
    if (leads(y, H)) return kLeader;
    return (row_lean(partner, H) == -l && leads(partner, H)) ? kAbsorbed : kSingle;  // mutual: the other one leads
  }
  if (row_lean(y - 1, H) == +1 && leads(y - 1, H)) { partner = y - 1; return kAbsorbed; }
  if (row_lean(y + 1, H) == -1 && leads(y + 1, H)) { partner = y + 1; return kAbsorbed; }
  return kSingle;
}

// Weights of the pair (leader y, partner p) on the two source rows: target y = a0*R_y + b0*R_p, target p = a1*R_p + b1*R_y
struct PairW {
  float a0, b0, a1, b1;
};
__device__ __forceinline__ PairW pair_weights(int y, int p, int H) {
  PairW w;
  const RowSel ry = make_row_sel(y, H), rp = make_row_sel(p, H);
  w.a0 = (ry.yA == y) ? ry.wA : ry.wB;
  w.b0 = (ry.yA == y) ? ry.wB : ry.wA;
  if (rp.nrows == 2) {  // mutual lean
    w.a1 = (rp.yA == p) ? rp.wA : rp.wB;
    w.b1 = (rp.yA == p) ? rp.wB : rp.wA;
  } else {
    w.a1 = rp.wA;  // exact row: 1
    w.b1 = 0.0f;
  }
  return w;
}

// ---- host mirror (launch planning only: which rows go together, in which order) ----------------------------------------
// make_row_sel on the host, operation by operation in fp32 (volatile: no contraction, no excess precision).  The kernels never
// TRUST it for correctness: a table built from it says which rows a workgroup serves, and the device re-derives every footprint.
struct HostRowSel { int nrows, yA, yB; float wA, wB, wy_main; };
inline HostRowSel host_row_sel(int y, int H) {
  volatile float hm1 = (float)(H - 1);
  volatile float q = (float)y / hm1;
  volatile float h = q - 0.5f;
  volatile float g = h * 2.0f;
  volatile float sv = g + 1.0f;
  volatile float hh = sv * 0.5f;
  volatile float iy = hh * hm1;
  const float yf = floorf(iy);
  volatile float yf1 = yf + 1.0f;
  volatile float wy0 = yf1 - iy, wy1 = iy - yf;
  const bool use0 = yf >= 0.0f && yf <= hm1 && wy0 != 0.0f, use1 = yf1 >= 0.0f && yf1 <= hm1 && wy1 != 0.0f;
  const int y0 = (int)yf;
  HostRowSel r;
  r.nrows = (int)use0 + (int)use1;
  r.yA = use0 ? y0 : y0 + 1;
  r.wA = use0 ? wy0 : (use1 ? wy1 : 0.0f);
  r.yB = y0 + 1;
  r.wB = wy1;
  if (r.nrows == 0) r.yA = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
  r.wy_main = (y0 == y) ? wy0 : ((y0 + 1 == y) ? wy1 : 0.0f);
  return r;
}

struct ColTap {    // horizontal footprint of one target pixel on one plane
  int x0;          // floor(ix)
  float w0, w1;    // torch's weights (x1 - ix), (ix - x0)
};

// ix = unnormalise(normalise(px)) of the reference, bit for bit, in 7 operations:
//   reference:  q = px/(W-1);  g = (q - 0.5)*2;            [trainer.py:550-552]
//               ix = ((g + 1)/2) * (W-1)                    [grid_sample, align_corners=True]
//   (g + 1)/2 = fl(2h + 1)/2 with h = fl(q - 0.5); scaling by 2 commutes with rounding, so it equals fl(h + 0.5).
// The ONE chain: every row kernel's ix goes through here (contraction off: each operation rounds on its own).
__device__ __forceinline__ float reference_ix(float px, float Wm1, float rcpWm1) {
#pragma clang fp contract(off)
  const float q = div_by(px, Wm1, rcpWm1);
  const float h = q - 0.5f;
  const float hh = h + 0.5f;
  return hh * Wm1;
}
// ix for target column xtf (an integer-valued float) under the shift sd; the sum rounds on its own as well
__device__ __forceinline__ float stream_ix(float xtf, float sd, float Wm1, float rcpWm1) {
#pragma clang fp contract(off)
  const float px = xtf + sd;
  return reference_ix(px, Wm1, rcpWm1);
}
// |px| <= 2W+2 by construction (the per-plane shift is clamped to +-(W+2), clamp_shift), so floor(ix) converts to int without
// saturating and x0*4 cannot alias into the row.
__device__ __forceinline__ ColTap make_col_tap(float px, float Wm1, float rcpWm1) {
  ColTap t;
  const float ix = reference_ix(px, Wm1, rcpWm1);
  const float xf = floorf(ix);
  t.w0 = (xf + 1.0f) - ix;
  t.w1 = ix - xf;
  t.x0 = (int)xf;
  return t;
}

// ---- a plane's shift along the row ---------------------------------------------------------------------------------------
// sd = sign * disparity, clamped to +-(W+2): beyond +-(W+1) nothing is in view either way.  NaN -> +lim.  `masked` (PD_MASK_ROWS: a
// masked plane samples as all-zero features, trainer.py:580 — exactly what a plane shifted out of view does, every tap being
// outside the row) overrides the shift with +lim.
__device__ __forceinline__ float clamp_shift(float sd, int W, bool masked) {
  const float lim = (float)(W + 2);
  return (!masked && sd >= -lim && sd <= lim) ? sd : ((sd < 0.0f && !masked) ? -lim : lim);
}

// frac(s*d) closer than this to an integer: the plane takes the general path of the kernels that pair target xt with source
// column xt + floor(s*d).  Worst-case error of the coordinate chain against exact arithmetic: fl(x + sd) <= ulp(2W)/2, the
// division, the two additions and the product by W-1 each <= ulp(.)/2 scaled by W-1 — 5.4e-7 * W in total (3.1e-4 at W = 640);
// the threshold keeps a factor of 2.4-3 up to W = 4096 (NOTEBOOK.md 3.6.3).
__device__ __forceinline__ float irregular_tol(int W) { return 2.5e-4f + 1.25e-6f * (float)W; }

struct ShiftClass {
  int k;         // floor(sd): the left tap of target xt is source column xt + k
  bool irr;      // in view and within irregular_tol of an integer
  bool inview;   // |sd| < W + 1
};
// (fills `c` in place: returned by value, the same function cost the post-process's segment and chain kernels 3-8 VGPRs each,
// four of them an occupancy step — profiles/row_layer_refactor_ab.md)
__device__ __forceinline__ void classify_shift(float sd, int W, ShiftClass& c) {
  const float fl = floorf(sd), fr = sd - fl;
  c.k = (int)fl;
  const float tol = irregular_tol(W);
  const bool inview = fabsf(sd) < (float)(W + 1);
  const bool irr = inview && (fr < tol || fr > 1.0f - tol);
  c.irr = irr;
  c.inview = inview;
}
// The stream kernels keep a plane's shift in LDS as (bits of sd, 2k + irr) — integers: a float-typed slot may flush a denormal.
__device__ __forceinline__ int2 pack_shift(float sd, const ShiftClass& c) { return make_int2(__float_as_int(sd), c.k * 2 + (c.irr ? 1 : 0)); }
__device__ __forceinline__ float packed_sd(int bits) { return __int_as_float(bits); }
__device__ __forceinline__ int packed_k(int kk) { return kk >> 1; }
__device__ __forceinline__ bool packed_irr(int kk) { return kk & 1; }

}  // namespace pd
