// Per-(pixel, plane) sampling geometry of the general sweep kernels (pd_plane_sweep.hip; the tile kernel that shared it is
// archived under docs/archive/), and the geometry pieces they share with the plane-uniform and gather kernels: the gradient
// of a homography's entries, the inverse matrix of the backward's gathers.
#pragma once
#include "pd_sweep.h"

namespace pd {

// ---------------------------------------------------------------------------------------------------------------
// Sampling position of target pixel (x,y) on plane n of image b, plus the padding mask.
// DISP:        trainer.py:540-554   (x + sign*d, y) normalised by (W-1, H-1)
// HOMOGRAPHY:  layers.py:221-233    p = H_t2s [x,y,1]; mask = ((K^-1 p_t).(R n) > 0) & (z > 1e-7); z<1e-7 -> 1e-7
// ---------------------------------------------------------------------------------------------------------------
struct PlaneGeom {   // per (pixel, plane) state needed again for the grid gradient
  float ix, iy;
  float p0, p1, zc;  // homography only
  bool z_clamped;
};

// Sizes the coordinates are normalised by, with their refined reciprocals (uniform; computed once per thread).
struct CoordNorm {
  float Wm1, Hm1, rcpW, rcpH;
  bool fast;  // sizes >= 2: the reciprocal form is exact (a size of 1 divides by zero; keep IEEE semantics there)
};
__device__ __forceinline__ CoordNorm make_coord_norm(int W, int H) {
  CoordNorm c;
  c.Wm1 = (float)(W - 1); c.Hm1 = (float)(H - 1);
  c.fast = (W >= 2) && (H >= 2);
  c.rcpW = c.fast ? refined_rcp(c.Wm1) : 0.0f;
  c.rcpH = c.fast ? refined_rcp(c.Hm1) : 0.0f;
  return c;
}

template <int MODE>
__device__ __forceinline__ PlaneGeom plane_coords(const SweepArgs& a, const CoordNorm& cn, int b, int n, int x, int y,
                                                  float iy_disp, bool& mask) {
  PlaneGeom g;
  if (MODE == PD_WARP_DISP) {
    float d;
    if (a.flags & PD_DISP_DENSE)
      d = a.plane[(((long)b * a.N + n) * a.H + y) * a.W + x];
    else
      d = a.plane[b * a.N + n];
    g.ix = normalise_roundtrip((float)x + a.sign * d, (float)(a.W - 1));
    g.iy = iy_disp;
    g.p0 = g.p1 = g.zc = 0.0f;
    g.z_clamped = false;
    mask = true;  // caller applies the padding_mask tensor
  } else {
    const float* Hm = a.plane + ((long)b * a.N + n) * 9;
    const float* Rn = a.plane_aux + ((long)b * a.N + n) * 3;
    const float* Ki = a.inv_K3 + (long)b * 9;
    const float fx = (float)x, fy = (float)y;
    g.p0 = hrow_dot(Hm[0], Hm[1], Hm[2], fx, fy);
    g.p1 = hrow_dot(Hm[3], Hm[4], Hm[5], fx, fy);
    const float z = hrow_dot(Hm[6], Hm[7], Hm[8], fx, fy);
    const float r0 = hrow_dot(Ki[0], Ki[1], Ki[2], fx, fy);
    const float r1 = hrow_dot(Ki[3], Ki[4], Ki[5], fx, fy);
    const float r2 = hrow_dot(Ki[6], Ki[7], Ki[8], fx, fy);
    const float facing = facing_dot(r0, r1, r2, Rn[0], Rn[1], Rn[2]);
    mask = (facing > 0.0f) && (z > kZMin);
    g.z_clamped = (z < kZMin);
    g.zc = g.z_clamped ? kZMin : z;
    if (cn.fast) {  // uniform
      g.ix = normalise_roundtrip_rcp(g.p0 / g.zc, cn.Wm1, cn.rcpW);
      g.iy = normalise_roundtrip_rcp(g.p1 / g.zc, cn.Hm1, cn.rcpH);
    } else {
      g.ix = normalise_roundtrip(g.p0 / g.zc, cn.Wm1);
      g.iy = normalise_roundtrip(g.p1 / g.zc, cn.Hm1);
    }
  }
  return g;
}

// ---- backward: from d loss / d (ix, iy) in pixels to the gradient of a homography's nine entries ------------------------
// Back through grid_sample's un-normalisation ((size-1)/2) and the reference's normalisation (*2, /(size-1)) in autograd's
// order (gradient side, no bit-exactness at stake).
__device__ __forceinline__ float grid_grad_scale(int size) { return (float)(size - 1) / 2 * 2.0f / (float)(size - 1); }

// gpx, gpy: d loss / d (p0 / zc, p1 / zc), i.e. the pixel gradients times grid_grad_scale; inv_z = refined_rcp(zc), handed in
// (the plane-uniform first pass computes it once per pixel, inside its image guard).
__device__ __forceinline__ void homography_grad9(float gpx, float gpy, float inv_z, float p0, float p1, bool z_clamped, float fx,
                                                 float fy, float (&gk)[9]) {
  const float gp0 = gpx * inv_z, gp1 = gpy * inv_z;
  const float gz = z_clamped ? 0.0f : -(gp0 * p0 + gp1 * p1) * inv_z;
  gk[0] = gp0 * fx; gk[1] = gp0 * fy; gk[2] = gp0;
  gk[3] = gp1 * fx; gk[4] = gp1 * fy; gk[5] = gp1;
  gk[6] = gz * fx;  gk[7] = gz * fy;  gk[8] = gz;
}

// Forward homography (source -> target) of a backward's gather: the fp64 adjugate inverse of h[9], rounded to fp32.  False
// where the matrix is not finite / not invertible.
__device__ __forceinline__ bool adjugate_inverse(const float* __restrict__ h, float (&Hs)[9]) {
  const double a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7], l = h[8];
  const double A = e * l - f * k, Bc = -(d * l - f * g), C = d * k - e * g;
  const double det = a * A + b * Bc + c * C, inv = 1.0 / det;
  Hs[0] = (float)(A * inv);  Hs[1] = (float)(-(b * l - c * k) * inv); Hs[2] = (float)((b * f - c * e) * inv);
  Hs[3] = (float)(Bc * inv); Hs[4] = (float)((a * l - c * g) * inv);  Hs[5] = (float)(-(a * f - c * d) * inv);
  Hs[6] = (float)(C * inv);  Hs[7] = (float)(-(a * k - b * g) * inv); Hs[8] = (float)((a * e - b * d) * inv);
  bool ok = (det == det) && fabs(det) > 1e-30 && fabs(inv) < 1e30;
  for (int j = 0; j < 9; ++j) ok = ok && (fabsf(Hs[j]) < 1e30f) && (Hs[j] == Hs[j]);
  return ok;
}

// bilinear weight with which target sample (ix, iy) reaches source pixel (sx, sy): torch's own expressions
// (x1 - ix) / (ix - x0) for the tap that IS (sx, sy), zero when neither tap column / row is
__device__ __forceinline__ float tap_weight_on(float ix, float iy, int sx, int sy) {
  const float xf = floorf(ix), yf = floorf(iy);
  const float fsx = (float)sx, fsy = (float)sy;
  float wx = 0.0f, wy = 0.0f;
  if (xf == fsx) wx = (xf + 1.0f) - ix; else if (xf + 1.0f == fsx) wx = ix - xf;
  if (yf == fsy) wy = (yf + 1.0f) - iy; else if (yf + 1.0f == fsy) wy = iy - yf;
  return wx * wy;
}

__device__ __forceinline__ bool read_mask(const SweepArgs& a, int b, int n, int x, int y) {
  return a.padding_mask[(((long)b * a.N + n) * a.H + y) * a.W + x] != 0.0f;
}

}  // namespace pd
