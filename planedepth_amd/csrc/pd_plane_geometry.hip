// The geometry head of DepthDecoder.forward without yz planes (reference networks/depth_decoder.py:148-207) in ROW form:
// every xy and xz plane has a disparity and a padding mask that are constant along x, so what the reference builds as dense
// [B,N,H,W] maps in ~6 elementwise passes plus two concatenations (and runs backwards through autograd) is [B,N,H]-sized
// information.  One launch each way:
//   fwd   residual [B,N] (may be NULL), grid [B,2,H,W] -> disp_rows, mask_rows [B,N,H], distance [B,N], norm [B,N,3]
//   bwd   g_disp_rows [B,N,H], g_distance [B,N] -> g_residual [B,N]
// Of the grid only column 0 of the y channel, columns 0 and W-1 of the x channel and four corner elements are read: the y
// channel is taken to be constant along x (every grid datasets/pair_transforms.py makes is; the Python layer checks it under
// PD_CHECK_CONTRACT).  Arithmetic: fp32 in the reference's operation order with contraction off, as pd_plane_levels
// (pd_batch.hip) does for :153-154 — Python-float constants are rounded to fp32 once, where torch rounds them.
// The backward's sum over H is one wave per (image, plane), lanes striding the rows, then a butterfly: a fixed order.
#include "pd_common.h"

namespace pd {

struct PlaneGeomArgs {
  int B, NL, NX, H, W;      // NL = no_levels, NX = xz_levels
  float base, disp_max, nl_m1, dist_num;   // (float)(disp_min / disp_max), no_levels - 1, 0.1 * 0.58 * W
  float xz_min, xz_span, nx_m1;            // (float)(xz_max - xz_min), xz_levels - 1
  float half_h, h_fy;                      // (float)(H / 2), (float)(H * 1.92)   (:200)
};

// height of ground plane m (:159-163)
__device__ __forceinline__ float xz_height(const PlaneGeomArgs& a, int m, float res) {
#pragma clang fp contract(off)
  const float gl = (float)m + res;
  const float t = a.xz_span * gl;
  return a.xz_min + t / a.nx_m1;
}

// 1 / sqrt(1 + t^2) and t = (py - H/2) / (H * 1.92 * fs) of image b (:197-202)
__device__ __forceinline__ float xz_normalize(const PlaneGeomArgs& a, const float* __restrict__ g, float& t) {
#pragma clang fp contract(off)
  const long HW = (long)a.H * a.W;
  const float gyc = (g[HW + (long)(a.H - 1) * a.W] + g[HW]) / 2.0f;
  const float py = (gyc + 1.0f) * (float)a.H / 2.0f;
  const float fs = (g[a.W - 1] - g[0]) / 2.0f;
  t = (py - a.half_h) / (a.h_fy * fs);
  return 1.0f / sqrtf(1.0f + t * t);
}

__global__ __launch_bounds__(kBlock) void plane_geometry_fwd_kernel(PlaneGeomArgs a, const float* __restrict__ residual,
                                                                    const float* __restrict__ grid,
                                                                    float* __restrict__ disp_rows, float* __restrict__ mask_rows,
                                                                    float* __restrict__ distance, float* __restrict__ norm) {
#pragma clang fp contract(off)
  const int N = a.NL + a.NX;
  const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long)a.B * N * a.H) return;
  const int y = (int)(idx % a.H);
  const int bn = (int)(idx / a.H), n = bn % N, b = bn / N;
  const float res = residual ? residual[bn] : 0.0f;
  const float* g = grid + (long)b * 2 * a.H * a.W;
  float d, mk = 1.0f, dist, n1 = 0.0f, n2 = 1.0f;
  if (n < a.NL) {
    const float e = ((float)n + res) / a.nl_m1;           // :152-153
    d = a.disp_max * powf(a.base, e);
    dist = a.dist_num / d;                                // :154
  } else {
    const float h = xz_height(a, n - a.NL, res);
    const float yv = g[(long)a.H * a.W + (long)y * a.W];  // grid[b,1,y,0]
    mk = (yv >= 1e-7f) ? 1.0f : 0.0f;                     // :168
    const float yc = (yv < 1e-7f) ? 1e-7f : yv;           // :170
    float gr = h * 1.92f / (yc / 2.0f);                   // :171
    gr = (g[(long)y * a.W + a.W - 1] - g[(long)y * a.W]) / 2.0f * gr;   // :172
    d = a.dist_num / gr;                                  // :181
    float t;
    const float inv = xz_normalize(a, g, t);
    n1 = 1.0f * inv; n2 = t * inv;                        // :201-203
    dist = h * inv;                                       // :204
  }
  disp_rows[idx] = d;
  if (mask_rows) mask_rows[idx] = mk;
  if (y == 0) {
    if (distance) distance[bn] = dist;
    if (norm) {
      norm[(long)bn * 3 + 0] = 0.0f;
      norm[(long)bn * 3 + 1] = n1;
      norm[(long)bn * 3 + 2] = n2;
    }
  }
}

// xy: d disp / d level = disp ln(base) / (no_levels - 1), d distance / d disp = -dist_num / disp^2 (pd_plane_levels_bwd), the
//     row gradients add up (the rows are one scalar).
// xz: disp[y] = c[y] / h, so d disp[y] / d h = -disp[y] / h; distance = h / |.|; d h / d level = (xz_max - xz_min) / (xz_levels - 1).
//     (The clamp of y and the mask touch the grid only: no gate on the way to h, as in the reference's autograd.)
__global__ __launch_bounds__(kBlock) void plane_geometry_bwd_kernel(PlaneGeomArgs a, float ln_base,
                                                                    const float* __restrict__ residual,
                                                                    const float* __restrict__ grid,
                                                                    const float* __restrict__ disp_rows,
                                                                    const float* __restrict__ g_disp_rows,
                                                                    const float* __restrict__ g_distance,
                                                                    float* __restrict__ g_residual) {
  const int N = a.NL + a.NX;
  const int lane = threadIdx.x & (kWave - 1);
  const int bn = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;   // one wave per (image, plane)
  if (bn >= a.B * N) return;
  const int n = bn % N, b = bn / N;
  const bool xy = n < a.NL;
  const float* d = disp_rows + (long)bn * a.H;
  float s = 0.0f;   // xy: sum_y g[y];  xz: sum_y g[y] * disp[y]
  if (g_disp_rows) {
    const float* gd = g_disp_rows + (long)bn * a.H;
    for (int y = lane; y < a.H; y += kWave) s += xy ? gd[y] : gd[y] * d[y];
  }
  s = wave_sum(s);
  if (lane != 0) return;
  const float gdist = g_distance ? g_distance[bn] : 0.0f;
  float g;
  if (xy) {
    const float d0 = d[0];
    g = (s - gdist * a.dist_num / (d0 * d0)) * d0 * ln_base / a.nl_m1;
  } else {
    const float h = xz_height(a, n - a.NL, residual[bn]);
    float t;
    const float inv = xz_normalize(a, grid + (long)b * 2 * a.H * a.W, t);
    g = (gdist * inv - s / h) * a.xz_span / a.nx_m1;
  }
  g_residual[bn] = g;
}

static int plane_geometry_args(PlaneGeomArgs* a, int B, int no_levels, int xz_levels, int H, int W, int flags, float disp_min,
                               float disp_max, float xz_min, float xz_max) {
  PD_REQUIRE(flags == 0, "unknown flags");
  PD_REQUIRE(B > 0 && H > 0 && W > 0, "bad shape");
  PD_REQUIRE(no_levels >= 2, "no_levels must be at least 2 (the reference divides by no_levels - 1)");
  PD_REQUIRE(xz_levels == 0 || xz_levels >= 2, "xz_levels must be 0 or at least 2 (the reference divides by xz_levels - 1)");
  PD_REQUIRE(disp_min > 0.0f && disp_max > 0.0f, "bad arguments");
  PD_REQUIRE((long)B * (no_levels + xz_levels) * H < (1L << 31) && (long)H * W < (1L << 30), "shape too large");
  a->B = B; a->NL = no_levels; a->NX = xz_levels; a->H = H; a->W = W;
  a->base = (float)((double)disp_min / (double)disp_max);   // the reference's Python-float quotient, rounded once
  a->disp_max = disp_max;
  a->nl_m1 = (float)(no_levels - 1);
  a->dist_num = (float)(0.1 * 0.58 * (double)W);
  a->xz_min = xz_min;
  a->xz_span = (float)((double)xz_max - (double)xz_min);
  a->nx_m1 = (float)(xz_levels - 1);
  a->half_h = (float)((double)H / 2.0);
  a->h_fy = (float)((double)H * 1.92);
  return 0;
}

}  // namespace pd

using namespace pd;

extern "C" int pd_plane_geometry_fwd(int B, int no_levels, int xz_levels, int H, int W, int flags, float disp_min,
                                     float disp_max, float xz_min, float xz_max, const float* residual, const float* grid,
                                     float* disp_rows, float* mask_rows, float* distance, float* norm, pd_stream_t stream) {
  PlaneGeomArgs a;
  if (int rc = plane_geometry_args(&a, B, no_levels, xz_levels, H, W, flags, disp_min, disp_max, xz_min, xz_max)) return rc;
  PD_REQUIRE(disp_rows && (grid || xz_levels == 0), "NULL pointer");
  const long total = (long)B * (no_levels + xz_levels) * H;
  plane_geometry_fwd_kernel<<<(unsigned)((total + kBlock - 1) / kBlock), kBlock, 0, (hipStream_t)stream>>>(
      a, residual, grid, disp_rows, mask_rows, distance, norm);
  return check_launch("plane_geometry_fwd_kernel");
}

extern "C" int pd_plane_geometry_bwd(int B, int no_levels, int xz_levels, int H, int W, int flags, float disp_min,
                                     float disp_max, float xz_min, float xz_max, const float* residual, const float* grid,
                                     const float* disp_rows, const float* g_disp_rows, const float* g_distance,
                                     float* g_residual, pd_stream_t stream) {
  PlaneGeomArgs a;
  if (int rc = plane_geometry_args(&a, B, no_levels, xz_levels, H, W, flags, disp_min, disp_max, xz_min, xz_max)) return rc;
  PD_REQUIRE(residual && disp_rows && g_residual && (grid || xz_levels == 0), "NULL pointer");
  PD_REQUIRE(g_disp_rows || g_distance, "NULL pointer: no upstream gradient");
  const int waves = B * (no_levels + xz_levels);
  plane_geometry_bwd_kernel<<<ceil_div(waves, kBlock / kWave), kBlock, 0, (hipStream_t)stream>>>(
      a, logf(a.base), residual, grid, disp_rows, g_disp_rows, g_distance, g_residual);
  return check_launch("plane_geometry_bwd_kernel");
}
