// The pose path in front of the plane-uniform sweeps, from the pose decoder's last conv output to Rt (reference
// networks/pose_net.py:148-155, layers.py:17-92, trainer.py:386-400):
//   v = scale * mean_hw(x[b, 6 frame .. 6 frame + 6])        axisangle = v[0:3], translation = v[3:6]
//   R = rot_from_axisangle(axisangle)  (axis = vec / (|vec| + 1e-7), NOT renormalised);  invert: R <- R^T
//   Rc = [[1,0,a],[0,1,b],[0,0,f]] from four corner reads of the grid;  Rt_Rc[:3,:3] = Rc R Rc^-1, everything else 0
// and its adjoint, as ONE launch each instead of ~50 torch operators a frame and a rocSOLVER inverse (which cannot be
// captured in a HIP graph).  As in pd_homography_matrices.hip the cost is launch latency, not arithmetic: everything,
// the hw accumulation included, is evaluated in fp64 and rounded once.
//
// One workgroup per image.  The hw positions of the six channels are summed by the lanes (kBlock apart), across each
// wave by a butterfly and across the waves through LDS in wave order: no atomics, the same bits on every call.  The 3x3
// chain is a few hundred flops and runs on lane 0; the backward then spreads the six channel gradients over g_x.
#include "pd_common.h"

namespace pd {

constexpr int kWaves = kBlock / kWave;
constexpr double kFocalX = 2 * 0.58, kFocalY = 2 * 1.92;   // trainer.py:391

template <class T> __device__ __forceinline__ double load_elem(const void* p, long i);
template <> __device__ __forceinline__ double load_elem<float>(const void* p, long i) {
  return (double)static_cast<const float*>(p)[i];
}
template <> __device__ __forceinline__ double load_elem<Bf16>(const void* p, long i) {
  return (double)__uint_as_float((unsigned)static_cast<const Bf16*>(p)[i] << 16);
}

__device__ __forceinline__ void store_elem(float* p, long i, double v) { p[i] = (float)v; }
// fp64 -> bf16 with ONE rounding to nearest even: through the fp32 value rounded to odd (truncated toward zero, last bit set when
// inexact), whose 16 spare bits keep the second rounding from seeing a false tie.  NaN stays NaN.
__device__ __forceinline__ void store_elem(Bf16* p, long i, double v) {
  const float f = (float)v;
  unsigned u = __float_as_uint(f);
  if (v == v && (double)f != v) {
    if (fabs((double)f) > fabs(v)) u -= 1u;
    u |= 1u;
  }
  p[i] = (Bf16)((u & 0x7FFFFFFFu) > 0x7F800000u ? (u >> 16) | 0x40u : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

struct PoseIn {         // what both directions read
  const void* x;        // [B, C, hw] through strides, or NULL (COLMAP mode: Rt instead)
  long x_sb, x_sc, x_ss;
  const float* Rt;      // [B,4,4]
  const float* grid;    // [B,2,gH,gW] through strides
  long g_sb, g_sc, g_sh, g_sw;
  int gH, gW, nch, hw, frame, invert;   // nch: channels read per image, 6 or (axis-angle only) 3
  double scale;
};

struct M3d {
  double m[3][3];
};

__device__ __forceinline__ M3d mul3(const M3d& a, const M3d& b) {
  M3d c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return c;
}

__device__ __forceinline__ M3d transpose3(const M3d& a) {
  M3d c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[j][i];
  return c;
}

// scale * mean over hw of the image's nch channels, in every lane.  red: kWaves * 6 doubles of LDS.
template <class T>
__device__ __forceinline__ void channel_means(const PoseIn& in, int b, double* red, double (&v)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = 0.0;
  const long base = (long)b * in.x_sb + (long)in.frame * 6 * in.x_sc;
  for (int i = threadIdx.x; i < in.hw; i += kBlock) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k < in.nch) v[k] += load_elem<T>(in.x, base + k * in.x_sc + i * in.x_ss);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[(threadIdx.x / kWave) * 6 + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double s = red[k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += red[w * 6 + k];
    v[k] = s / (double)in.hw * in.scale;
  }
}

struct Rot {
  double x, y, z, angle, d, sa, ca, C;   // axis = vec / d, d = angle + 1e-7
  M3d R;                                 // layers.py:81-89, before the transpose of `invert`
};

__device__ __forceinline__ Rot rotation(const double (&v)[6]) {
  Rot r;
  r.angle = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  r.d = r.angle + 1e-7;
  r.x = v[0] / r.d, r.y = v[1] / r.d, r.z = v[2] / r.d;
  r.ca = cos(r.angle), r.sa = sin(r.angle);
  r.C = 1.0 - r.ca;
  const double xs = r.x * r.sa, ys = r.y * r.sa, zs = r.z * r.sa;
  const double xC = r.x * r.C, yC = r.y * r.C, zC = r.z * r.C;
  const double xyC = r.x * yC, yzC = r.y * zC, zxC = r.z * xC;
  r.R.m[0][0] = r.x * xC + r.ca, r.R.m[0][1] = xyC - zs, r.R.m[0][2] = zxC + ys;
  r.R.m[1][0] = xyC + zs, r.R.m[1][1] = r.y * yC + r.ca, r.R.m[1][2] = yzC - xs;
  r.R.m[2][0] = zxC - ys, r.R.m[2][1] = yzC + xs, r.R.m[2][2] = r.z * zC + r.ca;
  return r;
}

struct Conj {
  M3d Rc, Rci;
};

__device__ __forceinline__ Conj grid_conjugation(const PoseIn& in, int b) {   // trainer.py:388-394, Rc^-1 in closed form
  const float* g = in.grid + (long)b * in.g_sb;
  const double x00 = (double)g[0], x0w = (double)g[(long)(in.gW - 1) * in.g_sw];
  const double y00 = (double)g[in.g_sc], yh0 = (double)g[in.g_sc + (long)(in.gH - 1) * in.g_sh];
  const double gx0 = (x0w + x00) / 2.0, gy0 = (yh0 + y00) / 2.0, f = (x0w - x00) / 2.0;
  const double a = -gx0 / kFocalX, bb = -gy0 / kFocalY;
  Conj c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.Rc.m[i][j] = c.Rci.m[i][j] = (i == j) ? 1.0 : 0.0;
  c.Rc.m[0][2] = a, c.Rc.m[1][2] = bb, c.Rc.m[2][2] = f;
  c.Rci.m[0][2] = -a / f, c.Rci.m[1][2] = -bb / f, c.Rci.m[2][2] = 1.0 / f;
  return c;
}

template <class T>
__global__ __launch_bounds__(kBlock) void pose_tail_fwd_kernel(PoseIn in, float* __restrict__ axisangle,
                                                               float* __restrict__ translation, float* __restrict__ Rc,
                                                               float* __restrict__ Rt_Rc) {
  __shared__ double red[kWaves * 6];
  const int b = blockIdx.x;
  double v[6];
  if (in.x) channel_means<T>(in, b, red, v);
  if (threadIdx.x != 0) return;
  const Conj c = grid_conjugation(in, b);
  M3d R;
  double t[3] = {0.0, 0.0, 0.0};   // reaches Rt_Rc in COLMAP mode only (trainer.py:397-398)
  if (in.x) {
    R = rotation(v).R;
    if (in.invert) R = transpose3(R);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (axisangle) axisangle[(long)b * 3 + k] = (float)v[k];
      if (translation) translation[(long)b * 3 + k] = (float)v[3 + k];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R.m[i][j] = (double)in.Rt[(long)b * 16 + i * 4 + j];
      t[i] = (double)in.Rt[(long)b * 16 + i * 4 + 3];
    }
  }
  if (Rc) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rc[(long)b * 9 + i * 3 + j] = (float)c.Rc.m[i][j];
  }
  if (!Rt_Rc) return;
  const M3d M = mul3(c.Rc, mul3(R, c.Rci));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Rt_Rc[(long)b * 16 + i * 4 + j] = (float)M.m[i][j];
    Rt_Rc[(long)b * 16 + i * 4 + 3] = (float)(c.Rc.m[i][0] * t[0] + c.Rc.m[i][1] * t[1] + c.Rc.m[i][2] * t[2]);
    Rt_Rc[(long)b * 16 + 12 + i] = 0.0f;
  }
  Rt_Rc[(long)b * 16 + 15] = 0.0f;   // the reference fills a zeros_like: [3,3] is 0, not 1
}

// Adjoint.  M = Rc R' Rc^-1 -> gR' = Rc^T gM Rc^-T;  R' = R^T under invert -> gR = gR'^T;  R(axis, sa, ca, C) -> the
// gradients of axis, sin, cos;  axis = vec / d, d = angle + 1e-7, angle = |vec| with d angle / d vec = vec / angle, taken as 0
// at angle = 0 (torch's norm backward) -> g_vec;  v = scale / hw * sum x -> every position of a channel gets scale / hw * g_v.
template <class T>
__global__ __launch_bounds__(kBlock) void pose_tail_bwd_kernel(PoseIn in, int C, const float* __restrict__ g_Rt_Rc,
                                                               const float* __restrict__ g_axisangle,
                                                               const float* __restrict__ g_translation,
                                                               T* __restrict__ g_x, long gx_sb, long gx_sc, long gx_ss) {
  __shared__ double red[kWaves * 6 + 6];
  const int b = blockIdx.x;
  double v[6];
  channel_means<T>(in, b, red, v);
  double* gch = red + kWaves * 6;   // the six channel gradients, already times scale / hw
  if (threadIdx.x == 0) {
    double gv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (g_Rt_Rc) {
      const Conj c = grid_conjugation(in, b);
      const Rot r = rotation(v);
      M3d gM;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) gM.m[i][j] = (double)g_Rt_Rc[(long)b * 16 + i * 4 + j];
      M3d G = mul3(transpose3(c.Rc), mul3(gM, transpose3(c.Rci)));
      if (in.invert) G = transpose3(G);
      const double s01 = G.m[0][1] + G.m[1][0], s02 = G.m[0][2] + G.m[2][0], s12 = G.m[1][2] + G.m[2][1];
      const double xC = r.x * r.C, yC = r.y * r.C, zC = r.z * r.C;
      const double gax = 2.0 * xC * G.m[0][0] + yC * s01 + zC * s02 + r.sa * (G.m[2][1] - G.m[1][2]);
      const double gay = xC * s01 + 2.0 * yC * G.m[1][1] + zC * s12 + r.sa * (G.m[0][2] - G.m[2][0]);
      const double gaz = xC * s02 + yC * s12 + 2.0 * zC * G.m[2][2] + r.sa * (G.m[1][0] - G.m[0][1]);
      const double gC = r.x * r.x * G.m[0][0] + r.y * r.y * G.m[1][1] + r.z * r.z * G.m[2][2] + r.x * r.y * s01 +
                        r.z * r.x * s02 + r.y * r.z * s12;
      const double gca = G.m[0][0] + G.m[1][1] + G.m[2][2] - gC;
      const double gsa = r.x * (G.m[2][1] - G.m[1][2]) + r.y * (G.m[0][2] - G.m[2][0]) + r.z * (G.m[1][0] - G.m[0][1]);
      const double g_d = -(gax * v[0] + gay * v[1] + gaz * v[2]) / (r.d * r.d);
      const double g_angle = gsa * r.ca - gca * r.sa + g_d;
      const double per = r.angle == 0.0 ? 0.0 : g_angle / r.angle;
      gv[0] = gax / r.d + per * v[0];
      gv[1] = gay / r.d + per * v[1];
      gv[2] = gaz / r.d + per * v[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (g_axisangle) gv[k] += (double)g_axisangle[(long)b * 3 + k];
      if (g_translation) gv[3 + k] = (double)g_translation[(long)b * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) gch[k] = gv[k] * in.scale / (double)in.hw;
  }
  __syncthreads();
  const int c0 = in.frame * 6, n = C * in.hw;   // (C * hw < 2^31: refused on the host otherwise)
  for (int e = threadIdx.x; e < n; e += kBlock) {
    const int c = e / in.hw, i = e - c * in.hw;
    const double g = (c >= c0 && c < c0 + in.nch) ? gch[c - c0] : 0.0;
    store_elem(g_x, (long)b * gx_sb + (long)c * gx_sc + (long)i * gx_ss, g);
  }
}

}  // namespace pd

using namespace pd;

static int pose_in(PoseIn* in, int B, int C, int hw, int frame, int dtype, int invert, double scale, const void* x,
                   int64_t x_sb, int64_t x_sc, int64_t x_ss, const float* Rt, const float* grid, int gH, int gW,
                   const int64_t* grid_strides) {
  PD_REQUIRE(B > 0, "bad shape: B = %d", B);
  PD_REQUIRE(grid && grid_strides, "null input: grid");
  PD_REQUIRE(gH > 0 && gW > 0, "bad shape: grid %d x %d", gH, gW);
  PD_REQUIRE((x != nullptr) != (Rt != nullptr), "exactly one of x and Rt (COLMAP mode) must be given");
  in->nch = 6;
  if (x) {
    PD_REQUIRE(dtype == PD_DTYPE_F32 || dtype == PD_DTYPE_BF16, "bad dtype %d: PD_DTYPE_F32 or PD_DTYPE_BF16", dtype);
    PD_REQUIRE(hw > 0, "bad shape: hw = %d", hw);
    PD_REQUIRE(C == 3 || (C > 0 && C % 6 == 0), "bad shape: C = %d is neither 6 F nor 3 (axis-angle only)", C);
    PD_REQUIRE(frame >= 0 && frame < (C == 3 ? 1 : C / 6), "frame %d out of range for C = %d", frame, C);
    PD_REQUIRE((int64_t)C * hw < ((int64_t)1 << 31), "C * hw = %lld is past the kernel's 32-bit element index",
               (long long)C * hw);
    in->nch = C == 3 ? 3 : 6;
  }
  in->x = x, in->x_sb = x_sb, in->x_sc = x_sc, in->x_ss = x_ss;
  in->Rt = Rt, in->grid = grid;
  in->g_sb = grid_strides[0], in->g_sc = grid_strides[1], in->g_sh = grid_strides[2], in->g_sw = grid_strides[3];
  in->gH = gH, in->gW = gW, in->hw = hw, in->frame = frame, in->invert = invert != 0, in->scale = scale;
  return PD_OK;
}

extern "C" int pd_pose_tail_fwd(int B, int C, int hw, int frame, int dtype, int invert, double scale, const void* x,
                                int64_t x_sb, int64_t x_sc, int64_t x_ss, const float* Rt, const float* grid, int gH,
                                int gW, const int64_t* grid_strides, float* axisangle, float* translation, float* Rc,
                                float* Rt_Rc, pd_stream_t stream) {
  PoseIn in;
  if (const int rc = pose_in(&in, B, C, hw, frame, dtype, invert, scale, x, x_sb, x_sc, x_ss, Rt, grid, gH, gW, grid_strides))
    return rc;
  PD_REQUIRE(x || (!axisangle && !translation), "COLMAP mode has no axisangle / translation output");
  PD_REQUIRE(in.nch == 6 || !translation, "C = 3 holds the axis-angle only: no translation output");
  if (x && dtype == PD_DTYPE_BF16)
    pose_tail_fwd_kernel<Bf16><<<B, kBlock, 0, (hipStream_t)stream>>>(in, axisangle, translation, Rc, Rt_Rc);
  else
    pose_tail_fwd_kernel<float><<<B, kBlock, 0, (hipStream_t)stream>>>(in, axisangle, translation, Rc, Rt_Rc);
  return check_launch("pose_tail_fwd_kernel");
}

extern "C" int pd_pose_tail_bwd(int B, int C, int hw, int frame, int dtype, int invert, double scale, const void* x,
                                int64_t x_sb, int64_t x_sc, int64_t x_ss, const float* grid, int gH, int gW,
                                const int64_t* grid_strides, const float* g_Rt_Rc, const float* g_axisangle,
                                const float* g_translation, void* g_x, int64_t gx_sb, int64_t gx_sc, int64_t gx_ss,
                                pd_stream_t stream) {
  PoseIn in;
  PD_REQUIRE(x && g_x, "null input: x / g_x (the backward has no COLMAP mode)");
  if (const int rc = pose_in(&in, B, C, hw, frame, dtype, invert, scale, x, x_sb, x_sc, x_ss, nullptr, grid, gH, gW,
                             grid_strides))
    return rc;
  PD_REQUIRE(g_Rt_Rc || g_axisangle || g_translation, "no upstream gradient");
  PD_REQUIRE(in.nch == 6 || !g_translation, "C = 3 holds the axis-angle only: no translation gradient");
  if (dtype == PD_DTYPE_BF16)
    pose_tail_bwd_kernel<Bf16><<<B, kBlock, 0, (hipStream_t)stream>>>(in, C, g_Rt_Rc, g_axisangle, g_translation,
                                                                        static_cast<Bf16*>(g_x), gx_sb, gx_sc, gx_ss);
  else
    pose_tail_bwd_kernel<float><<<B, kBlock, 0, (hipStream_t)stream>>>(in, C, g_Rt_Rc, g_axisangle, g_translation,
                                                                         static_cast<float*>(g_x), gx_sb, gx_sc, gx_ss);
  return check_launch("pose_tail_bwd_kernel");
}
