// The fp64 3x3 chain of a plane's homography (reference layers.py:206-219), shared by the kernels that form matrices on the
// device: pd_homography_matrices.hip (training: H_t2s, R n, their adjoint) and pd_render_poses.hip (inference: the per-(view,
// plane) records of a render at arbitrary poses).  One text, so that both write the same bits for the same plane and pose.
#pragma once
#include "pd_common.h"

namespace pd {

struct M3 {
  double m[3][3];
};

__device__ __forceinline__ M3 mul3(const M3& a, const M3& b) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return c;
}

__device__ __forceinline__ M3 transpose3(const M3& a) {
  M3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.m[i][j] = a.m[j][i];
  return c;
}

// adjugate / determinant in fp64: cond(H) ~ 1e3..1e4 here, far inside what 53 bits carry.  A singular matrix yields
// inf / nan entries (torch.inverse raises instead; the sweep then masks nothing sensible either way).
__device__ __forceinline__ M3 inverse3(const M3& a) {
  M3 c;
  const double c00 = a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1];
  const double c01 = a.m[1][2] * a.m[2][0] - a.m[1][0] * a.m[2][2];
  const double c02 = a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0];
  const double det = a.m[0][0] * c00 + a.m[0][1] * c01 + a.m[0][2] * c02;
  const double r = 1.0 / det;
  c.m[0][0] = c00 * r;
  c.m[1][0] = c01 * r;
  c.m[2][0] = c02 * r;
  c.m[0][1] = (a.m[0][2] * a.m[2][1] - a.m[0][1] * a.m[2][2]) * r;
  c.m[1][1] = (a.m[0][0] * a.m[2][2] - a.m[0][2] * a.m[2][0]) * r;
  c.m[2][1] = (a.m[0][1] * a.m[2][0] - a.m[0][0] * a.m[2][1]) * r;
  c.m[0][2] = (a.m[0][1] * a.m[1][2] - a.m[0][2] * a.m[1][1]) * r;
  c.m[1][2] = (a.m[0][2] * a.m[1][0] - a.m[0][0] * a.m[1][2]) * r;
  c.m[2][2] = (a.m[0][0] * a.m[1][1] - a.m[0][1] * a.m[1][0]) * r;
  return c;
}

__device__ __forceinline__ M3 load3_from44(const float* __restrict__ p) {   // the upper-left 3x3 of a [4,4] matrix
  M3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.m[i][j] = (double)p[i * 4 + j];
  return c;
}

struct PlaneOf {   // (n, d) of a homography slot
  double n[3], d;
};

struct Chain {
  M3 K, Ki, H;      // intrinsics, their inverse as handed over, H_t2s
  double t[3];
};

// T, K, inv_K: the [4,4] matrices of this pose and image
__device__ __forceinline__ Chain homography_chain_at(const float* __restrict__ T, const float* __restrict__ K,
                                                     const float* __restrict__ inv_K, const PlaneOf& p) {
  Chain c;
  c.K = load3_from44(K);
  c.Ki = load3_from44(inv_K);
  M3 M = load3_from44(T);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    c.t[i] = (double)T[i * 4 + 3];
#pragma unroll
    for (int j = 0; j < 3; ++j) M.m[i][j] += c.t[i] * p.n[j] / p.d;   // layers.py:216
  }
  c.H = inverse3(mul3(c.K, mul3(M, c.Ki)));                            // layers.py:218-219
  return c;
}

// one pose per image: T, K, inv_K are [B,4,4]
__device__ __forceinline__ Chain homography_chain(const float* __restrict__ T, const float* __restrict__ K,
                                                  const float* __restrict__ inv_K, int b, const PlaneOf& p) {
  return homography_chain_at(T + (long)b * 16, K + (long)b * 16, inv_K + (long)b * 16, p);
}

// R n of plane k under the pose T [4,4] (layers.py:223), each component summed in fp64 and rounded once
__device__ __forceinline__ void rotated_normal(const float* __restrict__ T, const float* __restrict__ norm, long k, float (&rn)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) s += (double)T[i * 4 + q] * (double)norm[k * 3 + q];
    rn[i] = (float)s;
  }
}

}  // namespace pd
