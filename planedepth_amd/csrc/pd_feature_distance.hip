// Perceptual feature distance (reference trainer.py:672-685), one feature level of the frozen perceptual net per call:
//   l_p = ((pred_f - target_f) ** 2).mean(1, True)
//   automask:  l_a = ((source_f - target_f) ** 2).mean(1, True);  l_p = min over cat([l_p, l_a], 1)
//   loss += l_p.mean()
// The net's convolutions stay MIOpen's; this is the elementwise-plus-reduction pass over its outputs, the largest tensors of
// the whole loss ([8,64,192,640] at the first VGG level).  Forward: 2 reads (3 with a source) of [B,C,h,w], a byte per pixel
// written; backward: 2 reads + the byte map, 1 write.  The torch chain moves at least 6 / 4 such tensors and keeps
// [B,C,h,w]-sized temporaries alive for autograd.
//
// Access shape.  The reduction runs over the channel stride h*w, so a lane owns ADJACENT pixels — 16 bytes (four fp32 or
// eight bf16) when h*w and the base addresses allow it, one pixel otherwise — and walks the channels with kFdUnroll loads
// per tensor in flight.  The four waves of a workgroup serve the SAME 64 lanes' pixels and split the channels between them
// (wave s takes c = s, s+4, ...): the 48x160 map of the third level would otherwise fill a fraction of the chip.  The four
// channel slices meet in LDS and are added in slice order.
//
// Ties.  `torch.min` over `cat([l_p, l_a], 1)` returns the first index of the minimum, so a tie selects the PREDICTION (the
// convention of pd_masked_loss.hip): the gradient flows.  Both sums are formed by the same function in the same order, so
// source_f == pred_f is a tie bit for bit, at every pixel.  The selection is written as one byte per pixel; the backward
// reads that map and never the source features.
//
// Deterministic: workgroup partial sums, finished by one wave in index order; no float atomics.
#include "pd_common.h"

namespace pd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kFdSlices = kBlock / kWave;  // channel slices of a workgroup: one per wave
constexpr int kFdUnroll = 4;               // channels per slice whose loads are issued before the first is consumed

// fp32 -> bf16, round to nearest even (a NaN stays a quiet NaN): the one rounding of a bf16 gradient element
__device__ __forceinline__ unsigned bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// How a lane reads and writes its V adjacent pixels of one channel.
struct PackF32x4 {
  typedef float elem;
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float* p, float (&o)[4]) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&o)[4]) {   // streamed: the next reader is another kernel
    const f32x4 v = {o[0], o[1], o[2], o[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
  }
};
struct PackF32x1 {
  typedef float elem;
  static constexpr int V = 1;
  static __device__ __forceinline__ void load(const float* p, float (&o)[1]) { o[0] = p[0]; }
  static __device__ __forceinline__ void store(float* p, const float (&o)[1]) { __builtin_nontemporal_store(o[0], p); }
};
struct PackBf16x8 {   // hipcc does not vectorise bf16 loads by itself: one 16-byte load, widened by shifts (exact)
  typedef uint16_t elem;
  static constexpr int V = 8;
  static __device__ __forceinline__ void load(const uint16_t* p, float (&o)[8]) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[2 * k] = __uint_as_float(v[k] << 16);
      o[2 * k + 1] = __uint_as_float(v[k] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void store(uint16_t* p, const float (&o)[8]) {
    u32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = bf16_rne(o[2 * k]) | (bf16_rne(o[2 * k + 1]) << 16);
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  }
};
struct PackBf16x1 {
  typedef uint16_t elem;
  static constexpr int V = 1;
  static __device__ __forceinline__ void load(const uint16_t* p, float (&o)[1]) { o[0] = __uint_as_float((unsigned)p[0] << 16); }
  static __device__ __forceinline__ void store(uint16_t* p, const float (&o)[1]) { p[0] = (uint16_t)bf16_rne(o[0]); }
};

// acc + (x - t)^2: the ONE accumulation step of both sums (prediction and source), so that equal inputs give equal bits
__device__ __forceinline__ float sq_acc(float x, float t, float acc) {
  const float d = x - t;
  return __builtin_fmaf(d, d, acc);
}

// grid (ceil(HW / (64 V)), B), kBlock threads.  sel [B,HW] bytes, partials [B][gridDim.x].
template <class P, bool SRC>
__global__ __launch_bounds__(kBlock) void feature_distance_fwd_kernel(int C, int HW, const typename P::elem* __restrict__ pred,
                                                                      const typename P::elem* __restrict__ tgt,
                                                                      const typename P::elem* __restrict__ src,
                                                                      uint8_t* __restrict__ sel, float* __restrict__ partials) {
  constexpr int V = P::V;
  __shared__ float red[SRC ? 2 : 1][kFdSlices - 1][V][kWave];
  const int lane = threadIdx.x & (kWave - 1), slice = threadIdx.x >> 6, b = blockIdx.y;
  const long pix = ((long)blockIdx.x * kWave + lane) * V;   // the first of this lane's V pixels (HW % V == 0: all or none inside)
  const bool live = pix < HW;
  float e[V], a[V];
#pragma unroll
  for (int v = 0; v < V; ++v) e[v] = a[v] = 0.0f;
  if (live) {
    const long base = (long)b * C * HW + pix;
    int c = slice;
    for (; c + (kFdUnroll - 1) * kFdSlices < C; c += kFdUnroll * kFdSlices) {
      float p[kFdUnroll][V], t[kFdUnroll][V], s[kFdUnroll][V];
#pragma unroll
      for (int u = 0; u < kFdUnroll; ++u) {
        const long at = base + (long)(c + u * kFdSlices) * HW;
        P::load(pred + at, p[u]);
        P::load(tgt + at, t[u]);
        if (SRC) P::load(src + at, s[u]);
      }
#pragma unroll
      for (int u = 0; u < kFdUnroll; ++u) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          e[v] = sq_acc(p[u][v], t[u][v], e[v]);
          if (SRC) a[v] = sq_acc(s[u][v], t[u][v], a[v]);
        }
      }
    }
    for (; c < C; c += kFdSlices) {
      float p[V], t[V], s[V];
      const long at = base + (long)c * HW;
      P::load(pred + at, p);
      P::load(tgt + at, t);
      if (SRC) P::load(src + at, s);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        e[v] = sq_acc(p[v], t[v], e[v]);
        if (SRC) a[v] = sq_acc(s[v], t[v], a[v]);
      }
    }
  }
  if (slice > 0) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      red[0][slice - 1][v][lane] = e[v];
      if (SRC) red[SRC ? 1 : 0][slice - 1][v][lane] = a[v];
    }
  }
  __syncthreads();
  if (slice > 0) return;
  float total = 0.0f;
  unsigned picked[(V + 3) / 4];
#pragma unroll
  for (int k = 0; k < (V + 3) / 4; ++k) picked[k] = 0u;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float ep = e[v], ea = a[v];
#pragma unroll
    for (int s = 0; s < kFdSlices - 1; ++s) {   // slice order, the same for both sums
      ep += red[0][s][v][lane];
      if (SRC) ea += red[SRC ? 1 : 0][s][v][lane];
    }
    const float lp = ep / (float)C, la = ea / (float)C;
    const bool sp = !SRC || lp <= la;   // a tie selects the prediction
    total += sp ? lp : la;
    picked[v >> 2] |= (sp ? 1u : 0u) << (8 * (v & 3));
  }
  if (live) {
    uint8_t* out = sel + (long)b * HW + pix;
    if (V == 1) {
      out[0] = (uint8_t)picked[0];
    } else {
#pragma unroll
      for (int k = 0; k < (V + 3) / 4; ++k) reinterpret_cast<unsigned*>(out)[k] = picked[k];
    }
  } else {
    total = 0.0f;
  }
  total = wave_sum(total);
  if (lane == 0) partials[(long)b * gridDim.x + blockIdx.x] = total;
}

// loss[0] = (accumulate ? loss[0] : 0) + sum(partials) * inv_count: the levels of one loss add up on the device
__global__ __launch_bounds__(kWave) void feature_distance_finish_kernel(const float* __restrict__ partials, int n, float inv_count,
                                                                        float* __restrict__ loss, int accumulate) {
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += kWave) s += partials[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = accumulate ? loss[0] + s * inv_count : s * inv_count;
}

// grid as the forward's.  g_pred = g_loss * scale * (pred - tgt) where sel, exact zeros elsewhere (nothing loaded there).
template <class P>
__global__ __launch_bounds__(kBlock) void feature_distance_bwd_kernel(int C, int HW, float scale,
                                                                      const typename P::elem* __restrict__ pred,
                                                                      const typename P::elem* __restrict__ tgt,
                                                                      const uint8_t* __restrict__ sel, const float* __restrict__ g_loss,
                                                                      typename P::elem* __restrict__ g_pred) {
  constexpr int V = P::V;
  const int lane = threadIdx.x & (kWave - 1), slice = threadIdx.x >> 6, b = blockIdx.y;
  const long pix = ((long)blockIdx.x * kWave + lane) * V;
  if (pix >= HW) return;
  bool m[V], any = false;
  const uint8_t* in = sel + (long)b * HW + pix;
  if (V == 1) {
    m[0] = in[0] != 0;
    any = m[0];
  } else {
#pragma unroll
    for (int k = 0; k < (V + 3) / 4; ++k) {
      const unsigned word = reinterpret_cast<const unsigned*>(in)[k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * k + j < V) m[4 * k + j] = ((word >> (8 * j)) & 0xffu) != 0u;
      any = any || word != 0u;
    }
  }
  const long base = (long)b * C * HW + pix;
  if (!any) {
    float z[V];
#pragma unroll
    for (int v = 0; v < V; ++v) z[v] = 0.0f;
    for (int c = slice; c < C; c += kFdSlices) P::store(g_pred + base + (long)c * HW, z);
    return;
  }
  const float g = g_loss[0] * scale;
  int c = slice;
  for (; c + (kFdUnroll - 1) * kFdSlices < C; c += kFdUnroll * kFdSlices) {
    float p[kFdUnroll][V], t[kFdUnroll][V];
#pragma unroll
    for (int u = 0; u < kFdUnroll; ++u) {
      const long at = base + (long)(c + u * kFdSlices) * HW;
      P::load(pred + at, p[u]);
      P::load(tgt + at, t[u]);
    }
#pragma unroll
    for (int u = 0; u < kFdUnroll; ++u) {
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = m[v] ? g * (p[u][v] - t[u][v]) : 0.0f;
      P::store(g_pred + base + (long)(c + u * kFdSlices) * HW, o);
    }
  }
  for (; c < C; c += kFdSlices) {
    float p[V], t[V], o[V];
    const long at = base + (long)c * HW;
    P::load(pred + at, p);
    P::load(tgt + at, t);
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = m[v] ? g * (p[v] - t[v]) : 0.0f;
    P::store(g_pred + at, o);
  }
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <class P>
static void launch_fwd(int B, int C, int HW, const void* pred, const void* target, const void* source, uint8_t* sel,
                       float* partials, int nblk, hipStream_t s) {
  typedef typename P::elem E;
  dim3 grid(nblk, B);
  if (source)
    feature_distance_fwd_kernel<P, true><<<grid, kBlock, 0, s>>>(C, HW, (const E*)pred, (const E*)target, (const E*)source, sel, partials);
  else
    feature_distance_fwd_kernel<P, false><<<grid, kBlock, 0, s>>>(C, HW, (const E*)pred, (const E*)target, nullptr, sel, partials);
}

template <class P>
static void launch_bwd(int B, int C, int HW, float scale, const void* pred, const void* target, const uint8_t* sel,
                       const float* g_loss, void* g_pred, hipStream_t s) {
  typedef typename P::elem E;
  dim3 grid(ceil_div(HW, kWave * P::V), B);
  feature_distance_bwd_kernel<P><<<grid, kBlock, 0, s>>>(C, HW, scale, (const E*)pred, (const E*)target, sel, g_loss, (E*)g_pred);
}

static int check_shape(int B, int C, int h, int w, int dtype) {
  PD_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0, "bad shape: B = %d, C = %d, h = %d, w = %d must all be positive", B, C, h, w);
  PD_REQUIRE(B <= 65535, "B = %d is beyond the launch grid's limit of 65535", B);
  PD_REQUIRE((long)B * h * w < (1L << 31), "B * h * w = %ld pixels is beyond the limit of 2^31", (long)B * h * w);
  PD_REQUIRE(dtype == PD_DTYPE_F32 || dtype == PD_DTYPE_BF16, "unknown dtype %d (PD_DTYPE_F32 = 0, PD_DTYPE_BF16 = 1)", dtype);
  return PD_OK;
}

}  // namespace pd

using namespace pd;

extern "C" int pd_feature_distance_fwd(int B, int C, int h, int w, int dtype, const void* pred, const void* target,
                                       const void* source, uint8_t* sel, float* partials, float* loss, int accumulate,
                                       pd_stream_t stream) {
  if (const int rc = check_shape(B, C, h, w, dtype)) return rc;
  PD_REQUIRE(pred && target && sel && partials && loss, "NULL pointer");
  const int HW = h * w;
  const int V = dtype == PD_DTYPE_BF16 ? 8 : 4;
  const bool vec = HW % V == 0 && aligned_to(pred, 16) && aligned_to(target, 16) && aligned_to(source, 16) && aligned_to(sel, 4);
  const int nblk = ceil_div(HW, kWave * (vec ? V : 1));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PD_DTYPE_BF16) {
    if (vec) launch_fwd<PackBf16x8>(B, C, HW, pred, target, source, sel, partials, nblk, s);
    else     launch_fwd<PackBf16x1>(B, C, HW, pred, target, source, sel, partials, nblk, s);
  } else {
    if (vec) launch_fwd<PackF32x4>(B, C, HW, pred, target, source, sel, partials, nblk, s);
    else     launch_fwd<PackF32x1>(B, C, HW, pred, target, source, sel, partials, nblk, s);
  }
  feature_distance_finish_kernel<<<1, kWave, 0, s>>>(partials, nblk * B, (float)(1.0 / ((double)B * (double)HW)), loss, accumulate);
  return check_launch("feature_distance_fwd_kernel");
}

extern "C" int pd_feature_distance_bwd(int B, int C, int h, int w, int dtype, const void* pred, const void* target,
                                       const uint8_t* sel, const float* g_loss, void* g_pred, pd_stream_t stream) {
  if (const int rc = check_shape(B, C, h, w, dtype)) return rc;
  PD_REQUIRE(pred && target && sel && g_loss && g_pred, "NULL pointer");
  const int HW = h * w;
  const int V = dtype == PD_DTYPE_BF16 ? 8 : 4;
  const bool vec = HW % V == 0 && aligned_to(pred, 16) && aligned_to(target, 16) && aligned_to(g_pred, 16) && aligned_to(sel, 4);
  const float scale = (float)(2.0 / ((double)C * (double)B * (double)HW));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PD_DTYPE_BF16) {
    if (vec) launch_bwd<PackBf16x8>(B, C, HW, scale, pred, target, sel, g_loss, g_pred, s);
    else     launch_bwd<PackBf16x1>(B, C, HW, scale, pred, target, sel, g_loss, g_pred, s);
  } else {
    if (vec) launch_bwd<PackF32x4>(B, C, HW, scale, pred, target, sel, g_loss, g_pred, s);
    else     launch_bwd<PackF32x1>(B, C, HW, scale, pred, target, sel, g_loss, g_pred, s);
  }
  return check_launch("feature_distance_bwd_kernel");
}
