// The reference's input pipeline on the device (datasets/pair_transforms.py: RandomResizeCrop :27-56, Resize :66-84, RandomGamma
// :94-102, RandomBrightness :112-121, RandomColorBrightness :131-141, driven from datasets/mono_dataset.py:149-187): from the decoded
// frames of a sample to the cropped `color` / `color_aug` windows in ONE kernel, and the nearest resize-crop of depth_gt in another.
// The reference resizes the whole frame on the host (F.interpolate bicubic, align_corners=True), clamps, crops and then runs three
// elementwise passes; here only the window is computed and the resized frame never exists.
//
// Arithmetic.  Output pixel (y, x) of a window at (h0, w0) inside a resize to full_h x full_w reads the source at
//   ry = (y + h0) (hs - 1) / (full_h - 1),   rx = (x + w0) (ws - 1) / (full_w - 1)              (align_corners=True)
// whose floor and fraction are the QUOTIENT and REMAINDER of an integer division, so the coordinate is exact wherever the window
// lies (ATen forms scale * index in fp32: 8e-5 off fp64 at the far corner of a KITTI frame).  Weights: ATen's cubic convolution,
// A = -0.75 (UpSample.h: get_cubic_upsample_coefficients); taps i-1 .. i+2 clamped into the frame (upsample_get_value_bounded);
// rows first, then columns of rows, as upsample_bicubic2d does.  uint8 sources become fp32 by the correctly rounded v / 255
// (ToTensor).  A whole-number coordinate has weights (0, 1, 0, 0) exactly, so full == source copies the source bit for bit.
//
// Shape.  A lane owns one output column of a band of kBandRows rows: its four column taps and weights are fixed for the band.  The
// source row index is wave-uniform; the lane keeps the four horizontally interpolated source rows the current output row needs
// (4 x 3 floats) and advances that window by as many source rows as the output row moved.  No LDS, no intermediate in memory.
//
// Memory.  Every tap is clamped into [0, hs-1] x [0, ws-1] with hs <= Hmax, ws <= Wmax, whatever the parameter tensors hold, and
// every load is one element wide through a buffer descriptor of exactly one frame, so nothing outside `src` is touched and padding
// rows / columns never reach a result.  Stores cover the two outputs exactly.
#include <math.h>

#include "pd_common.h"

namespace pd {

// Tuning knobs (scripts/build_variants.sh builds variants with -D...): lanes = output columns, and output rows, per workgroup
#ifndef PD_PIPE_BLOCK
#define PD_PIPE_BLOCK 128
#endif
#ifndef PD_PIPE_BAND_ROWS
#define PD_PIPE_BAND_ROWS 8
#endif
constexpr int kPipeBlock = PD_PIPE_BLOCK;
constexpr int kBandRows = PD_PIPE_BAND_ROWS;
constexpr int kMaxPos = 65535;    // (y + h0), (x + w0) are clamped here: with sizes <= 32768 the coordinate's numerator is < 2^31

typedef __amdgpu_buffer_rsrc_t FrameRsrc;

struct PipeArgs {
  int V, Hmax, Wmax, H, W;
  const void* src;
  const int* src_hw;
  const int* crop;
  const int* flags;
  const float* aug;
  float* color;
  float* color_aug;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// floor and fraction of pos * size_m1 / den, exact: pos in [0, kMaxPos], size_m1 < 32768, den >= 1
struct Coord {
  int i;
  float t;
};
__device__ __forceinline__ Coord src_coord(int pos, int size_m1, int den) {
  const unsigned n = (unsigned)pos * (unsigned)size_m1;
  const unsigned q = n / (unsigned)den, r = n - q * (unsigned)den;
  Coord c;
  c.i = (int)q;
  c.t = (float)r / (float)den;
  return c;
}

// ATen's cubic convolution coefficients (A = -0.75) of the taps i-1, i, i+1, i+2 at fraction t
__device__ __forceinline__ float cubic1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.0f; }            // |x| <= 1
__device__ __forceinline__ float cubic2(float x) { return ((-0.75f * x + 3.75f) * x - 6.0f) * x + 3.0f; }     // 1 < |x| < 2
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
  w[0] = cubic2(t + 1.0f);
  w[1] = cubic1(t);
  w[2] = cubic1(1.0f - t);
  w[3] = cubic2(2.0f - t);
}

// Source layouts: byte offset of channel 0 of (row, col) inside one frame, the step to the next channel, and the element load.
struct PxU8 {   // [Hmax, Wmax, 3] uint8, as an image decoder leaves a frame
  static __device__ __forceinline__ long frame_bytes(int Hmax, int Wmax) { return (long)Hmax * Wmax * 3; }
  static __device__ __forceinline__ unsigned row_off(int row, int Hmax, int Wmax) { return (unsigned)(row * Wmax) * 3u; }
  static __device__ __forceinline__ unsigned col_off(int col) { return (unsigned)col * 3u; }
  static __device__ __forceinline__ unsigned chan_step(int Hmax, int Wmax) { return 1u; }
  static __device__ __forceinline__ float load(FrameRsrc r, unsigned off) {
    // ToTensor's v / 255, correctly rounded: Markstein's correction from the correctly rounded reciprocal (div_by)
    const float v = (float)__builtin_amdgcn_raw_buffer_load_b8(r, (int)off, 0, 0);
    return div_by(v, 255.0f, 1.0f / 255.0f);
  }
};
struct PxF32 {   // [3, Hmax, Wmax] fp32
  static __device__ __forceinline__ long frame_bytes(int Hmax, int Wmax) { return (long)Hmax * Wmax * 12; }
  static __device__ __forceinline__ unsigned row_off(int row, int Hmax, int Wmax) { return (unsigned)(row * Wmax) * 4u; }
  static __device__ __forceinline__ unsigned col_off(int col) { return (unsigned)col * 4u; }
  static __device__ __forceinline__ unsigned chan_step(int Hmax, int Wmax) { return (unsigned)(Hmax * Wmax) * 4u; }
  static __device__ __forceinline__ float load(FrameRsrc r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
  }
};

// The reference's comparisons, which let a NaN through as torch's do
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
__device__ __forceinline__ float cap1(float v) { return v > 1.0f ? 1.0f : v; }

template <class Px>
__global__ __launch_bounds__(kPipeBlock) void resize_crop_augment_kernel(PipeArgs a) {
  const int bv = blockIdx.z, b = bv / a.V;
  const int x = blockIdx.x * kPipeBlock + threadIdx.x;
  if (x >= a.W) return;   // (no barrier below)
  const int y0 = blockIdx.y * kBandRows, y1 = min(y0 + kBandRows, a.H);

  // per sample, workgroup-uniform
  const int hs = clampi(a.src_hw[2 * b], 1, a.Hmax), ws = clampi(a.src_hw[2 * b + 1], 1, a.Wmax);
  const int den_w = max(a.crop[4 * b] - 1, 1), den_h = max(a.crop[4 * b + 1] - 1, 1);
  const int w0 = clampi(a.crop[4 * b + 2], 0, kMaxPos), h0 = clampi(a.crop[4 * b + 3], 0, kMaxPos);
  const int fl = a.flags[b];
  const bool flip = (fl & PD_PIPE_FLIP) != 0;
  const FrameRsrc frame = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(static_cast<const char*>(a.src)) + (long)bv * Px::frame_bytes(a.Hmax, a.Wmax), 0,
      (int)Px::frame_bytes(a.Hmax, a.Wmax), 0x00020000);
  const unsigned cstep = Px::chan_step(a.Hmax, a.Wmax);

  // the column chain, once per band: four taps (mirrored under flip: the frame is transposed before everything else) and weights
  const Coord cx = src_coord(min(x + w0, kMaxPos), ws - 1, den_w);
  float wx[4];
  cubic_weights(cx.t, wx);
  unsigned coff[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = clampi(cx.i - 1 + k, 0, ws - 1);
    coff[k] = Px::col_off(flip ? ws - 1 - c : c);
  }
  // one source row, interpolated along x
  auto hrow = [&](int r, float (&o)[3]) {
    const unsigned roff = Px::row_off(clampi(r, 0, hs - 1), a.Hmax, a.Wmax);
    float p[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[k][c] = Px::load(frame, roff + coff[k] + (unsigned)c * cstep);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = p[0][c] * wx[0] + p[1][c] * wx[1] + p[2][c] * wx[2] + p[3][c] * wx[3];
  };

  const float* ag = a.aug + (long)bv * 5;
  const float gamma = ag[0], bright = ag[1], ch[3] = {ag[2], ag[3], ag[4]};
  const size_t plane = (size_t)a.H * a.W;
  float* out = a.color + (size_t)bv * 3 * plane + x;
  float* out_aug = a.color_aug + (size_t)bv * 3 * plane + x;

  float win[4][3];   // source rows cur-1 .. cur+2, interpolated along x
  int cur = 0;
  for (int y = y0; y < y1; ++y) {
    const Coord cy = src_coord(min(y + h0, kMaxPos), hs - 1, den_h);   // wave-uniform
    if (y == y0 || cy.i - cur >= 4) {
      cur = cy.i;
#pragma unroll
      for (int k = 0; k < 4; ++k) hrow(cur - 1 + k, win[k]);
    }
    while (cur < cy.i) {   // the coordinate never moves backwards
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) win[k][c] = win[k + 1][c];
      hrow(cur + 3, win[3]);
      ++cur;
    }
    float wy[4];
    cubic_weights(cy.t, wy);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = clamp01(win[0][c] * wy[0] + win[1][c] * wy[1] + win[2][c] * wy[2] + win[3][c] * wy[3]);
      out[c * plane + (size_t)y * a.W] = v;
      float g = v;   // a stage whose bit is clear is skipped: flags 0 leaves the clone
      if (fl & PD_PIPE_GAMMA) g = powf(g, gamma);
      if (fl & PD_PIPE_BRIGHTNESS) g = cap1(g * bright);
      if (fl & PD_PIPE_CHANNEL) g = cap1(g * ch[c]);
      out_aug[c * plane + (size_t)y * a.W] = g;
    }
  }
}

// depth_gt: F.interpolate(mode="nearest") to full_h x full_w, then the crop (pair_transforms.py:50-54, 79-82).  ATen's legacy
// nearest index: min((int)floorf(dst * scale), in - 1), scale = (float)in / out, one fp32 product.
__device__ __forceinline__ int nearest_index(int dst, int in, int full) {
#pragma clang fp contract(off)
  const float scale = (float)in / (float)full;
  return min((int)floorf((float)dst * scale), in - 1);
}

__global__ __launch_bounds__(kBlock) void resize_crop_nearest_kernel(int Hd, int Wd, int H, int W, const float* __restrict__ src,
                                                                     const int* __restrict__ src_hw, const int* __restrict__ crop,
                                                                     const int* __restrict__ flags, float* __restrict__ out) {
  const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const int hs = clampi(src_hw[2 * b], 1, Hd), ws = clampi(src_hw[2 * b + 1], 1, Wd);
  const int full_w = max(crop[4 * b], 1), full_h = max(crop[4 * b + 1], 1);
  const int w0 = clampi(crop[4 * b + 2], 0, kMaxPos), h0 = clampi(crop[4 * b + 3], 0, kMaxPos);
  const int sy = clampi(nearest_index(y + h0, hs, full_h), 0, hs - 1);
  int sx = clampi(nearest_index(x + w0, ws, full_w), 0, ws - 1);
  if (flags[b] & PD_PIPE_FLIP) sx = ws - 1 - sx;   // np.fliplr of the source
  out[((size_t)b * H + y) * W + x] = src[((size_t)b * Hd + sy) * Wd + sx];
}

}  // namespace pd

using namespace pd;

extern "C" int pd_resize_crop_augment(int B, int V, int Hmax, int Wmax, int H, int W, int src_dtype, const void* src,
                                      const int32_t* src_hw, const int32_t* crop, const int32_t* flags, const float* aug,
                                      float* color, float* color_aug, pd_stream_t stream) {
  PD_REQUIRE(B > 0 && V > 0 && (long)B * V <= 65535, "bad shape: B = %d, V = %d (B * V <= 65535)", B, V);
  PD_REQUIRE(H > 0 && W > 0 && H <= 65536 && W <= 65536, "bad shape: window %d x %d", H, W);
  PD_REQUIRE(Hmax > 0 && Wmax > 0 && Hmax <= 32768 && Wmax <= 32768 && (long)Hmax * Wmax * 12 < (1L << 31),
             "bad shape: frames of %d x %d (each side <= 32768, one frame below 2 GiB)", Hmax, Wmax);
  PD_REQUIRE(src_dtype == PD_SRC_U8_HWC || src_dtype == PD_SRC_F32_CHW, "src_dtype %d is neither PD_SRC_U8_HWC nor PD_SRC_F32_CHW",
             src_dtype);
  PD_REQUIRE(src && src_hw && crop && flags && aug && color && color_aug, "NULL pointer");
  PD_REQUIRE(color != color_aug, "color and color_aug alias");
  PipeArgs a = {V, Hmax, Wmax, H, W, src, src_hw, crop, flags, aug, color, color_aug};
  const dim3 grid(ceil_div(W, kPipeBlock), ceil_div(H, kBandRows), B * V);
  if (src_dtype == PD_SRC_U8_HWC)
    resize_crop_augment_kernel<PxU8><<<grid, kPipeBlock, 0, (hipStream_t)stream>>>(a);
  else
    resize_crop_augment_kernel<PxF32><<<grid, kPipeBlock, 0, (hipStream_t)stream>>>(a);
  return check_launch("resize_crop_augment_kernel");
}

extern "C" int pd_resize_crop_nearest(int B, int Hd, int Wd, int H, int W, const float* src, const int32_t* src_hw,
                                      const int32_t* crop, const int32_t* flags, float* out, pd_stream_t stream) {
  PD_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && W <= 65536, "bad shape: B = %d, window %d x %d", B, H, W);
  PD_REQUIRE(Hd > 0 && Wd > 0 && Hd <= 32768 && Wd <= 32768, "bad shape: depth maps of %d x %d", Hd, Wd);
  PD_REQUIRE(src && src_hw && crop && flags && out, "NULL pointer");
  resize_crop_nearest_kernel<<<dim3(ceil_div(W, kBlock), H, B), kBlock, 0, (hipStream_t)stream>>>(Hd, Wd, H, W, src, src_hw, crop,
                                                                                                   flags, out);
  return check_launch("resize_crop_nearest_kernel");
}
