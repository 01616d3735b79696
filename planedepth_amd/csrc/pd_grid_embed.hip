// The decoders' positional encoding of inputs["grid"] as one operator (networks/depth_decoder.py:123-139, networks/pose_net.py:137-140,
// networks/plade_net.py:150-158, layers.py:308-354): the reference embeds the full-resolution grid [B,2,H,W] with `epconv` (Conv2d(2,16,1),
// ELU, Conv2d(16,E,1), ELU) or with `Embedder`, and then resamples the [B,E,H,W] map with F.interpolate(bilinear, align_corners=True) to
// every decoder level.  An output pixel depends on four grid points only, so here a lane owns one OUTPUT pixel of one level, evaluates the
// embedding at its four taps and blends: no [B,.,H,W] map is written, kept for backward or read again.  One launch serves every level of
// a call; the levels' outputs [B,E,h_l,w_l] follow each other in one flat buffer.
//
// Arithmetic.  Output row y of a level with h_l rows reads the source at y (H - 1) / (h_l - 1) (align_corners=True), whose floor and
// fraction are the QUOTIENT and REMAINDER of an integer division (as in pd_input_pipeline.hip): exact at any size, 0 / 0 for h_l = 1.
// The second tap is clamped to the last row / column.  Order of operations as ATen's upsample_bilinear2d: embed at the four taps, blend
// along x, then along y.  ELU (alpha = 1) evaluates expm1f on its negative branch.
//
// Dynamic E.  The neural kernels are instantiated for a padded channel count PE in {4, 8, 16}: every loop over channels is unrolled, so
// the per-channel accumulators of the backward are registers with static indices; the rows e >= E are skipped (wave-uniform test), which
// leaves their accumulators zero, and only E channels are loaded and stored.  The weights are read with wave-uniform addresses.
//
// Backward.  grid has no gradient.  A lane walks its items (output pixels) in a fixed order, recomputes z1 / e1 / z2 per tap from the grid
// and keeps PRIVATE sums of the 48 + 17 E parameter gradients; then one DPP reduction per wave, the four waves' results added in wave
// order, one row of partials per workgroup, and pd::reduce_partials.  No float atomics anywhere: two runs give the same bits.  PE = 16
// would need 320 accumulators per lane, so its W2 / b2 rows are split over two passes (blockIdx.y) of 8 rows each; pass 0 also owns W1 / b1.
//
// Memory.  Taps are clamped into [0, H-1] x [0, W-1]; stores cover exactly out[off_l + ((b E + e) h_l + y) w_l + x] for the items of the
// launch; the backward writes nblk rows of 48 + 17 E partials and the 48 + 17 E gradients.
#include <math.h>

#include "pd_common.h"

namespace pd {

constexpr int kHidden = 16;             // the reference hard-codes Conv2d(2, 16, 1)
constexpr int kEmbedMaxLevels = 8;
constexpr int kEmbedMaxChannels = 16;   // neural kind
constexpr int kEmbedMaxMultires = 16;   // frequency kind: E = 2 + 4 multires
constexpr int kEmbedBwdBlocks = 512;    // at most this many workgroups (rows of partials) in the backward

struct EmbedLevels {
  int n, B, H, W, E, total;             // total = items (output pixels of all samples) of all levels
  int h[kEmbedMaxLevels], w[kEmbedMaxLevels];
  int first[kEmbedMaxLevels];           // first item of level l
  size_t off[kEmbedMaxLevels];          // first float of level l in the flat buffer
};

// One output pixel: where it is stored and what it reads.
struct EmbedItem {
  size_t out;          // float offset of channel 0
  size_t chan;         // floats between two channels: h_l w_l
  unsigned g00, g01, g10, g11; // float offsets of the taps' x component (2 B H W < 2^31); the y component is H W further
  float tx, ty;        // fractions along x / y
};

// floor and fraction of pos * size_m1 / den, exact: the product is below 2^31 (sizes are bounded at the entry points), den >= 1
__device__ __forceinline__ void embed_coord(int pos, int size_m1, int den, int& i, float& t) {
  const unsigned n = (unsigned)pos * (unsigned)size_m1;
  const unsigned q = n / (unsigned)den, r = n - q * (unsigned)den;
  i = (int)q;
  t = (float)r / (float)den;
}

__device__ __forceinline__ EmbedItem embed_item(const EmbedLevels& L, int i) {
  // the level of item i: static indices only (a lane-dependent index into the kernel arguments would put them into scratch)
  int h = L.h[0], w = L.w[0], first = 0;
  size_t off = 0;
#pragma unroll
  for (int k = 1; k < kEmbedMaxLevels; ++k)
    if (k < L.n && i >= L.first[k]) {
      h = L.h[k];
      w = L.w[k];
      first = L.first[k];
      off = L.off[k];
    }
  unsigned r = (unsigned)(i - first);
  const unsigned per = (unsigned)h * (unsigned)w;
  const unsigned b = r / per;
  r -= b * per;
  const unsigned y = r / (unsigned)w, x = r - y * (unsigned)w;
  int y0, x0;
  EmbedItem it;
  embed_coord((int)y, L.H - 1, max(h - 1, 1), y0, it.ty);
  embed_coord((int)x, L.W - 1, max(w - 1, 1), x0, it.tx);
  const int y1 = min(y0 + 1, L.H - 1), x1 = min(x0 + 1, L.W - 1);
  const unsigned base = b * 2u * (unsigned)(L.H * L.W), r0 = base + (unsigned)(y0 * L.W), r1 = base + (unsigned)(y1 * L.W);
  it.g00 = r0 + x0;
  it.g01 = r0 + x1;
  it.g10 = r1 + x0;
  it.g11 = r1 + x1;
  it.chan = per;
  it.out = off + ((size_t)b * L.E * h + y) * w + x;
  return it;
}

// ATen's upsample_bilinear2d: h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) with w1 the fraction and w0 = 1 - w1
__device__ __forceinline__ float embed_blend(float v00, float v01, float v10, float v11, float tx, float ty) {
  const float wx0 = 1.0f - tx, wy0 = 1.0f - ty;
  return wy0 * (wx0 * v00 + tx * v01) + ty * (wx0 * v10 + tx * v11);
}

__device__ __forceinline__ float elu(float z) { return z > 0.0f ? z : expm1f(z); }

// e1 = ELU(W1 g + b1) at one grid point; prm = W1 [16,2], b1 [16], W2 [E,16], b2 [E]
__device__ __forceinline__ void embed_hidden(const float* __restrict__ prm, float gx, float gy, float (&e1)[kHidden]) {
#pragma unroll
  for (int j = 0; j < kHidden; ++j) e1[j] = elu(fmaf(prm[2 * j + 1], gy, fmaf(prm[2 * j], gx, prm[2 * kHidden + j])));
}

template <int PE>
__global__ __launch_bounds__(kBlock) void grid_embed_neural_fwd_kernel(EmbedLevels L, const float* __restrict__ grid,
                                                                       const float* __restrict__ prm, float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= L.total) return;   // (no barrier below)
  const EmbedItem it = embed_item(L, i);
  const unsigned plane = (unsigned)(L.H * L.W);
  const unsigned tap[4] = {it.g00, it.g01, it.g10, it.g11};
  float e1[4][kHidden];
#pragma unroll
  for (int t = 0; t < 4; ++t) embed_hidden(prm, grid[tap[t]], grid[tap[t] + plane], e1[t]);
  const float* W2 = prm + 3 * kHidden;
  const float* b2 = W2 + L.E * kHidden;
#pragma unroll
  for (int e = 0; e < PE; ++e) {
    if (e < L.E) {   // wave-uniform
      float v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float z = b2[e];
#pragma unroll
        for (int j = 0; j < kHidden; ++j) z = fmaf(W2[e * kHidden + j], e1[t][j], z);
        v[t] = elu(z);
      }
      out[it.out + e * it.chan] = embed_blend(v[0], v[1], v[2], v[3], it.tx, it.ty);
    }
  }
}

// PD_EMBED_FREQUENCY: cat(g, sin(g 2^k), cos(g 2^k)), k < multires, in Embedder's channel order (layers.py:318-339); PD_EMBED_IDENTITY
// is multires = 0.  Channel c: axis c & 1; c >= 2: k = (c - 2) / 4, cos when (c - 2) & 2.
__global__ __launch_bounds__(kBlock) void grid_embed_plain_fwd_kernel(EmbedLevels L, const float* __restrict__ grid,
                                                                      float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= L.total) return;
  const EmbedItem it = embed_item(L, i);
  const unsigned plane = (unsigned)(L.H * L.W);
  const float x00 = grid[it.g00], x01 = grid[it.g01], x10 = grid[it.g10], x11 = grid[it.g11];
  const float y00 = grid[it.g00 + plane], y01 = grid[it.g01 + plane], y10 = grid[it.g10 + plane], y11 = grid[it.g11 + plane];
  for (int c = 0; c < L.E; ++c) {   // wave-uniform
    const bool ax = c & 1;
    float v00 = ax ? y00 : x00, v01 = ax ? y01 : x01, v10 = ax ? y10 : x10, v11 = ax ? y11 : x11;
    if (c >= 2) {
      const float f = (float)(1 << ((c - 2) >> 2));   // torch: 2.**linspace(0, multires - 1, multires), exact powers of two
      if ((c - 2) & 2) {
        v00 = cosf(v00 * f); v01 = cosf(v01 * f); v10 = cosf(v10 * f); v11 = cosf(v11 * f);
      } else {
        v00 = sinf(v00 * f); v01 = sinf(v01 * f); v10 = sinf(v10 * f); v11 = sinf(v11 * f);
      }
    }
    out[it.out + c * it.chan] = embed_blend(v00, v01, v10, v11, it.tx, it.ty);
  }
}

// Columns of one row of partials (= the layout of params and of g_params): W1 [16,2] at 0, b1 [16] at 32, W2 [E,16] at 48, b2 [E] at
// 48 + 16 E.
template <int PE, int NPASS>
__global__ __launch_bounds__(kBlock) void grid_embed_bwd_kernel(EmbedLevels L, const float* __restrict__ grid, const float* __restrict__ prm,
                                                                const float* __restrict__ g_out, float* __restrict__ partials) {
  constexpr int EH = PE / NPASS;                      // W2 / b2 rows a pass accumulates
  constexpr int kCols = 3 * kHidden + EH * (kHidden + 1);
  const int pass = NPASS > 1 ? (int)blockIdx.y : 0;   // workgroup-uniform
  const bool first = pass == 0;                       // this pass owns W1 / b1, which need g_e1 over ALL rows e
  const int E = L.E;
  const unsigned plane = (unsigned)(L.H * L.W);
  const float* W2 = prm + 3 * kHidden;
  const float* b2 = W2 + E * kHidden;

  float aW1x[kHidden] = {}, aW1y[kHidden] = {}, ab1[kHidden] = {}, aW2[EH][kHidden] = {}, ab2[EH] = {};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < L.total; i += gridDim.x * kBlock) {
    const EmbedItem it = embed_item(L, i);
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      const float c = ((t & 2) ? it.ty : 1.0f - it.ty) * ((t & 1) ? it.tx : 1.0f - it.tx);
      if (c == 0.0f) continue;   // a tap without weight adds exact zeros (three of four taps where a level has the source's size)
      const unsigned tap = (t & 2) ? ((t & 1) ? it.g11 : it.g10) : ((t & 1) ? it.g01 : it.g00);
      const float gx = grid[tap], gy = grid[tap + plane];
      float e1[kHidden], ge1[kHidden] = {};
      embed_hidden(prm, gx, gy, e1);
#pragma unroll
      for (int e = 0; e < PE; ++e) {
        const bool mine = NPASS == 1 || e / EH == pass;
        if (e < E && (mine || first)) {   // wave-uniform
          float z = b2[e];
#pragma unroll
          for (int j = 0; j < kHidden; ++j) z = fmaf(W2[e * kHidden + j], e1[j], z);
          const float gz = g_out[it.out + e * it.chan] * c * (z > 0.0f ? 1.0f : expf(z));   // d ELU(z) / dz
          if (mine) {
#pragma unroll
            for (int j = 0; j < kHidden; ++j) aW2[e % EH][j] = fmaf(gz, e1[j], aW2[e % EH][j]);
            ab2[e % EH] += gz;
          }
          if (first) {
#pragma unroll
            for (int j = 0; j < kHidden; ++j) ge1[j] = fmaf(W2[e * kHidden + j], gz, ge1[j]);
          }
        }
      }
      if (first) {
#pragma unroll
        for (int j = 0; j < kHidden; ++j) {
          const float gz1 = ge1[j] * (e1[j] > 0.0f ? 1.0f : e1[j] + 1.0f);   // exp(z1) = expm1(z1) + 1 where z1 <= 0
          aW1x[j] = fmaf(gz1, gx, aW1x[j]);
          aW1y[j] = fmaf(gz1, gy, aW1y[j]);
          ab1[j] += gz1;
        }
      }
    }
  }

  // wave sums (DPP, the total arrives in lane 63), then the four waves in wave order
  __shared__ float red[kBlock / kWave][kCols];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  auto put = [&](int m, float v) {
    v = wave_sum_hi(v);
    if (lane == kWave - 1) red[wave][m] = v;
  };
#pragma unroll
  for (int j = 0; j < kHidden; ++j) {
    put(2 * j, aW1x[j]);
    put(2 * j + 1, aW1y[j]);
    put(2 * kHidden + j, ab1[j]);
  }
#pragma unroll
  for (int r = 0; r < EH; ++r) {
#pragma unroll
    for (int j = 0; j < kHidden; ++j) put(3 * kHidden + r * kHidden + j, aW2[r][j]);
    put(3 * kHidden + EH * kHidden + r, ab2[r]);
  }
  __syncthreads();
  const int M = 3 * kHidden + E * (kHidden + 1);
  float* row = partials + (size_t)blockIdx.x * M;
  for (int m = threadIdx.x; m < kCols; m += kBlock) {
    const float s = ((red[0][m] + red[1][m]) + red[2][m]) + red[3][m];
    if (m < 3 * kHidden) {
      if (first) row[m] = s;
    } else if (m < 3 * kHidden + EH * kHidden) {
      const int r = m - 3 * kHidden, e = pass * EH + r / kHidden;
      if (e < E) row[3 * kHidden + e * kHidden + r % kHidden] = s;
    } else {
      const int e = pass * EH + (m - 3 * kHidden - EH * kHidden);
      if (e < E) row[3 * kHidden + E * kHidden + e] = s;
    }
  }
}

// Validation shared by the three entry points; fills L.  `sizes`: n_levels pairs (h_l, w_l) on the HOST.
static int embed_levels(EmbedLevels& L, int B, int H, int W, int E, int n_levels, const int32_t* sizes) {
  PD_REQUIRE(n_levels >= 1 && n_levels <= kEmbedMaxLevels, "n_levels = %d: 1 to %d levels per call", n_levels, kEmbedMaxLevels);
  PD_REQUIRE(sizes, "NULL pointer: sizes");
  PD_REQUIRE(B > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && 2L * B * H * W < (1L << 31),
             "bad shape: grid [%d,2,%d,%d] (each side 1 to 32768, fewer than 2^31 elements)", B, H, W);
  L.n = n_levels;
  L.B = B;
  L.H = H;
  L.W = W;
  L.E = E;
  long items = 0;
  size_t off = 0;
  for (int l = 0; l < kEmbedMaxLevels; ++l) {
    const bool live = l < n_levels;
    const int h = live ? sizes[2 * l] : 1, w = live ? sizes[2 * l + 1] : 1;
    PD_REQUIRE(h >= 1 && w >= 1 && h <= 65536 && w <= 65536, "level %d is %d x %d (each side 1 to 65536)", l, h, w);
    L.h[l] = h;
    L.w[l] = w;
    L.first[l] = (int)items;
    L.off[l] = off;
    if (live) {
      items += (long)B * h * w;
      off += (size_t)B * E * h * w;
      PD_REQUIRE(items <= 0x7fffffffL - (long)kEmbedBwdBlocks * kBlock, "grid of the launch overflows: %ld output pixels up to level %d (B = %d)", items, l, B);
    }
  }
  L.total = (int)items;
  return PD_OK;
}

static int embed_padded(int E) { return E <= 4 ? 4 : (E <= 8 ? 8 : 16); }
static int embed_bwd_blocks(int total) { return min(ceil_div(total, kBlock), kEmbedBwdBlocks); }

}  // namespace pd

using namespace pd;

extern "C" int pd_grid_embed_fwd(int B, int H, int W, int kind, int E, int multires, int n_levels, const int32_t* sizes,
                                 const float* grid, const float* params, float* out, pd_stream_t stream) {
  PD_REQUIRE(kind == PD_EMBED_NEURAL || kind == PD_EMBED_FREQUENCY || kind == PD_EMBED_IDENTITY,
             "kind %d is none of PD_EMBED_NEURAL, PD_EMBED_FREQUENCY, PD_EMBED_IDENTITY", kind);
  if (kind == PD_EMBED_NEURAL) {
    PD_REQUIRE(E >= 1 && E <= kEmbedMaxChannels, "E = %d: the neural kind has 1 to %d channels", E, kEmbedMaxChannels);
    PD_REQUIRE(params, "NULL pointer: params");
  } else if (kind == PD_EMBED_FREQUENCY) {
    PD_REQUIRE(multires >= 0 && multires <= kEmbedMaxMultires, "multires = %d: 0 to %d", multires, kEmbedMaxMultires);
    PD_REQUIRE(E == 2 + 4 * multires, "E = %d, the frequency kind with multires = %d has 2 + 4 multires = %d channels", E, multires,
               2 + 4 * multires);
  } else {
    PD_REQUIRE(E == 2, "E = %d: the identity kind has the grid's 2 channels", E);
  }
  EmbedLevels L;
  if (int rc = embed_levels(L, B, H, W, E, n_levels, sizes)) return rc;
  PD_REQUIRE(grid && out, "NULL pointer: grid / out");
  const dim3 blocks(ceil_div(L.total, kBlock));
  hipStream_t s = (hipStream_t)stream;
  if (kind != PD_EMBED_NEURAL) {
    grid_embed_plain_fwd_kernel<<<blocks, kBlock, 0, s>>>(L, grid, out);
    return check_launch("grid_embed_plain_fwd_kernel");
  }
  switch (embed_padded(E)) {
    case 4: grid_embed_neural_fwd_kernel<4><<<blocks, kBlock, 0, s>>>(L, grid, params, out); break;
    case 8: grid_embed_neural_fwd_kernel<8><<<blocks, kBlock, 0, s>>>(L, grid, params, out); break;
    default: grid_embed_neural_fwd_kernel<16><<<blocks, kBlock, 0, s>>>(L, grid, params, out); break;
  }
  return check_launch("grid_embed_neural_fwd_kernel");
}

extern "C" size_t pd_grid_embed_bwd_workspace_floats(int B, int E, int n_levels, const int32_t* sizes) {
  EmbedLevels L;
  if (E < 1 || E > kEmbedMaxChannels || embed_levels(L, B, 1, 1, E, n_levels, sizes)) return 0;
  return (size_t)embed_bwd_blocks(L.total) * (3 * kHidden + E * (kHidden + 1));
}

extern "C" int pd_grid_embed_bwd(int B, int H, int W, int E, int n_levels, const int32_t* sizes, const float* grid, const float* params,
                                 const float* g_out, float* g_params, float* workspace, pd_stream_t stream) {
  PD_REQUIRE(E >= 1 && E <= kEmbedMaxChannels, "E = %d: the neural kind has 1 to %d channels", E, kEmbedMaxChannels);
  EmbedLevels L;
  if (int rc = embed_levels(L, B, H, W, E, n_levels, sizes)) return rc;
  PD_REQUIRE(grid && params && g_out && g_params && workspace, "NULL pointer: grid / params / g_out / g_params / workspace");
  const int nblk = embed_bwd_blocks(L.total);
  hipStream_t s = (hipStream_t)stream;
  switch (embed_padded(E)) {
    case 4: grid_embed_bwd_kernel<4, 1><<<dim3(nblk), kBlock, 0, s>>>(L, grid, params, g_out, workspace); break;
    case 8: grid_embed_bwd_kernel<8, 1><<<dim3(nblk), kBlock, 0, s>>>(L, grid, params, g_out, workspace); break;
    default: grid_embed_bwd_kernel<16, 2><<<dim3(nblk, 2), kBlock, 0, s>>>(L, grid, params, g_out, workspace); break;
  }
  if (int rc = check_launch("grid_embed_bwd_kernel")) return rc;
  return reduce_partials(workspace, g_params, nblk, 3 * kHidden + E * (kHidden + 1), 1, s);
}
