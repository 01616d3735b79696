// Memory layer of a target row, on top of pd_rowgeom.h's geometry, shared by the row-organised kernels (pd_plane_sweep_rowshift.hip
// with pd_rowshift_fwd.h: one pixel per lane; pd_plane_sweep_fwdstream.hip and pd_plane_sweep_rowstream.hip: two per lane;
// pd_postprocess.hip): dispatch order, buffer resources per (plane, row), the 8- and 12-byte tap loads and the stores, the tap
// ring of the two stream kernels, colour rows in LDS, the staged per-plane shifts.
#pragma once
#include <stdlib.h>

#include "pd_rowgeom.h"

namespace pd {

// Tuning knobs (scripts/build_variants.sh builds variants with -D...): plane-group size and the occupancy the register
// allocator must leave room for (waves per SIMD), of the plane-group forward and the row-shift backward.
#ifndef PD_FWD_U
#define PD_FWD_U 4
#endif
#ifndef PD_FWD_OCC
#define PD_FWD_OCC 3  // (the single-row bodies alone fit 128 VGPRs = 4 waves per SIMD; the pair body needs ~147)
#endif
#ifndef PD_BWD_U
#define PD_BWD_U 2
#endif
#ifndef PD_BWD_OCC
#define PD_BWD_OCC 3
#endif
constexpr int kRowThreadsMax = 512;  // row workgroups use <= 8 waves (row_threads)

// Row handled by workgroup r of an image.  The dispatcher deals consecutive workgroups to the 8 XCDs round-robin; the
// banded mapping gives each XCD (its own L2) a contiguous band of rows instead of every 8th row.
// (image, row) of this workgroup: row-major over the images (all images' row 0, then row 1, ...).  Two effects:
// (1) the rows that need two source rows (inexact vertical round trip) cluster at small y, so they are dispatched
//     FIRST — longest jobs first instead of the last image's heavy rows starting in the last round (forward 0.148 ->
//     0.137 ms);
// (2) consecutive workgroups go to the 8 XCDs round-robin, so with B a multiple of 8 the rows y and y+1 of one image
//     (B workgroups apart) share an XCD and run at the same time: the second source row of an inexact row is its
//     neighbour's main row and mostly hits in that XCD's L2 (PMC at B = 8: backward HBM traffic 995 -> 909 MB).  Padding
//     B to a multiple of 8 to get this for every batch size was measured and rejected: the padding workgroups all land
//     on the same XCDs and leave them idle (B = 4: 4.1 k -> 2.4 k images/s).
__device__ __forceinline__ int wg_image(int B, int H) {
  return (int)((blockIdx.y * gridDim.x + blockIdx.x) % (unsigned)B);
}
__device__ __forceinline__ int wg_rowid(int B, int H) {
  return (int)((blockIdx.y * gridDim.x + blockIdx.x) / (unsigned)B);
}
// The backward walks the rows in the opposite order of the forward: what the forward read last is what the backward reads
// first, and the other way round for the next step's forward — with the gradient stores streaming past the caches
// (PD_STREAM_STORE_AUX = nt) the 256 MB memory-side cache still holds those rows: step +2.4-2.8 % (forward 0.109 -> 0.105 ms,
// backward 0.178 -> 0.174), and the same inside the DDP training step.  (Round 1, write-back stores: no gain — the dirty
// gradient lines cycled the cache.  Forward bottom-up / backward top-down instead: +1 %, worse in the DDP step.)
__device__ __forceinline__ int bwd_rowid(int B, int H) {
  return H - 1 - wg_rowid(B, H);
}

// ---- memory access layer ------------------------------------------------------------------------------------------
// Row-sized buffer resources (SRD in SGPRs, built from workgroup-uniform values only) give three things at once:
//   * a 32-bit per-lane byte offset instead of 64-bit address arithmetic (the u64 adds were ~15% of all VALU cycles);
//   * hardware range checking: a tap left of column 0 (offset wraps to >= 2^31) or right of column W-1 reads as 0,
//     which IS grid_sample's padding_mode="zeros" — no validity compares, selects or clamped indices in the forward;
//   * loads without exec-mask branches, so a whole group's loads issue back to back.
typedef __amdgpu_buffer_rsrc_t Rsrc;
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v3f __attribute__((ext_vector_type(3)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ Rsrc row_rsrc(const float* row, int W) {  // `row` must be wave-uniform
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, W * 4, 0x00020000);
}
// Same, for an address the compiler is known to keep in VGPRs (it then wraps every access in a waterfall loop): state
// the uniformity explicitly.  Not the default: where the address already lives in SGPRs this costs extra moves.
__device__ __forceinline__ Rsrc row_rsrc_uniform(const float* row, int W) {
  const uint64_t p = reinterpret_cast<uint64_t>(row);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(((uint64_t)hi << 32) | lo), 0, W * 4, 0x00020000);
}
// Descriptor with an explicit extent: 0 bytes turns every access through it into a hardware no-op (how the backward
// skips a gradient nobody asked for without a branch per plane).
__device__ __forceinline__ Rsrc row_rsrc_bytes(const float* row, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float buf_load(Rsrc r, unsigned byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ void buf_store(Rsrc r, unsigned byte_off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)byte_off, 0, 0);
}

// Offset of plane n inside one image's [N,H,W] block, in floats: a 32-bit product (the host checks N*H*W < 2^31) added
// to a per-workgroup 64-bit base — the full 64-bit (b*N + n)*HW product per plane and tensor was a third of the scalar
// instructions of the plane loop.
__device__ __forceinline__ const float* plane_ptr(const float* image_base, int n, int HW) {
  return image_base + (unsigned)(n * HW);
}
__device__ __forceinline__ float* plane_ptr(float* image_base, int n, int HW) {
  return image_base + (unsigned)(n * HW);
}

// Storage type of the [B,N,H,W] tensors logits / sigma / g_logits / g_sigma: float, or bf16 bit patterns (PD_LOGITS_BF16) held
// as `Bf16` (pd_common.h, with elems, bf16_lo / bf16_hi and pack_bf16x2: the decoder tails use them too).
template <class T> __device__ __forceinline__ const T* plane_ptr_t(const T* image_base, int n, int HW) {
  return image_base + (unsigned)(n * HW);
}
template <class T> __device__ __forceinline__ T* plane_ptr_t(T* image_base, int n, int HW) { return image_base + (unsigned)(n * HW); }
template <class T> __device__ __forceinline__ Rsrc row_rsrc_t(const T* row, int W) {   // `row` must be wave-uniform
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(row), 0, W * (int)sizeof(T), 0x00020000);
}
__device__ __forceinline__ float elem_f32(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float elem_f32(const Bf16* p, long i) { return __uint_as_float((unsigned)p[i] << 16); }
// one element at column `col` through a row descriptor (range-checked like buf_load)
__device__ __forceinline__ float buf_load_elem(Rsrc r, int col, float*) { return buf_load(r, (unsigned)col << 2); }
__device__ __forceinline__ float buf_load_elem(Rsrc r, int col, Bf16*) {
  return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, (int)((unsigned)col << 1), 0, 0) << 16);
}

// The (up to) four taps of one scalar plane, loaded up-front.  Out-of-image taps come back as 0 from the hardware.
template <int NROWS>
struct Taps {
  float a0, a1, b0, b1;  // row A (x0, x0+1), row B (x0, x0+1)
};

__device__ __forceinline__ v2f buf_load2(Rsrc r, unsigned byte_off) {  // 8 bytes at any 4-byte-aligned offset
  return __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, (int)byte_off, 0, 0));
}
// 12 bytes at vector offset + scalar offset (wave-uniform); AUX: the cache-policy bits (1 = sc0, 2 = nt, 16 = sc1), an immediate
template <int AUX = 0>
__device__ __forceinline__ v3f buf_load3(Rsrc r, unsigned voff, unsigned soff = 0) {
  return __builtin_bit_cast(v3f, __builtin_amdgcn_raw_buffer_load_b96(r, (int)voff, (int)soff, AUX));
}

// Both horizontal taps of a row come from ONE 8-byte load at column x0 (measured on gfx950, scripts/probes/buf_probe:
// unaligned 8/16-byte buffer loads work, the range check is per dword at the upper end, and an access that STARTS
// left of the row reads as all-zero).  The only column pair that needs help is x0 = -1, whose second tap (column 0) is
// inside the image: it is fetched as the first dword of a load at column 0.
struct TapPos {
  unsigned off;   // byte offset of the load
  bool edge;      // x0 == -1
};

__device__ __forceinline__ TapPos tap_pos(const ColTap& c) {
  TapPos p;
  p.edge = (c.x0 == -1);
  p.off = p.edge ? 0u : ((unsigned)c.x0 << 2);
  return p;
}

template <int NROWS>
__device__ __forceinline__ Taps<NROWS> load_taps(Rsrc rowA, Rsrc rowB, const TapPos& p) {
  Taps<NROWS> t;
  const v2f va = buf_load2(rowA, p.off);
  t.a0 = va.x; t.a1 = va.y;
  t.b0 = t.b1 = 0.0f;
  if (NROWS == 2) {
    const v2f vb = buf_load2(rowB, p.off);
    t.b0 = vb.x; t.b1 = vb.y;
  }
  return t;
}

// Apply the x0 = -1 fix-up after the data has arrived (kept out of the issue phase so it does not wait on the load).
template <int NROWS>
__device__ __forceinline__ void fix_edge(Taps<NROWS>& t, bool edge) {
  t.a1 = edge ? t.a0 : t.a1;
  t.a0 = edge ? 0.0f : t.a0;
  if (NROWS == 2) {
    t.b1 = edge ? t.b0 : t.b1;
    t.b0 = edge ? 0.0f : t.b0;
  }
}

// w0A/w1A(/w0B/w1B): horizontal weight x vertical weight, computed once per plane and shared by all five channels
struct TapW {
  float a0, a1, b0, b1;
};

template <int NROWS>
__device__ __forceinline__ TapW tap_weights(const ColTap& c, const RowSel& r, float live) {
  TapW w;
  const float w0 = c.w0 * live, w1 = c.w1 * live;  // live = 1, or 0 for a plane the padding mask removes
  w.a0 = (NROWS == 1) ? w0 : w0 * r.wA;           // one-row bodies run only where that row's weight is exactly 1
  w.a1 = (NROWS == 1) ? w1 : w1 * r.wA;
  w.b0 = w.b1 = 0.0f;
  if (NROWS == 2) {
    w.b0 = w0 * r.wB;
    w.b1 = w1 * r.wB;
  }
  return w;
}

template <int NROWS>
__device__ __forceinline__ float tap_value(const Taps<NROWS>& t, const TapW& w) {
  float v = t.a0 * w.a0 + t.a1 * w.a1;
  if (NROWS == 2) v += t.b0 * w.b0 + t.b1 * w.b1;
  return v;
}

// d value / d ix = (ne - nw) * wyA + (se - sw) * wyB   (out-of-image taps already read as zero)
template <int NROWS>
__device__ __forceinline__ float tap_dx(const Taps<NROWS>& t, const RowSel& r) {
  float d = t.a1 - t.a0;
  if (NROWS == 2) d = d * r.wA + (t.b1 - t.b0) * r.wB;
  return d;
}

// Colour rows in LDS: per live row W+4 float4 (r,g,b,-) with two zero guard cells on each side, so taps at
// x0 in [-2, W] need no validity handling either.  lds_off = byte offset of tap x0 in row A.
__device__ __forceinline__ unsigned colour_off(int x0, int W) {
  const int xc = min(max(x0, -2), W);  // v_med3_i32: far-out shifts land on a guard cell
  return (unsigned)(xc + 2) << 4;
}

// Raw colour taps of one plane (read from LDS in the issue phase, so their latency overlaps like the global loads')
template <int NROWS>
struct ColourTaps {
  float4 nw, ne, sw, se;
};

template <int NROWS>
__device__ __forceinline__ ColourTaps<NROWS> load_colour_taps(const char* __restrict__ lrgb, int W, unsigned off) {
  ColourTaps<NROWS> c;
  c.nw = *reinterpret_cast<const float4*>(lrgb + off);
  c.ne = *reinterpret_cast<const float4*>(lrgb + off + 16);
  if (NROWS == 2) {
    const unsigned rb = (unsigned)(W + 4) << 4;
    c.sw = *reinterpret_cast<const float4*>(lrgb + rb + off);
    c.se = *reinterpret_cast<const float4*>(lrgb + rb + off + 16);
  }
  return c;
}

template <int NROWS>
__device__ __forceinline__ void colour_values(const ColourTaps<NROWS>& t, const TapW& w, float& c0, float& c1,
                                              float& c2) {
  c0 = t.nw.x * w.a0 + t.ne.x * w.a1;
  c1 = t.nw.y * w.a0 + t.ne.y * w.a1;
  c2 = t.nw.z * w.a0 + t.ne.z * w.a1;
  if (NROWS == 2) {
    c0 += t.sw.x * w.b0 + t.se.x * w.b1;
    c1 += t.sw.y * w.b0 + t.se.y * w.b1;
    c2 += t.sw.z * w.b0 + t.se.z * w.b1;
  }
}

template <int NROWS>
__device__ __forceinline__ void colour_dx(const ColourTaps<NROWS>& t, const RowSel& r, float& d0, float& d1,
                                          float& d2) {
  d0 = t.ne.x - t.nw.x;
  d1 = t.ne.y - t.nw.y;
  d2 = t.ne.z - t.nw.z;
  if (NROWS == 2) {
    d0 = d0 * r.wA + (t.se.x - t.sw.x) * r.wB;
    d1 = d1 * r.wA + (t.se.y - t.sw.y) * r.wB;
    d2 = d2 * r.wA + (t.se.z - t.sw.z) * r.wB;
  }
}

// Shift of plane i along target row `yrow` of image b: sign * disparity through clamp_shift; under PD_MASK_ROWS the row's mask
// value overrides it (out of view).
__device__ __forceinline__ float staged_shift(const SweepArgs& a, int b, int i, int yrow) {
  const long di = (a.flags & PD_DISP_ROWS) ? ((long)b * a.N + i) * a.H + yrow : (long)b * a.N + i;
  const float sd = a.sign * a.plane[di];
  const bool masked = a.mask_rows && a.mask_rows[((long)b * a.N + i) * a.H + yrow] == 0.0f;
  return clamp_shift(sd, a.W, masked);
}

// Stage the live source colour rows of image b into LDS as float4 (with zero guard cells), plus the per-plane shifts
// sdisp[n] (staged_shift).
template <int NROWS>
__device__ __forceinline__ void stage_row_constants(const SweepArgs& a, int b, const RowSel& r, float4* __restrict__ lrgb,
                                                    float* __restrict__ sdisp, int yrow) {
  const int W = a.W, HW = a.H * a.W, RS = W + 4;
  const float* srcb = a.src + (long)b * 3 * HW;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    const float* p = srcb + (long)r.yA * W + x;
    lrgb[2 + x] = make_float4(p[0], p[HW], p[2 * HW], 0.0f);
    if (NROWS == 2) {
      const float* q = srcb + (long)r.yB * W + x;
      lrgb[RS + 2 + x] = make_float4(q[0], q[HW], q[2 * HW], 0.0f);
    }
  }
  if (threadIdx.x < 4) {
    const int g = (threadIdx.x < 2) ? threadIdx.x : W + threadIdx.x;  // cells 0,1 and W+2,W+3
    lrgb[g] = z;
    if (NROWS == 2) lrgb[RS + g] = z;
  }
  for (int i = threadIdx.x; i < a.N; i += blockDim.x) sdisp[i] = staged_shift(a, b, i, yrow);
}

// ---- the two stream kernels (pd_plane_sweep_fwdstream.hip, pd_plane_sweep_rowstream.hip): a lane owns two adjacent columns -------
struct StreamRow {     // workgroup-uniform: the target row a wave works on
  int b, y, yA, yB;
  float wA, wB, wy;    // vertical weights of the two source rows; adjoint weight of the own row (backward)
};
template <int NROWS>
__device__ __forceinline__ StreamRow make_stream_row(int b, int y, const RowSel& row) {
  StreamRow r;
  r.y = y;
  r.b = b;
  r.yA = row.yA; r.yB = (NROWS == 2) ? row.yB : row.yA;
  r.wA = row.wA; r.wB = (NROWS == 2) ? row.wB : 0.0f;
  r.wy = row.wy_main;
  return r;
}

// One slot of the tap ring: the taps of a lane's two columns on one plane, L[c .. c+2] per live source row, logits and sigma.
template <class T, int NROWS>
struct StreamTaps {
  float l[NROWS][3], s[NROWS][3];
};
// bf16 storage: the raw 8 bytes of ONE load per tensor and row, four elements from a 4-byte-aligned (even) column; the three taps
// are picked and widened when the plane is reduced (stream_taps), so a slot holds 2 VGPRs per tensor and row instead of 3.
template <int NROWS>
struct StreamTaps<Bf16, NROWS> {
  unsigned l[NROWS][2], s[NROWS][2];
};

// Issue the tap loads of plane n for row r into slot g: per tensor (sigma with MIX) and live source row ONE load at byte offset
// voff (per lane) + soff (wave-uniform) through a descriptor of Wx elements (the row's width; 0 turns the loads into hardware
// no-ops that return zeros), cache-policy bits AUX.  soff = 0, Wx = a.W and AUX = 0 fold to the plain per-lane load.
template <bool MIX, int NROWS, int AUX>
__device__ __forceinline__ void issue_taps(StreamTaps<float, NROWS>& g, const SweepArgs& a, const StreamRow& r, int n, unsigned voff,
                                           unsigned soff, int Wx, int HW) {
  auto ld = [&](const float* row, float (&t)[3]) {
    const v3f v = buf_load3<AUX>(row_rsrc(row, Wx), voff, soff);
    t[0] = v.x; t[1] = v.y; t[2] = v.z;
  };
  const float* pl = plane_ptr(a.logits + (long)r.b * a.N * HW, n, HW);
  ld(pl + (long)r.yA * a.W, g.l[0]);
  if (NROWS == 2) ld(pl + (long)r.yB * a.W, g.l[NROWS - 1]);
  if (MIX) {
    const float* ps = plane_ptr(a.sigma + (long)r.b * a.N * HW, n, HW);
    ld(ps + (long)r.yA * a.W, g.s[0]);
    if (NROWS == 2) ld(ps + (long)r.yB * a.W, g.s[NROWS - 1]);
  }
}
template <bool MIX, int NROWS, int AUX>
__device__ __forceinline__ void issue_taps(StreamTaps<Bf16, NROWS>& g, const SweepArgs& a, const StreamRow& r, int n, unsigned voff,
                                           unsigned soff, int Wx, int HW) {
  auto ld = [&](const Bf16* row, unsigned (&w)[2]) {
    const v2u v = __builtin_bit_cast(v2u, __builtin_amdgcn_raw_buffer_load_b64(row_rsrc_t(row, Wx), (int)voff, (int)soff, AUX));
    w[0] = v.x; w[1] = v.y;
  };
  const Bf16* pl = plane_ptr_t(elems<Bf16>(a.logits) + (long)r.b * a.N * HW, n, HW);
  ld(pl + (long)r.yA * a.W, g.l[0]);
  if (NROWS == 2) ld(pl + (long)r.yB * a.W, g.l[NROWS - 1]);
  if (MIX) {
    const Bf16* ps = plane_ptr_t(elems<Bf16>(a.sigma) + (long)r.b * a.N * HW, n, HW);
    ld(ps + (long)r.yA * a.W, g.s[0]);
    if (NROWS == 2) ld(ps + (long)r.yB * a.W, g.s[NROWS - 1]);
  }
}

// The three fp32 taps of a slot per row and tensor.  bf16: elements (0,1,2) of the loaded four, or (1,2,3) when the first tap sits
// at the odd column (`odd`, wave-uniform: the forward loads from the even column below an odd one; the backward never does).
__device__ __forceinline__ void bf16_taps3(const unsigned (&w)[2], bool odd, float (&t)[3]) {
  t[0] = odd ? bf16_hi(w[0]) : bf16_lo(w[0]);
  t[1] = odd ? bf16_lo(w[1]) : bf16_hi(w[0]);
  t[2] = odd ? bf16_hi(w[1]) : bf16_lo(w[1]);
}
template <int NROWS>
__device__ __forceinline__ void stream_taps(const StreamTaps<float, NROWS>& g, bool, float (&l)[NROWS][3], float (&s)[NROWS][3]) {
#pragma unroll
  for (int r = 0; r < NROWS; ++r)
#pragma unroll
    for (int i = 0; i < 3; ++i) { l[r][i] = g.l[r][i]; s[r][i] = g.s[r][i]; }
}
template <int NROWS>
__device__ __forceinline__ void stream_taps(const StreamTaps<Bf16, NROWS>& g, bool odd, float (&l)[NROWS][3], float (&s)[NROWS][3]) {
#pragma unroll
  for (int r = 0; r < NROWS; ++r) { bf16_taps3(g.l[r], odd, l[r]); bf16_taps3(g.s[r], odd, s[r]); }
}

// The colour cell both stream kernels stage in LDS: source colour at column x of the row's footprint, zero outside the row; with
// two live source rows (`two`) vertically blended as fl(B*wB + fl(A*wA)) — the rounding of the four-tap sum of the target-ordered
// kernels when the column weights are (1, 0): with tgt == src and a zero disparity, sign(c - t) sits on the last ulp (DESIGN.md
// section 5, knife edge (d)), so the forward and the backward must stage the same bits.
__device__ __forceinline__ float4 blended_colour(const float* __restrict__ srcb, const RowSel& row, bool two, int x, int W, int HW) {
  float4 cc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (x >= 0 && x < W) {
    const float* p = srcb + (long)row.yA * W + x;
    cc = make_float4(p[0], p[HW], p[2 * HW], 0.0f);
    if (two) {
      const float* q = srcb + (long)row.yB * W + x;
      cc = make_float4(fmaf(q[0], row.wB, cc.x * row.wA), fmaf(q[HW], row.wB, cc.y * row.wA), fmaf(q[2 * HW], row.wB, cc.z * row.wA), 0.0f);
    }
  }
  return cc;
}

}  // namespace pd
