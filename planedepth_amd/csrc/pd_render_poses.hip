// Novel views at inference for arbitrary camera poses: from the decoder's conv outputs (or logits / sigma a tail already
// produced), the planes' distances and normals and the source image to V rendered views, one per 6-DoF pose T[b,v] — the
// reference's pred_novel_images with warp_type == "homography_warp" (trainer.py:556-603, layers.py:206-234) on the tail of
// DepthDecoder.forward (depth_decoder.py:256-291), forward only:
//   logits = raw_logits * mask; sigma = clamp(sigmoid(raw_sigma), .01, 1)       (per tap; skipped with PD_RENDER_TAIL_APPLIED)
//   per plane n: p = H_t2s [x,y,1]; mask = (K^-1 [x,y,1] . (R n) > 0) & (z > 1e-7); z clamped to 1e-7; the reference's normalise /
//   un-normalise round trip; bilinear, zeros padding: colour, logit, sigma and a ones image, each times mask
//   p_n = softmax_N(logit_rec) [/ clamp(sigma_rec, .01, 1), renormalised];  rgb = sum p_n colour_n;  coverage = sum p_n ones_n;
//   disp = sum p_n max(a x + b y + c, 0)   (the plane's inverse depth in the NEW camera as a rig disparity, 0.1 * 0.58 * W / z_t)
// Nothing [B,N,H,W]-sized is written, no atomics.
//
// Two launches.  render_poses_setup_kernel: one thread per (image, view, plane) writes a 16-float record into the workspace —
// H_t2s (9) and R n (3) with the fp64 chain of pd_homography_chain.h, the bits pd_homography_matrices_fwd(PD_HMAT_PLANES) writes for
// that pose; (a, b, c) = 0.1 * 0.58 * W * (K^-1)^T (R n) / d_t with d_t = d + (R n) . t, formed in fp64 and rounded once, 0 for
// d_t <= 0 (the plane lies behind the new camera); a validity word, 0 where the matrix is not finite or not invertible (d_t = 0:
// the new camera's centre lies on the plane), which masks the plane everywhere in that view.
// render_poses_kernel: one lane per target pixel, one workgroup per 256 pixels of one (image, view), the grid image-major so
// that the views of an image run next to each other and find its conv outputs in the cache.  A lane streams over the planes:
// the record is wave-uniform (scalar loads), the per-pixel chain is plane_coords<PD_WARP_HOMOGRAPHY>'s arithmetic (hrow_dot,
// facing_dot, normalise_roundtrip_rcp), the four taps come straight from memory with the tail step applied to each (a sample of
// sigmoid(x) is not sigmoid of a sample), and an online softmax keeps the view's state as in pd_render_views.  A view is its
// own set of workgroups, so its bits cannot depend on V or on the other views of the launch.
#include "pd_decoder_tail.h"
#include "pd_homography_chain.h"
#include "pd_sweep_geom.h"

namespace pd {

constexpr int kPoseRecord = 16;   // floats per (image, view, plane): H_t2s 0..8, R n 9..11, (a, b, c) 12..14, valid 15

struct PoseArgs {
  int B, N, H, W, V;
  int visible;        // PD_RENDER_VISIBLE_ONLY
  const float* logits;
  const float* sigma;
  const float* mask;  // [B,N,H] or NULL
  const float* image;
  const float* inv_K;
  const float* rec;
  float* rgb;
  float* coverage;
  float* disp;
};

__global__ __launch_bounds__(kBlock) void render_poses_setup_kernel(int B, int N, int V, int W, const float* __restrict__ distance,
                                                                    const float* __restrict__ norm, const float* __restrict__ T,
                                                                    const float* __restrict__ K, const float* __restrict__ inv_K,
                                                                    float* __restrict__ rec) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long)B * V * N) return;
  const int n = (int)(i % N);
  const long bv = i / N;
  const int b = (int)(bv / V);
  const long k = (long)b * N + n;
  const float* Tp = T + bv * 16;
  PlaneOf p;
  p.n[0] = norm[k * 3 + 0], p.n[1] = norm[k * 3 + 1], p.n[2] = norm[k * 3 + 2], p.d = distance[k];
  const Chain c = homography_chain_at(Tp, K + (long)b * 16, inv_K + (long)b * 16, p);
  float rn[3];
  rotated_normal(Tp, norm, k, rn);
  double nt[3], dt = p.d;   // n_t = R n, d_t = d + n_t . t: the plane in the new camera's frame (X_t = R X_s + t)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    nt[r] = (double)Tp[r * 4 + 0] * p.n[0] + (double)Tp[r * 4 + 1] * p.n[1] + (double)Tp[r * 4 + 2] * p.n[2];
    dt += nt[r] * c.t[r];
  }
  float* out = rec + i * kPoseRecord;
  bool ok = (dt == dt) && fabs(dt) < 1e30 && dt != 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float h = (float)c.H.m[r][q];
      out[r * 3 + q] = h;
      ok = ok && (fabsf(h) < 1e30f);   // (false for a NaN)
    }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    out[9 + r] = rn[r];
    ok = ok && (fabsf(rn[r]) < 1e30f);
  }
  const double s = 0.1 * 0.58 * (double)W / dt;
#pragma unroll
  for (int q = 0; q < 3; ++q) {   // column q of K^-1 against n_t
    const float v = (float)(s * (c.Ki.m[0][q] * nt[0] + c.Ki.m[1][q] * nt[1] + c.Ki.m[2][q] * nt[2]));
    out[12 + q] = (ok && dt > 0.0 && fabsf(v) < 1e30f) ? v : 0.0f;
  }
  out[15] = ok ? 1.0f : 0.0f;
}

__device__ __forceinline__ float tap_elem(const float* __restrict__ p, unsigned byte_off) { return at_byte(p, byte_off); }
__device__ __forceinline__ float tap_elem(const Bf16* __restrict__ p, unsigned byte_off) {   // byte_off counts 4-byte elements
  return __uint_as_float((unsigned)*reinterpret_cast<const Bf16*>(reinterpret_cast<const char*>(p) + (byte_off >> 1)) << 16);
}
// the four taps' blend, in one fixed order
__device__ __forceinline__ float tap_blend(float v00, float v01, float v10, float v11, const TapK& k) {
#pragma clang fp contract(off)
  return fmaf(v11, k.w11, fmaf(v10, k.w10, fmaf(v01, k.w01, v00 * k.w00)));
}

template <class ST, bool MIX, bool RAW>
__global__ __launch_bounds__(kBlock) void render_poses_kernel(PoseArgs a) {
  const int W = a.W, H = a.H, N = a.N, HW = H * W;
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= HW) return;
  const int bv = blockIdx.y, b = bv / a.V;
  const int y = pix / W, x = pix - y * W;
  const float fx = (float)x, fy = (float)y;
  const float* Ki = a.inv_K + (long)b * 16;
  const float r0 = hrow_dot(Ki[0], Ki[1], Ki[2], fx, fy);
  const float r1 = hrow_dot(Ki[4], Ki[5], Ki[6], fx, fy);
  const float r2 = hrow_dot(Ki[8], Ki[9], Ki[10], fx, fy);
  const CoordNorm cn = make_coord_norm(W, H);   // (H, W >= 2: the reciprocal form)

  const float* srcb = a.image + (long)b * 3 * HW;
  const ST* lg = elems<ST>(a.logits) + (long)b * N * HW;
  const ST* sg = MIX ? elems<ST>(a.sigma) + (long)b * N * HW : nullptr;
  const float* mrow = (RAW && a.mask) ? a.mask + (long)b * N * H : nullptr;
  const float* rec = a.rec + (long)bv * N * kPoseRecord;

  float m = -INFINITY, Sw = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, cov = 0.0f, dsum = 0.0f;
  for (int n = 0; n < N; ++n) {
    const float* r = rec + n * kPoseRecord;
    const float p0 = hrow_dot(r[0], r[1], r[2], fx, fy);
    const float p1 = hrow_dot(r[3], r[4], r[5], fx, fy);
    const float z = hrow_dot(r[6], r[7], r[8], fx, fy);
    const float facing = facing_dot(r0, r1, r2, r[9], r[10], r[11]);
    const bool mk = (r[15] != 0.0f) && (facing > 0.0f) && (z > kZMin);
    if (a.visible && !mk) continue;   // PD_RENDER_VISIBLE_ONLY: no part at all
    float l = 0.0f, s = 0.0f, k0 = 0.0f, k1 = 0.0f, k2 = 0.0f, kc = 0.0f;   // a masked plane: all-zero features (trainer.py:580)
    if (mk) {
      const float zc = (z < kZMin) ? kZMin : z;
      const float ix = normalise_roundtrip_rcp(p0 / zc, cn.Wm1, cn.rcpW);
      const float iy = normalise_roundtrip_rcp(p1 / zc, cn.Hm1, cn.rcpH);
      const Tap tp = make_tap(ix, iy, W, H);
      const TapK t = tap_kernel(tp, W, H);
      const ST* pl = lg + (unsigned)(n * HW);
      float l00 = tap_elem(pl, t.o00), l01 = tap_elem(pl, t.o01), l10 = tap_elem(pl, t.o10), l11 = tap_elem(pl, t.o11);
      if (mrow) {   // depth_decoder.py:259 on the taps' own rows
        const float mA = mrow[n * H + min(max(tp.y0, 0), H - 1)], mB = mrow[n * H + min(max(tp.y0 + 1, 0), H - 1)];
        l00 *= mA; l01 *= mA; l10 *= mB; l11 *= mB;
      }
      l = tap_blend(l00, l01, l10, l11, t);
      if (MIX) {
        const ST* ps = sg + (unsigned)(n * HW);
        float s00 = tap_elem(ps, t.o00), s01 = tap_elem(ps, t.o01), s10 = tap_elem(ps, t.o10), s11 = tap_elem(ps, t.o11);
        if (RAW) {   // :278-279
          s00 = clamp_sigma(sigmoid_f(s00)); s01 = clamp_sigma(sigmoid_f(s01));
          s10 = clamp_sigma(sigmoid_f(s10)); s11 = clamp_sigma(sigmoid_f(s11));
        }
        s = tap_blend(s00, s01, s10, s11, t);
      }
      k0 = tap_blend(at_byte(srcb, t.o00), at_byte(srcb, t.o01), at_byte(srcb, t.o10), at_byte(srcb, t.o11), t);
      k1 = tap_blend(at_byte(srcb + HW, t.o00), at_byte(srcb + HW, t.o01), at_byte(srcb + HW, t.o10), at_byte(srcb + HW, t.o11), t);
      k2 = tap_blend(at_byte(srcb + 2 * HW, t.o00), at_byte(srcb + 2 * HW, t.o01), at_byte(srcb + 2 * HW, t.o10),
                     at_byte(srcb + 2 * HW, t.o11), t);
      kc = tap_blend(1.0f, 1.0f, 1.0f, 1.0f, t);   // the ones image
    }
    const float dn = fmaxf(fmaf(r[12], fx, fmaf(r[13], fy, r[14])), 0.0f);
    if (l > m) {   // move the reference to the new maximum
      const float sc = __expf(m - l);
      Sw *= sc; c0 *= sc; c1 *= sc; c2 *= sc; cov *= sc; dsum *= sc;
      m = l;
    }
    float w = __expf(l - m);
    if (MIX) w = w * fast_rcp(clamp_sigma(s));   // trainer.py:597-600
    Sw += w;
    c0 = fmaf(w, k0, c0);
    c1 = fmaf(w, k1, c1);
    c2 = fmaf(w, k2, c2);
    cov = fmaf(w, kc, cov);
    dsum = fmaf(w, dn, dsum);
  }
  const float inv = (Sw > 0.0f) ? 1.0f / Sw : 0.0f;   // (Sw = 0: PD_RENDER_VISIBLE_ONLY at a pixel no plane reaches)
  a.rgb[((long)bv * 3 + 0) * HW + pix] = c0 * inv;
  a.rgb[((long)bv * 3 + 1) * HW + pix] = c1 * inv;
  a.rgb[((long)bv * 3 + 2) * HW + pix] = c2 * inv;
  if (a.coverage) a.coverage[(long)bv * HW + pix] = cov * inv;
  if (a.disp) a.disp[(long)bv * HW + pix] = dsum * inv;
}

template <class ST, bool MIX>
static int render_poses_launch(const PoseArgs& a, bool raw, hipStream_t stream) {
  const dim3 grid(ceil_div(a.H * a.W, kBlock), a.B * a.V);
  if (raw) render_poses_kernel<ST, MIX, true><<<grid, kBlock, 0, stream>>>(a);
  else render_poses_kernel<ST, MIX, false><<<grid, kBlock, 0, stream>>>(a);
  return check_launch("render_poses_kernel");
}

}  // namespace pd

using namespace pd;

extern "C" size_t pd_render_poses_workspace_floats(int B, int N, int V) {
  if (B < 1 || N < 1 || V < 1) return 0;
  return (size_t)kPoseRecord * (size_t)B * (size_t)V * (size_t)N;
}

extern "C" int pd_render_poses(int B, int N, int H, int W, int V, int flags, const float* logits_in, const float* sigma_in,
                               const float* mask_rows, const float* distance, const float* norm, const float* T, const float* K,
                               const float* inv_K, const float* image, float* rgb, float* coverage, float* disp, float* workspace,
                               pd_stream_t stream) {
  PD_REQUIRE(B > 0 && N > 0 && H > 1 && W > 1, "bad shape (B >= 1, N >= 1, H >= 2, W >= 2)");
  PD_REQUIRE(V >= 1, "V = %d: a launch renders at least one view", V);
  PD_REQUIRE((long)B * V <= 65535, "B*V = %ld: the grid takes at most 65535 (image, view) pairs per launch", (long)B * V);
  PD_REQUIRE(!(flags & PD_TAIL_DISP_ROWS), "flags: PD_TAIL_DISP_ROWS has no meaning here (planes come in as distance / norm)");
  PD_REQUIRE(!(flags & PD_TAIL_DISP_DENSE), "flags: PD_TAIL_DISP_DENSE has no meaning here (planes come in as distance / norm)");
  PD_REQUIRE((flags & ~(PD_TAIL_MIXTURE | PD_TAIL_BF16 | PD_TAIL_MASK_ROWS | PD_RENDER_TAIL_APPLIED | PD_RENDER_VISIBLE_ONLY)) == 0,
             "unknown flags");
  PD_REQUIRE(!(flags & PD_TAIL_MASK_ROWS) || mask_rows, "NULL pointer (PD_TAIL_MASK_ROWS in flags: mask_rows is read as [B,N,H])");
  PD_REQUIRE((flags & PD_TAIL_MASK_ROWS) || !mask_rows,
             "mask_rows without PD_TAIL_MASK_ROWS in flags (the only mask form is [B,N,H]; NULL = all ones)");
  PD_REQUIRE(!(flags & PD_TAIL_MIXTURE) || sigma_in, "NULL pointer (PD_TAIL_MIXTURE in flags: the mixture needs sigma_in)");
  PD_REQUIRE(workspace, "NULL pointer (workspace: pd_render_poses_workspace_floats(B, N, V) floats)");
  PD_REQUIRE(T, "NULL pointer (T: [B,V,4,4])");
  PD_REQUIRE(K, "NULL pointer (K: [B,4,4])");
  PD_REQUIRE(inv_K, "NULL pointer (inv_K: [B,4,4])");
  PD_REQUIRE(distance, "NULL pointer (distance: [B,N])");
  PD_REQUIRE(norm, "NULL pointer (norm: [B,N,3])");
  PD_REQUIRE(logits_in && image && rgb, "NULL pointer (logits_in, image and rgb are required; coverage and disp may be NULL)");
  PD_REQUIRE((long)N * H * W < (1L << 31), "N*H*W = %ld: a plane set of 2^31 elements or more is not addressable here",
             (long)N * H * W);
  const uintptr_t st_mask = (flags & PD_TAIL_BF16) ? 1 : 3;
  PD_REQUIRE(!((reinterpret_cast<uintptr_t>(logits_in) | reinterpret_cast<uintptr_t>(sigma_in)) & st_mask),
             "misaligned pointer (logits_in / sigma_in: %d-byte elements)", (int)st_mask + 1);
  PD_REQUIRE(!((reinterpret_cast<uintptr_t>(mask_rows) | reinterpret_cast<uintptr_t>(distance) | reinterpret_cast<uintptr_t>(norm) |
                reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(inv_K) |
                reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(workspace)) & 3),
             "misaligned pointer (mask_rows, distance, norm, T, K, inv_K, image, workspace: 4-byte elements)");
  PD_REQUIRE(!((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(coverage) | reinterpret_cast<uintptr_t>(disp)) & 3),
             "misaligned pointer (rgb, coverage, disp: 4-byte elements)");

  const hipStream_t s = (hipStream_t)stream;
  const long records = (long)B * V * N;
  render_poses_setup_kernel<<<(unsigned)((records + kBlock - 1) / kBlock), kBlock, 0, s>>>(B, N, V, W, distance, norm, T, K, inv_K,
                                                                                          workspace);
  if (int rc = check_launch("render_poses_setup_kernel")) return rc;

  PoseArgs a;
  a.B = B; a.N = N; a.H = H; a.W = W; a.V = V;
  a.visible = (flags & PD_RENDER_VISIBLE_ONLY) != 0;
  a.logits = logits_in; a.sigma = sigma_in; a.mask = mask_rows; a.image = image; a.inv_K = inv_K; a.rec = workspace;
  a.rgb = rgb; a.coverage = coverage; a.disp = disp;
  const bool raw = !(flags & PD_RENDER_TAIL_APPLIED);
  if (flags & PD_TAIL_BF16)
    return (flags & PD_TAIL_MIXTURE) ? render_poses_launch<Bf16, true>(a, raw, s) : render_poses_launch<Bf16, false>(a, raw, s);
  return (flags & PD_TAIL_MIXTURE) ? render_poses_launch<float, true>(a, raw, s) : render_poses_launch<float, false>(a, raw, s);
}
