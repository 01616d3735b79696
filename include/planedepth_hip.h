/*
 * planedepth_hip.h — C ABI of the MI355X (gfx950) implementation of PlaneDepth's
 * photometric-reconstruction hot path.
 *
 * The reference (svip-lab/PlaneDepth) has NO native/FFI boundary for this path: it is
 * Python calling stock ATen ops.  This header is therefore the
 * boundary a maintainer would bind with ctypes; every entry point
 * cites the reference code it replaces.
 *
 * Conventions
 *   - all tensors are fp32, contiguous NCHW device pointers owned by the caller
 *     (outputs are caller-allocated; nothing is allocated, freed or synchronised here) — except, under PD_LOGITS_BF16,
 *     the sweep's logits / sigma / g_logits / g_sigma, which then hold bf16 bit patterns (see the flag);
 *   - `stream` is a hipStream_t (0 = the null stream); launches are asynchronous;
 *   - every function returns PD_OK (0) or a PD_ERR_* code; pd_last_error() returns a
 *     thread-local human-readable message for the last non-zero return on this thread;
 *   - safe to call from any thread (e.g. the autograd thread) and for any device: the entry points work on the CURRENT
 *     device (hipSetDevice / torch.cuda.device by the caller) and keep nothing between calls except per-device caches of
 *     device facts — the LDS a workgroup can be given, the dynamic-LDS limit already granted to a kernel — held in
 *     atomics indexed by the device ordinal (the rare raise is serialised by a mutex).  The two process-environment
 *     switches (PD_PP_SEG, PD_ROW_EPS) are read ONCE, when the library is first used, never on the launch path; kernel
 *     selection per call goes through pd_sweep_desc.impl.
 */
#ifndef PLANEDEPTH_HIP_H
#define PLANEDEPTH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pd_stream_t; /* hipStream_t */

enum pd_status {
  PD_OK = 0,
  PD_ERR_ARG = 1,         /* NULL pointer / bad shape / bad enum */
  PD_ERR_UNSUPPORTED = 2, /* valid request this build does not implement */
  PD_ERR_LAUNCH = 3       /* hipGetLastError() != hipSuccess after a launch */
};

/* How the per-plane sampling grid is generated (reference: opt.warp_type, trainer.py:533-560). */
enum pd_warp_mode {
  PD_WARP_DISP = 0,      /* trainer.py:540-554: x -> x + sign*disp_layered, y unchanged          */
  PD_WARP_HOMOGRAPHY = 1 /* layers.py:221-233: p = H_t2s [x,y,1]^T, projective divide, mask      */
};

enum pd_sweep_flags {
  PD_MIXTURE = 1,     /* opt.use_mixture_loss: sigma channel, Laplacian-mixture NLL (trainer.py:594-602, 728-730) */
  PD_AUTOMASK = 2,    /* opt.automask: min with the identity-reprojection loss (trainer.py:731-734, 739-741)      */
  PD_RENDER_PROB = 4, /* opt.render_probability: alpha compositing instead of softmax (trainer.py:584-591)        */
  PD_DISP_DENSE = 8,  /* disp mode: `plane` is a dense [B,N,H,W] map (xz/yz planes) instead of [B,N] scalars      */
  PD_DISP_ROWS = 16,  /* disp mode: `plane` is [B,N,H], one disparity per plane and ROW (xy + xz planes: the decoder's
                         map is constant along x, depth_decoder.py:153-181).  Only where pd_sweep_uses_rowshift() */
  PD_MASK_ROWS = 32   /* disp mode: `padding_mask` is [B,N,H], one value per plane and row (the xz horizon mask is
                         constant along x, depth_decoder.py:166).  Only where pd_sweep_uses_rowshift(): a masked plane
                         row is treated as shifted out of view, so the mask costs no per-pixel traffic at all */
  ,
  PD_HOMO_UNIFORM = 64 /* homography mode: every plane of an image shares ONE homography.  What Trainer.predict_poses hands
                         over for the novel frames without COLMAP: zero translation (trainer.py:386-400), hence
                         K (R + t n^T/d) K^-1 = K R K^-1 for every plane.  `plane` is [B,4,3,3]: slice 0 = H_t2s, slices
                         1..3 = the homographies of virtual planes with n/d = e_0, e_1, e_2 (same values at t = 0);
                         `plane_aux` stays [B*N,3] (the facing test depends on the plane's normal); `padding_mask` carries
                         the [B,N,3] weights n_n/d_n or NULL.  g_plane [B,4,3,3] = (sum_n G_n, sum_n G_n n_n[j]/d_n):
                         back-propagated through f(R + t e_j^T) it gives the exact translation gradient of the per-plane
                         formulation.  Served by pd_plane_sweep_uniform.hip: geometry once per pixel, atomic-free
                         two-pass backward */
  ,
  PD_BWD_ACCUMULATE = 128 /* pd_plane_sweep_bwd only: g_logits / g_sigma are ADDED TO instead of overwritten, so the target
                         views of one step (trainer.py:532: the same logits / sigma feed every side) sum their
                         gradients in place instead of through [B,N,H,W]-sized add kernels.  Honoured where
                         pd_sweep_bwd_accumulates() says so (the plane-uniform kernels: read-modify-write stores; the
                         general kernels: their atomics simply skip the zero-fill); refused elsewhere */
  ,
  PD_BWD_DEFER_GATHER = 256 /* pd_plane_sweep_bwd, PD_HOMO_UNIFORM only: run the first pass (per-pixel plane gradients into the
                         scratch inside `workspace`, g_plane, g_dists) and leave g_logits / g_sigma untouched; the caller
                         then hands the workspaces of TWO such calls over the same logits / sigma to
                         pd_uniform_gather_pair, which gathers both views in one kernel (one store per gradient element
                         instead of a read-modify-write per view) */
  ,
  PD_PH_MEAN_ZEROED = 512 /* pd_plane_sweep_fwd: the caller hands `ph_mean` over holding 0.0f already (e.g. a slot of a buffer it
                         zeroed once for many calls): the kernels add into it, and the entry point then issues no memset
                         launch of its own (4-5 us per call next to a 0.1 ms kernel).  Ignored by the other entry points */
  ,
  PD_BWD_PLANE_ZEROED = 1024 /* pd_plane_sweep_bwd / _bwd_tail / _bwd_tail_rows, PD_WARP_DISP with one disparity per plane: the caller hands `g_plane`
                         [B,N] over holding zeros (e.g. a slice of a buffer it zeroed once for many calls).  Where
                         pd_sweep_bwd_plane_adds(d) == 1 (the row-stream backward) every row workgroup then ADDS its share with
                         atomics and the entry point launches no reduction kernel of its own (4-5 us + a launch gap per call next
                         to a 0.18 ms kernel; the sum's order, hence its last bits, varies from run to run); elsewhere the kernels
                         overwrite `g_plane` as always — the promise is harmless there */,
  PD_LOGITS_BF16 = 2048 /* pd_plane_sweep_fwd / _bwd: `logits`, `sigma`, `g_logits` and `g_sigma` hold bf16 (torch.bfloat16) bit
                         patterns, 4-byte aligned; everything else stays fp32 (src, tgt, plane, padding mask, dists, rgb_rec,
                         ph_map, ph_mean, stash, workspace, g_plane).  The arithmetic is the fp32 kernels': a bf16 element widens
                         exactly on load, and every gradient element is rounded to bf16 ONCE (round to nearest even) from the
                         fp32 value that holds all of its contributions — no bf16 read-modify-write, no bf16 atomics — so the
                         gradients equal the fp32 route's on the widened inputs rounded once.  Served where
                         pd_sweep_native_bf16(d) == 1 (the segment-stream forward and the row-stream backward); elsewhere, with
                         a per-pixel padding mask, with PD_BWD_ACCUMULATE / PD_BWD_DEFER_GATHER and in pd_plane_sweep_bwd_tail
                         and the pair entry points the call returns PD_ERR_UNSUPPORTED naming the flag */
};

enum pd_padding_mode { PD_PAD_ZEROS = 0, PD_PAD_BORDER = 1 };

/* Kernel selection.  The row kernels apply to PD_WARP_DISP with per-plane or per-row disparities (forward:
 * pd_plane_sweep_fwdstream.hip, a wave per 128-pixel segment streaming over the planes — pd_plane_sweep_rowshift.hip,
 * plane groups, with a per-pixel mask or PD_RENDER_PROB; backward: pd_plane_sweep_rowstream.hip, source-ordered); homography_warp
 * with one matrix per image (PD_HOMO_UNIFORM) or per plane runs a two-pass gather backward without atomics
 * (pd_plane_sweep_uniform.hip, pd_plane_sweep_gather.hip); the general kernels handle everything (and are the
 * cross-check for the specialised ones in the tests). */
enum pd_sweep_impl {
  PD_IMPL_AUTO = 0,      /* the specialised kernels where they apply, exact footprints (default) */
  PD_IMPL_GENERAL = 1,   /* general kernels only: atomic scatter in the backward (the cross-check in the tests) */
  PD_IMPL_FAST_ROWS = 2  /* as AUTO, but a second source row whose bilinear weight is below 2^-16 (fp32 noise of the
                            reference's y round trip, <= 6e-6) is dropped: ~11% faster, results within 1e-4 of the
                            tensors' range on random inputs instead of 1e-6 (opt-in) */
  ,
  PD_IMPL_TILE = 3       /* REMOVED: the backward returns PD_ERR_UNSUPPORTED (the value stays reserved).  It selected the
                            owned-tile homography backward (LDS accumulators per source tile, plain stores, no zero-fill):
                            exact and atomic-free in HBM, but 2-2.5x SLOWER on gfx950 (ds_add_f32 costs ~110 cycles per
                            wave instruction: NOTEBOOK.md 3.4.6) */
  ,
  PD_IMPL_ROWS1 = 4      /* as AUTO, but forward and backward are the target-ordered, one-pixel-per-lane row-shift kernels
                            (pd_plane_sweep_rowshift.hip, the headline kernels of rounds 1-2) instead of the segment-stream
                            forward (pd_plane_sweep_fwdstream.hip) and the source-ordered row-stream backward
                            (pd_plane_sweep_rowstream.hip): cross-check and A/B runs */
  ,
  PD_IMPL_UNIFORM_DIRECT = 5 /* as AUTO, but pass 2 of the two-pass homography backwards (plane-uniform and per-plane) gathers
                            directly from the scratch instead of staging it through LDS (the form large boxes fall back
                            to anyway): cross-check */
  ,
  PD_IMPL_EXACT_ROWS = 6 /* as AUTO, with every second source row served whatever its weight: the reference's last-ulp row
                            weights (the y round trip of trainer.py:552 + grid_sample returns y + e, |e| <= 6e-6, on a
                            quarter of the rows at H = 192).  What AUTO itself does about those rows is stated at
                            PD_IMPL_AUTO / pd_sweep_auto_fast_rows() */
};

/* The bilinear weight below which PD_IMPL_AUTO (and the impls documented "as AUTO") drops a second source row: 0 = never
 * (as PD_IMPL_EXACT_ROWS); PD_IMPL_FAST_ROWS uses 2^-16. */
float pd_sweep_auto_row_eps(void);

typedef struct pd_sweep_desc {
  int32_t B, N, H, W;
  int32_t mode;  /* pd_warp_mode */
  int32_t flags; /* OR of pd_sweep_flags */
  float sign;    /* PD_WARP_DISP: +1 for target "r" (x + d), -1 for target "l" (x - d), 0 = grid untouched */
  int32_t impl;  /* pd_sweep_impl: 0 = pick the fastest applicable kernels, 1 = force the general (atomic) kernels */
} pd_sweep_desc;

int pd_version(void);
const char* pd_last_error(void);
/* sha256[:16] over the kernel sources and headers this library was compiled from (the .hip and .h files under csrc/ and
 * include/: __graft_entry__.source_hash), baked in at build time (-DPD_SRC_HASH); "unknown" for a build without it. */
const char* pd_source_hash(void);
/* Always 0.  It reported a library built with the kernels that lost their A/B runs, which are no longer part of the
 * sources; kept so that callers that check it keep working. */
int pd_experiments(void);
/* Always 0.  It reported experiments (1) and timing-ablation / trace builds (2, results wrong by design), neither of which
 * can be built any more; kept because bench.py's `library` block and tests/test_capi.py read it. */
int pd_build_flags(void);

/* 1 if pd_plane_sweep_bwd adds into a pre-zeroed g_plane under PD_BWD_PLANE_ZEROED for this descriptor (see the flag; a
 * per-pixel padding mask sends the call to a kernel that overwrites instead), else 0. */
int pd_sweep_bwd_plane_adds(const pd_sweep_desc* d);
/* 1 if pd_plane_sweep_bwd honours PD_BWD_ACCUMULATE for this descriptor (see the flag), else 0. */
int pd_sweep_bwd_accumulates(const pd_sweep_desc* d);
/* 1 if this descriptor is served by the row-shift kernels (PD_WARP_DISP, scalar or per-row disparities), else 0. */
int pd_sweep_uses_rowshift(const pd_sweep_desc* d);
/* 1 if PD_LOGITS_BF16 is served for this descriptor (the flag itself need not be set in d->flags), else 0: PD_WARP_DISP with
 * per-plane disparities or PD_DISP_ROWS (with or without PD_MASK_ROWS), mixture or L1, with or without automask, impl AUTO /
 * FAST_ROWS / EXACT_ROWS, no PD_RENDER_PROB, even W, and a row whose LDS fits.  Needs no GPU. */
int pd_sweep_native_bf16(const pd_sweep_desc* d);

/* Floats per image the forward pass stashes for the backward pass (softmax statistics + mask bits). */
size_t pd_sweep_stash_floats(const pd_sweep_desc* d);
/* Floats of scratch pd_plane_sweep_bwd needs for its per-block partial reductions of the plane-parameter gradient. */
size_t pd_sweep_bwd_workspace_floats(const pd_sweep_desc* d);

/*
 * Fused replacement for Trainer.pred_novel_images (trainer.py:523-603, one target view) plus the photometric part
 * of Trainer.compute_losses (trainer.py:717-742) — SURVEY.md rows A1, A2/A3, A5-A9.
 *
 *   src, tgt      [B,3,H,W]  source colour (inputs[(color,"l")]) and target colour
 *   logits        [B,N,H,W]  outputs["logits"];  sigma [B,N,H,W] outputs["sigma"] (NULL unless PD_MIXTURE)
 *   plane         PD_WARP_DISP:       outputs["disp_layered"] as [B,N] ([B,N,H,W] with PD_DISP_DENSE, [B,N,H] with
 *                                     PD_DISP_ROWS)
 *                 PD_WARP_HOMOGRAPHY: H_t2s [B*N,3,3] (layers.py:219)
 *   plane_aux     PD_WARP_HOMOGRAPHY: R·n [B*N,3] (layers.py:223); else NULL
 *   inv_K3        PD_WARP_HOMOGRAPHY: inv_K[:, :3, :3] as [B,3,3]; else NULL
 *   padding_mask  PD_WARP_DISP: outputs["padding_mask"] [B,N,H,W] float 0/1, or NULL (= all ones);
 *                 PD_WARP_HOMOGRAPHY: must be NULL (the mask is computed, layers.py:223-226)
 *   dists         [B,N-1,H,W] outputs["dists"] with PD_RENDER_PROB, else NULL
 * outputs
 *   rgb_rec       [B,3,H,W]  outputs[("rgb_rec", side)]
 *   ph_map        [B,1,H,W]  per-pixel photometric loss BEFORE the mean / mask_novel product of trainer.py:735-742
 *   ph_mean       [1] or NULL: mean(ph_map), i.e. the `.mean()` of trainer.py:742 fused into the sweep (block sums and
 *                 one fp32 atomic per wave: the last bits depend on the order; use ph_map where that matters)
 *   stash         [B, pd_sweep_stash_floats/(H*W), H, W] opaque, consumed by pd_plane_sweep_bwd
 */
int pd_plane_sweep_fwd(const pd_sweep_desc* d, const float* src, const float* tgt, const float* logits,
                       const float* sigma, const float* plane, const float* plane_aux, const float* inv_K3,
                       const float* padding_mask, const float* dists, float* rgb_rec, float* ph_map, float* ph_mean,
                       float* stash, pd_stream_t stream);

/*
 * Backward of the above: what autograd computes through trainer.py:567-603 + 728-742 in the reference
 * (grid_sampler_2d_backward, softmax/clamp/div/sum/log/abs backward ...).
 *   g_rgb_rec [B,3,H,W] upstream gradient of rgb_rec (perceptual loss etc.), may be NULL (= zeros)
 *   g_ph_map  [B,1,H,W] upstream gradient of ph_map, may be NULL (= zeros)
 *   g_ph_mean [1] device scalar: upstream gradient of ph_mean, may be NULL (= zero); both gradients add up
 * outputs (each may be NULL to skip it)
 *   g_logits, g_sigma  [B,N,H,W]  — fully overwritten
 *   g_plane            same shape as `plane` (disp: [B,N] or dense [B,N,H,W]; homography: [B*N,3,3]) — overwritten
 *   g_dists            [B,N-1,H,W] gradient of `dists` (PD_RENDER_PROB only) — overwritten
 *   workspace          pd_sweep_bwd_workspace_floats(d) floats of scratch (partial sums of g_plane; boundary spill of
 *                      the row-shift kernels) — uninitialised is fine, one per concurrent call
 */
int pd_plane_sweep_bwd(const pd_sweep_desc* d, const float* src, const float* tgt, const float* logits,
                       const float* sigma, const float* plane, const float* plane_aux, const float* inv_K3,
                       const float* padding_mask, const float* dists, const float* rgb_rec, const float* stash,
                       const float* g_rgb_rec, const float* g_ph_map, const float* g_ph_mean, float* g_logits,
                       float* g_sigma, float* g_plane, float* g_dists, float* workspace, pd_stream_t stream);

/*
 * pd_plane_sweep_bwd with the backward of the fused decoder tail (pd_decoder_tail_fwd, networks/depth_decoder.py:258-291)
 * riding along — SURVEY.md 8f rank 1's "removes the round-trips": where the decoder's logits / sigma come from
 * pd_decoder_tail_fwd without a padding mask (xy planes only), the gradients this call writes are those of the decoder's
 * CONV outputs:
 *   g_raw_logits = g_logits + t,  g_raw_sigma = (g_sigma - t / sigma) * sigmoid'(raw_sigma) * [clamp passed],
 *   t = gD (d_n - disp) P_n,  P = softmax(logits) / sigma / sum(pi / sigma),  gD = g_disp - g_depth * 0.1 * 0.58 * W / disp^2,
 * and g_plane [B,N] carries the sum of the warp's and the tail's (sum_pixels gD P_n) disparity gradients.  The
 * [B,N,H,W]-sized g_logits / g_sigma are then never re-read by a tail kernel (pd_decoder_tail_bwd reads 4 N + writes 2 N
 * floats per pixel for what costs this kernel ~20 instructions per element on values it holds anyway).
 *   logits, sigma   what pd_decoder_tail_fwd returned (logits = its raw_logits input when there is no mask)
 *   raw_sigma       [B,N,H,W] the sigma conv's output (read only where sigma sits on the clamp's lower bound)
 *   tail_stash, disp  pd_decoder_tail_fwd's stash [B,2,H,W] and disp [B,1,H,W]
 *   g_disp, g_depth   [B,1,H,W] upstream gradients of the tail's disp / depth outputs, either may be NULL
 * Served where pd_sweep_bwd_tail_fuses(d) == 1 (PD_WARP_DISP, PD_MIXTURE, one disparity per plane, sign = +-1, the row-stream
 * backward's plain LDS layout); PD_ERR_UNSUPPORTED otherwise (the caller then runs pd_plane_sweep_bwd + pd_decoder_tail_bwd).
 */
int pd_sweep_bwd_tail_fuses(const pd_sweep_desc* d);
int pd_plane_sweep_bwd_tail(const pd_sweep_desc* d, const float* src, const float* tgt, const float* logits,
                            const float* sigma, const float* plane, const float* rgb_rec, const float* stash,
                            const float* g_rgb_rec, const float* g_ph_map, const float* g_ph_mean, const float* raw_sigma,
                            const float* tail_stash, const float* disp, const float* g_disp, const float* g_depth,
                            float* g_raw_logits, float* g_raw_sigma, float* g_plane, float* workspace, pd_stream_t stream);

/*
 * pd_plane_sweep_bwd_tail for the row form of xy + xz planes (networks/depth_decoder.py:153-181: disparity and padding mask
 * are constant along x): `plane` is [B,N] or, PD_DISP_ROWS, [B,N,H]; `mask_rows` is the [B,N,H] float 0 / 1 mask that BOTH
 * pd_decoder_tail_fwd (PD_TAIL_MASK_ROWS) and the sweep (PD_MASK_ROWS) were given — required with PD_MASK_ROWS, NULL without it.
 * All four combinations are served; with neither flag the call is pd_plane_sweep_bwd_tail's.  The results are what
 * pd_plane_sweep_bwd + pd_decoder_tail_bwd (PD_TAIL_DISP_ROWS / PD_TAIL_MASK_ROWS) produce: with m = the mask,
 * P = m softmax(logits) / sigma / sum(m pi / sigma) (tail_stash holds the log-sum-exp over the MASKED logits, where a masked plane
 * enters with logit 0, and sum(m pi / sigma)); at an unmasked element the formulas of pd_plane_sweep_bwd_tail hold as they stand.
 * At a masked (b, n, y) g_raw_logits, g_raw_sigma and the tail's share of g_plane are exact zeros by selection — whatever
 * `plane` holds there, a non-finite value included.  g_plane has the shape of `plane`: with PD_DISP_ROWS the row workgroup
 * that owns (b, y) writes the warp's + the tail's share of [B,N,H] directly (no workspace, no reduction launch); else as in
 * pd_plane_sweep_bwd_tail (PD_BWD_PLANE_ZEROED honoured).
 * Served where pd_sweep_bwd_tail_rows_fuses(d) == 1: PD_WARP_DISP, PD_MIXTURE, sign = +-1, fp32 storage, no PD_DISP_DENSE, no
 * PD_RENDER_PROB, even W, the row-stream backward's plain LDS layout (+ 4 N bytes for a row form); PD_ERR_UNSUPPORTED otherwise and
 * for PD_LOGITS_BF16.  pd_sweep_bwd_tail_fuses keeps answering for pd_plane_sweep_bwd_tail alone (0 for the row flags).
 */
int pd_sweep_bwd_tail_rows_fuses(const pd_sweep_desc* d);
int pd_plane_sweep_bwd_tail_rows(const pd_sweep_desc* d, const float* src, const float* tgt, const float* logits,
                                 const float* sigma, const float* plane, const float* mask_rows, const float* rgb_rec,
                                 const float* stash, const float* g_rgb_rec, const float* g_ph_map, const float* g_ph_mean,
                                 const float* raw_sigma, const float* tail_stash, const float* disp, const float* g_disp,
                                 const float* g_depth, float* g_raw_logits, float* g_raw_sigma, float* g_plane,
                                 float* workspace, pd_stream_t stream);

/*
 * The per-plane tensors the reference stores in `outputs` and the fused path never needs (trainer.py:582-602):
 * rgb_rec_layered [B,N,3,H,W], logit_rec, probability_rec, sigma_rec, pi_rec [B,N,H,W].  Any output may be NULL.
 * Forward only (values for logging / inspection; gradients flow through pd_plane_sweep_fwd/bwd).
 */
int pd_plane_sweep_layers(const pd_sweep_desc* d, const float* src, const float* logits, const float* sigma,
                          const float* plane, const float* plane_aux, const float* inv_K3, const float* padding_mask,
                          const float* dists, float* rgb_rec_layered, float* logit_rec, float* probability_rec,
                          float* sigma_rec, float* pi_rec, pd_stream_t stream);

/*
 * SSIM (layers.py:276-306: 3x3 box, ReflectionPad2d(1), clamp((1-n/d)/2,0,1)) and
 * Trainer.compute_reprojection_loss (trainer.py:687-699) — SURVEY.md row A10.
 *   pd_ssim_fwd:        x,y [B,C,H,W] -> out [B,C,H,W]
 *   pd_reproj_loss_fwd: pred,target [B,3,H,W] -> loss [B,1,H,W] = use_ssim ? 0.85*mean_c ssim + 0.15*mean_c|t-p| : mean_c|t-p|
 *   pd_reproj_loss_bwd: g_loss [B,1,H,W] -> g_pred [B,3,H,W] (overwritten); g_target may be NULL
 *   pd_ssim_bwd:        g_out [B,C,H,W] -> g_x, g_y [B,C,H,W] (either may be NULL)
 */
int pd_ssim_fwd(int B, int C, int H, int W, const float* x, const float* y, float* out, pd_stream_t stream);
int pd_ssim_bwd(int B, int C, int H, int W, const float* x, const float* y, const float* g_out, float* g_x, float* g_y,
                pd_stream_t stream);
int pd_reproj_loss_fwd(int B, int H, int W, int use_ssim, const float* pred, const float* target, float* loss,
                       pd_stream_t stream);
int pd_reproj_loss_bwd(int B, int H, int W, int use_ssim, const float* pred, const float* target, const float* g_loss,
                       float* g_pred, float* g_target, pd_stream_t stream);

/*
 * multimodal_loss (layers.py:465-466) on materialised tensors:
 *   out[b,0,p] = -log( sum_n pi * dist(error; sigma) + 1e-7 ),  dist = laplacian (layers.py:454) if `laplacian` else
 *   gaussian (layers.py:451).  error, sigma, pi [B,N,H,W] -> out [B,1,H,W].  bwd: any of g_error/g_sigma/g_pi may be NULL.
 */
int pd_mixture_nll_fwd(int B, int N, int H, int W, int laplacian, const float* error, const float* sigma,
                       const float* pi, float* out, pd_stream_t stream);
int pd_mixture_nll_bwd(int B, int N, int H, int W, int laplacian, const float* error, const float* sigma,
                       const float* pi, const float* g_out, float* g_error, float* g_sigma, float* g_pi,
                       pd_stream_t stream);

/*
 * Fused tail of DepthDecoder.forward (networks/depth_decoder.py:256-260, 274-291, softmax branch):
 *   logits = raw_logits * padding_mask; pi = softmax_N(logits); sigma = clamp(sigmoid(raw_sigma), .01, 1);
 *   probability = (pi / sigma * mask) / sum_N (mixture) or pi; disp = sum_N probability * disp_layered;
 *   depth = 0.1 * 0.58 * W / disp.
 * raw_logits, raw_sigma (mixture only), padding_mask (NULL = all ones) [B,N,H,W]; disp_layered [B,N], or [B,N,H,W] with
 * PD_TAIL_DISP_DENSE.  fwd writes logits (only when there is a mask; without one logits == raw_logits), sigma
 * (mixture), disp and depth [B,1,H,W] and a stash [B,2,H,W] {log-sum-exp, sum pi*mask/sigma}.  pi / probability are not
 * materialised by fwd (training reads them for their shape only): pd_decoder_tail_layers writes either or both on demand.
 * bwd: upstream g_logits, g_sigma [B,N,H,W], g_disp, g_depth [B,1,H,W] (each may be NULL = zero) -> g_raw_logits,
 * g_raw_sigma [B,N,H,W], g_disp_layered (same layout as disp_layered; the [B,N] form needs `workspace` of
 * pd_decoder_tail_bwd_workspace_floats floats); outputs that are NULL are skipped.
 *
 * PD_TAIL_BF16 (torch.autocast: the conv outputs are bf16; fwd, layers and bwd of both tails take it): the signatures do not
 * change, but these `float*` parameters hold torch.bfloat16 bit patterns: raw_logits, raw_sigma; fwd's outputs logits, sigma;
 * bwd's inputs g_logits, g_sigma and outputs g_raw_logits, g_raw_sigma.  Everything else stays fp32: padding_mask,
 * disp_layered, disp, depth, stash, g_disp, g_depth, g_disp_layered, workspace, pi, probability.  A bf16 element widens exactly
 * on load, every operation is the fp32 kernel's in the same order, and every bf16 output element is rounded once, to nearest
 * even, from the fp32 value that holds all of its contributions.  So disp, depth, stash, pi and probability are what the fp32
 * entry gives on the widened inputs (they come from the UNROUNDED fp32 sigma, where the reference under autocast would carry a
 * bf16-rounded sigma into probability), `sigma` is that fp32 sigma rounded once (bf16(0.01) = 0.010009765625 >= 0.01: it never
 * falls below the sweep's clamp), and bwd decides the clamp gate in fp32 on the sigmoid it recomputes from raw_sigma.
 * NULL and shape checks are the same with and without the flag; bf16 tensors need 2-byte alignment only (8-byte alignment of
 * all of them, 16-byte of the fp32 ones, and H*W % 4 == 0 select the form with 4 pixels per lane).
 *
 * Row form (fwd, layers and bwd of the decoder tail, fp32 and PD_TAIL_BF16; the PladeNet tail does not take it).  xy and xz
 * planes have a disparity and a padding mask that are constant along x (depth_decoder.py:153-181; pd_plane_geometry_fwd makes
 * them in this form):
 *   PD_TAIL_DISP_ROWS   disp_layered is [B,N,H] and g_disp_layered is written as [B,N,H]: g[b,n,y] = the sum over x of what the
 *                       dense form writes, reduced on the device by the workgroup that owns row y — no atomics, no workspace,
 *                       the same bits on every run.  Refused together with PD_TAIL_DISP_DENSE.
 *   PD_TAIL_MASK_ROWS   padding_mask is [B,N,H].  Refused with a NULL mask.
 *                       (A NULL-pointer refusal under either flag names the flag and the layout it announces.)
 * Either flag may stand alone (a dense map next to a row mask, and the reverse).  Per pixel the arithmetic and its order are
 * the dense form's on the expanded values: fwd's outputs, pi / probability and g_raw_logits / g_raw_sigma have the dense
 * route's bits.  The row tensors are read one scalar per plane and row and need 4-byte alignment only.  4 pixels per lane are
 * taken for a row form only when additionally W % 4 == 0, so that a group of 4 never straddles two rows (H = 2, W = 6 has
 * H*W % 4 == 0 and would); every other width runs one pixel per lane.
 * pd_decoder_tail_bwd_workspace_floats is the per-plane form's need and the maximum over the forms (dense and rows: none).
 */
enum pd_tail_flags {
  PD_TAIL_MIXTURE = 1,
  PD_TAIL_DISP_DENSE = 2,
  PD_TAIL_BF16 = 4,
  PD_TAIL_DISP_ROWS = 8,
  PD_TAIL_MASK_ROWS = 16
};
size_t pd_decoder_tail_bwd_workspace_floats(int B, int N, int H, int W);
int pd_decoder_tail_fwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                        const float* padding_mask, const float* disp_layered, float* logits, float* sigma, float* disp,
                        float* depth, float* stash, pd_stream_t stream);
int pd_decoder_tail_layers(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                           const float* padding_mask, const float* stash, float* pi, float* probability,
                           pd_stream_t stream);
int pd_decoder_tail_bwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                        const float* padding_mask, const float* disp_layered, const float* stash, const float* disp,
                        const float* g_logits, const float* g_sigma, const float* g_disp, const float* g_depth,
                        float* g_raw_logits, float* g_raw_sigma, float* g_disp_layered, float* workspace,
                        pd_stream_t stream);

/*
 * Fused tail of PladeNet.forward with --render_probability (networks/plade_net.py:309-341; the live producer of
 * outputs["dists"], which the sweep's PD_RENDER_PROB branch consumes, trainer.py:584-591):
 *   depth_layered = 0.1 * 0.58 * W / disp_layered; dists_n = (depth_layered_{n+1} - depth_layered_n) * ray_norm;
 *   alpha_n = 1 - exp(-relu(raw_logits_n) * dists_n) (n < N-1), alpha_{N-1} = 1; pi_n = alpha_n prod_{m<n}(1 - alpha_m + 1e-10);
 *   logits = cat(raw_logits, ones); sigma = clamp(sigmoid(raw_sigma), .01, 1);
 *   probability = (pi / sigma) / sum_N (mixture) or pi; disp = sum_N probability * disp_layered; depth = 0.1 * 0.58 * W / disp.
 * raw_logits [B,N-1,H,W] (conv0's output), raw_sigma [B,N,H,W] (conv_sigma's, mixture only); disp_layered [B,N], or [B,N,H,W]
 * with PD_TAIL_DISP_DENSE; ray_norm [H,W] = |K^-1 [x, y, 1]| of layers.py:468-492 (create_camera_plane).  fwd writes logits
 * [B,N,H,W], dists [B,N-1,H,W], sigma (mixture), disp, depth [B,1,H,W] and a stash [B,1,H,W] {sum pi/sigma};
 * pd_plade_tail_layers writes pi / probability on demand.  bwd: upstream g_logits [B,N,H,W] (its last channel is the constant
 * ones plane), g_dists [B,N-1,H,W], g_sigma [B,N,H,W], g_disp, g_depth (each may be NULL = zero) -> g_raw_logits [B,N-1,H,W],
 * g_raw_sigma, g_disp_layered (layout of disp_layered; the [B,N] form needs `workspace` of
 * pd_decoder_tail_bwd_workspace_floats floats); outputs that are NULL are skipped.
 * PD_TAIL_BF16, under the rule stated above: bf16 are raw_logits, raw_sigma, fwd's logits and sigma (the appended ones channel
 * is an exact bf16 1), bwd's g_logits, g_sigma, g_raw_logits and g_raw_sigma; ray_norm, dists, g_dists and everything the
 * decoder tail keeps in fp32 stay fp32.
 */
int pd_plade_tail_fwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                      const float* disp_layered, const float* ray_norm, float* logits, float* dists, float* sigma, float* disp,
                      float* depth, float* stash, pd_stream_t stream);
int pd_plade_tail_layers(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                         const float* disp_layered, const float* ray_norm, const float* stash, float* pi, float* probability,
                         pd_stream_t stream);
int pd_plade_tail_bwd(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                      const float* disp_layered, const float* ray_norm, const float* stash, const float* disp,
                      const float* g_logits, const float* g_dists, const float* g_sigma, const float* g_disp,
                      const float* g_depth, float* g_raw_logits, float* g_raw_sigma, float* g_disp_layered, float* workspace,
                      pd_stream_t stream);

/*
 * Inference tails: the two tails above, forward only, for a caller that wants a depth map and not a training step
 * (evaluate_depth_HR.py:144-168 reads outputs["disp"] and outputs["probability"].amax(1) only).  One pass over the planes;
 * nothing [B,N,H,W]-sized is written (no logits, sigma or dists).
 * Inputs, flags, refusals, alignment rules and the choice between 4 pixels and 1 pixel per lane are those of
 * pd_decoder_tail_fwd (all five PD_TAIL_* flags, row forms included) and pd_plade_tail_fwd (PD_TAIL_MIXTURE,
 * PD_TAIL_DISP_DENSE, PD_TAIL_BF16; a row flag is refused, N >= 2).  The output pointers listed below count for the alignment
 * rule like the fp32 ones of fwd (16 bytes each for 4 pixels per lane); under PD_TAIL_BF16 only raw_logits / raw_sigma are bf16.
 * Outputs, all [B,1,H,W] unless said otherwise; `disp` is required, every other one may be NULL and is skipped then:
 *   disp, depth   bit-identical to what the matching fwd writes for the same inputs and flags
 *   confidence    fp32, max_n probability_n: with the mixture the weights (pi / sigma * mask) / sum_N of depth_decoder.py:282-285
 *                 (pi / sigma / sum_N for PladeNet), without it pi.  A masked plane keeps logit 0 in the softmax, as in the
 *                 reference.  Within rounding of pd_*_tail_layers' probability, not bit-identical for the decoder tail (the best
 *                 weight is carried through the online softmax and rescaled when its reference moves).
 *   plane_index   int32, the plane that attains that maximum; the lowest index among equal maxima (the comparison is strict)
 *   disp_best     fp32, disp_layered at plane_index
 *   stash         [B,2,H,W] (decoder) / [B,1,H,W] (PladeNet), bit-identical to fwd's: pd_*_tail_layers serve pi / probability
 *                 from it on demand
 * Forward only: there is no backward for these entries; a differentiable caller uses pd_*_tail_fwd / _bwd.
 */
int pd_decoder_tail_infer(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                          const float* padding_mask, const float* disp_layered, float* disp, float* depth, float* confidence,
                          int* plane_index, float* disp_best, float* stash, pd_stream_t stream);
int pd_plade_tail_infer(int B, int N, int H, int W, int flags, const float* raw_logits, const float* raw_sigma,
                        const float* disp_layered, const float* ray_norm, float* disp, float* depth, float* confidence,
                        int* plane_index, float* disp_best, float* stash, pd_stream_t stream);

/*
 * Novel views at inference: what the network IS — a layered view synthesiser — as one forward-only entry, in the style of the
 * inference tails above.  From the decoder's conv outputs and the source image to V rendered views in one launch: the tail of
 * DepthDecoder.forward (depth_decoder.py:256-291) followed by pred_novel_images (trainer.py:540-603, disp_warp) with the
 * disparity scaled per view by a baseline factor s (any finite float): +1 is the reference's target "r", -1 its target "l", 0
 * the source camera, 0.5 half the rig's baseline.  Per view:
 *   logits = logits_in * mask; sigma = clamp(sigmoid(sigma_in), .01, 1)      (the tail step, on the SOURCE rows' mask)
 *   per plane n, at px = x + fl(s * d_n) (fp32, the reference's coordinate chain), bilinear, zeros padding, times mask_n of the
 *   TARGET row: colour_n, logit_n, sigma_n and ones_n (a ones image);  an out-of-view tap enters the softmax with logit 0
 *   p = softmax_N(logit); with PD_TAIL_MIXTURE p = (p / clamp(sigma, .01, 1)) / sum_N
 *   rgb = sum_N p colour;  coverage = sum_N p ones  (the share of the composite that came from inside the source image: 1 in
 *   the interior, towards 0 where the view looks past the image's edge);  disp = sum_N p d  (the rig's disparity in the NEW view)
 * Nothing [B,N,H,W]-sized is written, there is no workspace, and logits_in / sigma_in are read from memory once per launch
 * whatever V is (a workgroup owns a target row, stages each plane's source row in LDS once and serves every view's taps from it).
 * A view's results do not depend on V or on the other views of its launch, bit for bit.
 * Flags: pd_tail_flags (PD_TAIL_MIXTURE, PD_TAIL_BF16: logits_in / sigma_in hold bf16 and widen exactly, every output is fp32;
 * PD_TAIL_DISP_ROWS: disp_layered is [B,N,H]; PD_TAIL_MASK_ROWS: mask_rows is [B,N,H]) ORed with pd_render_flags:
 *   PD_RENDER_TAIL_APPLIED   logits_in / sigma_in are `logits` / `sigma` as a tail already wrote them (pd_decoder_tail_fwd, the
 *                            stock DepthDecoder, FalNet): the tail step is skipped, the sampled features still take the mask
 * baselines is a HOST array of V floats, copied into the launch arguments (nothing of it is read after the call returns).
 * rgb [B,V,3,H,W] is required; coverage and disp [B,V,1,H,W] may be NULL and are skipped then.  Every element of an output
 * that is given is written.
 * Refused before anything touches the device, naming the argument or flag: V outside 1..PD_RENDER_MAX_VIEWS; a non-finite
 * baseline; PD_TAIL_MASK_ROWS with a NULL mask_rows, or mask_rows without the flag; sigma_in NULL with PD_TAIL_MIXTURE;
 * N*H*W >= 2^31; H or W below 2; a pointer that is not aligned to its element (4 bytes; 2 for bf16).  PD_ERR_UNSUPPORTED:
 * PD_TAIL_DISP_DENSE (dense disparities or masks: yz planes), and a row wider than the staged-row layout takes (2048 pixels).
 * --render_probability (the PladeNet tail) has no form here; homography_warp views (arbitrary camera poses) are pd_render_poses,
 * below.
 * Forward only.
 */
enum { PD_RENDER_MAX_VIEWS = 4 };
enum pd_render_flags { PD_RENDER_TAIL_APPLIED = 256, PD_RENDER_VISIBLE_ONLY = 512 };
int pd_render_views(int B, int N, int H, int W, int V, int flags, const float* logits_in, const float* sigma_in,
                    const float* mask_rows, const float* disp_layered, const float* image, const float* baselines, float* rgb,
                    float* coverage, float* disp, pd_stream_t stream);
/* The columns a lane owns in a pd_render_views launch of V views on rows of W pixels, answered on the host (no GPU needed): 1, or
 * 2 for W > 1024 and for W >= 513 with V <= 2; 0 for what the entry point refuses (W < 2, W > 2048, V outside
 * 1..PD_RENDER_MAX_VIEWS).  The entry point switches on the same function; a pixel's bits are the same in both forms. */
int pd_render_cols_per_lane(int W, int V);

/*
 * Novel views at inference for arbitrary camera poses: pd_render_views' counterpart for homography_warp.  From the decoder's conv
 * outputs, the planes (distance [B,N], norm [B,N,3]) and the source image to V views, one per pose T[b,v] ([B,V,4,4]; T maps
 * source to target, X_t = R X_s + t, as in H_s2t = K (R + t n^T / d) K^-1): the tail of DepthDecoder.forward followed by
 * pred_novel_images with warp_type == "homography_warp" (trainer.py:556-603, layers.py:206-234).  Per view:
 *   logits = logits_in * mask_rows[b,n,y_src]; sigma = clamp(sigmoid(sigma_in), .01, 1)     (the tail step, applied to each tap)
 *   per plane n: p = H_t2s [x,y,1]; mask = (K^-1 [x,y,1] . (R n) > 0) and (z > 1e-7); z clamped to 1e-7; the reference's normalise /
 *   un-normalise round trip (the training kernels' arithmetic); bilinear, zeros padding: colour_n, logit_n, sigma_n and ones_n (a
 *   ones image), each times mask.  A masked plane keeps logit 0 and sigma 0.01 in the mixture, as in the reference.
 *   p = softmax_N(logit); with PD_TAIL_MIXTURE p = (p / clamp(sigma, .01, 1)) / sum_N
 *   rgb = sum_N p colour;  coverage = sum_N p ones;  disp = sum_N p disp_n(x,y) with disp_n = max(a x + b y + c, 0), the plane's
 *   inverse depth in the NEW camera as a rig disparity (0.1 * 0.58 * W / z_t): 0.1 * 0.58 * W / disp is the new view's depth.
 *   (a, b, c) = 0.1 * 0.58 * W * (K^-1[:3,:3])^T n_t / d_t with n_t = R n, d_t = d + n_t . t; 0 for d_t <= 0.
 * Two launches: a setup kernel writes one 16-float record per (b, v, n) into `workspace` (pd_render_poses_workspace_floats(B, N,
 * V) = 16 * B * V * N floats, answered on the host) — H_t2s (9) and R n (3), bit-identical to what
 * pd_homography_matrices_fwd(PD_HMAT_PLANES) writes for that image with the pose T[b,v]; (a, b, c), formed in fp64 and rounded
 * once; a validity word: a record whose matrix is not finite or not invertible (d_t = 0, the new camera's centre lies on the
 * plane — a case outside the reference, whose torch.inverse fails there) masks its plane everywhere in that view.  The render
 * kernel has one lane per target pixel and streams over the planes, the grid image-major.  Nothing [B,N,H,W]-sized is written,
 * there are no atomics, and a view's bits do not depend on V or on the other views of the launch.
 * Flags: PD_TAIL_MIXTURE, PD_TAIL_BF16 (logits_in / sigma_in hold bf16 and widen exactly; every output is fp32),
 * PD_TAIL_MASK_ROWS (mask_rows is [B,N,H]; not read with PD_RENDER_TAIL_APPLIED), PD_RENDER_TAIL_APPLIED as in pd_render_views, and
 *   PD_RENDER_VISIBLE_ONLY   a plane whose mask is off at a pixel takes no part at all (weight 0, not logit 0); a pixel where no
 *                            plane is visible gets rgb = coverage = disp = 0.  (The reference lets masked planes enter the mixture
 *                            with weight p / 0.01, which darkens a view in which planes leave the frustum: right for parity with
 *                            rgb_rec, wrong for a picture.)
 * rgb [B,V,3,H,W] is required; coverage and disp [B,V,1,H,W] may be NULL.  Every element of an output that is given is written.
 * Refused before anything touches the device, naming the argument or flag: V < 1 or B*V > 65535; PD_TAIL_DISP_ROWS and
 * PD_TAIL_DISP_DENSE (planes come in as distance / norm); PD_TAIL_MASK_ROWS with a NULL mask_rows, or mask_rows without the flag;
 * sigma_in NULL with PD_TAIL_MIXTURE; a NULL workspace, T, K, inv_K, distance or norm; N*H*W >= 2^31; H or W below 2; a pointer
 * that is not aligned to its element (4 bytes; 2 for bf16).  --render_probability and the PladeNet tail have no form here.
 * Forward only; no allocation, no synchronisation.
 */
size_t pd_render_poses_workspace_floats(int B, int N, int V);
int pd_render_poses(int B, int N, int H, int W, int V, int flags, const float* logits_in, const float* sigma_in,
                    const float* mask_rows, const float* distance, const float* norm, const float* T, const float* K,
                    const float* inv_K, const float* image, float* rgb, float* coverage, float* disp, float* workspace,
                    pd_stream_t stream);

/*
 * get_smooth_loss_disp (layers.py:243-256; trainer.py:768):
 *   out[0] = mean_x |d(x)-d(x+1)| exp(-gamma mean_c|I(x)-I(x+1)|) + the same along y.
 * disp [B,1,H,W], img [B,C,H,W]; both may be crops of wider tensors: unit column stride, the other strides (in floats)
 * are passed explicitly.  bwd: g_out[0] (device scalar) -> g_disp, contiguous [B,1,H,W].
 */
int pd_smooth_loss_fwd(int B, int C, int H, int W, const float* disp, int64_t disp_stride_b, int64_t disp_stride_h,
                       const float* img, int64_t img_stride_b, int64_t img_stride_c, int64_t img_stride_h, float gamma,
                       float* out, pd_stream_t stream);
int pd_smooth_loss_bwd(int B, int C, int H, int W, const float* disp, int64_t disp_stride_b, int64_t disp_stride_h,
                       const float* img, int64_t img_stride_b, int64_t img_stride_c, int64_t img_stride_h, float gamma,
                       const float* g_out, float* g_disp, pd_stream_t stream);
/* As pd_smooth_loss_bwd, for a crop that drops the first x_pad columns of a wider tensor (trainer.py:768 crops 0.2 W):
 * g_disp is the gradient of the UNCROPPED disparity, contiguous [B,1,H,W + x_pad], its first x_pad columns written as
 * the zeros they are — the caller's autograd graph then needs no slice node (a zero-fill and a strided copy per step). */
int pd_smooth_loss_bwd_padded(int B, int C, int H, int W, int x_pad, const float* disp, int64_t disp_stride_b,
                              int64_t disp_stride_h, const float* img, int64_t img_stride_b, int64_t img_stride_c,
                              int64_t img_stride_h, float gamma, const float* g_out, float* g_disp, pd_stream_t stream);

/*
 * Warps of Trainer.generate_post_process_disp (trainer.py:421-466), forward only:
 *   pd_warp_softmax  out[b,n] = softmax over n of planes[b,n] sampled at (x + sign*disp[b,n], y)   [B,N,H,W] -> [B,N,H,W]
 *   pd_warp_sum      out[b,0] = min(cap, sum over n of planes[b,n] sampled at (x + sign*disp[b,n], y))      -> [B,1,H,W]
 * bilinear, zeros padding, align_corners=True, coordinates through the reference's normalise / un-normalise round trip.
 * disp [B,N], with PD_PP_DISP_ROWS [B,N,H] (one disparity per plane and row: the decoder's xz planes) or, with PD_PP_DISP_DENSE,
 * [B,N,H,W]; PD_PP_FLIP_SRC reads `planes` mirrored along x (the .flip(-1) of
 * trainer.py:451) without a flipped copy.  Per-plane disparities with an even W and N <= 64 (pd_warp_sum: any N) take the segment
 * form (two pixels per lane, 12-byte taps, the softmax's samples of all planes in registers: sampled once); PD_PP_SEG=0 keeps
 * the one-pixel-per-lane row kernels (exact: cross-check); dense disparities take the per-pixel gather form.
 */
enum pd_pp_flags { PD_PP_DISP_DENSE = 1, PD_PP_FLIP_SRC = 2, PD_PP_DISP_ROWS = 4 };
int pd_warp_softmax(int B, int N, int H, int W, float sign, int flags, const float* planes, const float* disp,
                    float* out, pd_stream_t stream);
int pd_warp_sum(int B, int N, int H, int W, float sign, int flags, const float* planes, const float* disp, float cap,
                float* out, pd_stream_t stream);
/* disp_pp of trainer.py:458-461 in one pass: disp [2B,1,H,W] (the fixed model's output for cat([image, mirrored image])),
 * o_fr / o_l [B,1,H,W] (the two occlusion masks pd_warp_sum produced) -> disp_pp [B,1,H,W];
 *   mean = disp[b] / 2 + flip(disp[B + b]) / 2;  pp = mean o_fr + disp[b] (1 - o_fr);  disp_pp = pp o_l + flip(disp[B + b]) (1 - o_l). */
int pd_pp_combine(int B, int H, int W, const float* disp, const float* o_fr, const float* o_l, float* disp_pp,
                  pd_stream_t stream);

/* trainer.py:443-465 behind ONE call (three launches on `stream` where a row's softmax fits the CU's LDS — per-plane disparities,
 * even W <= 1024, N <= 64: the "row chains" keep softmax(warp(logits)) in LDS and take the second warp's plane sum from there, the
 * [B,N,H,W] intermediate never reaches memory; PD_PP_SEG=0 or any other shape: the six launches of the single warps): logits / probability [2B,N,H,W] and disp [2B,1,H,W] are the fixed
 * model's outputs for cat([image, mirrored image]) (B = half of that batch; of `probability` only the first B images are read),
 * disp_layered [2B,N], PD_PP_DISP_ROWS [2B,N,H] or PD_PP_DISP_DENSE [2B,N,H,W]; workspace: pd_post_process_workspace_floats floats;
 * -> disp_pp, mask_novel [B,1,H,W]. */
size_t pd_post_process_workspace_floats(int B, int N, int H, int W);
int pd_post_process(int B, int N, int H, int W, int flags, const float* logits, const float* probability, const float* disp,
                    const float* disp_layered, float* workspace, float* disp_pp, float* mask_novel, pd_stream_t stream);

/* Which kernel serves a post-process call: the ONE decision the three entry points above dispatch on, answered on the host (no
 * GPU needed: the LDS size falls back to gfx950's 160 KiB) from the shape, the flags and the ALIGNMENT of the buffers named —
 * the pointers are never dereferenced, and NULL stands for an 8-byte aligned buffer.  An entry point launches what its query
 * reports and nothing else (a combination without a kernel is an error return, not a fall-back).
 *   family     the warps: per-pixel gather (dense disparities), row kernels (one pixel per lane), segment kernels (a pixel pair
 *              per lane: even W, 8-byte aligned out, the softmax with N <= 64); the fused call: the six single warps (each on
 *              its own pd_warp_route), the row chain with one wave per segment (pp_chain_kernel), or with the planes of a
 *              segment dealt to three waves (pp_chain_split_kernel: W <= 640)
 *   flip       PD_PP_FLIP_SRC (a template argument of every warp kernel; the chains run both reads: 0)
 *   nmax       the planes a lane's registers are unrolled over: 32 / 52 / 64 (segment softmax, pp_chain_kernel), 11 / 18 / 22
 *              per part (pp_chain_split_kernel); 0 = a run-time loop over the planes
 *   rows2      the chains' second warp takes per-row shifts (PD_PP_DISP_ROWS): three S maps per chain
 *   alias      pp_chain_split_kernel keeps the parts' statistics inside the row buffer (the row buffer nearly fills the LDS)
 *   lds_bytes  dynamic LDS per workgroup */
enum pd_pp_kind { PD_PP_KIND_SOFTMAX = 0, PD_PP_KIND_SUM = 1 };
enum pd_pp_family {
  PD_PP_FAMILY_GATHER = 0, PD_PP_FAMILY_ROWS = 1, PD_PP_FAMILY_SEG = 2,          /* pd_warp_softmax / pd_warp_sum */
  PD_PP_FAMILY_SINGLE = 3, PD_PP_FAMILY_CHAIN = 4, PD_PP_FAMILY_CHAIN_SPLIT = 5  /* pd_post_process */
};
typedef struct pd_pp_route {
  int32_t family; /* pd_pp_family */
  int32_t flip, nmax, rows2, alias;
  uint32_t lds_bytes;
} pd_pp_route;
/* flags as for the entry point (pd_warp_route: PD_PP_FLIP_SRC included); returns PD_OK, or the entry point's own refusal of
 * the shape or the flags. */
int pd_warp_route(int kind, int B, int N, int H, int W, int flags, const void* out, pd_pp_route* route);
int pd_post_process_route(int B, int N, int H, int W, int flags, const void* workspace, const void* disp_pp, pd_pp_route* route);

/*
 * Trainer.add_flip_right_inputs (trainer.py:252-276): out [2B,C,H,W] = cat([own, flip(other, -1)]);
 * negate_c0 flips the sign of channel 0 in the mirrored half (the x-coordinate channel of `grid`, trainer.py:258-260).
 */
int pd_cat_flip(int B, int C, int H, int W, const float* own, const float* other, int negate_c0, float* out,
                pd_stream_t stream);

/*
 * inputs["grid"] of the data pipeline on the device: RandomResizeCrop / Resize of
 * datasets/pair_transforms.py:27-37, 63-68.  params [B][4] int32 on the device = (full_w, full_h, w0, h0): the resized
 * frame's size and the crop window's origin; grid [B,2,H,W] receives torch.linspace(-1, 1, full_w)[w0 + x] and
 * torch.linspace(-1, 1, full_h)[h0 + y] (scalar formula; within one ulp of ATen's vectorised CPU kernel).
 */
int pd_crop_grid(int B, int H, int W, const int32_t* params, float* grid, pd_stream_t stream);

/*
 * The images of the data pipeline on the device (pd_input_pipeline.hip): ToTensor, RandomResizeCrop / Resize, RandomGamma,
 * RandomBrightness and RandomColorBrightness of datasets/pair_transforms.py (:27-56, :66-84, :94-141) as mono_dataset.py:149-187
 * drives them, from the decoded frames to the cropped windows in one launch; the resized full frame is never formed.
 *   src        the B * V decoded frames (V views per sample), padded to one size: PD_SRC_U8_HWC [B,V,Hmax,Wmax,3] uint8, or
 *              PD_SRC_F32_CHW [B,V,3,Hmax,Wmax] fp32 (values as ToTensor leaves them)
 *   src_hw     [B][2] int32 (hs, ws): the true frame size of sample b, shared by its views.  Rows / columns beyond it are padding
 *              and never influence a result (nor are they read)
 *   crop       [B][4] int32 (full_w, full_h, w0, h0), the layout of pd_crop_grid: the frame is resized to full_h x full_w and the
 *              H x W window at (h0, w0) is kept.  Resize is full = (W, H), origin 0
 *   flags      [B] int32, pd_pipe_flags: which augmentation stages run for sample b, and the horizontal flip (the source is read
 *              mirrored, ws - 1 - x: the transpose mono_dataset.py applies before everything else)
 *   aug        [B][V][5] fp32 (gamma, brightness, c0, c1, c2)
 *   color      [B,V,3,H,W]: bicubic (A = -0.75, align_corners=True), clamped to [0, 1].  The source coordinate
 *              (y + h0) (hs - 1) / (full_h - 1) is split into floor and fraction by an integer division, exactly; uint8 / 255 is
 *              correctly rounded; full == source copies the source bit for bit
 *   color_aug  [B,V,3,H,W]: color, then x^gamma (PD_PIPE_GAMMA), min(x * brightness, 1) (PD_PIPE_BRIGHTNESS), min(x * c_ch, 1)
 *              (PD_PIPE_CHANNEL), in this order; a stage whose bit is clear is skipped, so flags without stage bits give color's bits
 * Memory: every tap is clamped into the true frame and hs, ws into Hmax, Wmax, whatever the parameter tensors hold, so no byte
 * outside `src` is read for any parameter values; writes cover exactly the two outputs.
 * Limits, refused on the host: B * V <= 65535, H, W <= 65536, Hmax, Wmax <= 32768, Hmax * Wmax * 12 < 2^31.
 *
 * pd_resize_crop_nearest: the depth_gt branch (:50-54, :79-82).  src [B,1,Hd,Wd] fp32 with its own src_hw -> out [B,1,H,W] by
 * ATen's legacy nearest index min((int)floorf((float)dst * scale), in - 1), scale = (float)in / (float)full in fp32, with the same
 * crop window and flip bit (np.fliplr of the source).  A selection: bit-exact.
 */
enum pd_src_format { PD_SRC_U8_HWC = 0, PD_SRC_F32_CHW = 1 };
enum pd_pipe_flags { PD_PIPE_GAMMA = 1, PD_PIPE_BRIGHTNESS = 2, PD_PIPE_CHANNEL = 4, PD_PIPE_FLIP = 8 };
int pd_resize_crop_augment(int B, int V, int Hmax, int Wmax, int H, int W, int src_dtype, const void* src, const int32_t* src_hw,
                           const int32_t* crop, const int32_t* flags, const float* aug, float* color, float* color_aug,
                           pd_stream_t stream);
int pd_resize_crop_nearest(int B, int Hd, int Wd, int H, int W, const float* src, const int32_t* src_hw, const int32_t* crop,
                           const int32_t* flags, float* out, pd_stream_t stream);

/*
 * The decoders' positional encoding of inputs["grid"] (pd_grid_embed.hip): `epconv` on the full-resolution grid followed by
 * F.interpolate(bilinear, align_corners=True) to every decoder level (networks/depth_decoder.py:123-139, networks/pose_net.py:137-140,
 * networks/plade_net.py:150-158), as ONE launch that evaluates the embedding at the four source points of each output pixel and
 * blends: nothing of the size [B,.,H,W] is written or kept.
 *   grid       [B,2,H,W] fp32, any values, not only windows of one linspace (the flipped half of a batch holds the negated, mirrored x)
 *   sizes      n_levels pairs (h_l, w_l) of int32 ON THE HOST, read before the call returns; 1 <= n_levels <= 8, every side >= 1, not
 *              required to divide H or W, and a level may be as large as the source or larger
 *   kind       PD_EMBED_NEURAL: e1 = ELU(W1 g + b1) with 16 hidden channels, out = ELU(W2 e1 + b2), 1 <= E <= 16 (ELU: alpha = 1, expm1
 *              on the negative branch; `multires` is ignored).  PD_EMBED_FREQUENCY: cat(g, sin(g 2^k), cos(g 2^k)), k < multires, in
 *              layers.py:308-354's channel order, E = 2 + 4 multires, multires <= 16.  PD_EMBED_IDENTITY: the grid itself, E = 2.  The
 *              last two read no `params` and have no backward
 *   params     one block of 48 + 17 E floats: W1 [16,2], b1 [16], W2 [E,16], b2 [E]
 *   out        the levels' [B,E,h_l,w_l] one after the other in one flat buffer of B E sum(h_l w_l) floats
 * Resampling as ATen's upsample_bilinear2d: blend along x, then along y.  The source coordinate y (H - 1) / (h_l - 1) is split into
 * floor and fraction by an integer division (exact at any size; row 0, fraction 0 for h_l = 1); the second tap is clamped to the last
 * row / column.  A level of the source's size reproduces the embedding at the pixel, the identity kind the grid's bits.
 *
 * pd_grid_embed_bwd (neural kind): g_out in the forward's flat layout -> g_params, the gradient in the layout of `params`
 * (g_W1 [16,2], g_b1 [16], g_W2 [E,16], g_b2 [E]).  z1, e1, z2 are recomputed per tap from the grid: the forward leaves nothing behind.
 * No float atomics: private sums per lane, a wave and workgroup reduction into `workspace`
 * (pd_grid_embed_bwd_workspace_floats(B, E, n_levels, sizes) floats = min(ceil(B sum(h_l w_l) / 256), 512) (48 + 17 E); host only,
 * callable without a GPU, 0 for arguments the backward refuses), then a fixed-order sum: two runs give the same bits.  grid gets no
 * gradient.
 * Limits, refused on the host: H, W <= 32768, every level side <= 65536, B sum(h_l w_l) < 2^31 - 2^17.
 */
enum pd_embed_kind { PD_EMBED_NEURAL = 0, PD_EMBED_FREQUENCY = 1, PD_EMBED_IDENTITY = 2 };
int pd_grid_embed_fwd(int B, int H, int W, int kind, int E, int multires, int n_levels, const int32_t* sizes, const float* grid,
                      const float* params, float* out, pd_stream_t stream);
size_t pd_grid_embed_bwd_workspace_floats(int B, int E, int n_levels, const int32_t* sizes);
int pd_grid_embed_bwd(int B, int H, int W, int E, int n_levels, const int32_t* sizes, const float* grid, const float* params,
                      const float* g_out, float* g_params, float* workspace, pd_stream_t stream);

/*
 * The decoders' disparity levels (networks/depth_decoder.py:147-152, networks/plade_net.py:280-285), one launch each way:
 *   disp[m] = disp_max * (disp_min / disp_max) ** (levels[m] / (no_levels - 1));   distance[m] = dist_num / disp[m]
 * over M = B * N values (levels = arange(no_levels) + the learnt residual; dist_num = 0.1 * 0.58 * W, `distance` may be NULL).
 * pd_plane_levels_bwd: g_levels from the upstream gradients of disp and / or distance (either may be NULL) and the forward's disp.
 */
int pd_plane_levels_fwd(int M, int no_levels, float disp_min, float disp_max, float dist_num, const float* levels, float* disp,
                        float* distance, pd_stream_t stream);
int pd_plane_levels_bwd(int M, int no_levels, float disp_min, float disp_max, float dist_num, const float* disp,
                        const float* g_disp, const float* g_distance, float* g_levels, pd_stream_t stream);

/*
 * The geometry head of DepthDecoder.forward without yz planes (networks/depth_decoder.py:148-207) in ROW form, one launch each
 * way.  N = no_levels + xz_levels planes: no_levels fronto-parallel (xy) planes and xz_levels ground (xz) planes.
 *   residual [B,N]   sigmoid(residualconv) - 0.5 (:151); NULL without --plane_residual (all zeros)
 *   grid [B,2,H,W]   inputs["grid"]; read are grid[b,1,y,0] (the row's y coordinate), grid[b,0,y,0] and grid[b,0,y,W-1] (its x
 *                    extent, :172) and the corners grid[b,1,0,0], grid[b,1,H-1,0], grid[b,0,0,0], grid[b,0,0,W-1] (:197-199).  The
 *                    y channel is taken to be constant along x, which holds for every grid datasets/pair_transforms.py makes; a
 *                    sheared or rotated grid must keep the reference's dense lines.
 * fwd writes
 *   disp_rows [B,N,H]   xy: disp_max * (disp_min / disp_max) ** ((n + residual) / (no_levels - 1)) on every row (:153);
 *                       xz: 0.1 * 0.58 * W / ((x_last - x_first) / 2 * (h * 1.92 / (max(y, 1e-7) / 2))) with the height
 *                       h = xz_min + (xz_max - xz_min) * (m + residual) / (xz_levels - 1) (:163-181)
 *   mask_rows [B,N,H]   float 0 / 1: ones for xy, y >= 1e-7 for xz (:168, decided on the fp32 grid value)
 *   distance [B,N]      0.1 * 0.58 * W / disp (xy, :154); h / sqrt(1 + t^2) (xz, :204), t the principal point's offset (:197-200)
 *   norm [B,N,3]        [0,0,1] (xy); [0, 1, t] / sqrt(1 + t^2) (xz, :201-203)
 * in fp32 and the reference's operation order (no contraction), as pd_plane_levels does for :153-154; xz_levels == 0 gives
 * pd_plane_levels' values on every row.  mask_rows / distance / norm may be NULL (skipped).
 * bwd: upstream g_disp_rows [B,N,H] and g_distance [B,N] (either may be NULL = zero, not both), the forward's residual, grid and
 * disp_rows -> g_residual [B,N].  norm and mask_rows carry no gradient.  One wave per (image, plane) adds the rows in a fixed
 * order: no atomics, the same bits on every run.
 * Refused: no_levels < 2, xz_levels == 1 or < 0 (the reference divides by levels - 1), flags != 0 (none defined yet), NULL
 * pointers, bwd with a NULL residual.
 */
int pd_plane_geometry_fwd(int B, int no_levels, int xz_levels, int H, int W, int flags, float disp_min, float disp_max,
                          float xz_min, float xz_max, const float* residual, const float* grid, float* disp_rows,
                          float* mask_rows, float* distance, float* norm, pd_stream_t stream);
int pd_plane_geometry_bwd(int B, int no_levels, int xz_levels, int H, int W, int flags, float disp_min, float disp_max,
                          float xz_min, float xz_max, const float* residual, const float* grid, const float* disp_rows,
                          const float* g_disp_rows, const float* g_distance, float* g_residual, pd_stream_t stream);

/*
 * Photometric loss under the occlusion mask `mask_novel` (trainer.py:724-742; the mask is produced after
 * pred_novel_images, trainer.py:342-349, so it cannot enter the sweep's forward):
 *   pred = rgb_rec * mask + target * (1 - mask)                      -> pred [B,3,H,W] (may be NULL)
 *   mixture = 0:  mean over (b, pixel) of mean_c |pred - target|, or of min(that, mean_c |source - target|) when
 *                 `source` (the automask's identity view) is given   (trainer.py:738-742)
 *   mixture = 1:  mean over (b, pixel) of ph_map * mask, ph_map [B,1,H,W] = the sweep's per-pixel NLL (:736, :742)
 * mask [B,1,H,W] (NULL = all ones).  partials: workspace of B * ceil(H*W / 256) floats; mean: 1 float.
 * Backward: g_mean [1] (d loss / d mean, device scalar, may be NULL) and g_pred [B,3,H,W] (upstream gradient of the
 * blended prediction, e.g. from the perceptual net; may be NULL) -> g_rgb_rec [B,3,H,W], g_ph_map [B,1,H,W] (mixture).
 */
int pd_masked_photometric_fwd(int B, int H, int W, int mixture, const float* rgb_rec, const float* target,
                              const float* source, const float* mask, const float* ph_map, float* pred, float* partials,
                              float* mean, pd_stream_t stream);
int pd_masked_photometric_bwd(int B, int H, int W, int mixture, const float* rgb_rec, const float* target,
                              const float* source, const float* mask, const float* g_mean, const float* g_pred,
                              float* g_rgb_rec, float* g_ph_map, pd_stream_t stream);

/*
 * Perceptual feature distance (trainer.py:672-685; pd_feature_distance.hip), ONE feature level of the perceptual net per call:
 *   l_p = mean_c (pred - target)^2;  with `source` (opt.automask): l_p = min(l_p, mean_c (source - target)^2);
 *   loss[0] = (accumulate ? loss[0] : 0) + mean over [B,h,w] of l_p
 * so the reference's three levels are three calls with accumulate = 0, 1, 1 on one `loss`.  The net itself is not part of this
 * library.
 *   dtype     PD_DTYPE_F32 or PD_DTYPE_BF16: the element type of pred / target / source / g_pred, all [B,C,h,w] contiguous NCHW.
 *             bf16 (what the net emits under torch.autocast) widens exactly on load, every sum is fp32, and a gradient element
 *             is rounded to bf16 once, to nearest even — the rule of PD_LOGITS_BF16.  Anything else: PD_ERR_ARG naming it.
 *   source    may be NULL (no automask)
 *   sel       out (forward) / in (backward): [B,h,w] bytes, 1 where the prediction's distance is the minimum.  A TIE selects the
 *             prediction (torch.min over cat([l_p, l_a]) returns the first index); both sums are formed in the same order, so
 *             source == pred is a tie at every pixel, bit for bit.  All ones without a source.
 *   partials  workspace, B * ceil(h*w / 64) floats, contents unspecified afterwards (no zero-fill needed)
 *   loss      one float.  Deterministic: workgroup partial sums finished by one wave in index order, no float atomics
 *   g_loss    one float (device): the gradient of the scalar
 *   g_pred    [B,C,h,w], overwritten: g_loss * 2 (pred - target) / (C * B*h*w) where sel, exact zeros elsewhere (pred / target are
 *             not read there).  target and source get no gradient (dataset images through a frozen net in the reference).
 * A lane owns 16 bytes of adjacent pixels (four fp32, eight bf16) when h*w is a multiple of that count, the tensors are
 * 16-byte aligned and sel is 4-byte aligned; one pixel per lane otherwise.  Per pixel the arithmetic is the same either way (the mean's summation order differs).
 * Limits, refused on the host: B <= 65535, B*h*w < 2^31.
 */
enum pd_dtype { PD_DTYPE_F32 = 0, PD_DTYPE_BF16 = 1 };
int pd_feature_distance_fwd(int B, int C, int h, int w, int dtype, const void* pred, const void* target, const void* source,
                            uint8_t* sel, float* partials, float* loss, int accumulate, pd_stream_t stream);
int pd_feature_distance_bwd(int B, int C, int h, int w, int dtype, const void* pred, const void* target, const uint8_t* sel,
                            const float* g_loss, void* g_pred, pd_stream_t stream);

/*
 * The O(B*N) 3x3 algebra of HomographyWarp.forward (layers.py:206-219, 223-225) and its adjoint, one launch each:
 *   M = R + t n^T / d;  H_t2s = inverse(K M K^-1);  Rn = R n          (R, t from T [B,4,4]; K, inv_K [B,4,4])
 * evaluated in fp64 and rounded once to fp32.  distance [B,N], norm [B,N,3].
 *   PD_HMAT_PLANES       H_t2s [B,N,3,3], Rn [B,N,3]
 *   PD_HMAT_UNIFORM      zero-translation poses (trainer.py:386-400): H_t2s [B,4,3,3] in the PD_HOMO_UNIFORM layout
 *                        (slice 0: plane 0 with the translation detached; slices 1..3: virtual planes n/d = e_j with the
 *                        rotation detached), Rn [B,N,3]
 *   PD_HMAT_STEREO_ROWS  identity rotation, x translation, normals without x component (mono_dataset.py:203-211,
 *                        depth_decoder.py:153-207): shift [B,N,rows] = h01*y + h02 in pixels and mask [B,N,rows] =
 *                        facing test && z > 1e-7 (layers.py:223-225) per (plane, row): the inputs of the disp_warp sweep
 *                        with PD_DISP_ROWS | PD_MASK_ROWS.  H_t2s and Rn may be NULL.
 * Backward: g_H in the forward's H_t2s layout (may be NULL in PD_HMAT_STEREO_ROWS) and/or g_shift [B,N,rows];
 * g_distance [B,N], g_norm [B,N,3], g_T [B,4,4] (rows 0..2; row 3 zero) — each may be NULL.  K and inv_K get none (the
 * reference's are dataset constants).  In PD_HMAT_STEREO_ROWS only g_distance is meaningful (h00 is not part of the
 * shift, so the pose / normal derivatives are incomplete).
 */
enum pd_hmat_mode { PD_HMAT_PLANES = 0, PD_HMAT_UNIFORM = 1, PD_HMAT_STEREO_ROWS = 2 };
int pd_homography_matrices_fwd(int B, int N, int mode, int rows, const float* distance, const float* norm, const float* T,
                               const float* K, const float* inv_K, float* H_t2s, float* Rn, float* shift, float* mask,
                               pd_stream_t stream);
int pd_homography_matrices_bwd(int B, int N, int mode, int rows, const float* distance, const float* norm, const float* T,
                               const float* K, const float* inv_K, const float* g_H, const float* g_shift,
                               float* g_distance, float* g_norm, float* g_T, pd_stream_t stream);

/*
 * The pose path in front of pd_homography_matrices_* (pd_pose_tail.hip): the tail of PoseDecoder.forward (pose_net.py:148-155),
 * transformation_from_parameters' rotation (layers.py:17-92) and the conjugation with Rc (trainer.py:386-400), one launch each way,
 * evaluated in fp64 (the hw sum included) and rounded once.  Per image b:
 *   v[0:6]   = scale * mean over hw of x[b, 6 frame + k, :]        axisangle = v[0:3], translation = v[3:6]
 *   R        = rot_from_axisangle(axisangle), axis = vec / (|vec| + 1e-7) as the reference has it;  invert != 0: R^T
 *   Rc       = [[1,0,a],[0,1,b],[0,0,f]],  a = -gx0 / (2 0.58), b = -gy0 / (2 1.92),  gx0 = (grid[b,0,0,gW-1] + grid[b,0,0,0]) / 2,
 *              gy0 = (grid[b,1,gH-1,0] + grid[b,1,0,0]) / 2,  f = (grid[b,0,0,gW-1] - grid[b,0,0,0]) / 2
 *   Rt_Rc    [B,4,4]: [:3,:3] = Rc R Rc^-1, every other element 0 — [3,3] too (the reference fills a zeros_like)
 *   x        [B,C,hw] in `dtype` (PD_DTYPE_F32 / PD_DTYPE_BF16) through the ELEMENT strides x_sb (image), x_sc (channel), x_ss
 *            (position); C = 6 F with frame in [0, F), or C = 3: an axis-angle alone (frame 0; no translation output / gradient).
 *            An averaged axisangle tensor is hw = 1, scale = 1.
 *   Rt       COLMAP mode, forward only, given INSTEAD of x (exactly one of the two is non-NULL): [B,4,4] contiguous;
 *            Rt_Rc[:3,:3] = Rc Rt[:3,:3] Rc^-1, Rt_Rc[:3,3] = Rc Rt[:3,3], row 3 zero; axisangle / translation must be NULL.
 *   grid     [B,2,gH,gW] fp32 through grid_strides[4] (host array of element strides: image, channel, row, column)
 * Outputs, each may be NULL: axisangle [B,3], translation [B,3], Rc [B,3,3], Rt_Rc [B,4,4], contiguous fp32.
 * pd_pose_tail_bwd recomputes from x: g_Rt_Rc [B,4,4] (only [:3,:3] is read), g_axisangle [B,3], g_translation [B,3] — each may be
 * NULL, not all — -> g_x [B,C,hw] in `dtype` through its own element strides, overwritten in full: channel 6 frame + k gets
 * scale / hw times its gradient at every position (the translation channels g_translation alone), every other channel exact
 * zeros.  At vec = 0 the gradient of |vec| is taken as 0 (torch's convention): finite, what the reference's graph yields.  grid and
 * Rt get no gradient (dataset constants).  One workgroup per image, no float atomics: deterministic.
 * Refused on the host with PD_ERR_ARG: NULL required pointers, B <= 0, hw <= 0, C neither 3 nor a multiple of 6, frame out of
 * range, an unknown dtype, gH or gW < 1, C * hw >= 2^31.
 */
int pd_pose_tail_fwd(int B, int C, int hw, int frame, int dtype, int invert, double scale, const void* x, int64_t x_sb,
                     int64_t x_sc, int64_t x_ss, const float* Rt, const float* grid, int gH, int gW,
                     const int64_t* grid_strides, float* axisangle, float* translation, float* Rc, float* Rt_Rc,
                     pd_stream_t stream);
int pd_pose_tail_bwd(int B, int C, int hw, int frame, int dtype, int invert, double scale, const void* x, int64_t x_sb,
                     int64_t x_sc, int64_t x_ss, const float* grid, int gH, int gW, const int64_t* grid_strides,
                     const float* g_Rt_Rc, const float* g_axisangle, const float* g_translation, void* g_x, int64_t gx_sb,
                     int64_t gx_sc, int64_t gx_ss, pd_stream_t stream);

/*
 * Geometry modules.
 *   pd_backproject     BackprojectDepth.forward, layers.py:150-156: depth [B,1,H,W], inv_K [B,4,4] -> cam [B,4,H*W]
 *   pd_backproject_bwd g_cam [B,4,H*W] -> g_depth [B,1,H,W]
 *   pd_project3d       Project3D.forward, layers.py:169-182: cam [B,4,H*W], P=(K@T)[:, :3, :] [B,3,4] -> grid [B,H,W,2]
 *   pd_project3d_bwd   g_grid -> g_cam [B,4,H*W] (may be NULL) and g_P [B,3,4] (may be NULL; needs workspace of
 *                      12 * B * ceil(H*W/256) floats)
 *   pd_homography_grid HomographyWarp.forward per-pixel part, layers.py:221-233: H_t2s [M,3,3], Rn [M,3],
 *                      inv_K3 [M,3,3] -> grid [M,H,W,2], mask [M,H,W] (uint8 0/1)
 *   pd_homography_grid_bwd  g_grid [M,H,W,2] -> g_H [M,3,3] (workspace: 9 * M * ceil(H*W/256) floats)
 */
int pd_backproject(int B, int H, int W, const float* depth, const float* inv_K, float* cam, pd_stream_t stream);
int pd_backproject_bwd(int B, int H, int W, const float* inv_K, const float* g_cam, float* g_depth, pd_stream_t stream);
int pd_project3d(int B, int H, int W, float eps, const float* cam, const float* P, float* grid, pd_stream_t stream);
int pd_project3d_bwd(int B, int H, int W, float eps, const float* cam, const float* P, const float* g_grid,
                     float* g_cam, float* g_P, float* workspace, pd_stream_t stream);
int pd_homography_grid(int M, int H, int W, const float* H_t2s, const float* Rn, const float* inv_K3, float* grid,
                       uint8_t* mask, pd_stream_t stream);
int pd_homography_grid_bwd(int M, int H, int W, const float* H_t2s, const float* g_grid, float* g_H, float* workspace,
                           pd_stream_t stream);

/*
 * Second pass of TWO plane-uniform backward calls (PD_HOMO_UNIFORM | PD_BWD_DEFER_GATHER, the same descriptor and the
 * same logits / sigma: the novel frames -1 / +1 of the reference's mono training, trainer.py:532) in one kernel:
 *   g_logits / g_sigma [B,N,H,W] = (PD_BWD_ACCUMULATE in d->flags: their old contents +) view a's gradient + view b's.
 * `plane_*` [B,4,3,3] and `inv_K3_*` [B,3,3] are the views' arguments of pd_plane_sweep_bwd, `workspace_*` the workspaces
 * those calls filled (pd_sweep_bwd_workspace_floats each).  g_sigma may be NULL without PD_MIXTURE.
 */
int pd_uniform_gather_pair(const pd_sweep_desc* d, const float* plane_a, const float* inv_K3_a, float* workspace_a,
                           const float* plane_b, const float* inv_K3_b, float* workspace_b, float* g_logits, float* g_sigma,
                           pd_stream_t stream);

/*
 * TWO plane-uniform target views of the same source image in one call each way (the novel frames -1 / +1 of the reference's
 * mono training: `for target_side in self.target_sides` over the same outputs, trainer.py:532).  The views' workgroups for
 * the same image tile are dispatched next to each other on one XCD, so the second view finds the logits / sigma lines of the
 * first in that XCD's L2; results are those of two pd_plane_sweep_fwd / pd_plane_sweep_bwd calls, bit for bit.
 *   pd_sweep_view: what differs between the views.  Forward: tgt, plane [B,4,3,3], plane_aux [B*N,3], inv_K3 [B,3,3], dists
 *                  (PD_RENDER_PROB) in; rgb_rec, ph_map, ph_mean (may be NULL), stash out.  Backward: the same inputs +
 *                  padding_mask ([B,N,3] translation weights or NULL), rgb_rec, stash, g_rgb_rec / g_ph_map / g_ph_mean
 *                  (each may be NULL) in; g_plane [B,4,3,3] (may be NULL), g_dists (may be NULL) and `workspace`
 *                  (pd_sweep_bwd_workspace_floats(d) floats per view) out.
 *   pd_uniform_fwd_pair   d: PD_WARP_HOMOGRAPHY | PD_HOMO_UNIFORM; PD_PH_MEAN_ZEROED as in pd_plane_sweep_fwd.
 *   pd_uniform_bwd_pair   g_logits / g_sigma [B,N,H,W] = (PD_BWD_ACCUMULATE: their old contents +) both views' gradients;
 *                         g_logits NULL: only g_plane / g_dists are produced.
 */
typedef struct pd_sweep_view {
  const float* tgt;
  const float* plane;
  const float* plane_aux;
  const float* inv_K3;
  const float* padding_mask;
  const float* dists;
  float* rgb_rec;
  float* ph_map;
  float* ph_mean;
  float* stash;
  const float* g_rgb_rec;
  const float* g_ph_map;
  const float* g_ph_mean;
  float* g_plane;
  float* g_dists;
  float* workspace;
} pd_sweep_view;
int pd_uniform_fwd_pair(const pd_sweep_desc* d, const float* src, const float* logits, const float* sigma,
                        const pd_sweep_view* view_a, const pd_sweep_view* view_b, pd_stream_t stream);
int pd_uniform_bwd_pair(const pd_sweep_desc* d, const float* src, const float* logits, const float* sigma,
                        const pd_sweep_view* view_a, const pd_sweep_view* view_b, float* g_logits, float* g_sigma,
                        pd_stream_t stream);

/*
 * F.grid_sample(input, grid, mode="bilinear", padding_mode=zeros|border, align_corners=True) as the reference calls it
 * (trainer.py:444-463, 573-577, 624-628) — SURVEY.md row A5.
 *   input [M,C,Hi,Wi], grid [M,Ho,Wo,2] -> out [M,C,Ho,Wo]
 *   bwd: g_out -> g_input [M,C,Hi,Wi] (must be ZERO-FILLED by the caller; accumulated with atomics; may be NULL),
 *                 g_grid [M,Ho,Wo,2] (overwritten; may be NULL)
 */
int pd_grid_sample_fwd(int M, int C, int Hi, int Wi, int Ho, int Wo, int padding_mode, const float* input,
                       const float* grid, float* out, pd_stream_t stream);
int pd_grid_sample_bwd(int M, int C, int Hi, int Wi, int Ho, int Wo, int padding_mode, const float* input,
                       const float* grid, const float* g_out, float* g_input, float* g_grid, pd_stream_t stream);

/*
 * Depth evaluation (pd_depth_eval.hip): the Eigen metrics with median scaling of evaluate_depth_HR.py:148-166, 217-279
 * (compute_errors :30-49, batch_post_process_disparity :51-59) and Trainer.compute_depth_losses (trainer.py:775-810 with
 * layers.py:356-374).  The full contract is the header comment of pd_depth_eval.hip and planedepth_amd/metrics.py.
 *   pred      A: disparity [M,h,w] ([2M,h,w] with PD_EVAL_POST_PROCESS: image i's mirrored pass is image i+M);
 *             PD_EVAL_TRAINER: depth [M,1,h,w] at the GT's resolution
 *   grid      PD_EVAL_TRAINER only: channel 0 of inputs["grid"], [M,h,grid_w] (the per-row divisor grid[..,gw-1] - grid[..,0])
 *   gt, meta  GT of every image packed into one fp32 buffer; meta int64 [M][8] on the device = (offset of the image in `gt`
 *             in floats, gt_h, gt_w, crop y0, y1, x0, x1, 0); the crop is the whole image for non-Eigen splits
 *   max_tiles ceil(max_i gt_h*gt_w / PD_EVAL_TILE): the launch grid is [M][max_tiles] tiles
 *   disp_num  float32(0.1*0.58*width) (A); scale_factor: A 1 or 5.4 before the medians, PD_EVAL_TRAINER the factor used
 *             instead of the medians (5.4)
 * Outputs over S segments (S = M; 1 with PD_EVAL_TRAINER, which pools the batch): metrics [S,7] fp32 (abs_rel, sq_rel, rmse,
 * rmse_log, a1, a2, a3), ratio [S], medians [S,2] (of gt, of depth; NaN without PD_EVAL_MEDIAN), counts [S,4] int32
 * (n, #a1, #a2, #a3).  workspace: pd_depth_eval_workspace_bytes bytes (no zero-fill needed).  Deterministic: integer
 * atomics only, fixed-order floating-point sums.
 * pd_depth_eval_resize: the resized (and, PD_EVAL_POST_PROCESS, post-processed) disparity of step A2 alone, written into a
 * buffer packed like `gt` (max_hw = max_i gt_h*gt_w).
 */
enum pd_eval_flags {
  PD_EVAL_POST_PROCESS = 1, /* evaluate_depth_HR.py:163-165: average with the mirrored pass before resizing        */
  PD_EVAL_EIGEN = 2,        /* eigen_raw / eigen_improved: 1e-3 < gt < 80 inside the Eigen crop (:237-249); else gt > 0 */
  PD_EVAL_MEDIAN = 4,       /* median scaling (A: numpy's median; PD_EVAL_TRAINER: opt.no_stereo, torch's lower median)  */
  PD_EVAL_TRAINER = 8       /* Trainer.compute_depth_losses: depth input, per-row grid divisor, pooled batch            */
};
enum { PD_EVAL_TILE = 16384 };
size_t pd_depth_eval_workspace_bytes(int M, int max_tiles, int flags);
int pd_depth_eval(int M, int h, int w, int flags, int max_tiles, float disp_num, float scale_factor, const float* pred,
                  const float* grid, int grid_w, const float* gt, const int64_t* meta, void* workspace, float* metrics,
                  float* ratio, float* medians, int32_t* counts, pd_stream_t stream);
int pd_depth_eval_resize(int M, int h, int w, int flags, int max_hw, const float* pred, const int64_t* meta, float* out,
                         pd_stream_t stream);

/*
 * Diagnostics (used by tests/ and scripts/, not by the product path).
 *   pd_selftest_division        counts, over `count` samples lo + i*step, where the row kernels' fast division by W-1
 *                               (refined reciprocal) differs from the IEEE quotient; *d_mismatches (device int) += count.
 *   pd_debug_gather_flags, pd_debug_poison_lds, pd_debug_count_lds_nans   see below (PD_DEBUG_POISON_LDS=1 makes the Python layer poison before every launch).
 */
int pd_selftest_division(float Wm1, int count, float lo, float step, int* d_mismatches, pd_stream_t stream);
/* The gather backward's device flags of the LAST pd_plane_sweep_bwd launch that used `workspace` with this descriptor
 * (per-plane homographies, PD_IMPL_AUTO): host_out[0] = 1 if some plane was irregular (line at infinity near the view,
 * strong minification, non-finite matrix) and took the atomic fix-up, host_out[1] = 1 if a gather window was cut at its
 * size limit (a plane the prepare kernel should have sent to the fix-up: always 0 in the tests).  Synchronises `stream`. */
int pd_debug_gather_flags(const pd_sweep_desc* d, const float* workspace, int* host_out, pd_stream_t stream);
/* Fills the LDS of the device's CUs with NaNs (a kernel that reads shared memory it never wrote then yields NaNs). */
int pd_debug_poison_lds(pd_stream_t stream);
/* *d_count += the NaNs 2048 workgroups find in 32 KB of shared memory they never wrote (checks that the poison sticks). */
int pd_debug_count_lds_nans(int* d_count, pd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PLANEDEPTH_HIP_H */
