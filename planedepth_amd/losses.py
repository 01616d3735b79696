"""Loss operators: SSIM / reprojection loss (layers.py:276-306, trainer.py:687-699), the mixture NLL (layers.py:454-466), the
photometric loss under mask_novel (trainer.py:724-742), the perceptual feature distance (trainer.py:672-685), the smoothness
loss (layers.py:243-256).
"""
import ctypes
import os

from . import _capi as C
from . import _state as S
from ._buffers import torch, _timed, _desc, _contig, _zero_scalar, _zero_block, _plane_grad_buffer


# ---------------------------------------------------------------------------------------------------------------------
# SSIM / reprojection loss
# ---------------------------------------------------------------------------------------------------------------------
class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        C.require_gpu_tensor("x", x)
        C.require_gpu_tensor("y", y, x.shape)
        x, y = x.contiguous(), y.contiguous()
        B, Cc, H, W = x.shape
        out = torch.empty_like(x)
        C.call("pd_ssim_fwd", x.device, B, Cc, H, W, x, y, out)
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B, Cc, H, W = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if gx is None and gy is None:
            return None, None
        C.call("pd_ssim_bwd", x.device, B, Cc, H, W, x, y, g.contiguous(), gx, gy)
        return gx, gy


def ssim(x, y):
    """layers.py:292-306 — per-pixel, per-channel clamp((1 - SSIM)/2, 0, 1) with a 3x3 reflected box window."""
    return _SSIM.apply(x, y)


class _ReprojLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, use_ssim):
        B, Cc, H, W = pred.shape
        if Cc != 3:
            raise ValueError("compute_reprojection_loss expects 3-channel images")
        C.require_gpu_tensor("pred", pred)
        C.require_gpu_tensor("target", target, pred.shape)
        pred, target = pred.contiguous(), target.contiguous()
        loss = torch.empty(B, 1, H, W, device=pred.device, dtype=torch.float32)
        C.call("pd_reproj_loss_fwd", pred.device, B, H, W, int(use_ssim), pred, target, loss)
        ctx.save_for_backward(pred, target)
        ctx.use_ssim = int(use_ssim)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        B, _, H, W = pred.shape
        gp = torch.empty_like(pred)
        gt = torch.empty_like(target) if ctx.needs_input_grad[1] else None
        C.call("pd_reproj_loss_bwd", pred.device, B, H, W, ctx.use_ssim, pred, target, g.contiguous(), gp, gt)
        return gp, gt, None


def reprojection_loss(pred, target, use_ssim=True):
    """trainer.py:687-699 fused: 0.85 * mean_c SSIM(pred, target) + 0.15 * mean_c |target - pred|  -> [B,1,H,W]."""
    return _ReprojLoss.apply(pred, target, bool(use_ssim))


class _MixtureNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, error, sigma, pi, laplacian):
        C.require_gpu_tensor("error", error)
        B, N, H, W = error.shape
        error, sigma, pi = (t.expand(B, N, H, W).contiguous() for t in (error, sigma, pi))
        C.require_gpu_tensor("sigma", sigma)
        C.require_gpu_tensor("pi", pi)
        out = torch.empty(B, 1, H, W, device=error.device, dtype=torch.float32)
        C.call("pd_mixture_nll_fwd", error.device, B, N, H, W, int(laplacian), error, sigma, pi, out)
        ctx.save_for_backward(error, sigma, pi)
        ctx.lap = int(laplacian)
        return out

    @staticmethod
    def backward(ctx, g):
        error, sigma, pi = ctx.saved_tensors
        B, N, H, W = error.shape
        ge = torch.empty_like(error) if ctx.needs_input_grad[0] else None
        gs = torch.empty_like(sigma) if ctx.needs_input_grad[1] else None
        gp = torch.empty_like(pi) if ctx.needs_input_grad[2] else None
        if ge is None and gs is None and gp is None:
            return None, None, None, None
        C.call("pd_mixture_nll_bwd", error.device, B, N, H, W, ctx.lap, error, sigma, pi, g.contiguous(), ge, gs, gp)
        return ge, gs, gp, None


def multimodal_loss(error, sigma, pi, dist="gaussian"):
    """layers.py:465-466 on materialised [B,N,H,W] tensors -> [B,1,H,W] (one kernel each way instead of ~10 passes)."""
    return _MixtureNLL.apply(error, sigma, pi, dist != "gaussian")




# ---------------------------------------------------------------------------------------------------------------------
# Photometric loss under mask_novel (trainer.py:724-742)
# ---------------------------------------------------------------------------------------------------------------------
class _MaskedPhotometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_rec, ph_map, target, source, mask):
        B, _, H, W = rgb_rec.shape
        dev = rgb_rec.device
        mix = ph_map is not None
        rgb_rec, target = _contig(rgb_rec.detach()), _contig(target)
        source = _contig(source) if source is not None else None
        mask = _contig(mask.float()) if mask is not None else None
        C.require_gpu_tensor("rgb_rec", rgb_rec, (B, 3, H, W))
        C.require_gpu_tensor("target", target, (B, 3, H, W))
        if mask is not None:
            C.require_gpu_tensor("mask_novel", mask, (B, 1, H, W))
        pm = _contig(ph_map.detach()) if mix else None
        pred = torch.empty_like(rgb_rec)
        partials = torch.empty(B * ((H * W + 255) // 256), device=dev)
        mean = torch.empty(1, device=dev)
        C.call("pd_masked_photometric_fwd", dev, B, H, W, int(mix), rgb_rec, target, source, mask, pm, pred, partials, mean)
        ctx.save_for_backward(rgb_rec, target, source, mask)
        ctx.mix = mix
        return pred, mean.reshape(())

    @staticmethod
    def backward(ctx, g_pred, g_mean):
        rgb_rec, target, source, mask = ctx.saved_tensors
        B, _, H, W = rgb_rec.shape
        dev = rgb_rec.device
        g_pred = _contig(g_pred) if g_pred is not None else None
        g_mean = _contig(g_mean.reshape(1)) if g_mean is not None else None
        g_rgb = torch.empty_like(rgb_rec) if ctx.needs_input_grad[0] else None
        g_ph = torch.empty(B, 1, H, W, device=dev) if (ctx.mix and ctx.needs_input_grad[1]) else None
        if g_rgb is not None or g_ph is not None:
            C.call("pd_masked_photometric_bwd", dev, B, H, W, int(ctx.mix), rgb_rec, target, source, mask, g_mean, g_pred,
                   g_rgb, g_ph)
        return g_rgb, g_ph, None, None, None


def masked_photometric(rgb_rec, target, mask, *, source=None, ph_map=None):
    """trainer.py:724-742 under ``outputs["mask_novel"]``: returns ``(pred, ph_loss)`` with
    ``pred = rgb_rec * mask + target * (1 - mask)`` (what the perceptual net is fed) and the scalar photometric loss —
    ``ph_map`` given (mixture): ``(ph_map * mask).mean()``; otherwise L1 on ``pred`` with the automask's ``min`` against
    ``source`` when that is given.  One kernel each way (pd_masked_loss.hip)."""
    return _MaskedPhotometric.apply(rgb_rec, ph_map, target, source, mask)


# ---------------------------------------------------------------------------------------------------------------------
# Perceptual feature distance (trainer.py:672-685)
# ---------------------------------------------------------------------------------------------------------------------
_FEATURE_DTYPES = {torch.float32: C.PD_DTYPE_F32, torch.bfloat16: C.PD_DTYPE_BF16}


class _FeatureDistance(torch.autograd.Function):
    """All levels in one node: ``args`` = the prediction's features, then the target's, then (``has_source``) the source's."""

    @staticmethod
    def forward(ctx, levels, has_source, *args):
        preds, targets = args[:levels], args[levels:2 * levels]
        sources = args[2 * levels:] if has_source else (None,) * levels
        dev = preds[0].device
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        saved = []
        for i, (p, t, s) in enumerate(zip(preds, targets, sources)):
            p, t, s = _contig(p.detach()), _contig(t), _contig(s)   # channels-last or sliced features are copied
            B, Cc, h, w = p.shape
            sel = torch.empty(B, h, w, device=dev, dtype=torch.uint8)
            partials = torch.empty(B * ((h * w + 63) // 64), device=dev, dtype=torch.float32)
            C.call("pd_feature_distance_fwd", dev, B, Cc, h, w, _FEATURE_DTYPES[p.dtype], p, t, s, sel, partials, loss, int(i > 0))
            saved += [p, t, sel]
        ctx.save_for_backward(*saved)
        ctx.levels = levels
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        saved = ctx.saved_tensors
        dev = saved[0].device
        g_loss = g_loss.reshape(1).contiguous().float()
        grads = []
        for i in range(ctx.levels):
            p, t, sel = saved[3 * i:3 * i + 3]
            if not ctx.needs_input_grad[2 + i]:
                grads.append(None)
                continue
            B, Cc, h, w = p.shape
            g = torch.empty_like(p)
            C.call("pd_feature_distance_bwd", dev, B, Cc, h, w, _FEATURE_DTYPES[p.dtype], p, t, sel, g_loss, g)
            grads.append(g)
        return (None, None) + tuple(grads) + (None,) * (len(ctx.needs_input_grad) - 2 - ctx.levels)


def _feature_levels(name, feats):
    if torch.is_tensor(feats):
        return [feats]
    feats = list(feats)
    if not feats:
        raise ValueError("feature_distance: %s holds no feature level" % name)
    return feats


def feature_distance(pred_feats, target_feats, source_feats=None):
    """Trainer.perceptual_loss (trainer.py:672-685) on the perceptual net's OUTPUTS: over the feature levels (a sequence of
    [B,C,h,w] tensors each; a bare tensor is one level) the sum of ``((pred_f - target_f) ** 2).mean(1, True)``, with
    ``source_feats`` (opt.automask) its per-pixel ``min`` with the source's distance, ``.mean()`` -> a 0-dim fp32 tensor.  One
    kernel per level each way, added up on the device (pd_feature_distance.hip).

    fp32 or bf16 features (a level's tensors share one dtype); the gradient has the prediction's dtype.  Only the prediction's
    features get a gradient: in the reference the target's and the source's are dataset images through a frozen net, and the
    kernels produce none for them — a target or source feature that requires grad is refused rather than silently detached.
    Non-contiguous (channels-last, sliced) features are copied."""
    preds, targets = _feature_levels("pred_feats", pred_feats), _feature_levels("target_feats", target_feats)
    sources = _feature_levels("source_feats", source_feats) if source_feats is not None else None
    if len(targets) != len(preds) or (sources is not None and len(sources) != len(preds)):
        raise ValueError("feature_distance: %d prediction levels, %d target levels%s" % (
            len(preds), len(targets), "" if sources is None else ", %d source levels" % len(sources)))
    for i, p in enumerate(preds):
        if not torch.is_tensor(p) or p.dim() != 4:
            raise ValueError("feature_distance: pred_feats[%d] must be a [B,C,h,w] tensor" % i)
        if p.dtype not in _FEATURE_DTYPES:
            raise TypeError("feature_distance: pred_feats[%d] is %s; float32 and bfloat16 features are served" % (i, p.dtype))
        others = [("target_feats", targets[i])] + ([("source_feats", sources[i])] if sources is not None else [])
        for name, t in others:
            if torch.is_tensor(t) and t.requires_grad:
                raise ValueError("feature_distance: %s[%d] requires grad, but the fused operator produces a gradient for the "
                                 "prediction's features only (the reference feeds dataset images through a frozen net "
                                 "there); detach it, or freeze the perceptual net" % (name, i))
        C.require_gpu_tensor("pred_feats[%d]" % i, p, dtype=p.dtype)
        for name, t in others:
            C.require_gpu_tensor("%s[%d]" % (name, i), t, p.shape, dtype=p.dtype)
            if t.device != p.device:
                raise ValueError("feature_distance: %s[%d] is on %s, pred_feats[%d] on %s" % (name, i, t.device, i, p.device))
        if p.device != preds[0].device:
            raise ValueError("feature_distance: pred_feats[%d] is on %s, pred_feats[0] on %s" % (i, p.device, preds[0].device))
    return _FeatureDistance.apply(len(preds), sources is not None, *preds, *targets, *(sources or ()))


# ---------------------------------------------------------------------------------------------------------------------
# Smoothness loss
# ---------------------------------------------------------------------------------------------------------------------
def _row_strided(name, t):
    """A [B,C,H,W] fp32 GPU tensor whose columns are unit-stride (e.g. the crop t[..., k:]) as it is, else a copy."""
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError("%s must be a float32 GPU tensor (got %s on %s)" % (name, t.dtype, t.device))
    return t if (t.stride(3) == 1 and min(t.stride()[:3]) >= 0) else t.contiguous()


class _SmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img, gamma, x0):
        B, Cn, H, Wf = img.shape
        if tuple(disp.shape) != (B, 1, H, Wf):
            raise ValueError("disp must be [B,1,H,W] matching img, got %s vs %s" % (tuple(disp.shape), tuple(img.shape)))
        disp, img = _row_strided("disp", disp), _row_strided("img", img)
        W = Wf - x0
        out = torch.empty(1, device=disp.device, dtype=torch.float32)
        # the crop [..., x0:] is an offset on the two base pointers: same strides, W - x0 columns
        dptr, iptr = ctypes.c_void_p(disp.data_ptr() + 4 * x0), ctypes.c_void_p(img.data_ptr() + 4 * x0)
        C.call("pd_smooth_loss_fwd", disp.device, B, Cn, H, W, dptr, disp.stride(0), disp.stride(2), iptr, img.stride(0),
               img.stride(1), img.stride(2), float(gamma), out)
        ctx.save_for_backward(disp, img)
        ctx.gamma, ctx.x0 = float(gamma), int(x0)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        disp, img = ctx.saved_tensors
        B, Cn, H, Wf = img.shape
        x0 = ctx.x0
        g_disp = torch.empty(B, 1, H, Wf, device=disp.device, dtype=torch.float32)
        g = g.reshape(1).contiguous().float()
        dptr, iptr = ctypes.c_void_p(disp.data_ptr() + 4 * x0), ctypes.c_void_p(img.data_ptr() + 4 * x0)
        # one kernel writes the whole [B,1,H,W] gradient, zeros in the cropped-away columns included
        C.call("pd_smooth_loss_bwd_padded", disp.device, B, Cn, H, Wf - x0, x0, dptr, disp.stride(0), disp.stride(2), iptr,
               img.stride(0), img.stride(1), img.stride(2), ctx.gamma, g, g_disp)
        return g_disp, None, None, None


def smooth_loss_disp(disp, img, gamma=1.0, x0=0):
    """get_smooth_loss_disp (reference layers.py:243-256) as one kernel each way.  ``x0``: evaluate on the crop
    ``[..., x0:]`` of both tensors (trainer.py:768 passes ``disp[..., int(0.2 * W):]``) WITHOUT slicing them in the autograd
    graph: the crop is a pointer offset in the forward, and the backward writes the gradient of the uncropped ``disp``
    directly (zeros left of the crop) — no slice node, i.e. no zero-fill, strided copy and three operator calls per step.
    Tensors that already are crops (``x0 = 0``) are read in place through their strides as before."""
    x0 = int(x0)
    if not 0 <= x0 <= disp.shape[-1] - 2:   # the crop is a pointer offset: a bad one would read past every row
        raise ValueError("smooth_loss_disp: x0 = %d is not a crop of a width-%d tensor (need 0 <= x0 <= W - 2)" % (x0, disp.shape[-1]))
    return _SmoothLoss.apply(disp, img, gamma, x0)


