"""From images to depth maps: the prediction loop of the reference's ``evaluate_depth_HR.py`` (lines 139-168) on the device — the
producer of what ``metrics.eval_depth_errors`` and ``planedepth_amd.evaluate`` consume.

``model(images, grids)`` is the reference's ``depth_decoder(encoder(x), grids)`` or ``PladeNet`` and returns the outputs dict.  With
the inference tail inside (``decoder_tail.fused_decoder_tail_inference`` / ``fused_plade_tail_inference``) nothing plane-sized is
written on the way to ``outputs["disp"]`` and ``outputs["confidence"]``; a model that still carries the training tail works too
(its confidence is taken from ``outputs["probability"].amax(1)``, which materialises the [B,N,H,W] tensor).
"""
import collections

import torch

from . import _capi as C
from . import ops
from . import planeform as PF

Prediction = collections.namedtuple("Prediction", "raw_disp disp depth confidence mean_confidence")


def eval_grid(batch, height, width, device):
    """``inputs["grid"]`` of evaluate_depth_HR.py:139-152: ``linspace(-1, 1)`` over the width and the height, meshgrid "xy",
    stacked (x, y) and expanded over the batch — [batch,2,height,width], built on the host as the reference builds it."""
    grid = torch.stack(torch.meshgrid(torch.linspace(-1, 1, width), torch.linspace(-1, 1, height), indexing="xy"), dim=0)
    return grid.to(device)[None].expand(batch, -1, -1, -1)


def _prediction(outputs, M, w, post_process):
    d = outputs["disp"]
    confidence = outputs.get("confidence")
    if confidence is None:   # a training tail: probability is a [B,N,H,W] tensor (or the lazy stand-in for one)
        confidence = outputs["probability"].amax(1, keepdim=True)
    raw_disp = d[:, 0]
    disp = 0.5 * (d[:M] + d[M:].flip(-1)) if post_process else d
    depth = disp.new_full((), 0.1 * 0.58 * w) / disp   # (a true division: ``scalar / tensor`` is reciprocal-times-scalar)
    mean_confidence = confidence[:, 0].mean(-1).mean(-1)
    return Prediction(raw_disp, disp, depth, confidence, mean_confidence)


def predict(model, images, *, post_process=False, autocast=False):
    """Disparity, depth and confidence of ``images`` [M,3,h,w] (fp32, on the GPU) under ``torch.no_grad()``, and under
    ``torch.autocast("cuda", torch.bfloat16)`` when ``autocast``.  With ``post_process`` the batch is ``[images ; mirrored images]``
    (``ops.cat_flip``: two forward passes per image, evaluate_depth_HR.py:148-150).  Returns the named tuple

    * ``raw_disp`` [M,h,w], [2M,h,w] with ``post_process``: ``outputs["disp"][:, 0]`` — what ``metrics.eval_depth_errors(...,
      post_process=...)`` takes;
    * ``disp`` [M,1,h,w]: ``outputs["disp"]``, or with ``post_process`` ``0.5f * (d[:M] + d[M:].flip(-1))`` — the live part of
      ``batch_post_process_disparity`` (contract A1 of ``metrics``);
    * ``depth`` = ``float32(0.1 * 0.58 * w) / disp``;
    * ``confidence`` [M or 2M,1,h,w]: ``max_n probability_n`` of every pass;
    * ``mean_confidence`` [M or 2M]: its mean over the image, the reference's ``probabilities_max`` (:168).

    The averages and the mean are plain torch on [.,1,h,w] tensors."""
    C.require_gpu_tensor("images", images)
    if images.dim() != 4:
        raise ValueError("images must be [M,C,h,w], got %s" % (tuple(images.shape),))
    M, _, h, w = images.shape
    with torch.no_grad():
        batch = ops.cat_flip(images, images) if post_process else images
        grids = eval_grid(batch.shape[0], h, w, images.device)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(autocast)):
            outputs = model(batch, grids)
        return _prediction(outputs, M, w, post_process)


def _render_mask(outputs, shape):
    """The mask ``ops.render_views`` takes for ``outputs["padding_mask"]``: ``None`` for none, a row view as it is, and ``None``
    for a dense mask that holds ones only — the stock decoder's ``torch.ones_like(disp_layered)`` of xy planes (one reduction
    and a host sync).  Any other dense mask (yz planes) goes through and is refused by name."""
    mask = outputs.get("padding_mask")
    if mask is None or PF._row_view(mask, *shape, "padding_mask"):
        return mask
    return None if bool((mask == 1).all()) else mask


def render(model, images, baselines, *, autocast=False):
    """``images`` [M,3,h,w] (fp32, on the GPU) seen from the cameras ``baselines`` names (``ops.render_views``: +1 the rig's right
    view, -1 its left view, 0 the source camera, any finite factor in between and beyond), next to the depth prediction of the
    same forward pass.  Runs ``model(images, grids)`` once under ``torch.no_grad()`` (and ``torch.autocast`` when ``autocast``)
    and returns ``(Views, Prediction)``: ``Views(rgb [M,V,3,h,w], coverage [M,V,1,h,w], disp [M,V,1,h,w])`` and what ``predict``
    returns without ``post_process``.

    The views come from ``outputs["raw_logits"]`` / ``["raw_sigma"]`` when the model kept its conv outputs
    (``fused_decoder_tail_inference(..., keep_conv_outputs=True)``: nothing plane-sized is written anywhere), otherwise from
    ``outputs["logits"]`` / ``["sigma"]`` as a training tail or a stock network wrote them (``tail_applied=True``); a net without
    ``outputs["sigma"]`` (FalNet, ``use_mixture_loss`` off) renders without the mixture; logits and sigma of two dtypes (a stock
    tail under autocast) are widened to fp32 first.  Planes and mask are ``outputs["disp_layered"]`` / ``["padding_mask"]``."""
    C.require_gpu_tensor("images", images)
    if images.dim() != 4:
        raise ValueError("images must be [M,C,h,w], got %s" % (tuple(images.shape),))
    M, _, h, w = images.shape
    with torch.no_grad():
        grids = eval_grid(M, h, w, images.device)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(autocast)):
            outputs = model(images, grids)
        raw = "raw_logits" in outputs
        logits = outputs["raw_logits" if raw else "logits"]
        sigma = outputs.get("raw_sigma" if raw else "sigma")
        if sigma is not None and sigma.dtype != logits.dtype:   # a stock tail under autocast: fp32 logits (* mask), bf16 sigma
            logits, sigma = logits.float(), sigma.float()
        views = ops.render_views(logits, sigma, _render_mask(outputs, tuple(logits.shape)), outputs["disp_layered"], images,
                                 baselines, use_mixture_loss=sigma is not None, tail_applied=not raw)
        return views, _prediction(outputs, M, w, False)


def render_poses(model, images, poses, K=None, inv_K=None, *, autocast=False, visible_only=False):
    """``images`` [M,3,h,w] (fp32, on the GPU) seen from the cameras at ``poses`` — [M,V,4,4], or [V,4,4] for every image; a pose
    maps source to target coordinates, as the reference's ``inputs[("Rt", side)]`` (``ops.render_poses``) — next to the depth
    prediction of the same forward pass.  Runs ``model(images, grids)`` once under ``torch.no_grad()`` (and ``torch.autocast`` when
    ``autocast``) and returns ``(Views, Prediction)`` as ``render`` does.  ``K`` / ``inv_K`` [M,4,4] default to the dataset's
    intrinsics at this size (``synthetic.dataset_intrinsics``).

    The views come from ``outputs["raw_logits"]`` / ``["raw_sigma"]`` when the model kept its conv outputs, otherwise from
    ``outputs["logits"]`` / ``["sigma"]`` (``tail_applied=True``: no mask is read, so yz-plane models are served too), exactly as
    in ``render``; the planes are ``outputs["distance"]`` / ``["norm"]``, the mask ``outputs["padding_mask"]``."""
    C.require_gpu_tensor("images", images)
    if images.dim() != 4:
        raise ValueError("images must be [M,C,h,w], got %s" % (tuple(images.shape),))
    M, _, h, w = images.shape
    if (K is None) != (inv_K is None):
        raise ValueError("K and inv_K come together (both None: the dataset's intrinsics at this size)")
    with torch.no_grad():
        if K is None:
            from .synthetic import dataset_intrinsics
            K, inv_K = (t.to(images.device) for t in dataset_intrinsics(M, h, w))
        grids = eval_grid(M, h, w, images.device)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(autocast)):
            outputs = model(images, grids)
        raw = "raw_logits" in outputs
        logits = outputs["raw_logits" if raw else "logits"]
        sigma = outputs.get("raw_sigma" if raw else "sigma")
        if sigma is not None and sigma.dtype != logits.dtype:   # a stock tail under autocast: fp32 logits (* mask), bf16 sigma
            logits, sigma = logits.float(), sigma.float()
        mask = _render_mask(outputs, tuple(logits.shape)) if raw else None
        views = ops.render_poses(logits, sigma, mask, outputs["distance"].float(), outputs["norm"].float(), images, poses, K,
                                 inv_K, use_mixture_loss=sigma is not None, tail_applied=not raw, visible_only=visible_only)
        return views, _prediction(outputs, M, w, False)


predict.render = render
predict.render_poses = render_poses   # (``planedepth_amd.predict`` is the function: the package re-exports it over this module's name)
