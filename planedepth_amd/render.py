"""Novel views at inference: from the decoder's conv outputs and the source image to rendered views, forward only, with nothing
[B,N,H,W]-sized written on the way — the reference's ``pred_novel_images`` (trainer.py:523-603) on the tail of
``DepthDecoder.forward`` (networks/depth_decoder.py:256-291).  ``render_views`` (``pd_render_views``) moves the camera along the
rig's baseline (disp_warp), ``render_poses`` (``pd_render_poses``) to any 6-DoF pose (homography_warp).
"""
import collections
import ctypes

from . import _capi as C
from . import planeform as PF
from ._buffers import torch, _timed, _contig
from .tails import _checked, _decoder_operands, _infer_no_grad, _storage_flag

Views = collections.namedtuple("Views", "rgb coverage disp")
_WANT = ("coverage", "disp")


def _baselines(baselines):
    try:
        values = [float(s) for s in baselines]
    except TypeError:
        raise TypeError("baselines must be a sequence of numbers (one baseline factor per view)")
    if not values:
        raise ValueError("baselines is empty: one baseline factor per view, at least one view")
    for i, s in enumerate(values):
        if s != s or s in (float("inf"), float("-inf")):
            raise ValueError("baselines[%d] = %r is not finite" % (i, s))
    return values


def render_cols_per_lane(W, V):
    """The columns a lane owns in a ``pd_render_views`` launch of ``V`` views on rows of ``W`` pixels (``pd_render_cols_per_lane``,
    the function the entry point itself switches on; answered on the host): 1 or 2, 0 for what the entry point refuses."""
    return int(C.load().pd_render_cols_per_lane(int(W), int(V)))


def render_views(raw_logits, raw_sigma, padding_mask, disp_layered, image, baselines, use_mixture_loss=True,
                 tail_applied=False, want=("coverage", "disp")):
    """The other camera's picture: ``rgb`` [B,V,3,H,W] of ``image`` [B,3,H,W] seen from V cameras, one per entry of
    ``baselines``, and, as ``want`` names them, ``coverage`` and ``disp`` [B,V,1,H,W].  Returns the named tuple
    ``Views(rgb, coverage, disp)``; what was not asked for is ``None``.

    A baseline factor ``s`` scales the rig's disparity: ``+1`` is the reference's target ``"r"``, ``-1`` its target ``"l"``, ``0``
    the source camera, ``0.5`` half the rig's baseline; any finite float is legal.  Per view the result is the reference's
    ``rgb_rec`` for ``grid = disp_grid(float32(s) * disp_layered, "r")`` after ``decoder_tail``: softmax over the sampled logits
    (an out-of-view tap enters with logit 0), divided by the sampled sigma clamped to [0.01, 1] with the mixture, zeros padding,
    the mask on the source side and on the sampled features.  ``coverage`` is the same composite of a ones image — the share of
    the pixel that came from inside the source image; ``disp`` is ``(probability_rec * disp_layered).sum(1)``, the rig's
    disparity in the new view.

    ``raw_logits`` / ``raw_sigma`` are the decoder's conv outputs, fp32 or both bf16 (``raw_sigma`` is ignored without the
    mixture).  With ``tail_applied`` they are ``logits`` / ``sigma`` as a tail already produced them (``fused_decoder_tail``, the
    stock ``DepthDecoder``, FalNet's ``outputs["logits"]``): the tail transform is skipped, the sampled features still take the
    mask.  ``disp_layered`` is per plane (an H/W-expanded view) or a row view; ``padding_mask`` is ``None`` or a row view
    (``ops.row_view`` / ``ops.plane_geometry``).  Dense maps and masks (yz planes) are refused by name.

    One forward-only kernel per four views (``PD_RENDER_MAX_VIEWS``) that reads the conv outputs once per launch; a view's bits do
    not depend on which other views share its launch.  A longer list is served in chunks of four, each written straight into its
    slice of the outputs (per image then: the slice of one image is contiguous).  With gradients enabled an input that requires
    grad raises ``ValueError``: ``decoder_tail`` + ``plane_sweep_disp`` is the differentiable route."""
    want = (want,) if isinstance(want, str) else tuple(want)
    for w in want:
        if w not in _WANT:
            raise ValueError("want: unknown output %r (rgb is always returned; the optional ones are %s)" % (w, ", ".join(_WANT)))
    values = _baselines(baselines)
    B, N, H, W = raw_logits.shape
    mix = bool(use_mixture_loss)
    _storage_flag(raw_logits, raw_sigma, mix)   # (a wrong dtype is reported before anything else)
    _infer_no_grad("plane_sweep_disp", "render_views", raw_logits=raw_logits, raw_sigma=raw_sigma if mix else None,
                   padding_mask=padding_mask, disp_layered=disp_layered, image=image)
    with torch.no_grad():
        flags, _, raw_sigma, padding_mask, plane = _decoder_operands(raw_logits, raw_sigma, padding_mask, disp_layered, mix,
                                                                     grad=False)
        if padding_mask is not None and not flags & C.PD_TAIL_MASK_ROWS:
            raise C.PlaneDepthHipError("render_views: padding_mask is a dense [B,N,H,W] mask (yz planes), which is not served: "
                                       "None or a row view (stride(3) == 0) only")
        if flags & C.PD_TAIL_DISP_DENSE:
            raise C.PlaneDepthHipError("render_views: disp_layered is a dense [B,N,H,W] map (yz planes), which is not served "
                                       "(PD_TAIL_DISP_DENSE): per-plane scalars or a row view (stride(3) == 0) only")
        rl, rs, dl, pm = _checked(flags, N, raw_logits.detach(), None if raw_sigma is None else raw_sigma.detach(), plane,
                                  "padding_mask", padding_mask)
        C.require_gpu_tensor("image", image, (B, 3, H, W))
        image = image.detach().contiguous()
        flags |= C.PD_RENDER_TAIL_APPLIED if tail_applied else 0
        dev = rl.device
        V = len(values)
        new = lambda c: torch.empty(B, V, c, H, W, device=dev, dtype=torch.float32)  # noqa: E731
        rgb = new(3)
        coverage = new(1) if "coverage" in want else None
        disp = new(1) if "disp" in want else None
        step = C.PD_RENDER_MAX_VIEWS
        with _timed("render_views", dev):
            if V <= step:
                arr = (ctypes.c_float * V)(*values)
                C.call("pd_render_views", dev, B, N, H, W, V, flags, rl, rs, pm, dl, image, arr, rgb, coverage, disp)
            else:
                for v0 in range(0, V, step):
                    arr = (ctypes.c_float * len(values[v0:v0 + step]))(*values[v0:v0 + step])
                    for b in range(B):   # [b, v0:v0+4] is contiguous; [:, v0:v0+4] is not
                        at = lambda t: None if t is None else t[b:b + 1]                 # noqa: E731
                        out = lambda t: None if t is None else t[b, v0:v0 + len(arr)]    # noqa: E731
                        C.call("pd_render_views", dev, 1, N, H, W, len(arr), flags, at(rl), at(rs), at(pm), at(dl), at(image),
                               arr, out(rgb), out(coverage), out(disp))
    return Views(rgb, coverage, disp)


def render_poses(raw_logits, raw_sigma, padding_mask, distance, norm, image, T, K, inv_K, use_mixture_loss=True,
                 tail_applied=False, visible_only=False, want=("coverage", "disp")):
    """``image`` [B,3,H,W] seen from V cameras at arbitrary poses: ``rgb`` [B,V,3,H,W] and, as ``want`` names them, ``coverage``
    and ``disp`` [B,V,1,H,W], as the named tuple ``Views(rgb, coverage, disp)``; what was not asked for is ``None``.

    ``T`` is [B,V,4,4], or [V,4,4] broadcast over the batch; a pose maps source to target coordinates (``X_t = R X_s + t``, the
    reference's ``inputs[("Rt", side)]``).  ``K`` / ``inv_K`` are [B,4,4].  The planes are ``distance`` [B,N] and ``norm``
    (anything that expands to [B,N,3]): ``outputs["distance"]`` / ``outputs["norm"]`` of the decoders.  Per view the result is the
    reference's ``rgb_rec`` of ``pred_novel_images`` with ``warp_type == "homography_warp"`` after ``decoder_tail`` (the matrices
    formed in fp64 and rounded once, as ``ops.plane_sweep_homography`` forms them): softmax over the sampled logits, divided by
    the sampled sigma clamped to [0.01, 1] with the mixture, zeros padding, each plane masked where it faces away or lies behind
    the camera.  ``coverage`` is the same composite of a ones image; ``disp`` is the composite of the planes' inverse depths in the
    NEW camera, scaled as a rig disparity: ``0.1 * 0.58 * W / disp`` is the new view's depth.

    ``visible_only``: a plane that is masked at a pixel takes no part there (the reference keeps it in the mixture with logit 0
    and sigma 0.01, which darkens a view in which planes leave the frustum); a pixel no plane reaches is 0 in every output.

    ``raw_logits`` / ``raw_sigma`` are the decoder's conv outputs, fp32 or both bf16; with ``tail_applied`` they are ``logits`` /
    ``sigma`` as a tail already produced them.  ``padding_mask`` is ``None`` or a row view (``ops.row_view``); a dense mask (yz
    planes) is refused by name, except with ``tail_applied``, where no mask is read: that is how yz-plane models are served.

    Two launches (the per-plane records, then one lane per target pixel) whatever V is; a view's bits do not depend on which
    other views share its call.  With gradients enabled an input that requires grad raises ``ValueError``: ``decoder_tail`` +
    ``plane_sweep_homography`` is the differentiable route."""
    want = (want,) if isinstance(want, str) else tuple(want)
    for w in want:
        if w not in _WANT:
            raise ValueError("want: unknown output %r (rgb is always returned; the optional ones are %s)" % (w, ", ".join(_WANT)))
    B, N, H, W = raw_logits.shape
    mix = bool(use_mixture_loss)
    flags = _storage_flag(raw_logits, raw_sigma, mix) | (C.PD_TAIL_MIXTURE if mix else 0)
    if not torch.is_tensor(T) or T.dim() not in (3, 4) or tuple(T.shape[-2:]) != (4, 4) or (T.dim() == 4 and T.shape[0] != B) \
            or T.shape[-3] < 1:
        raise ValueError("T must be [B,V,4,4] (B = %d) or [V,4,4] with at least one pose, got %s"
                         % (B, tuple(T.shape) if torch.is_tensor(T) else type(T).__name__))
    _infer_no_grad("plane_sweep_homography", "render_poses", raw_logits=raw_logits, raw_sigma=raw_sigma if mix else None,
                   padding_mask=padding_mask, distance=distance, norm=norm, image=image, T=T, K=K, inv_K=inv_K)
    with torch.no_grad():
        pm = None
        if padding_mask is not None and not tail_applied:
            form, pm = PF.mask_operand(padding_mask, B, N, H, W)
            if form != PF.ROWS:
                raise C.PlaneDepthHipError("render_poses: padding_mask is a dense [B,N,H,W] mask (yz planes), which is not served: "
                                           "None or a row view (stride(3) == 0) only, or tail_applied=True, where no mask is read")
            flags |= C.PD_TAIL_MASK_ROWS
        V = T.shape[-3]
        st = raw_logits.dtype
        C.require_gpu_tensor("raw_logits", raw_logits, dtype=st)
        if mix:
            C.require_gpu_tensor("raw_sigma", raw_sigma, (B, N, H, W), dtype=st)
        if pm is not None:
            C.require_gpu_tensor("padding_mask", pm, (B, N, H))
        C.require_gpu_tensor("distance", distance, (B, N))
        C.require_gpu_tensor("norm", norm)
        if tuple(norm.shape) != (B, N, 3):
            norm = norm.expand(B, N, 3)
        C.require_gpu_tensor("image", image, (B, 3, H, W))
        C.require_gpu_tensor("T", T)
        if T.dim() == 3:
            T = T[None].expand(B, V, 4, 4)
        C.require_gpu_tensor("K", K, (B, 4, 4))
        C.require_gpu_tensor("inv_K", inv_K, (B, 4, 4))
        rl, rs, pm, distance, norm, image, T, K, inv_K = (
            None if t is None else _contig(t.detach()) for t in (raw_logits, raw_sigma if mix else None, pm, distance, norm, image,
                                                                 T, K, inv_K))
        flags |= (C.PD_RENDER_TAIL_APPLIED if tail_applied else 0) | (C.PD_RENDER_VISIBLE_ONLY if visible_only else 0)
        dev = rl.device
        new = lambda c: torch.empty(B, V, c, H, W, device=dev, dtype=torch.float32)  # noqa: E731
        rgb = new(3)
        coverage = new(1) if "coverage" in want else None
        disp = new(1) if "disp" in want else None
        workspace = torch.empty(int(C.load().pd_render_poses_workspace_floats(B, N, V)), device=dev, dtype=torch.float32)
        with _timed("render_poses", dev):
            C.call("pd_render_poses", dev, B, N, H, W, V, flags, rl, rs, pm, distance, norm, T, K, inv_K, image, rgb, coverage, disp,
                   workspace)
    return Views(rgb, coverage, disp)
