"""Network tails: DepthDecoder's (networks/depth_decoder.py:258-291) and PladeNet's compositing tail
(networks/plade_net.py:309-341).
"""
import collections
import os

from . import _capi as C
from . import planeform as PF
from ._buffers import torch, _timed, _contig
from .sweep import TailLink

_DISP_FLAG = {PF.PER_PLANE: 0, PF.ROWS: C.PD_TAIL_DISP_ROWS, PF.DENSE: C.PD_TAIL_DISP_DENSE}


def _storage_flag(raw_logits, raw_sigma, mix):
    """PD_TAIL_BF16 or 0 from the conv outputs' dtype: fp32, or bf16 as ``torch.autocast`` emits it (the kernels read and write
    bf16 natively then).  Anything else — and a mixture whose two conv outputs disagree — is a TypeError: no widening copy, no
    torch fall-back."""
    for name, t in (("raw_logits", raw_logits),) + ((("raw_sigma", raw_sigma),) if mix else ()):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("%s must be torch.float32 or torch.bfloat16, got %s" % (name, t.dtype))
    if mix and raw_sigma.dtype != raw_logits.dtype:
        raise TypeError("raw_logits and raw_sigma must have one dtype, got %s and %s" % (raw_logits.dtype, raw_sigma.dtype))
    return C.PD_TAIL_BF16 if raw_logits.dtype == torch.bfloat16 else 0


def _storage_grad(name, g, dtype):
    """An upstream gradient of a storage-typed output (logits / sigma) arrives in that output's dtype."""
    if g is not None and g.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, g.dtype))
    return g


def _decoder_operands(raw_logits, raw_sigma, padding_mask, disp_layered, use_mixture_loss, grad=True):
    """(flags, form, raw_sigma | None, padding_mask, plane) of a decoder tail, training or inference: the storage flag from the conv
    outputs' dtype, ``disp_layered`` and ``padding_mask`` each in its own form (rows from the strides only: this tail takes no
    promise).  ``grad=False``: a forward-only caller, whose ``plane`` is contiguous and carries no autograd path."""
    B, N, H, W = raw_logits.shape
    form, plane = PF.disp_operand(disp_layered, B, N, H, W, grad=grad)
    flags = _storage_flag(raw_logits, raw_sigma, use_mixture_loss) | _DISP_FLAG[form] | (C.PD_TAIL_MIXTURE if use_mixture_loss else 0)
    if padding_mask is not None:
        mask_form, padding_mask = PF.mask_operand(padding_mask, B, N, H, W)
        flags |= C.PD_TAIL_MASK_ROWS if mask_form == PF.ROWS else 0
    return flags, form, (raw_sigma if use_mixture_loss else None), padding_mask, plane


def _plade_operands(raw_logits, raw_sigma, disp_layered, ray_norm, use_mixture_loss, grad=True):
    """(flags, raw_sigma | None, plane, ray_norm) of a PladeNet tail, training or inference (no row form: ``row_views=False``)."""
    B, Nm1, H, W = raw_logits.shape
    form, plane = PF.disp_operand(disp_layered, B, Nm1 + 1, H, W, grad=grad, row_views=False)
    flags = _storage_flag(raw_logits, raw_sigma, use_mixture_loss) | _DISP_FLAG[form] | (C.PD_TAIL_MIXTURE if use_mixture_loss else 0)
    if ray_norm is None:
        ray_norm = camera_ray_norm(H, W, raw_logits.device)
    return flags, (raw_sigma if use_mixture_loss else None), plane, ray_norm


def _checked(flags, N, raw_logits, raw_sigma, disp_layered, name, fourth):
    """A tail's operands as its entry points take them: on the GPU, in the shapes ``flags`` announce, contiguous.  ``fourth`` is the
    decoder tail's ``padding_mask`` (may be None) or the PladeNet tail's ``ray_norm``, as ``name`` says."""
    B, _, H, W = raw_logits.shape
    st = raw_logits.dtype   # storage type of logits / sigma and their gradients (_storage_flag checked it: PD_TAIL_BF16)
    C.require_gpu_tensor("raw_logits", raw_logits, dtype=st)
    if flags & C.PD_TAIL_MIXTURE:
        C.require_gpu_tensor("raw_sigma", raw_sigma, (B, N, H, W), dtype=st)
    C.require_gpu_tensor("disp_layered", disp_layered, (B, N, H, W) if flags & C.PD_TAIL_DISP_DENSE else
                         (B, N, H) if flags & C.PD_TAIL_DISP_ROWS else (B, N))
    if fourth is not None:
        C.require_gpu_tensor(name, fourth, (H, W) if name == "ray_norm" else
                             (B, N, H) if flags & C.PD_TAIL_MASK_ROWS else (B, N, H, W))
    return tuple(map(_contig, (raw_logits, raw_sigma, disp_layered, fourth)))


def _layers_of(entry, N, flags, operands, stash):
    """The ``layers(want_pi=True, want_probability=True)`` of a tail, training or inference: ``(pi, probability)``, fp32 [B,N,H,W]
    (with bf16 conv outputs too), materialised on demand from the stash by ``entry`` (pd_decoder_tail_layers /
    pd_plade_tail_layers) — no gradient: nothing in the reference's losses reads them.  ``operands``: the entry point's inputs
    in its order, ``raw_logits`` first; they are detached and made contiguous when ``layers`` is called.  ``layers.stash`` is what
    pd_*_tail_fwd wrote (the inference kernels write the same bits)."""
    B, _, H, W = operands[0].shape
    dev = operands[0].device

    def layers(want_pi=True, want_probability=True):
        with torch.no_grad():
            pi = torch.empty(B, N, H, W, device=dev, dtype=torch.float32) if want_pi else None
            prob = torch.empty(B, N, H, W, device=dev, dtype=torch.float32) if want_probability else None
            ins = [None if t is None else _contig(t.detach()) for t in operands]
            C.call(entry, dev, B, N, H, W, flags, *ins, stash, pi, prob)
        return pi, prob

    layers.stash = stash
    return layers


def _needs(ctx):
    """Which of (raw_logits, raw_sigma, disp_layered) a tail's backward owes a gradient (raw_sigma: with the mixture only)."""
    return ctx.needs_input_grad[0], ctx.needs_input_grad[1] and bool(ctx.flags & C.PD_TAIL_MIXTURE), ctx.needs_input_grad[2]


def _grad_buffers(lib, needs, raw_logits, raw_sigma, disp_layered, N, own_reduction):
    """What a tail's backward writes: (g_raw_logits, g_raw_sigma, g_disp_layered, workspace), each None where ``needs`` does not
    want it.  The workspace serves the per-plane form's reduction only: ``own_reduction`` = the dense form (nothing to reduce) or
    the row form (reduced inside its kernel)."""
    need_l, need_s, need_d = needs
    B, _, H, W = raw_logits.shape
    ws = None
    if need_d and not own_reduction:
        ws = torch.empty(lib.pd_decoder_tail_bwd_workspace_floats(B, N, H, W), device=raw_logits.device, dtype=torch.float32)
    return (torch.empty_like(raw_logits) if need_l else None, torch.empty_like(raw_sigma) if need_s else None,
            torch.empty_like(disp_layered) if need_d else None, ws)


def _upstream(mix, dtype, g_logits, g_sigma, *fp32):
    """A tail's upstream gradients, contiguous: g_logits / g_sigma in the storage dtype (g_sigma only with the mixture), then
    the fp32 ones."""
    g = tuple(map(_contig, (g_logits, g_sigma if mix else None) + fp32))
    _storage_grad("g_logits", g[0], dtype)
    _storage_grad("g_sigma", g[1], dtype)
    return g

# ---------------------------------------------------------------------------------------------------------------------
# Decoder tail
# ---------------------------------------------------------------------------------------------------------------------
class _DecoderTail(torch.autograd.Function):
    """(raw_logits, raw_sigma, disp_layered[, padding_mask]) -> (logits, sigma, disp, depth, stash)."""

    @staticmethod
    def forward(ctx, raw_logits, raw_sigma, disp_layered, padding_mask, flags, link=None):
        B, N, H, W = raw_logits.shape
        mix = bool(flags & C.PD_TAIL_MIXTURE)
        ctx.link = link
        st = raw_logits.dtype
        raw_logits, raw_sigma, disp_layered, padding_mask = _checked(flags, N, raw_logits, raw_sigma, disp_layered, "padding_mask",
                                                                       padding_mask)
        dev = raw_logits.device
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
        logits = new(B, N, H, W, dtype=st) if padding_mask is not None else None
        sigma = new(B, N, H, W, dtype=st) if mix else None
        disp, depth, stash = new(B, 1, H, W), new(B, 1, H, W), new(B, 2, H, W)
        with _timed("tail_fwd", dev):
            C.call("pd_decoder_tail_fwd", dev, B, N, H, W, flags, raw_logits, raw_sigma, padding_mask, disp_layered, logits,
                   sigma, disp, depth, stash)
        ctx.save_for_backward(raw_logits, raw_sigma, disp_layered, padding_mask, stash, disp)
        ctx.flags = flags
        ctx.mark_non_differentiable(stash)
        ctx.set_materialize_grads(False)   # an output nobody differentiates (depth, usually) arrives as None, not as a zero tensor
        if link is not None:
            link.raw_sigma, link.stash, link.disp = raw_sigma, stash, disp.detach()
            link.mask_rows = padding_mask   # ([B,N,H], contiguous, or None: decoder_tail links no other mask form)
            link.disp_rows = disp_layered if flags & C.PD_TAIL_DISP_ROWS else None
        if logits is None:       # no mask: the logits ARE the conv output (reference: logits * ones)
            logits = raw_logits.view_as(raw_logits)
        if sigma is None:
            sigma = new(0)
            ctx.mark_non_differentiable(sigma)
        return logits, sigma, disp, depth, stash

    @staticmethod
    def backward(ctx, g_logits, g_sigma, g_disp, g_depth, _g_stash):
        lib = C.load()
        raw_logits, raw_sigma, disp_layered, padding_mask, stash, disp = ctx.saved_tensors
        B, N, H, W = raw_logits.shape
        flags = ctx.flags
        mix = bool(flags & C.PD_TAIL_MIXTURE)
        need_l, need_s, need_d = needs = _needs(ctx)
        if not any(needs):
            return None, None, None, None, None, None
        link = ctx.link
        extra = None
        applied = None
        if link is not None:
            link.enter_pass()                            # (a note of another backward pass is not this pass's: TailLink)
            applied, link.applied = link.applied, None   # per-pass state: consumed here
            link.seen.clear()
        if applied is not None:
            # the sweep's backward kernel applied this node's backward already (pd_plane_sweep_bwd_tail): g_logits / g_sigma ARE
            # the conv outputs' gradients, the disparity share went into the sweep's g_plane.  Only an upstream gradient of
            # disp / depth that the sweep did not see is still owed: the plain kernel on that remainder alone, added on top.
            def rest(got, used):
                if got is None:
                    return None
                if used is None:
                    return got
                if got.data_ptr() == used.data_ptr() and got.shape == used.shape:
                    return None
                return got - used
            r_disp, r_depth = rest(g_disp, applied["disp"]), rest(g_depth, applied["depth"])
            if r_disp is None and r_depth is None:
                return (g_logits if need_l else None), (g_sigma if need_s else None), None, None, None, None
            extra = (g_logits, g_sigma)
            g_logits, g_sigma, g_disp, g_depth = None, None, r_disp, r_depth
        g_raw_logits, g_raw_sigma, g_dl, ws = _grad_buffers(lib, needs, raw_logits, raw_sigma, disp_layered, N,
                                                            flags & (C.PD_TAIL_DISP_DENSE | C.PD_TAIL_DISP_ROWS))
        g_logits, g_sigma, g_disp, g_depth = _upstream(mix, raw_logits.dtype, g_logits, g_sigma, g_disp, g_depth)
        with _timed("tail_bwd", raw_logits.device):
            C.call("pd_decoder_tail_bwd", raw_logits.device, B, N, H, W, flags, raw_logits, raw_sigma, padding_mask,
                   disp_layered, stash, disp, g_logits, g_sigma, g_disp, g_depth, g_raw_logits, g_raw_sigma, g_dl, ws)
        if extra is not None:
            if g_raw_logits is not None and extra[0] is not None:
                g_raw_logits += extra[0]
            if g_raw_sigma is not None and extra[1] is not None:
                g_raw_sigma += extra[1]
        return g_raw_logits, g_raw_sigma, g_dl, None, None, None


def decoder_tail(raw_logits, raw_sigma, padding_mask, disp_layered, use_mixture_loss=True, fuse_sweep_backward=False):
    """Tail of DepthDecoder.forward (networks/depth_decoder.py:256-291, softmax branch) in one fused pass.

    Returns (logits, sigma | None, disp, depth, layers) where ``layers()`` materialises ``(pi, probability)`` on demand
    (no gradient: nothing in the reference's losses reads them).  ``disp_layered`` may be the decoder's expanded view of
    per-plane scalars or a dense map; ``padding_mask=None`` means all ones (xy planes only).

    Row form.  A map and / or a mask that is a row view — [B,N,H,W] with ``stride(3) == 0``, what ``plane_geometry`` returns
    (xy + xz planes) — goes in as its [B,N,H] rows (``PD_TAIL_DISP_ROWS`` / ``PD_TAIL_MASK_ROWS``), each tensor in its own form: a
    dense one next to a row view is legal.  The outputs and the conv outputs' gradients have the dense route's bits; the map's
    gradient is [B,N,H], summed over x on the device by the workgroup that owns the row (deterministic).  Nothing
    [B,N,H,W]-sized is read or written for the map and the mask.

    ``raw_logits`` / ``raw_sigma`` are fp32, or both bf16 (``torch.autocast``: PD_TAIL_BF16).  ``logits`` / ``sigma`` and the
    conv outputs' gradients then are bf16 too, each element rounded once from the fp32 value; ``disp``, ``depth``, ``pi`` and
    ``probability`` stay fp32 and come from the unrounded fp32 sigma (the fp32 route on the widened inputs).  With bf16,
    ``fuse_sweep_backward`` takes no tail link: the sweep's bf16 backward and this tail's run as two kernels, with the results of
    ``fuse_sweep_backward=False``.

    ``fuse_sweep_backward=True`` links this tail to the one plane sweep that consumes its logits / sigma (``TailLink``) for
    per-plane scalars AND for the row form — row-view disparities and / or a row-view mask, the reference's default 49 xy + 14 xz
    planes as ``plane_geometry`` returns them.  A dense map or a per-pixel mask gets no link (two kernels, the same results).
    """
    flags, form, raw_sigma, padding_mask, plane = _decoder_operands(raw_logits, raw_sigma, padding_mask, disp_layered,
                                                                    use_mixture_loss)
    # fuse_sweep_backward: the caller's promise that logits / sigma feed (with gradient) exactly ONE plane sweep — the trainer's
    # single-view pred_novel_images — whose backward kernel then applies this tail's backward too (TailLink).  Sweeps are
    # counted (a second one, or one the fused form does not serve, switches the fusion off); any OTHER differentiable consumer
    # of ``sigma`` (a regulariser on outputs["sigma"]) is NOT detected: its gradient would arrive in sigma space on top of one
    # the sweep already wrote in conv-output space, without the sigmoid' factor and the clamp gate.  (``logits`` are safe:
    # d logits / d raw_logits is the identity here.)  Leave the flag off for such a graph.
    # bf16 conv outputs: no link (the row-stream backward's tail form has no bf16 instantiation); two kernels, the same results.
    # Forms that link: disparities per plane or as rows, no mask or a row mask (pd_plane_sweep_bwd_tail / _bwd_tail_rows); a dense
    # map or a per-pixel mask does not.
    link = TailLink(None, None, None) if (fuse_sweep_backward and use_mixture_loss and form != PF.DENSE and
                                           (padding_mask is None or flags & C.PD_TAIL_MASK_ROWS)
                                           and not flags & C.PD_TAIL_BF16 and torch.is_grad_enabled()) else None
    logits, sigma, disp, depth, stash = _DecoderTail.apply(raw_logits, raw_sigma, plane, padding_mask, flags, link)
    if link is not None:
        logits._pd_tail_link = link
        sigma._pd_tail_link = link

    layers = _layers_of("pd_decoder_tail_layers", raw_logits.shape[1], flags, (raw_logits, raw_sigma, padding_mask), stash)
    return logits, (sigma if use_mixture_loss else None), disp, depth, layers


class _PladeTail(torch.autograd.Function):
    """(raw_logits [B,N-1,H,W], raw_sigma, disp_layered, ray_norm) -> (logits, dists, sigma, disp, depth, stash)."""

    @staticmethod
    def forward(ctx, raw_logits, raw_sigma, disp_layered, ray_norm, flags):
        B, Nm1, H, W = raw_logits.shape
        N = Nm1 + 1
        mix = bool(flags & C.PD_TAIL_MIXTURE)
        st = raw_logits.dtype
        raw_logits, raw_sigma, disp_layered, ray_norm = _checked(flags, N, raw_logits, raw_sigma, disp_layered, "ray_norm", ray_norm)
        dev = raw_logits.device
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
        logits, dists = new(B, N, H, W, dtype=st), new(B, N - 1, H, W)
        sigma = new(B, N, H, W, dtype=st) if mix else None
        disp, depth, stash = new(B, 1, H, W), new(B, 1, H, W), new(B, 1, H, W)
        with _timed("plade_fwd", dev):
            C.call("pd_plade_tail_fwd", dev, B, N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm, logits, dists,
                   sigma, disp, depth, stash)
        ctx.save_for_backward(raw_logits, raw_sigma, disp_layered, ray_norm, stash, disp)
        ctx.flags = flags
        ctx.mark_non_differentiable(stash)
        if sigma is None:
            sigma = new(0)
            ctx.mark_non_differentiable(sigma)
        return logits, dists, sigma, disp, depth, stash

    @staticmethod
    def backward(ctx, g_logits, g_dists, g_sigma, g_disp, g_depth, _g_stash):
        lib = C.load()
        raw_logits, raw_sigma, disp_layered, ray_norm, stash, disp = ctx.saved_tensors
        B, Nm1, H, W = raw_logits.shape
        N = Nm1 + 1
        flags = ctx.flags
        needs = _needs(ctx)
        if not any(needs):
            return None, None, None, None, None, None
        g_raw_logits, g_raw_sigma, g_dl, ws = _grad_buffers(lib, needs, raw_logits, raw_sigma, disp_layered, N,
                                                            flags & C.PD_TAIL_DISP_DENSE)
        g_logits, g_sigma, g_dists, g_disp, g_depth = _upstream(bool(flags & C.PD_TAIL_MIXTURE), raw_logits.dtype, g_logits,
                                                                g_sigma, g_dists, g_disp, g_depth)
        C.call("pd_plade_tail_bwd", raw_logits.device, B, N, H, W, flags, raw_logits, raw_sigma, disp_layered, ray_norm, stash,
               disp, g_logits, g_dists, g_sigma, g_disp, g_depth, g_raw_logits, g_raw_sigma, g_dl, ws)
        return g_raw_logits, g_raw_sigma, g_dl, None, None


_RAY_NORM = {}   # (H, W, device) -> [H, W]: the ray lengths depend on the image size only (plade_net.py:314 rebuilds them per call)


def camera_ray_norm(height, width, device):
    """|K^-1 [x, y, 1]| per pixel, [H, W]: torch.linalg.norm(create_camera_plane(H, W), dim=1) of the reference
    (layers.py:468-492, plade_net.py:314-315) — the same fp32 torch.inverse / matmul chain on the host, once per image
    size and device (cached)."""
    key = (height, width, str(device))
    if key not in _RAY_NORM:
        _RAY_NORM[key] = _camera_ray_norm(height, width).to(device)
    return _RAY_NORM[key]


def _camera_ray_norm(height, width):
    K = torch.tensor([[0.58 * width, 0, 0.5 * width], [0, 1.92 * height, 0.5 * height], [0, 0, 1]], dtype=torch.float32)
    K_inv = torch.inverse(K)
    ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(height * width)], 0)
    return torch.linalg.norm(torch.matmul(K_inv, pix).reshape(3, height, width), dim=0).contiguous()


def plade_tail(raw_logits, raw_sigma, disp_layered, ray_norm=None, use_mixture_loss=True):
    """Tail of PladeNet.forward with --render_probability (networks/plade_net.py:309-341) in one fused pass.

    ``raw_logits`` [B,N-1,H,W] = conv0's output, ``raw_sigma`` [B,N,H,W] = conv_sigma's (mixture only), ``disp_layered`` the
    network's expanded view of per-plane scalars or a dense map (ground planes).  Returns (logits [B,N,H,W], dists
    [B,N-1,H,W], sigma | None, disp, depth, layers) where ``layers()`` materialises ``(pi, probability)`` on demand (no
    gradient: nothing in the reference's losses reads them).  bf16 conv outputs (``torch.autocast``) are taken natively under the
    rule of ``decoder_tail``: ``logits`` / ``sigma`` and the conv outputs' gradients are bf16, ``dists`` and the rest fp32.
    This tail has no row form: a row view (``plane_geometry``'s ``disp_layered``, ``stride(3) == 0``) is materialised to the dense
    map by ``_contig`` — correct, and no faster than a dense map."""
    flags, raw_sigma, plane, ray_norm = _plade_operands(raw_logits, raw_sigma, disp_layered, ray_norm, use_mixture_loss)
    logits, dists, sigma, disp, depth, stash = _PladeTail.apply(raw_logits, raw_sigma, plane, ray_norm, flags)

    layers = _layers_of("pd_plade_tail_layers", raw_logits.shape[1] + 1, flags, (raw_logits, raw_sigma, plane, ray_norm), stash)
    return logits, dists, (sigma if use_mixture_loss else None), disp, depth, layers


# ---------------------------------------------------------------------------------------------------------------------
# Inference tails: forward only, nothing [B,N,H,W]-sized written (pd_decoder_tail_infer / pd_plade_tail_infer)
# ---------------------------------------------------------------------------------------------------------------------
InferenceTail = collections.namedtuple("InferenceTail", "disp depth confidence plane_index disp_best layers")
_INFER_WANT = ("depth", "confidence", "plane_index", "disp_best", "layers")


def _infer_want(want):
    want = (want,) if isinstance(want, str) else tuple(want)
    for w in want:
        if w not in _INFER_WANT:
            raise ValueError("want: unknown output %r (disp is always returned; the optional ones are %s)"
                             % (w, ", ".join(_INFER_WANT)))
    return want


def _infer_no_grad(differentiable, operator=None, **tensors):
    """The inference tails build no autograd node: an input that asks for a gradient is a caller's mistake, not a silent detach.
    ``operator``: the forward-only caller's name where it is not ``<differentiable>_inference`` (``render_views``)."""
    if torch.is_grad_enabled():
        for name, t in tensors.items():
            if torch.is_tensor(t) and t.requires_grad:
                raise ValueError("%s requires grad, but %s is forward-only: call it under torch.no_grad(), or use "
                                 "ops.%s, the differentiable operator" % (name, operator or differentiable + "_inference",
                                                                           differentiable))


def _infer_outputs(B, H, W, dev, want, stash_channels):
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
    return (new(B, 1, H, W),
            new(B, 1, H, W) if "depth" in want else None,
            new(B, 1, H, W) if "confidence" in want else None,
            new(B, 1, H, W, dtype=torch.int32) if "plane_index" in want else None,
            new(B, 1, H, W) if "disp_best" in want else None,
            new(B, stash_channels, H, W) if "layers" in want else None)


def decoder_tail_inference(raw_logits, raw_sigma, padding_mask, disp_layered, use_mixture_loss=True,
                           want=("depth", "confidence")):
    """``decoder_tail`` for inference: ``disp`` and, as ``want`` names them, ``depth``, ``confidence`` (``max_n probability_n``,
    fp32 [B,1,H,W]), ``plane_index`` (int32: the plane that attains it, the lowest index among equal maxima — the
    ``candidates_idx`` of depth_decoder.py:286), ``disp_best`` (``disp_layered`` at that plane) and ``layers`` (the stash is then
    kept and ``layers()`` materialises ``(pi, probability)`` on demand, as ``decoder_tail``'s does).  Returns the named tuple
    ``(disp, depth, confidence, plane_index, disp_best, layers)``; what was not asked for is ``None``.

    One forward-only kernel (``pd_decoder_tail_infer``) that writes nothing [B,N,H,W]-sized — no ``logits``, no ``sigma`` — where
    ``decoder_tail`` under ``no_grad`` writes both.  ``disp`` / ``depth`` have ``decoder_tail``'s bits.  Inputs, their forms (per
    plane, row views recognised by their strides, dense) and dtypes (fp32, or both conv outputs bf16) are ``decoder_tail``'s.
    The results carry no autograd node: with gradients enabled an input that requires grad raises ``ValueError`` —
    ``decoder_tail`` is the differentiable operator."""
    want = _infer_want(want)
    B, N, H, W = raw_logits.shape
    _storage_flag(raw_logits, raw_sigma, use_mixture_loss)   # (a wrong dtype is reported before anything else)
    _infer_no_grad("decoder_tail", raw_logits=raw_logits, raw_sigma=raw_sigma if use_mixture_loss else None,
                   padding_mask=padding_mask, disp_layered=disp_layered)
    with torch.no_grad():
        flags, _, raw_sigma, padding_mask, plane = _decoder_operands(raw_logits, raw_sigma, padding_mask, disp_layered,
                                                                     use_mixture_loss, grad=False)
        rl, rs, dl, pm = _checked(flags, N, raw_logits.detach(), None if raw_sigma is None else raw_sigma.detach(), plane,
                                  "padding_mask", padding_mask)
        dev = rl.device
        disp, depth, conf, index, best, stash = _infer_outputs(B, H, W, dev, want, 2)
        with _timed("tail_infer", dev):
            C.call("pd_decoder_tail_infer", dev, B, N, H, W, flags, rl, rs, pm, dl, disp, depth, conf, index, best, stash)
    layers = _layers_of("pd_decoder_tail_layers", N, flags, (rl, rs, pm), stash) if stash is not None else None
    return InferenceTail(disp, depth, conf, index, best, layers)


def plade_tail_inference(raw_logits, raw_sigma, disp_layered, ray_norm=None, use_mixture_loss=True,
                         want=("depth", "confidence")):
    """``plade_tail`` for inference, with ``decoder_tail_inference``'s outputs and rules: one forward-only kernel
    (``pd_plade_tail_infer``) that writes none of ``logits``, ``dists`` and ``sigma``.  ``raw_logits`` [B,N-1,H,W], ``raw_sigma``
    [B,N,H,W] (mixture only), ``disp_layered`` per plane or dense (a row view is materialised: this tail has no row form).
    ``confidence`` is ``layers()``'s ``probability.amax(1)``; ``plade_tail`` is the differentiable operator."""
    want = _infer_want(want)
    B, Nm1, H, W = raw_logits.shape
    N = Nm1 + 1
    _storage_flag(raw_logits, raw_sigma, use_mixture_loss)   # (a wrong dtype is reported before anything else)
    _infer_no_grad("plade_tail", raw_logits=raw_logits, raw_sigma=raw_sigma if use_mixture_loss else None,
                   disp_layered=disp_layered, ray_norm=ray_norm)
    with torch.no_grad():
        flags, raw_sigma, plane, ray_norm = _plade_operands(raw_logits, raw_sigma, disp_layered, ray_norm, use_mixture_loss,
                                                            grad=False)
        rl, rs, dl, ray = _checked(flags, N, raw_logits.detach(), None if raw_sigma is None else raw_sigma.detach(), plane,
                                   "ray_norm", ray_norm.detach())
        dev = rl.device
        disp, depth, conf, index, best, stash = _infer_outputs(B, H, W, dev, want, 1)
        with _timed("plade_infer", dev):
            C.call("pd_plade_tail_infer", dev, B, N, H, W, flags, rl, rs, dl, ray, disp, depth, conf, index, best, stash)
    layers = _layers_of("pd_plade_tail_layers", N, flags, (rl, rs, dl, ray), stash) if stash is not None else None
    return InferenceTail(disp, depth, conf, index, best, layers)


# ---------------------------------------------------------------------------------------------------------------------
# The decoders' disparity levels (networks/depth_decoder.py:147-152, networks/plade_net.py:280-285)
# ---------------------------------------------------------------------------------------------------------------------
class _PlaneLevels(torch.autograd.Function):
    """levels [B,N] -> (disp [B,N], distance [B,N]); one launch each way instead of ~5 + ~8 elementwise ones."""

    @staticmethod
    def forward(ctx, levels, no_levels, disp_min, disp_max, dist_num):
        C.require_gpu_tensor("levels", levels)
        levels = _contig(levels)
        disp, distance = torch.empty_like(levels), torch.empty_like(levels)
        C.call("pd_plane_levels_fwd", levels.device, levels.numel(), int(no_levels), float(disp_min), float(disp_max),
               float(dist_num), levels, disp, distance)
        ctx.save_for_backward(disp)
        ctx.cfg = (int(no_levels), float(disp_min), float(disp_max), float(dist_num))
        return disp, distance

    @staticmethod
    def backward(ctx, g_disp, g_distance):
        disp, = ctx.saved_tensors
        g = torch.empty_like(disp)
        g_disp, g_distance = _contig(g_disp), _contig(g_distance)
        C.call("pd_plane_levels_bwd", disp.device, disp.numel(), *ctx.cfg, disp, g_disp, g_distance, g)
        return g, None, None, None, None


def plane_disparities(levels, disp_min, disp_max, width, no_levels=None):
    """``disp_max * (disp_min / disp_max) ** (levels / (no_levels - 1))`` and ``0.1 * 0.58 * W / that`` of the decoders
    (networks/depth_decoder.py:150-152): ``levels`` [B,N,1,1] or [B,N] = arange(no_levels) (+ the plane residual).  Returns
    (disp_layered [B,N,1,1] — expand it over H, W as the decoder does —, distance [B,N]); gradients flow into ``levels``."""
    B, N = levels.shape[:2]
    disp, distance = _PlaneLevels.apply(levels.reshape(B, N), N if no_levels is None else no_levels, disp_min, disp_max,
                                        0.1 * 0.58 * width)
    return disp.reshape(B, N, 1, 1), distance


# ---------------------------------------------------------------------------------------------------------------------
# The decoder's geometry head in row form (networks/depth_decoder.py:148-207, yz_levels == 0)
# ---------------------------------------------------------------------------------------------------------------------
class _PlaneGeometry(torch.autograd.Function):
    """(grid [B,2,H,W], residual [B,N] | None) -> (disp_rows [B,N,H], mask_rows [B,N,H], distance [B,N], norm [B,N,3]); one launch
    each way (pd_plane_geometry_fwd / _bwd).  Gradients flow into ``residual`` from ``disp_rows`` and ``distance``."""

    @staticmethod
    def forward(ctx, grid, residual, cfg):
        no_levels, xz_levels = cfg[0], cfg[1]
        B, _, H, W = grid.shape
        N = no_levels + xz_levels
        grid, residual = _contig(grid), _contig(residual)
        dev = grid.device
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
        disp_rows, mask_rows, distance, norm = new(B, N, H), new(B, N, H), new(B, N), new(B, N, 3)
        with _timed("plane_geometry_fwd", dev):
            C.call("pd_plane_geometry_fwd", dev, B, no_levels, xz_levels, H, W, 0, *cfg[2:], residual, grid, disp_rows,
                   mask_rows, distance, norm)
        ctx.save_for_backward(grid, residual, disp_rows)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(mask_rows, norm)
        ctx.set_materialize_grads(False)
        return disp_rows, mask_rows, distance, norm

    @staticmethod
    def backward(ctx, g_rows, _g_mask, g_distance, _g_norm):
        grid, residual, disp_rows = ctx.saved_tensors
        if residual is None or not ctx.needs_input_grad[1] or (g_rows is None and g_distance is None):
            return None, None, None
        B, _, H, W = grid.shape
        g_rows, g_distance = _contig(g_rows), _contig(g_distance)
        g_residual = torch.empty_like(residual)
        with _timed("plane_geometry_bwd", grid.device):
            C.call("pd_plane_geometry_bwd", grid.device, B, ctx.cfg[0], ctx.cfg[1], H, W, 0, *ctx.cfg[2:], residual, grid,
                   disp_rows, g_rows, g_distance, g_residual)
        return None, g_residual, None


def plane_geometry(grid, residual, *, no_levels, xz_levels, disp_min, disp_max, xz_min, xz_max, check_contract=None):
    """The geometry head of ``DepthDecoder.forward`` for xy + xz planes (networks/depth_decoder.py:148-207, ``yz_levels == 0``) as
    one autograd node: ``grid`` = ``inputs["grid"]`` [B,2,H,W], ``residual`` = ``sigmoid(residualconv) - 0.5`` as [B,N] or
    [B,N,1,1] (N = no_levels + xz_levels; ``None`` without ``--plane_residual``).  Returns ``(disp_layered, padding_mask,
    distance [B,N], norm [B,N,3])``: ``disp_layered`` and ``padding_mask`` (float 0 / 1) have the reference's shape [B,N,H,W]
    and are ROW VIEWS — ``stride(3) == 0`` over [B,N,H] row tensors; nothing [B,N,H,W]-sized exists behind them.
    ``decoder_tail``, ``plane_sweep_disp``, ``post_process_disp`` and the trainer path recognise such a view by its strides and
    take their row forms with no ``row_uniform`` promise.

    Gradients reach ``residual`` through ``disp_layered`` and ``distance``.  The package's row consumers hang on the rows
    tensor's node directly (their gradient is [B,N,H]); a foreign torch consumer of the view gets the right gradient as well
    (``_RowView``: summed over x; a gradient that is itself constant along x is not touched W times).

    The y channel of ``grid`` is taken to be constant along x and the x extent of a row is taken from its first and last column:
    true for every grid datasets/pair_transforms.py makes.  ``check_contract=True`` (default: the environment's
    ``PD_CHECK_CONTRACT``) verifies the y channel on the data (one reduction and a host sync) and raises ``ValueError``; a
    sheared or rotated grid must keep the reference's dense lines."""
    C.require_gpu_tensor("grid", grid)
    if grid.dim() != 4 or grid.shape[1] != 2:
        raise ValueError("grid must be [B,2,H,W], got %s" % (tuple(grid.shape),))
    B, _, H, W = grid.shape
    no_levels, xz_levels = int(no_levels), int(xz_levels)
    N = no_levels + xz_levels
    if residual is not None:
        C.require_gpu_tensor("residual", residual)
        if tuple(residual.shape) not in ((B, N), (B, N, 1, 1)):
            raise ValueError("residual must be [B,N] or [B,N,1,1] with N = no_levels + xz_levels = %d, got %s"
                             % (N, tuple(residual.shape)))
        residual = residual.reshape(B, N)
    if check_contract is None:
        check_contract = bool(os.environ.get("PD_CHECK_CONTRACT"))
    if check_contract and xz_levels > 0 and not bool((grid[:, 1] == grid[:, 1, :, :1]).all()):
        raise ValueError("plane_geometry takes a grid whose y channel is constant along x, but this one is not (a sheared or "
                         "rotated grid must keep the reference's dense geometry)")
    cfg = (no_levels, xz_levels, float(disp_min), float(disp_max), float(xz_min), float(xz_max))
    disp_rows, mask_rows, distance, norm = _PlaneGeometry.apply(grid, residual, cfg)
    return PF.row_view(disp_rows, W), PF.row_view(mask_rows, W), distance, norm
