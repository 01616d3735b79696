"""The decoders' positional encoding of ``inputs["grid"]`` as one operator: embedding and bilinear pyramid, forward and backward.

``DepthDecoder.forward`` (networks/depth_decoder.py:123-139) runs ``epconv`` — ``Conv2d(2,16,1)``, ELU, ``Conv2d(16,num_ep,1)``, ELU —
on the full-resolution grid ``[B,2,H,W]`` and then calls ``F.interpolate(bilinear, align_corners=True)`` once per decoder level;
``PoseDecoder.forward`` (networks/pose_net.py:137-140) does the same for one level, ``PladeNet`` (networks/plade_net.py:150-158)
resamples the raw grid, and ``--pe_type frequency`` swaps the MLP for ``layers.get_embedder``.  Every pixel of those small maps
depends on four grid points, so ``grid_embedding`` evaluates the embedding there and blends (``pd_grid_embed_fwd``: one launch for all
levels); the backward recomputes from the grid and reduces the parameter gradients (``pd_grid_embed_bwd``).  Nothing of the size
``[B,.,H,W]`` is written or kept for backward.  ``fused_grid_embedding`` takes the reference's own module.  No eager / CPU
implementation stands behind the operator.
"""
import ctypes

import torch

from . import _capi as C

HIDDEN = 16        # the reference hard-codes Conv2d(2, 16, 1)
MAX_LEVELS = 8
KINDS = {"neural": C.PD_EMBED_NEURAL, "frequency": C.PD_EMBED_FREQUENCY, "identity": C.PD_EMBED_IDENTITY}


def _sizes_array(sizes):
    return (ctypes.c_int32 * (2 * len(sizes)))(*[v for hw in sizes for v in hw])


def _split(flat, B, E, sizes):
    """The levels' ``[B,E,h,w]`` views of the flat buffer."""
    out, at = [], 0
    for h, w in sizes:
        n = B * E * h * w
        out.append(flat[at:at + n].view(B, E, h, w))
        at += n
    return tuple(out)


def _launch_fwd(grid, sizes, kind, E, multires, params):
    B, _, H, W = (int(s) for s in grid.shape)
    flat = torch.empty(B * E * sum(h * w for h, w in sizes), device=grid.device, dtype=torch.float32)
    C.call("pd_grid_embed_fwd", grid.device, B, H, W, kind, E, multires, len(sizes), _sizes_array(sizes), grid, params, flat)
    return flat


class _GridEmbedding(torch.autograd.Function):
    """Neural kind: (grid, w1, b1, w2, b2) -> the levels.  Saves the grid and the packed parameters, nothing computed."""

    @staticmethod
    def forward(ctx, grid, sizes, w1, b1, w2, b2):
        E = int(w2.shape[0])
        with torch.no_grad():
            params = torch.cat([w1.reshape(-1), b1.reshape(-1), w2.reshape(-1), b2.reshape(-1)]).float().contiguous()
        flat = _launch_fwd(grid, sizes, C.PD_EMBED_NEURAL, E, 0, params)
        ctx.save_for_backward(grid, params)
        ctx.sizes, ctx.E = sizes, E
        ctx.shapes = (w1.shape, b1.shape, w2.shape, b2.shape)
        ctx.dtypes = (w1.dtype, b1.dtype, w2.dtype, b2.dtype)
        return _split(flat, int(grid.shape[0]), E, sizes)

    @staticmethod
    def backward(ctx, *g_levels):
        lib = C.load()
        grid, params = ctx.saved_tensors
        sizes, E = ctx.sizes, ctx.E
        B, _, H, W = (int(s) for s in grid.shape)
        dev = grid.device
        parts = []
        for g, (h, w) in zip(g_levels, sizes):   # the levels' gradients in the forward's flat layout (a level nobody used: zeros)
            parts.append(torch.zeros(B * E * h * w, device=dev) if g is None else g.float().reshape(-1))
        g_out = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)
        arr = _sizes_array(sizes)
        ws = torch.empty(int(lib.pd_grid_embed_bwd_workspace_floats(B, E, len(sizes), arr)), device=dev, dtype=torch.float32)
        g_params = torch.empty_like(params)
        C.call("pd_grid_embed_bwd", dev, B, H, W, E, len(sizes), arr, grid, params, g_out, g_params, ws)
        cuts = (0, 2 * HIDDEN, 3 * HIDDEN, 3 * HIDDEN + E * HIDDEN, 3 * HIDDEN + E * HIDDEN + E)
        grads = tuple(g_params[cuts[k]:cuts[k + 1]].view(ctx.shapes[k]).to(ctx.dtypes[k]) if ctx.needs_input_grad[2 + k] else None
                      for k in range(4))
        return (None, None) + grads


def _check_sizes(sizes):
    try:
        sizes = tuple((int(h), int(w)) for h, w in sizes)
    except (TypeError, ValueError):
        raise TypeError("sizes must be a sequence of (h, w) pairs")
    if not 1 <= len(sizes) <= MAX_LEVELS:
        raise ValueError("sizes holds %d levels: 1 to %d per call" % (len(sizes), MAX_LEVELS))
    for l, (h, w) in enumerate(sizes):
        if h < 1 or w < 1:
            raise ValueError("sizes[%d] = (%d, %d): every side must be >= 1" % (l, h, w))
    return sizes


def grid_embedding(grid, sizes, weights=None, *, kind="neural", multires=None):
    """The embedding of ``grid`` ``[B,2,H,W]`` resampled (bilinear, ``align_corners=True``) to every ``(h, w)`` of ``sizes`` (1 to 8
    levels, any sizes): a tuple of ``[B,E,h,w]`` fp32 tensors, views of one allocation, from one launch.

    ``kind="neural"``: ``weights = (w1, b1, w2, b2)`` of ``ELU(conv1x1(ELU(conv1x1(grid))))`` with 16 hidden channels — ``w1``
    ``[16,2]`` or conv-shaped ``[16,2,1,1]``, ``b1`` ``[16]``, ``w2`` ``[E,16]`` or ``[E,16,1,1]``, ``b2`` ``[E]``, 1 <= E <= 16;
    differentiable in the four parameters (no gradient for ``grid``: ``ValueError`` if it requires one).  ``kind="frequency"``:
    ``cat(g, sin(g 2^k), cos(g 2^k))`` for k < ``multires`` in ``layers.Embedder``'s channel order, E = 2 + 4 multires.
    ``kind="identity"``: the grid itself, E = 2.  The last two take no weights.  Under ``torch.autocast`` the result is computed and
    returned in fp32.  ``PlaneDepthHipError`` for CPU tensors: there is no fallback."""
    if kind not in KINDS:
        raise ValueError("kind %r is none of %s" % (kind, sorted(KINDS)))
    if not torch.is_tensor(grid):
        raise TypeError("grid must be a tensor")
    if grid.dim() != 4 or grid.shape[1] != 2:
        raise ValueError("grid must be [B,2,H,W], got %s" % (tuple(grid.shape),))
    if grid.requires_grad:
        raise ValueError("grid requires a gradient: grid_embedding has none for it (the reference's grid never requires one)")
    sizes = _check_sizes(sizes)
    B = int(grid.shape[0])
    if kind != "neural":
        if weights is not None:
            raise ValueError("kind %r takes no weights" % kind)
        if kind == "identity":
            if multires not in (None, 0):
                raise ValueError("kind 'identity' takes no multires")
            multires = 0
        elif multires is None or int(multires) < 0:
            raise ValueError("kind 'frequency' needs multires >= 0, got %r" % (multires,))
        multires = int(multires)
        E = 2 + 4 * multires
        C.require_gpu_tensor("grid", grid)
        with torch.no_grad():
            return _split(_launch_fwd(grid.contiguous(), sizes, KINDS[kind], E, multires, None), B, E, sizes)
    if multires is not None:
        raise ValueError("kind 'neural' takes no multires")
    if weights is None or len(weights) != 4:
        raise ValueError("kind 'neural' needs weights = (w1, b1, w2, b2)")
    w1, b1, w2, b2 = weights
    for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
    E = int(w2.shape[0]) if w2.dim() >= 1 else 0
    for name, t, shapes in (("w1", w1, ((HIDDEN, 2), (HIDDEN, 2, 1, 1))), ("b1", b1, ((HIDDEN,),)),
                            ("w2", w2, ((E, HIDDEN), (E, HIDDEN, 1, 1))), ("b2", b2, ((E,),))):
        if tuple(t.shape) not in shapes:
            raise ValueError("%s must have shape %s, got %s" % (name, " or ".join(str(list(s)) for s in shapes), tuple(t.shape)))
        if not t.is_floating_point():
            raise TypeError("%s must be a floating-point tensor, got %s" % (name, t.dtype))
    if not 1 <= E <= 16:
        raise ValueError("w2 has %d output channels: 1 to 16" % E)
    C.require_gpu_tensor("grid", grid)   # arguments first, devices last: what is wrong with a call does not depend on where it runs
    for name, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if not t.is_cuda:
            raise C.PlaneDepthHipError("%s is on %s: planedepth_amd runs on the GPU only (no CPU fallback)" % (name, t.device))
    return _GridEmbedding.apply(grid.contiguous(), sizes, w1, b1, w2, b2)


def _describe(m):
    if isinstance(m, torch.nn.Conv2d):
        return "Conv2d(%d, %d, kernel_size=%s)" % (m.in_channels, m.out_channels, tuple(m.kernel_size))
    return type(m).__name__


def _conv1x1(m, where, c_in, c_out=None):
    if not isinstance(m, torch.nn.Conv2d):
        raise ValueError("epconv[%d] is %s, expected Conv2d(%d, %s, 1)" % (where, _describe(m), c_in, c_out or "num_ep"))
    ok = (m.in_channels == c_in and (c_out is None or m.out_channels == c_out) and tuple(m.kernel_size) == (1, 1)
          and tuple(m.stride) == (1, 1) and tuple(m.padding) == (0, 0) and tuple(m.dilation) == (1, 1) and m.groups == 1
          and m.bias is not None)
    if not ok:
        raise ValueError("epconv[%d] is %s (stride %s, padding %s, groups %d, bias %s), expected Conv2d(%d, %s, kernel_size=1) with "
                         "a bias" % (where, _describe(m), tuple(m.stride), tuple(m.padding), m.groups, m.bias is not None, c_in,
                                     c_out or "num_ep"))
    return m


def _elu(m, where):
    if not isinstance(m, torch.nn.ELU) or m.alpha != 1.0:
        raise ValueError("epconv[%d] is %s, expected ELU(alpha=1)" % (where, _describe(m)))


def fused_grid_embedding(epconv, grid, sizes):
    """``[F.interpolate(epconv(grid), size=s, mode="bilinear", align_corners=True) for s in sizes]`` in one launch, from the
    reference's own module: the four-element ``nn.Sequential`` of networks/depth_decoder.py:66-71 / networks/pose_net.py:116-121
    (gradients reach its parameters), an ``Embedder``-shaped object (layers.py:308-354, recognised by its ``kwargs``), or ``None``
    for the raw grid (networks/plade_net.py:150-158).  Any other structure: ``ValueError`` naming what differs."""
    if epconv is None:
        return grid_embedding(grid, sizes, kind="identity")
    kw = getattr(epconv, "kwargs", None)
    if isinstance(kw, dict) and "num_freqs" in kw:
        n = int(kw["num_freqs"])
        want = dict(include_input=True, input_dims=2, max_freq_log2=n - 1, log_sampling=True)
        for key, v in want.items():
            if kw.get(key) != v:
                raise ValueError("Embedder has %s = %r, the fused embedding covers %r (layers.get_embedder)" % (key, kw.get(key), v))
        fns = list(kw.get("periodic_fns", ()))
        if fns != [torch.sin, torch.cos]:
            raise ValueError("Embedder has periodic_fns = %r, the fused embedding covers [torch.sin, torch.cos]" % (fns,))
        return grid_embedding(grid, sizes, kind="frequency", multires=n)
    if not isinstance(epconv, torch.nn.Sequential):
        raise ValueError("epconv is %s, expected nn.Sequential(Conv2d(2,16,1), ELU, Conv2d(16,num_ep,1), ELU), an Embedder or None"
                         % _describe(epconv))
    if len(epconv) != 4:
        raise ValueError("epconv has %d elements, expected 4: Conv2d(2,16,1), ELU, Conv2d(16,num_ep,1), ELU" % len(epconv))
    c1 = _conv1x1(epconv[0], 0, 2, HIDDEN)
    _elu(epconv[1], 1)
    c2 = _conv1x1(epconv[2], 2, HIDDEN)
    _elu(epconv[3], 3)
    return grid_embedding(grid, sizes, (c1.weight, c1.bias, c2.weight, c2.bias))


def decoder_embedding_sizes(input_features):
    """The five sizes ``DepthDecoder.forward`` asks for, in its order (networks/depth_decoder.py:127-139): the deepest feature's
    size, then twice that after each of the upsamplings i = 4 .. 1 (nearest, scale 2)."""
    h, w = (int(s) for s in input_features[-1].shape[2:4])
    return tuple((h << k, w << k) for k in range(5))
