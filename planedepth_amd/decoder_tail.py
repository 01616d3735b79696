"""Drop-in for the tail of the reference ``DepthDecoder.forward`` (networks/depth_decoder.py:256-291, softmax branch).

The reference computes, after its last convolutions::

    logits = self.convs["dispconv"](x) * padding_mask ; probability = softmax(logits)
    sigma = clamp(sigmoid(self.convs["sigmaconv"](x)), 0.01, 1) ; pi = probability
    probability = (pi / sigma * padding_mask) / sum ; disp = sum(probability * disp_layered) ; depth = 0.1*0.58*W/disp

as ~12 full-tensor passes.  ``fused_decoder_tail`` does it in one HIP kernel (and one for the backward) and writes the
same ``outputs`` entries.  It stays opt-in because ``networks/*`` are meant to drop in unchanged:
a maintainer replaces lines 256-291 of ``depth_decoder.py`` with::

    from planedepth_amd.decoder_tail import fused_decoder_tail
    fused_decoder_tail(self.outputs, self.convs["dispconv"](x),
                       self.convs["sigmaconv"](x) if self.use_mixture_loss else None,
                       use_mixture_loss=self.use_mixture_loss, all_ones_mask=(self.xz_levels + self.yz_levels == 0))

``DepthDecoder`` with ``--render_probability`` keeps the reference's own code (its compositing branch raises on its own: the
padding mask has N channels, ``dispconv`` N-1).  The live producer of ``outputs["dists"]`` is ``PladeNet``
(networks/plade_net.py:309-341), whose tail ``fused_plade_tail`` replaces the same way: lines 309-340 become::

    from planedepth_amd.decoder_tail import fused_plade_tail
    fused_plade_tail(self.outputs, self.conv0(dlog), self.conv_sigma(features) if self.use_mixture_loss else None,
                     use_mixture_loss=self.use_mixture_loss)

Geometry head.  With xy + xz planes (``--xz_levels 14``, the reference's default plane set) the lines in front of the tail,
depth_decoder.py:148-257, build dense [B,N,H,W] maps for information that is [B,N,H]-sized.  ``fused_plane_geometry`` replaces
them with one kernel each way and hands ``outputs["disp_layered"]`` / ``["padding_mask"]`` over as row views (reference shape,
``stride(3) == 0``); the tail, the sweep and the post-process recognise the strides and take their row forms::

    from planedepth_amd.decoder_tail import fused_plane_geometry, fused_decoder_tail
    residual = self.sigmoid(self.convs["residualconv"](x)) - 0.5 if self.plane_residual else None
    fused_plane_geometry(self.outputs, input_grids, residual, no_levels=self.no_levels, xz_levels=self.xz_levels,
                         disp_min=self.disp_min, disp_max=self.disp_max, xz_min=self.xz_min, xz_max=self.xz_max)
    fused_decoder_tail(self.outputs, self.convs["dispconv"](x), ...)

With ``yz_levels > 0`` (disparities that vary along x) the reference's lines stay.

Mixed precision.  Under ``torch.autocast("cuda", dtype=torch.bfloat16)`` the convolutions emit bf16, and both tails take it as
it is (``PD_TAIL_BF16``; no ``.float()`` on the conv outputs, which would bring the [B,N,H,W] fp32 activations and gradients
back).  ``outputs["logits"]`` / ``["sigma"]`` are then bf16 — what the plane sweep reads natively — and so
are the gradients handed back to the convolutions; ``disp``, ``depth``, ``dists``, ``pi`` and ``probability`` stay fp32.
The arithmetic is the fp32 kernels' on the exactly widened inputs, and every bf16 element is rounded once from its fp32
value.  One deliberate difference from the reference under autocast, which would carry a bf16-rounded sigma into
``probability``: here ``disp`` / ``depth`` / ``probability`` use the unrounded fp32 sigma, and ``outputs["sigma"]`` is that
sigma rounded once (never below the sweep's clamp: bf16(0.01) >= 0.01).  Both conv outputs must have one dtype; fp16 and a
bf16 / fp32 mix raise ``TypeError``.
"""
import torch

from . import ops


class LazyLayers:
    """``outputs["probability"]`` / ``outputs["pi"]`` stand-in: has ``.shape`` (all the training loop reads,
    trainer.py:528, 610, 704) and materialises the tensor on first real use."""

    def __init__(self, shape, make, device=None, dtype=None):
        self.shape = tuple(shape)
        self.device = device
        self.dtype = dtype
        self._make = make
        self._value = None

    def dim(self):
        return len(self.shape)

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def tensor(self):
        """The materialised [B,N,H,W] tensor.  It carries NO gradient (nothing in the reference's losses back-propagates
        through ``probability`` / ``pi``: trainer.py reads them for their shape, the post-process under no_grad)."""
        if self._value is None:
            if torch.is_grad_enabled() and not getattr(LazyLayers, "_warned", False):
                import warnings
                LazyLayers._warned = True
                warnings.warn("planedepth_amd: outputs['probability'] / outputs['pi'] of the fused decoder tail are "
                              "materialised WITHOUT gradient (the reference's losses never back-propagate through them; "
                              "gradients flow through 'disp', 'logits' and 'sigma').  Use the unfused decoder if a custom "
                              "loss needs them differentiable.", stacklevel=3)
            self._value = self._make()
        return self._value

    def __getattr__(self, name):          # anything beyond shape / device / dtype: behave like the tensor
        # private and dunder names are never forwarded: copy / pickle look them up on objects created without __init__,
        # where forwarding would recurse through `_value` for ever
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.tensor(), name)

    def __getitem__(self, idx):
        return self.tensor()[idx]


def fused_decoder_tail(outputs, dispconv_out, sigmaconv_out=None, *, use_mixture_loss=True, all_ones_mask=False,
                       materialize_layers=False, fuse_sweep_backward=False):
    """Fills ``outputs`` with "logits", "sigma", "pi", "probability", "disp", "depth" as depth_decoder.py:258-291 does.
    Reads ``outputs["disp_layered"]`` and ``outputs["padding_mask"]`` (skipped when ``all_ones_mask`` says the decoder
    built it with ``torch.ones_like``, i.e. xy planes only).

    ``fuse_sweep_backward=True`` (mixture loss, one target view; xy planes, or xy + xz planes in the row form that
    ``fused_plane_geometry`` puts into ``outputs``): the promise that ``outputs["logits"]`` / ``["sigma"]`` are consumed — as far
    as gradients go — by the trainer's plane sweep alone.  The sweep's backward kernel then applies this tail's backward on the
    values it holds anyway and writes the conv outputs' gradients directly (``ops.TailLink``; ``pd_plane_sweep_bwd_tail``, or
    ``pd_plane_sweep_bwd_tail_rows`` for row-view disparities / a row-view mask — the views' strides decide, there is no switch);
    the tail's own backward kernel, which re-reads the [B,N,H,W]-sized gradients the sweep has just written, no longer runs.  A
    dense ``disp_layered`` or a per-pixel ``padding_mask`` (yz planes) takes no link: two kernels, the same results.  NOT detected: another differentiable consumer of ``outputs["sigma"]``
    (a regulariser) — its gradient would be added, in sigma space, to one already in conv-output space; keep the flag off then.
    With bf16 conv outputs (autocast) the flag is accepted and no link is made: the sweep's fused backward has no bf16 form, so
    the sweep's native bf16 backward and then this tail's run as two kernels, with the results of ``fuse_sweep_backward=False``."""
    mask = None if all_ones_mask else outputs["padding_mask"]
    logits, sigma, disp, depth, layers = ops.decoder_tail(dispconv_out, sigmaconv_out, mask, outputs["disp_layered"],
                                                          use_mixture_loss=use_mixture_loss,
                                                          fuse_sweep_backward=fuse_sweep_backward)
    outputs["logits"] = logits
    if use_mixture_loss:
        outputs["sigma"] = sigma
    shape = dispconv_out.shape
    if materialize_layers:
        pi, prob = layers(want_pi=use_mixture_loss, want_probability=True)
        outputs["probability"] = prob
        if use_mixture_loss:
            outputs["pi"] = pi
    else:
        dev, dt = dispconv_out.device, torch.float32    # (pi / probability are fp32 with bf16 conv outputs too)
        outputs["probability"] = LazyLayers(shape, lambda: layers(False, True)[1], dev, dt)
        if use_mixture_loss:
            outputs["pi"] = LazyLayers(shape, lambda: layers(True, False)[0], dev, dt)
    outputs["disp"] = disp
    outputs["depth"] = depth
    return outputs


def fused_plane_geometry(outputs, input_grids, residual_levels, *, no_levels, xz_levels, disp_min, disp_max, xz_min, xz_max,
                         check_contract=None):
    """Opt-in drop-in for depth_decoder.py:148-257 with ``yz_levels == 0``: fills ``outputs["distance"]`` [B,N], ``["norm"]``
    [B,N,3], ``["disp_layered"]`` and ``["padding_mask"]`` [B,N,H,W] from ``input_grids`` [B,2,H,W] and ``residual_levels``
    (``sigmoid(residualconv(x)) - 0.5``, [B,N,1,1] or [B,N]; ``None`` without ``--plane_residual``) through
    ``ops.plane_geometry`` — one HIP kernel each way.  The two maps are row views (``stride(3) == 0`` over [B,N,H] rows): nothing
    [B,N,H,W]-sized is built, and ``fused_decoder_tail`` / the trainer path take their row forms on seeing the strides.

    Opt-in because ``networks/*`` drop in unchanged.  With ``yz_levels > 0`` the maintainer keeps the reference's lines (yz
    planes vary along x; they have no row form).  The operator assumes what every grid of datasets/pair_transforms.py gives: a
    y channel that is constant along x, the x extent of a row at its first and last column.  ``check_contract=True``, or
    ``PD_CHECK_CONTRACT=1`` in the environment (the trainer path's ``opt.pd_check_contract`` convention), checks the y channel on
    the data and raises ``ValueError``; a sheared or rotated grid must keep the reference's lines as well."""
    disp_layered, padding_mask, distance, norm = ops.plane_geometry(
        input_grids, residual_levels, no_levels=no_levels, xz_levels=xz_levels, disp_min=disp_min, disp_max=disp_max,
        xz_min=xz_min, xz_max=xz_max, check_contract=check_contract)
    outputs["distance"] = distance
    outputs["norm"] = norm
    outputs["disp_layered"] = disp_layered
    outputs["padding_mask"] = padding_mask
    return outputs


def fused_plade_tail(outputs, conv0_out, conv_sigma_out=None, *, use_mixture_loss=True, materialize_layers=False):
    """Fills ``outputs`` with "logits", "dists", "sigma", "pi", "probability", "disp", "depth" as plade_net.py:309-340 does
    with ``render_probability`` (alpha compositing of the N-1 logit channels of ``conv0`` against the distances between the
    depth layers).  Reads ``outputs["disp_layered"]`` (per-plane levels with the learnt residual, or the dense map with
    ground planes).  A row view from ``fused_plane_geometry`` is accepted and materialised to the dense map (``_contig``): correct,
    no faster — this tail has no row form."""
    B, Nm1, H, W = conv0_out.shape
    logits, dists, sigma, disp, depth, layers = ops.plade_tail(conv0_out, conv_sigma_out, outputs["disp_layered"],
                                                                use_mixture_loss=use_mixture_loss)
    outputs["logits"] = logits
    outputs["dists"] = dists
    if use_mixture_loss:
        outputs["sigma"] = sigma
    shape = (B, Nm1 + 1, H, W)
    if materialize_layers:
        pi, prob = layers(want_pi=use_mixture_loss, want_probability=True)
        outputs["probability"] = prob
        if use_mixture_loss:
            outputs["pi"] = pi
    else:
        dev, dt = conv0_out.device, torch.float32
        outputs["probability"] = LazyLayers(shape, lambda: layers(False, True)[1], dev, dt)
        if use_mixture_loss:
            outputs["pi"] = LazyLayers(shape, lambda: layers(True, False)[0], dev, dt)
    outputs["disp"] = disp
    outputs["depth"] = depth
    return outputs


def _fill_inference(outputs, res, shape, device):
    outputs["disp"] = res.disp
    outputs["depth"] = res.depth
    outputs["confidence"] = res.confidence
    outputs["plane_index"] = res.plane_index
    outputs["disp_best"] = res.disp_best
    outputs["probability"] = LazyLayers(shape, lambda: res.layers(False, True)[1], device, torch.float32)
    return outputs


_INFERENCE_WANT = ("depth", "confidence", "plane_index", "disp_best", "layers")


def fused_decoder_tail_inference(outputs, dispconv_out, sigmaconv_out=None, *, use_mixture_loss=True, all_ones_mask=False,
                                 keep_conv_outputs=False):
    """``fused_decoder_tail`` for a network that only predicts (``planedepth_amd.predict``, the reference's
    evaluate_depth_HR.py): fills ``outputs["disp"]``, ``["depth"]``, ``["confidence"]`` (``max_n probability_n``, fp32 [B,1,H,W]:
    what evaluate_depth_HR.py:168 reduces ``probability`` to), ``["plane_index"]`` (int32, the plane that attains it;
    depth_decoder.py:286), ``["disp_best"]`` (``disp_layered`` at that plane) and ``["probability"]`` — a ``LazyLayers``, so
    ``output["probability"].amax(1)`` keeps working unchanged and the [B,N,H,W] tensor exists only if something touches it.
    One forward-only kernel (``ops.decoder_tail_inference``); ``disp`` / ``depth`` have ``fused_decoder_tail``'s bits.

    NOT set: ``outputs["logits"]``, ``["sigma"]`` and ``["pi"]`` — writing those [B,N,H,W] tensors is what this call saves.  A
    caller that wants them (the plane sweep, the losses, the self-distillation post-process) uses ``fused_decoder_tail``, under
    ``torch.no_grad()`` where no gradient is needed.  Call it under ``torch.no_grad()``: conv outputs that require grad raise
    ``ValueError`` otherwise.

    ``keep_conv_outputs=True`` also sets ``outputs["raw_logits"]`` / ``["raw_sigma"]`` (the latter with the mixture) to the conv
    outputs themselves — by reference, no copy — which is what ``planedepth_amd.predict.render`` renders novel views from
    (``ops.render_views``).  The default sets neither key."""
    mask = None if all_ones_mask else outputs["padding_mask"]
    res = ops.decoder_tail_inference(dispconv_out, sigmaconv_out, mask, outputs["disp_layered"],
                                     use_mixture_loss=use_mixture_loss, want=_INFERENCE_WANT)
    if keep_conv_outputs:
        outputs["raw_logits"] = dispconv_out
        if use_mixture_loss:
            outputs["raw_sigma"] = sigmaconv_out
    return _fill_inference(outputs, res, dispconv_out.shape, dispconv_out.device)


def fused_plade_tail_inference(outputs, conv0_out, conv_sigma_out=None, *, use_mixture_loss=True):
    """``fused_plade_tail`` for a network that only predicts: the keys of ``fused_decoder_tail_inference`` from one forward-only
    kernel (``ops.plade_tail_inference``), with ``fused_plade_tail``'s bits in ``disp`` / ``depth``.

    NOT set: ``outputs["logits"]``, ``["dists"]``, ``["sigma"]`` and ``["pi"]``; a caller that wants them uses ``fused_plade_tail``
    (under ``torch.no_grad()`` where no gradient is needed)."""
    B, Nm1, H, W = conv0_out.shape
    res = ops.plade_tail_inference(conv0_out, conv_sigma_out, outputs["disp_layered"], use_mixture_loss=use_mixture_loss,
                                   want=_INFERENCE_WANT)
    return _fill_inference(outputs, res, (B, Nm1 + 1, H, W), conv0_out.device)
