"""The fused plane sweep + photometric loss (reference trainer.py:523-603, 717-742): autograd nodes over pd_plane_sweep_*,
routing between the kernel families, the homography algebra, the per-plane layer tensors on demand.

Every function launches hand-written HIP kernels through ctypes on torch's current stream; there is no eager / CPU
implementation behind these operators.
"""
import ctypes
import functools
from typing import NamedTuple

from . import _capi as C
from . import _state as S
from . import planeform as PF
from ._buffers import torch, _timed, _desc, _contig, _zero_scalar, _plane_grad_buffer


# ---------------------------------------------------------------------------------------------------------------------
# Fused plane sweep + photometric loss
# ---------------------------------------------------------------------------------------------------------------------
class SweepCall(NamedTuple):
    """One target view's sweep: what ``plane_sweep_disp(..., defer=True)`` / ``plane_sweep_homography(..., defer=True)`` return,
    what ``_PlaneSweep.apply(*call)`` takes.  ``link``: the fused decoder tail whose backward this sweep's backward applies
    (single-view nodes only)."""
    src: object
    tgt: object
    logits: object
    sigma: object
    plane: object
    plane_aux: object
    inv_K3: object
    padding_mask: object
    dists: object
    mode: int
    flags: int
    sign: float
    link: object = None


# What a view's forward keeps for its backward (contiguous tensors or None).
SweepSaved = NamedTuple("SweepSaved", [(k, object) for k in ("src", "tgt", "logits", "sigma", "plane", "plane_aux", "inv_K3",
                                                              "padding_mask", "dists", "rgb_rec", "stash")])


_GRAD_FIELDS = ("logits", "sigma", "plane", "dists")   # the inputs of ``_PlaneSweep.apply(*call)`` that can take a gradient
_GRAD_AT = tuple(SweepCall._fields.index(k) for k in _GRAD_FIELDS)


def _call_grads(*grads):
    """backward()'s return value of ``_PlaneSweep``: ``grads`` (in _GRAD_FIELDS' order) at their inputs' places, None elsewhere."""
    out = [None] * len(SweepCall._fields)
    for i, g in zip(_GRAD_AT, grads):
        out[i] = g
    return tuple(out)


def _scalar_grad(g_ph_mean):
    """The upstream gradient of ph_mean as the kernels read it: a contiguous fp32 [1] (or None)."""
    return None if g_ph_mean is None else g_ph_mean.reshape(1).to(torch.float32).contiguous()


def _workspace(lib, d, device):
    """Scratch of one backward call: partial sums of the plane-parameter gradient, the row-shift kernels' boundary spill,
    the gather kernels' per-pixel gradients."""
    return torch.empty(max(int(lib.pd_sweep_bwd_workspace_floats(ctypes.byref(d))), 1), device=device, dtype=torch.float32)


def _forward_view(lib, call, first=None):
    """What every forward does per view: argument checks, contiguous tensors, the descriptor, outputs and stash.  ``first``:
    what this function returned for another view of the same src / logits / sigma and configuration (the pair forward) —
    the shared tensors, the descriptor and the stash depth are taken from there instead of being checked and asked again.
    Returns (descriptor, stash depth, SweepSaved, ph_map, ph_mean)."""
    src, logits, sigma = call.src, call.logits, call.sigma
    tgt, plane, plane_aux, inv_K3, padding_mask, dists = call.tgt, call.plane, call.plane_aux, call.inv_K3, call.padding_mask, call.dists
    mode, flags, sign = call.mode, call.flags, call.sign
    S.LAST_SWEEP_FLAGS = flags
    B, N, H, W = logits.shape
    if first is None:
        edt = torch.bfloat16 if flags & C.PD_LOGITS_BF16 else torch.float32   # storage of logits / sigma and their gradients
        C.require_gpu_tensor("logits", logits, dtype=edt)
        C.require_gpu_tensor("src", src, (B, 3, H, W))
        if flags & C.PD_MIXTURE:
            C.require_gpu_tensor("sigma", sigma, (B, N, H, W), dtype=edt)
        src, logits, sigma = _contig(src), _contig(logits), _contig(sigma)
        d = _desc(B, N, H, W, mode, flags, sign)
        k = lib.pd_sweep_stash_floats(ctypes.byref(d)) // (H * W)
        d.flags |= C.PD_PH_MEAN_ZEROED   # ph_mean is a pre-zeroed slot: the entry point then launches no memset
    else:
        d, k, shared, _, _ = first
        src, logits, sigma = shared.src, shared.logits, shared.sigma
    C.require_gpu_tensor("tgt", tgt, (B, 3, H, W))
    if mode == C.PD_WARP_DISP:
        C.require_gpu_tensor("disp", plane, (B, N, H, W) if flags & C.PD_DISP_DENSE else
                             ((B, N, H) if flags & C.PD_DISP_ROWS else (B, N)))
        if padding_mask is not None:
            C.require_gpu_tensor("padding_mask", padding_mask, (B, N, H) if flags & C.PD_MASK_ROWS else (B, N, H, W))
    else:
        C.require_gpu_tensor("H_t2s", plane, (B, 4, 3, 3) if flags & C.PD_HOMO_UNIFORM else (B * N, 3, 3))
        if flags & C.PD_HOMO_UNIFORM and padding_mask is not None:
            C.require_gpu_tensor("translation weights", padding_mask, (B, N, 3))
        C.require_gpu_tensor("Rn", plane_aux, (B * N, 3))
        C.require_gpu_tensor("inv_K3", inv_K3, (B, 3, 3))
    if flags & C.PD_RENDER_PROB:
        C.require_gpu_tensor("dists", dists, (B, N - 1, H, W))
    else:
        dists = None
    dev = logits.device
    rgb_rec = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
    ph_map = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
    ph_mean = _zero_scalar(dev)
    stash = torch.empty(B, k, H, W, device=dev, dtype=torch.float32)
    if S.DEBUG_STASH is not None:
        S.DEBUG_STASH.append(stash)
    saved = SweepSaved(src, _contig(tgt), logits, sigma, _contig(plane), _contig(plane_aux), _contig(inv_K3),
                       _contig(padding_mask), _contig(dists), rgb_rec, stash)
    return d, k, saved, ph_map, ph_mean


def _sweep_forward(*call):
    """One target view (the fields of a SweepCall, with or without its link) through pd_plane_sweep_fwd ->
    ((rgb_rec, ph_map, ph_mean[1]), SweepSaved)."""
    lib = C.load()
    d, _, s, ph_map, ph_mean = _forward_view(lib, SweepCall(*call))
    dev = s.logits.device
    with _timed("fwd", dev):
        C.call("pd_plane_sweep_fwd", dev, ctypes.byref(d), s.src, s.tgt, s.logits, s.sigma, s.plane, s.plane_aux, s.inv_K3,
               s.padding_mask, s.dists, s.rgb_rec, ph_map, ph_mean, s.stash)
    return (s.rgb_rec, ph_map, ph_mean), s


def _sweep_forward_pair(call_a, call_b):
    """pd_uniform_fwd_pair: two plane-uniform target views (SweepCalls of equal mode / flags / sign over the same src / logits /
    sigma) in one launch.  Returns what two ``_sweep_forward`` calls return."""
    lib = C.load()
    view_a = _forward_view(lib, call_a)
    d, _, sa, ph_map_a, ph_mean_a = view_a
    _, _, sb, ph_map_b, ph_mean_b = _forward_view(lib, call_b, first=view_a)
    views = [C.sweep_view(tgt=s.tgt, plane=s.plane, plane_aux=s.plane_aux, inv_K3=s.inv_K3, dists=s.dists, rgb_rec=s.rgb_rec,
                          ph_map=ph_map, ph_mean=ph_mean, stash=s.stash)
             for s, ph_map, ph_mean in ((sa, ph_map_a, ph_mean_a), (sb, ph_map_b, ph_mean_b))]
    dev = sa.logits.device
    with _timed("fwd", dev):
        C.call("pd_uniform_fwd_pair", dev, ctypes.byref(d), sa.src, sa.logits, sa.sigma, ctypes.byref(views[0]),
               ctypes.byref(views[1]))
    return ((sa.rgb_rec, ph_map_a, ph_mean_a), sa), ((sb.rgb_rec, ph_map_b, ph_mean_b), sb)


def _sweep_backward_pair(view_a, view_b, cfg, need_a, need_b, g_logits, g_sigma, accumulate):
    """pd_uniform_bwd_pair: the backward of two plane-uniform views (``view_*`` = (SweepSaved, upstream gradients)) of the
    same logits / sigma — both first passes in one launch, then the pair gather into (``accumulate``: added to)
    g_logits / g_sigma (None: only the views' own gradients).  Returns ((g_plane_a, g_dists_a), (g_plane_b, g_dists_b))."""
    lib = C.load()
    mode, flags, sign = cfg
    first = view_a[0]
    B, N, H, W = first.logits.shape
    dev = first.logits.device
    mix = bool(flags & C.PD_MIXTURE)
    d = _desc(B, N, H, W, mode, flags | C.PD_BWD_DEFER_GATHER | (C.PD_BWD_ACCUMULATE if accumulate else 0), sign)
    ws_floats = max(int(lib.pd_sweep_bwd_workspace_floats(ctypes.byref(d))), 1)   # (asked once: both views are d's)
    views, outs, keep = [], [], []
    for (s, grads), need in ((view_a, need_a), (view_b, need_b)):
        g_rgb_rec, g_ph_map, g_ph_mean = grads
        g_rgb_rec, g_ph_map, g_ph_mean = _contig(g_rgb_rec), _contig(g_ph_map), _scalar_grad(g_ph_mean)
        _, _, need_plane, need_dists = need
        g_plane = torch.empty_like(s.plane) if need_plane else None
        g_dists = torch.empty_like(s.dists) if (s.dists is not None and need_dists) else None
        ws = torch.empty(ws_floats, device=dev, dtype=torch.float32)
        views.append(C.sweep_view(tgt=s.tgt, plane=s.plane, plane_aux=s.plane_aux, inv_K3=s.inv_K3, padding_mask=s.padding_mask,
                                  dists=s.dists, rgb_rec=s.rgb_rec, stash=s.stash, g_rgb_rec=g_rgb_rec, g_ph_map=g_ph_map,
                                  g_ph_mean=g_ph_mean, g_plane=g_plane, g_dists=g_dists, workspace=ws))
        outs.append((g_plane, g_dists))
        keep.append((g_rgb_rec, g_ph_map, g_ph_mean, ws))   # alive until the call is enqueued
        if S.DEBUG_WORKSPACE is not None:
            S.DEBUG_WORKSPACE.append((d, ws))
    with _timed("bwd", dev):
        C.call("pd_uniform_bwd_pair", dev, ctypes.byref(d), first.src, first.logits, first.sigma, ctypes.byref(views[0]),
               ctypes.byref(views[1]), g_logits, g_sigma if mix else None)
    del keep
    return outs


def _sweep_backward(saved, cfg, grads, need, into=None, accumulate=False):
    """pd_plane_sweep_bwd of one target view.  ``need`` = (logits, sigma, plane, dists) gradients wanted; ``into`` =
    (g_logits, g_sigma) buffers to write (or, ``accumulate``: add) into instead of fresh ones.
    Returns (g_logits, g_sigma, g_plane, g_dists)."""
    lib = C.load()
    s = SweepSaved(*saved)
    mode, flags, sign = cfg
    g_rgb_rec, g_ph_map, g_ph_mean = grads
    B, N, H, W = s.logits.shape
    dev = s.logits.device
    need_logits, need_sigma, need_plane, need_dists = need
    g_plane, plane_flag = _plane_grad_buffer(s.plane, B, N, H, W, mode, flags, sign) if need_plane else (None, 0)
    d = _desc(B, N, H, W, mode, flags | plane_flag | (C.PD_BWD_ACCUMULATE if accumulate else 0), sign)
    mix = bool(flags & C.PD_MIXTURE)
    if into is not None:
        g_logits, g_sigma = into
        edt = torch.bfloat16 if flags & C.PD_LOGITS_BF16 else torch.float32   # the buffers hold what the flag says
        if g_logits is not None:
            C.require_gpu_tensor("g_logits", g_logits, dtype=edt)
        if g_sigma is not None:
            C.require_gpu_tensor("g_sigma", g_sigma, dtype=edt)
    else:
        g_logits = torch.empty_like(s.logits) if need_logits else None
        g_sigma = torch.empty_like(s.sigma) if (need_sigma and mix) else None
    g_dists = torch.empty_like(s.dists) if (s.dists is not None and need_dists) else None
    ws = _workspace(lib, d, dev)
    g_rgb_rec, g_ph_map, g_ph_mean = _contig(g_rgb_rec), _contig(g_ph_map), _scalar_grad(g_ph_mean)
    with _timed("bwd", dev):
        C.call("pd_plane_sweep_bwd", dev, ctypes.byref(d), s.src, s.tgt, s.logits, s.sigma, s.plane, s.plane_aux, s.inv_K3,
               s.padding_mask, s.dists, s.rgb_rec, s.stash, g_rgb_rec, g_ph_map, g_ph_mean, g_logits,
               g_sigma if mix else None, g_plane, g_dists, ws)
    if S.DEBUG_WORKSPACE is not None:
        S.DEBUG_WORKSPACE.append((d, ws))
    return g_logits, (g_sigma if mix else None), g_plane, g_dists


def _sweep_backward_tail(saved, cfg, grads, need, link):
    """pd_plane_sweep_bwd_tail — or, with per-row disparities and / or a row mask, pd_plane_sweep_bwd_tail_rows: the sweep's
    backward with the linked decoder tail's backward riding along.  Returns (g_raw_logits, g_raw_sigma, g_plane) — handed to
    autograd as the gradients of logits / sigma; the tail's node passes them through (TailLink).  ``g_plane`` has the shape of
    the disparities ([B,N] or [B,N,H]) and holds the warp's and the tail's share."""
    lib = C.load()
    s = SweepSaved(*saved)
    mode, flags, sign = cfg
    g_rgb_rec, g_ph_map, g_ph_mean = grads
    B, N, H, W = s.logits.shape
    dev = s.logits.device
    _, _, need_plane, _ = need
    g_plane, plane_flag = _plane_grad_buffer(s.plane, B, N, H, W, mode, flags, sign) if need_plane else (None, 0)
    d = _desc(B, N, H, W, mode, flags | plane_flag, sign)
    link.enter_pass()
    g_disp, g_depth = link.seen.pop("disp", None), link.seen.pop("depth", None)   # (what the taps of THIS backward pass left)
    gl, gs = torch.empty_like(s.logits), torch.empty_like(s.sigma)
    ws = _workspace(lib, d, dev)
    g_rgb_rec, g_ph_map, gd, gz = map(_contig, (g_rgb_rec, g_ph_map, g_disp, g_depth))
    g_ph_mean = _scalar_grad(g_ph_mean)
    tail_args = (s.rgb_rec, s.stash, g_rgb_rec, g_ph_map, g_ph_mean, link.raw_sigma, link.stash, link.disp, gd, gz, gl, gs,
                 g_plane, ws)
    head = (ctypes.byref(d), s.src, s.tgt, s.logits, s.sigma, s.plane)
    with _timed("bwd", dev):
        if flags & (C.PD_DISP_ROWS | C.PD_MASK_ROWS):   # (plane_sweep_disp checked: the sweep's row mask IS the tail's)
            C.call("pd_plane_sweep_bwd_tail_rows", dev, *head, s.padding_mask, *tail_args)
        else:
            C.call("pd_plane_sweep_bwd_tail", dev, *head, *tail_args)
    link.applied = {"disp": g_disp, "depth": g_depth}   # until the tail's node of this pass has consumed it
    link.fused_passes += 1
    return gl, gs, g_plane


class TailLink:
    """What ties a fused decoder tail (``decoder_tail(..., fuse_sweep_backward=True)``) to the ONE plane sweep that consumes
    its logits / sigma, so that the sweep's backward kernel can apply the tail's backward as well
    (``pd_plane_sweep_bwd_tail``, ``pd_plane_sweep_bwd_tail_rows`` for row-form disparities / mask: the [B,N,H,W]-sized
    g_logits / g_sigma are never re-read by a tail kernel).

    Autograd runs the sweep's node before the tail's, and the tail's other upstream gradients (d loss / d disp from the
    smoothness term, d / d depth) reach the tail's node only — so ``pred_novel_images`` routes ``outputs["disp"]`` /
    ``["depth"]`` through gradient taps created AFTER the sweep's node: nodes created later run earlier, the taps have
    handed their gradients over by the time the sweep's backward runs.  The tail's own backward then passes g_logits /
    g_sigma through, and runs its kernel only on whatever upstream gradient of disp / depth the sweep did NOT see (none in
    the trainer's graph; a consumer that took ``disp`` before the tap existed, for example) — correct in any order.

    The fused kernel takes the tail's disparities and mask from the SWEEP's arguments, and the sweep's plane gradient carries the
    tail's share.  For the row form ``plane_sweep_disp`` therefore fuses only when its [B,N,H] rows are the tail's memory
    (``disp_rows`` / ``mask_rows``: the rows tensor behind ``plane_geometry``'s or ``row_view``'s views; a ``row_uniform`` dense
    copy, an untagged stride-0 view or rows on one side only count as a consumer the fused form does not serve).  Per-plane
    scalars are not compared — ``_per_plane_view`` may hand the two nodes different views of the decoder's [B,N,1,1] tensor: there
    the flag's promise includes that the sweep is given the ``disp_layered`` the tail was given, as ``pred_novel_images`` does.

    Per-pass state.  ``seen`` and ``applied`` belong to ONE backward pass — the autograd engine's graph task, ``pass_id`` — and a
    pass need not run all three of tap, sweep and tail (``torch.autograd.grad`` over a part of a retained graph).  Every backward
    that touches the link calls ``enter_pass`` first: state of another pass is dropped, and a callback at the end of the pass
    (the engine's ``queue_callback``) clears what this one leaves, so nothing a pass wrote is ever read by a later one.

    The refused pass.  ``torch.autograd.grad(loss, [logits, sigma])`` makes the engine run the sweep's backward and only CAPTURE
    at the tail's node: the caller would receive the conv outputs' gradients (sigmoid', the clamp gate, the mask and the disparity
    share applied) as d loss / d logits, d loss / d sigma.  The sweep cannot tell such a pass from one that runs the tail's node,
    and the fused kernel has no output-space gradients to return, so the choice made here is to REFUSE: the end-of-pass callback
    finds ``applied`` never consumed and raises ``PlaneDepthHipError`` naming ``fuse_sweep_backward``; the link is clean afterwards and
    the graph stays usable.  Build the graph with ``fuse_sweep_backward=False`` for such a pass."""

    def __init__(self, raw_sigma, stash, disp, mask_rows=None):
        self.raw_sigma, self.stash, self.disp = raw_sigma, stash, disp
        self.mask_rows = mask_rows   # the tail's [B,N,H] padding mask (PD_TAIL_MASK_ROWS) or None: the sweep must have been given the same
        self.disp_rows = None        # the tail's [B,N,H] disparities (PD_TAIL_DISP_ROWS) or None: likewise
        self.consumers = 0        # sweeps that registered as consumers of this tail's logits / sigma
        self.pass_id = None       # the backward pass (torch._C._current_graph_task_id()) that ``seen`` / ``applied`` belong to
        self.seen = {}            # "disp" / "depth" -> gradient handed over by its tap (taken by the sweep's backward of the pass)
        self.applied = None       # {"disp": g or None, "depth": g or None}: a sweep's backward has applied the tail's terms in THIS
                                  # backward pass; the tail's node consumes it and resets it
        self.fused_passes = 0     # backward passes in which the sweep's kernel applied the tail's backward (diagnostics / tests)

    def enter_pass(self):
        """First thing in every backward that reads or writes ``seen`` / ``applied`` (tap, sweep, tail)."""
        pass_id = torch._C._current_graph_task_id()   # (-1 outside the engine: no end of a pass to book)
        if pass_id != self.pass_id:
            self.pass_id, self.applied = pass_id, None
            self.seen.clear()
            if pass_id >= 0:
                torch.autograd.Variable._execution_engine.queue_callback(lambda: self._end_pass(pass_id))

    def _end_pass(self, pass_id):
        if pass_id != self.pass_id:
            return
        applied, self.applied, self.pass_id = self.applied, None, None
        self.seen.clear()
        if applied is not None:   # the sweep applied the tail's backward and the tail's node never ran: see "The refused pass"
            raise C.PlaneDepthHipError(
                "fuse_sweep_backward: this backward pass ran the plane sweep's fused backward but not the decoder tail's node "
                "(torch.autograd.grad with logits / sigma as inputs?), so the gradients it holds at logits / sigma are those of the "
                "decoder's conv outputs, not d / d logits and d / d sigma.  Build the graph with fuse_sweep_backward=False for such "
                "a pass.")


class _GradTap(torch.autograd.Function):
    """Identity whose backward leaves the gradient with the TailLink on its way through."""

    @staticmethod
    def forward(ctx, x, link, which):
        ctx.link, ctx.which = link, which
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.link.enter_pass()
        ctx.link.seen[ctx.which] = g
        return g, None, None


def tail_taps(outputs):
    """Called by ``pred_novel_images`` right after the sweep's node exists: ``outputs["disp"]`` / ``["depth"]`` of a linked
    fused decoder tail go through gradient taps (see TailLink).  No-op without a link or with more than one consumer."""
    link = getattr(outputs.get("logits"), "_pd_tail_link", None)
    if link is None or link.consumers != 1:
        return
    for k in ("disp", "depth"):
        t = outputs.get(k)
        if torch.is_tensor(t) and t.requires_grad:
            outputs[k] = _GradTap.apply(t, link, k)


class _PlaneSweep(torch.autograd.Function):
    """apply(*SweepCall) -> (rgb_rec [B,3,H,W], ph_map [B,1,H,W], ph_mean []).

    ``ph_mean`` is ``ph_map.mean()`` accumulated inside the sweep kernel (the `.mean()` of trainer.py:742 without a
    reduction kernel of its own); its upstream gradient is a device scalar that the backward kernel applies per pixel.

    Gradients: logits, sigma, plane (disp_layered or H_t2s), dists.  src / tgt are images (no gradient, as in the reference
    where they are dataset tensors).
    """

    @staticmethod
    def forward(ctx, src, tgt, logits, sigma, plane, plane_aux, inv_K3, padding_mask, dists, mode, flags, sign, link=None):
        (rgb_rec, ph_map, ph_mean), saved = _sweep_forward(src, tgt, logits, sigma, plane, plane_aux, inv_K3,
                                                           padding_mask, dists, mode, flags, sign)
        ctx.save_for_backward(*saved)
        ctx.cfg = (mode, flags, sign)
        ctx.link = link
        ctx.set_materialize_grads(False)  # unused outputs arrive as None in backward, not as zero tensors
        return rgb_rec, ph_map, ph_mean.reshape(())

    @staticmethod
    def backward(ctx, g_rgb_rec, g_ph_map, g_ph_mean):
        need = tuple(ctx.needs_input_grad[i] for i in _GRAD_AT)
        need_logits, need_sigma, _, _ = need
        link = ctx.link
        if link is not None and link.consumers == 1 and need_logits and need_sigma:
            g_logits, g_sigma, g_plane = _sweep_backward_tail(ctx.saved_tensors, ctx.cfg, (g_rgb_rec, g_ph_map, g_ph_mean),
                                                              need, link)
            return _call_grads(g_logits, g_sigma, g_plane, None)
        g_logits, g_sigma, g_plane, g_dists = _sweep_backward(ctx.saved_tensors, ctx.cfg,
                                                              (g_rgb_rec, g_ph_map, g_ph_mean), need)
        return _call_grads(g_logits, g_sigma, g_plane, g_dists)


_SHARED = ("src", "logits", "sigma")   # what every view of a _MultiPlaneSweep node sweeps, in apply()'s order
_SIDE_FIELDS = tuple(k for k in SweepCall._fields if k not in _SHARED + ("link",))   # what each view brings along
_PER_SIDE = len(_SIDE_FIELDS)
_SIDE_PLANE, _SIDE_DISTS = _SIDE_FIELDS.index("plane"), _SIDE_FIELDS.index("dists")


def _plane_uniform(mode, flags):
    return mode == C.PD_WARP_HOMOGRAPHY and bool(flags & C.PD_HOMO_UNIFORM)


class _MultiPlaneSweep(torch.autograd.Function):
    """Every target view of one step (trainer.py:532: ``for target_side in self.target_sides``) over the SAME source
    image, logits and sigma as ONE autograd node: the views' gradients into logits / sigma are summed inside the backward
    kernels (PD_BWD_ACCUMULATE) instead of by [B,N,H,W]-sized add kernels between separate nodes (at 8x49x192x640 each
    such add moves 0.58 GB; three views need four of them).

    apply(src, logits, sigma, *flat) with ``flat`` = per view its ``_SIDE_FIELDS`` (tgt, plane, plane_aux, inv_K3,
    padding_mask, dists, mode, flags, sign) -> per view (rgb_rec, ph_map, ph_mean)."""

    @staticmethod
    def forward(ctx, src, logits, sigma, *flat):
        n = len(flat) // _PER_SIDE
        calls = []
        for i in range(n):
            tgt, plane, plane_aux, inv_K3, padding_mask, dists, mode, flags, sign = flat[i * _PER_SIDE:(i + 1) * _PER_SIDE]   # _SIDE_FIELDS
            calls.append(SweepCall(src, tgt, logits, sigma if flags & C.PD_MIXTURE else None, plane, plane_aux, inv_K3,
                                   padding_mask, dists, mode, flags, sign))
        cfgs = [(c.mode, c.flags, c.sign) for c in calls]
        done = {}   # plane-uniform views of equal configuration go through the forward two at a time (pd_uniform_fwd_pair)
        if S.PAIR_VIEWS:
            uni = [i for i in range(n) if _plane_uniform(calls[i].mode, calls[i].flags)]
            while len(uni) >= 2:
                i = uni.pop(0)
                j = next((q for q in uni if cfgs[q] == cfgs[i]), None)
                if j is None:
                    continue
                uni.remove(j)
                done[i], done[j] = _sweep_forward_pair(calls[i], calls[j])
        outs, tensors, layout = [], [], []
        for i in range(n):
            (rgb_rec, ph_map, ph_mean), saved = done[i] if i in done else _sweep_forward(*calls[i])
            outs += [rgb_rec, ph_map, ph_mean.reshape(())]
            idx = []
            for t in saved:     # save_for_backward takes tensors only: remember where the Nones were
                if t is None:
                    idx.append(-1)
                else:
                    idx.append(len(tensors))
                    tensors.append(t)
            layout.append(idx)
        ctx.save_for_backward(*tensors)
        ctx.cfgs, ctx.layout, ctx.n = cfgs, layout, n
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        lib = C.load()
        tensors = ctx.saved_tensors
        n = ctx.n
        need_logits, need_sigma = (ctx.needs_input_grad[_SHARED.index(k)] for k in ("logits", "sigma"))
        views = []
        for i in range(n):
            g = grads[3 * i:3 * i + 3]
            if all(x is None for x in g):
                continue   # this view took no part in the loss
            saved = SweepSaved(*(None if j < 0 else tensors[j] for j in ctx.layout[i]))
            B, N, H, W = saved.logits.shape
            can = bool(lib.pd_sweep_bwd_accumulates(ctypes.byref(_desc(B, N, H, W, *ctx.cfgs[i]))))
            base = len(_SHARED) + i * _PER_SIDE
            need = (need_logits, need_sigma, ctx.needs_input_grad[base + _SIDE_PLANE], ctx.needs_input_grad[base + _SIDE_DISTS])
            views.append((i, saved, g, can, need))
        views.sort(key=lambda v: v[3])   # kernels that cannot add in place (the row-shift ones) first: one of them starts the sum
        g_logits = g_sigma = None
        per_view = {}

        def pairable(i):   # plane-uniform views with the same kernel configuration go through the backward together
            mode, flags, _ = ctx.cfgs[i]
            return S.PAIR_VIEWS and _plane_uniform(mode, flags) and (need_logits or need_sigma)
        k = 0
        while k < len(views):
            i, saved, g, can, need = views[k]
            nxt = views[k + 1] if k + 1 < len(views) else None
            if nxt is not None and pairable(i) and pairable(nxt[0]) and ctx.cfgs[i] == ctx.cfgs[nxt[0]]:
                # both first passes in one launch, the pair gather, the reductions: one call (pd_uniform_bwd_pair)
                j, saved_j, g_j, _, need_j = nxt
                started = g_logits is not None or g_sigma is not None
                _, flags, _ = ctx.cfgs[i]
                if g_logits is None:
                    g_logits = torch.zeros_like(saved.logits) if started else torch.empty_like(saved.logits)
                if flags & C.PD_MIXTURE and g_sigma is None:
                    g_sigma = torch.zeros_like(saved.logits) if started else torch.empty_like(saved.logits)
                per_view[i], per_view[j] = _sweep_backward_pair((saved, g), (saved_j, g_j), ctx.cfgs[i], need, need_j,
                                                                g_logits, g_sigma, accumulate=started)
                k += 2
                continue
            if g_logits is None and g_sigma is None:
                g_logits, g_sigma, gp, gd = _sweep_backward(saved, ctx.cfgs[i], g, need)
            elif can:
                gl, gs, gp, gd = _sweep_backward(saved, ctx.cfgs[i], g, need, into=(g_logits, g_sigma), accumulate=True)
                g_sigma = g_sigma if g_sigma is not None else gs
            else:
                gl, gs, gp, gd = _sweep_backward(saved, ctx.cfgs[i], g, need)
                if gl is not None:
                    g_logits = gl if g_logits is None else g_logits.add_(gl)
                if gs is not None:
                    g_sigma = gs if g_sigma is None else g_sigma.add_(gs)
            per_view[i] = (gp, gd)
            k += 1
        out = [None, g_logits, g_sigma]
        for i in range(n):
            side = [None] * _PER_SIDE
            side[_SIDE_PLANE], side[_SIDE_DISTS] = per_view.get(i, (None, None))
            out += side
        return tuple(out)


def as_f32(t):
    """``t`` as fp32 for the fp32 route (``t`` itself when it is fp32 already or None).  The copy is cached on ``t`` (per
    version and grad mode): every view of one step that falls back sweeps the SAME fp32 tensor, so plane_sweep_multi
    accepts them and their gradients add in fp32 before the cast's backward rounds the sum to ``t``'s dtype once.

    Memory: the copy (twice the size of a bf16 ``t``) lives as long as ``t`` does.  For a LEAF ``t`` that requires grad the
    copy's graph refers back to ``t``, a cycle through autograd's C++ nodes that Python's collector cannot break: ``del
    t._pd_f32`` when such a tensor is done with (the trainer's tensors are decoder outputs, not leaves)."""
    if t is None or t.dtype == torch.float32:
        return t
    key = (t._version, torch.is_grad_enabled())
    c = getattr(t, "_pd_f32", None)
    if c is not None and c[0] == key:
        return c[1]
    f = t.float()
    t._pd_f32 = (key, f)
    return f


def _storage_route(logits, sigma, mix, desc):
    """Where the SweepCall is built: (logits, sigma, extra flags).  fp32 inputs pass as they are; bf16 logits (and bf16
    sigma with the mixture) go to the kernels as bf16 with PD_LOGITS_BF16 where pd_sweep_native_bf16(desc) says the
    descriptor is served (desc None: never); everything else — mixed dtypes, fp16, a descriptor outside the native set —
    runs the fp32 route on as_f32 copies (their backward rounds each fp32 gradient once)."""
    sig = sigma if mix else None
    if logits.dtype == torch.float32 and (sig is None or sig.dtype == torch.float32):
        return logits, sigma, 0
    if (desc is not None and logits.dtype == torch.bfloat16 and (sig is None or sig.dtype == torch.bfloat16)
            and C.load().pd_sweep_native_bf16(ctypes.byref(desc))):
        return logits, sigma, C.PD_LOGITS_BF16
    return as_f32(logits), as_f32(sig) if mix else sigma, 0


def plane_sweep_multi(deferred):
    """``deferred``: one SweepCall per target view as returned by ``plane_sweep_disp(..., defer=True)`` /
    ``plane_sweep_homography(..., defer=True)`` — all over the same (src, logits, sigma).  Returns a list of
    ``(rgb_rec, ph_map, ph_mean)`` per view; see _MultiPlaneSweep."""
    deferred = [SweepCall(*d) for d in deferred]
    if any(d.flags & C.PD_LOGITS_BF16 for d in deferred):
        # one node sums the views' gradients in place (PD_BWD_ACCUMULATE): fp32 only — every view sweeps ONE fp32 copy
        deferred = [d._replace(logits=as_f32(d.logits), sigma=as_f32(d.sigma), flags=d.flags & ~C.PD_LOGITS_BF16) for d in deferred]
    src, logits = deferred[0].src, deferred[0].logits
    sigma = next((d.sigma for d in deferred if d.sigma is not None), None)
    flat = []
    for d in deferred:
        if d.src is not src or d.logits is not logits or (d.sigma is not None and d.sigma is not sigma):
            raise ValueError("plane_sweep_multi: every view must sweep the same src / logits / sigma tensors")
        flat += [getattr(d, k) for k in _SIDE_FIELDS]   # (the decoder tail's link serves single-view nodes only)
    outs = _MultiPlaneSweep.apply(src, logits, sigma, *flat)
    return [tuple(outs[3 * i:3 * i + 3]) for i in range(len(deferred))]


_DISP_FLAG = {PF.PER_PLANE: 0, PF.ROWS: C.PD_DISP_ROWS, PF.DENSE: C.PD_DISP_DENSE}


def _flags(use_mixture_loss, automask, form=PF.PER_PLANE, render=False):
    return ((C.PD_MIXTURE if use_mixture_loss else 0) | (C.PD_AUTOMASK if automask else 0) |
            (C.PD_RENDER_PROB if render else 0) | _DISP_FLAG[form])


_SIGN = {"r": 1.0, "l": -1.0}


@functools.lru_cache(maxsize=None)
def _row_kernels(B, N, H, W, impl):
    """Do the row kernels serve disp mode at this shape under ``impl``?  pd_sweep_uses_rowshift (the per-row flags do not
    enter its answer), asked once per shape."""
    return bool(C.load().pd_sweep_uses_rowshift(ctypes.byref(C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, 0, 1.0, impl))))


def _same_mask_rows(rows, any_mask, tail_rows):
    """Does the sweep apply the padding mask the linked tail applied?  Neither has one, or both read the same [B,N,H] memory
    (``rows``: this call's row mask or None; ``any_mask``: it has a mask of some form; ``tail_rows``: TailLink.mask_rows).  Also
    asked about the per-row disparities (``any_mask`` False, TailLink.disp_rows)."""
    if rows is None or tail_rows is None:
        return rows is None and tail_rows is None and not any_mask
    return (rows.data_ptr() == tail_rows.data_ptr() and tuple(rows.shape) == tuple(tail_rows.shape)
            and rows.stride() == tail_rows.stride() and rows.dtype == tail_rows.dtype)


def _finish(call, defer, return_mean):
    """The end of plane_sweep_disp / plane_sweep_homography: the SweepCall itself (``defer``: for plane_sweep_multi, several
    target views as one autograd node) or its node's (rgb_rec, ph_map[, ph_map.mean() fused into the kernel])."""
    if defer:
        return call
    out = _PlaneSweep.apply(*call)
    return out if return_mean else out[:2]


def plane_sweep_disp(src, tgt, logits, sigma, disp_layered, padding_mask=None, *, target_side="r",
                     use_mixture_loss=True, automask=False, render_probability=False, dists=None, row_uniform=False,
                     return_mean=False, defer=False, _rows=None):
    """``disp_warp`` sweep (reference trainer.py:540-554 + 567-603 + 728-742) -> (rgb_rec, ph_map).

    ``disp_layered`` is the decoder's ``outputs["disp_layered"]``: either an expanded view of per-plane scalars
    ``[B,N,1,1] -> [B,N,H,W]`` (xy planes only; detected from its strides and passed as ``[B,N]`` without ever
    being materialised) or a dense ``[B,N,H,W]`` map (xz / yz planes present).  ``row_uniform=True`` promises that a
    dense map is constant along x (true for xy and xz planes: networks/depth_decoder.py:153-181 build them from the
    y-grid only; false once yz planes exist): its first column is then used as ``[B,N,H]`` per-row disparities, which
    keeps the row-shift kernels applicable.  A ROW VIEW — ``stride(3) == 0``, as ``ops.plane_geometry`` returns it, for the map
    and / or the mask — says the same through its strides: it takes the row route without the promise (``_row_view``).

    Gradient of a dense ``row_uniform`` map.  The reference's autograd hands ``disp_layered`` a dense [B,N,H,W] gradient
    (every column its own share).  Here the row's total ``g[b,n,y]`` comes back SPREAD EVENLY, ``g / W`` on every column, as
    a stride-0 view (``_FirstColumn``): anything that built the map from x-independent quantities — the decoder's
    ``expand`` and its y-grid formula, depth_decoder.py:153-181 — sums over x and receives exactly the reference's
    gradient, and nothing [B,N,H,W]-sized is written.  Per-column values differ from the reference's (their sum over x does
    not): a hook or a consumer that reads individual columns of ``disp_layered.grad`` must not pass ``row_uniform=True``.  A
    map that is a LEAF (``disp_layered.is_leaf``: somebody wants ``.grad`` itself) gets the plain select gradient instead —
    the row totals on column 0, zeros elsewhere.
    """
    B, N, H, W = logits.shape
    lib = C.load()
    sign = _SIGN.get(target_side, 0.0)  # any other key leaves the grid untouched (trainer.py:546-549)
    row_kernels = _row_kernels(B, N, H, W, S.SWEEP_IMPL)
    if _rows is not None:
        # internal (the stereo view of homography_warp): per-row shifts [B,N,H] and per-row mask [B,N,H] as they are — no
        # [B,N,H,W] view whose slice-backward would zero-fill and reduce 190 MB per step
        if row_kernels:
            shift, mask = _rows
            flags = _flags(use_mixture_loss, automask, PF.ROWS, render_probability) | C.PD_MASK_ROWS
            logits, sigma, bf = _storage_route(logits, sigma, use_mixture_loss, _desc(B, N, H, W, C.PD_WARP_DISP, flags, sign))
            return _finish(SweepCall(src, tgt, logits, sigma if use_mixture_loss else None, shift, None, None, mask,
                                     dists if render_probability else None, C.PD_WARP_DISP, flags | bf, sign), defer, return_mean)
        disp_layered, padding_mask = (t[..., None].expand(B, N, H, W) for t in _rows)   # PD_IMPL_GENERAL & co.
    # rows: a row view (constant along x by its strides: no promise, no data check) or row_uniform, where the row kernels serve
    form, plane = PF.disp_operand(disp_layered, B, N, H, W, rows=row_kernels, promise=row_uniform)
    flags = _flags(use_mixture_loss, automask, form, render_probability)
    if padding_mask is not None:
        # the mask of xy / xz planes is constant along x as well (depth_decoder.py:157, 166): hand over its first column
        mask_form, padding_mask = PF.mask_operand(padding_mask, B, N, H, W, rows=form != PF.DENSE and row_kernels,
                                                  promise=row_uniform)
        flags |= C.PD_MASK_ROWS if mask_form == PF.ROWS else 0
    # bf16 logits / sigma: native where the library serves the descriptor; a per-pixel mask is a fact of the call that no
    # descriptor shows, and PD_LOGITS_BF16 is refused with one — fp32 copies there and everywhere else
    per_pixel_mask = padding_mask is not None and not flags & C.PD_MASK_ROWS
    logits, sigma, bf = _storage_route(logits, sigma, use_mixture_loss,
                                       None if per_pixel_mask else _desc(B, N, H, W, C.PD_WARP_DISP, flags, sign))
    flags |= bf
    call = SweepCall(src, tgt, logits, sigma if use_mixture_loss else None, plane, None, None, padding_mask,
                     dists if render_probability else None, C.PD_WARP_DISP, flags, sign)
    # a fused decoder tail that asked for it (decoder_tail(..., fuse_sweep_backward=True)) gets its backward applied by this
    # sweep's backward kernel — where the library serves that form for this descriptor (mixture, one disparity per plane or per
    # row, ...: pd_sweep_bwd_tail_fuses, or pd_sweep_bwd_tail_rows_fuses for PD_DISP_ROWS / PD_MASK_ROWS), the call has fp32
    # storage and its padding mask is the tail's: none, or the same [B,N,H] rows.  Anything else — a per-pixel mask here, a mask
    # on one side only — is a consumer the fused form does not serve
    link = getattr(logits, "_pd_tail_link", None)
    fuses = lib.pd_sweep_bwd_tail_rows_fuses if flags & (C.PD_DISP_ROWS | C.PD_MASK_ROWS) else lib.pd_sweep_bwd_tail_fuses
    if (link is not None and not bf and getattr(sigma, "_pd_tail_link", None) is link
            and _same_mask_rows(padding_mask if flags & C.PD_MASK_ROWS else None, padding_mask is not None, link.mask_rows)
            and _same_mask_rows(plane if form == PF.ROWS else None, False, link.disp_rows)
            and fuses(ctypes.byref(_desc(B, N, H, W, C.PD_WARP_DISP, flags, sign)))):
        link.consumers += 1
        call = call._replace(link=link)
    elif link is not None:
        link.consumers += 2   # a consumer the fused form does not serve: nobody fuses
    return _finish(call, defer, return_mean)


def homography_matrices(d, n, T, K, inv_K):
    """The O(B*N) 3x3 algebra of HomographyWarp.forward (layers.py:206-219, 223) in stock torch.

    Stays in torch on purpose: it keeps ``torch.inverse``'s rounding and lets autograd carry the
    gradient of ``H_t2s`` on to the pose network / plane distances.  Returns (H_t2s [BN,3,3], R·n [BN,3]).
    """
    B, N = d.shape
    Rm = T[:, :3, :3]
    t = T[:, :3, 3:4]
    nn_ = n.reshape(B * N, 1, 3)
    Rtnd = Rm + torch.matmul(t, nn_) / d.reshape(B * N, 1, 1)
    H_s2t = torch.matmul(K[:, :3, :3], torch.matmul(Rtnd, inv_K[:, :3, :3]))
    H_t2s = torch.inverse(H_s2t)
    Rn = torch.matmul(Rm, nn_.transpose(1, 2))[:, :, 0]
    return H_t2s, Rn


class _HomographyMatrices(torch.autograd.Function):
    """pd_homography_matrices_fwd/bwd: (distance [B,N], norm [B,N,3], T, K, inv_K [B,4,4]) -> per ``mode``
    (H_t2s, Rn) or (shift, mask, Rn).  Gradients to distance, norm and T."""

    @staticmethod
    def forward(ctx, distance, norm, T, K, inv_K, mode, rows):
        B, N = distance.shape
        dev = distance.device
        distance, norm, T, K, inv_K = (_contig(t.detach().float()) for t in (distance, norm, T, K, inv_K))
        for name, t, shape in (("distance", distance, (B, N)), ("norm", norm, (B, N, 3)), ("T", T, (B, 4, 4)),
                               ("K", K, (B, 4, 4)), ("inv_K", inv_K, (B, 4, 4))):
            C.require_gpu_tensor(name, t, shape)
        Rn = torch.empty(B, N, 3, device=dev)
        Hm = shift = mask = None
        if mode == C.PD_HMAT_STEREO_ROWS:
            shift, mask = torch.empty(B, N, rows, device=dev), torch.empty(B, N, rows, device=dev)
        else:
            Hm = torch.empty(B, 4 if mode == C.PD_HMAT_UNIFORM else N, 3, 3, device=dev)
        C.call("pd_homography_matrices_fwd", dev, B, N, mode, rows, distance, norm, T, K, inv_K, Hm, Rn, shift, mask)
        ctx.save_for_backward(distance, norm, T, K, inv_K)
        ctx.mode, ctx.rows = mode, rows
        ctx.set_materialize_grads(False)   # (else autograd zero-fills gradients for the non-differentiable Rn / mask: two launches)
        if mode == C.PD_HMAT_STEREO_ROWS:
            ctx.mark_non_differentiable(mask, Rn)   # (one call: a second call replaces the first one's set)
            return shift, mask, Rn
        ctx.mark_non_differentiable(Rn)
        return Hm, Rn

    @staticmethod
    def backward(ctx, g_first, *_):
        distance, norm, T, K, inv_K = ctx.saved_tensors
        B, N = distance.shape
        dev = distance.device
        need_d, need_n, need_T = ctx.needs_input_grad[:3]
        stereo = ctx.mode == C.PD_HMAT_STEREO_ROWS
        if stereo and (need_n or need_T):
            raise RuntimeError("PD_HMAT_STEREO_ROWS carries the gradient of `distance` only (h00 is not part of the "
                               "per-row shift); use PD_HMAT_PLANES when the pose or the normals need gradients")
        if g_first is None:   # the matrices took no part in the loss
            return None, None, None, None, None, None, None
        g_first = _contig(g_first.float())
        gd = torch.empty(B, N, device=dev) if need_d else None
        gn = torch.empty(B, N, 3, device=dev) if need_n else None
        gT = torch.empty(B, 4, 4, device=dev) if need_T else None
        C.call("pd_homography_matrices_bwd", dev, B, N, ctx.mode, ctx.rows, distance, norm, T, K, inv_K,
               None if stereo else g_first, g_first if stereo else None, gd, gn, gT)
        return gd, gn, gT, None, None, None, None


def homography_matrices_fused(distance, norm, T, K, inv_K, mode=C.PD_HMAT_PLANES, rows=0):
    """layers.py:206-219, 223-225 in one launch (fp64 inside, rounded once): see include/planedepth_hip.h,
    ``pd_homography_matrices_fwd``.  distance [B,N], norm [B,N,3], T / K / inv_K [B,4,4] (NOT expanded over planes).
    Returns (H_t2s, Rn) — [B,N,3,3] or, PD_HMAT_UNIFORM, [B,4,3,3] — or (shift, mask, Rn) for PD_HMAT_STEREO_ROWS."""
    B, N = distance.shape
    if tuple(norm.shape) != (B, N, 3):
        norm = norm.expand(B, N, 3)
    return _HomographyMatrices.apply(distance, norm, T, K, inv_K, int(mode), int(rows))


def plane_sweep_homography(src, tgt, logits, sigma, distance, norm, T, K, inv_K, *, use_mixture_loss=True,
                           automask=False, render_probability=False, dists=None, return_mean=False, plane_uniform=False,
                           stereo_rows=False, defer=False):
    """``homography_warp`` sweep (reference trainer.py:556-560 + layers.py:206-234 + trainer.py:567-603, 728-742).

    distance [B,N], norm [B,N,3]; T, K, inv_K are the per-image [B,4,4] matrices (expanded over planes here).

    ``plane_uniform=True`` is the caller's promise that T has ZERO translation (what Trainer.predict_poses produces for
    the novel frames without COLMAP, trainer.py:386-400): K (R + t n^T/d) K^-1 is then the same matrix for every plane,
    so ONE homography per image is formed (from plane 0's d, n — they drop out) and the plane-uniform kernels run
    (geometry once per pixel, atomic-free backward).  The facing test keeps its per-plane normals.

    ``stereo_rows=True`` is the caller's promise that T is the dataset's stereo extrinsic (identity rotation, translation
    along x only: datasets/mono_dataset.py:203-211) and that no plane normal has an x component (xy and xz planes,
    networks/depth_decoder.py:153-207).  K (I + t n^T/d) K^-1 then differs from the identity in h01 and h02 only: the
    warp is a horizontal shift ``h01*y + h02`` per (plane, row) and the facing test is constant along x, i.e. exactly
    the ``disp_warp`` sweep with per-row disparities and a per-row mask, which runs on the row-shift kernels (no
    atomics).  H_t2s is still formed by the reference's chain (torch.inverse and all) and autograd carries the
    gradient of the shifts back into ``distance``; it is NOT taken when T or norm require gradients (their
    derivatives need h00 as well).
    """
    B, N, H, W = logits.shape
    if plane_uniform and N * H * W >= (1 << 29):
        plane_uniform = False   # the plane-uniform kernels address one image's [N,H,W] block with 32-bit byte offsets; beyond
        # that the per-plane route below (one matrix per plane, 64-bit addressing) serves the same poses
    # (PD_TORCH_HOMOGRAPHY: the row form's premise h00 = 1, z = 1 holds to 2e-7 for the fp64-formed matrices only; an fp32
    # torch.inverse at cond ~1e3 leaves h00 - 1 ~ 1e-5, i.e. up to 6e-3 pixels across a 640-pixel row, which the reference's own
    # chain carries into the result (measured on the reference-captured matrices: rgb_rec 1.9e-4 off) -> per-plane kernels)
    if stereo_rows and not S.TORCH_HOMOGRAPHY and not T.requires_grad and not norm.requires_grad:
        return _stereo_rows_sweep(src, tgt, logits, sigma, distance, norm, T, K, inv_K, use_mixture_loss, automask,
                                  return_mean, defer, render_probability, dists)
    ex = lambda M: M[:, None].expand(-1, N, -1, -1).reshape(B * N, 4, 4)  # noqa: E731
    inv_K3 = inv_K[:, :3, :3]
    logits, sigma, _ = _storage_route(logits, sigma, use_mixture_loss, None)   # (per-plane / plane-uniform matrices: fp32 only)
    flags = _flags(use_mixture_loss, automask, render=render_probability)
    tw = None
    if plane_uniform:
        # One matrix per image (slice 0, layers.py:216-218 for plane 0 with the — zero — translation detached) plus the
        # homographies of three virtual planes n/d = e_j that carry the translation's gradient (include/planedepth_hip.h,
        # PD_HOMO_UNIFORM): dL/dt = sum_j <sum_n G_n n_n[j]/d_n, d f(R + t e_j^T)/dt> is the per-plane formulation's.
        if S.TORCH_HOMOGRAPHY:
            Rm, t = T[:, :3, :3], T[:, :3, 3:4]
            K3 = K[:, :3, :3]
            n0 = norm[:, 0].reshape(B, 1, 3)
            eye = torch.eye(3, device=T.device, dtype=T.dtype)
            # [B,4,3,3] in one batch: slice 0 = R + t_detached n0^T / d0, slices 1..3 = R_detached + t e_j^T
            Rtnd = torch.cat([(Rm + torch.matmul(t.detach(), n0) / distance[:, 0].reshape(B, 1, 1))[:, None],
                              Rm.detach()[:, None] + t[:, None] * eye.reshape(1, 3, 1, 3)], 1)
            H_t2s = torch.inverse(torch.matmul(K3[:, None], torch.matmul(Rtnd, inv_K3[:, None])))       # [B,4,3,3]
            with torch.no_grad():
                Rn = torch.matmul(Rm[:, None], norm.reshape(B, N, 3, 1))[..., 0].reshape(B * N, 3)
        else:
            H_t2s, Rn = homography_matrices_fused(distance.detach(), norm.detach(), T, K, inv_K, C.PD_HMAT_UNIFORM)
            Rn = Rn.reshape(B * N, 3)
        with torch.no_grad():
            tw = (norm / distance[..., None]).contiguous()                                # [B,N,3]
        flags |= C.PD_HOMO_UNIFORM
    elif S.TORCH_HOMOGRAPHY:
        H_t2s, Rn = homography_matrices(distance, norm, ex(T), ex(K), ex(inv_K))
    else:
        H_t2s, Rn = homography_matrices_fused(distance, norm, T, K, inv_K)
        H_t2s, Rn = H_t2s.reshape(B * N, 3, 3), Rn.reshape(B * N, 3)
    call = SweepCall(src, tgt, logits, sigma if use_mixture_loss else None, H_t2s, Rn.detach().contiguous(), inv_K3.detach(), tw,
                     dists if render_probability else None, C.PD_WARP_HOMOGRAPHY, flags, 0.0)
    return _finish(call, defer, return_mean)


def _stereo_rows_sweep(src, tgt, logits, sigma, distance, norm, T, K, inv_K, mix, automask, return_mean, defer=False,
                       render=False, dists=None):
    B, N, H, W = logits.shape
    shift, mask, _ = homography_matrices_fused(distance, norm, T, K, inv_K, C.PD_HMAT_STEREO_ROWS, rows=H)
    return plane_sweep_disp(src, tgt, logits, sigma, None, None, target_side="r", use_mixture_loss=mix,
                            automask=automask, row_uniform=True, return_mean=return_mean, defer=defer,
                            render_probability=render, dists=dists, _rows=(shift, mask))


def plane_sweep_layers(src, logits, sigma, *, disp_layered=None, padding_mask=None, target_side="r",
                       homography=None, use_mixture_loss=True, render_probability=False, dists=None,
                       want=("rgb_rec_layered", "logit_rec", "probability_rec", "sigma_rec", "pi_rec")):
    """Materialise the per-plane tensors the reference keeps in ``outputs`` (trainer.py:582-602).  No gradients."""
    B, N, H, W = logits.shape
    with torch.no_grad():
        logits, sigma, _ = _storage_route(logits, sigma, use_mixture_loss, None)   # (the layers kernel reads fp32 only)
        if homography is None:
            form, plane = PF.disp_operand(disp_layered, B, N, H, W, grad=False, row_views=False)   # layers: general kernels
            aux = k3 = None
            mode, sign = C.PD_WARP_DISP, _SIGN.get(target_side, 0.0)
            flags = _flags(use_mixture_loss, False, form, render_probability)
            if padding_mask is not None:
                padding_mask = PF.mask_operand(padding_mask, B, N, H, W, row_views=False)[1].contiguous()
        else:
            plane, aux, k3 = (t.contiguous() for t in homography)
            mode, sign, padding_mask = C.PD_WARP_HOMOGRAPHY, 0.0, None
            flags = _flags(use_mixture_loss, False, render=render_probability)
        dev = logits.device
        out = {}
        shapes = dict(rgb_rec_layered=(B, N, 3, H, W), logit_rec=(B, N, H, W), probability_rec=(B, N, H, W),
                      sigma_rec=(B, N, H, W), pi_rec=(B, N, H, W))
        for k in want:
            if k in ("sigma_rec", "pi_rec") and not use_mixture_loss:
                continue
            out[k] = torch.empty(shapes[k], device=dev, dtype=torch.float32)
        d = _desc(B, N, H, W, mode, flags, sign)
        C.call("pd_plane_sweep_layers", dev, ctypes.byref(d), src.contiguous(), logits.contiguous(),
               _contig(sigma) if use_mixture_loss else None, plane, aux, k3, padding_mask,
               dists.contiguous() if render_probability else None, out.get("rgb_rec_layered"), out.get("logit_rec"),
               out.get("probability_rec"), out.get("sigma_rec"), out.get("pi_rec"))
    return out
