"""The pose path of ``Trainer.predict_poses`` (reference trainer.py:358-402) as one operator each way: from the pose decoder's last
conv output, or from its ``axisangle``, to ``Rt``.

Per novel frame the reference runs the tail of ``PoseDecoder.forward`` (networks/pose_net.py:148-155: two means, a scale, a view, two
slices), ``transformation_from_parameters`` (layers.py:17-92: about twenty element-wise operators and nine indexed stores), builds
``Rc`` from six indexed reads of ``inputs["grid"]`` and conjugates with a batched ``torch.inverse`` (trainer.py:386-400) — some fifty
launches forward, as many backward, for ``B`` 3x3 matrices.  ``pd_pose_tail_fwd`` / ``pd_pose_tail_bwd`` (pd_pose_tail.hip) are one
launch each, in fp64 and rounded once, and can be captured in a HIP graph.  Nothing but the inputs is kept for backward.  No eager /
CPU implementation stands behind the operators.
"""
import ctypes

import torch

from . import _capi as C

DEFAULT_SCALE = 0.01   # networks/pose_net.py:150


class RawPose:
    """What a ``PoseDecoder.forward`` returns INSTEAD of executing networks/pose_net.py:148-155: its last conv output ``[B,6F,h,w]``,
    untouched.  ``trainer_path.predict_poses`` then takes mean, scale, rotation and conjugation in one launch."""
    __slots__ = ("out",)

    def __init__(self, out):
        if not torch.is_tensor(out) or out.dim() != 4 or out.shape[1] % 6:
            raise ValueError("RawPose takes the pose decoder's last conv output [B,6F,h,w], got %s"
                             % (tuple(out.shape) if torch.is_tensor(out) else type(out).__name__,))
        self.out = out


def _position_stride(t):
    """Element stride of the flattened ``h*w`` axis of a ``[B,C,h,w]`` tensor, or None where the two axes do not flatten."""
    h, w = int(t.shape[2]), int(t.shape[3])
    if h * w == 1:
        return 0
    if w == 1:
        return t.stride(2)
    if h == 1 or t.stride(2) == w * t.stride(3):
        return t.stride(3)
    return None


def _layout(t):
    """(C, hw, image / channel / position strides) of a conv output ``[B,C,h,w]`` or an axis-angle ``[B,3]`` / ``[B,1,3]``."""
    if t.dim() == 4:
        return int(t.shape[1]), int(t.shape[2] * t.shape[3]), t.stride(0), t.stride(1), _position_stride(t)
    return 3, 1, t.stride(0), t.stride(-1), 0


def _grid_args(grid):
    return int(grid.shape[2]), int(grid.shape[3]), (ctypes.c_int64 * 4)(*grid.stride())


def _check_grid(grid, B):
    if not torch.is_tensor(grid):
        raise TypeError("grid must be a tensor")
    if grid.dim() != 4 or grid.shape[0] != B or grid.shape[1] != 2 or grid.shape[2] < 1 or grid.shape[3] < 1:
        raise ValueError("grid must be [%d,2,H,W], got %s" % (B, tuple(grid.shape)))
    if grid.requires_grad:
        raise ValueError("grid requires a gradient: the pose operators have none for it (the reference's grid never requires one)")


def _gpu_grid(grid):
    if not grid.is_cuda:
        raise C.PlaneDepthHipError("grid is on %s: planedepth_amd runs on the GPU only (no CPU fallback)" % grid.device)
    return grid if grid.dtype == torch.float32 else grid.float()


class _PoseTail(torch.autograd.Function):
    """pd_pose_tail_fwd/bwd: (x, grid) -> (axisangle [B,3], translation [B,3], Rc [B,3,3], Rt_Rc [B,4,4]); ``x`` is the conv output
    ``[B,6F,h,w]`` or an axis-angle ``[B,3]`` / ``[B,1,3]`` (then the first two results are None).  Gradient to ``x``."""

    @staticmethod
    def forward(ctx, x, grid, invert, frame, scale):
        dev = x.device
        in_dtype = x.dtype
        x = x.detach()
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        if x.dim() == 4 and _position_stride(x) is None:
            x = x.contiguous()
        B = int(x.shape[0])
        Cn, hw, sb, sc, ss = _layout(x)
        tail = x.dim() == 4
        aa = torch.empty(B, 3, device=dev) if tail else None
        tr = torch.empty(B, 3, device=dev) if tail else None
        Rc = torch.empty(B, 3, 3, device=dev)
        Rt_Rc = torch.empty(B, 4, 4, device=dev)
        dtype = C.PD_DTYPE_BF16 if x.dtype == torch.bfloat16 else C.PD_DTYPE_F32
        gH, gW, gs = _grid_args(grid)
        C.call("pd_pose_tail_fwd", dev, B, Cn, hw, frame, dtype, int(invert), scale, x, sb, sc, ss, None, grid, gH, gW, gs, aa,
               tr, Rc, Rt_Rc)
        ctx.save_for_backward(x, grid)
        ctx.args = (invert, frame, scale, dtype, in_dtype)
        ctx.set_materialize_grads(False)   # (an output nobody used stays None: a NULL pointer, not a zero-fill launch)
        ctx.mark_non_differentiable(Rc)    # (the only call: a second one would replace this set)
        return aa, tr, Rc, Rt_Rc

    @staticmethod
    def backward(ctx, g_aa, g_tr, _g_Rc, g_Rt_Rc):
        if (g_aa is None and g_tr is None and g_Rt_Rc is None) or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        x, grid = ctx.saved_tensors
        invert, frame, scale, dtype, in_dtype = ctx.args
        dev = x.device
        B = int(x.shape[0])
        Cn, hw, sb, sc, ss = _layout(x)
        g_aa, g_tr, g_Rt_Rc = (None if g is None else g.float().contiguous() for g in (g_aa, g_tr, g_Rt_Rc))
        g_x = torch.empty_like(x)
        if g_x.dim() == 4 and _position_stride(g_x) is None:
            g_x = torch.empty(x.shape, device=dev, dtype=x.dtype)
        _, _, gsb, gsc, gss = _layout(g_x)
        gH, gW, gs = _grid_args(grid)
        C.call("pd_pose_tail_bwd", dev, B, Cn, hw, frame, dtype, int(invert), scale, x, sb, sc, ss, grid, gH, gW, gs, g_Rt_Rc,
               g_aa, g_tr, g_x, gsb, gsc, gss)
        return (g_x if g_x.dtype == in_dtype else g_x.to(in_dtype)), None, None, None, None


def _require_gpu_float(name, t):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor" % name)
    if not t.is_floating_point():
        raise TypeError("%s must be a floating-point tensor, got %s" % (name, t.dtype))
    if not t.is_cuda:
        raise C.PlaneDepthHipError("%s is on %s: planedepth_amd runs on the GPU only (no CPU fallback)" % (name, t.device))


def pose_matrices(axisangle, grid, invert=False):
    """``transformation_from_parameters(axisangle, ., invert)`` conjugated with ``Rc`` (trainer.py:381-400 without COLMAP) in one
    launch: ``(Rt_Rc [B,4,4], Rc [B,3,3])``.  ``axisangle`` is ``[B,1,3]`` or ``[B,3]`` with any strides (the reference's
    ``axisangle[:, 0]`` is read in place) and receives the gradient; the network's translation never reaches ``Rt_Rc`` there, and
    ``Rt_Rc[:, 3, 3]`` is 0 as in the reference.  ``PlaneDepthHipError`` for CPU tensors: there is no fallback."""
    if not torch.is_tensor(axisangle):
        raise TypeError("axisangle must be a tensor")
    if not (axisangle.dim() in (2, 3) and axisangle.shape[-1] == 3 and (axisangle.dim() == 2 or axisangle.shape[1] == 1)):
        raise ValueError("axisangle must be [B,1,3] or [B,3], got %s" % (tuple(axisangle.shape),))
    _check_grid(grid, int(axisangle.shape[0]))
    _require_gpu_float("axisangle", axisangle)   # arguments first, devices last: what is wrong with a call does not depend on where it runs
    grid = _gpu_grid(grid)
    _, _, Rc, Rt_Rc = _PoseTail.apply(axisangle, grid, bool(invert), 0, 1.0)
    return Rt_Rc, Rc


def pose_tail(conv_out, grid, invert=False, frame=0, scale=DEFAULT_SCALE):
    """The tail of ``PoseDecoder.forward`` (networks/pose_net.py:148-155) and trainer.py:381-400 from the decoder's last conv output
    ``[B,6F,h,w]`` (fp32 or bf16, contiguous or channels-last read in place) for one ``frame`` of its ``F``:
    ``(axisangle [B,1,1,3], translation [B,1,1,3], Rc [B,3,3], Rt_Rc [B,4,4])``, fp32.  The gradient of all but ``Rc`` reaches
    ``conv_out`` in its own dtype.  ``PlaneDepthHipError`` for CPU tensors: there is no fallback."""
    if not torch.is_tensor(conv_out):
        raise TypeError("conv_out must be a tensor")
    if conv_out.dim() != 4 or conv_out.shape[1] % 6 or conv_out.shape[1] == 0 or conv_out.shape[2] * conv_out.shape[3] == 0:
        raise ValueError("conv_out must be [B,6F,h,w], got %s" % (tuple(conv_out.shape),))
    frame = int(frame)
    if not 0 <= frame < conv_out.shape[1] // 6:
        raise ValueError("frame %d: conv_out holds %d" % (frame, conv_out.shape[1] // 6))
    B = int(conv_out.shape[0])
    _check_grid(grid, B)
    _require_gpu_float("conv_out", conv_out)
    grid = _gpu_grid(grid)
    aa, tr, Rc, Rt_Rc = _PoseTail.apply(conv_out, grid, bool(invert), frame, float(scale))
    return aa.view(B, 1, 1, 3), tr.view(B, 1, 1, 3), Rc, Rt_Rc


def pose_conjugate(Rt, grid):
    """The COLMAP mode of trainer.py:384-400: ``Rt_Rc[:, :3, :3] = Rc Rt[:, :3, :3] Rc^-1``, ``Rt_Rc[:, :3, 3] = Rc Rt[:, :3, 3]``, row 3
    zero.  ``Rt`` is ``[B,4,4]``, a dataset constant: ``ValueError`` if it requires a gradient.  Returns ``(Rt_Rc, Rc)``."""
    if not torch.is_tensor(Rt):
        raise TypeError("Rt must be a tensor")
    if Rt.dim() != 3 or tuple(Rt.shape[1:]) != (4, 4):
        raise ValueError("Rt must be [B,4,4], got %s" % (tuple(Rt.shape),))
    if Rt.requires_grad:
        raise ValueError("Rt requires a gradient: pose_conjugate is forward only (COLMAP poses are dataset constants)")
    B = int(Rt.shape[0])
    _check_grid(grid, B)
    _require_gpu_float("Rt", Rt)
    grid = _gpu_grid(grid)
    dev = Rt.device
    with torch.no_grad():
        Rt = Rt.float().contiguous()
        Rc = torch.empty(B, 3, 3, device=dev)
        Rt_Rc = torch.empty(B, 4, 4, device=dev)
        gH, gW, gs = _grid_args(grid)
        C.call("pd_pose_tail_fwd", dev, B, 0, 0, 0, C.PD_DTYPE_F32, 0, 1.0, None, 0, 0, 0, Rt, grid, gH, gW, gs, None, None, Rc,
               Rt_Rc)
    return Rt_Rc, Rc
