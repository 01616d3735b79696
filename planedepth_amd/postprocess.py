"""Forward-only operators around the batch: the self-distillation post-process (trainer.py:404-466), the batch doubling of
add_flip_right_inputs (trainer.py:252-276), the dataset's crop grid (datasets/pair_transforms.py:27-56).
"""
import ctypes

from . import _capi as C
from . import planeform as PF
from ._buffers import torch, _contig

_DISP_FLAG = {PF.PER_PLANE: 0, PF.ROWS: C.PD_PP_DISP_ROWS, PF.DENSE: C.PD_PP_DISP_DENSE}


# ---------------------------------------------------------------------------------------------------------------------
# Post-process warps — forward only, as in the reference (no_grad networks, detached result)
# ---------------------------------------------------------------------------------------------------------------------
def _pp_disp(disp_layered, B, N, H, W, row_uniform=False):
    """(tensor, flags) of ``PF.disp_operand``: rows for a row view, under the ``row_uniform`` promise (xy and xz planes:
    networks/depth_decoder.py:153-181; yz planes are not) and for a [B,N,H,1] map, which the expand over x makes a row view."""
    form, disp = PF.disp_operand(disp_layered, B, N, H, W, promise=row_uniform or (disp_layered.shape[-1] == 1 and W > 1), grad=False)
    return disp, _DISP_FLAG[form]


def _route_dict(r):
    return dict(family=C.PD_PP_FAMILIES[r.family], flip=bool(r.flip), nmax=int(r.nmax), rows2=bool(r.rows2), alias=bool(r.alias),
                lds_bytes=int(r.lds_bytes))


def warp_route(kind, B, N, H, W, flags=0, out_ptr=0):
    """The kernel ``pd_warp_softmax`` (``kind="softmax"``) / ``pd_warp_sum`` (``"sum"``) runs for this shape, these
    ``PD_PP_*`` flags and an ``out`` buffer at address ``out_ptr`` (only its alignment counts; 0: 8-byte aligned), as a dict
    of ``pd_pp_route``'s fields with the family by name.  Answered on the host: no GPU needed."""
    r = C.PpRoute()
    C.check(C.load().pd_warp_route({"softmax": C.PD_PP_KIND_SOFTMAX, "sum": C.PD_PP_KIND_SUM}[kind], B, N, H, W, int(flags),
                                   ctypes.c_void_p(int(out_ptr)), ctypes.byref(r)), "pd_warp_route")
    return _route_dict(r)


def post_process_route(B, N, H, W, flags=0, workspace_ptr=0, disp_pp_ptr=0):
    """The kernels ``pd_post_process`` runs (B: half of the doubled batch): ``family`` "chain" / "chain_split" (the fused row
    chains) or "single" (two warp-softmaxes, three warp-sums and the blend, each on its own ``warp_route``)."""
    r = C.PpRoute()
    C.check(C.load().pd_post_process_route(B, N, H, W, int(flags), ctypes.c_void_p(int(workspace_ptr)),
                                           ctypes.c_void_p(int(disp_pp_ptr)), ctypes.byref(r)), "pd_post_process_route")
    return _route_dict(r)


def warp_softmax(planes, disp_layered, sign, flip_src=False, row_uniform=False):
    """softmax over the planes of ``planes`` sampled at x + sign * disp (trainer.py:443-446 / 451-453)."""
    C.require_gpu_tensor("planes", planes)
    B, N, H, W = planes.shape
    with torch.no_grad():
        planes = planes.detach().contiguous()
        disp, flags = _pp_disp(disp_layered.detach(), B, N, H, W, row_uniform)
        out = torch.empty_like(planes)
        C.call("pd_warp_softmax", planes.device, B, N, H, W, float(sign), flags | (C.PD_PP_FLIP_SRC if flip_src else 0), planes,
               disp, out)
    return out


def warp_sum(planes, disp_layered, sign, cap=1.0, flip_src=False, row_uniform=False):
    """min(cap, sum over the planes of ``planes`` sampled at x + sign * disp) (trainer.py:447-449, 454-456, 463-465)."""
    C.require_gpu_tensor("planes", planes)
    B, N, H, W = planes.shape
    with torch.no_grad():
        planes = planes.detach().contiguous()
        disp, flags = _pp_disp(disp_layered.detach(), B, N, H, W, row_uniform)
        out = torch.empty(B, 1, H, W, device=planes.device, dtype=torch.float32)
        C.call("pd_warp_sum", planes.device, B, N, H, W, float(sign), flags | (C.PD_PP_FLIP_SRC if flip_src else 0), planes,
               disp, float(cap), out)
    return out


def pp_combine(disp, o_fr, o_l):
    """disp_pp of trainer.py:458-461 in one launch: ``disp`` [2B,1,H,W] (image, mirrored image), the occlusion masks
    ``o_fr`` / ``o_l`` [B,1,H,W] -> mean-of-both where o_fr says so, the mirrored pass's disparity where o_l is 0."""
    C.require_gpu_tensor("disp", disp)
    B2, _, H, W = disp.shape
    B = B2 // 2
    C.require_gpu_tensor("o_fr", o_fr, (B, 1, H, W))
    C.require_gpu_tensor("o_l", o_l, (B, 1, H, W))
    with torch.no_grad():
        disp, o_fr, o_l = (_contig(t.detach()) for t in (disp, o_fr, o_l))
        out = torch.empty(B, 1, H, W, device=disp.device, dtype=torch.float32)
        C.call("pd_pp_combine", disp.device, B, H, W, disp, o_fr, o_l, out)
    return out


def post_process_disp(logits, probability, disp, disp_layered, row_uniform=False):
    """trainer.py:421-466 given the fixed model's outputs for cat([image, mirrored image]) -> (disp_pp, mask_novel): ONE C-ABI
    call (pd_post_process: row chains where a row's softmax fits the CU's LDS, else two warp-softmaxes, three warp-sums and the
    blend).  ``row_uniform=True`` promises a dense ``disp_layered`` that is constant along x (no yz planes): it is then read as
    one disparity per (plane, row) and the row kernels / chains serve it instead of the per-pixel gather form.
    bf16 ``logits`` / ``probability`` (a teacher run under ``torch.autocast``) are widened with ``.float()`` first — exact, and
    no native bf16 kernel yet; any other dtype raises."""
    lib = C.load()
    C.require_gpu_tensor("logits", logits, dtype=torch.bfloat16 if logits.dtype == torch.bfloat16 else torch.float32)
    B2, N, H, W = logits.shape
    B = B2 // 2
    with torch.no_grad():
        prob = probability.tensor() if hasattr(probability, "tensor") else probability
        if logits.dtype == torch.bfloat16:
            logits = logits.float()
        if torch.is_tensor(prob) and prob.dtype == torch.bfloat16:
            prob = prob.float()
        logits, prob, disp = (_contig(t.detach()) for t in (logits, prob, disp))
        dl, flags = _pp_disp(disp_layered.detach(), B2, N, H, W, row_uniform)
        dev = logits.device
        ws = torch.empty(lib.pd_post_process_workspace_floats(B, N, H, W), device=dev, dtype=torch.float32)
        disp_pp = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
        mask_novel = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
        C.call("pd_post_process", dev, B, N, H, W, flags, logits, prob, disp, dl, ws, disp_pp, mask_novel)
    return disp_pp, mask_novel


def post_process_disp_stepwise(logits, probability, disp, disp_layered, row_uniform=False):
    """The same through the single operators (cross-check of pd_post_process; what round 5 ran)."""
    B = probability.shape[0] // 2
    with torch.no_grad():
        dl_r, dl_l = disp_layered[:B], disp_layered[B:]
        ru = dict(row_uniform=row_uniform)
        plr = warp_softmax(logits[:B], dl_r, +1.0, **ru)                 # :443-446
        o_l = warp_sum(plr, dl_l, -1.0, **ru)                            # :447-449
        pfrl = warp_softmax(logits[B:], dl_l, -1.0, flip_src=True, **ru)  # :451-453 (the flip is folded into the read)
        o_fr = warp_sum(pfrl, dl_r, +1.0, **ru)                          # :454-456
        disp_pp = pp_combine(disp, o_fr, o_l)                            # :458-461
        prob = probability.tensor() if hasattr(probability, "tensor") else probability
        mask_novel = warp_sum(prob[:B], dl_r, +1.0, **ru)                # :463-465
    return disp_pp, mask_novel


# ---------------------------------------------------------------------------------------------------------------------
# Batch doubling of add_flip_right_inputs
# ---------------------------------------------------------------------------------------------------------------------
def cat_flip(own, other, negate_c0=False):
    """cat([own, other.flip(-1)], dim=0) in one kernel (trainer.py:253-262); ``negate_c0`` for the grid tensor."""
    C.require_gpu_tensor("own", own)
    C.require_gpu_tensor("other", other, tuple(own.shape))
    B, Cn, H, W = own.shape
    with torch.no_grad():
        own, other = own.contiguous(), other.contiguous()
        out = torch.empty(2 * B, Cn, H, W, device=own.device, dtype=torch.float32)
        C.call("pd_cat_flip", own.device, B, Cn, H, W, own, other, int(bool(negate_c0)), out)
    return out


def crop_grid(params, height, width):
    """``inputs["grid"]`` [B,2,H,W] on the device from per-sample crop parameters [B,4] int32 = (full_w, full_h, w0, h0)
    (datasets/pair_transforms.py:27-37: the RandomResizeCrop grid; Resize is full = (W, H), origin 0) — the reference's
    ``torch.linspace`` / ``meshgrid`` / crop to one ulp (torch's vectorised linspace itself differs in the last bit between
    host CPUs: tests/test_gpu_parity.py::test_on_device_grid_matches_the_reference_pipeline_to_one_ulp)."""
    C.require_gpu_tensor("params", params, dtype=torch.int32)
    if params.dim() != 2 or params.shape[1] != 4:
        raise ValueError("params must be [B,4] int32 (full_w, full_h, w0, h0), got %s" % (tuple(params.shape),))
    B = params.shape[0]
    params = params.contiguous()
    grid = torch.empty(B, 2, int(height), int(width), device=params.device, dtype=torch.float32)
    C.call("pd_crop_grid", params.device, B, int(height), int(width), params, grid)
    return grid
