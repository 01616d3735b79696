"""The three forms of the decoder's ``disp_layered`` / ``padding_mask`` — per-plane scalars [B,N], per-row values [B,N,H], a dense
[B,N,H,W] map — and the tensor a kernel reads for each, decided in ONE place for the plane sweep, the two tails and the post-process.
The fused tail backward depends on the sweep and the decoder tail deriving the same [B,N,H] memory (``sweep._same_mask_rows``).
Pure torch on metadata and views: nothing here launches a kernel."""
import torch

PER_PLANE, ROWS, DENSE = 0, 1, 2


def _per_plane_view(disp_layered):
    """[B,N] view of an H/W-expanded disparity tensor, taken from the tensor it was expanded FROM when possible.

    ``disp_layered[:, :, 0, 0]`` would be correct but makes autograd materialise a zero [B,N,H,W] gradient and then
    reduce it again (ExpandBackward): ~0.1 ms per step of pure overhead at 8x49x192x640.  When the view's base is the
    decoder's [B,N,1,1] tensor (networks/depth_decoder.py:153-156) the gradient is handed to that tensor directly.
    """
    B, N = disp_layered.shape[:2]
    base = disp_layered._base
    if (base is not None and base.dim() == 4 and tuple(base.shape) == (B, N, 1, 1)
            and base.storage_offset() == disp_layered.storage_offset()
            and base.stride()[:2] == disp_layered.stride()[:2]
            and base.requires_grad == disp_layered.requires_grad):
        return base.reshape(B, N)
    return disp_layered[:, :, 0, 0]


class _FirstColumn(torch.autograd.Function):
    """``dense[..., 0]`` of a [B,N,H,W] map that is constant along x by the caller's promise (``row_uniform``: xy and xz
    planes, networks/depth_decoder.py:153-181) -> contiguous [B,N,H].

    Backward: the row's gradient goes back as ``g / W`` on EVERY column, as an expanded (stride-0) view — whatever built
    the map from x-independent quantities (the decoder's ``expand`` / its y-grid formula) sums over x and receives exactly
    ``g``.  A plain ``dense[..., 0]`` hands autograd a SelectBackward that zero-fills a [B,N,H,W] tensor per step to carry one
    column (248 MB at 8x63x192x640: 0.037 ms next to a 0.38 ms path) and makes that expand-backward read it all."""

    @staticmethod
    def forward(ctx, dense):
        ctx.W = dense.shape[-1]
        return dense[..., 0].contiguous()

    @staticmethod
    def backward(ctx, g):
        return (g * (1.0 / ctx.W)).unsqueeze(-1).expand(*g.shape, ctx.W)


def _row_view(t, B, N, H, W, name="disp_layered"):
    """Is ``t`` a ROW VIEW: a [B,N,H,W] tensor with ``stride(3) == 0`` (and W > 1) that is not an H/W-expanded view of per-plane
    scalars — what ``ops.plane_geometry`` returns for ``disp_layered`` / ``padding_mask``, or any tensor with those strides (a
    batch slice ``view[:B]`` included).  Such a tensor IS constant along x, by construction: the row kernels take it with no
    ``row_uniform`` promise and no check of the data.  A stride-0 view of another shape raises ``ValueError``."""
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[3] <= 1 or t.stride(3) != 0 or (t.stride(2) == 0 and t.shape[2] > 1):
        return False
    if tuple(t.shape) != (B, N, H, W):
        raise ValueError("%s is a row view (stride(3) == 0) of shape %s, expected %s" % (name, tuple(t.shape), (B, N, H, W)))
    return True


def _rows_of(view):
    """The [B,N,H] rows of a row view (``_row_view``).  A view made by ``ops.plane_geometry`` carries the rows tensor it was
    expanded from (``_pd_rows``): the consumer then hangs on that tensor's autograd node directly, and its gradient arrives
    [B,N,H]-sized — nothing is spread over W and summed again, and several consumers add up in [B,N,H].  Any other row view
    goes through ``_FirstColumn``: the row total comes back as ``g / W`` on every column, a stride-0 gradient."""
    rows = getattr(view, "_pd_rows", None)
    if (rows is not None and rows.data_ptr() == view.data_ptr() and tuple(rows.shape) == tuple(view.shape[:3])
            and rows.stride() == view.stride()[:3]):
        return rows
    if view.requires_grad and torch.is_grad_enabled():
        return _FirstColumn.apply(view)
    return view.detach()[..., 0]


class _RowView(torch.autograd.Function):
    """rows [B,N,H] -> the [B,N,H,W] view with ``stride(3) == 0`` (the reference's shape of ``outputs["disp_layered"]``, nothing
    [B,N,H,W]-sized behind it).  Backward: a gradient that is itself constant along x (``stride(3) == 0``: ``_FirstColumn``'s
    ``g / W`` on every column) gives ``W * g[..., 0]`` without touching W times as many elements; any other gradient — a foreign
    torch consumer of the view — is summed over x.  The package's own row consumers do not come through here at all
    (``_rows_of``)."""

    @staticmethod
    def forward(ctx, rows, W):
        ctx.W = int(W)
        ctx.set_materialize_grads(False)
        return rows.unsqueeze(-1).expand(*rows.shape, int(W))

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        if ctx.W > 1 and g.stride(-1) == 0:
            return g[..., 0] * float(ctx.W), None
        return g.sum(-1), None


def row_view(rows, W):
    """``_RowView`` + the ``_pd_rows`` tag ``_rows_of`` reads."""
    view = _RowView.apply(rows, W) if rows.requires_grad else rows.unsqueeze(-1).expand(*rows.shape, int(W))
    view._pd_rows = rows
    return view


def disp_operand(disp_layered, B, N, H, W, rows=True, promise=False, grad=True, row_views=True):
    """(form, what a kernel reads for it: [B,N], [B,N,H] or the [B,N,H,W] map).  PER_PLANE: an H/W-expanded view of per-plane
    scalars.  ROWS, where the caller's kernels take ``rows``: a row view (``_row_view``), or any other map under the caller's
    ``promise`` that it is constant along x (``row_uniform``).  ``row_views=False``: a consumer without a row form, which never
    asks ``_row_view``.  With ``grad`` the operand keeps the cheapest autograd path — ``_per_plane_view``; ``_rows_of``; for a
    promise ``_FirstColumn``, or the plain select of a LEAF map (the exact select gradient: g on column 0, zeros elsewhere);
    without (forward-only consumers) it is contiguous."""
    view = row_views and _row_view(disp_layered, B, N, H, W)
    if not view and tuple(disp_layered.shape) != (B, N, H, W):
        disp_layered = disp_layered.expand(B, N, H, W)
    if not view and disp_layered.stride(2) == 0 and disp_layered.stride(3) == 0:
        return PER_PLANE, _per_plane_view(disp_layered) if grad else disp_layered[:, :, 0, 0].contiguous()
    if not (rows and (view or promise)):
        return DENSE, disp_layered if grad else disp_layered.contiguous()
    if not grad:
        return ROWS, disp_layered[..., 0].contiguous()
    if view:
        return ROWS, _rows_of(disp_layered)
    return ROWS, disp_layered[..., 0].contiguous() if disp_layered.is_leaf else _FirstColumn.apply(disp_layered)


def mask_operand(padding_mask, B, N, H, W, rows=True, promise=False, row_views=True):
    """(ROWS, fp32 [B,N,H]) or (DENSE, fp32 [B,N,H,W]).  A row view goes in as its first column where the caller's kernels take
    ``rows`` — detached, with no copy when it is fp32 (the sweep and a linked decoder tail then hold ONE ``data_ptr``), widened
    AFTER the column is taken.  Any other mask is widened BEFORE the expand (nothing broadcast is materialised) and gives its first
    column only under the caller's ``promise`` that it is constant along x.  ``row_views`` as in ``disp_operand``."""
    if row_views and _row_view(padding_mask, B, N, H, W, "padding_mask"):
        if rows:
            padding_mask = padding_mask.detach()[..., 0]
        return (ROWS if rows else DENSE), (padding_mask if padding_mask.dtype == torch.float32 else padding_mask.float())
    if padding_mask.dtype != torch.float32:
        padding_mask = padding_mask.float()
    if tuple(padding_mask.shape) != (B, N, H, W):
        padding_mask = padding_mask.expand(B, N, H, W)
    return (ROWS, padding_mask[..., 0]) if rows and promise else (DENSE, padding_mask)
