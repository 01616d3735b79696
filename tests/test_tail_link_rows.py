"""The tail link on the row form (pd_plane_sweep_bwd_tail_rows): with ``fuse_sweep_backward=True`` and row-view disparities
and / or a row-view padding mask — xy + xz planes as ``ops.plane_geometry`` returns them — the row-stream backward applies the
decoder tail's backward and the tail's own backward kernel does not run.

Modelled on test_sweep_backward_applies_the_fused_decoder_tail (tests/test_gpu_parity.py): the trainer-shaped objective
(photometric mean + weights on rgb_rec, disp, depth) through the patched ``pred_novel_images``, and the same three-way comparison
with its tolerances — fused against unfused on the GPU < 5e-6, each against CPU autograd through ``oracle.decoder_tail`` +
``oracle.warp_and_loss`` on the dense mask and map < 1e-4 — of g_raw_logits, g_raw_sigma and the gradient that reaches the plane
residual (or the rows tensor / the per-plane levels).

Measured on an MI355X (max |a - b| / max |b|; fused vs unfused | unfused vs oracle | fused vs oracle), worst of the three
gradients: see profiles/operator_parity.md, "Tail link on the row form"."""
import types

import pytest
import torch

from cases import rel_err
from planedepth_amd import ops, synthetic
from planedepth_amd.decoder_tail import fused_decoder_tail, fused_plane_geometry

pytestmark = pytest.mark.gpu
TOL = 1e-4        # against the oracle (the suite's tolerance)
TOL_FUSED = 5e-6  # fused against unfused
DEV = "cuda"
XZ = dict(xz_min=0.1852, xz_max=0.3704)


def C_auto_row_eps():
    from planedepth_amd import _capi as C
    return float(C.load().pd_sweep_auto_row_eps())


def make_opt(xz_levels):
    return types.SimpleNamespace(warp_type="disp_warp", match_aug=False, use_mixture_loss=True, automask=False,
                                 render_probability=False, alpha_pc=0.0, alpha_self=0.0, self_distillation=0.0,
                                 gamma_smooth=2.0, alpha_smooth=0.0, use_ssim=False, xz_levels=xz_levels, yz_levels=0)


class Case:
    """Inputs of one case on the CPU + how its plane tensors are built from the leaf ``p`` on either device.
    ``build(p, dev, dense)`` -> (disp_layered, padding_mask | None): row views (or the per-plane expand) for the product, the dense
    [B,N,H,W] tensors for the oracle."""

    def __init__(self, shape, side, seed, leaf, build, xz_levels, sigma_bounds=False):
        B, N, H, W = self.shape = shape
        g = torch.Generator().manual_seed(seed)
        self.side, self.leaf, self.build, self.xz_levels = side, leaf, build, xz_levels
        self.rl = torch.randn(B, N, H, W, generator=g) * 2.5
        self.rs = torch.randn(B, N, H, W, generator=g) * 3 - 1
        if sigma_bounds:
            self.rs[:, :, :, :40] = -9.0      # sigmoid = 1.2e-4: clamped to 0.01, gate closed
            self.rs[:, :, :, 40:80] = 30.0    # sigmoid = 1.0 exactly: on the upper bound, sigmoid' = 0
        self.col_l, self.col_t = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
        self.gw = [torch.randn(B, 3, H, W, generator=g) * 1e-3, torch.randn(B, 1, H, W, generator=g) * 1e-2,
                   torch.randn(B, 1, H, W, generator=g) * 1e-3]
        self.K, self.inv_K = synthetic.intrinsics(B, H, W)

    def objective(self, ph, rgb, disp, depth, dev):
        gw = self.gw
        return ph + (rgb * gw[0].to(dev)).sum() + (disp * gw[1].to(dev)).sum() + (depth * gw[2].to(dev)).sum()


def run_gpu(c, fuse, expect_link=True, early_disp=False, passes=1):
    """The product path.  Returns the three gradients (and the link)."""
    B, N, H, W = c.shape
    a, s, p = (t.to(DEV).clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
    dl, pm = c.build(p, DEV, False)
    outputs = {"disp_layered": dl, "padding_mask": pm}
    fused_decoder_tail(outputs, a, s, use_mixture_loss=True, all_ones_mask=pm is None, fuse_sweep_backward=fuse)
    link = getattr(outputs["logits"], "_pd_tail_link", None)
    early = outputs["disp"]                                      # taken BEFORE pred_novel_images installs the taps
    inputs = {("color", "l"): c.col_l.to(DEV), "K": c.K.to(DEV), "inv_K": c.inv_K.to(DEV)}
    if c.side != "l":
        inputs[("color", c.side)] = c.col_t.to(DEV)
    from gpu_cases import make_stub_trainer
    trainer = make_stub_trainer(make_opt(c.xz_levels if pm is not None else 0), [c.side])
    ops.KERNEL_EVENTS = {"fwd": [], "bwd": []}
    try:
        trainer.pred_novel_images(inputs, outputs)
        obj = c.objective(outputs[("ph_mean", c.side)], outputs[("rgb_rec", c.side)], early if early_disp else outputs["disp"],
                          outputs["depth"], DEV)
        grads = []
        for i in range(passes):
            for t in (a, s, p):
                t.grad = None
            obj.backward(retain_graph=i + 1 < passes)
            grads.append({k: v.grad.detach().cpu() for k, v in (("g_raw_logits", a), ("g_raw_sigma", s), ("g_plane", p))})
        tail_launches = len(ops.KERNEL_EVENTS.get("tail_bwd", []))
    finally:
        ops.KERNEL_EVENTS = None
    assert (link is not None) == (fuse and expect_link)
    if link is not None and not early_disp:
        assert link.fused_passes == passes and link.applied is None and not link.seen   # applied by the sweep, consumed by the tail's node
        assert tail_launches == 0, "the tail's own backward kernel ran although the sweep applied it"
    elif link is None:
        assert tail_launches == passes
    return (grads[0] if passes == 1 else grads), link


def run_cpu(c):
    """Autograd through the oracle's decoder tail + warp_and_loss on the dense mask and map."""
    from oracle import planedepth_oracle as orc
    B, N, H, W = c.shape
    a, s, p = (t.clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
    dl, pm = c.build(p, "cpu", True)
    pm = torch.ones(B, N, H, W) if pm is None else pm
    # (an absurd disparity at a masked element: the reference multiplies it by a zero probability; the warp's grid there only has
    # to be finite, so the oracle's warp sees it clamped — the mask removes the element either way)
    o = orc.decoder_tail(a, s, pm, dl, W, use_mixture_loss=True)
    r = orc.warp_and_loss(c.col_l, c.col_l if c.side == "l" else c.col_t, o["logits"], o["sigma"], warp_type="disp_warp",
                          target_side=c.side, disp_layered=dl.clamp(max=1e6), padding_mask=pm, distance=None, norm=None,
                          T=torch.eye(4)[None].repeat(B, 1, 1), K=c.K, inv_K=c.inv_K, use_mixture_loss=True, automask=False)
    c.objective(r["ph_loss"], r["rgb_rec"], o["disp"], o["depth"], "cpu").backward()
    return {"g_raw_logits": a.grad, "g_raw_sigma": s.grad, "g_plane": p.grad}


def three_way(c, name):
    plain, _ = run_gpu(c, False)
    fused, link = run_gpu(c, True)
    want = run_cpu(c)
    for k in want:
        e = (rel_err(fused[k], plain[k]), rel_err(plain[k], want[k]), rel_err(fused[k], want[k]))
        print("%s %s: fused vs unfused %.2e | unfused vs oracle %.2e | fused vs oracle %.2e" % ((name, k) + e))
    for k in want:
        assert torch.isfinite(fused[k]).all() and torch.isfinite(plain[k]).all(), k
        assert rel_err(fused[k], plain[k]) < TOL_FUSED, (k, "fused vs unfused", rel_err(fused[k], plain[k]))
        assert rel_err(plain[k], want[k]) < TOL, (k, "unfused vs oracle", rel_err(plain[k], want[k]))
        assert rel_err(fused[k], want[k]) < TOL, (k, "fused vs oracle", rel_err(fused[k], want[k]))
    return plain, fused, link


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def geometry_case(shape, split, crop, side, seed):
    """xy + xz planes from a crop grid and a plane residual: ``ops.plane_geometry`` for the product, the dense torch formulation
    of the same geometry for the oracle.  The leaf is the residual [B,N]."""
    B, N, H, W = shape
    nl, nx = split
    grid = synthetic.crop_grid(H, W, *crop)[None].repeat(B, 1, 1, 1)
    cfg = dict(no_levels=nl, xz_levels=nx, disp_min=2.0, disp_max=0.3 * W, **XZ)
    g = torch.Generator().manual_seed(seed + 1000)
    residual = torch.rand(B, N, generator=g) - 0.5

    def build(p, dev, dense):
        if dense:
            geo = synthetic.decoder_plane_geometry(grid.to(dev), p, **cfg)
            return geo["disp_layered"], geo["padding_mask"]
        outputs = fused_plane_geometry({}, grid.to(dev), p, **cfg)
        return outputs["disp_layered"], outputs["padding_mask"]
    return Case(shape, side, seed, residual, build, nx)


def hand_built_rows(mask, rows_disp):
    """[2,7,9,256]: sigma on both clamp bounds, one (n, y) with an integer disparity (the irregular path, whose rows start from
    the tail's own term), one plane masked on some rows with an absurd disparity there.  ``mask`` / ``rows_disp``: the mixed forms
    (rows with no mask; per-plane disparities with a row mask)."""
    B, N, H, W = shape = (2, 7, 9, 256)
    g = torch.Generator().manual_seed(77)
    lv = 0.3 * W * (2.0 / (0.3 * W)) ** ((torch.arange(N, dtype=torch.float32)[None, :, None] + torch.rand(B, N, 1, generator=g) - 0.5)
                                         / (N - 1))
    m = torch.ones(B, N, H)
    m[:, 5, :4] = 0.0      # the horizon of a ground plane: masked above it
    m[1, 2, 6:] = 0.0
    if rows_disp:
        leaf = (lv * (1.0 + 0.03 * torch.arange(H, dtype=torch.float32)[None, None, :])).contiguous()   # [B,N,H]: grows with the row
        leaf[:, 3, 4] = 17.0                 # an integer shift on one (n, y): the irregular path
        if mask:
            leaf[:, 5, :4] = 1e30            # absurd where the plane is masked
    else:
        leaf = lv[:, :, :, None].contiguous()   # [B,N,1,1]
        leaf[:, 3] = 17.0

    def build(p, dev, dense):
        mm = m.to(dev)
        if rows_disp:
            dl = p[..., None].expand(B, N, H, W) if dense else ops.row_view(p, W)
        else:
            dl = p.expand(B, N, H, W)
        if not mask:
            return dl, None
        return dl, (mm[..., None].expand(B, N, H, W).contiguous() if dense else ops.row_view(mm, W))
    return Case(shape, "r", 78, leaf, build, 3, sigma_bounds=True), m


def two_source_rows(H):
    """How many target rows of an H-row image blend two source rows (the vertical round trip of trainer.py:552 + grid_sample is
    inexact there: the NROWS = 2 body of the row kernels), by the library's own row selection (pd_debug_fwd_row_groups, as
    tests/test_row_groups.py reads it)."""
    import ctypes
    import numpy as np
    from planedepth_amd import _capi as C
    fn = C.load().pd_debug_fwd_row_groups
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    out = np.full(((H + 2) // 3) * 3, 0xFFFF, dtype=np.uint16)
    links, cut = ctypes.c_int(0), ctypes.c_int(0)
    fn(H, 3, 0.0, out.ctypes.data, ctypes.byref(links), ctypes.byref(cut))
    return links.value


def test_geometry_route():
    """Rows above and below the horizon of the ground planes, and both row kinds — rows that read one source row and rows that
    blend two — at the height test_plane_geometry's residual test uses (the window of synthetic.crop_grid(H, W, 60, 200, 11, 37)
    there; the resized image is 400 wide here so that a 256-pixel window fits)."""
    c = geometry_case((2, 7, 24, 256), (4, 3), (60, 400, 11, 37), "r", 1)
    assert 0 < two_source_rows(24) < 24                                            # both the NROWS = 1 and the NROWS = 2 body run
    assert ops.SWEEP_IMPL == 0 and C_auto_row_eps() == 0.0                         # ... and no second source row is dropped
    _, pm = c.build(c.leaf.to(DEV), DEV, False)
    rows = ops._rows_of(pm)
    assert set(rows.unique().tolist()) == {0.0, 1.0}                               # the mask rows hold zeros and ones
    xz = rows[:, 4:]
    assert bool((xz == 0).all(1).any()) and bool((xz == 1).all(1).any())           # rows above and rows below the horizon
    plain, fused, link = three_way(c, "geometry_route")
    assert link.mask_rows is not None
    dead = (rows == 0).cpu()[..., None].expand(-1, -1, -1, 256)
    assert float(fused["g_raw_logits"][dead].abs().max()) == 0.0 and float(fused["g_raw_sigma"][dead].abs().max()) == 0.0


def test_every_segment_count_with_negative_shifts():
    """49 + 14 planes, target "l" (negative shifts: the epilogue's x0 = -1 targets), W = 640 (five segments), the horizon inside
    the crop."""
    c = geometry_case((1, 63, 12, 640), (49, 14), (40, 900, 14, 130), "l", 2)
    _, pm = c.build(c.leaf.to(DEV), DEV, False)
    rows = ops._rows_of(pm)[:, 49:]
    assert bool((rows == 0).any()) and bool((rows == 1).any())
    three_way(c, "every_segment_count_left_view")


def test_hand_built_rows_clamp_bounds_integer_shift_and_absurd_masked_disparity():
    c, m = hand_built_rows(mask=True, rows_disp=True)
    plain, fused, link = three_way(c, "hand_built_rows")
    B, N, H, W = c.shape
    dead = (m == 0)
    for res in (plain, fused):
        for k in ("g_raw_logits", "g_raw_sigma"):
            assert torch.isfinite(res[k]).all()
            assert float(res[k][dead[..., None].expand(B, N, H, W)].abs().max()) == 0.0, k   # exact zeros by selection
        assert torch.isfinite(res["g_plane"]).all()
    # the tail's share of the masked rows' disparity gradient is an exact zero as well (the warp's is: the plane is out of view)
    assert float(fused["g_plane"][dead].abs().max()) == 0.0


@pytest.mark.parametrize("form", ["rows_no_mask", "per_plane_row_mask"])
def test_mixed_forms(form):
    c, m = hand_built_rows(mask=form == "per_plane_row_mask", rows_disp=form == "rows_no_mask")
    _, fused, link = three_way(c, form)
    assert (link.mask_rows is None) == (form == "rows_no_mask")
    if form == "per_plane_row_mask":
        B, N, H, W = c.shape
        dead = (m == 0)[..., None].expand(B, N, H, W)
        assert float(fused["g_raw_logits"][dead].abs().max()) == 0.0 and float(fused["g_raw_sigma"][dead].abs().max()) == 0.0


@pytest.mark.parametrize("form", ["dense_map", "per_pixel_mask"])
def test_dense_forms_take_no_link(form):
    """A dense map or a per-pixel mask with the flag set: no link, the unfused results."""
    c, m = hand_built_rows(mask=True, rows_disp=True)
    build = c.build

    def dense(p, dev, _):
        dl, pm = build(p, dev, False)
        if form == "dense_map":
            return p[..., None].expand(*c.shape).contiguous(), pm
        return dl, pm.contiguous()
    want, _ = run_gpu(c, False)
    c.build = dense
    c.xz_levels = 3
    got, link = run_gpu(c, True, expect_link=False)
    assert link is None
    for k in want:
        assert rel_err(got[k], want[k]) < TOL_FUSED, (k, rel_err(got[k], want[k]))


def test_a_second_sweep_on_the_same_logits_switches_the_fusion_off():
    c, _ = hand_built_rows(mask=True, rows_disp=True)
    B, N, H, W = c.shape
    res = {}
    for fuse in (False, True):
        a, s, p = (t.to(DEV).clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
        dl, pm = c.build(p, DEV, False)
        logits, sigma, disp, depth, _ = ops.decoder_tail(a, s, pm, dl, fuse_sweep_backward=fuse)
        link = getattr(logits, "_pd_tail_link", None)
        assert (link is not None) == fuse
        ops.KERNEL_EVENTS = {"fwd": [], "bwd": []}
        try:
            m1 = ops.plane_sweep_disp(c.col_l.to(DEV), c.col_t.to(DEV), logits, sigma, dl, pm, return_mean=True)[2]
            m2 = ops.plane_sweep_disp(c.col_l.to(DEV), c.col_t.to(DEV), logits, sigma, dl, pm, target_side="l", return_mean=True)[2]
            (m1 + m2 + (disp * c.gw[1].to(DEV)).sum()).backward()
            tail_launches = len(ops.KERNEL_EVENTS.get("tail_bwd", []))
        finally:
            ops.KERNEL_EVENTS = None
        if fuse:
            assert link.consumers == 2 and link.fused_passes == 0
        assert tail_launches == 1
        res[fuse] = [t.grad.cpu() for t in (a, s, p)]
    for x, y in zip(res[False], res[True]):
        assert rel_err(y, x) < TOL_FUSED, rel_err(y, x)


def test_a_mask_the_tail_did_not_see_is_an_unserved_consumer():
    """The sweep's row mask must be the tail's: another [B,N,H] tensor (equal values, other memory) is not fused."""
    c, m = hand_built_rows(mask=True, rows_disp=True)
    B, N, H, W = c.shape
    a, s, p = (t.to(DEV).clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
    dl, pm = c.build(p, DEV, False)
    logits, sigma, disp, depth, _ = ops.decoder_tail(a, s, pm, dl, fuse_sweep_backward=True)
    link = logits._pd_tail_link
    ops.plane_sweep_disp(c.col_l.to(DEV), c.col_t.to(DEV), logits, sigma, dl, ops.row_view(m.to(DEV).clone(), W), return_mean=True)
    assert link.consumers == 2
    logits, sigma, disp, depth, _ = ops.decoder_tail(a, s, pm, dl, fuse_sweep_backward=True)
    ops.plane_sweep_disp(c.col_l.to(DEV), c.col_t.to(DEV), logits, sigma, dl, None, return_mean=True)
    assert logits._pd_tail_link.consumers == 2


def test_disparities_the_tail_did_not_see_are_an_unserved_consumer():
    """The fused kernel reads the tail's disparities from the sweep's argument: a tail fed a row view and a sweep fed a dense
    ``row_uniform`` copy of it (other memory) are not fused, and the gradients are the unfused ones."""
    c, m = hand_built_rows(mask=True, rows_disp=True)
    B, N, H, W = c.shape
    res = {}
    for fuse in (False, True):
        a, s, p = (t.to(DEV).clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
        dl, pm = c.build(p, DEV, False)
        logits, sigma, disp, depth, _ = ops.decoder_tail(a, s, pm, dl, fuse_sweep_backward=fuse)
        dense = p[..., None].expand(B, N, H, W).clamp(max=1e30).contiguous()      # equal values, other memory, no row view
        ph_mean = ops.plane_sweep_disp(c.col_l.to(DEV), c.col_t.to(DEV), logits, sigma, dense, pm, row_uniform=True, return_mean=True)[2]
        if fuse:
            link = logits._pd_tail_link
            assert link.disp_rows is not None and link.consumers == 2
        (ph_mean + (disp * c.gw[1].to(DEV)).sum()).backward()
        if fuse:
            assert link.fused_passes == 0
        res[fuse] = [t.grad.cpu() for t in (a, s, p)]
    for x, y in zip(res[False], res[True]):
        assert rel_err(y, x) < TOL_FUSED, rel_err(y, x)


def test_disp_consumed_before_the_taps_on_the_row_form():
    """The remainder path: a consumer that took ``disp`` before the taps existed delivers its gradient to the tail's node only; the
    tail's backward (row flags) then adds that remainder itself."""
    c, _ = hand_built_rows(mask=True, rows_disp=True)
    want, _ = run_gpu(c, False, early_disp=True)
    got, link = run_gpu(c, True, early_disp=True)
    assert link is not None and link.fused_passes == 1 and link.applied is None
    for k in want:
        assert rel_err(got[k], want[k]) < TOL_FUSED, (k, rel_err(got[k], want[k]))


def test_two_fused_backward_passes_over_a_retained_graph_are_identical():
    """Per-row disparities: every sum of the fused kernel has one owner and one order (no float atomics into g_plane [B,N,H])."""
    c = geometry_case((2, 7, 24, 256), (4, 3), (60, 400, 11, 37), "r", 1)
    (first, second), link = run_gpu(c, True, passes=2)
    assert link.fused_passes == 2
    for k in first:
        assert torch.equal(first[k], second[k]), k
