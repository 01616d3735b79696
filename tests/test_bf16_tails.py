"""bf16 conv outputs through the fused decoder tails (PD_TAIL_BF16) on the GPU: the bf16 kernels against the fp32 route on the
widened inputs and against the oracle, the dtype rule, the trainer under torch.autocast with the tail as the sweep's producer,
and the post-process on a teacher's bf16 logits."""
import types

import pytest
import torch

from cases import rel_err
from planedepth_amd import _capi as C
from planedepth_amd import _state as S
from planedepth_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
TOL = 1e-4   # tests/test_gpu_parity.py: the fp32 outputs against the oracle


def _ulp_dist(a, b):
    """bf16 bit-pattern distance, +0 == -0."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def _rounded_once(name, got, want32):
    """``got`` (bf16) is ``want32`` rounded once: within 1 bf16 ulp, and at most 1e-4 of the elements differ at all."""
    assert got.dtype == BF, (name, got.dtype)
    d = _ulp_dist(got, want32.to(BF))
    assert int(d.max()) <= 1, (name, int(d.max()))
    assert int((d != 0).sum()) <= 1e-4 * d.numel(), (name, int((d != 0).sum()), d.numel())


def _close_f32(name, got, want, rel):
    assert got.dtype == torch.float32, (name, got.dtype)
    scale = float(want.abs().max()) or 1.0
    err = float((got - want).abs().max())
    assert err <= rel * scale, (name, err, scale, int((got != want).sum()))


def _near_rounded(name, got, want32, tol_abs):
    """A bf16 output against the oracle's fp32 value rounded to bf16.  If the fp32 values behind both are within ``tol_abs``,
    rounding each to nearest moves it by at most half a bf16 spacing, 2^-8 of its magnitude: the rounded values are within
    tol_abs + 2^-8 (|a| + |b|) <= 1.01 tol_abs + 2^-7 |want32| of each other, element by element."""
    assert got.dtype == BF, (name, got.dtype)
    w = want32.to(got.device)
    excess = (got.float() - w.to(BF).float()).abs() - (1.01 * tol_abs + w.abs() * 2.0 ** -7)
    assert float(excess.max()) <= 0.0, (name, float(excess.max()), tol_abs)


def _bf16_leafable(t, offset):
    """t rounded to bf16 on the device; ``offset``: as a contiguous view that starts one element (2 bytes) into its storage, which
    breaks the 8-byte alignment of the four-pixel form."""
    t = t.to(DEV).to(BF)
    if not offset:
        return t
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=BF)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 8 == 2
    return v


def _mask(B, N, H, W):
    """0/1 mask in the shape xz planes give it: the last quarter of the planes is out of view in the upper half of the image."""
    pm = torch.ones(B, N, H, W, device=DEV)
    pm[:, max(1, N - N // 4):, :H // 2] = 0.0
    return pm


def _raw_sigma(shape, g):
    rs = torch.randn(*shape, generator=g) * 3 - 1
    flat = rs.view(-1)
    flat[0::7] = -12.0    # sigmoid = 6e-6: clamped to 0.01, gate closed
    flat[1::7] = 12.0     # sigmoid = 0.999994: just inside, gate open
    flat[2::11] = 30.0    # sigmoid = 1.0 exactly: on the upper bound, sigmoid' = 0
    return rs


def _gate_closed(rs):
    return (rs.float() <= -12.0) | (rs.float() >= 30.0)


def _levels(B, N, W, g):
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(B, N, 1, 1, generator=g) - 0.5
    return (300.0 * (W / 640.0) * (2.0 / 300.0) ** (lv / max(N - 1, 1))).to(DEV)


def _disp_leaf(lv, H, W, dense, g_seed):
    """(leaf, disp_layered): the decoder's expanded view of per-plane levels, or a dense map (levels times a per-row gain)."""
    if not dense:
        leaf = lv.clone().requires_grad_(True)
        return leaf, leaf.expand(-1, -1, H, W)
    g = torch.Generator().manual_seed(g_seed)
    gain = (1.0 + 0.2 * torch.rand(1, 1, H, 1, generator=g)).to(DEV)
    leaf = (lv * gain).expand(-1, -1, H, W).contiguous().requires_grad_(True)
    return leaf, leaf


def _decoder_route(rl_b, rs_b, pm, lv, ups, mix, dense, widen):
    """ops.decoder_tail forward + backward on the bf16 tensors as they are, or (``widen``) on their exact fp32 copies."""
    B, N, H, W = rl_b.shape
    cast = (lambda t: t.float()) if widen else (lambda t: t)
    a = cast(rl_b).detach().requires_grad_(True)
    s = cast(rs_b).detach().requires_grad_(True) if mix else None
    leaf, dl = _disp_leaf(lv, H, W, dense, 77)
    logits, sigma, disp, depth, layers = ops.decoder_tail(a, s, pm, dl, use_mixture_loss=mix)
    gl, gs, gd, gz = ups
    outs, grads = [logits, disp, depth], [cast(gl), gd, gz]
    if mix:
        outs.append(sigma)
        grads.append(cast(gs))
    torch.autograd.backward(outs, grads)
    return dict(a=a, logits=logits.detach(), sigma=sigma.detach() if mix else None, disp=disp.detach(), depth=depth.detach(),
                stash=layers.stash, layers=layers, g_rl=a.grad, g_rs=s.grad if mix else None, g_dl=leaf.grad)


def _decoder_case(shape, mix, mask, dense, offset=False, seed=0):
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    rl_b = _bf16_leafable(torch.randn(B, N, H, W, generator=g) * 2.5, offset)
    rs_b = _bf16_leafable(_raw_sigma(shape, g), offset)
    pm = _mask(B, N, H, W) if mask else None
    lv = _levels(B, N, W, g)
    ups = (torch.randn(B, N, H, W, generator=g).to(DEV).to(BF), torch.randn(B, N, H, W, generator=g).to(DEV).to(BF),
           torch.randn(B, 1, H, W, generator=g).to(DEV), (torch.randn(B, 1, H, W, generator=g) * 0.1).to(DEV))
    return rl_b, rs_b, pm, lv, ups


DECODER_SHAPES = [("headline", (8, 49, 192, 640), False), ("n63", (2, 63, 192, 640), False), ("hw_not_4", (3, 5, 7, 13), False),
                  ("offset", (2, 6, 8, 16), True), ("one_plane", (4, 1, 8, 16), False)]


@pytest.mark.parametrize("dense", [False, True], ids=["per_plane", "dense"])
@pytest.mark.parametrize("mask", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("tag,shape,offset", DECODER_SHAPES, ids=[s[0] for s in DECODER_SHAPES])
def test_decoder_tail_bf16_equals_fp32_route_rounded_once(tag, shape, offset, mix, mask, dense):
    rl_b, rs_b, pm, lv, ups = _decoder_case(shape, mix, mask, dense, offset)
    got = _decoder_route(rl_b, rs_b, pm, lv, ups, mix, dense, widen=False)
    want = _decoder_route(rl_b, rs_b, pm, lv, ups, mix, dense, widen=True)
    assert want["logits"].dtype == torch.float32 and want["g_rl"].dtype == torch.float32
    for k in ("disp", "depth", "stash"):
        _close_f32(k, got[k], want[k], 1e-6)
    if mix:
        _rounded_once("sigma", got["sigma"], want["sigma"])
        assert float(got["sigma"].float().min()) >= 0.01   # never below the sweep's clamp
    assert got["logits"].dtype == BF
    if mask:
        assert torch.equal(got["logits"].float(), rl_b.float() * pm)
    else:
        assert got["logits"].data_ptr() == got["a"].data_ptr()   # still the view of the conv output
    _rounded_once("g_raw_logits", got["g_rl"], want["g_rl"])
    if mix:
        _rounded_once("g_raw_sigma", got["g_rs"], want["g_rs"])
        closed = _gate_closed(rs_b)
        assert int(closed.sum()) > 0
        assert bool((got["g_rs"][closed] == 0).all()) and bool((want["g_rs"][closed] == 0).all())
        assert bool((got["g_rs"][~closed] != 0).any())
    _close_f32("g_disp_layered", got["g_dl"], want["g_dl"], 1e-5)


def _plade_route(rl_b, rs_b, lv, ups, mix, dense, widen):
    B, N, H, W = (rs_b.shape if rs_b is not None else (rl_b.shape[0], rl_b.shape[1] + 1) + tuple(rl_b.shape[2:]))
    cast = (lambda t: t.float()) if widen else (lambda t: t)
    a = cast(rl_b).detach().requires_grad_(True)
    s = cast(rs_b).detach().requires_grad_(True) if mix else None
    leaf, dl = _disp_leaf(lv, H, W, dense, 78)
    logits, dists, sigma, disp, depth, layers = ops.plade_tail(a, s, dl, use_mixture_loss=mix)
    gl, gs, gt, gd, gz = ups
    outs, grads = [logits, dists, disp, depth], [cast(gl), gt, gd, gz]
    if mix:
        outs.append(sigma)
        grads.append(cast(gs))
    torch.autograd.backward(outs, grads)
    return dict(logits=logits.detach(), dists=dists.detach(), sigma=sigma.detach() if mix else None, disp=disp.detach(),
                depth=depth.detach(), layers=layers, g_rl=a.grad, g_rs=s.grad if mix else None, g_dl=leaf.grad)


def _plade_case(shape, seed=0):
    B, N, H, W = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    rl_b = (torch.randn(B, N - 1, H, W, generator=g) * 1.5).to(DEV).to(BF)
    rs_b = _raw_sigma(shape, g).to(DEV).to(BF)
    lv = _levels(B, N, W, g)
    ups = (torch.randn(B, N, H, W, generator=g).to(DEV).to(BF), torch.randn(B, N, H, W, generator=g).to(DEV).to(BF),
           (torch.randn(B, N - 1, H, W, generator=g) * 0.05).to(DEV), torch.randn(B, 1, H, W, generator=g).to(DEV),
           (torch.randn(B, 1, H, W, generator=g) * 0.1).to(DEV))
    return rl_b, rs_b, lv, ups


@pytest.mark.parametrize("dense", [False, True], ids=["per_plane", "dense"])
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("shape", [(8, 49, 192, 640), (2, 49, 24, 80), (3, 9, 17, 33), (1, 2, 5, 7)])
def test_plade_tail_bf16_equals_fp32_route_rounded_once(shape, mix, dense):
    rl_b, rs_b, lv, ups = _plade_case(shape)
    got = _plade_route(rl_b, rs_b, lv, ups, mix, dense, widen=False)
    want = _plade_route(rl_b, rs_b, lv, ups, mix, dense, widen=True)
    assert got["dists"].dtype == torch.float32 and torch.equal(got["dists"], want["dists"])
    for k in ("disp", "depth"):
        _close_f32(k, got[k], want[k], 1e-6)
    assert got["logits"].dtype == BF
    assert torch.equal(got["logits"][:, :-1], rl_b) and bool((got["logits"][:, -1] == 1).all())
    if mix:
        _rounded_once("sigma", got["sigma"], want["sigma"])
    _rounded_once("g_raw_logits", got["g_rl"], want["g_rl"])
    if mix:
        _rounded_once("g_raw_sigma", got["g_rs"], want["g_rs"])
        closed = _gate_closed(rs_b)
        assert bool((got["g_rs"][closed] == 0).all())
    _close_f32("g_disp_layered", got["g_dl"], want["g_dl"], 1e-5)
    pi, prob = got["layers"]()
    pi32, prob32 = want["layers"]()
    _close_f32("pi", pi, pi32, 1e-6)
    _close_f32("probability", prob, prob32, 1e-6)


@pytest.mark.parametrize("mix,mask,shape", [(True, False, (2, 49, 24, 80)), (True, True, (2, 63, 20, 72)),
                                            (False, False, (3, 9, 17, 33))])
def test_decoder_tail_bf16_vs_oracle(mix, mask, shape):
    """The cases and the 1e-4 of tests/test_gpu_parity.py::test_decoder_tail_vs_oracle_per_plane_disparities, the oracle fed the
    widened bf16 inputs.  fp32 outputs: the same bound.  bf16 outputs: against the oracle's rounded to bf16, with the rounding of
    both sides allowed for (_near_rounded)."""
    from oracle import planedepth_oracle as orc
    B, N, H, W = shape
    g = torch.Generator().manual_seed(5 + N)
    rl = (torch.randn(B, N, H, W, generator=g) * 2.5).to(BF)
    rs = (torch.randn(B, N, H, W, generator=g) * 3 - 1).to(BF)
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(B, N, 1, 1, generator=g) - 0.5
    pm = (torch.rand(B, N, H, W, generator=g) > 0.2).float() if mask else None
    if mask:
        pm[:, :5] = 1.0  # never mask every plane of a pixel
    gw = [torch.randn(B, N, H, W, generator=g).to(BF), torch.randn(B, N, H, W, generator=g).to(BF),
          torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g) * 0.1]

    def run(device, fused):
        cast = (lambda t: t) if fused else (lambda t: t.float())
        a, s = (cast(t).to(device).clone().requires_grad_(True) for t in (rl, rs))
        l = lv.to(device).clone().requires_grad_(True)
        dl = (300.0 * (2.0 / 300.0) ** (l / (N - 1))).expand(-1, -1, H, W)
        m = None if pm is None else pm.to(device)
        if fused:
            logits, sigma, disp, depth, layers = ops.decoder_tail(a, s if mix else None, m, dl, use_mixture_loss=mix)
            prob = layers()[1]
        else:
            o = orc.decoder_tail(a, s, m if m is not None else torch.ones_like(a), dl, W, use_mixture_loss=mix)
            logits, sigma, disp, depth, prob = o["logits"], o.get("sigma"), o["disp"], o["depth"], o["probability"]
        outs, grads = [logits, disp, depth], [cast(gw[0]).to(device), gw[2].to(device), gw[3].to(device)]
        if mix:
            outs.append(sigma)
            grads.append(cast(gw[1]).to(device))
        torch.autograd.backward(outs, grads)
        res = dict(logits=logits, disp=disp, depth=depth, prob=prob, g_rl=a.grad, g_lv=l.grad)
        if mix:
            res.update(sigma=sigma, g_rs=s.grad)
        return {k: v.detach().cpu() for k, v in res.items()}

    got, want = run(DEV, True), run("cpu", False)
    for k in want:
        if k in ("logits", "sigma", "g_rl", "g_rs"):
            _near_rounded(k, got[k], want[k], TOL * float(want[k].abs().max()))
        else:
            assert got[k].dtype == torch.float32
            assert rel_err(got[k], want[k]) < TOL, (k, rel_err(got[k], want[k]))


@pytest.mark.parametrize("mix,shape", [(True, (2, 49, 24, 80)), (False, (3, 9, 17, 33)), (True, (1, 2, 5, 7))])
def test_plade_tail_bf16_vs_oracle(mix, shape):
    """The cases and bounds of tests/test_gpu_parity.py::test_plade_tail_vs_oracle_per_plane_disparities on the widened bf16 inputs:
    forward 1e-4 against the fp32 oracle, gradients three-way against its fp64 evaluation (e_got <= 2 e_ref + 1e-4).  A bf16
    gradient is compared with the fp32 oracle's rounded to bf16: its fp32 value is within (2 e_ref + 1e-4) max of the fp64 one and
    the fp32 oracle's within e_ref max, so the two are within (3 e_ref + 1e-4) max before both are rounded (_near_rounded)."""
    from oracle import planedepth_oracle as orc
    B, N, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    rl0 = (torch.randn(B, N - 1, H, W, generator=g) * 1.5).to(BF)
    rs0 = (torch.randn(B, N, H, W, generator=g) * 2.0).to(BF)
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(B, N, 1, 1, generator=g) - 0.5
    dl0 = 300.0 * (W / 640.0) * (2.0 / 300.0) ** (lv / max(N - 1, 1))
    gws = [torch.randn(B, N, H, W, generator=g).to(BF), torch.randn(B, N - 1, H, W, generator=g) * 0.05,
           torch.randn(B, N, H, W, generator=g).to(BF), torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g) * 0.1]

    def run(device, dtype, fused):
        st = BF if fused else dtype
        rl, rs = (t.detach().clone().to(device=device, dtype=st).requires_grad_(True) for t in (rl0, rs0))
        d0 = dl0.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
        dl = d0.expand(-1, -1, H, W)
        if fused:
            logits, dists, sigma, disp, depth, _ = ops.plade_tail(rl, rs if mix else None, dl, use_mixture_loss=mix)
            o = dict(logits=logits, dists=dists, sigma=sigma, disp=disp, depth=depth)
        else:
            o = orc.plade_tail(rl, rs if mix else None, dl, W, orc.camera_ray_norm(H, W, dtype), mix)
        w = [gws[0].to(device=device, dtype=st), gws[1].to(device=device, dtype=dtype), gws[2].to(device=device, dtype=st),
             gws[3].to(device=device, dtype=dtype), gws[4].to(device=device, dtype=dtype)]
        outs, grads = [o["logits"], o["dists"], o["disp"], o["depth"]], [w[0], w[1], w[3], w[4]]
        if mix:
            outs.append(o["sigma"])
            grads.append(w[2])
        torch.autograd.backward(outs, grads)
        res = {k: o[k].detach().cpu() for k in ("logits", "dists", "disp", "depth") + (("sigma",) if mix else ())}
        res.update(g_raw_logits=rl.grad.cpu(), g_disp_pp=d0.grad.cpu())
        if mix:
            res["g_raw_sigma"] = rs.grad.cpu()
        return res

    got, want, exact = run(DEV, torch.float32, True), run("cpu", torch.float32, False), run("cpu", torch.float64, False)
    for k in want:
        scale = float(exact[k].abs().max())
        e_ref = rel_err(want[k], exact[k])
        if k in ("g_raw_logits", "g_raw_sigma"):
            _near_rounded(k, got[k], want[k], (3.0 * e_ref + TOL) * scale)
        elif k in ("logits", "sigma"):
            _near_rounded(k, got[k], want[k], TOL * float(want[k].abs().max()))
        elif k.startswith("g_"):
            assert got[k].dtype == torch.float32
            assert rel_err(got[k], exact[k]) <= 2.0 * e_ref + TOL, (k, rel_err(got[k], exact[k]), e_ref)
        else:
            assert got[k].dtype == torch.float32
            assert rel_err(got[k], want[k]) < TOL, (k, rel_err(got[k], want[k]))


@pytest.mark.parametrize("mask", [False, True], ids=["no_mask", "mask"])
def test_layers_are_fp32_and_equal_the_fp32_routes(mask):
    from planedepth_amd.decoder_tail import fused_decoder_tail, LazyLayers
    shape = (2, 9, 24, 80)
    B, N, H, W = shape
    rl_b, rs_b, pm, lv, _ = _decoder_case(shape, True, mask, False)
    dl = lv.expand(-1, -1, H, W)
    with torch.no_grad():
        _, _, _, _, layers = ops.decoder_tail(rl_b, rs_b, pm, dl)
        _, _, _, _, layers32 = ops.decoder_tail(rl_b.float(), rs_b.float(), pm, dl)
        (pi, prob), (pi32, prob32) = layers(), layers32()
        _close_f32("pi", pi, pi32, 1e-6)
        _close_f32("probability", prob, prob32, 1e-6)
        outputs = {"disp_layered": dl, "padding_mask": pm}
        fused_decoder_tail(outputs, rl_b, rs_b, use_mixture_loss=True, all_ones_mask=not mask)
        for k in ("probability", "pi"):
            assert isinstance(outputs[k], LazyLayers) and outputs[k].dtype is torch.float32
            assert outputs[k].tensor().dtype == torch.float32 and tuple(outputs[k].shape) == shape
        assert torch.equal(outputs["probability"].tensor(), prob)
        assert outputs["logits"].dtype == BF and outputs["sigma"].dtype == BF and outputs["disp"].dtype == torch.float32
        outputs = {"disp_layered": dl}
        from planedepth_amd.decoder_tail import fused_plade_tail
        fused_plade_tail(outputs, rl_b[:, :-1].contiguous(), rs_b)
        assert outputs["probability"].dtype is torch.float32 and outputs["pi"].tensor().dtype == torch.float32
        assert outputs["dists"].dtype == torch.float32 and outputs["logits"].dtype == BF


def test_dtype_rule():
    B, N, H, W = 2, 5, 8, 16
    g = torch.Generator().manual_seed(3)
    rl, rs = torch.randn(B, N, H, W, generator=g).to(DEV), torch.randn(B, N, H, W, generator=g).to(DEV)
    dl = _levels(B, N, W, g).expand(-1, -1, H, W)
    with pytest.raises(TypeError, match=r"bfloat16.*float32|float32.*bfloat16"):
        ops.decoder_tail(rl.to(BF), rs, None, dl)
    with pytest.raises(TypeError, match=r"bfloat16.*float32|float32.*bfloat16"):
        ops.plade_tail(rl[:, :-1].contiguous().to(BF), rs, dl)
    with pytest.raises(TypeError, match="float16"):
        ops.decoder_tail(rl.half(), rs.half(), None, dl)
    with pytest.raises(TypeError, match="float16"):
        ops.plade_tail(rl[:, :-1].contiguous().half(), rs.half(), dl)
    with pytest.raises(TypeError, match="float16"):
        ops.decoder_tail(rl.half(), None, None, dl, use_mixture_loss=False)
    with pytest.raises(TypeError):   # disp_layered stays fp32 only
        ops.decoder_tail(rl.to(BF), rs.to(BF), None, dl.to(BF))
    logits, sigma, disp, depth, layers = ops.decoder_tail(rl, rs, torch.ones_like(rl), dl)
    assert all(t.dtype == torch.float32 for t in (logits, sigma, disp, depth) + tuple(layers()))
    logits, dists, sigma, disp, depth, layers = ops.plade_tail(rl[:, :-1].contiguous(), rs, dl)
    assert all(t.dtype == torch.float32 for t in (logits, dists, sigma, disp, depth) + tuple(layers()))


def _opt(**kw):
    base = dict(warp_type="disp_warp", match_aug=False, use_mixture_loss=True, automask=False, render_probability=False,
                alpha_pc=0.0, alpha_self=0.0, self_distillation=0.0, gamma_smooth=2.0, alpha_smooth=0.04, use_ssim=True,
                xz_levels=0, yz_levels=0, materialize_layers=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _fuse_graph(shape, fuse, level_grad):
    """fused_decoder_tail(bf16, fuse_sweep_backward=fuse) -> pred_novel_images -> the trainer-shaped objective of
    tests/test_gpu_parity.py::test_sweep_backward_applies_the_fused_decoder_tail -> backward.  Returns (loss, bit patterns of the conv
    outputs' gradients, gradient of the plane levels or None)."""
    from gpu_cases import make_stub_trainer
    from planedepth_amd.decoder_tail import fused_decoder_tail
    from planedepth_amd.synthetic import intrinsics
    B, N, H, W = shape
    g = torch.Generator().manual_seed(321)
    rl = (torch.randn(B, N, H, W, generator=g) * 2.5).to(BF)
    rs = _raw_sigma((B, N, H, W), g).to(BF)
    lv = 0.3 * W * (2.0 / (0.3 * W)) ** ((torch.arange(N, dtype=torch.float32)[None, :, None, None] +
                                          torch.rand(B, N, 1, 1, generator=g) - 0.5) / (N - 1))
    col_l, col_t = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    gw = [torch.randn(B, 3, H, W, generator=g) * 1e-3, torch.randn(B, 1, H, W, generator=g) * 1e-2,
          torch.randn(B, 1, H, W, generator=g) * 1e-3]
    K, inv_K = intrinsics(B, H, W)
    a, s = (t.to(DEV).clone().requires_grad_(True) for t in (rl, rs))
    d = lv.to(DEV).clone().requires_grad_(level_grad)
    outputs = {"disp_layered": d.expand(-1, -1, H, W), "padding_mask": None}
    fused_decoder_tail(outputs, a, s, use_mixture_loss=True, all_ones_mask=True, fuse_sweep_backward=fuse)
    assert getattr(outputs["logits"], "_pd_tail_link", None) is None
    assert getattr(outputs["sigma"], "_pd_tail_link", None) is None
    inputs = {("color", "l"): col_l.to(DEV), ("color", "r"): col_t.to(DEV), "K": K.to(DEV), "inv_K": inv_K.to(DEV)}
    trainer = make_stub_trainer(_opt(alpha_smooth=0.0, use_ssim=False), ["r"])
    S.LAST_SWEEP_FLAGS = None
    ops.KERNEL_EVENTS = {"fwd": [], "bwd": []}
    try:
        trainer.pred_novel_images(inputs, outputs)
        assert S.LAST_SWEEP_FLAGS & C.PD_LOGITS_BF16
        loss = outputs[("ph_mean", "r")] + (outputs[("rgb_rec", "r")] * gw[0].to(DEV)).sum() + \
            (outputs["disp"] * gw[1].to(DEV)).sum() + (outputs["depth"] * gw[2].to(DEV)).sum()
        loss.backward()
        assert len(ops.KERNEL_EVENTS.get("tail_bwd", [])) == 1   # the tail's own backward kernel ran: two kernels
    finally:
        ops.KERNEL_EVENTS = None
    assert a.grad.dtype == BF and s.grad.dtype == BF
    return loss.detach(), a.grad.view(torch.int16), s.grad.view(torch.int16), (d.grad if level_grad else None)


def test_fuse_sweep_backward_with_bf16_takes_no_link_and_changes_nothing():
    """No TailLink with bf16, and the loss and every gradient bit-identical to ``fuse_sweep_backward=False``.

    The case is chosen so that bit-identity can be asked of everything in the graph.  Two sums of the sweep are taken with
    floating-point atomics in arrival order, in fp32 and bf16 alike, and so are not reproducible between two runs of ONE setting
    once more than two addends meet: the fused ``ph_mean`` (one addend per forward workgroup, which serves up to 3 rows of an
    image) and the gradient of the per-plane levels (one addend per row).  So: B = 2 and H = 3, two forward workgroups and two
    addends to ``ph_mean`` (a + b = b + a), and plane levels that are constants, the decoder without ``--plane_residual``.  Every
    gradient of that graph is a gradient of a conv output.  The larger case with learnt levels is the next test."""
    plain, fused = _fuse_graph((2, 7, 3, 256), False, False), _fuse_graph((2, 7, 3, 256), True, False)
    for name, x, y in zip(("loss", "g_raw_logits", "g_raw_sigma"), plain, fused):
        assert torch.equal(x, y), name
    assert bool((plain[1] != 0).any()) and bool((plain[2] != 0).any())


def test_fuse_sweep_backward_with_bf16_on_learnt_levels():
    """The same at the shape of the fp32 fusion test with levels that take a gradient: still no link and two kernels; the conv
    outputs' gradients (no atomics on their way) stay bit-identical; the loss and the level gradient, whose sums are taken with
    atomics in arrival order (see above), are held to the bounds tests/test_bf16_sweep.py uses for ph_mean (1e-6) and g_plane
    (1e-5 of the maximum)."""
    plain, fused = _fuse_graph((2, 7, 9, 256), False, True), _fuse_graph((2, 7, 9, 256), True, True)
    assert torch.equal(plain[1], fused[1]) and torch.equal(plain[2], fused[2])
    assert abs(float(plain[0]) - float(fused[0])) <= 1e-6 * abs(float(plain[0])) + 1e-12
    assert plain[3].dtype == torch.float32
    assert float((plain[3] - fused[3]).abs().max()) <= 1e-5 * float(plain[3].abs().max())


def _trainer_inputs(B, N, H, W, sides, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    feats = torch.rand(B, 8, H, W, generator=g).to(DEV)
    inputs = {("color", "l"): torch.rand(B, 3, H, W, generator=g).to(DEV), "K": torch.eye(4, device=DEV)[None].repeat(B, 1, 1),
              "inv_K": torch.eye(4, device=DEV)[None].repeat(B, 1, 1)}
    inputs["K"][:, 0, 0] = 0.58 * W
    inputs["K"][:, 1, 1] = 1.92 * H
    inputs["K"][:, 0, 2] = 0.5 * W
    inputs["K"][:, 1, 2] = 0.5 * H
    inputs["inv_K"] = torch.inverse(inputs["K"])
    for s in sides:
        inputs[("color", s)] = torch.rand(B, 3, H, W, generator=g).to(DEV)
    return feats, inputs


@pytest.mark.parametrize("sides", [["r"], ["r", -1, 1]])
def test_autocast_bf16_through_the_fused_tail_and_the_trainer(sides):
    """The set-up of tests/test_bf16_sweep.py::test_autocast_bf16_through_the_trainer with the fused tail as the sweep's producer:
    dispconv / sigmaconv emit bf16 under autocast and go into fused_decoder_tail as they are."""
    from gpu_cases import make_stub_trainer
    from planedepth_amd.decoder_tail import fused_decoder_tail
    B, N, H, W = 2, 8, 16, 64
    feats, inputs = _trainer_inputs(B, N, H, W, sides)
    torch.manual_seed(0)
    dispconv = torch.nn.Conv2d(8, N, 3, padding=1).to(DEV)
    sigmaconv = torch.nn.Conv2d(8, N, 3, padding=1).to(DEV)
    trainer = make_stub_trainer(_opt(), sides)

    def step(native):
        for p in list(dispconv.parameters()) + list(sigmaconv.parameters()):
            p.grad = None
        with torch.autocast("cuda", dtype=BF):
            raw_l, raw_s = dispconv(feats), sigmaconv(feats)
            assert raw_l.dtype == BF and raw_s.dtype == BF
            raw_l.retain_grad()
            raw_s.retain_grad()
            levels = torch.linspace(1.0, 30.0, N, device=DEV).reshape(1, N, 1, 1).expand(B, N, 1, 1)
            outputs = {"disp_layered": levels.expand(B, N, H, W), "padding_mask": torch.ones(B, N, H, W, device=DEV),
                       "distance": 0.1 * 0.58 * W / levels[:, :, 0, 0],
                       "norm": torch.tensor([0.0, 0.0, 1.0], device=DEV)[None, None].expand(B, N, -1)}
            if native:
                fused_decoder_tail(outputs, raw_l, raw_s, use_mixture_loss=True, all_ones_mask=True)
            else:   # the fp32 tail on .float() inputs, its logits / sigma cast back: what an autocast user had to write before
                fused_decoder_tail(outputs, raw_l.float(), raw_s.float(), use_mixture_loss=True, all_ones_mask=True)
                outputs["logits"], outputs["sigma"] = outputs["logits"].to(BF), outputs["sigma"].to(BF)
            assert outputs["logits"].dtype == BF and outputs["sigma"].dtype == BF and outputs["disp"].dtype == torch.float32
            for s in sides:
                T = torch.eye(4, device=DEV)[None].repeat(B, 1, 1)
                if s == "r":
                    T[:, 0, 3] = -0.1
                outputs[("Rt", s)] = T
            S.LAST_SWEEP_FLAGS = None
            trainer.pred_novel_images(inputs, outputs)
            flags = S.LAST_SWEEP_FLAGS
            losses = trainer.compute_losses(inputs, outputs)
        loss = losses["loss/total_loss"]
        assert torch.isfinite(loss)
        loss.backward()
        assert raw_l.grad is not None and raw_l.grad.dtype == BF and raw_s.grad is not None and raw_s.grad.dtype == BF
        for conv in (dispconv, sigmaconv):
            assert conv.weight.grad.dtype == torch.float32 and torch.isfinite(conv.weight.grad).all()
        return flags, raw_l.grad.clone(), raw_s.grad.clone()

    flags, g_l, g_s = step(native=True)
    if len(sides) == 1:
        assert flags & C.PD_LOGITS_BF16
        flags32, w_l, w_s = step(native=False)
        assert flags32 & C.PD_LOGITS_BF16   # the same sweep
        _rounded_once("g_raw_logits", g_l, w_l.float())
        _rounded_once("g_raw_sigma", g_s, w_s.float())
    else:
        assert not flags & C.PD_LOGITS_BF16


def _pp_inputs(B, N, H, W, seed=31):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(2 * B, N, H, W, generator=g) * 2
    sigma = torch.rand(2 * B, N, H, W, generator=g) * 0.9 + 0.05
    w = torch.softmax(logits.to(BF).float(), 1) / sigma
    prob = w / w.sum(1, True)
    lv = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(2 * B, N, 1, 1, generator=g) - 0.5
    dl = (40.0 * (2.0 / 40.0) ** (lv / (N - 1))).expand(-1, -1, H, W)
    disp = (prob * dl).sum(1, True)
    return logits.to(DEV), prob.to(DEV), disp.to(DEV), dl.to(DEV)


def test_post_process_widens_bf16_logits():
    logits, prob, disp, dl = _pp_inputs(2, 9, 24, 80)
    got = ops.post_process_disp(logits.bfloat16(), prob, disp, dl, row_uniform=True)
    want = ops.post_process_disp(logits.bfloat16().float(), prob, disp, dl, row_uniform=True)
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    got = ops.post_process_disp(logits.bfloat16(), prob.bfloat16(), disp, dl, row_uniform=True)   # a bf16 probability tensor too
    want = ops.post_process_disp(logits.bfloat16().float(), prob.bfloat16().float(), disp, dl, row_uniform=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    with pytest.raises(TypeError, match="float16"):
        ops.post_process_disp(logits.half(), prob, disp, dl, row_uniform=True)


def test_generate_post_process_disp_with_a_teacher_under_autocast():
    import planedepth_amd as pa
    from planedepth_amd.decoder_tail import fused_decoder_tail
    B, N, H, W = 2, 8, 16, 64
    torch.manual_seed(1)
    enc = torch.nn.Conv2d(3, 8, 3, padding=1).to(DEV)
    dispconv = torch.nn.Conv2d(8, N, 3, padding=1).to(DEV)
    sigmaconv = torch.nn.Conv2d(8, N, 3, padding=1).to(DEV)
    levels = torch.linspace(1.0, 30.0, N, device=DEV).reshape(1, N, 1, 1).expand(2 * B, N, 1, 1)

    def encoder(x):
        with torch.autocast("cuda", dtype=BF):
            return enc(x)

    def depth(feats, grids):
        with torch.autocast("cuda", dtype=BF):
            outputs = {"disp_layered": levels.expand(2 * B, N, H, W)}
            fused_decoder_tail(outputs, dispconv(feats), sigmaconv(feats), use_mixture_loss=True, all_ones_mask=True)
        assert outputs["logits"].dtype == BF
        return outputs

    ns = types.SimpleNamespace(opt=types.SimpleNamespace(num_ep=1, net_type="ResNet", yz_levels=0),
                               fixed_models={"encoder": encoder, "depth": depth})
    g = torch.Generator().manual_seed(2)
    inputs = {("color_aug", "l"): torch.rand(B, 3, H, W, generator=g).to(DEV), "grid": torch.zeros(B, 2, H, W, device=DEV)}
    with torch.no_grad():
        disp_pp, mask_novel = pa.generate_post_process_disp(ns, inputs)
    for t in (disp_pp, mask_novel):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B, 1, H, W) and bool(torch.isfinite(t).all())


def test_bf16_backward_is_deterministic():
    """Two runs of the bf16 backward give the same bit patterns in the bf16 gradients (and in the dense fp32 disparity gradient,
    stored per pixel; the per-plane form is a block sum that fp32 takes the same way and is not part of this check)."""
    shape = (2, 12, 24, 640)
    for dense in (False, True):
        rl_b, rs_b, pm, lv, ups = _decoder_case(shape, True, True, dense)
        runs = []
        for _ in range(2):
            r = _decoder_route(rl_b, rs_b, pm, lv, ups, True, dense, widen=False)
            runs.append((r["g_rl"].view(torch.int16).clone(), r["g_rs"].view(torch.int16).clone()) + ((r["g_dl"].clone(),) if dense else ()))
        assert all(torch.equal(x, y) for x, y in zip(*runs))
    rl_b, rs_b, lv, ups = _plade_case(shape)
    runs = []
    for _ in range(2):
        r = _plade_route(rl_b, rs_b, lv, ups, True, True, widen=False)
        runs.append((r["g_rl"].view(torch.int16).clone(), r["g_rs"].view(torch.int16).clone(), r["g_dl"].clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
