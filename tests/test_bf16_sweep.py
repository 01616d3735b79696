"""bf16 logits / sigma (PD_LOGITS_BF16) on the GPU: the native kernels against the fp32 route on the widened inputs, the fallback
routes, and a tiny decoder under torch.autocast through the patched trainer."""
import types

import pytest
import torch

from cases import run_oracle
from planedepth_amd import _capi as C
from planedepth_amd import _state as S
from planedepth_amd import ops
from planedepth_amd.synthetic import build_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream_tol(W):   # pd_rowgeom.h irregular_tol(W)
    return 2.5e-4 + 1.25e-6 * W


# the parameter list of tests/test_gpu_parity.py::test_rowstream_backward_equals_rowshift_backward_and_oracle, plus the headline shapes
SHAPES = [
    (640, 6, 12, "r", True, "threshold"),
    (130, 7, 12, "l", True, "threshold"),
    (1280, 4, 12, "r", True, "threshold"),
    (258, 9, 7, "r", True, dict(disp_min=0.5, disp_max=120.0)),
    (70, 5, 5, "l", True, dict(disp_min=0.3, disp_max=40.0)),
    (2, 3, 2, "r", True, dict(disp_min=0.2, disp_max=1.5)),
    (257, 5, 5, "l", True, dict(disp_min=0.5, disp_max=80.0)),
    (640, 12, 9, "r", True, dict(disp_min=2.0, disp_max=300.0)),
    (70, 11, 10, "r", True, dict(special_disp=[0.0, 1.0, 2.0, 1.9999999, 3.0000002, 7.5, 68.9999, 69.0, 75.0, 1e6], disp_min=0.5, disp_max=9.0)),
    (130, 7, 9, "l", True, dict(special_disp=[0.25, 1.0, 63.0, 64.0, 64.00001, 65.5, 127.99999, 129.0, 200.0], disp_min=0.5, disp_max=9.0)),
    (300, 8, 8, "r", False, dict(special_disp=[299.99997, 2.0000002, 1.9999998, 0.99999994, 100.0, 33.333332, 255.0, 256.00003], disp_min=0.5, disp_max=9.0)),
    (1280, 6, 4, "r", True, dict(disp_min=2.0, disp_max=300.0)),
    (1024, 4, 9, "l", True, dict(disp_min=2.0, disp_max=400.0)),
    (2048, 3, 3, "l", True, dict(disp_min=2.0, disp_max=900.0)),
    (2600, 2, 2, "r", True, dict(disp_min=2.0, disp_max=900.0)),
    (3000, 2, 2, "r", True, dict(disp_min=2.0, disp_max=900.0)),
    (640, 3, 1, "r", True, dict(disp_min=5.0, disp_max=5.0)),
    (130, 3, 2, "r", True, dict(special_disp=[5.0, 9.3], disp_min=0.5, disp_max=9.0)),
    (384, 8, 63, "r", False, dict(disp_min=0.5, disp_max=200.0)),
    (200, 33, 12, "r", True, dict(disp_min=0.5, disp_max=60.0, n_xz=4)),
    (200, 33, 12, "l", False, dict(disp_min=0.5, disp_max=60.0, n_xz=4)),
]


def _case(W, H, N, kw, B=2, seed=None):
    if kw == "threshold":
        t = _stream_tol(W)
        ks = [1.0, 7.0, 64.0, float(W // 2)]
        disps = [ks[0], ks[0] + 0.9 * t, ks[0] + 1.1 * t, ks[1] - 0.9 * t, ks[1] - 1.1 * t, ks[1] + 0.5,
                 ks[2], ks[2] + 1.1 * t, ks[2] - 1.1 * t, ks[3] + 0.9 * t, ks[3] - 0.9 * t, float(W + 3)]
        kw = dict(special_disp=disps[:N], disp_min=0.5, disp_max=9.0)
    return build_case(B=B, N=N, H=H, W=W, seed=seed if seed is not None else 5000 + W + H, sigma_interior=True, **dict(kw))


def _sweep(case, lg, sg, side, mix, automask, **kw):
    """plane_sweep_disp on (lg, sg) -> outputs, gradients (of lg, sg, the plane disparities) and the flags it ran with."""
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}
    B, N, H, W = c["logits"].shape
    disp_pp = c["disp_pp"].clone().requires_grad_(True)
    disp = disp_pp.expand(-1, -1, H, W) * c["row_gain"] if case["dense_disp"] else disp_pp.expand(-1, -1, H, W)
    pm = c["padding_mask"] if (case["dense_disp"] and kw.pop("mask", True)) else None
    src, tgt = (c["color_l"], c["color_r"]) if side == "r" else (c["color_r"], c["color_l"])
    rgb, ph, ph_mean = ops.plane_sweep_disp(src, tgt, lg, sg if mix else None, disp, pm, target_side=side, use_mixture_loss=mix,
                                            automask=automask, row_uniform=kw.pop("row_uniform", True), return_mean=True, **kw)
    flags = S.LAST_SWEEP_FLAGS
    _retain_f32_copies(lg, sg)
    g = c["g_rgb_rec"]
    ((rgb * g).sum() + ph_mean * 3.0 + (ph * g[:, :1]).sum()).backward()
    return dict(rgb_rec=rgb.detach(), ph_map=ph.detach(), ph_mean=ph_mean.detach(), g_plane=disp_pp.grad), flags


def _retain_f32_copies(*ts):
    """The fallback's fp32 copies (ops.as_f32) keep their gradient: the one the cast's backward rounds."""
    for t in ts:
        f = getattr(t, "_pd_f32", None)
        if f is not None and f[1].requires_grad:
            f[1].retain_grad()


def _rounded_once(t):
    """t.grad is its fp32 copy's gradient rounded once (the fallback route)."""
    f = t._pd_f32[1]
    return torch.equal(t.grad, f.grad.to(t.dtype))


def _leaves(case, dtype):
    lg = case["logits"].to(DEV).to(dtype).requires_grad_(True)
    sg = case["sigma"].to(DEV).to(dtype).requires_grad_(True)
    return lg, sg


def _ulp_dist(a, b):
    """bf16 bit-pattern distance, +0 == -0."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def _check(case, side, mix, automask, **kw):
    lb, sb = _leaves(case, torch.bfloat16)
    got, flags = _sweep(case, lb, sb, side, mix, automask, **dict(kw))
    lf = lb.detach().float().requires_grad_(True)
    sf = sb.detach().float().requires_grad_(True)
    want, flags32 = _sweep(case, lf, sf, side, mix, automask, **dict(kw))
    assert not flags32 & C.PD_LOGITS_BF16
    for k in ("rgb_rec", "ph_map"):
        ndiff = int((got[k] != want[k]).sum())
        scale = float(want[k].abs().max()) or 1.0
        err = float((got[k] - want[k]).abs().max())
        assert err <= 1e-6 * scale, (k, err, scale, ndiff)
    assert abs(float(got["ph_mean"]) - float(want["ph_mean"])) <= 1e-6 * abs(float(want["ph_mean"])) + 1e-12
    grads = [("g_logits", lb.grad, lf.grad)] + ([("g_sigma", sb.grad, sf.grad)] if mix else [])
    for name, gb, g32 in grads:
        assert gb.dtype == torch.bfloat16
        d = _ulp_dist(gb, g32.to(torch.bfloat16))
        assert int(d.max()) <= 1, (name, int(d.max()))
        assert int((d != 0).sum()) <= 1e-4 * d.numel(), (name, int((d != 0).sum()))
    gp, gp32 = got["g_plane"], want["g_plane"]
    assert float((gp - gp32).abs().max()) <= 1e-5 * max(float(gp32.abs().max()), 1e-30), "g_plane"
    return flags, (lb, sb)


@pytest.mark.parametrize("W,H,N,side,mix,kw", SHAPES)
def test_native_bf16_equals_fp32_route_rounded_once(W, H, N, side, mix, kw):
    case = _case(W, H, N, kw)
    automask = 0.0 not in (kw.get("special_disp", ()) if isinstance(kw, dict) else ())
    flags, _ = _check(case, side, mix, automask)
    d = C.SweepDesc(2, N, H, W, C.PD_WARP_DISP, flags & ~C.PD_LOGITS_BF16, 1.0, 0)
    assert bool(flags & C.PD_LOGITS_BF16) == bool(C.load().pd_sweep_native_bf16(d))
    if W % 2 == 0 and W <= 2048:
        assert flags & C.PD_LOGITS_BF16, (W, flags)


@pytest.mark.parametrize("N,n_xz,automask", [(49, 0, False), (63, 14, True)])
def test_native_bf16_headline_shapes(N, n_xz, automask):
    case = build_case(B=8, N=N, H=192, W=640, seed=11, disp_min=0.5, disp_max=300.0, sigma_interior=True, n_xz=n_xz)
    flags, _ = _check(case, "r", True, automask)
    assert flags & C.PD_LOGITS_BF16


def test_native_bf16_backward_is_deterministic():
    case = build_case(B=2, N=12, H=24, W=640, seed=3, disp_min=0.5, disp_max=300.0, sigma_interior=True, n_xz=3)
    runs = []
    for _ in range(2):
        lb, sb = _leaves(case, torch.bfloat16)
        _, flags = _sweep(case, lb, sb, "l", True, True)
        assert flags & C.PD_LOGITS_BF16
        runs.append((lb.grad.view(torch.int16).clone(), sb.grad.view(torch.int16).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_native_bf16_against_the_oracle():
    case = build_case(B=2, N=9, H=24, W=80, seed=7, disp_min=0.5, disp_max=40.0, sigma_interior=True)
    case = dict(case)
    case["logits"] = case["logits"].to(torch.bfloat16).float()
    case["sigma"] = case["sigma"].to(torch.bfloat16).float()
    lb, sb = _leaves(case, torch.bfloat16)
    got, flags = _sweep(case, lb, sb, "r", True, False)
    assert flags & C.PD_LOGITS_BF16
    want = run_oracle(case, dict(target_side="r", use_mixture_loss=True))
    err = float((got["rgb_rec"].cpu() - want["rgb_rec"]).abs().max()) / float(want["rgb_rec"].abs().max())
    assert err < 1e-4, err


@pytest.mark.parametrize("route", ["dense_yz", "pixel_mask", "render", "general", "rows1", "odd_w"])
def test_fallback_routes_equal_fp32_exactly(route):
    W = 257 if route == "odd_w" else 130
    case = build_case(B=2, N=6, H=9, W=W, seed=21, disp_min=0.5, disp_max=40.0, sigma_interior=True,
                      n_xz=2 if route in ("dense_yz", "pixel_mask") else 0)
    kw = {}
    if route in ("dense_yz", "pixel_mask"):
        kw["row_uniform"] = False
        kw["mask"] = route == "pixel_mask"
    if route == "render":
        kw.update(render_probability=True, dists=torch.rand(2, 5, 9, W, device=DEV) + 0.1)
    impl = {"general": C.PD_IMPL_GENERAL, "rows1": C.PD_IMPL_ROWS1}.get(route, C.PD_IMPL_AUTO)
    ops.SWEEP_IMPL = impl
    try:
        lb, sb = _leaves(case, torch.bfloat16)
        got, flags = _sweep(case, lb, sb, "r", True, False, **dict(kw))
        lf = lb.detach().float().requires_grad_(True)
        sf = sb.detach().float().requires_grad_(True)
        want, _ = _sweep(case, lf, sf, "r", True, False, **dict(kw))
    finally:
        ops.SWEEP_IMPL = C.PD_IMPL_AUTO
    assert not flags & C.PD_LOGITS_BF16
    for k in ("rgb_rec", "ph_map"):
        assert torch.equal(got[k], want[k]), k
    assert lb.grad.dtype == torch.bfloat16
    assert _rounded_once(lb) and _rounded_once(sb)
    for gb, g32 in ((lb.grad, lf.grad), (sb.grad, sf.grad)):   # (the general kernels add with atomics: the last fp32 bit may move)
        assert int(_ulp_dist(gb, g32.to(torch.bfloat16)).max()) <= 1


@pytest.mark.parametrize("uniform", [False, True])
def test_homography_falls_back(uniform):
    B, N, H, W = 2, 5, 12, 64
    case = build_case(B=B, N=N, H=H, W=W, seed=31, disp_min=0.5, disp_max=20.0, sigma_interior=True)
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}
    distance = (0.1 * 0.58 * W / c["disp_pp"][:, :, 0, 0]).detach()
    norm = torch.tensor([0.0, 0.0, 1.0], device=DEV)[None, None].expand(B, N, -1).contiguous()
    T = torch.eye(4, device=DEV)[None].repeat(B, 1, 1)
    if not uniform:
        T[:, 0, 3] = 0.1
    T[:, 0, 1] = 0.01
    res = []
    for dt in (torch.bfloat16, torch.float32):
        lb = case["logits"].to(DEV).to(torch.bfloat16)
        sb = case["sigma"].to(DEV).to(torch.bfloat16)
        lg = (lb if dt == torch.bfloat16 else lb.float()).requires_grad_(True)
        sg = (sb if dt == torch.bfloat16 else sb.float()).requires_grad_(True)
        rgb, ph = ops.plane_sweep_homography(c["color_l"], c["color_r"], lg, sg, distance, norm, T, c["K"], c["inv_K"],
                                             plane_uniform=uniform)
        assert not S.LAST_SWEEP_FLAGS & C.PD_LOGITS_BF16
        _retain_f32_copies(lg, sg)
        ((rgb * c["g_rgb_rec"]).sum() + ph.sum()).backward()
        res.append((rgb.detach(), lg, sg))
    assert torch.equal(res[0][0], res[1][0])
    assert _rounded_once(res[0][1]) and _rounded_once(res[0][2])
    for a, b in ((res[0][1], res[1][1]), (res[0][2], res[1][2])):
        assert int(_ulp_dist(a.grad, b.grad.to(torch.bfloat16)).max()) <= 1


def test_fp32_never_sets_the_flag():
    case = build_case(B=2, N=5, H=8, W=128, seed=1, disp_min=0.5, disp_max=20.0, sigma_interior=True)
    lf, sf = _leaves(case, torch.float32)
    _, flags = _sweep(case, lf, sf, "r", True, False)
    assert not flags & C.PD_LOGITS_BF16
    assert lf.grad.dtype == torch.float32


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
def test_autocast_bf16_through_the_trainer(sides):
    from gpu_cases import make_stub_trainer
    B, N, H, W = 2, 8, 16, 64
    feats, inputs = _trainer_inputs(B, N, H, W, sides)
    dispconv = torch.nn.Conv2d(8, N, 3, padding=1).to(DEV)
    sigmaconv = torch.nn.Conv2d(8, N, 3, padding=1).to(DEV)
    opt = types.SimpleNamespace(warp_type="disp_warp", match_aug=False, use_mixture_loss=True, automask=False,
                                render_probability=False, alpha_pc=0.0, alpha_self=0.0, self_distillation=0.0,
                                gamma_smooth=2.0, alpha_smooth=0.04, use_ssim=True, xz_levels=0, yz_levels=0,
                                materialize_layers=False)
    trainer = make_stub_trainer(opt, sides)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = dispconv(feats)
        sigma = torch.sigmoid(sigmaconv(feats)).clamp(0.01, 1.0)
        assert logits.dtype == torch.bfloat16 and sigma.dtype == torch.bfloat16
        logits.retain_grad()
        levels = torch.linspace(1.0, 30.0, N, device=DEV).reshape(1, N, 1, 1).expand(B, N, 1, 1)
        disp_layered = levels.expand(B, N, H, W)
        prob = torch.softmax(logits.float(), 1)
        outputs = {"logits": logits, "sigma": sigma, "probability": prob, "disp_layered": disp_layered,
                   "padding_mask": torch.ones(B, N, H, W, device=DEV),
                   "disp": (prob * disp_layered).sum(1, True),
                   "distance": 0.1 * 0.58 * W / levels[:, :, 0, 0], "norm": torch.tensor([0.0, 0.0, 1.0], device=DEV)[None, None].expand(B, N, -1)}
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
    assert logits.grad is not None and logits.grad.dtype == torch.bfloat16
    assert dispconv.weight.grad.dtype == torch.float32 and sigmaconv.weight.grad.dtype == torch.float32
    assert torch.isfinite(dispconv.weight.grad).all() and torch.isfinite(sigmaconv.weight.grad).all()
    if len(sides) == 1:
        assert flags & C.PD_LOGITS_BF16
    else:
        assert not flags & C.PD_LOGITS_BF16
