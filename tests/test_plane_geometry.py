"""The row form on the GPU: ``ops.plane_geometry`` against the reference-captured fixture (tests/golden/plane_geometry.npz, written
by tests/golden/make_plane_geometry_golden.py), the decoder tail's row form against its dense form bit for bit, determinism,
the stride-derived routes of the sweep / post-process / trainer path, the allocation count of the row route, and the guards."""
import json
import os
import types

import numpy as np
import pytest
import torch

from cases import rel_err
from conftest import GOLDEN
from planedepth_amd import _capi as C
from planedepth_amd import decoder_tail, ops, synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
XZ = dict(xz_min=0.1852, xz_max=0.3704)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "plane_geometry.npz"))
    meta = json.loads(str(z["meta"]))
    cases = {}
    for tag, kw in meta["cases"].items():
        t = {k.split("/", 1)[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/")}
        for k in ("grid", "q_logits", "q_sigma"):
            t.setdefault(k, torch.from_numpy(z["%s/%s" % (kw["inputs_of"], k)]))
        cases[tag] = (kw, t)
    return meta, cases


def geom_kw(meta, kw):
    return dict(no_levels=kw["no_levels"], xz_levels=kw["xz_levels"], **meta["cfg"])


@pytest.mark.parametrize("tag", ["xz_res", "xz_nores", "xy_res"])
def test_geometry_matches_the_reference(golden, tag):
    meta, cases = golden
    kw, t = cases[tag]
    B, H, W = kw["B"], kw["H"], kw["W"]
    residual = t["residual"].to(DEV) if kw["plane_residual"] else None
    dl, pm, distance, norm = ops.plane_geometry(t["grid"].to(DEV), residual, **geom_kw(meta, kw))
    N = kw["no_levels"] + kw["xz_levels"]
    assert tuple(dl.shape) == tuple(pm.shape) == (B, N, H, W) and dl.stride(3) == 0 and pm.stride(3) == 0
    for name, got, want in (("disp_rows", dl[..., 0], t["disp_rows"]), ("distance", distance, t["distance"]),
                            ("norm", norm, t["norm"])):
        e = rel_err(got.cpu(), want)
        print(tag, name, e)
        assert e < TOL, (name, e)
    assert torch.equal(pm[..., 0].cpu(), t["mask_rows"])
    if kw["xz_levels"]:
        assert 0 < int((t["mask_rows"] == 0).sum()) < t["mask_rows"].numel()     # the horizon is inside the crop
    else:   # xz_levels == 0: what pd_plane_levels gives, on every row
        d0, dist0 = ops.plane_disparities(torch.arange(N, device=DEV, dtype=torch.float32)[None] + residual,
                                          meta["cfg"]["disp_min"], meta["cfg"]["disp_max"], W)
        assert torch.equal(dl[:, :, 0, 0], d0.reshape(B, N)) and torch.equal(dl[:, :, -1, 0], d0.reshape(B, N))
        assert torch.equal(distance, dist0)


@pytest.mark.parametrize("tag", ["xz_res", "xz_nores", "xy_res"])
def test_fused_geometry_and_tail_match_the_reference_end_to_end(golden, tag):
    meta, cases = golden
    kw, t = cases[tag]
    s, y0, x0 = meta["stride"]
    sub = lambda v: v[..., y0::s, x0::s].cpu()  # noqa: E731
    raw_logits = (t["q_logits"].float() / 8).to(DEV).requires_grad_(True)
    raw_sigma = (t["q_sigma"].float() / 8).to(DEV).requires_grad_(True)
    residual = t["residual"].to(DEV).requires_grad_(True) if kw["plane_residual"] else None
    o = {}
    decoder_tail.fused_plane_geometry(o, t["grid"].to(DEV), residual, **geom_kw(meta, kw))
    decoder_tail.fused_decoder_tail(o, raw_logits, raw_sigma, use_mixture_loss=True)
    d = {k: v.to(DEV) for k, v in t.items() if k.startswith("gw_")}
    obj = ((o["logits"] * (d["gw_plane_logits"] * d["gw_pix_logits"])).sum()
           + (o["sigma"] * (d["gw_plane_sigma"] * d["gw_pix_sigma"])).sum() + (o["disp"] * d["gw_disp"]).sum()
           + (o["depth"] * d["gw_depth"]).sum() + (o["distance"] * d["gw_distance"]).sum())
    obj.backward()
    checks = [("logits", sub(o["logits"]), t["logits"]), ("sigma", sub(o["sigma"]), t["sigma"]), ("disp", o["disp"].cpu(), t["disp"]),
              ("depth", o["depth"].cpu(), t["depth"]), ("g_raw_logits", sub(raw_logits.grad), t["g_raw_logits"]),
              ("g_raw_sigma", sub(raw_sigma.grad), t["g_raw_sigma"])]
    if residual is not None:
        checks.append(("g_residual", residual.grad.cpu(), t["g_residual"]))
    for name, got, want in checks:
        e = rel_err(got.detach(), want)
        print(tag, name, e)
        assert e < TOL, (name, e)


# ---------------------------------------------------------------------------------------------------------------------
# row form against dense form
# ---------------------------------------------------------------------------------------------------------------------
SPLIT = {5: (3, 2), 7: (4, 3), 63: (49, 14)}
SHAPES = [(2, 6), (3, 4), (5, 7), (8, 16), (24, 80)]


def rows_inputs(B, N, H, W, seed=0, residual_grad=False):
    """Row views from ops.plane_geometry on the plain Resize grid (an odd H has a grid row at exactly y = 0: masked)."""
    g = torch.Generator().manual_seed(seed)
    nl, nx = SPLIT[N]
    grid = synthetic.crop_grid(H, W, H, W, 0, 0)[None].repeat(B, 1, 1, 1).to(DEV)
    residual = (torch.rand(B, N, generator=g) - 0.5).to(DEV).requires_grad_(residual_grad)
    dl, pm, distance, norm = ops.plane_geometry(grid, residual, no_levels=nl, xz_levels=nx, disp_min=2.0, disp_max=30.0, **XZ)
    return grid, residual, dl, pm, distance, norm


def tail_run(raw_logits, raw_sigma, pm, dl, mix, gw):
    rl, rs = raw_logits.clone().requires_grad_(True), raw_sigma.clone().requires_grad_(True)
    dl = dl.detach().requires_grad_(True) if dl.is_contiguous() else dl
    logits, sigma, disp, depth, layers = ops.decoder_tail(rl, rs if mix else None, pm, dl, use_mixture_loss=mix)
    pi, prob = layers(want_pi=mix, want_probability=True)
    obj = (logits.float() * gw["l"]).sum() + (disp * gw["d"]).sum() + (depth * gw["z"]).sum()
    if mix:
        obj = obj + (sigma.float() * gw["s"]).sum()
    obj.backward()
    return dict(logits=logits, sigma=sigma, disp=disp, depth=depth, pi=pi, prob=prob, g_l=rl.grad, g_s=rs.grad if mix else None,
                g_dl=dl.grad if dl.is_leaf else None)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mix", [True, False], ids=["mix", "l1"])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("N", [5, 7, 63])
def test_row_form_has_the_dense_forms_bits(N, H, W, mix, bf16):
    B = 2
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    _, _, dl, pm, _, _ = rows_inputs(B, N, H, W)
    rows_d = dl._pd_rows.detach()
    if H % 2:
        assert bool((pm[:, SPLIT[N][0]:, H // 2, 0] == 0).all())           # the row at exactly y = 0 is masked
    st = torch.bfloat16 if bf16 else torch.float32
    raw_logits = (torch.randn(B, N, H, W, generator=g) * 3).to(DEV).to(st)
    raw_sigma = (torch.randn(B, N, H, W, generator=g) * 3.5 - 1.0).to(DEV).to(st)       # hits both clamp bounds of sigma
    sg = torch.sigmoid(raw_sigma.float())
    if N * H * W >= 300:
        assert bool((sg < 0.01).any()) and bool((sg == 1.0).any() or (sg > 0.999).any())
    gw = dict(l=torch.randn(B, N, H, W, generator=g).to(DEV), s=torch.randn(B, N, H, W, generator=g).to(DEV),
              d=torch.randn(B, 1, H, W, generator=g).to(DEV), z=(torch.randn(B, 1, H, W, generator=g) * 0.1).to(DEV))
    dense_d, dense_m = dl.detach().contiguous(), pm.contiguous()
    view_d = ops.row_view(rows_d.clone().requires_grad_(True), W)
    want = tail_run(raw_logits, raw_sigma, dense_m, dense_d, mix, gw)
    forms = dict(rows=(pm, view_d), mask_rows_dense_map=(pm, dense_d), dense_mask_row_map=(dense_m, view_d))
    for name, (m, d) in forms.items():
        if d is view_d:
            view_d._pd_rows.grad = None
        got = tail_run(raw_logits, raw_sigma, m, d, mix, gw)
        for k in ("logits", "sigma", "disp", "depth", "pi", "prob", "g_l", "g_s"):
            if want[k] is None:
                continue
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (name, k)
        if d is view_d:
            g_rows = view_d._pd_rows.grad
            assert tuple(g_rows.shape) == (B, N, H)
            e = rel_err(g_rows, want["g_dl"].sum(-1))
            assert e < TOL, (name, e)
        else:
            assert torch.equal(got["g_dl"], want["g_dl"]), name


def test_backward_is_deterministic():
    B, N, H, W = 2, 63, 24, 80
    g = torch.Generator().manual_seed(3)
    raw_logits = (torch.randn(B, N, H, W, generator=g) * 3).to(DEV)
    raw_sigma = (torch.randn(B, N, H, W, generator=g) * 3.5 - 1.0).to(DEV)
    gw = torch.randn(B, 1, H, W, generator=g).to(DEV)
    gdist = torch.randn(B, N, generator=g).to(DEV)
    grads = []
    for _ in range(2):
        _, residual, dl, pm, distance, _ = rows_inputs(B, N, H, W, seed=5, residual_grad=True)
        _, _, disp, depth, _ = ops.decoder_tail(raw_logits, raw_sigma, pm, dl)
        ((disp * gw).sum() + (depth * gw).sum() * 0.1 + (distance * gdist).sum()).backward()
        grads.append(residual.grad.clone())
    assert bool(grads[0].abs().sum() > 0) and torch.equal(grads[0], grads[1])


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------
def sweep_inputs(B, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    src, tgt = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    logits = torch.randn(B, N, H, W, generator=g).to(DEV)
    sigma = (0.011 + 0.978 * torch.rand(B, N, H, W, generator=g)).to(DEV)
    return src, tgt, logits, sigma


def test_sweep_and_post_process_take_the_row_route_from_the_strides():
    B, N, H, W = 2, 7, 24, 80
    _, _, dl, pm, _, _ = rows_inputs(B, N, H, W, seed=1)
    src, tgt, logits, sigma = sweep_inputs(B, N, H, W, 2)
    dense_d, dense_m = dl.detach().contiguous(), pm.contiguous()
    got = ops.plane_sweep_disp(src, tgt, logits, sigma, dl, pm)                               # no promise
    want = ops.plane_sweep_disp(src, tgt, logits, sigma, dense_d, dense_m, row_uniform=True)
    for a, b in zip(got, want):
        assert rel_err(a, b) < TOL
    sliced = ops.plane_sweep_disp(src[:1], tgt[:1], logits[:1], sigma[:1], dl[:1], pm[:1])    # a batch slice keeps the strides
    assert rel_err(sliced[0], want[0][:1]) < TOL
    disp = (torch.softmax(logits, 1) * dense_d).sum(1, True)
    prob = torch.softmax(logits, 1)
    got = ops.post_process_disp(logits, prob, disp, dl)
    want = ops.post_process_disp(logits, prob, disp, dense_d, row_uniform=True)
    for a, b in zip(got, want):
        assert rel_err(a, b) < TOL


def test_patched_trainer_takes_the_views():
    from gpu_cases import make_stub_trainer
    B, N, H, W = 2, 7, 24, 80
    src, tgt, logits, sigma = sweep_inputs(B, N, H, W, 4)
    res = {}
    for form in ("views", "dense"):
        _, _, dl, pm, distance, norm = rows_inputs(B, N, H, W, seed=1)
        if form == "dense":
            dl, pm = dl.detach().contiguous(), pm.contiguous()
        lg, sg = logits.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
        opt = types.SimpleNamespace(warp_type="disp_warp", match_aug=False, use_mixture_loss=True, automask=False,
                                    render_probability=False, alpha_pc=0.0, alpha_self=0.0, self_distillation=0.0, gamma_smooth=2.0,
                                    alpha_smooth=0.04, use_ssim=True, xz_levels=3, yz_levels=0, novel_frame_ids=[],
                                    pd_check_contract=True)
        trainer = make_stub_trainer(opt, ["r"], DEV)
        K, inv_K = synthetic.intrinsics(B, H, W)
        Rt = torch.eye(4, device=DEV)[None].repeat(B, 1, 1)
        Rt[:, 0, 3] = -0.1
        inputs = {("color", "l"): src, ("color", "r"): tgt, "K": K.to(DEV), "inv_K": inv_K.to(DEV),
                  "grid": synthetic.crop_grid(H, W, H, W, 0, 0)[None].repeat(B, 1, 1, 1).to(DEV)}
        outputs = {"probability": torch.empty(B, N, H, W, device="meta"), "logits": lg, "sigma": sg, "disp_layered": dl,
                   "padding_mask": pm, "distance": distance, "norm": norm, ("Rt", "r"): Rt,
                   "disp": (torch.softmax(logits, 1) * dl.detach()).sum(1, True)}
        trainer.pred_novel_images(inputs, outputs)
        losses = trainer.compute_losses(inputs, outputs)
        losses["loss/total_loss"].backward()
        res[form] = (outputs[("rgb_rec", "r")].detach(), losses["loss/total_loss"].detach(), lg.grad, sg.grad)
    for a, b in zip(res["views"], res["dense"]):
        assert rel_err(a, b) < TOL


def test_residual_gradient_through_sweep_tail_and_geometry():
    B, N, H, W = 1, 7, 24, 80
    nl, nx = SPLIT[N]
    g = torch.Generator().manual_seed(9)
    src, tgt, _, _ = sweep_inputs(B, N, H, W, 6)
    raw_logits = torch.randn(B, N, H, W, generator=g).to(DEV)
    raw_sigma = torch.randn(B, N, H, W, generator=g).to(DEV)
    grid = synthetic.crop_grid(H, W, 60, 200, 11, 37)[None].to(DEV)
    res0 = (torch.rand(B, N, generator=g) - 0.5).to(DEV)
    cfg = dict(no_levels=nl, xz_levels=nx, disp_min=2.0, disp_max=30.0, **XZ)
    grads = {}
    for form in ("rows", "dense"):
        residual = res0.clone().requires_grad_(True)
        if form == "rows":
            dl, pm, _, _ = ops.plane_geometry(grid, residual, **cfg)
            kw = {}
        else:
            geo = synthetic.decoder_plane_geometry(grid, residual, **cfg)      # torch autograd over the dense formulation
            dl, pm, kw = geo["disp_layered"], geo["padding_mask"], dict(row_uniform=True)
        logits, sigma, disp, _, _ = ops.decoder_tail(raw_logits, raw_sigma, pm, dl)
        _, ph_map = ops.plane_sweep_disp(src, tgt, logits, sigma, dl, pm, **kw)
        (ph_map.mean() + disp.mean() * 0.01).backward()
        grads[form] = residual.grad
    e = rel_err(grads["rows"], grads["dense"])
    print("g_residual rows vs dense", e)
    assert e < TOL, e


def test_row_route_requests_no_dense_block():
    """Bytes newly requested from torch's allocator (a deterministic counter) by forward + backward of geometry + tail with a loss
    on disp: the row route stays below the dense route's minus three [B,N,H,W] fp32 blocks (map, mask, g_disp_layered)."""
    B, N, H, W = 1, 63, 64, 256
    nl, nx = SPLIT[N]
    g = torch.Generator().manual_seed(2)
    raw_logits = torch.randn(B, N, H, W, generator=g).to(DEV).requires_grad_(True)
    raw_sigma = torch.randn(B, N, H, W, generator=g).to(DEV).requires_grad_(True)
    grid = synthetic.crop_grid(H, W, H, W, 0, 0)[None].to(DEV)
    residual = (torch.rand(B, N, generator=g) - 0.5).to(DEV).requires_grad_(True)
    cfg = dict(no_levels=nl, xz_levels=nx, disp_min=2.0, disp_max=300.0, **XZ)

    def requested(route):
        raw_logits.grad = raw_sigma.grad = residual.grad = None
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
        if route == "rows":
            dl, pm, _, _ = ops.plane_geometry(grid, residual, **cfg)
        else:
            geo = synthetic.decoder_plane_geometry(grid, residual, **cfg)
            dl, pm = geo["disp_layered"], geo["padding_mask"]
        _, _, disp, _, _ = ops.decoder_tail(raw_logits, raw_sigma, pm, dl)
        disp.sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - before

    requested("rows")      # (first calls: pools and caches)
    rows, dense = requested("rows"), requested("dense")
    block = B * N * H * W * 4
    print("requested bytes: rows %d, dense %d, [B,N,H,W] block %d" % (rows, dense, block))
    assert rows < dense - 3 * block, (rows, dense, block)


def test_guards():
    B, N, H, W = 2, 7, 5, 8
    grid, residual, dl, pm, _, _ = rows_inputs(B, N, H, W)
    raw = torch.randn(B, N, H, W, device=DEV)
    with pytest.raises(ValueError):                       # stride(3) == 0, wrong shape
        ops.decoder_tail(raw[:, :, :, :6].contiguous(), raw[:, :, :, :6].contiguous(), pm, dl)
    with pytest.raises(ValueError):
        ops.plane_sweep_disp(raw[:, :3], raw[:, :3], raw, raw.sigmoid(), dl[:, :5], None)
    with pytest.raises(ValueError):
        ops.post_process_disp(raw, raw.softmax(1), raw[:, :1], dl[:, :, :4])
    with pytest.raises(TypeError):                        # a non-fp32 map
        ops.decoder_tail(raw, raw, pm, ops.row_view(dl._pd_rows.detach().double(), W))
    with pytest.raises(TypeError):
        ops.plane_geometry(grid.double(), residual, no_levels=4, xz_levels=3, disp_min=2.0, disp_max=30.0, **XZ)
    with pytest.raises(ValueError):
        ops.plane_geometry(grid, residual[:, :5], no_levels=4, xz_levels=3, disp_min=2.0, disp_max=30.0, **XZ)
    with pytest.raises(C.PlaneDepthHipError):
        ops.plane_geometry(grid, residual[:, :5].contiguous(), no_levels=4, xz_levels=1, disp_min=2.0, disp_max=30.0, **XZ)
    sheared = grid.clone()
    sheared[:, 1] += torch.linspace(0, 0.1, W, device=DEV)
    ops.plane_geometry(sheared, residual, no_levels=4, xz_levels=3, disp_min=2.0, disp_max=30.0, check_contract=False, **XZ)
    with pytest.raises(ValueError):
        ops.plane_geometry(sheared, residual, no_levels=4, xz_levels=3, disp_min=2.0, disp_max=30.0, check_contract=True, **XZ)


def test_contract_check_follows_the_environment(monkeypatch):
    B, N, H, W = 1, 7, 5, 8
    grid, residual, _, _, _, _ = rows_inputs(B, N, H, W)
    sheared = grid.clone()
    sheared[:, 1] += torch.linspace(0, 0.1, W, device=DEV)
    monkeypatch.setenv("PD_CHECK_CONTRACT", "1")
    with pytest.raises(ValueError):
        decoder_tail.fused_plane_geometry({}, sheared, residual, no_levels=4, xz_levels=3, disp_min=2.0, disp_max=30.0, **XZ)
