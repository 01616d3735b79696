"""Generate the golden vectors under tests/golden/ from the REFERENCE ITSELF.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden.py

It imports the reference's ``trainer.py`` / ``layers.py`` from where they lie
(see ref_import.py), drives the unbound methods ``Trainer.pred_novel_images``,
``Trainer.compute_losses`` and ``Trainer.compute_reprojection_loss`` plus the
``layers`` modules on seeded synthetic inputs, and stores inputs + every output +
every gradient as small ``.npz`` fixtures, and full-size (192x640x49) cases as
scalar known answers in ``kat_fullsize.json``.  Only data is written — no
reference source text.

``--only-live`` writes just the vectors of tests/test_oracle_vs_reference.py
(``live_<i>.npz``, ``add_flip_right_inputs.npz``, ``pair_transforms.npz``);
``--check`` writes nothing and checks what only the reference itself can tell
(the committed fixtures are current; see ``check_against_reference``).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_import import load_reference, make_trainer_namespace  # noqa: E402


from planedepth_amd.synthetic import build_case, intrinsics, small_pose, survey_fullsize_case  # noqa: E402,F401


class record_inverse:
    """Context manager: every matrix ``torch.inverse`` returns while it is active, in call order.  The reference forms
    ``H_t2s = torch.inverse(H_s2t)`` inside ``HomographyWarp.forward`` (layers.py:219) and nowhere else on the path, so what
    is recorded around ``Trainer.pred_novel_images`` is the H_t2s THE REFERENCE COMPUTED, one [B*N,3,3] block per target side —
    stored in the fixtures so that the HIP kernels can be held to 1e-4 against the reference's outputs on the reference's own
    matrices (an fp32 inverse at cond 1e3-1e4 differs between LAPACK, rocSOLVER and a hand-written adjugate by more than that)."""

    def __enter__(self):
        self.got, self._orig = [], torch.inverse

        def spy(x, *a, **k):
            r = self._orig(x, *a, **k)
            self.got.append(r.detach().clone())
            return r
        torch.inverse = spy
        return self

    def __exit__(self, *exc):
        torch.inverse = self._orig
        return False


def run_reference(ref, case, *, warp_type="disp_warp", target_side="r", use_mixture_loss=True, automask=False,
                  render_probability=False):
    B, N, H, W = case["logits"].shape
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    logits, sigma, disp_pp = leaf(case["logits"]), leaf(case["sigma"]), leaf(case["disp_pp"])
    Rt = leaf(case["Rt"])
    disp_layered = disp_pp.expand(-1, -1, H, W) * case["row_gain"]
    distance = 0.1 * 0.58 * W / disp_pp[:, :, 0, 0]
    norm = torch.tensor([0.0, 0.0, 1.0])[None, None].expand(B, N, -1)
    inputs = {("color", "l"): case["color_l"], ("color", target_side): case["color_r"],
              "K": case["K"], "inv_K": case["inv_K"], ("Rt", target_side): Rt}
    inputs[("color", "l")] = case["color_l"]
    prob = torch.softmax(logits.detach(), 1)
    outputs = {"probability": prob, "logits": logits, "sigma": sigma, "disp_layered": disp_layered,
               "padding_mask": case["padding_mask"], "distance": distance, "norm": norm,
               ("Rt", target_side): Rt,
               "disp": (prob * disp_layered.detach()).sum(1, True)}
    if "mask_novel" in case:
        outputs["mask_novel"] = case["mask_novel"]
    if render_probability:
        outputs["dists"] = case["dists"]
    ns = make_trainer_namespace(ref, H, W, warp_type=warp_type, use_mixture_loss=use_mixture_loss, automask=automask,
                                render_probability=render_probability, target_sides=[target_side])
    Trainer = ref.trainer.Trainer
    with record_inverse() as rec:
        Trainer.pred_novel_images(ns, inputs, outputs)
    losses = Trainer.compute_losses(ns, inputs, outputs)
    rgb_rec = outputs[("rgb_rec", target_side)]
    objective = losses["loss/ph_loss"] + (rgb_rec * case["g_rgb_rec"]).sum()
    objective.backward()
    res = {
        "rgb_rec": rgb_rec, "ph_loss": losses["loss/ph_loss"], "smooth_loss": losses["loss/smooth_loss"],
        "total_loss": losses["loss/total_loss"],
        "rgb_rec_layered": outputs[("rgb_rec_layered", target_side)], "logit_rec": outputs[("logit_rec", target_side)],
        "probability_rec": outputs[("probability_rec", target_side)],
        "g_logits": logits.grad, "g_sigma": sigma.grad if sigma.grad is not None else torch.zeros_like(sigma),
        "g_disp_pp": disp_pp.grad if disp_pp.grad is not None else torch.zeros_like(disp_pp),
        "g_Rt": Rt.grad if Rt.grad is not None else torch.zeros_like(Rt),
    }
    if use_mixture_loss:
        res["sigma_rec"] = outputs[("sigma_rec", target_side)]
        res["pi_rec"] = outputs[("pi_rec", target_side)]
    if warp_type == "homography_warp":
        assert len(rec.got) == 1 and tuple(rec.got[0].shape) == (B * N, 3, 3)
        res["H_t2s"] = rec.got[0]                       # the reference's own fp32 torch.inverse (layers.py:219)
    return {k: v.detach() for k, v in res.items()}


SMALL_CASES = [
    # name, build kwargs, run kwargs
    ("disp_mix_r", dict(B=2, N=5, H=8, W=16, seed=11, disp_min=0.5, disp_max=9.0), dict()),
    ("disp_mix_l", dict(B=2, N=5, H=8, W=16, seed=12, disp_min=0.5, disp_max=9.0), dict(target_side="l")),
    ("disp_mix_automask", dict(B=2, N=5, H=8, W=16, seed=13, disp_min=0.5, disp_max=9.0), dict(automask=True)),
    ("disp_l1", dict(B=2, N=5, H=8, W=16, seed=14, disp_min=0.5, disp_max=9.0), dict(use_mixture_loss=False)),
    ("disp_l1_automask", dict(B=1, N=6, H=9, W=20, seed=15, disp_min=0.5, disp_max=9.0),
     dict(use_mixture_loss=False, automask=True)),
    ("disp_mix_xz", dict(B=2, N=7, H=12, W=20, seed=16, disp_min=0.5, disp_max=12.0, n_xz=3), dict()),
    ("disp_mix_oob", dict(B=1, N=6, H=8, W=16, seed=17, disp_min=2.0, disp_max=40.0), dict()),  # planes fully out of view (F9)
    ("disp_mix_integer_d", dict(B=1, N=6, H=8, W=24, seed=18, disp_min=1.0, disp_max=8.0,
                                special_disp=[0.0, 1.0, 2.0, 1.9999999, 3.0000002, 7.5]), dict()),
    ("disp_mix_masknovel", dict(B=2, N=5, H=8, W=16, seed=19, disp_min=0.5, disp_max=9.0, with_mask_novel=True), dict()),
    ("disp_l1_masknovel", dict(B=2, N=5, H=8, W=16, seed=20, disp_min=0.5, disp_max=9.0, with_mask_novel=True),
     dict(use_mixture_loss=False)),
    ("homo_mix_stereo", dict(B=2, N=5, H=8, W=16, seed=21, disp_min=0.5, disp_max=9.0), dict(warp_type="homography_warp")),
    ("homo_mix_pose", dict(B=2, N=5, H=12, W=20, seed=22, disp_min=0.5, disp_max=9.0, stereo_T=False),
     dict(warp_type="homography_warp", automask=True)),
    ("homo_l1_pose", dict(B=1, N=4, H=12, W=20, seed=23, disp_min=0.5, disp_max=9.0, stereo_T=False),
     dict(warp_type="homography_warp", use_mixture_loss=False)),
    ("disp_mix_render", dict(B=2, N=5, H=8, W=16, seed=24, disp_min=0.5, disp_max=9.0, render_probability=True),
     dict(render_probability=True)),
]

# tests/test_oracle_vs_reference.py: fresh seeds, away from SMALL_CASES' sizes, stored as live_<i>.npz (same layout)
LIVE_CASES = [
    (dict(B=2, N=6, H=10, W=24, seed=101, disp_min=0.5, disp_max=14.0), dict()),
    (dict(B=1, N=9, H=16, W=32, seed=102, disp_min=0.5, disp_max=20.0, n_xz=3), dict(automask=True)),
    (dict(B=2, N=5, H=10, W=24, seed=103, disp_min=0.5, disp_max=9.0, stereo_T=False),
     dict(warp_type="homography_warp")),
    (dict(B=1, N=5, H=10, W=24, seed=104, disp_min=0.5, disp_max=9.0), dict(use_mixture_loss=False, target_side="l")),
    (dict(B=1, N=5, H=10, W=24, seed=105, disp_min=0.5, disp_max=9.0, render_probability=True),
     dict(render_probability=True, automask=True)),
]


def flip_inputs(seed=8, B=2, H=6, W=10):
    """The batch Trainer.add_flip_right_inputs is fed in tests/test_oracle_vs_reference.py (seeded: rebuilt there)."""
    g = torch.Generator().manual_seed(seed)
    inputs = {(k, s): torch.rand(B, 3, H, W, generator=g) for k in ("color", "color_aug") for s in ("l", "r", 1)}
    inputs.update({("depth_gt", s): torch.rand(B, 1, H, W, generator=g) for s in ("l", "r")})
    inputs["grid"] = torch.randn(B, 2, H, W, generator=g)
    inputs.update({k: torch.randn(B, 4, 4, generator=g) for k in ("K", "inv_K", ("Rt", "l"), ("Rt", "r"))})
    return inputs


def flip_vectors(ref):
    """trainer.py:252-276 on flip_inputs(): every output tensor as key_<i>, the dict keys (tuples as lists) in `meta`."""
    import types
    ns = types.SimpleNamespace(opt=types.SimpleNamespace(novel_frame_ids=[1]))
    want = ref.trainer.Trainer.add_flip_right_inputs(ns, flip_inputs())
    keys = list(want)
    out = {"key_%d" % i: want[k].numpy() for i, k in enumerate(keys)}
    out["meta"] = np.frombuffer(json.dumps([list(k) if isinstance(k, tuple) else k for k in keys]).encode(), dtype=np.uint8)
    return out


PAIR_H, PAIR_W, PAIR_FH, PAIR_FW, PAIR_SEED = 24, 80, 60, 200, 5


def pair_transform_vectors(ref):
    """The crop grids of datasets/pair_transforms.py: Resize((H, W)) of a 37x123 pair, and RandomResizeCrop((H, W),
    factor=(0.75, 1.5)) of a FHxFW pair with numpy's and python's generators seeded PAIR_SEED (the test replays the draws)."""
    import importlib
    import random
    pt = importlib.import_module("datasets.pair_transforms")
    H, W, FH, FW = PAIR_H, PAIR_W, PAIR_FH, PAIR_FW
    out = pt.Resize((H, W))({("color", "r", -1): torch.rand(3, 37, 123), ("color", "l", -1): torch.rand(3, 37, 123)})
    resize_grid = out["grid"]
    src = {("color", "r", -1): torch.rand(3, FH, FW), ("color", "l", -1): torch.rand(3, FH, FW)}
    np.random.seed(PAIR_SEED)
    random.seed(PAIR_SEED)
    out = pt.RandomResizeCrop((H, W), factor=(0.75, 1.5))(dict(src))
    return {"resize_grid": resize_grid.numpy(), "random_resize_crop_grid": out["grid"].numpy()}


def check_against_reference(ref):
    """What needs the reference tree itself and so is no test: the committed decoder-tail and post-process fixtures are
    what the reference produces now (stale fixtures), and the reference's DepthDecoder raises with render_probability
    (networks/depth_decoder.py:94-95, 259: the dispconv has all_levels - 1 channels, `logits * padding_mask` does not
    broadcast), which is why --render_probability is served for PladeNet's outputs only."""
    for fname, fresh in (("decoder_tail.npz", decoder_tail_vectors(ref)), ("post_process.npz", post_process_vectors(ref))):
        stored = np.load(os.path.join(HERE, fname))
        assert set(stored.files) == set(fresh), fname
        for k in stored.files:
            np.testing.assert_allclose(stored[k], fresh[k], rtol=1e-6, atol=1e-7, err_msg="%s:%s" % (fname, k))
    B, H, W = 1, 64, 64
    for xz in (0, 2):
        dec = ref.networks.DepthDecoder([64, 64, 128, 256, 512], use_denseaspp=False, no_levels=4, xz_levels=xz,
                                        use_mixture_loss=True, render_probability=True)
        feats = [torch.randn(B, c, H >> (i + 1), W >> (i + 1)) for i, c in enumerate([64, 64, 128, 256, 512])]
        ys = torch.linspace(-1, 1, H)[None, None, :, None].expand(B, 1, H, W)
        xs = torch.linspace(-1, 1, W)[None, None, None, :].expand(B, 1, H, W)
        try:
            dec(feats, torch.cat([xs, ys], 1).contiguous())
        except RuntimeError as e:
            assert "must match the size" in str(e), e
        else:
            raise AssertionError("the reference DepthDecoder ran with render_probability (xz_levels=%d)" % xz)
    print("check: fixtures current, DepthDecoder + render_probability raises")


def write_live_vectors(ref):
    for i, (bkw, rkw) in enumerate(LIVE_CASES):
        case = build_case(**bkw)
        res = run_reference(ref, case, **rkw)
        blob = {"in_" + k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in case.items()}
        blob.update({"out_" + k: v.numpy() for k, v in res.items()})
        blob["meta"] = np.frombuffer(json.dumps(dict(build=bkw, run=rkw)).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, "live_%d.npz" % i), **blob)
    np.savez_compressed(os.path.join(HERE, "add_flip_right_inputs.npz"), **flip_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "pair_transforms.npz"), **pair_transform_vectors(ref))


FULL_CASES = [
    ("full_disp_mix", dict(), dict()),
    ("full_disp_l1", dict(), dict(use_mixture_loss=False)),
    ("full_homo_mix", dict(), dict(warp_type="homography_warp")),
    ("full_disp_mix_automask", dict(), dict(automask=True)),
]


def module_vectors(ref):
    """Direct calls of the reference's layers (rows A3, A4, A9, A10, smoothness)."""
    g = torch.Generator().manual_seed(77)
    B, N, H, W = 2, 3, 10, 14
    out = {}
    K, inv_K = intrinsics(B, H, W)
    depth = torch.rand(B, 1, H, W, generator=g) * 5 + 0.5
    T = small_pose(g, B, rot=0.05, trans=0.2)
    bp = ref.layers.BackprojectDepth(H, W)
    pj = ref.layers.Project3D(H, W)
    cam = bp(depth, inv_K)
    out.update(bp_depth=depth, bp_K=K, bp_inv_K=inv_K, bp_T=T, bp_cam=cam, pj_grid=pj(cam, K, T))
    hw = ref.layers.HomographyWarp(H, W)
    d = torch.rand(B, N, generator=g) * 4 + 0.3
    n = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    ex = lambda M: M[:, None].expand(-1, N, -1, -1).reshape(B * N, 4, 4)  # noqa: E731
    hgrid, hmask = hw(d, n, ex(T), ex(K), ex(inv_K))
    out.update(hw_d=d, hw_n=n, hw_grid=hgrid, hw_mask=hmask.float())
    x = torch.rand(B, 3, H, W, generator=g)
    y = (x + 0.2 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    xr = x.clone().requires_grad_(True)
    ssim_mod = ref.layers.SSIM()
    s = ssim_mod(xr, y)
    ns = make_trainer_namespace(ref, H, W, use_ssim=True)
    rl = ref.trainer.Trainer.compute_reprojection_loss(ns, xr, y)
    gw = torch.rand(B, 1, H, W, generator=g)
    (rl * gw).sum().backward()
    ns2 = make_trainer_namespace(ref, H, W, use_ssim=False)
    out.update(ssim_x=x, ssim_y=y, ssim_out=s, reproj_ssim=rl, reproj_gw=gw, reproj_g_pred=xr.grad,
               reproj_l1=ref.trainer.Trainer.compute_reprojection_loss(ns2, x, y))
    err = torch.rand(B, N, H, W, generator=g)
    sg = torch.rand(B, N, H, W, generator=g).clamp(0.01, 1)
    pi = torch.softmax(torch.randn(B, N, H, W, generator=g), 1)
    out.update(mm_err=err, mm_sigma=sg, mm_pi=pi, mm_lap=ref.layers.multimodal_loss(err, sg, pi, dist="lap"),
               mm_gauss=ref.layers.multimodal_loss(err, sg, pi), lap=ref.layers.laplacian(err, sg),
               gauss=ref.layers.gaussian(err, sg))
    disp = torch.rand(B, 1, H, W, generator=g)
    out.update(sm_disp=disp, sm_img=x, sm_loss=ref.layers.get_smooth_loss_disp(disp, x, gamma=2))
    # border-mode grid_sample as used by pred_self_images (trainer.py:624-628)
    grid = pj(cam, K, T)
    out.update(gs_border=torch.nn.functional.grid_sample(x, grid, padding_mode="border", align_corners=True),
               gs_zeros=torch.nn.functional.grid_sample(x, grid, padding_mode="zeros", align_corners=True))
    return {k: v.detach().numpy() for k, v in out.items()}


def decoder_tail_vectors(ref):
    """The reference DepthDecoder's own tail (networks/depth_decoder.py:256-291) on prescribed conv outputs: forward hooks
    replace what dispconv / sigmaconv return by seeded leaf tensors, everything after them is the reference's code."""
    out = {}
    g = torch.Generator().manual_seed(4242)
    H, W, B = 64, 64, 1   # smallest the decoder's five stride-2 levels accept (reflection pad at H/32)
    for tag, kw in (("mix_xz", dict(no_levels=4, xz_levels=2, use_mixture_loss=True, plane_residual=True)),
                    ("mix_xy", dict(no_levels=5, xz_levels=0, use_mixture_loss=True, plane_residual=True)),
                    ("l1_xy", dict(no_levels=4, xz_levels=0, use_mixture_loss=False, plane_residual=False))):
        torch.manual_seed(11)
        dec = ref.networks.DepthDecoder([64, 64, 128, 256, 512], use_denseaspp=False, **kw)
        N = kw["no_levels"] + kw["xz_levels"]
        feats = [torch.randn(B, c, H >> (i + 1), W >> (i + 1), generator=g) * 0.5
                 for i, c in enumerate([64, 64, 128, 256, 512])]
        raw_logits = (torch.randn(B, N, H, W, generator=g) * 3).requires_grad_(True)
        raw_sigma = (torch.randn(B, N, H, W, generator=g) * 3.5 - 1.0).requires_grad_(True)  # both clamp bounds are hit
        dec.convs["dispconv"].register_forward_hook(lambda m, i, o: raw_logits)
        if kw["use_mixture_loss"]:
            dec.convs["sigmaconv"].register_forward_hook(lambda m, i, o: raw_sigma)
        ys = torch.linspace(-1, 1, H)[None, None, :, None].expand(B, 1, H, W)
        xs = torch.linspace(-1, 1, W)[None, None, None, :].expand(B, 1, H, W)
        grid = torch.cat([xs, ys], 1).contiguous()
        o = dec(feats, grid)
        if o["disp_layered"].requires_grad:  # only with plane_residual (the levels are constants otherwise)
            o["disp_layered"].retain_grad()
        gw_l = torch.randn(B, N, H, W, generator=g)
        gw_s = torch.randn(B, N, H, W, generator=g)
        gw_d = torch.randn(B, 1, H, W, generator=g)
        gw_z = torch.randn(B, 1, H, W, generator=g) * 0.1
        obj = (o["logits"] * gw_l).sum() + (o["disp"] * gw_d).sum() + (o["depth"] * gw_z).sum()
        if kw["use_mixture_loss"]:
            obj = obj + (o["sigma"] * gw_s).sum()
        obj.backward()
        blob = dict(raw_logits=raw_logits, raw_sigma=raw_sigma, padding_mask=o["padding_mask"].float(),
                    disp_layered=o["disp_layered"], logits=o["logits"], probability=o["probability"], disp=o["disp"],
                    depth=o["depth"], gw_logits=gw_l, gw_sigma=gw_s, gw_disp=gw_d, gw_depth=gw_z,
                    g_raw_logits=raw_logits.grad)
        if o["disp_layered"].grad is not None:
            blob.update(g_disp_layered=o["disp_layered"].grad)
        if kw["use_mixture_loss"]:
            blob.update(sigma=o["sigma"], pi=o["pi"], g_raw_sigma=raw_sigma.grad)
        out.update({"%s/%s" % (tag, k): v.detach().numpy() for k, v in blob.items()})
        out["%s/mixture" % tag] = np.asarray(int(kw["use_mixture_loss"]))
        print("decoder_tail %-8s disp mean %.5f" % (tag, float(o["disp"].detach().mean())))
    return out


def plade_tail_vectors(ref):
    """The reference PladeNet's own tail (networks/plade_net.py:277-341) with --render_probability: forward hooks replace
    what conv0 (the N-1 logit channels) and conv_sigma return by seeded leaf tensors, everything after them — plane levels
    with the learnt residual, depth-layer distances scaled by the camera rays, alpha compositing, mixture weights, disp,
    depth — is the reference's code.  The backbone runs on a seeded image but its output is discarded by the hooks."""
    out = {}
    g = torch.Generator().manual_seed(777)
    H, W, B = 32, 64, 1
    for tag, kw in (("mix_xy", dict(no_levels=6, xz_levels=0, use_mixture_loss=True, plane_residual=True)),
                    ("mix_xz", dict(no_levels=4, xz_levels=3, use_mixture_loss=True, plane_residual=True)),
                    ("l1_xy", dict(no_levels=5, xz_levels=0, use_mixture_loss=False, plane_residual=False))):
        torch.manual_seed(23)
        net = ref.networks.PladeNet(False, kw["no_levels"], 2.0, 300.0 * W / 640.0, xz_levels=kw["xz_levels"],
                                    use_mixture_loss=kw["use_mixture_loss"], render_probability=True,
                                    plane_residual=kw["plane_residual"])
        N = kw["no_levels"] + kw["xz_levels"]
        raw_logits = (torch.randn(B, N - 1, H, W, generator=g) * 1.5).requires_grad_(True)   # relu(): about half are inactive
        raw_sigma = (torch.randn(B, N, H, W, generator=g) * 3.5 - 1.0).requires_grad_(True)  # both clamp bounds are hit
        net.conv0.register_forward_hook(lambda m, i, o: raw_logits)
        if kw["use_mixture_loss"]:
            net.conv_sigma.register_forward_hook(lambda m, i, o: raw_sigma)
        image = torch.rand(B, 3, H, W, generator=g)
        ys = torch.linspace(0.3, 1, H)[None, None, :, None].expand(B, 1, H, W)   # below the horizon: ground planes in front
        xs = torch.linspace(-1, 1, W)[None, None, None, :].expand(B, 1, H, W)
        grid = torch.cat([xs, ys], 1).contiguous()
        o = net(image, grid)
        if o["disp_layered"].requires_grad:
            o["disp_layered"].retain_grad()
        gw_l = torch.randn(B, N, H, W, generator=g)
        gw_t = torch.randn(B, N - 1, H, W, generator=g) * 0.05
        gw_s = torch.randn(B, N, H, W, generator=g)
        gw_d = torch.randn(B, 1, H, W, generator=g)
        gw_z = torch.randn(B, 1, H, W, generator=g) * 0.1
        obj = (o["logits"] * gw_l).sum() + (o["dists"] * gw_t).sum() + (o["disp"] * gw_d).sum() + (o["depth"] * gw_z).sum()
        if kw["use_mixture_loss"]:
            obj = obj + (o["sigma"] * gw_s).sum()
        obj.backward()
        blob = dict(raw_logits=raw_logits, raw_sigma=raw_sigma, disp_layered=o["disp_layered"], logits=o["logits"],
                    dists=o["dists"], probability=o["probability"], disp=o["disp"], depth=o["depth"],
                    gw_logits=gw_l, gw_dists=gw_t, gw_sigma=gw_s, gw_disp=gw_d, gw_depth=gw_z,
                    g_raw_logits=raw_logits.grad, ray_norm=torch.linalg.norm(ref.layers.create_camera_plane(H, W), dim=1))
        if o["disp_layered"].grad is not None:
            blob.update(g_disp_layered=o["disp_layered"].grad)
        if kw["use_mixture_loss"]:
            blob.update(sigma=o["sigma"], pi=o["pi"], g_raw_sigma=raw_sigma.grad)
        out.update({"%s/%s" % (tag, k): v.detach().numpy() for k, v in blob.items()})
        out["%s/mixture" % tag] = np.asarray(int(kw["use_mixture_loss"]))
        print("plade_tail %-8s disp mean %.5f" % (tag, float(o["disp"].detach().mean())))
    return out


def post_process_vectors(ref):
    """Trainer.generate_post_process_disp (trainer.py:404-466) with the fixed networks replaced by a stub that returns
    prescribed decoder outputs for the batch cat([image, mirrored image])."""
    import types
    g = torch.Generator().manual_seed(909)
    out = {}
    for tag, (B, N, H, W, dense) in (("xy", (2, 6, 10, 48, False)), ("rows", (1, 5, 9, 70, True))):
        logits = torch.randn(2 * B, N, H, W, generator=g) * 2
        sigma = torch.rand(2 * B, N, H, W, generator=g) * 0.9 + 0.05
        w = torch.softmax(logits, 1) / sigma
        probability = w / w.sum(1, True)
        levels = torch.arange(N, dtype=torch.float32)[None, :, None, None] + torch.rand(2 * B, N, 1, 1, generator=g) - 0.5
        disp_layered = (0.4 * W) * (1.0 / (0.4 * W)) ** (levels / (N - 1))
        disp_layered = disp_layered.expand(-1, -1, H, W)
        if dense:  # row-dependent disparities as xz planes give
            disp_layered = disp_layered * (0.5 + torch.linspace(0, 1, H)[None, None, :, None])
        disp = (probability * disp_layered).sum(1, True)
        fixed = dict(logits=logits, probability=probability, disp=disp, disp_layered=disp_layered)
        ns = types.SimpleNamespace()
        ns.opt = types.SimpleNamespace(num_ep=1, net_type="ResNet")
        ns.softmax = torch.nn.Softmax(1)
        ns.fixed_models = {"encoder": lambda x: None, "depth": lambda f, gr: fixed}
        color = torch.rand(B, 3, H, W, generator=g)
        inputs = {("color_aug", "l"): color, "grid": torch.zeros(B, 2, H, W)}
        disp_pp, mask_novel = ref.trainer.Trainer.generate_post_process_disp(ns, inputs)
        out.update({"%s/%s" % (tag, k): v.detach().numpy() for k, v in
                    dict(fixed, disp_pp=disp_pp, mask_novel=mask_novel).items()})
        print("post_process %-5s disp_pp mean %.5f mask_novel mean %.5f" % (tag, float(disp_pp.mean()), float(mask_novel.mean())))
    return out


def trainer_mono_vectors(ref):
    """BASELINE configs[3] as the trainer runs it (trainer.py:325-356): the reference DepthDecoder WITH xz planes
    (non-frontal normals, horizon mask, per-plane distances: networks/depth_decoder.py:158-207) -> Trainer.predict_poses
    (:358-402, pose nets replaced by a stub that returns seeded axis-angles: F8 zero translation, Rt[3,3] = 0) ->
    Trainer.pred_novel_images over ALL target sides -> Trainer.compute_losses (incl. `losses /= len(target_sides)` before
    the smoothness term, :765-771).  Stored: the decoder outputs / poses the hot path consumes, every rgb_rec, the loss
    dict and the gradients w.r.t. logits, sigma, distance / disp_layered and every Rt."""
    import types
    from planedepth_amd.synthetic import crop_grid, dataset_intrinsics
    out = {}
    H, W, B = 64, 64, 2
    configs = (
        ("homo3", dict(warp_type="homography_warp", target_sides=["r", -1, 1], automask=True, use_mixture_loss=True)),
        ("homo_nostereo_l1", dict(warp_type="homography_warp", target_sides=[-1, 1], automask=True, use_mixture_loss=False)),
        ("disp_xz", dict(warp_type="disp_warp", target_sides=["r"], automask=False, use_mixture_loss=True)),
    )
    for ci, (tag, cfg) in enumerate(configs):
        g = torch.Generator().manual_seed(5150 + ci)
        mix = cfg["use_mixture_loss"]
        no_levels, xz_levels = 4, 3
        N = no_levels + xz_levels
        torch.manual_seed(23 + ci)
        dec = ref.networks.DepthDecoder([64, 64, 128, 256, 512], use_denseaspp=False, no_levels=no_levels,
                                        xz_levels=xz_levels, disp_min=0.5, disp_max=0.3 * W, use_mixture_loss=mix,
                                        plane_residual=True)
        feats = [torch.randn(B, c, H >> (i + 1), W >> (i + 1), generator=g) * 0.5
                 for i, c in enumerate([64, 64, 128, 256, 512])]
        raw_logits = (torch.randn(B, N, H, W, generator=g) * 2).requires_grad_(True)
        raw_sigma = (torch.randn(B, N, H, W, generator=g) * 2.0 - 0.5).requires_grad_(True)
        dec.convs["dispconv"].register_forward_hook(lambda m, i, o, t=raw_logits: t)
        if mix:
            dec.convs["sigmaconv"].register_forward_hook(lambda m, i, o, t=raw_sigma: t)
        # two different random crops of a resized KITTI-like frame: the principal point is off-centre, so the xz planes'
        # normal [0, 1, py_cy_fys] / |.| is not frontal and the horizon row differs per sample
        grid = torch.stack([crop_grid(H, W, 96, 150, 20, 50), crop_grid(H, W, 110, 170, 6, 90)], 0)
        o = dec(feats, grid)
        outputs = dict(o)
        for k in ("logits", "sigma", "distance", "disp_layered"):
            if k in outputs and outputs[k].requires_grad:
                outputs[k].retain_grad()
        outputs["disp"] = o["disp"].detach()   # the smoothness term's path into the decoder tail is not part of this fixture
        K, inv_K = dataset_intrinsics(B, H, W)
        Rt_r = torch.eye(4)[None].repeat(B, 1, 1)
        Rt_r[:, 0, 3] = -0.1
        Rt_r.requires_grad_(True)
        inputs = {"grid": grid, "K": K, "inv_K": inv_K, ("Rt", "r"): Rt_r}
        for s in ("l", "r", -1, 1):
            inputs[("color", s)] = torch.rand(B, 3, H, W, generator=g)
            inputs[("color_aug", s)] = inputs[("color", s)]
        novel = [s for s in cfg["target_sides"] if s != "r"]
        ns = make_trainer_namespace(ref, H, W, warp_type=cfg["warp_type"], use_mixture_loss=mix, automask=cfg["automask"],
                                    target_sides=cfg["target_sides"], novel_frame_ids=novel, use_colmap=False)
        pose_leafs = {}

        class PoseStub:
            def __init__(self):
                self.calls = 0

            def __call__(self, feats_, grid_):
                f = novel[self.calls]
                self.calls += 1
                aa = (torch.randn(B, 1, 1, 3, generator=g) * 0.02).requires_grad_(True)
                tr = (torch.randn(B, 1, 1, 3, generator=g) * 0.05).requires_grad_(True)
                pose_leafs[f] = (aa, tr)
                return aa, tr

        ns.models = {"pose_encoder": lambda x: x, "pose": PoseStub()}
        Trainer = ref.trainer.Trainer
        outputs.update(Trainer.predict_poses(ns, inputs))
        for f in novel:
            outputs[("Rt", f)].retain_grad()
        with record_inverse() as rec:
            Trainer.pred_novel_images(ns, inputs, outputs)
        losses = Trainer.compute_losses(ns, inputs, outputs)
        gw = {s: torch.randn(B, 3, H, W, generator=g) * 1e-3 for s in cfg["target_sides"]}
        obj = losses["loss/total_loss"] + sum((outputs[("rgb_rec", s)] * gw[s]).sum() for s in cfg["target_sides"])
        obj.backward()
        blob = dict(grid=grid, K=K, inv_K=inv_K, logits=outputs["logits"], disp_layered=outputs["disp_layered"],
                    padding_mask=outputs["padding_mask"].float(), distance=outputs["distance"], norm=outputs["norm"],
                    disp=outputs["disp"], ph_loss=losses["loss/ph_loss"], total_loss=losses["loss/total_loss"],
                    smooth_loss=losses["loss/smooth_loss"], g_logits=outputs["logits"].grad)
        if mix:
            blob.update(sigma=outputs["sigma"], g_sigma=outputs["sigma"].grad)
        if cfg["warp_type"] == "homography_warp":
            blob.update(g_distance=outputs["distance"].grad)
        else:
            blob.update(g_disp_layered=outputs["disp_layered"].grad)
        for s in ("l", "r", -1, 1):
            blob["color_%s" % s] = inputs[("color", s)]
        for s in cfg["target_sides"]:
            Rt = outputs[("Rt", s)]
            blob["Rt_%s" % s] = Rt
            gR = Rt.grad if Rt.grad is not None else torch.zeros_like(Rt)
            blob["g_Rt_%s" % s] = gR
            blob["gw_%s" % s] = gw[s]
            blob["rgb_rec_%s" % s] = outputs[("rgb_rec", s)]
        if cfg["warp_type"] == "homography_warp":   # the reference's own H_t2s, one block per target side in loop order (trainer.py:532)
            assert len(rec.got) == len(cfg["target_sides"])
            for s, Hm in zip(cfg["target_sides"], rec.got):
                assert tuple(Hm.shape) == (B * N, 3, 3)
                blob["H_t2s_%s" % s] = Hm
        out.update({"%s/%s" % (tag, k): v.detach().numpy() for k, v in blob.items()})
        out["%s/meta" % tag] = np.frombuffer(json.dumps(dict(cfg, no_levels=no_levels, xz_levels=xz_levels)).encode(),
                                             dtype=np.uint8)
        print("trainer_mono %-18s ph=%.8f total=%.8f masked=%.3f norm_xz=%s" % (
            tag, float(losses["loss/ph_loss"]), float(losses["loss/total_loss"]),
            float(1 - outputs["padding_mask"].float().mean()), outputs["norm"][0, -1].tolist()))
    return out


def pipeline_vectors(ref):
    """inputs["grid"] as the reference's own transforms make it (datasets/pair_transforms.py: RandomResizeCrop :27-37,
    Resize :63-68), with the crop parameters recovered by replaying the transform's random draws.  Fixture for the
    on-device grid kernel."""
    import importlib
    import random
    pt = importlib.import_module("datasets.pair_transforms")
    out = {}
    cases = [("kitti_192x640", (192, 640), (375, 1242), (0.75, 1.5), 11), ("small_24x80", (24, 80), (60, 200), (0.75, 1.5), 5),
             ("hr_384x1280", (384, 1280), (375, 1242), (1.05, 1.5), 3), ("odd_17x33", (17, 33), (41, 97), (0.5, 2.0), 9)]
    for tag, (H, W), (FH, FW), fac, seed in cases:
        np.random.seed(seed); random.seed(seed)
        src = {("color", "r", -1): torch.rand(3, FH, FW), ("color", "l", -1): torch.rand(3, FH, FW)}
        res = pt.RandomResizeCrop((H, W), factor=fac)(dict(src))
        np.random.seed(seed); random.seed(seed)
        fmin = max(max((H + 1) / FH, (W + 1) / FW), fac[0])
        factor = np.random.uniform(low=fmin, high=fac[1])
        h0 = random.randint(0, int(FH * factor - H)); w0 = random.randint(0, int(FW * factor - W))
        out[tag + "/params"] = np.asarray([int(FW * factor), int(FH * factor), w0, h0], dtype=np.int32)
        out[tag + "/grid"] = res["grid"].numpy()
        out[tag + "/hw"] = np.asarray([H, W], dtype=np.int32)
    H, W = 24, 80
    res = pt.Resize((H, W))({("color", "r", -1): torch.rand(3, 37, 123), ("color", "l", -1): torch.rand(3, 37, 123)})
    out["resize_24x80/params"] = np.asarray([W, H, 0, 0], dtype=np.int32)
    out["resize_24x80/grid"] = res["grid"].numpy()
    out["resize_24x80/hw"] = np.asarray([H, W], dtype=np.int32)
    return out


def fullsize_pinned_homography(ref):
    """192 x 640 x 63 planes, a pose with rotation AND translation (one homography per plane), mixture + automask: the
    reference's own H_t2s [63,3,3] plus what the reference computed from them — scalars, rgb_rec in full, the gradients on a
    stride-8 lattice — so that the per-plane homography kernels are pinned at the benchmark size to the reference's outputs
    on the reference's matrices.  Inputs are regenerated from the seed by whoever reads this (survey_fullsize_case)."""
    case = survey_fullsize_case(B=1, N=63, sigma_interior=True)
    case["Rt"] = small_pose(torch.Generator().manual_seed(77), 1)
    res = run_reference(ref, case, warp_type="homography_warp", automask=True)
    sub = lambda t: t[..., ::8, ::8].contiguous()  # noqa: E731
    blob = dict(Rt=case["Rt"], H_t2s=res["H_t2s"], rgb_rec=res["rgb_rec"], ph_loss=res["ph_loss"],
                g_logits_sub8=sub(res["g_logits"]), g_sigma_sub8=sub(res["g_sigma"]),
                l1_g_logits=res["g_logits"].double().abs().sum(), l1_g_sigma=res["g_sigma"].double().abs().sum(),
                max_g_logits=res["g_logits"].abs().max(), max_g_sigma=res["g_sigma"].abs().max(),
                sum_rgb_rec=res["rgb_rec"].double().sum())
    print("fullsize_pinned_homography ph=%.8f sum_rgb=%.4f cond(H) up to %.3g" % (
        float(res["ph_loss"]), float(blob["sum_rgb_rec"]), float(torch.linalg.cond(res["H_t2s"].double()).max())))
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in blob.items()}


def scalars(res):
    f = lambda t: float(t.double().sum())  # noqa: E731
    a = lambda t: float(t.double().abs().sum())  # noqa: E731
    return dict(ph_loss=float(res["ph_loss"]), smooth_loss=float(res["smooth_loss"]), total_loss=float(res["total_loss"]),
                sum_rgb_rec=f(res["rgb_rec"]), l1_g_logits=a(res["g_logits"]), l1_g_sigma=a(res["g_sigma"]),
                sum_g_disp_pp=f(res["g_disp_pp"]), l1_g_disp_pp=a(res["g_disp_pp"]), l1_g_Rt=a(res["g_Rt"]))


def main():
    ref = load_reference()
    torch.manual_seed(0)
    if "--only-trainer-mono" in sys.argv:   # add the configs[3] fixtures without touching the others
        np.savez_compressed(os.path.join(HERE, "trainer_mono.npz"), **trainer_mono_vectors(ref))
        return
    if "--only-homography-pins" in sys.argv:   # round 6: the reference's own H_t2s into the homography fixtures (everything else
        # in them is regenerated bit for bit: seeded generators) + the full-size pinned KAT
        for name, bkw, rkw in SMALL_CASES:
            if rkw.get("warp_type") != "homography_warp":
                continue
            case = build_case(**bkw)
            res = run_reference(ref, case, **rkw)
            old = np.load(os.path.join(HERE, name + ".npz"))
            for k in old.files:   # nothing else may move
                if k.startswith("out_"):
                    assert np.array_equal(old[k], res[k[4:]].numpy()), (name, k)
            blob = {"in_" + k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in case.items()}
            blob.update({"out_" + k: v.numpy() for k, v in res.items()})
            blob["meta"] = np.frombuffer(json.dumps(dict(build=bkw, run=rkw)).encode(), dtype=np.uint8)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **blob)
        old = np.load(os.path.join(HERE, "trainer_mono.npz"))
        new = trainer_mono_vectors(ref)
        for k in old.files:
            assert np.array_equal(old[k], new[k]), k
        np.savez_compressed(os.path.join(HERE, "trainer_mono.npz"), **new)
        np.savez_compressed(os.path.join(HERE, "homography_pinned_fullsize.npz"), **fullsize_pinned_homography(ref))
        return
    if "--only-pipeline" in sys.argv:
        np.savez_compressed(os.path.join(HERE, "pipeline.npz"), **pipeline_vectors(ref))
        return
    if "--only-live" in sys.argv:
        write_live_vectors(ref)
        return
    if "--check" in sys.argv:
        check_against_reference(ref)
        return
    for name, bkw, rkw in SMALL_CASES:
        case = build_case(**bkw)
        res = run_reference(ref, case, **rkw)
        blob = {"in_" + k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in case.items()}
        blob.update({"out_" + k: v.numpy() for k, v in res.items()})
        blob["meta"] = np.frombuffer(json.dumps(dict(build=bkw, run=rkw)).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **blob)
        print("%-24s ph=%.8f sum_rgb=%.6f" % (name, float(res["ph_loss"]), float(res["rgb_rec"].sum())))
    np.savez_compressed(os.path.join(HERE, "modules.npz"), **module_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "decoder_tail.npz"), **decoder_tail_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "plade_tail.npz"), **plade_tail_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "post_process.npz"), **post_process_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "trainer_mono.npz"), **trainer_mono_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "pipeline.npz"), **pipeline_vectors(ref))
    np.savez_compressed(os.path.join(HERE, "homography_pinned_fullsize.npz"), **fullsize_pinned_homography(ref))
    write_live_vectors(ref)
    kat = {}
    for name, _, rkw in FULL_CASES:
        case = survey_fullsize_case()
        res = run_reference(ref, case, **rkw)
        kat[name] = dict(run=rkw, **scalars(res))
        print(name, kat[name])
    with open(os.path.join(HERE, "kat_fullsize.json"), "w") as f:
        json.dump(kat, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
