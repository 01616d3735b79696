"""Plane sweep: every kernel route against the fp64 oracle, measured per (b, n, y) ROW (cases.slice_report) instead of per tensor.

Why.  ``g_logits[b,n,y,:]`` and ``g_sigma[b,n,y,:]`` scale with the plane's probability and with how much of the row is in view: the
largest entry of a row goes down to 1.5e-4 (g_logits) and 2e-5 (g_sigma) of the tensor's maximum on stream_130_mix, so under ``rel_err`` (max|a-b| / max|b| of the whole tensor) a
kernel that mishandles a low-probability plane, the last plane of a mask word, a partly visible row or the row under a horizon mask
has thousands of times the parity budget to hide in.  Here every row is measured against its own scale.

The bar (per tensor, against the oracle's fp64 run of the same case; ``err`` = slice_report(...)["err"]):

    err(product) <= 2 * E_ref + 1e-4,   E_ref = err(oracle fp32)          (cases.three_way with err in place of rel_err)

next to the tensor-norm bar of the rest of the suite, taken against fp64 in both modes: rel_err < 1e-4, 2e-4 for the disparity
gradient.  Two conditions keep the bar from
hiding a failure, both proven on the CPU by ``test_conditions_cpu``: E_ref <= E_REF_CAP for every tensor of every case, and
PLANE_FLOOR is the smallest of 1e-3, 1e-2, 1e-1 at which that holds (chosen from the oracle alone; the floor exists because a masked
row next to a live one holds ~1e-6 of its neighbour in the fp32 oracle — the y round trip of the normalised grid — 1e-14 in fp64 and
exactly 0 in the product, whose row kernels drop that cross-row adjoint term: pd_rowgeom.h, two_row_form).

Kink-free cases, no element excluded (one tensor is: see _noise_only).  Every sampling coordinate keeps MARGIN = 0.05 px from an integer (asserted from the fp64 grid), so
the fp32 and the fp64 oracle take the same taps everywhere: disparities with fractional parts in [0.06, 0.94] (per row for ground
planes), homographies from a pure-translation family (R = I, t = (tx, ty, 0), fronto-parallel planes: ix = x + a_n, iy = y + rho a_n,
picked by seeded rejection; the plane-uniform kernels get the same family through the rotation slot, one shift per image).  sigma
stays inside its clamp, no automask case has a zero-disparity plane.

The operators are called directly (``ops.plane_sweep_disp`` / ``ops.plane_sweep_homography`` with ``return_mean=True``), with upstream
gradients the test controls: objective ``(rgb_rec*G1).sum() + (ph_map*G2).sum() + 3*ph_mean``.  Every case also runs the three parts
alone — {mean} alone is the training configuration: ``g_rgb_rec`` and ``g_ph_map`` arrive as None — holds {mean} to the bar above, and
the sum of the three partial results to the joint one (the backward is linear in its upstream gradients: make_pixel_ctx is their only
reader).

PD_SWEEP_PARITY_JSON=<file> writes the worst ``err`` per route and tensor (product and oracle fp32) and E_ref per case: the source
of profiles/sweep_slice_parity.md."""
import ctypes
import json
import math
import os
import zlib
from typing import NamedTuple

import pytest
import torch

from cases import rel_err, slice_report
from oracle import planedepth_oracle as orc

PLANE_FLOOR = 1e-2   # the smallest of 1e-3, 1e-2, 1e-1 at which every case meets E_REF_CAP (test_conditions_cpu; profile)
E_REF_CAP = 2e-3     # the oracle's own fp32 run, per row: measured 2e-5 .. 1e-3
MARGIN = 0.05        # px between any sampling coordinate and the nearest integer
TOL, DISP_TOL = 1e-4, 2e-4
LINEAR_TOL, LINEAR_PLANE_TOL = 3e-6, 5e-5   # test_rowstream_backward_equals_rowshift_backward_and_oracle's figures
W_MEAN = 3.0
COMBOS = ("all", "rgb", "map", "mean")
REPORT = {}      # (route, tensor) -> {"product": worst err, "oracle_fp32": worst E_ref}
E_REF = {}       # case -> {tensor: E_ref}


class Spec(NamedTuple):
    name: str
    kind: str            # "disp" | "homo"
    shape: tuple         # (B, N, H, W)
    impl: str            # AUTO | EXACT_ROWS | ROWS1 | GENERAL | UNIFORM_DIRECT
    mix: bool
    automask: bool
    route: tuple         # (forward family, backward family) the case is meant to reach, from sweep_route's conditions
    side: str = "r"
    render: bool = False
    form: str = "plane"  # disp: plane | rows_view | rows_dense | dense;  homo: planes | uniform
    mask: str = "none"   # none | rows | pixel
    n_xz: int = 0
    g2: str = "rand"     # upstream gradient of ph_map: rand (non-negative) | randn (signed)
    zeros: bool = False  # claims a plane fully out of view AND a masked row band
    draw: int = 0        # which seeded draw of the inputs: moved on where the oracle's own fp32 run exceeds E_REF_CAP
    low_plane: int = -1  # this plane's logits are lowered by 8: a plane of probability ~1e-4 everywhere


SS, RS, RSH, GEN, SC, GA = "segment_stream", "row_stream", "row_shift", "general", "scatter", "gather"
UNI, UST, UDI = "uniform", "uniform_staged", "uniform_direct"

SPECS = [
    # segment-stream forward / row-stream backward: AUTO (and EXACT_ROWS), no per-pixel mask, even width
    Spec("stream_130_mix", "disp", (2, 9, 7, 130), "AUTO", True, False, (SS, RS), mask="rows", zeros=True),
    Spec("stream_130_mix_signed_map", "disp", (2, 9, 7, 130), "AUTO", True, False, (SS, RS), side="l", g2="randn"),
    Spec("stream_130_l1_auto", "disp", (2, 9, 7, 130), "AUTO", False, True, (SS, RS), side="l"),
    Spec("stream_64_mix", "disp", (1, 5, 2, 64), "AUTO", True, False, (SS, RS)),
    Spec("stream_258_l1", "disp", (2, 7, 5, 258), "AUTO", False, False, (SS, RS), side="l"),
    Spec("stream_640_mix_auto", "disp", (1, 12, 4, 640), "AUTO", True, True, (SS, RS), side="l"),
    Spec("stream_1416_l1_auto", "disp", (1, 4, 3, 1416), "AUTO", False, True, (SS, RS)),
    Spec("stream_65planes_mix", "disp", (1, 65, 4, 128), "AUTO", True, False, (SS, RS)),
    Spec("stream_33planes_exact_mix_auto", "disp", (1, 33, 3, 66), "EXACT_ROWS", True, True, (SS, RS)),
    Spec("stream_33planes_low_word_end_mix", "disp", (1, 33, 3, 66), "AUTO", True, False, (SS, RS), low_plane=31),
    Spec("stream_rows_view_mix", "disp", (2, 12, 9, 200), "AUTO", True, False, (SS, RS), form="rows_view", mask="rows", n_xz=4,
         zeros=True, draw=3),
    Spec("stream_rows_dense_l1_auto", "disp", (2, 12, 9, 200), "AUTO", False, True, (SS, RS), side="l", form="rows_dense",
         mask="rows", n_xz=4, zeros=True),
    # segment-stream forward / row-shift backward: alpha compositing under AUTO
    Spec("render_130_mix_auto", "disp", (2, 9, 7, 130), "AUTO", True, True, (SS, RSH), render=True, mask="rows", zeros=True),
    Spec("render_640_l1_auto", "disp", (1, 12, 4, 640), "AUTO", False, True, (SS, RSH), side="l", render=True),
    Spec("render_258_mix", "disp", (2, 7, 5, 258), "AUTO", True, False, (SS, RSH), side="l", render=True, draw=2),
    Spec("render_rows_view_130_mix", "disp", (2, 9, 7, 130), "AUTO", True, False, (SS, RSH), render=True, form="rows_view"),
    # row-shift forward / row-shift backward: odd width under AUTO, PD_IMPL_ROWS1, a per-pixel mask under AUTO
    Spec("odd_257_mix", "disp", (1, 5, 5, 257), "AUTO", True, False, (RSH, RSH)),
    Spec("odd_257_l1_auto", "disp", (1, 5, 5, 257), "AUTO", False, True, (RSH, RSH), side="l"),
    Spec("rows1_130_mix_auto", "disp", (2, 9, 7, 130), "ROWS1", True, True, (RSH, RSH), side="l"),
    Spec("rows1_33planes_l1", "disp", (1, 33, 3, 66), "ROWS1", False, False, (RSH, RSH)),
    Spec("rows1_rows_view_mix", "disp", (2, 12, 9, 200), "ROWS1", True, False, (RSH, RSH), form="rows_view", mask="rows", n_xz=4,
         zeros=True, draw=3),
    Spec("rows1_rows_dense_l1_auto", "disp", (2, 12, 9, 200), "ROWS1", False, True, (RSH, RSH), side="l", form="rows_dense",
         mask="rows", n_xz=4, zeros=True),
    Spec("rows1_render_64_mix", "disp", (1, 5, 2, 64), "ROWS1", True, False, (RSH, RSH), side="l", render=True),
    Spec("pixelmask_258_mix", "disp", (2, 7, 5, 258), "AUTO", True, False, (RSH, RSH), mask="pixel", zeros=True, draw=1),
    Spec("pixelmask_65planes_l1_auto", "disp", (1, 65, 4, 128), "AUTO", False, True, (RSH, RSH), side="l", mask="pixel",
         zeros=True),
    # general forward / scatter backward: PD_IMPL_GENERAL in disparity mode; dense disparities under any impl
    Spec("general_130_mix", "disp", (2, 9, 7, 130), "GENERAL", True, False, (GEN, SC)),
    Spec("general_130_l1_auto", "disp", (2, 9, 7, 130), "GENERAL", False, True, (GEN, SC), side="l"),
    Spec("general_dense_258_mix_auto", "disp", (2, 7, 5, 258), "AUTO", True, True, (GEN, SC), form="dense", mask="pixel",
         zeros=True),
    Spec("general_rows_view_l1", "disp", (2, 12, 9, 200), "GENERAL", False, False, (GEN, SC), side="l", form="rows_view",
         mask="rows", n_xz=4, zeros=True),
    Spec("general_render_64_mix", "disp", (1, 5, 2, 64), "GENERAL", True, False, (GEN, SC), render=True),
    # homography, one matrix per plane: gather backward (gradients wanted) / scatter backward (PD_IMPL_GENERAL: gather_fits false)
    Spec("gather_80_mix", "homo", (2, 7, 8, 80), "AUTO", True, False, (GEN, GA), form="planes"),
    Spec("gather_96_l1_auto", "homo", (1, 5, 6, 96), "AUTO", False, True, (GEN, GA), form="planes"),
    Spec("gather_80_render_mix_auto", "homo", (2, 7, 8, 80), "AUTO", True, True, (GEN, GA), form="planes", render=True),
    Spec("hscatter_80_mix_auto", "homo", (2, 7, 8, 80), "GENERAL", True, True, (GEN, SC), form="planes", draw=1),
    Spec("hscatter_96_l1_auto", "homo", (1, 5, 6, 96), "GENERAL", False, True, (GEN, SC), form="planes", g2="randn"),
    Spec("hscatter_96_mix", "homo", (1, 5, 6, 96), "GENERAL", True, False, (GEN, SC), form="planes"),
    Spec("hscatter_96_render_mix", "homo", (1, 5, 6, 96), "GENERAL", True, False, (GEN, SC), form="planes", render=True,
         draw=1),
    # plane-uniform homography: pass 2 staged through LDS (AUTO) and direct (PD_IMPL_UNIFORM_DIRECT)
    Spec("uniform_80_mix", "homo", (2, 7, 8, 80), "AUTO", True, False, (UNI, UST), form="uniform", draw=1),
    Spec("uniform_96_l1_auto", "homo", (1, 5, 6, 96), "AUTO", False, True, (UNI, UST), form="uniform"),
    Spec("uniform_96_render_mix", "homo", (1, 5, 6, 96), "AUTO", True, False, (UNI, UST), form="uniform", render=True),
    Spec("uniform_direct_80_mix_auto", "homo", (2, 7, 8, 80), "UNIFORM_DIRECT", True, True, (UNI, UDI), form="uniform", draw=1),
    Spec("uniform_direct_96_l1_auto", "homo", (1, 5, 6, 96), "UNIFORM_DIRECT", False, True, (UNI, UDI), form="uniform"),
    Spec("uniform_direct_96_mix", "homo", (1, 5, 6, 96), "UNIFORM_DIRECT", True, False, (UNI, UDI), form="uniform"),
    Spec("uniform_direct_96_render_mix", "homo", (1, 5, 6, 96), "UNIFORM_DIRECT", True, False, (UNI, UDI), form="uniform",
         render=True),
]
IDS = [s.name for s in SPECS]
ROUTES = [(SS, RS), (SS, RSH), (RSH, RSH), (GEN, SC), (GEN, GA), (UNI, UST), (UNI, UDI)]


def _capi():
    from planedepth_amd import _capi as C
    return C


def _seed(spec):
    return zlib.crc32(spec.name.encode()) % 100000 + 7 * spec.draw   # the same inputs in every process


def _route_key(spec):
    return "%s/%s/%s" % (spec.kind, spec.route[0], spec.route[1])


# =====================================================================================================================
# inputs
# =====================================================================================================================
def _frac_ok(v):
    f = v - torch.floor(v)
    return bool(((f >= 0.06) & (f <= 0.94)).all())


def _plane_disparities(N, W, g, gains=None, first=0, render=False):
    """N disparities with fractional parts in [0.06, 0.94] (``gains``: also of every product d * gain).  Integer parts: most in
    view, plane 1 leaves a single column (W - 1), plane 2 two (W - 2), plane N - 2 (N - 3 where that is the last plane of a mask
    word) is beyond the row (W + 3), every fourth is
    negative; with 40 planes or more plane 5 sits at 1e6.  ``render``: the last plane shifts by less than a pixel — alpha compositing
    hands it all the remaining probability, and where it is out of view the mixture density is the 1e-7 inside the logarithm: the
    loss gradient is amplified 1e7 times there and no fp32 evaluation of it means anything."""
    res = []
    out = N - 2 if (N - 2) % 32 != 31 else N - 3   # (the last plane of a mask word stays in view)
    for i in range(N):
        k = first + i
        while True:
            ip = float(torch.randint(0, max(2, min(W // 3, 40)), (1,), generator=g))
            if gains is None:
                if k == 1:
                    ip = float(W - 1)
                elif k == 2 and N >= 5:
                    ip = float(W - 2)
                elif k == out:
                    ip = float(W + 3)
                elif k == N - 1 and render:
                    ip = 0.0
            d = torch.tensor(ip + 0.06 + 0.88 * float(torch.rand(1, generator=g)), dtype=torch.float32)
            if gains is None and N >= 40 and k == 5:
                d = torch.tensor(1000000.5, dtype=torch.float32)
            if gains is None and k % 4 == 3 and not (render and k == N - 1):
                d = -d
            if _frac_ok(d[None]) and (gains is None or _frac_ok(d * gains)):
                res.append(float(d))
                break
    return res


def _band_limited(shape, gen, lo, hi, cutoff=0.12):
    """White noise low-passed in the Fourier domain and rescaled to [lo, hi], as test_gpu_parity._band_limited makes it: at x ~ 600
    the reference's fp32 coordinate chain is 1e-5 px off, which white-noise colours turn into 1e-4 of the tensor norm."""
    x = torch.randn(shape, generator=gen)
    H, W = shape[-2:]
    keep = ((torch.fft.fftfreq(H).abs()[:, None] * 2.0 <= cutoff) & (torch.fft.rfftfreq(W).abs()[None, :] * 2.0 <= cutoff)).to(x.dtype)
    x = torch.fft.irfft2(torch.fft.rfft2(x) * keep, s=(H, W))
    flat = x.flatten(-2)
    mn, mx = flat.min(-1)[0][..., None, None], flat.max(-1)[0][..., None, None]
    return lo + (hi - lo) * (x - mn) / (mx - mn)


def _images(spec, c, g):
    """src, tgt, logits, sigma of a build_case draw; band-limited from 640 columns on."""
    B, N, H, W = spec.shape
    if W < 640:
        return dict(src=c["color_l"], tgt=c["color_r"], logits=c["logits"], sigma=c["sigma"])
    return dict(src=_band_limited((B, 3, H, W), g, 0.0, 1.0), tgt=_band_limited((B, 3, H, W), g, 0.0, 1.0),
                logits=_band_limited((B, N, H, W), g, -3.0, 3.0), sigma=_band_limited((B, N, H, W), g, 0.02, 0.9))


def _disp_inputs(spec):
    from planedepth_amd.synthetic import build_case
    B, N, H, W = spec.shape
    g = torch.Generator().manual_seed(_seed(spec))
    n_xy = N - spec.n_xz
    disps = _plane_disparities(n_xy, W, g, render=spec.render)
    if spec.n_xz:   # ground planes: the disparity grows with the row (build_case's row_gain), masked above the horizon
        ycoord = torch.linspace(-1, 1, H)
        gains = torch.unique(0.4 + 0.6 * ycoord.clamp_min(0.0))
        disps += _plane_disparities(spec.n_xz, W, g, gains=gains, first=n_xy)
    c = build_case(B, N, H, W, _seed(spec), disp_min=1.0, disp_max=2.0, n_xz=spec.n_xz, special_disp=disps,
                   render_probability=spec.render, sigma_interior=True)
    inp = _images(spec, c, g)
    if spec.low_plane >= 0:
        inp["logits"] = inp["logits"].clone()
        inp["logits"][:, spec.low_plane] -= 8.0
    if spec.render:
        inp["dists"] = c["dists"]
    rows = (c["disp_pp"].expand(B, N, H, 1) * c["row_gain"])[..., 0].contiguous()           # [B,N,H], fp32 products
    if spec.form == "plane":
        inp["plane"] = c["disp_pp"].clone()                                                    # [B,N,1,1]
    elif spec.form in ("rows_view", "rows_dense"):
        inp["plane"] = rows
    else:   # a dense map that varies per pixel: integer part of the plane, fractional part in [0.12, 0.88]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        d = c["disp_pp"]                                                                       # [B,N,1,1]
        wave = 0.38 * torch.sin(0.7 * xs + 1.3 * ys + torch.arange(N, dtype=torch.float32).reshape(1, N, 1, 1))
        inp["plane"] = (torch.sign(d) * (torch.floor(d.abs()) + 0.5 + wave)).expand(B, N, H, W).contiguous()
    if spec.mask == "rows":
        m = c["padding_mask"][..., 0].clone()                                                  # [B,N,H]: the horizon of the xz planes
        m[:, 0, :2] = 0.0                                                                      # and a band of plane 0
        inp["mask"] = m
    elif spec.mask == "pixel":
        m = (torch.rand(B, N, H, W, generator=g) > 0.25).float()
        m[:, 0, :2] = 0.0
        inp["mask"] = m
    return inp


_SHIFT_STEPS = [0, 1, 2, 4, 7, 12, 20]


def _homo_inputs(spec):
    from planedepth_amd.synthetic import build_case, intrinsics
    B, N, H, W = spec.shape
    g = torch.Generator().manual_seed(_seed(spec))
    c = build_case(B, N, H, W, _seed(spec), disp_min=1.0, disp_max=2.0, render_probability=spec.render, sigma_interior=True)
    inp = dict(src=c["color_l"], tgt=c["color_r"], logits=c["logits"], sigma=c["sigma"])
    if spec.render:
        inp["dists"] = c["dists"]
    K, inv_K = intrinsics(B, H, W)
    fx, fy = float(K[0, 0, 0]), float(K[0, 1, 1])
    T = torch.eye(4)[None].repeat(B, 1, 1)
    r = lambda: float(torch.rand(1, generator=g))  # noqa: E731
    if spec.form == "uniform":
        # zero translation; K R K^-1 is the pixel translation (ix, iy) = (x + a_b, y + c_b) of every plane of image b
        for b in range(B):
            a = (1.0 if b % 2 == 0 else -1.0) * (3.0 + b + 0.06 + 0.88 * r())
            cy = (-1.0 if b % 2 == 0 else 1.0) * (1.0 + 0.06 + 0.88 * r())
            T[b, 0, 2], T[b, 1, 2] = -a / fx, -cy / fy
        distance = 1.0 + torch.rand(B, N, generator=g)
        # every plane samples the same colour here, so the colour share of g_logits / g_sigma cancels to fp32 noise that 1 / sigma
        # amplifies: sigma in [0.3, 0.9] keeps it below the mixture share
        inp["sigma"] = 0.3 + 0.6 * (c["sigma"] - 0.011) / 0.978
    else:
        # R = I, t = (tx, ty, 0), n = e_z: ix = x + s_b a_n, iy = y + s_b rho a_n with a_n = 0.1 fx / d_n, rho = fy ty / (fx tx)
        while True:
            rho = 0.2 + 0.25 * r()
            ints = [float(k) for k in _SHIFT_STEPS[:N - 1]] + [float(W + 2)]   # the last plane is out of view
            if spec.render:   # ... the first one under alpha compositing (see _plane_disparities)
                ints.reverse()
            a = torch.tensor([k + 0.06 + 0.88 * r() for k in ints])
            if _frac_ok(a) and _frac_ok(rho * a):
                break
        distance = (0.1 * fx / a)[None].repeat(B, 1)
        for b in range(B):
            s = 1.0 if b % 2 == 0 else -1.0
            T[b, 0, 3] = -0.1 * s
            T[b, 1, 3] = rho * fx * (-0.1 * s) / fy
    norm = torch.tensor([0.0, 0.0, 1.0])[None, None].repeat(B, N, 1)
    inp.update(distance=distance.float().contiguous(), T=T, K=K, inv_K=inv_K, norm=norm)
    return inp


def _weights(spec):
    B, N, H, W = spec.shape
    g = torch.Generator().manual_seed(_seed(spec) + 1)
    G1 = torch.randn(B, 3, H, W, generator=g)
    G2 = torch.randn(B, 1, H, W, generator=g) if spec.g2 == "randn" else torch.rand(B, 1, H, W, generator=g)
    return G1, G2


def _objective(combo, rgb_rec, ph_map, ph_mean, G1, G2):
    parts = dict(rgb=lambda: (rgb_rec * G1).sum(), map=lambda: (ph_map * G2).sum(), mean=lambda: W_MEAN * ph_mean)
    return sum(parts[k]() for k in parts) if combo == "all" else parts[combo]()


def _leaf_names(spec):
    names = ["logits"] + (["sigma"] if spec.mix else []) + (["dists"] if spec.render else [])
    if spec.kind == "disp":
        return names + ["plane"]
    return names + (["T"] if spec.form == "uniform" else ["distance", "T"])


_GRAD_NAME = dict(logits="g_logits", sigma="g_sigma", dists="g_dists", plane="g_disp", distance="g_distance", T="g_Rt")


def _collect(spec, leaves, outs, weights, combos):
    """{combo: {tensor name: CPU tensor}}: the forward tensors under "all", the gradients of every leaf per combination."""
    rgb_rec, ph_map, ph_mean = outs
    names = _leaf_names(spec)
    res = {}
    for combo in combos:
        obj = _objective(combo, rgb_rec, ph_map, ph_mean, *weights)
        grads = torch.autograd.grad(obj, [leaves[k] for k in names], retain_graph=True, allow_unused=True)
        r = {}
        for k, gr in zip(names, grads):
            gr = torch.zeros_like(leaves[k]) if gr is None else gr
            if k == "plane" and spec.form == "plane":
                gr = gr.reshape(gr.shape[0], gr.shape[1])
            if k == "T":
                gr = gr[:, :3]
            r[_GRAD_NAME[k]] = gr.detach().cpu()
        res[combo] = r
    res["all"].update(rgb_rec=rgb_rec.detach().cpu(), ph_map=ph_map.detach().cpu(), ph_mean=ph_mean.detach().reshape(1).cpu())
    return res


def _run_oracle(spec, inp, dtype, combos=("all", "mean")):
    B, N, H, W = spec.shape
    c = {k: v.to(dtype) for k, v in inp.items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in _leaf_names(spec)}
    kw = dict(use_mixture_loss=spec.mix, automask=spec.automask, render_probability=spec.render, dists=leaves.get("dists"))
    sigma = leaves.get("sigma")
    if spec.kind == "disp":
        plane = leaves["plane"]
        disp_layered = (plane if plane.dim() == 4 else plane[..., None]).expand(B, N, H, W)
        mask = c["mask"] if "mask" in c else torch.ones(B, N, H, W, dtype=dtype)
        mask = (mask if mask.dim() == 4 else mask[..., None]).expand(B, N, H, W)
        r = orc.warp_and_loss(c["src"], c["tgt"], leaves["logits"], sigma, warp_type="disp_warp", target_side=spec.side,
                              disp_layered=disp_layered, padding_mask=mask, **kw)
    else:
        r = orc.warp_and_loss(c["src"], c["tgt"], leaves["logits"], sigma, warp_type="homography_warp",
                              distance=leaves.get("distance", c["distance"]), norm=c["norm"], T=leaves["T"], K=c["K"],
                              inv_K=c["inv_K"], **kw)
    weights = tuple(w.to(dtype) for w in _weights(spec))
    res = _collect(spec, leaves, (r["rgb_rec"], r["ph_map"], r["ph_loss"]), weights, combos)
    res["grid"] = r["grid"].detach()
    return res


_REFS = {}


def references(spec):
    """(inputs, oracle fp32, oracle fp64) of a case: computed once per process, shared by the CPU and the GPU test, never modified."""
    if spec.name not in _REFS:
        inp = _disp_inputs(spec) if spec.kind == "disp" else _homo_inputs(spec)
        _REFS[spec.name] = (inp, _run_oracle(spec, inp, torch.float32), _run_oracle(spec, inp, torch.float64))
    return _REFS[spec.name]


# =====================================================================================================================
# routes: sweep_route's conditions restated (pd_plane_sweep.hip), confirmed by the capability queries where one exists
# =====================================================================================================================
def _descriptor(spec):
    """(SweepDesc the operator builds for the case, per-pixel mask?)."""
    C = _capi()
    lib = C.load()
    B, N, H, W = spec.shape
    impl = getattr(C, "PD_IMPL_" + spec.impl)
    flags = (C.PD_MIXTURE if spec.mix else 0) | (C.PD_AUTOMASK if spec.automask else 0) | (C.PD_RENDER_PROB if spec.render else 0)
    if spec.kind == "homo":
        flags |= C.PD_HOMO_UNIFORM if spec.form == "uniform" else 0
        return C.SweepDesc(B, N, H, W, C.PD_WARP_HOMOGRAPHY, flags, 0.0, impl), False
    row_kernels = bool(lib.pd_sweep_uses_rowshift(ctypes.byref(C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, 0, 1.0, impl))))
    rows_form = spec.form in ("rows_view", "rows_dense") and row_kernels
    dense = spec.form == "dense" or (spec.form != "plane" and not rows_form)
    flags |= C.PD_DISP_ROWS if rows_form else (C.PD_DISP_DENSE if dense else 0)
    mask_rows = spec.mask == "rows" and not dense and row_kernels
    flags |= C.PD_MASK_ROWS if mask_rows else 0
    return C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, flags, 1.0 if spec.side == "r" else -1.0, impl), spec.mask != "none" and not mask_rows


def expected_route(spec):
    """(forward family, backward family) by sweep_route's conditions, LDS limits aside (every shape here is far inside them)."""
    C = _capi()
    d, per_pixel_mask = _descriptor(spec)
    B, N, H, W = spec.shape
    if spec.kind == "homo":
        if spec.form == "uniform":
            return UNI, (UDI if spec.impl == "UNIFORM_DIRECT" else UST)
        return GEN, (GA if spec.impl in ("AUTO", "UNIFORM_DIRECT", "FAST_ROWS", "EXACT_ROWS") else SC)   # gather_bwd_applicable
    rows = spec.impl != "GENERAL" and not d.flags & C.PD_DISP_DENSE
    if not rows:
        return GEN, SC
    stream_ok = spec.impl != "ROWS1" and not per_pixel_mask and W % 2 == 0
    fwd = SS if stream_ok and (not spec.render or (H * W) % 2 == 0) else RSH
    bwd = RS if stream_ok and not spec.render else RSH
    return fwd, bwd


def check_route(spec):
    """The table entry is the family sweep_route's conditions give, and every capability query that can see it agrees.

    Stated but confirmed by no query: gather against scatter in homography mode (both accumulate; expected_route restates
    gather_bwd_applicable's list of `impl` values) and staged against direct pass 2 of the plane-uniform backward (`impl ==
    PD_IMPL_UNIFORM_DIRECT` in uniform_bwd).  A change to either condition has to be carried into expected_route by hand."""
    C = _capi()
    lib = C.load()
    d, per_pixel_mask = _descriptor(spec)
    fwd, bwd = expected_route(spec)
    assert (fwd, bwd) == spec.route, (spec.name, spec.route, (fwd, bwd))
    q = lambda fn: bool(fn(ctypes.byref(d)))  # noqa: E731
    rows = fwd in (SS, RSH)
    assert q(lib.pd_sweep_uses_rowshift) == rows, spec.name
    assert q(lib.pd_sweep_bwd_accumulates) == (not rows), spec.name            # the non-row families add in place
    if not per_pixel_mask:   # (the queries assume a call without one)
        per_plane = not d.flags & (C.PD_DISP_ROWS | C.PD_DISP_DENSE)
        assert q(lib.pd_sweep_bwd_plane_adds) == (bwd == RS and per_plane), spec.name
        if spec.kind == "disp":   # native bf16 storage is served exactly where both stream kernels run
            assert q(lib.pd_sweep_native_bf16) == ((fwd, bwd) == (SS, RS)), spec.name
    return d, per_pixel_mask


# =====================================================================================================================
# the bars
# =====================================================================================================================
def _grid_margin(spec, grid):
    """Smallest distance of a sampling coordinate of the fp64 grid from an integer (x only in disparity mode: iy = y there)."""
    B, N, H, W = spec.shape
    ix = (grid[..., 0] + 1) / 2 * (W - 1)
    m = float((ix - torch.round(ix)).abs().min())
    if spec.kind == "homo":
        iy = (grid[..., 1] + 1) / 2 * (H - 1)
        m = min(m, float((iy - torch.round(iy)).abs().min()))
    return m


def _tensor_norm_ok(spec, who, combo, name, got, r64):
    """The suite's tensor-norm bar against fp64, next to the row-scaled one: rel_err < 1e-4, 2e-4 for the disparity gradient — in
    both modes, for the product and for the oracle's own fp32 run (test_conditions_cpu)."""
    e = rel_err(got, r64)
    bar = DISP_TOL if name == "g_disp" else TOL
    if who == "product":
        bar = max(bar, NAMED_NORM_BARS.get((spec.name, combo, name), 0.0))
    return e < bar, e


# A route and tensor that misses the common bar for a documented, deliberate reason gets a named constant of twice the measured
# value (profiles/sweep_slice_parity.md); the common bar stays.
#
# Plane-uniform homography under alpha compositing, g_sigma: measured 1.348e-4 (joint objective) against 2 * 1.53e-5 + 1e-4.  The
# product forms H_t2s in fp64 and rounds once ("homography_warp end to end"); the oracle's fp32 run inverts in
# fp32.  On this case the oracle's OWN per-pixel fp32 arithmetic, given the fp64-formed matrices, lands at 1.351e-4 (ph_map 4.001e-5,
# the product's figure to four digits): test_named_constant_is_the_oracles_fp32_arithmetic_on_fp64_formed_matrices shows it without
# a device.  The kernel computes what the reference's arithmetic computes on its matrices; E_ref is small by the luck of one inverse.
UNIFORM_RENDER_G_SIGMA = 2.7e-4
NAMED_BARS = {("uniform_96_render_mix", "g_sigma"): UNIFORM_RENDER_G_SIGMA}
# The same case, tensor and cause under the tensor-norm bar, fused mean alone: measured 1.029e-4 against 1e-4; the oracle's fp32
# arithmetic on the fp64-formed matrices gives the same (the CPU test above covers both objectives).
UNIFORM_RENDER_G_SIGMA_NORM = 2.1e-4
NAMED_NORM_BARS = {("uniform_96_render_mix", "mean", "g_sigma"): UNIFORM_RENDER_G_SIGMA_NORM}
EPS32 = 2.0 ** -24


def _noise_only(spec, name):
    """The one exclusion (stated in profiles/sweep_slice_parity.md).  Plane-uniform sweep under the L1 loss: every plane samples the
    same colour c, rgb_rec = sum_n pi_n c does not depend on the logits, and g_logits = pi_n (g . c - g . rgb_rec) is an exact zero
    in exact arithmetic — what a kernel returns is fp32 cancellation noise, to which no relative measure applies."""
    return spec.form == "uniform" and not spec.mix and name == "g_logits"


def _noise_cap(spec, combo):
    """Bound of that noise from the number format: rgb_rec is a sum of N products, each rounded (N eps |c| with |c| <= 1), and
    g . c - g . rgb_rec adds three channels of it times the largest upstream gradient of a colour — G1, plus a third of the
    gradient of ph_map (the L1 term hands sgn / 3 per channel) — with pi_n <= 1.  Measured: 6e-8 .. 1.5e-7 against ~4e-6."""
    B, N, H, W = spec.shape
    G1, G2 = _weights(spec)
    gp = W_MEAN / (B * H * W) + (float(G2.abs().max()) if combo in ("all", "map") else 0.0)
    g = (float(G1.abs().max()) if combo in ("all", "rgb") else 0.0) + gp / 3.0
    return 3 * N * EPS32 * g


def hold(spec, who, combo, res, r32, r64):
    """Every tensor of ``res`` against the bars; returns {tensor: slice_report}."""
    reps, missed = {}, []
    for name, ref in r64.items():
        got = res[name]
        assert got.shape == ref.shape, (spec.name, name, tuple(got.shape), tuple(ref.shape))
        if _noise_only(spec, name):
            print("%s %s/%s %s: max |.| %.1e (an exact zero: noise only)" % (who, spec.name, combo, name, float(got.abs().max())))
            assert float(got.abs().max()) <= _noise_cap(spec, combo), (spec.name, combo, name, float(got.abs().max()), _noise_cap(spec, combo))
            continue
        rep = slice_report(got, ref, PLANE_FLOOR)
        e_ref = slice_report(r32[name], ref, PLANE_FLOOR)["err"]
        ok_norm, e_norm = _tensor_norm_ok(spec, who, combo, name, got, ref)
        print("%s %s/%s %s: err %.3e  E_ref %.3e  tensor-norm %.3e  zero planes %d  zero rows %d  |zero| %.1e"
              % (who, spec.name, combo, name, rep["err"], e_ref, e_norm, rep["zero_planes"], rep["zero_rows"], rep["zero_abs"]))
        if combo == "all":
            slot = REPORT.setdefault((_route_key(spec), name), {})
            slot[who] = max(slot.get(who, 0.0), rep["err"])
            slot["oracle_fp32"] = max(slot.get("oracle_fp32", 0.0), e_ref)
            E_REF.setdefault(spec.name, {})[name] = e_ref
        assert math.isfinite(rep["err"]) and bool(torch.isfinite(got).all()), (spec.name, combo, name)
        if not rep["zero_ok"]:
            missed.append((name, "nonzero where the fp64 reference is identically zero", rep["zero_abs"], rep["scale"]))
        bar = 2.0 * e_ref + 1e-4
        if who == "product":
            bar = max(bar, NAMED_BARS.get((spec.name, name), 0.0))
        if not rep["err"] <= bar:
            missed.append((name, "row-scaled bar: err, E_ref", rep["err"], e_ref))
        if not ok_norm:
            missed.append((name, "tensor-norm bar", e_norm))
        reps[name] = rep
    assert not missed, (spec.name, who, combo, missed)   # (after every tensor's figures are printed)
    return reps


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("PD_SWEEP_PARITY_JSON")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump({"plane_floor": PLANE_FLOOR, "e_ref_cap": E_REF_CAP,
                       "routes": {"%s %s" % k: v for k, v in sorted(REPORT.items())},
                       "e_ref_per_case": {k: E_REF[k] for k in sorted(E_REF)}}, f, indent=1)


# =====================================================================================================================
# CPU: the conditions, without a device
# =====================================================================================================================
@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_conditions_cpu(spec):
    """Integer margin of the coordinates, the E_ref cap, the oracle's own fp32 run under the tensor-norm bar, the route."""
    inp, r32, r64 = references(spec)
    assert _grid_margin(spec, r64["grid"]) >= MARGIN, (spec.name, _grid_margin(spec, r64["grid"]))
    if spec.kind == "disp":
        p = inp["plane"].double()
        f = p - torch.floor(p)
        assert bool(((f >= MARGIN) & (f <= 1 - MARGIN)).all()), spec.name    # per plane, per row, per pixel: whatever the form
        assert not (spec.automask and bool((inp["plane"] == 0).any())), spec.name   # knife edge (d) of DESIGN.md section 5
    s = inp["sigma"]
    assert float(s.min()) > 0.01 and float(s.max()) < 1.0, spec.name   # no clamp kinks
    for combo in ("all", "mean"):
        reps = hold(spec, "oracle_fp32", combo, r32[combo], r32[combo], r64[combo])
        for name, rep in reps.items():
            assert rep["err"] <= E_REF_CAP, (spec.name, combo, name, "E_ref beyond the cap: change the case's inputs", rep["err"])
    if spec.zeros:
        B = spec.shape[0]
        assert slice_report(r32["all"]["g_logits"], r64["all"]["g_logits"], PLANE_FLOOR)["zero_planes"] >= B, spec.name
        m = inp["mask"]
        band = m.reshape(m.shape[0], m.shape[1], m.shape[2], -1).amax(3) == 0                 # [B,N,H]: fully masked rows
        assert bool(band.any(2).any()), spec.name
    check_route(spec)


@pytest.mark.parametrize("floor", [1e-1, 1e-2, 1e-3])
def test_plane_floor_is_the_smallest_that_meets_the_cap(floor):
    """PLANE_FLOOR from the oracle alone: the smallest of 1e-3, 1e-2, 1e-1 at which every tensor of every case has E_ref within
    the cap."""
    worst = 0.0
    for spec in SPECS:
        _, r32, r64 = references(spec)
        for combo in ("all", "mean"):
            for name, ref in r64[combo].items():
                if _noise_only(spec, name):
                    continue
                worst = max(worst, slice_report(r32[combo][name], ref, floor)["err"])
    meets = worst <= E_REF_CAP
    print("plane_floor %g: worst E_ref %.3e" % (floor, worst))
    assert meets == (floor >= PLANE_FLOOR), (floor, worst)


def test_row_scale_sees_a_low_row_error_that_the_tensor_norm_passes():
    """What the measure is for, on the reference itself: every low-scale row (largest entry below 1e-2 of the tensor's) off by 1 %
    passes rel_err < 1e-4 and misses the row-scaled bar tenfold or more."""
    spec = next(s for s in SPECS if s.name == "stream_65planes_mix")
    _, r32, r64 = references(spec)
    for name in ("g_logits", "g_sigma"):
        ref = r64["all"][name]
        rowmax = ref.abs().amax(3, keepdim=True)
        low = (rowmax > 0) & (rowmax < 1e-2 * ref.abs().max())
        assert int(low.sum()) >= 1, name
        broken = torch.where(low, ref * 1.01, ref)
        e_ref = slice_report(r32["all"][name], ref, PLANE_FLOOR)["err"]
        assert rel_err(broken, ref) < TOL, name
        assert slice_report(broken, ref, PLANE_FLOOR)["err"] > 5 * (2.0 * e_ref + 1e-4), name


def test_named_constant_is_the_oracles_fp32_arithmetic_on_fp64_formed_matrices():
    """UNIFORM_RENDER_G_SIGMA without a device: the oracle's fp32 run of that case on H_t2s formed in fp64 and rounded once (the
    product's documented matrix route) is more than four times as far from fp64 as its run on its own fp32 inverse, beyond 1e-4 by
    itself, and inside the named constant."""
    (name, tensor), = NAMED_BARS
    spec = next(s for s in SPECS if s.name == name)
    B, N, H, W = spec.shape
    inp, r32, r64 = references(spec)
    c64 = {k: v.double() for k, v in inp.items()}
    ex = lambda M: M[:, None].expand(-1, N, -1, -1).reshape(B * N, 4, 4)  # noqa: E731
    H64, _ = orc.homography_matrices(c64["distance"], c64["norm"], ex(c64["T"]), ex(c64["K"]), ex(c64["inv_K"]))
    c = {k: v.float() for k, v in inp.items()}
    sigma, dists = c["sigma"].clone().requires_grad_(True), c["dists"].clone().requires_grad_(True)
    r = orc.warp_and_loss(c["src"], c["tgt"], c["logits"], sigma, warp_type="homography_warp", distance=c["distance"],
                          norm=c["norm"], T=c["T"], K=c["K"], inv_K=c["inv_K"], use_mixture_loss=True, automask=spec.automask,
                          render_probability=True, dists=dists, H_t2s=H64.float())
    outs = (r["rgb_rec"], r["ph_map"], r["ph_loss"])
    g_sigma, = torch.autograd.grad(_objective("all", *outs, *_weights(spec)), [sigma], retain_graph=True)
    g_mean, = torch.autograd.grad(_objective("mean", *outs, *_weights(spec)), [sigma])
    norm_mean = rel_err(g_mean, r64["mean"][tensor])   # UNIFORM_RENDER_G_SIGMA_NORM: the fused mean alone, tensor norm
    print("fp32 oracle on fp64-formed matrices, mean alone: %s tensor norm %.3e" % (tensor, norm_mean))
    assert 0.5 * TOL < norm_mean <= NAMED_NORM_BARS[(name, "mean", tensor)], norm_mean   # (1.017e-4: at the bar by itself)
    err = slice_report(g_sigma, r64["all"][tensor], PLANE_FLOOR)["err"]
    e_ref = slice_report(r32["all"][tensor], r64["all"][tensor], PLANE_FLOOR)["err"]
    print("fp32 oracle on fp64-formed matrices: %s err %.3e, on its own fp32 inverse %.3e" % (tensor, err, e_ref))
    # (E_ref moves by some 15 % with the host's fp32 inverse: the statements are kept clear of that)
    assert 1e-4 < err <= NAMED_BARS[(name, tensor)] and e_ref < 0.25 * err, (err, e_ref)


def test_table_covers_every_family_loss_form_and_constant():
    C = _capi()
    by_route = {r: [s for s in SPECS if s.route == r] for r in ROUTES}
    assert {s.route for s in SPECS} == set(ROUTES)
    for route, specs in by_route.items():
        assert specs, route
        assert any(s.mix and not s.automask for s in specs) and any(not s.mix and s.automask for s in specs), route
        assert any(s.mix for s in specs) and any(not s.mix for s in specs) and any(s.automask for s in specs), route
        if specs[0].kind == "disp":
            assert {s.side for s in specs} == {"l", "r"}, route
            assert any(s.zeros for s in specs), route                       # an out-of-view plane and a masked row band
    disp = [s for s in SPECS if s.kind == "disp"]
    render_routes = {s.route for s in SPECS if s.render}
    assert render_routes >= {(SS, RSH), (RSH, RSH), (GEN, SC), (GEN, GA), (UNI, UST), (UNI, UDI)}   # (row-stream never serves it)
    assert any(s.render and s.kind == "disp" and s.route == (GEN, SC) for s in SPECS)
    assert any(s.render and s.kind == "homo" and s.route == (GEN, SC) for s in SPECS)
    assert any(s.render and s.form == "rows_view" for s in SPECS)     # row-form disparities under alpha compositing
    assert any(s.low_plane % 32 == 31 for s in SPECS)                 # a low-probability last plane of a mask word
    assert not any(s.render for s in by_route[(SS, RS)])
    forms = lambda r: {s.form for s in by_route[r]}  # noqa: E731
    assert forms((SS, RS)) >= {"plane", "rows_view", "rows_dense"} and forms((RSH, RSH)) >= {"plane", "rows_view", "rows_dense"}
    assert forms((GEN, SC)) >= {"plane", "rows_view", "dense", "planes"}
    assert any(s.g2 == "randn" for s in SPECS)
    # how the routes are forced (the issue's table): AUTO and EXACT_ROWS on the stream pair; odd width and render under AUTO,
    # ROWS1 and a per-pixel mask under AUTO on the row-shift kernels; GENERAL in both modes; UNIFORM_DIRECT
    has = lambda **kw: any(all(getattr(s, k) == v for k, v in kw.items()) for s in SPECS)  # noqa: E731
    assert has(route=(SS, RS), impl="AUTO") and has(route=(SS, RS), impl="EXACT_ROWS")
    assert has(route=(SS, RSH), impl="AUTO", render=True)
    assert has(route=(RSH, RSH), impl="ROWS1") and has(route=(RSH, RSH), impl="AUTO", mask="pixel")
    assert any(s.route == (RSH, RSH) and s.impl == "AUTO" and s.shape[3] % 2 == 1 for s in SPECS)
    assert has(route=(GEN, SC), impl="GENERAL", kind="disp") and has(route=(GEN, SC), impl="GENERAL", kind="homo")
    assert has(route=(GEN, GA), impl="AUTO") and has(route=(UNI, UST), impl="AUTO") and has(route=(UNI, UDI), impl="UNIFORM_DIRECT")
    # the kernels' constants: wave 64, 128-pixel segment, two pixels per lane, five-segment column block, 32-plane mask words,
    # the even-width rule of the row-stream backward, H > 1
    shapes = {s.shape for s in SPECS}
    assert shapes >= {(2, 9, 7, 130), (1, 5, 2, 64), (2, 7, 5, 258), (1, 12, 4, 640), (1, 4, 3, 1416), (1, 65, 4, 128),
                      (1, 33, 3, 66), (1, 5, 5, 257), (2, 12, 9, 200), (2, 7, 8, 80), (1, 5, 6, 96)}
    widths = {s.shape[3] for s in disp}
    assert any(w < 128 and w % 64 == 0 for w in widths)                      # half a segment, one wave of single pixels
    assert any(w > 128 and w % 128 not in (0, 1) and w % 2 == 0 for w in widths)   # ragged last segment
    assert any(w % 128 == 2 for w in widths)                                 # one lane pair beyond a segment
    assert any(w == 5 * 128 for w in widths) and any(w > 2 * 5 * 128 and w % (5 * 128) for w in widths)   # column blocks, last ragged
    assert any(w % 2 for w in widths)                                        # the even-width rule
    planes = {s.shape[1] for s in disp}
    assert any(n > 64 for n in planes) and any(n == 33 for n in planes)      # three mask words; one plane into the second
    assert min(s.shape[2] for s in SPECS) == 2
    assert any(s.n_xz and s.form == "rows_view" for s in SPECS) and any(s.n_xz and s.form == "rows_dense" for s in SPECS)
    assert all(hasattr(C, "PD_IMPL_" + s.impl) for s in SPECS)


# =====================================================================================================================
# GPU
# =====================================================================================================================
def _run_product(spec, inp, device="cuda"):
    from planedepth_amd import ops
    C = _capi()
    B, N, H, W = spec.shape
    c = {k: v.to(device) for k, v in inp.items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in _leaf_names(spec)}
    kw = dict(use_mixture_loss=spec.mix, automask=spec.automask, render_probability=spec.render, dists=leaves.get("dists"),
              return_mean=True)
    sigma = leaves.get("sigma")
    prev = ops.SWEEP_IMPL
    ops.SWEEP_IMPL = getattr(C, "PD_IMPL_" + spec.impl)
    try:
        if spec.kind == "disp":
            plane, mask = leaves["plane"], c.get("mask")
            row_uniform = spec.form == "rows_dense"
            if spec.form == "plane":
                disp_layered = plane.expand(B, N, H, W)                      # the decoder's view of [B,N,1,1] scalars
            elif spec.form == "rows_view":
                disp_layered = ops.row_view(plane, W)
            elif spec.form == "rows_dense":
                disp_layered = plane[..., None].expand(B, N, H, W).contiguous()   # a dense map under the row_uniform promise
            else:
                disp_layered = plane
            if mask is not None and mask.dim() == 3:
                mask = mask[..., None].expand(B, N, H, W).contiguous() if row_uniform else ops.row_view(mask, W)
            outs = ops.plane_sweep_disp(c["src"], c["tgt"], leaves["logits"], sigma, disp_layered, mask, target_side=spec.side,
                                        row_uniform=row_uniform, **kw)
        else:
            outs = ops.plane_sweep_homography(c["src"], c["tgt"], leaves["logits"], sigma, leaves.get("distance", c["distance"]),
                                              c["norm"], leaves["T"], c["K"], c["inv_K"], plane_uniform=spec.form == "uniform", **kw)
        flags = ops.LAST_SWEEP_FLAGS
        weights = tuple(w.to(device) for w in _weights(spec))
        res = _collect(spec, leaves, outs, weights, COMBOS)
    finally:
        ops.SWEEP_IMPL = prev
    return res, flags


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_route_against_fp64_per_row(spec):
    """The product on the case's route: every tensor under the row-scaled and the tensor-norm bar for the joint objective and for
    {mean} alone (g_rgb_rec = g_ph_map = None, the training configuration); the three partial backward results add up to the joint
    one; planes out of view stay clean."""
    C = _capi()
    inp, r32, r64 = references(spec)
    d, _ = check_route(spec)
    res, flags = _run_product(spec, inp)
    keep = ~(C.PD_BWD_ACCUMULATE | C.PD_BWD_DEFER_GATHER | C.PD_PH_MEAN_ZEROED | C.PD_BWD_PLANE_ZEROED | C.PD_LOGITS_BF16)
    assert flags & keep == d.flags, (spec.name, "the operator built another descriptor than the table states", flags, d.flags)
    reps = hold(spec, "product", "all", res["all"], r32["all"], r64["all"])
    hold(spec, "product", "mean", res["mean"], r32["mean"], r64["mean"])
    if spec.zeros:
        assert reps["g_logits"]["zero_planes"] >= spec.shape[0], (spec.name, reps["g_logits"])
        if spec.mix:
            assert reps["g_sigma"]["zero_planes"] >= spec.shape[0], (spec.name, reps["g_sigma"])
    for name, joint in res["all"].items():
        if not name.startswith("g_") or _noise_only(spec, name):
            continue
        total = res["rgb"][name].double() + res["map"][name].double() + res["mean"][name].double()
        tol = LINEAR_PLANE_TOL if name in ("g_disp", "g_distance", "g_Rt") else LINEAR_TOL
        e = rel_err(total, joint) if float(joint.abs().max()) > 0 else float(total.abs().max())
        print("product %s linear %s: %.3e" % (spec.name, name, e))
        assert e < tol, (spec.name, name, "sum of the partial backward results differs from the joint one", e)
