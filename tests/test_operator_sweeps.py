"""Standalone operators (SSIM / reprojection loss, mixture NLL, grid_sample, geometry, masked photometric, smoothness):
shape, edge and per-element parity sweep against the fp64 oracle.

Reference: the oracle function of the same operation in fp64 on the CPU, autograd for the gradients.  Yardstick: the same
function in fp32.  Two bars:
  1  regular inputs: ``elementwise_report(got, ref64, rtol=1e-4, floor=1e-4)["frac_beyond"] == 0`` (the project's 1e-4 parity bar,
     per element);
  2  ill-conditioned inputs (nearly flat / nearly identical SSIM windows, gradients through fp32 sampling coordinates):
     ``three_way(got, ref32, ref64)``.
Elements on a non-differentiable point (a sampling coordinate within 1e-3 pixel of an integer, an SSIM value within 1e-5 of 0
or 1, an automask tie) may be left out of a per-element comparison.  The selection comes from the fp64 reference alone, its
share is asserted to be at most 1 %, and ``test_conditions_cpu`` proves for every case, without a GPU, that the share holds
and that the oracle's own fp32 run meets the bar the product is held to.

Sizes come from the kernels' constants: block 256, wave 64, SSIM tile 32x8, kHgPix = 8, kSmoothRows = 4.

Set PD_OPERATOR_PARITY_JSON=<file> to get the worst per-element error per operator and output (product and oracle fp32, in units
of the allowance) written at the end of the run: the source of profiles/operator_parity.md."""
import ctypes
import json
import math
import os
import zlib

import pytest
import torch

from cases import elementwise_report, rel_err, three_way
from oracle import planedepth_oracle as orc

gpu = pytest.mark.gpu
DEV = "cuda"
MAX_SHARE = 0.01
REPORT = {}   # (operator, output) -> {"product": worst_over_allowance, "oracle_fp32": ...}


def _ops():
    from planedepth_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(spec):
    return zlib.crc32(repr(spec).encode()) % 100000   # the same inputs in every process (hash() of a str is salted)


def rand(g, *shape):
    return torch.rand(*shape, generator=g)


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


class Case:
    """One operator call: ``prod(*args)`` on the GPU against ``orc(*args)`` on the CPU.  ``wrt``: indices of the arguments that
    get a gradient.  ``names``: one per output, then one per gradient.  ``bars``: name -> 1 | 2 | None (None: checked by
    ``extra`` alone).  ``exclude(args64) -> {name: bool mask}``: elements left out (from the fp64 inputs alone).
    ``deterministic``: True (every output and gradient), False, or the names that two runs must give bit-identical.
    ``extra(res, r64, who)``: further assertions on a result dict (run on the product on the GPU and on the oracle's fp32 run on the
    CPU); ``gpu_extra(res, r64)``: assertions that only the product can meet (exact zeros, bit-equality)."""

    def __init__(self, op, prod, orc_fn, args, wrt, names, bar=1, bars=None, exclude=None, extra=None, gpu_extra=None,
                 deterministic=True, seed=1):
        self.op, self.prod, self.orc, self.args, self.wrt, self.names = op, prod, orc_fn, args, tuple(wrt), names
        self.bars = {n: bar for n in names}
        self.bars.update(bars or {})
        self.exclude, self.extra, self.gpu_extra, self.deterministic, self.seed = exclude, extra, gpu_extra, deterministic, seed


def run(fn, case, dtype=None, device="cpu"):
    """fn(*args) with the float tensors moved to (device, dtype), objective sum_k (out_k * gw_k).sum() with seeded gw_k; returns
    {name: tensor on the CPU} for the outputs and the gradients, and the converted arguments."""
    a = []
    for i, t in enumerate(case.args):
        if torch.is_tensor(t):
            t = t.detach().to(device=device, dtype=(dtype or t.dtype) if t.is_floating_point() else t.dtype).clone()
            if i in case.wrt:
                t.requires_grad_(True)
        a.append(t)
    out = fn(*a)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    obj = 0.0
    for k, o in enumerate(outs):
        gw = torch.randn(o.shape, generator=_gen(case.seed + 17 * k))
        obj = obj + (o * gw.to(device=o.device, dtype=o.dtype)).sum()
    grads = torch.autograd.grad(obj, [a[i] for i in case.wrt], allow_unused=True) if case.wrt else []
    grads = [torch.zeros_like(a[i]) if g is None else g for i, g in zip(case.wrt, grads)]
    res = {n: t.detach().cpu() for n, t in zip(case.names, outs + grads)}
    assert len(res) == len(case.names) == len(outs) + len(grads), (case.names, len(outs), len(grads))
    return res, a


def references(case):
    r64, a64 = run(case.orc, case, torch.float64)
    r32, _ = run(case.orc, case, torch.float32)
    masks = case.exclude([t.detach() if torch.is_tensor(t) else t for t in a64]) if case.exclude else {}
    for name, m in masks.items():
        assert m.shape == r64[name].shape, (name, m.shape, r64[name].shape)
        share = float(m.double().mean())
        assert share <= MAX_SHARE, "%s: %.2f %% of %s left out (at most 1 %%)" % (case.op, 100 * share, name)
    return r32, r64, masks


def _keep(t, masks, name):
    return t[~masks[name]] if name in masks else t


def compare(case, res, r32, r64, masks, who):
    """The per-name bars of ``case`` on the result dict ``res``."""
    for name in case.names:
        bar = case.bars[name]
        got, ref = res[name], r64[name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if bar == 1:
            rep = elementwise_report(_keep(got, masks, name), _keep(ref, masks, name), rtol=1e-4, floor=1e-4)
            print("%s %s %s: %s" % (who, case.op, name, rep))
            slot = REPORT.setdefault((case.op, name), {})
            slot[who] = max(slot.get(who, 0.0), rep["worst_over_allowance"])
            assert math.isfinite(rep["worst_over_allowance"]), (case.op, name, who, rep)
            assert rep["frac_beyond"] == 0, (case.op, name, who, rep)
        elif bar == 2 and who == "product":
            ok, e_got, e_ref = three_way(got, r32[name], ref)
            print("%s %s %s: three-way err_got %.3e err_ref %.3e" % (who, case.op, name, e_got, e_ref))
            assert ok, (case.op, name, e_got, e_ref)
    if case.extra:
        case.extra(res, r64, who)


def check_on_gpu(case):
    r32, r64, masks = references(case)
    res, _ = run(case.prod, case, device=DEV)
    compare(case, res, r32, r64, masks, "product")
    if case.gpu_extra:
        case.gpu_extra(res, r64)
    if case.deterministic:   # no atomics in these kernels: a second run gives the same bits
        again, _ = run(case.prod, case, device=DEV)
        for name in (case.names if case.deterministic is True else case.deterministic):
            assert torch.equal(res[name].view(torch.int32), again[name].view(torch.int32)), \
                "%s %s differs between two runs" % (case.op, name)
    return res, r32, r64


def check_on_cpu(case):
    r32, r64, masks = references(case)
    compare(case, r32, r32, r64, masks, "oracle_fp32")


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("PD_OPERATOR_PARITY_JSON")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump({"%s/%s" % k: v for k, v in sorted(REPORT.items())}, f, indent=1)


def ids(specs):
    return ["-".join(str(v).replace(" ", "") for v in s) for s in specs]


# =====================================================================================================================
# SSIM / reprojection loss                                                                      (pd_ssim.hip: tile 32x8)
# =====================================================================================================================
SSIM_SHAPES = [(2, 2), (2, 33), (8, 32), (9, 33), (7, 31), (16, 64), (17, 65), (3, 257)]
FULL = (192, 640)
# (kind, B, C, H, W, regime, wrt, layout)   kind: ssim | reproj1 (use_ssim) | reproj0;  wrt: "x" | "y" | "xy"
SSIM_SPECS = []
for _i, (_h, _w) in enumerate(SSIM_SHAPES):
    SSIM_SPECS.append(("ssim", (1, 3)[_i % 2], (1, 3, 4)[_i % 3], _h, _w, "random", "xy", "plain"))
    SSIM_SPECS.append(("reproj1", (3, 1)[_i % 2], 3, _h, _w, "random", "xy", "plain"))
SSIM_SPECS += [("reproj0", 1, 3, 2, 2, "random", "xy", "plain"), ("reproj0", 3, 3, 9, 33, "random", "xy", "plain"),
               ("reproj0", 1, 3, 17, 65, "random", "y", "plain")]
for _k in ("ssim", "reproj1"):
    for _hw in ((9, 33), (17, 65)):
        SSIM_SPECS += [(_k, 1, 3) + _hw + ("random", "x", "plain"), (_k, 3, 3) + _hw + ("random", "y", "plain")]
    SSIM_SPECS += [(_k, 3, 3, 9, 33, "random", "xy", "crop"), (_k, 1, 3, 9, 33, "random", "xy", "strided_grad"),
                   (_k, 1, 3, 17, 65, "flat", "xy", "plain"), (_k, 3, 3, 17, 65, "close", "xy", "plain"),
                   (_k, 1, 3, 17, 65, "identical", "xy", "plain"), (_k, 1, 3, 2, 33, "close", "xy", "plain")]
SSIM_SPECS += [("ssim", 1, 3) + FULL + ("random", "xy", "plain"), ("ssim", 1, 3) + FULL + ("flat", "xy", "plain"),
               ("ssim", 1, 3) + FULL + ("close", "xy", "plain"), ("reproj1", 3, 3) + FULL + ("random", "xy", "plain")]


def ssim_case(spec):
    kind, B, C, H, W, regime, wrt, layout = spec
    g = _gen(_seed(spec[:6]))
    pad = 5 if layout == "crop" else 0
    x = rand(g, B, C, H, W + pad)
    y = rand(g, B, C, H, W + pad)
    if regime == "flat":
        x = 0.7 + 1e-4 * randn(g, B, C, H, W + pad)
    elif regime == "close":
        y = x + 1e-3 * randn(g, B, C, H, W + pad)
    elif regime == "identical":
        y = x.clone()
    ops = _ops() if torch.cuda.is_available() else None
    if kind == "ssim":
        f_prod, f_orc, op = (lambda a, b: ops.ssim(a, b)), orc.ssim, "ssim"
    else:
        us = kind == "reproj1"
        f_prod, f_orc = (lambda a, b: ops.reprojection_loss(a, b, us)), (lambda a, b: orc.reprojection_loss(a, b, us))
        op = "reprojection_loss" if us else "reprojection_loss(l1)"

    def shaped(f):
        if layout == "crop":             # a width crop of a wider tensor: non-contiguous inputs
            return lambda a, b: f(a[..., 2:2 + W], b[..., 2:2 + W])
        if layout == "strided_grad":     # the objective is formed on a transposed view: a non-contiguous upstream gradient
            return lambda a, b: f(a, b).transpose(-1, -2)
        return f
    names = ["out"] + ["g_" + n for n in wrt]
    well = regime == "random"

    def exclude(a64):
        # an SSIM value within 1e-5 of the clamp bounds: fp32 and fp64 may sit on different sides of it
        xx, yy = (t[..., 2:2 + W] if layout == "crop" else t for t in a64[:2])
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        mu_x, mu_y = orc._box3_reflect(xx), orc._box3_reflect(yy)
        sx, sy = orc._box3_reflect(xx * xx) - mu_x ** 2, orc._box3_reflect(yy * yy) - mu_y ** 2
        sxy = orc._box3_reflect(xx * yy) - mu_x * mu_y
        v = (1 - (2 * mu_x * mu_y + C1) * (2 * sxy + C2) / ((mu_x ** 2 + mu_y ** 2 + C1) * (sx + sy + C2))) / 2
        near = ((v.abs() < 1e-5) | ((v - 1).abs() < 1e-5))
        if kind != "ssim":
            near = near.any(1, keepdim=True)
        # the gradient at a pixel gathers the centres within one pixel of it
        spread = torch.nn.functional.max_pool2d(near.double(), 3, 1, 1) > 0
        out_m = near if layout != "strided_grad" else near.transpose(-1, -2)
        full = torch.zeros(B, C, H, W + pad, dtype=torch.bool)
        full[..., 2 if pad else 0:(2 if pad else 0) + W] = spread.expand(B, C, H, W)
        m = {"out": out_m}
        m.update({n: full for n in names[1:]})
        return m

    def extra(res, r64, who):
        for n in names:
            assert torch.isfinite(res[n]).all(), (op, n, who)
        assert float(res["out"].min()) >= 0.0 and float(res["out"].max()) <= 1.0, (op, who)

    def gpu_extra(res, r64):
        if regime == "identical":
            assert float(res["out"].abs().max()) == 0.0, "identical images: the forward is exactly 0 (max %g)" % float(res["out"].abs().max())

    return Case(op + ("" if well else "[%s]" % regime), shaped(f_prod), shaped(f_orc), [x, y],
                [i for i, n in enumerate("xy") if n in wrt], names, bar=1 if well else 2,
                bars={"out": None} if regime == "identical" else None,   # exactly 0 (gpu_extra), not "close to a zero reference"
                exclude=exclude if (well and kind != "reproj0") else None, extra=extra if kind != "reproj0" else None,
                gpu_extra=gpu_extra)


@gpu
@pytest.mark.parametrize("spec", SSIM_SPECS, ids=ids(SSIM_SPECS))
def test_ssim_reprojection(spec):
    check_on_gpu(ssim_case(spec))


@gpu
def test_ssim_host_side_refusals():
    ops = _ops()
    x = torch.rand(1, 3, 1, 8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.ssim(x, x)
    with pytest.raises(RuntimeError):
        ops.ssim(x.transpose(2, 3).contiguous(), x.transpose(2, 3).contiguous())
    with pytest.raises(RuntimeError):
        ops.reprojection_loss(x, x)
    x4 = torch.rand(1, 4, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.reprojection_loss(x4, x4)


# =====================================================================================================================
# Mixture NLL                                                                         (pd_mixture.hip: one thread per pixel)
# =====================================================================================================================
MIX_HW = [(1, 1), (3, 85), (16, 16), (1, 257), (9, 33)]
# (dist, B, N, H, W, regime, wrt, broadcast)
MIX_SPECS = []
for _i, _n in enumerate((1, 2, 49, 64)):
    for _j, (_h, _w) in enumerate(MIX_HW):
        MIX_SPECS.append((("lap", "gaussian")[(_i + _j) % 2], (1, 3)[(_i + _j // 2) % 2], _n, _h, _w, "random", "esp", False))
for _d in ("lap", "gaussian"):
    MIX_SPECS += [(_d, 3, 2, 9, 33, "sigma_lo", "esp", False), (_d, 1, 49, 1, 257, "sigma_lo", "esp", False),
                  (_d, 1, 1, 3, 85, "sigma_lo", "esp", False), (_d, 3, 49, 9, 33, "sigma_hi", "esp", False),
                  (_d, 3, 2, 9, 33, "underflow", "esp", False), (_d, 1, 49, 16, 16, "underflow", "esp", False),
                  (_d, 3, 49, 9, 33, "random", "esp", True), (_d, 1, 2, 1, 257, "random", "esp", True),
                  (_d, 3, 2, 9, 33, "random", "e", False), (_d, 3, 2, 9, 33, "random", "s", False),
                  (_d, 3, 2, 9, 33, "random", "p", False)]


def mixture_case(spec):
    dist, B, N, H, W, regime, wrt, bcast = spec
    g = _gen(_seed(spec[:6]))
    e = rand(g, B, N, H, W) * 2 - 1
    s = 0.01 + 0.99 * rand(g, B, N, H, W)
    p = torch.softmax(randn(g, B, N, H, W), 1)
    if regime == "sigma_lo":     # the lower clamp bound of sigma; |error| / sigma up to 80, where a fast exponential is worst
        s = torch.full_like(s, 0.01)
        e = (rand(g, B, N, H, W) * 2 - 1) * 0.8
    elif regime == "sigma_hi":
        s = torch.full_like(s, 1.0)
    elif regime == "underflow":  # every density underflows fp32: the output is -log(1e-7)
        s = torch.full_like(s, 0.01)
        e = (1.5 + rand(g, B, N, H, W)) * torch.where(rand(g, B, N, H, W) < 0.5, -1.0, 1.0)
    if bcast:
        s = s[:, :, :1, :1].contiguous()
        p = torch.softmax(randn(g, B, 1, H, W), 0)
    ops = _ops() if torch.cuda.is_available() else None
    names = ["out"] + ["g_" + {"e": "error", "s": "sigma", "p": "pi"}[n] for n in wrt]
    bars = {n: None for n in names[1:]} if regime == "underflow" else None

    def extra(res, r64, who):
        for n in names:
            assert torch.isfinite(res[n]).all(), (n, who)
            assert res[n].shape == r64[n].shape
    return Case("multimodal_loss(%s)" % dist + ("[underflow]" if regime == "underflow" else ""),
                lambda a, b, c: ops.multimodal_loss(a, b, c, dist), lambda a, b, c: orc.multimodal_loss(a, b, c, dist),
                [e, s, p], [i for i, n in enumerate("esp") if n in wrt], names, bars=bars, extra=extra)


@gpu
@pytest.mark.parametrize("spec", MIX_SPECS, ids=ids(MIX_SPECS))
def test_multimodal_loss(spec):
    check_on_gpu(mixture_case(spec))


# =====================================================================================================================
# grid_sample                                                         (pd_grid_sample.hip: lane-to-lane hand-over of left taps)
# =====================================================================================================================
# (pad, M, C, (Hi, Wi), (Ho, Wo), coords, wrt)   coords: random | ("shift", s) | constant | exact   wrt: "i" | "g" | "ig"
GS_SPECS = []
for _i, (_in, _out) in enumerate([((11, 19), (7, 70)), ((5, 300), (9, 65)), ((1, 8), (3, 5)), ((6, 1), (4, 4))]):
    for _j, _pad in enumerate(("zeros", "border")):
        GS_SPECS.append((_pad, (2, 1)[_j], (1, 3, 5)[(_i + _j) % 3], _in, _out, "random", "ig"))
GS_SPECS += [("zeros", 2, 3, (11, 19), (3, 85), "random", "ig"), ("border", 1, 5, (11, 19), (16, 16), "random", "ig"),
             ("zeros", 3, 1, (11, 19), (1, 257), "random", "ig"), ("border", 2, 3, (11, 19), (1, 257), "random", "ig")]
for _s in (0.0, -1.5, -0.5, 0.5, 1.5):
    _wrt = "i" if _s == 0.0 else "ig"   # the identity samples at integers, where the coordinate derivative jumps
    GS_SPECS += [("zeros", 2, 3, (7, 70), (7, 70), ("shift", _s), _wrt), ("border", 1, 3, (7, 70), (7, 70), ("shift", _s), _wrt),
                 ("zeros", 1, 1, (5, 300), (5, 300), ("shift", _s), _wrt)]
for _pad in ("zeros", "border"):
    GS_SPECS += [(_pad, 2, 3, (11, 19), (7, 70), "constant", "ig"), (_pad, 1, 3, (5, 300), (9, 65), "exact", "ig"),
                 (_pad, 2, 3, (11, 19), (7, 70), "random", "i"), (_pad, 2, 3, (11, 19), (7, 70), "random", "g")]


def gs_pixel_coords(grid, Hi, Wi):
    return (grid[..., 0] + 1) / 2 * (Wi - 1), (grid[..., 1] + 1) / 2 * (Hi - 1)


def gs_near_integer(grid64, Hi, Wi):
    """[M,Ho,Wo,2] bool: the component's own coordinate (unclamped, fp64) is within 1e-3 pixel of an integer: d sample / d that
    coordinate jumps there.  A dimension of size 1 has a zero derivative on both sides and is never marked."""
    ix, iy = gs_pixel_coords(grid64, Hi, Wi)
    near = lambda v: (v - v.round()).abs() < 1e-3  # noqa: E731
    return torch.stack([near(ix) & (Wi > 1), near(iy) & (Hi > 1)], -1)


def gs_clamped(grid64, Hi, Wi):
    """[M,Ho,Wo,2] bool: border mode clamps this coordinate (torch's clip_coordinates_set_grad: at or beyond the bound)."""
    ix, iy = gs_pixel_coords(grid64, Hi, Wi)
    return torch.stack([(ix <= 0) | (ix >= Wi - 1), (iy <= 0) | (iy >= Hi - 1)], -1)


def gs_case(spec):
    pad, M, C, (Hi, Wi), (Ho, Wo), coords, wrt = spec
    g = _gen(_seed(spec))
    inp = rand(g, M, C, Hi, Wi)
    if coords == "random":
        grid = rand(g, M, Ho, Wo, 2) * 2.6 - 1.3
    elif coords == "constant":   # every output pixel adds into the same four input pixels
        grid = torch.tensor([0.31, -0.43]).expand(M, Ho, Wo, 2).contiguous()
    elif coords == "exact":      # coordinates exactly -1 and +1 in a few positions of a random grid
        grid = rand(g, M, Ho, Wo, 2) * 2.6 - 1.3
        grid[:, 0, 0, 0], grid[:, 3, 64, 0], grid[:, 2, 7, 1], grid[:, Ho - 1, Wo - 1, 1] = -1.0, 1.0, -1.0, 1.0
    else:                        # the identity grid shifted by s pixels along x and y: the hand-over runs along whole rows
        s = coords[1]
        ys, xs = torch.meshgrid(torch.arange(Ho, dtype=torch.float64), torch.arange(Wo, dtype=torch.float64), indexing="ij")
        grid = torch.stack([(xs + s) / (Wi - 1) * 2 - 1, (ys + s) / (Hi - 1) * 2 - 1], -1).float()
        grid = grid[None].expand(M, -1, -1, -1).contiguous()
    ops = _ops() if torch.cuda.is_available() else None
    names = ["out"] + ["g_" + {"i": "input", "g": "grid"}[n] for n in wrt]

    def exclude(a64):
        if "g" not in wrt:
            return {}
        m = gs_near_integer(a64[1], Hi, Wi)
        if pad == "border":      # a clamped coordinate has a zero derivative in every precision; the bound itself is the kink
            ix, iy = gs_pixel_coords(a64[1], Hi, Wi)
            beyond = torch.stack([(ix < -1e-3) | (ix > Wi - 1 + 1e-3), (iy < -1e-3) | (iy > Hi - 1 + 1e-3)], -1)
            m = m & ~beyond
        return {"g_grid": m}

    def gpu_extra(res, r64):
        if pad == "border" and "g" in wrt:
            cl = gs_clamped(case.args[1].double(), Hi, Wi)
            assert cl.any() or coords == "constant"
            assert not cl.any() or float(res["g_grid"][cl].abs().max()) == 0.0, "border mode: g_grid is exactly 0 where the coordinate was clamped"
    case = Case("grid_sample(%s)" % pad, lambda a, b: ops.grid_sample(a, b, padding_mode=pad),
                lambda a, b: orc.bilinear_sample(a, b, pad), [inp, grid], [i for i, n in enumerate("ig") if n in wrt], names,
                exclude=exclude, gpu_extra=gpu_extra, deterministic="i" not in wrt)   # g_input is accumulated with atomics
    return case


@gpu
@pytest.mark.parametrize("spec", GS_SPECS, ids=ids(GS_SPECS))
def test_grid_sample(spec):
    check_on_gpu(gs_case(spec))


@gpu
@pytest.mark.parametrize("sizes", [((11, 19), (7, 70)), ((5, 300), (9, 65))], ids=["11x19-7x70", "5x300-9x65"])
def test_grid_sample_non_finite_coordinates(sizes):
    """1e6, inf and NaN in a few positions of a regular grid, zeros mode: those outputs and their gradients are 0 (as
    F.grid_sample gives: no tap is inside the image) and the regular positions are unaffected."""
    (Hi, Wi), (Ho, Wo) = sizes
    ops = _ops()
    g = _gen(14)
    M, C = 2, 3
    inp = rand(g, M, C, Hi, Wi)
    grid = rand(g, M, Ho, Wo, 2) * 2.6 - 1.3
    bad = torch.zeros(M, Ho, Wo, dtype=torch.bool)
    spots = [(0, 0, 0), (0, 1, 63), (0, 1, 64), (1, 2, 5), (1, Ho - 1, Wo - 1), (0, 3, 17), (1, 4, 30), (0, 5, 1), (1, 0, 40)]
    vals = [(1e6, 0.1), (float("inf"), 0.2), (0.1, float("inf")), (float("nan"), 0.0), (0.3, float("nan")),
            (float("-inf"), float("-inf")), (-1e6, 1e6), (float("nan"), float("nan")), (0.0, -1e6)]
    dirty = grid.clone()
    for (m, y, x), v in zip(spots, vals):
        dirty[m, y, x] = torch.tensor(v)
        bad[m, y, x] = True
    clean = grid.clone()
    clean[bad] = 5.03   # far outside: contributes nothing, in any precision
    case = Case("grid_sample(zeros)[non-finite]", lambda a, b: ops.grid_sample(a, b, padding_mode="zeros"),
                lambda a, b: orc.bilinear_sample(a, b, "zeros"), [inp, clean], [0, 1], ["out", "g_input", "g_grid"],
                exclude=lambda a64: {"g_grid": gs_near_integer(a64[1], Hi, Wi)}, deterministic=False)
    r32, r64, masks = references(case)
    case.args = [inp, dirty]
    res, _ = run(case.prod, case, device=DEV)
    for n in case.names:
        assert torch.isfinite(res[n]).all(), "%s is not finite" % n
    assert float(res["out"].permute(0, 2, 3, 1)[bad].abs().max()) == 0.0
    assert float(res["g_grid"][bad].abs().max()) == 0.0
    compare(case, res, r32, r64, masks, "product")   # the regular positions, and g_input as a whole


# =====================================================================================================================
# Geometry                                          (pd_geometry.hip: g_P over blocks of 256, g_H over blocks of 8 x 256 pixels)
# =====================================================================================================================
GEO_SHAPES = [(3, 85), (16, 16), (1, 257), (23, 89), (32, 64), (3, 683)]   # H*W = 255, 256, 257, 2047, 2048, 2049


def intrinsics(B, H, W, dtype=torch.float64):
    K = torch.eye(4, dtype=dtype)
    K[0, 0], K[0, 2], K[1, 1], K[1, 2] = 0.58 * W, 0.5 * W, 1.92 * H, 0.5 * H
    return K[None].repeat(B, 1, 1)


def poses(g, B, scale=0.05):
    w = randn(g, B, 3).double() * scale
    Wx = torch.zeros(B, 3, 3, dtype=torch.float64)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    T = torch.eye(4, dtype=torch.float64)[None].repeat(B, 1, 1)
    T[:, :3, :3] = torch.matrix_exp(Wx)
    T[:, :3, 3] = randn(g, B, 3).double() * scale
    return T


BP_SPECS = [(1,) + GEO_SHAPES[0], (3,) + GEO_SHAPES[1], (50,) + GEO_SHAPES[2], (1,) + GEO_SHAPES[3], (3,) + GEO_SHAPES[4],
            (1,) + GEO_SHAPES[5], (50, 3, 85), (3,) + FULL]


def backproject_case(spec):
    B, H, W = spec
    g = _gen(B * 1000 + H * W)
    depth = 0.5 + 9.5 * rand(g, B, 1, H, W)
    inv_K = torch.inverse(intrinsics(B, H, W)).float()
    ops = _ops() if torch.cuda.is_available() else None
    return Case("backproject_depth", lambda d, k: ops.backproject_depth(d, k), orc.backproject_depth, [depth, inv_K], [0],
                ["cam", "g_depth"])


@gpu
@pytest.mark.parametrize("spec", BP_SPECS, ids=ids(BP_SPECS))
def test_backproject_depth(spec):
    check_on_gpu(backproject_case(spec))


# (B, H, W, wrt)   wrt: "p" (points) | "t" (T) | "pt"
P3_SPECS = [(1, 3, 85, "pt"), (3, 16, 16, "pt"), (3, 23, 89, "pt"), (1, 32, 64, "pt"), (3, 3, 683, "pt"), (50, 3, 85, "pt"),
            (50, 16, 16, "t"), (3, 3, 85, "p"), (3, 3, 85, "t"), (1, 23, 89, "p"), (1, 3, 683, "t"), (3,) + FULL + ("pt",)]


def project_case(spec):
    B, H, W, wrt = spec
    g = _gen(B * 1000 + H * W + len(wrt))
    depth = 0.5 + 9.5 * rand(g, B, 1, H, W)
    depth = torch.where(rand(g, B, 1, H, W) < 0.05, -depth, depth)   # some points behind the camera
    K = intrinsics(B, H, W)
    pts = orc.backproject_depth(depth.double(), torch.inverse(K)).float()
    T = poses(g, B).float()
    K = K.float()
    ops = _ops() if torch.cuda.is_available() else None
    names = ["grid"] + ["g_" + {"p": "points", "t": "T"}[n] for n in wrt]
    return Case("project_3d", lambda p, t: ops.project_3d(p, K.to(p.device), t, H, W),
                lambda p, t: orc.project_3d(p, K.to(p.dtype), t, H, W), [pts, T], [i for i, n in enumerate("pt") if n in wrt], names,
                deterministic=["grid"] + (["g_points"] if "p" in wrt else []))   # g_P adds its wave sums in LDS in arrival order


@gpu
@pytest.mark.parametrize("spec", P3_SPECS, ids=ids(P3_SPECS))
def test_project_3d(spec):
    check_on_gpu(project_case(spec))


# (M, H, W, crossing)
HG_SPECS = [(1, 3, 85, False), (3, 16, 16, False), (3, 1 + 1, 257, False), (1, 23, 89, False), (3, 32, 64, False),
            (1, 3, 683, False), (50, 3, 85, False), (50, 23, 89, False), (3, 23, 89, True), (50, 16, 16, True), (3,) + FULL + (False,),
            (1,) + FULL + (True,)]


def homography_setup(spec):
    M, H, W, crossing = spec
    g = _gen(M * 1000 + H * W + int(crossing))
    K = intrinsics(M, H, W)
    inv_K = torch.inverse(K)
    T = poses(g, M)
    d = (1.0 + 20.0 * rand(g, M, 1)).double()
    n = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(M, 1, 3) + 0.1 * randn(g, M, 1, 3).double()
    H_t2s, Rn = orc.homography_matrices(d, n, T, K, inv_K)
    if crossing:   # the third row makes z fall through 1e-7 inside the view (at a non-integer column or row)
        frac = 0.2 + 0.6 * rand(g, M).double()
        H_t2s = H_t2s.clone()
        H_t2s[0::2, 2, 0], H_t2s[0::2, 2, 1], H_t2s[0::2, 2, 2] = -1.0 / (frac[0::2] * (W - 1) + 0.37), 0.0, 1.0
        H_t2s[1::2, 2, 0], H_t2s[1::2, 2, 1], H_t2s[1::2, 2, 2] = 0.0, -1.0 / (frac[1::2] * (H - 1) + 0.37), 1.0
    return d, n, T, K, inv_K, H_t2s.float(), Rn.reshape(M, 3).float()


def homography_terms(H_t2s64, Rn64, inv_K64, H, W):
    """fp64 z and facing value per pixel and, for each, the largest term of its row sum: the scale of their fp32 rounding."""
    M = H_t2s64.shape[0]
    pix = orc._pixel_rays(H, W, torch.float64).expand(M, -1, -1)
    z = torch.matmul(H_t2s64[:, 2:3, :], pix)[:, 0]
    z_scale = (H_t2s64[:, 2, :, None].abs() * pix.abs()).max(1).values
    rays = torch.matmul(inv_K64[:, :3, :3], pix)
    facing = (rays * Rn64[:, :, None]).sum(1)
    f_scale = (rays.abs() * Rn64[:, :, None].abs()).max(1).values
    return z, z_scale, facing, f_scale


def homography_case(spec):
    M, H, W, crossing = spec
    d, n, T, K, inv_K, H32, Rn32 = homography_setup(spec)
    ops = _ops() if torch.cuda.is_available() else None
    invK3 = inv_K[:, :3, :3].float().contiguous()

    def f_prod(Hm):
        return ops._HomographyGrid.apply(Hm, Rn32.to(Hm.device), invK3.to(Hm.device), H, W)[0]

    def f_orc(Hm):   # the [M,3,3] algebra pinned: the per-pixel part alone
        return orc.homography_grid(d.to(Hm.dtype), n.to(Hm.dtype), T.to(Hm.dtype), K.to(Hm.dtype), inv_K.to(Hm.dtype), H, W,
                                   H_t2s=Hm, Rn=Rn32.to(Hm.dtype))[0]

    def exclude(a64):
        z, z_scale, _, _ = homography_terms(a64[0], Rn32.double(), inv_K, H, W)
        near = ((z - 1e-7).abs() <= 1e-5 * z_scale).reshape(M, H, W)
        return {"grid": near[..., None].expand(M, H, W, 2)}

    def extra(res, r64, who):
        if crossing:   # row 2 of g_H gets nothing through clamped pixels; rows 0 and 1 carry their 1 / 1e-7: one bar per row
            for r in range(3):
                rep = elementwise_report(res["g_H"][:, r], r64["g_H"][:, r])
                print("%s homography_grid g_H row %d: %s" % (who, r, rep))
                assert rep["frac_beyond"] == 0, (who, r, rep)
    return Case("homography_grid" + ("[z crossing]" if crossing else ""), f_prod, f_orc, [H32], [0], ["grid", "g_H"],
                exclude=exclude, extra=extra, deterministic=["grid"])   # g_H adds its wave sums in LDS in arrival order


@gpu
@pytest.mark.parametrize("spec", HG_SPECS, ids=ids(HG_SPECS))
def test_homography_grid(spec):
    check_on_gpu(homography_case(spec))


@gpu
@pytest.mark.parametrize("spec", [s for s in HG_SPECS if s[1:3] != FULL], ids=ids([s for s in HG_SPECS if s[1:3] != FULL]))
def test_homography_mask(spec):
    """The padding mask, exactly, on every pixel whose fp64 z and facing value are further than 1e-5 (relative to their row's
    largest term) from their thresholds."""
    M, H, W, crossing = spec
    d, n, T, K, inv_K, H32, Rn32 = homography_setup(spec)
    ops = _ops()
    _, mask = ops._HomographyGrid.apply(H32.to(DEV), Rn32.to(DEV), inv_K[:, :3, :3].float().contiguous().to(DEV), H, W)
    z, z_scale, facing, f_scale = homography_terms(H32.double(), Rn32.double(), inv_K, H, W)
    sure = ((z - 1e-7).abs() > 1e-5 * z_scale) & (facing.abs() > 1e-5 * f_scale)
    assert float((~sure).double().mean()) <= MAX_SHARE
    want = (facing > 0) & (z > 1e-7)
    got = mask.cpu().reshape(M, H * W).bool()
    assert set(mask.unique().tolist()) <= {0, 1}
    assert torch.equal(got[sure], want[sure])
    if crossing:
        assert want.any() and (~want).any()


@gpu
def test_project_then_sample_gradients_three_way():
    """Gradients through fp32 sampling coordinates (project_3d -> grid_sample): two fp32 evaluations legitimately differ in the
    bilinear derivative, so the bar is the three-way one."""
    B, H, W = 3, 23, 89
    g = _gen(23)
    ops = _ops()
    depth = 0.5 + 9.5 * rand(g, B, 1, H, W)
    K = intrinsics(B, H, W)
    inv_K, T, feat = torch.inverse(K).float(), poses(g, B).float(), rand(g, B, 3, H, W)
    K = K.float()

    def chain(bp, pr, gs):
        return lambda dd, tt, ff: gs(ff, pr(bp(dd, inv_K.to(dd)), K.to(dd), tt, H, W))
    case = Case("project_3d->grid_sample", chain(ops.backproject_depth, ops.project_3d, lambda f, q: ops.grid_sample(f, q, padding_mode="border")),
                chain(orc.backproject_depth, orc.project_3d, lambda f, q: orc.bilinear_sample(f, q, "border")),
                [depth, T, feat], [0, 1, 2], ["out", "g_depth", "g_T", "g_feat"], bar=2, deterministic=False)
    check_on_gpu(case)


# =====================================================================================================================
# masked_photometric                                          (pd_masked_loss.hip: block partials, finished by a one-wave loop)
# =====================================================================================================================
# (mode, B, H, W, mask)   mode: l1 | l1auto | mix   mask: none | float | bool
MP_SPECS = []
for _i, (_h, _w) in enumerate([(1, 1), (3, 85), (16, 16), (1, 257), (37, 150)]):
    for _j, _mode in enumerate(("l1", "l1auto", "mix")):
        MP_SPECS.append((_mode, (1, 3)[(_i + _j) % 2], _h, _w, ("none", "float", "bool")[(_i + _j) % 3]))
MP_SPECS += [("l1auto", 3) + FULL + ("float",), ("mix", 3) + FULL + ("bool",), ("l1", 3) + FULL + ("none",)]


def masked_case(spec):
    mode, B, H, W, mk = spec
    g = _gen(_seed(spec))
    rgb, tgt, src = rand(g, B, 3, H, W), rand(g, B, 3, H, W), rand(g, B, 3, H, W)
    src = tgt + 0.6 * (src - tgt)   # the automask's identity loss wins on a good share of the pixels
    ph_map = 3.0 * rand(g, B, 1, H, W)
    mask = {"none": None, "float": rand(g, B, 1, H, W), "bool": rand(g, B, 1, H, W) < 0.7}[mk]
    ops = _ops() if torch.cuda.is_available() else None
    mix, auto = mode == "mix", mode == "l1auto"

    def f_prod(r, pm):
        m = None if mask is None else mask.to(r.device)
        return ops.masked_photometric(r, tgt.to(r.device), m, source=src.to(r.device) if auto else None, ph_map=pm if mix else None)

    def f_orc(r, pm):
        m = None if mask is None else mask.to(r.dtype)
        if mix:
            pred = r if m is None else r * m + tgt.to(r.dtype) * (1.0 - m)
            return pred, (pm if m is None else pm * m).mean()
        ph, pred = orc.photometric_loss({"rgb_rec": r}, tgt.to(r.dtype), src.to(r.dtype), use_mixture_loss=False, automask=auto,
                                        mask_novel=m)
        return pred, ph.mean()

    def exclude(a64):   # an automask tie: fp32 and fp64 may pick different branches of the min
        if not auto:
            return {}
        m = 1.0 if mask is None else mask.double()
        pred = a64[0] * m + tgt.double() * (1.0 - m)
        e, a = (pred - tgt.double()).abs().mean(1, True), (src.double() - tgt.double()).abs().mean(1, True)
        return {"g_rgb_rec": ((e - a).abs() < 1e-6).expand(B, 3, H, W)}

    def extra(res, r64, who):   # the bound tests/test_gpu_parity.py uses for this sum
        rel = abs(float(res["loss"]) - float(r64["loss"])) / max(abs(float(r64["loss"])), 1e-30)
        print("%s masked_photometric loss rel err %.3e" % (who, rel))
        assert rel <= 2e-6, (who, rel)

    def gpu_extra(res, r64):
        m = 1.0 if mask is None else mask.float().to(DEV)
        want = (rgb.to(DEV) * m + tgt.to(DEV) * (1.0 - m)).cpu()
        assert torch.equal(res["pred"].view(torch.int32), want.view(torch.int32)), "pred is bit-equal to the torch expression"
    return Case("masked_photometric(%s)" % mode, f_prod, f_orc, [rgb, ph_map], [0, 1] if mix else [0],
                ["pred", "loss", "g_rgb_rec"] + (["g_ph_map"] if mix else []), bars={"pred": 1, "loss": None}, exclude=exclude,
                extra=extra, gpu_extra=gpu_extra)


@gpu
@pytest.mark.parametrize("spec", MP_SPECS, ids=ids(MP_SPECS))
def test_masked_photometric(spec):
    check_on_gpu(masked_case(spec))


# =====================================================================================================================
# smooth_loss_disp                                           (pd_smooth.hip: x in steps of 256, 4 rows per block, one atomic each)
# =====================================================================================================================
# (B, C, H, W, x0, gamma, kind)   kind: random | runs (integer-valued disparities with runs of equal neighbours)
SM_SPECS = []
for _i, (_h, _w) in enumerate([(2, 2), (2, 300), (5, 256), (5, 257), (9, 513), FULL]):
    _x0s = [0] if _w == 2 else [0, 1, int(0.2 * _w), _w - 2]
    for _j, _x0 in enumerate(_x0s):
        SM_SPECS.append(((1, 3)[(_i + _j) % 2], (3, 1)[(_i + _j // 2) % 2], _h, _w, _x0, (2.0, 0.0)[_j % 2], "random"))
SM_SPECS += [(3, 3, 5, 257, 0, 2.0, "runs"), (1, 1, 9, 513, 102, 2.0, "runs"), (1, 3, 2, 2, 0, 0.0, "runs"),
             (3, 1, 5, 256, 0, 0.0, "random"), (1, 3, 5, 256, 0, 2.0, "random")]


def smooth_case(spec):
    B, C, H, W, x0, gamma, kind = spec
    g = _gen(_seed(spec))
    disp = rand(g, B, 1, H, W) * 10
    if kind == "runs":
        disp = torch.randint(0, 3, (B, 1, H, W), generator=g).float()
    img = rand(g, B, C, H, W)
    ops = _ops() if torch.cuda.is_available() else None

    def gpu_extra(res, r64):
        if kind == "runs":   # a tie has a zero subgradient on both sides (torch's abs backward): exactly 0, not nearly
            tie = r64["g_disp"] == 0
            assert tie.any() or H * W <= 4
            assert not tie.any() or float(res["g_disp"][tie].abs().max()) == 0.0
        if x0:
            assert float(res["g_disp"][..., :x0].abs().max()) == 0.0
    case = Case("smooth_loss_disp", lambda dd, ii: ops.smooth_loss_disp(dd, ii, gamma, x0),
                lambda dd, ii: orc.smooth_loss_disp(dd[..., x0:], ii[..., x0:], gamma), [disp, img], [0], ["loss", "g_disp"],
                gpu_extra=gpu_extra, deterministic=False)   # the forward adds block sums with an atomic
    return case


@gpu
@pytest.mark.parametrize("spec", SM_SPECS, ids=ids(SM_SPECS))
def test_smooth_loss_disp(spec):
    res, _, _ = check_on_gpu(smooth_case(spec))
    again, _ = run(smooth_case(spec).prod, smooth_case(spec), device=DEV)   # the backward has no atomics
    assert torch.equal(res["g_disp"].view(torch.int32), again["g_disp"].view(torch.int32))


# =====================================================================================================================
# Conditions on the inputs: CPU only.  Every parametrised case above leaves out at most 1 % of a tensor, and the oracle's own
# fp32 run meets the per-element bar the product is held to: the inputs are fair before a kernel is looked at.
# =====================================================================================================================
ALL_CASES = ([("ssim", s, ssim_case) for s in SSIM_SPECS] + [("mix", s, mixture_case) for s in MIX_SPECS] +
             [("gs", s, gs_case) for s in GS_SPECS] + [("bp", s, backproject_case) for s in BP_SPECS] +
             [("p3", s, project_case) for s in P3_SPECS] + [("hg", s, homography_case) for s in HG_SPECS] +
             [("mp", s, masked_case) for s in MP_SPECS] + [("sm", s, smooth_case) for s in SM_SPECS])


@pytest.mark.parametrize("entry", ALL_CASES, ids=[e[0] + "-" + i for e, i in zip(ALL_CASES, ids([e[1] for e in ALL_CASES]))])
def test_conditions_cpu(entry):
    _, spec, build = entry
    check_on_cpu(build(spec))


def test_case_tables_cover_the_kernel_constants():
    """The tables keep the sizes the kernels' constants ask for (a later edit that drops one fails here, without a GPU)."""
    hw = {(s[3], s[4]) for s in SSIM_SPECS}
    assert {(2, 2), (2, 33), (8, 32), (9, 33), (7, 31), (16, 64), (17, 65), (3, 257), FULL} <= hw
    assert {s[2] for s in SSIM_SPECS if s[0] == "ssim"} >= {1, 3, 4} and {s[1] for s in SSIM_SPECS} >= {1, 3}
    assert {s[6] for s in SSIM_SPECS} >= {"x", "y", "xy"} and {s[5] for s in SSIM_SPECS} >= {"random", "flat", "close", "identical"}
    assert {s[2] for s in MIX_SPECS} >= {1, 2, 49, 64} and {s[3] * s[4] for s in MIX_SPECS} >= {1, 255, 256, 257, 297}
    assert {s[4][0] * s[4][1] for s in GS_SPECS} >= {255, 256, 257, 490} and {s[2] for s in GS_SPECS} >= {1, 3, 5}
    sizes = {255, 256, 2047, 2048, 2049, 192 * 640}   # 257 is prime: only backproject_depth takes it (the others need H, W >= 2)
    assert {s[1] * s[2] for s in BP_SPECS} >= sizes | {257}
    assert {s[1] * s[2] for s in P3_SPECS} >= sizes and {s[1] * s[2] for s in HG_SPECS} >= sizes | {2 * 257}
    for table in (BP_SPECS, P3_SPECS, HG_SPECS):
        assert {s[0] for s in table} >= {1, 3, 50}
    assert {s[2] * s[3] for s in MP_SPECS} >= {1, 255, 256, 257, 37 * 150, 192 * 640}
    assert {(s[2], s[3]) for s in SM_SPECS} >= {(2, 2), (2, 300), (5, 256), (5, 257), (9, 513), FULL}


# =====================================================================================================================
# Every element written, nothing written beyond: the C entry points on buffers with a recognisable NaN in every element and
# 256 guard floats behind the documented extent.  Reads of memory the test owns; nothing is provoked.
# =====================================================================================================================
PATTERN = 0x7FC0BEEF   # a quiet NaN no kernel produces
GUARD = 256


class Guarded:
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GUARD,), PATTERN, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def check(self, what, written=None):
        """All guard floats untouched; the first ``written`` (default: all n) elements no longer hold the pattern."""
        host = self.buf.cpu()
        assert bool((host[self.n:] == PATTERN).all()), "%s: written past its end" % what
        w = self.n if written is None else written
        left = int((host[:w] == PATTERN).sum())
        assert left == 0, "%s: %d of %d elements never written" % (what, left, w)

    def floats(self):
        return self.buf[:self.n].view(torch.float32)


def _inp(t):
    """An input with the NaN pattern behind it: a kernel that reads past the end shows up as a NaN in its output."""
    t = t.to(DEV).contiguous().float()
    g = Guarded(t.numel())
    g.floats().copy_(t.reshape(-1))
    return g


def _call(name, *a):
    from planedepth_amd import _capi as C
    lib = C.load()
    with C.on_device(torch.device(DEV)):
        C.check(getattr(lib, name)(*a, C.stream_handle(torch.device(DEV))), name)
    torch.cuda.synchronize()


RAGGED = [(3, 9, 33), (3, 1, 257), (3, 257, 2)]   # W = 33; H * W = 257; B = 3


@gpu
@pytest.mark.parametrize("B,H,W", RAGGED[:1] + RAGGED[2:])
def test_guards_ssim_reprojection(B, H, W):
    g = _gen(1)
    for Cc in (1, 3):
        n = B * Cc * H * W
        x, y, go = _inp(rand(g, n)), _inp(rand(g, n)), _inp(randn(g, n))
        out, gx, gy = Guarded(n), Guarded(n), Guarded(n)
        _call("pd_ssim_fwd", B, Cc, H, W, x.ptr, y.ptr, out.ptr)
        out.check("pd_ssim_fwd out")
        _call("pd_ssim_bwd", B, Cc, H, W, x.ptr, y.ptr, go.ptr, gx.ptr, gy.ptr)
        gx.check("pd_ssim_bwd g_x"), gy.check("pd_ssim_bwd g_y")
        gx1, gy1 = Guarded(n), Guarded(n)
        _call("pd_ssim_bwd", B, Cc, H, W, x.ptr, y.ptr, go.ptr, gx1.ptr, None)
        _call("pd_ssim_bwd", B, Cc, H, W, x.ptr, y.ptr, go.ptr, None, gy1.ptr)
        gx1.check("pd_ssim_bwd g_x alone"), gy1.check("pd_ssim_bwd g_y alone")
        assert torch.equal(gx1.buf, gx.buf) and torch.equal(gy1.buf, gy.buf)
        for t in (out, gx, gy):
            assert torch.isfinite(t.floats()).all()
    n = B * 3 * H * W
    p, t, gl = _inp(rand(g, n)), _inp(rand(g, n)), _inp(randn(g, B * H * W))
    for use_ssim in (1, 0):
        loss, gp, gt, gp1 = Guarded(B * H * W), Guarded(n), Guarded(n), Guarded(n)
        _call("pd_reproj_loss_fwd", B, H, W, use_ssim, p.ptr, t.ptr, loss.ptr)
        loss.check("pd_reproj_loss_fwd loss")
        _call("pd_reproj_loss_bwd", B, H, W, use_ssim, p.ptr, t.ptr, gl.ptr, gp.ptr, gt.ptr)
        gp.check("pd_reproj_loss_bwd g_pred"), gt.check("pd_reproj_loss_bwd g_target")
        _call("pd_reproj_loss_bwd", B, H, W, use_ssim, p.ptr, t.ptr, gl.ptr, gp1.ptr, None)
        gp1.check("pd_reproj_loss_bwd g_pred alone")
        assert torch.equal(gp1.buf, gp.buf)
        for b in (loss, gp, gt):
            assert torch.isfinite(b.floats()).all()


@gpu
@pytest.mark.parametrize("B,H,W", RAGGED[:2])
def test_guards_mixture(B, H, W):
    g = _gen(2)
    N = 5
    n = B * N * H * W
    e, s, p, go = _inp(rand(g, n) - 0.5), _inp(0.05 + rand(g, n)), _inp(rand(g, n) / N), _inp(randn(g, B * H * W))
    for lap in (1, 0):
        out, ge, gs, gp = Guarded(B * H * W), Guarded(n), Guarded(n), Guarded(n)
        _call("pd_mixture_nll_fwd", B, N, H, W, lap, e.ptr, s.ptr, p.ptr, out.ptr)
        out.check("pd_mixture_nll_fwd out")
        _call("pd_mixture_nll_bwd", B, N, H, W, lap, e.ptr, s.ptr, p.ptr, go.ptr, ge.ptr, gs.ptr, gp.ptr)
        for b, what in ((ge, "g_error"), (gs, "g_sigma"), (gp, "g_pi")):
            b.check("pd_mixture_nll_bwd " + what)
            assert torch.isfinite(b.floats()).all()
        assert torch.isfinite(out.floats()).all()


@gpu
@pytest.mark.parametrize("B,H,W", RAGGED[:2])
def test_guards_grid_sample(B, H, W):
    from planedepth_amd import _capi as C
    g = _gen(3)
    Cc, Hi, Wi = 3, 6, 11
    inp = _inp(rand(g, B * Cc * Hi * Wi))
    grid = _inp(rand(g, B * H * W * 2) * 2.6 - 1.3)
    go = _inp(randn(g, B * Cc * H * W))
    for pm in (C.PD_PAD_ZEROS, C.PD_PAD_BORDER):
        out, g_grid = Guarded(B * Cc * H * W), Guarded(B * H * W * 2)
        g_in = Guarded(B * Cc * Hi * Wi)
        g_in.floats().zero_()   # an accumulator, pre-zeroed by the caller: only its guard is checked
        _call("pd_grid_sample_fwd", B, Cc, Hi, Wi, H, W, pm, inp.ptr, grid.ptr, out.ptr)
        out.check("pd_grid_sample_fwd out")
        _call("pd_grid_sample_bwd", B, Cc, Hi, Wi, H, W, pm, inp.ptr, grid.ptr, go.ptr, g_in.ptr, g_grid.ptr)
        g_grid.check("pd_grid_sample_bwd g_grid")
        g_in.check("pd_grid_sample_bwd g_input", written=0)
        for b in (out, g_grid, g_in):
            assert torch.isfinite(b.floats()).all()


@gpu
@pytest.mark.parametrize("B,H,W", RAGGED)
def test_guards_geometry(B, H, W):
    g = _gen(4)
    HW = H * W
    inv_K = _inp(torch.inverse(intrinsics(B, max(H, 2), W)).float())
    depth = _inp(0.5 + rand(g, B * HW))
    cam, g_depth = Guarded(B * 4 * HW), Guarded(B * HW)
    _call("pd_backproject", B, H, W, depth.ptr, inv_K.ptr, cam.ptr)
    cam.check("pd_backproject cam")
    g_cam_in = _inp(randn(g, B * 4 * HW))
    _call("pd_backproject_bwd", B, H, W, inv_K.ptr, g_cam_in.ptr, g_depth.ptr)
    g_depth.check("pd_backproject_bwd g_depth")
    assert torch.isfinite(cam.floats()).all() and torch.isfinite(g_depth.floats()).all()
    if H < 2:
        return
    P = _inp(torch.matmul(intrinsics(B, H, W), poses(g, B))[:, :3, :].float())
    pts = _inp(cam.floats())
    grid, g_cam, g_P = Guarded(B * HW * 2), Guarded(B * 4 * HW), Guarded(B * 12)
    ws = Guarded(12 * B * ((HW + 255) // 256))
    g_grid = _inp(randn(g, B * HW * 2))
    _call("pd_project3d", B, H, W, ctypes.c_float(1e-7), pts.ptr, P.ptr, grid.ptr)
    grid.check("pd_project3d grid")
    _call("pd_project3d_bwd", B, H, W, ctypes.c_float(1e-7), pts.ptr, P.ptr, g_grid.ptr, g_cam.ptr, g_P.ptr, ws.ptr)
    g_cam.check("pd_project3d_bwd g_cam"), g_P.check("pd_project3d_bwd g_P"), ws.check("pd_project3d_bwd workspace")
    g_P1, ws1, g_cam1 = Guarded(B * 12), Guarded(ws.n), Guarded(B * 4 * HW)
    _call("pd_project3d_bwd", B, H, W, ctypes.c_float(1e-7), pts.ptr, P.ptr, g_grid.ptr, None, g_P1.ptr, ws1.ptr)
    _call("pd_project3d_bwd", B, H, W, ctypes.c_float(1e-7), pts.ptr, P.ptr, g_grid.ptr, g_cam1.ptr, None, None)
    g_P1.check("pd_project3d_bwd g_P alone"), g_cam1.check("pd_project3d_bwd g_cam alone")
    assert torch.equal(g_cam1.buf, g_cam.buf)
    for b in (grid, g_cam, g_P):
        assert torch.isfinite(b.floats()).all()
    # homography: M = B planes
    spec = (B, H, W, False)
    _, _, _, _, inv_K64, H32, Rn32 = homography_setup(spec)
    Hm, Rn, K3 = _inp(H32), _inp(Rn32), _inp(inv_K64[:, :3, :3].float())
    hgrid, g_H = Guarded(B * HW * 2), Guarded(B * 9)
    mask = Guarded((B * HW + 3) // 4)
    hws = Guarded(9 * B * ((HW + 255) // 256))
    _call("pd_homography_grid", B, H, W, Hm.ptr, Rn.ptr, K3.ptr, hgrid.ptr, mask.ptr)
    hgrid.check("pd_homography_grid grid")
    mb = mask.buf.cpu().view(torch.uint8)
    pat = torch.full((mask.n + GUARD,), PATTERN, dtype=torch.int32).view(torch.uint8)
    assert bool((mb[:B * HW] <= 1).all()), "pd_homography_grid mask: a byte never written"
    assert torch.equal(mb[B * HW:], pat[B * HW:]), "pd_homography_grid mask: written past its end"
    _call("pd_homography_grid_bwd", B, H, W, Hm.ptr, g_grid.ptr, g_H.ptr, hws.ptr)
    g_H.check("pd_homography_grid_bwd g_H")
    # the documented workspace (9 * M * ceil(H*W/256)) is an upper bound: the kernel fills 9 * M * ceil(H*W/2048) of it
    hws.check("pd_homography_grid_bwd workspace", written=9 * B * ((HW + 2047) // 2048))
    assert torch.isfinite(g_H.floats()).all(), "a NaN here means g_grid was read past its end"
    z = 2.0 / (W - 1) * g_grid.floats().double().cpu().reshape(B, HW, 2)[..., 0]   # g_H[:, 0, 2] = sum g.x * sx / z
    zz = homography_terms(H32.double(), Rn32.double(), inv_K64, H, W)[0]
    want = (z / zz).sum(1)
    got = g_H.floats().cpu().reshape(B, 3, 3)[:, 0, 2].double()
    assert float(((got - want).abs() / want.abs().clamp_min(1e-3)).max()) < 1e-3, (got, want)


@gpu
@pytest.mark.parametrize("B,H,W", RAGGED[:2])
def test_guards_masked_photometric(B, H, W):
    g = _gen(5)
    HW = H * W
    rgb, tgt, src = _inp(rand(g, B * 3 * HW)), _inp(rand(g, B * 3 * HW)), _inp(rand(g, B * 3 * HW))
    mask, pm = _inp(rand(g, B * HW)), _inp(rand(g, B * HW))
    g_mean, g_pred = _inp(torch.ones(1)), _inp(randn(g, B * 3 * HW))
    for mix in (0, 1):
        pred, partials, mean = Guarded(B * 3 * HW), Guarded(B * ((HW + 255) // 256)), Guarded(1)
        _call("pd_masked_photometric_fwd", B, H, W, mix, rgb.ptr, tgt.ptr, None if mix else src.ptr, mask.ptr, pm.ptr, pred.ptr,
              partials.ptr, mean.ptr)
        pred.check("pd_masked_photometric_fwd pred"), partials.check("pd_masked_photometric_fwd partials")
        mean.check("pd_masked_photometric_fwd mean")
        g_rgb, g_ph = Guarded(B * 3 * HW), Guarded(B * HW)
        _call("pd_masked_photometric_bwd", B, H, W, mix, rgb.ptr, tgt.ptr, None if mix else src.ptr, mask.ptr, g_mean.ptr,
              g_pred.ptr, g_rgb.ptr, g_ph.ptr if mix else None)
        g_rgb.check("pd_masked_photometric_bwd g_rgb_rec")
        if mix:
            g_ph.check("pd_masked_photometric_bwd g_ph_map")
        for b in (pred, partials, mean, g_rgb):
            assert torch.isfinite(b.floats()).all()


@gpu
@pytest.mark.parametrize("B,H,W", RAGGED[:1] + [(3, 2, 300)])
def test_guards_smooth_loss(B, H, W):
    g = _gen(6)
    Cn, x0 = 3, 5
    disp, img = _inp(rand(g, B * H * W)), _inp(rand(g, B * Cn * H * W))
    g_out = _inp(torch.ones(1))
    out, g_disp, g_pad = Guarded(1), Guarded(B * H * W), Guarded(B * H * W)
    L = ctypes.c_int64
    strides = (disp.ptr, L(H * W), L(W), img.ptr, L(Cn * H * W), L(H * W), L(W), ctypes.c_float(2.0))
    _call("pd_smooth_loss_fwd", B, Cn, H, W, *strides, out.ptr)
    out.check("pd_smooth_loss_fwd out")
    _call("pd_smooth_loss_bwd", B, Cn, H, W, *strides, g_out.ptr, g_disp.ptr)
    g_disp.check("pd_smooth_loss_bwd g_disp")
    # the crop [..., x0:] as a pointer offset, the gradient written into the uncropped tensor
    off = (ctypes.c_void_p(disp.buf.data_ptr() + 4 * x0), L(H * W), L(W), ctypes.c_void_p(img.buf.data_ptr() + 4 * x0),
           L(Cn * H * W), L(H * W), L(W), ctypes.c_float(2.0))
    _call("pd_smooth_loss_bwd_padded", B, Cn, H, W - x0, x0, *off, g_out.ptr, g_pad.ptr)
    g_pad.check("pd_smooth_loss_bwd_padded g_disp")
    for b in (out, g_disp, g_pad):
        assert torch.isfinite(b.floats()).all()
